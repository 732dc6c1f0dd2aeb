// iqlhip_var_row_body.inc — the body of iql_var_row_kernel and iql_var_row_group_kernel (iqlhip_variance_kernels.h:
// what it computes).  In scope: VarRowParams p.
#pragma clang fp contract(off)
  __shared__ float samp[VAR_MAX_ROWS], nnt[VAR_MAX_ROWS], rw[VAR_MAX_ROWS], gdir[VAR_MAX_ROWS];
  __shared__ float red[4];
  const int tid = threadIdx.x, B = p.B;
  for (int t = tid; t < B; t += 256) {
    nnt[t] = 1.f - p.nd[t];
    rw[t] = p.rew[p.aligned ? t : (t == 0 ? B - 1 : t - 1)];
  }
  __syncthreads();
  if (tid == 0) {
    float next = p.out[B];
    for (int t = B - 1; t >= 0; --t) {
      const float gn = VAR_GAMMA * next;
      const float s = rw[t] + gn * nnt[t];
      samp[t] = s;
      next = s;
    }
  }
  __syncthreads();
  const float inv_b = 1.f / (float)B;
  float lsum = 0.f;
  for (int t = tid; t < B; t += 256) {
    const float pred = p.out[t], s = p.out[VAR_LD + t];
    const float e = expf(s);
    const bool open = (e >= VAR_CLIP_LO) && (e <= VAR_CLIP_HI);
    const float var = fminf(fmaxf(e, VAR_CLIP_LO), VAR_CLIP_HI);
    const float d = pred - samp[t];
    const float q = (d * d) / var;
    lsum = lsum + 0.5f * (logf(var) + q);
    const float gp = (d / var) * inv_b;
    gdir[t] = -gp;
    p.vals[t] = samp[t];
    p.vals[VAR_LD + t] = pred;
    p.vals[2 * VAR_LD + t] = var;
    if (p.vals2) {
      p.vals2[t] = samp[t];
      p.vals2[B + t] = pred;
      p.vals2[2 * B + t] = var;
    }
    if (p.which == 0) p.dy[t] = gp;
    else if (p.which == 1) p.dy[t] = open ? (0.5f * (1.f - q)) * inv_b : 0.f;
  }
  const float total = block_sum_256(lsum, red);      // (its barriers publish gdir)
  if (tid == 0) {
    p.loss[0] = total / (float)B;
    if (p.which == 0) {
      float G = gdir[0];
      for (int t = 1; t < B; ++t) G = gdir[t] + (VAR_GAMMA * nnt[t - 1]) * G;
      p.dy[B] = (VAR_GAMMA * nnt[B - 1]) * G;
    }
  }
