// iqlhip_var_fwd_body.inc — the body of iql_var_fwd_kernel and iql_var_fwd_group_kernel (iqlhip_variance_kernels.h:
// what it computes).  In scope: VarFwdParams p, int tile (32-row tile), int net.
  const int n = net ? p.rows1 : p.rows0;
  if (tile * 32 >= n) return;                 // (block-uniform: before any barrier)
  const NetPtrs np = net ? p.net[1] : p.net[0];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int S = p.S;
  const bool keep = p.keep == net;
  __shared__ __attribute__((aligned(16))) float H0s[32 * H0_LD];
  __shared__ float part[16 * 32];

  const int row0 = tile * 32 + l15, row1 = row0 + 16;
  f32x4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  score_l0(acc, np.w0, p.x + (size_t)min(row0, n - 1) * S, p.x + (size_t)min(row1, n - 1) * S, S, (S + 3) >> 2, wave, l15, g);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int unit = wave * 64 + ct * 16 + 4 * g;
    const f32x4 bias0 = *(const f32x4*)(np.b0 + unit);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      f32x4 h;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) h[reg] = fmaxf(acc[rt][ct][reg] + bias0[reg], 0.f);
      *(f32x4*)(H0s + (rt * 16 + l15) * H0_LD + unit) = h;
      const int row = rt ? row1 : row0;
      if (keep && row < n) *(f32x4*)(p.h0 + (size_t)row * HID + unit) = h;
    }
  }
  __syncthreads();

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  score_l0(acc, np.w1, H0s + l15 * H0_LD, H0s + (16 + l15) * H0_LD, HID, HID / 4, wave, l15, g);
  float hp[2] = {0.f, 0.f};
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int unit = wave * 64 + ct * 16 + 4 * g;
    const f32x4 bias1 = *(const f32x4*)(np.b1 + unit);
    const f32x4 w2 = *(const f32x4*)(np.w2 + unit);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      f32x4 h;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        h[reg] = fmaxf(acc[rt][ct][reg] + bias1[reg], 0.f);
        hp[rt] = fmaf(h[reg], w2[reg], hp[rt]);
      }
      const int row = rt ? row1 : row0;
      if (keep && row < n) *(f32x4*)(p.h1 + (size_t)row * HID + unit) = h;
    }
  }
  part[(wave * 4 + g) * 32 + l15] = hp[0];
  part[(wave * 4 + g) * 32 + 16 + l15] = hp[1];
  __syncthreads();
  if (tid < 32) {
    const int row = tile * 32 + tid;
    if (row < n) {
      float s = part[tid];
#pragma unroll
      for (int i = 1; i < 16; ++i) s += part[i * 32 + tid];
      p.out[net * VAR_LD + row] = s + np.b2[0];
    }
  }
