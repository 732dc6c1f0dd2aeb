// iqlhip_score_rows_body.inc — the body of iql_score_rows_kernel and iql_score_rows_group_kernel (iqlhip_score_kernels.h).
// The including kernel provides: `p` (a ScoreRowsParams: the kernel argument, or the member's record), constexpr bool
// GROUP, chunk_done / chunk_n as iqlhip_score_fwd_body.inc, and chunk_out: where a group launch stores the chunk's rows.
  const int n = GROUP ? chunk_n : p.n;
  const int n_tiles = GROUP ? (chunk_n + RT_ROWS - 1) / RT_ROWS : p.n_tiles;
  const long long* idx = (GROUP && p.idx) ? p.idx + chunk_done : p.idx;
  const long long row0 = GROUP ? p.row0 + chunk_done : p.row0;
  float* const out = GROUP ? chunk_out : p.out;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x * 4 + wave;
  if (tile >= n_tiles) return;
  const int r = lane & 31, h = lane >> 5;
  const int pos = tile * RT_ROWS + r;
  const bool live = pos < n;
  const int pc = min(pos, n - 1);
  const long long srow = idx ? idx[pc] : row0 + pc;
  const float* row = p.rows + srow * p.ld;
  const int S = p.S, A = p.A;
  f32x4 hd[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) hd[i] = *(const f32x4*)(p.heads + ((size_t)pc * HEAD_LD + 4 * i));
  const float rew = row[2 * S + A], done = row[2 * S + A + 1];
  const bool gauss = p.policy == IQLHIP_POLICY_GAUSSIAN;

  float bc_half = 0.f;
  for (int d = h; d < A; d += 2) {
    const float mu = tanhf(sum4(*(const f32x4*)(p.pi + ((size_t)pc * A + d) * NSPLIT)));
    const float diff = row[S + d] - mu;
    if (gauss) {
      const float ls = fminf(fmaxf(p.log_std[d], p.hy.log_std_min), p.hy.log_std_max);
      const float sig = expf(ls);
      // -Normal.log_prob = (a - mu)^2 / (2 var) + log(sigma) + log(sqrt(2 pi))
      bc_half += diff * diff / (2.f * (sig * sig)) + ls + 0.9189385332046727f;
    } else {
      bc_half += diff * diff;
    }
  }
  const float bc_other = __shfl_xor(bc_half, 32);
  const float bc = (h == 0) ? bc_half + bc_other : bc_other + bc_half;      // even dims + odd dims, on both halves

  const float nv = sum4(hd[0]), v = sum4(hd[1]);
  const float tq = fminf(sum4(hd[2]), sum4(hd[3]));
  const float q1 = sum4(hd[4]), q2 = sum4(hd[5]);
  const float adv = tq - v;
  const float ew = fminf(expf(p.hy.beta * adv), p.hy.exp_adv_max);
  const float wgt = fabsf(p.hy.iql_tau - ((adv < 0.f) ? 1.f : 0.f));
  const float y = rew + ((1.f - done) * p.hy.discount) * nv;
  const float e1 = q1 - y, e2 = q2 - y;

  const bool mine = live && h == 0;
  if (mine && out) {
    float* o = out + (size_t)pos * IQLHIP_N_SCORE;
    *(f32x4*)o = (f32x4){v, nv, q1, q2};
    *(f32x4*)(o + 4) = (f32x4){tq, adv, ew, bc};
  }
  float s[11] = {wgt * adv * adv, e1 * e1 + e2 * e2, ew * bc, v, nv, q1, q2, tq, adv, ew, bc};
#pragma unroll
  for (int j = 0; j < 11; ++j) {
    float t = mine ? s[j] : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    s[j] = t;
  }
  if (lane == 0) {
    float* pt = p.part + (size_t)tile * SCORE_N_PART;
    *(f32x4*)pt = (f32x4){s[0], s[1], s[2], s[3]};
    *(f32x4*)(pt + 4) = (f32x4){s[4], s[5], s[6], s[7]};
    *(f32x4*)(pt + 8) = (f32x4){s[8], s[9], s[10], 0.f};
  }
