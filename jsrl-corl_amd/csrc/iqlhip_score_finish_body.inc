// iqlhip_score_finish_body.inc — the body of iql_score_finish_kernel and iql_score_finish_group_kernel: the including
// kernel provides part, n_tiles, acc, first, n_total and summary (its arguments, or the member's).
  const int j = threadIdx.x >> 4, s = threadIdx.x & 15;
  const int seg = (n_tiles + 15) >> 4;
  const int t0 = s * seg, t1 = min(t0 + seg, n_tiles);
  double v = 0.0;
  if (j < 11)
    for (int t = t0; t < t1; ++t) v += (double)part[(size_t)t * SCORE_N_PART + j];
  double tot = (first || j >= 11) ? 0.0 : acc[j];
  const int base = (threadIdx.x & 63) & ~15;
#pragma unroll
  for (int s2 = 0; s2 < 16; ++s2) tot += __shfl(v, base + s2);
  if (s == 0 && j < 11) {
    acc[j] = tot;
    if (summary) summary[j] = (float)(tot / (double)n_total * (j == 1 ? 0.5 : 1.0));
  }
