// iqlhip_var_pack_body.inc — the body of iql_var_pack_window_kernel and iql_var_pack_window_group_kernel
// (iqlhip_variance_kernels.h: what it does).  In scope: VarPackParams p, bool DRAWN; VAR_PACK_ELEMENT:
// the thread's element e < (B + 1) * (S + 2) <= 1025 * 129, an int expression.
  const int S = p.S, B = p.B, W = S + 2;
  const int e = VAR_PACK_ELEMENT;
  if (e >= (B + 1) * W) return;
  long long start = p.start;
  if (DRAWN) {
    start = draw_index(p.seed, 0ull, p.j, p.span);
    if (p.starts) start = min(max(p.starts[start], 0ll), p.last_start);
    if (e == 0) *p.start_out = start;
  }
  const int t = e / W, c = e - t * W;
  const int r = 2 * S + p.A;
  if (t < B) {
    const float* row = p.rows + (start + (long long)t) * p.ld;
    if (c < S) p.out[t * S + c] = row[c];
    else if (c == S) p.out[(B + 1) * S + t] = row[r];
    else p.out[(B + 1) * S + B + t] = row[r + 1];
  } else if (c < S) {
    p.out[B * S + c] = p.rows[(start + (long long)(B - 1)) * p.ld + (S + p.A + c)];
  }
