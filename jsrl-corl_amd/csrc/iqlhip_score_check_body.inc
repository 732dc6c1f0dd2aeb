// iqlhip_score_check_body.inc — the body of iql_score_check_idx_kernel and iql_score_check_idx_group_kernel: the
// including kernel provides idx, n, n_rows and status (its arguments, or the member's) and check_first / check_stride:
// the thread's place along x and the threads of the grid along x.
  for (long long i = check_first; i < n; i += check_stride) {
    const long long v = idx[i];
    if (v < 0 || v >= n_rows) {
      status[1] = (unsigned long long)v;
      status[0] = 1ull;
    }
  }
