// iqlhip_var_bwd_body.inc — the body of iql_var_bwd_kernel and iql_var_bwd_group_kernel (iqlhip_variance_kernels.h:
// what it computes).  In scope: VarBwdParams p, int blk (0 .. VAR_BWD_BLOCKS - 1).
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int n = p.n, S = p.S;
  const NetPtrs np = p.np;
  __shared__ float W2s[HID];
  W2s[tid] = np.w2[tid];
  __syncthreads();

  if (blk < 16) {
    // ---- dW1[u][k] = sum_t dH1[t][u] H0[t][k]: 16 units u of this block, wave w the columns k = 64 w .. 64 w + 63.
    // A = dH1^T (m = unit, k = row), B = H0 (k = row, n = column)
    const int u = blk * 16 + l15;
    const float w2u = W2s[u];
    f32x4 acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nts = (n + 3) >> 2;
#pragma unroll 4
    for (int ts = 0; ts < nts; ++ts) {
      const int tt = 4 * ts + g, tc = min(tt, n - 1);
      const float h1v = p.h1[(size_t)tc * HID + u];
      const float a = (tt < n && h1v > 0.f) ? p.dy[tc] * w2u : 0.f;
      float b[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) b[ct] = p.h0[(size_t)tc * HID + wave * 64 + ct * 16 + l15];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[ct] = MFMA16(a, b[ct], acc[ct]);
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        p.grad[p.g_w1 + (unsigned)((blk * 16 + 4 * g + reg) * HID + wave * 64 + ct * 16 + l15)] = acc[ct][reg];
  } else if (blk < 32) {
    // ---- dH0[t][k] for the 16 layer-0 units k = k0 .. k0 + 15 and every row: sum_u dH1[t][u] W1[u][k], masked by
    // H0[t][k] > 0.  A = W1^T (m = unit k, k = unit u: the same for every row tile, kept in registers), B = dH1^T
    // (k = unit u, n = row).  Wave w takes the 16-row tiles w, w + 4, ...
    const int k0 = (blk - 16) * 16;
    float a[64];
#pragma unroll
    for (int us = 0; us < 64; ++us) a[us] = np.w1[(unsigned)((4 * us + g) * HID + k0 + l15)];
    const int nt16 = (n + 15) >> 4;
    for (int tile = wave; tile < nt16; tile += 4) {
      const int tt = tile * 16 + l15, tc = min(tt, n - 1);
      const float dyt = (tt < n) ? p.dy[tc] : 0.f;
      const float* h1r = p.h1 + (size_t)tc * HID;
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll      // (whole: a[] is indexed by constants and stays in registers)
      for (int us = 0; us < 64; ++us) {
        const int uu = 4 * us + g;
        const float b = (h1r[uu] > 0.f) ? dyt * W2s[uu] : 0.f;
        acc = MFMA16(a[us], b, acc);
      }
      // acc[reg] = dH0[row tile * 16 + l15][k0 + 4 g + reg]
      const f32x4 h0v = *(const f32x4*)(p.h0 + (size_t)tc * HID + k0 + 4 * g);
      f32x4 d;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) d[reg] = (tt < n && h0v[reg] > 0.f) ? acc[reg] : 0.f;
      *(f32x4*)(p.dh0 + (size_t)tt * HID + k0 + 4 * g) = d;      // (tt < nt16 * 16 <= VAR_LD)
    }
    __syncthreads();      // the block's own dH0 columns, rows 0 .. 16 nt16 - 1, are visible to all its waves
    // ---- dW0[k][j] = sum_t dH0[t][k] X[t][j], and db0[k] as column j = S of ones.  A = dH0^T (m = unit, k = row),
    // B = X (k = row, n = column).  Wave w takes the column tiles w, w + 4, ...
    const int njt = (S + 1 + 15) >> 4;
    const int nts = (n + 3) >> 2;
    for (int jt = wave; jt < njt; jt += 4) {
      const int jc = jt * 16 + l15;
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int ts = 0; ts < nts; ++ts) {
        const int tt = 4 * ts + g, tc = min(tt, n - 1);
        const float av = p.dh0[(size_t)tt * HID + k0 + l15];
        const float xv = p.x[(size_t)tc * S + min(jc, S - 1)];
        const float b = (jc < S) ? xv : ((jc == S) ? 1.f : 0.f);
        acc = MFMA16(av, b, acc);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int k = k0 + 4 * g + reg;
        if (jc < S) p.grad[p.g_w0 + (unsigned)(k * S + jc)] = acc[reg];
        else if (jc == S) p.grad[p.g_b0 + (unsigned)k] = acc[reg];
      }
    }
  } else {
    // ---- thread u: dW2[u] = sum_t dy[t] H1[t][u], db1[u] = W2[u] sum_{t: H1[t][u] > 0} dy[t]; db2 = sum_t dy[t]
    float sw = 0.f, sb = 0.f, s2 = 0.f;
    for (int t = 0; t < n; ++t) {
      const float d = p.dy[t], h = p.h1[(size_t)t * HID + tid];
      sw = fmaf(d, h, sw);
      sb += (h > 0.f) ? d : 0.f;
      s2 += d;
    }
    p.grad[p.g_w2 + tid] = sw;
    p.grad[p.g_b1 + tid] = sb * W2s[tid];
    if (tid == 0) p.grad[p.g_b2] = s2;
  }
