// iqlhip_score_fwd_body.inc — the body of iql_score_fwd_kernel and iql_score_fwd_group_kernel (iqlhip_score_kernels.h).
// The including kernel provides: `p` (a ScoreParams: the kernel argument, or the member's record), constexpr bool GROUP,
// and chunk_done / chunk_n / chunk_ngrp — a group launch's chunk (rows chunk_done .. chunk_done + chunk_n of the call p
// describes) and its tile streams per member (gridDim.x / 28, passed as an argument: see the group kernels); a solo
// launch's p describes its chunk itself (GROUP = false: the three are unused constants).
  const int unit = blockIdx.x % 28, grp = blockIdx.x / 28, ngrp = GROUP ? chunk_ngrp : gridDim.x / 28;
  const int inst = unit >> 2, ns = unit & 3;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;

  const NetPtrs np = p.inst[inst];
  const int xoff = p.xoff[inst];
  const int k0 = np.k0;
  const int nks = (k0 + 3) >> 2;
  const int D = np.d;
  const int ld = (int)p.ld;
  const int n = GROUP ? chunk_n : p.n;
  const int n_tiles = GROUP ? (chunk_n + RT_ROWS - 1) / RT_ROWS : p.n_tiles;
  const int Aact = p.A;
  const float* rows = p.rows;
  const long long* idx = (GROUP && p.idx) ? p.idx + chunk_done : p.idx;
  const long long row0 = GROUP ? p.row0 + chunk_done : p.row0;
  float* headsg = p.heads;
  float* pig = p.pi;
  PIN_P(np.w0); PIN_P(np.b0); PIN_P(np.w1); PIN_P(np.b1); PIN_P(np.w2); PIN_P(np.b2);
  PIN_S(k0); PIN_S(D); PIN_S(xoff); PIN_S(ld); PIN_S(n); PIN_S(Aact);
  PIN_P(rows); PIN_P(idx); PIN_P(headsg); PIN_P(pig);
  const bool w0_lds = k0 <= W0_LDS_MAX_K;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* H0s = smem;                         // [32][H0_LD]
  float* H1s = H0s + RT_ROWS * H0_LD;        // [32][T64_LD]
  float* Xr = H1s + RT_ROWS * T64_LD;        // [32][xld] the instance's input columns of the tile's rows
  const int xld = ((k0 + 3) & ~3) + 1;       // (odd: the 32 rows of an operand read spread over the banks)
  float* W2s = Xr + RT_ROWS * SCORE_XLD_MAX; // [Dp][W2_LD] head weights of this slice (rows beyond D zero), then b2[D]
  const int Dp = (D + 15) & ~15;
  const int w2s_words = ((Aact + 15) & ~15) * W2_LD + 32;
  float* B0s = W2s + w2s_words;              // [256] layer-0 bias
  float* W0s = B0s + HID;                    // [256 * k0] (when w0_lds)

  // ---- a tile's rows: only the instance's k0 input columns are staged.  Thread -> (row tid >> 3 of the tile, columns
  // (tid & 7) + 8 j): ONE source row per thread, looked up one tile ahead of the loads that use it (an index list costs
  // a dependent load).  Rows past the chunk's end repeat its last row; their results are never stored.
  const int xrl = tid >> 3, xsub = tid & 7;
  float xr[SCORE_XR_MAX];
#define SCORE_LOOKUP(tile_) (idx ? idx[min((tile_) * RT_ROWS + xrl, n - 1)] : row0 + min((tile_) * RT_ROWS + xrl, n - 1))
#define SCORE_ISSUE(J0, J1)                                                                      \
  _Pragma("unroll") for (int j = J0; j < J1; ++j) xr[j] = xsrc[min(xsub + 8 * j, k0 - 1)];
  // (tiers of 4 / 8 / 16 straight-line loads, as xr_load: a load under a run-time trip count is waited for individually)
#define SCORE_ISSUE_ALL()                                                                        \
  do {                                                                                           \
    const float* xsrc = rows + (src * (long long)ld + xoff);                                     \
    SCORE_ISSUE(0, 4)                                                                            \
    if (k0 > 32) {                                                                               \
      SCORE_ISSUE(4, 8)                                                                          \
      if (k0 > 64) { SCORE_ISSUE(8, 16) }                                                        \
    }                                                                                            \
  } while (0)
#pragma unroll
  for (int j = 0; j < SCORE_XR_MAX; ++j) xr[j] = 0.f;

  int tile = grp;
  if (tile >= n_tiles) return;               // (block-uniform: before any barrier)
  long long src = SCORE_LOOKUP(tile);
  SCORE_ISSUE_ALL();
  src = SCORE_LOOKUP(min(tile + ngrp, n_tiles - 1));

  // ---- the block's weights, once
  B0s[tid] = np.b0[tid];                      // (layer 0's bias in LDS: 16 registers less across the tile loop)
  const f32x4 bias1 = *(const f32x4*)(np.b1 + (unsigned)(ns * 64 + wave * 16 + 4 * g));
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int e = tid + 256 * q;
    if (e < Dp * 16) {
      f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (e < D * 16) v = *(const f32x4*)(np.w2 + (unsigned)((e >> 4) * HID + ns * 64 + 4 * (e & 15)));
      *(f32x4*)(W2s + (e >> 4) * W2_LD + 4 * (e & 15)) = v;
    }
  }
  if (tid < D) W2s[Dp * W2_LD + tid] = np.b2[tid];
  if (w0_lds) {
    const int n_w0v = 64 * k0;               // float4 of W0 [256][k0]
    for (int f = tid; f < n_w0v; f += 256) *(f32x4*)(W0s + 4 * f) = *(const f32x4*)(np.w0 + 4u * (unsigned)f);
  }
  // this wave's W1 rows (16 output units x 256 k) as MFMA fragments: k = 16 ks + 4 g + t
  const int n1 = ns * 64 + wave * 16 + l15;
  f32x4 bw[16];
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) bw[ks] = *(const f32x4*)(np.w1 + (unsigned)(n1 * HID + 16 * ks + 4 * g));

  for (;;) {
    // the tile's rows: registers -> LDS; then the NEXT tile's rows are requested and stay in flight under this tile's
    // MFMAs (their source rows were looked up a tile ago), and the tile after that is looked up
#pragma unroll
    for (int j = 0; j < SCORE_XR_MAX; ++j) {
      const int col = xsub + 8 * j;
      if (col < k0) Xr[xrl * xld + col] = xr[j];
    }
    __syncthreads();     // Xr (and, first tile, the weights) visible; every thread is done with the last tile's H1s
    const int tile_next = tile + ngrp;
    if (tile_next < n_tiles) {
      SCORE_ISSUE_ALL();
      src = SCORE_LOOKUP(min(tile_next + ngrp, n_tiles - 1));
    }

    // ---- layer 0: A = W0 (m = hidden unit), B = X (n = row): a lane's 4 accumulators are 4 consecutive units of one row
    {
      f32x4 acc[2][4];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const float* x0 = Xr + l15 * xld;
      const float* x1 = Xr + (16 + l15) * xld;
      if (w0_lds) score_l0(acc, W0s, x0, x1, k0, nks, wave, l15, g);
      else score_l0(acc, np.w0, x0, x1, k0, nks, wave, l15, g);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const f32x4 bias0 = *(const f32x4*)(B0s + wave * 64 + ct * 16 + 4 * g);
#pragma unroll
        for (int rtile = 0; rtile < 2; ++rtile) {
          f32x4 h;
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) h[reg] = fmaxf(acc[rtile][ct][reg] + bias0[reg], 0.f);
          *(f32x4*)(H0s + (rtile * 16 + l15) * H0_LD + wave * 64 + ct * 16 + 4 * g) = h;
        }
      }
    }
    __syncthreads();

    // ---- layer 1: this wave computes H1[32][16 units]; A = W1 fragments (m = unit), B = H0 (n = row)
    {
      f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        const f32x4 a0 = *(const f32x4*)(H0s + l15 * H0_LD + 16 * ks + 4 * g);
        const f32x4 a1 = *(const f32x4*)(H0s + (16 + l15) * H0_LD + 16 * ks + 4 * g);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          acc0 = MFMA16(bw[ks][t], a0[t], acc0);
          acc1 = MFMA16(bw[ks][t], a1[t], acc1);
        }
      }
      f32x4 h0, h1;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        h0[reg] = fmaxf(acc0[reg] + bias1[reg], 0.f);
        h1[reg] = fmaxf(acc1[reg] + bias1[reg], 0.f);
      }
      *(f32x4*)(H1s + l15 * T64_LD + wave * 16 + 4 * g) = h0;
      *(f32x4*)(H1s + (16 + l15) * T64_LD + wave * 16 + 4 * g) = h1;
    }
    __syncthreads();

    // ---- head partial sums over this block's 64 hidden-1 units (slice 0 also adds the bias)
    {
      const int rl = tid >> 3, sub = tid & 7;
      const int pos = tile * RT_ROWS + rl;
      if (D == 1) {
        const f32x4 ha = *(const f32x4*)(H1s + rl * T64_LD + 4 * sub);
        const f32x4 hb = *(const f32x4*)(H1s + rl * T64_LD + 32 + 4 * sub);
        const f32x4 wa = *(const f32x4*)(W2s + 4 * sub);
        const f32x4 wb = *(const f32x4*)(W2s + 32 + 4 * sub);
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf(ha[e], wa[e], acc);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf(hb[e], wb[e], acc);
        acc += __shfl_xor(acc, 1);
        acc += __shfl_xor(acc, 2);
        acc += __shfl_xor(acc, 4);
        if (ns == 0) acc += W2s[Dp * W2_LD];
        if (sub == 0 && pos < n) {
          if (inst < 6) headsg[(size_t)pos * HEAD_LD + inst * NSPLIT + ns] = acc;
          else pig[(size_t)pos * NSPLIT + ns] = acc;           // a policy with one action dim
        }
      } else if (16 * (wave >> 1) < Dp) {
        // policy head on the matrix cores: partial[32 rows][Dp] = H1s[32][64] x W2s^T — wave w takes row tile w & 1 and
        // the 16 action dims of tile w >> 1.  A = H1 (m = row, k = unit), B = W2 (k = unit, n = dim, zero rows beyond D)
        const int i = wave & 1, nt = wave >> 1;
        float a[16], b[16];
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          a[ks] = H1s[(16 * i + l15) * T64_LD + 4 * ks + g];
          b[ks] = W2s[(16 * nt + l15) * W2_LD + 4 * ks + g];
        }
        f32x4 hacc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) hacc = MFMA16(a[ks], b[ks], hacc);
        const int dd = 16 * nt + l15;
        const float bias = (ns == 0) ? W2s[Dp * W2_LD + min(dd, D - 1)] : 0.f;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int prow = tile * RT_ROWS + 16 * i + 4 * g + reg;
          if (dd < D && prow < n) pig[((size_t)prow * Aact + dd) * NSPLIT + ns] = hacc[reg] + bias;
        }
      }
    }
    if (tile_next >= n_tiles) break;
    tile = tile_next;
  }
#undef SCORE_LOOKUP
#undef SCORE_ISSUE
#undef SCORE_ISSUE_ALL
