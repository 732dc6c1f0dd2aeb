// iqlhip_score_kernels.h — scoring transitions without a step (iqlhip_score_rows).
// Included by iqlhip.hip behind iqlhip_kernels.h (HID, RT_ROWS, H0_LD, T64_LD, W2_LD, NSPLIT, HEAD_LD, MFMA16, NetPtrs,
// PIN_S / PIN_P, sum4).
//
//   iql_score_fwd_kernel     fp32 forward of the seven instances over the row tiles of a chunk: head partials only
//   iql_score_rows_kernel    per row: the eight score columns; per 32-row tile: partial sums of 3 loss numerators + 8 columns
//   iql_score_finish_kernel  one block: tile partials added in tile order, in double; the 11 summary floats
//   iql_score_check_idx_kernel  the index list against [0, n_rows), in front of everything else
//
// Nothing here shares mutable memory with the step: the kernels read the parameter and target arenas and the caller's
// rows, and write a scratch of their own (and the caller's output).
#pragma once

#define SCORE_XR_MAX 16          // input columns per thread of a tile: 8 threads per row, k_in <= IQLHIP_MAX_INPUT = 128
#define SCORE_XLD_MAX 132         // LDS row stride of the input tile at the widest input (129, kept 16-byte aligned)
#define SCORE_N_PART 12          // floats per tile partial: 3 loss numerators, 8 column sums, 1 pad

struct ScoreParams {
  NetPtrs inst[7];               // V(s'), V(s), Qt1, Qt2, Q1, Q2, pi — always the fp32 masters
  int xoff[7];                   // first column of the instance's input inside a row (0 or S + A)
  const float* rows;             // the replay row store [s | a | s' | r | d | pad]
  long long ld;                  // its row stride in floats (a multiple of 4)
  const long long* idx;          // the chunk's part of the index list, or null: rows row0 .. row0 + n - 1
  long long row0;
  int n;                         // rows of this chunk
  int n_tiles;                   // (n + 31) / 32
  int A;
  float* heads;                  // [chunk][HEAD_LD] scalar partials: inst 0..5 x column slice 0..3 (bias inside slice 0)
  float* pi;                     // [chunk][A][NSPLIT] policy head partials
};

// Layer 0 of one wave: H0[32 rows][64 * wave .. + 64) into acc, operands W0 [256][k0] (LDS or global: the caller's
// pointer decides, one inlined copy each) and the tile's rows in LDS.  Eight k-steps are read in one batch, then their
// MFMAs run back to back (iqlhip_fwd_body.inc: why).  A last k-step that reaches beyond k0: zeros on the X side, the
// weight side is read with a clamped column (finite x 0 = 0).
__device__ __forceinline__ void score_l0(f32x4 (&acc)[2][4], const float* wbase, const float* x0, const float* x1, int k0,
                                         int nks, int wave, int l15, int g) {
  const float* wl[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) wl[ct] = wbase + (wave * 64 + ct * 16 + l15) * k0;
  for (int base = 0; base < nks; base += 8) {
    float bq[8][4], aq[8][2];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int kk = 4 * (base + ks) + g;
      const int kc = min(kk, k0 - 1);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) bq[ks][ct] = wl[ct][kc];
      const float xa = x0[kc], xb_ = x1[kc];
      aq[ks][0] = (kk < k0) ? xa : 0.f;
      aq[ks][1] = (kk < k0) ? xb_ : 0.f;
    }
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) asm volatile("" : "+v"(aq[ks][0]), "+v"(aq[ks][1]));
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      if (base + ks < nks) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          acc[0][ct] = MFMA16(bq[ks][ct], aq[ks][0], acc[0][ct]);
          acc[1][ct] = MFMA16(bq[ks][ct], aq[ks][1], acc[1][ct]);
        }
      }
    }
  }
}

// blockIdx = group * 28 + instance * 4 + column slice: the block stages its weights ONCE (W0 in LDS when k_in <=
// W0_LDS_MAX_K, streamed from the cache hierarchy above that; its W1 slice as MFMA fragments in registers; its head
// slice in LDS) and then walks the row tiles group, group + n_groups, ... of the chunk.  A tile is always computed the
// same way, whatever its place in the call, so a row's partials depend on the row alone.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void iql_score_fwd_kernel(ScoreParams p) {
  const int unit = blockIdx.x % 28, grp = blockIdx.x / 28, ngrp = gridDim.x / 28;
  const int inst = unit >> 2, ns = unit & 3;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;

  const NetPtrs np = p.inst[inst];
  const int xoff = p.xoff[inst];
  const int k0 = np.k0;
  const int nks = (k0 + 3) >> 2;
  const int D = np.d;
  const int ld = (int)p.ld;
  const int n = p.n;
  const int n_tiles = p.n_tiles;
  const int Aact = p.A;
  const float* rows = p.rows;
  const long long* idx = p.idx;
  const long long row0 = p.row0;
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
}

// ---------------------------------------------------------------------------
struct ScoreRowsParams {
  const float* rows;
  long long ld;
  const long long* idx;
  long long row0;
  int n, n_tiles;
  int S, A, policy;
  iqlhip_hyper hy;
  const float* log_std;          // Gaussian policy: A floats of the parameter arena; else null
  const float* heads;
  const float* pi;
  float* out;                    // [n][IQLHIP_N_SCORE] of this chunk, or null
  float* part;                   // [n_tiles][SCORE_N_PART]
};

// One wave per 32-row tile: lane l works on row l & 31; the two lane halves split the action dims of the row's
// behaviour-cloning term (even dims / odd dims) and add their two sums once.  The tile partials are butterfly sums over
// the wave: a fixed lane order.
__global__ __launch_bounds__(256) void iql_score_rows_kernel(ScoreRowsParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x * 4 + wave;
  if (tile >= p.n_tiles) return;
  const int r = lane & 31, h = lane >> 5;
  const int pos = tile * RT_ROWS + r;
  const bool live = pos < p.n;
  const int pc = min(pos, p.n - 1);
  const long long srow = p.idx ? p.idx[pc] : p.row0 + pc;
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
  if (mine && p.out) {
    float* o = p.out + (size_t)pos * IQLHIP_N_SCORE;
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
}

// One block.  Thread (j = tid >> 4, s = tid & 15) adds partial j of the s-th sixteenth of the chunk's tiles in tile
// order, in double; the sixteen sums are then added in order s = 0 .. 15 onto the call's running sums acc[j] (`first`:
// the call's first chunk starts them at zero).  `summary` (host-mapped; the call's last chunk): the three losses as
// means over n_total — q_loss with the reference's / 2 — then the eight column means.
__global__ __launch_bounds__(256) void iql_score_finish_kernel(const float* part, int n_tiles, double* acc, int first,
                                                               long long n_total, float* summary) {
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
}

// status[0] = 1 and status[1] = an offending index when some idx[i] lies outside [0, n_rows) (status is host-mapped
// and zeroed by the host before the launch; which offender is reported is not defined).
__global__ __launch_bounds__(256) void iql_score_check_idx_kernel(const long long* idx, long long n, long long n_rows,
                                                                  unsigned long long* status) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long v = idx[i];
    if (v < 0 || v >= n_rows) {
      status[1] = (unsigned long long)v;
      status[0] = 1ull;
    }
  }
}
