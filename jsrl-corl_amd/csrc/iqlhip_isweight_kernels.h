// iqlhip_isweight_kernels.h — importance-sampling weights of a weighted draw (include/iqlhip.h
// "iqlhip_draw_indices_weighted_is").  Included by iqlhip.hip behind every other kernel of the library (the
// existing kernels keep their places in the code object); needs iqlhip_weighted_kernels.h (draw_index_weighted, WTab).
//
// A row drawn by weight has probability q_r / total, q_r its quantised weight (a table integer).  With per-batch max
// normalisation the total and the row count cancel:  c_r = (q_min / q_r)^beta,  q_min the smallest q among the batch's
// rows, so c_r in (0, 1] and the rarest row of every batch has c = 1 exactly.  Zero-weight rows are never drawn: q_r > 0.
#pragma once

// THE formula, for every caller: q and q_min as fp32 (the conversion of a table integer < 2^40 rounds once, monotonically:
// the smallest integer gives the smallest float, and equal integers equal floats), the power through the hardware's
// log2 / exp2 (about 1 ulp each).  q == q_min gives log2(1) = 0 and exp2(0) = 1 exactly; beta == 0 gives 1 for every row.
__device__ __forceinline__ float is_weight(float q, float q_min, float beta) {
  return __builtin_amdgcn_exp2f(beta * __builtin_amdgcn_logf(q_min / q));
}

// Leaf value of row i (iql_wt_leaves_kernel's expression): the row's quantised weight.
__device__ __forceinline__ unsigned long long wt_leaf(const WTab& wt, unsigned i) {
  return wt.tab[i] - (((wt.local ? (i & 63u) : i) != 0u) ? wt.tab[i - 1u] : 0ull);
}

// iql_draw_indices_weighted_kernel (the same descents, hence the same indices) that also stages each drawn row's q as
// fp32 at qf[j].
__global__ __launch_bounds__(256) void iql_draw_indices_weighted_q_kernel(long long* idx, float* qf, long long n_idx, WTab wt,
                                                                          unsigned long long seed, unsigned long long offset) {
  const long long wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  const long long n_waves = (long long)gridDim.x * 4;
  for (long long j0 = wave; j0 < n_idx; j0 += 2 * n_waves) {
    const long long j1 = j0 + n_waves;
    const unsigned long long j[2] = {(unsigned long long)j0, (unsigned long long)(j1 < n_idx ? j1 : j0)};
    long long i[2];
    draw_index_weighted<2>(wt, seed, offset, j, i);
    if ((threadIdx.x & 63) == 0) {
      idx[j0] = i[0];
      qf[j0] = (float)wt_leaf(wt, (unsigned)i[0]);      // (the descent is clamped to the table: i < wt.n)
      if (j1 < n_idx) {
        idx[j1] = i[1];
        qf[j1] = (float)wt_leaf(wt, (unsigned)i[1]);
      }
    }
  }
}

// c[j] <- is_weight(c[j], min of the staged q over j's group, beta), in place; block b owns group b = indices
// [b * group, min((b + 1) * group, n)) — the last group may be short and is normalised over the rows it has.
__global__ __launch_bounds__(256) void iql_is_weights_kernel(float* c, long long n, long long group, float beta) {
  __shared__ float red[4];
  const long long lo = (long long)blockIdx.x * group, hi = min(lo + group, n);
  float m = __builtin_inff();
  for (long long j = lo + threadIdx.x; j < hi; j += 256) m = fminf(m, c[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  const float q_min = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  for (long long j = lo + threadIdx.x; j < hi; j += 256) c[j] = is_weight(c[j], q_min, beta);
}

// ---- weighted chunk graphs with importance-sampling weights (iqlhip_train_steps_weighted_is) ------------------------------
// gather_rows_drawn_weighted that also stages each drawn row's q as fp32 at qf[r] (the wave that resolved the index holds
// it; lane 0 reads the leaf and stores).
__device__ __forceinline__ void gather_rows_drawn_weighted_q(const float* rows, long long ld, float* xb, float* qf, int n,
                                                             const WTab& wt, unsigned long long seed, unsigned long long ctr0,
                                                             unsigned long long j0, int wave, int n_waves) {
  const int q = (int)(ld >> 2);
  const int lane = (int)(threadIdx.x & 63);
  for (int r0 = wave; r0 < n; r0 += 2 * n_waves) {
    const int r1 = r0 + n_waves;
    const bool two = r1 < n;
    const unsigned long long j[2] = {j0 + (unsigned long long)r0, j0 + (unsigned long long)(two ? r1 : r0)};
    long long i[2];
    draw_index_weighted<2>(wt, seed, ctr0, j, i);
    if (lane == 0) {
      qf[r0] = (float)wt_leaf(wt, (unsigned)i[0]);
      if (two) qf[r1] = (float)wt_leaf(wt, (unsigned)i[1]);
    }
    for (int c4 = lane; c4 < q; c4 += 64) {
      const f32x4 a = *(const f32x4*)(rows + i[0] * ld + 4 * c4);
      f32x4 b = a;
      if (two) b = *(const f32x4*)(rows + i[1] * ld + 4 * c4);
      *(f32x4*)(xb + (long long)r0 * ld + 4 * c4) = a;
      if (two) *(f32x4*)(xb + (long long)r1 * ld + 4 * c4) = b;
    }
  }
}
__device__ __forceinline__ void idle_gather_weighted_q(const IdleWork& w, unsigned long long seed, unsigned long long ctr0,
                                                       unsigned long long j0, int blk, int nblk) {
  const WTab wt = w.wt;
  const int wave = __builtin_amdgcn_readfirstlane(blk * 4 + (int)(threadIdx.x >> 6));
  gather_rows_drawn_weighted_q(w.rows, w.ld, w.xb_dst, w.q_dst, w.n, wt, seed, ctr0, j0, wave, nblk * 4);
}
// c[r] = is_weight(q[r], min q, beta), r < n, by the first wave of ONE block: iql_is_weights_kernel's arithmetic on the
// step's staged q (a minimum of floats is the same in any order), beta read from the call's device word.  No LDS and no
// barrier: the forward's dynamic LDS allowance stays what it is, and the block's other waves go on with their work.
__device__ __forceinline__ void idle_is_weights(const IdleWork& w) {
  if (threadIdx.x < 64) {
    const float beta = *w.is_beta;
    float m = __builtin_inff();
    for (int r = (int)threadIdx.x; r < w.n; r += 64) m = fminf(m, w.q_src[r]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o));
    for (int r = (int)threadIdx.x; r < w.n; r += 64) w.c_dst[r] = is_weight(w.q_src[r], m, beta);
  }
}

// iql_call_setup_weighted_kernel that stages step 0's q next to its rows and publishes the call's beta (every call, a
// continuation included: beta is the call's, the staged rows and q may be the previous call's).
__global__ __launch_bounds__(256) void iql_call_setup_weighted_is_kernel(unsigned long long* hdr, ChunkHdr h,
                                                                         iqlhip_step_scalars* sched_call,
                                                                         const iqlhip_step_scalars* sched_src, int n_steps,
                                                                         const float* rows, long long ld, float* xb, int B,
                                                                         unsigned* drop_dst, int drop_words, unsigned drop_thresh,
                                                                         unsigned* arrivals, unsigned long long* ack,
                                                                         unsigned long long ack_val, WTab wt, float* q_dst,
                                                                         float* beta_dev, float beta) {
  call_setup_head(hdr, h, sched_call, sched_src, n_steps, arrivals, ack, ack_val);
  if (blockIdx.x == 0 && threadIdx.x == 0) *beta_dev = beta;
  if (B > 0)
    gather_rows_drawn_weighted_q(rows, ld, xb, q_dst, B, wt, h.w[HDR_SEED], h.w[HDR_OFFSET], h.w[HDR_POS],
                                 __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6))), (int)gridDim.x * 4);
  if (drop_dst)
    dropmask_words(drop_dst, drop_words, drop_thresh, h.w[HDR_DROP_SEED], h.w[HDR_DROP_STEP],
                   ((int)gridDim.x - 1 - (int)blockIdx.x) * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
}

// The training forward of such a chunk: iql_fwd_kernel's body once more, fp32 (the row-weighted backward is), the idle
// blocks doing idle_block_work<3>.
template <bool W0DMA, bool MULTI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void iql_fwd_weighted_is_kernel(StepParams p) {
  constexpr bool BF16 = false, ONE = false, ROW_EXIT = false;
  constexpr int MIXED_IDLE = 3;
  FWD_NOT_EARLY();
#include "iqlhip_fwd_body.inc"
}
