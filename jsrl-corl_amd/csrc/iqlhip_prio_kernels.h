// iqlhip_prio_kernels.h — prioritised replay: TD errors as new priorities of an updatable table (include/iqlhip.h
// "iqlhip_weights_update_td", "iqlhip_train_steps_prioritized"; DESIGN.md 6j "Prioritised replay inside the chunk
// graphs").  Included by iqlhip.hip behind iqlhip_isweight_kernels.h (the existing kernels keep their places in the code
// object); needs it (is_weight's intrinsics, wt_leaf, idle_is_weights) and iqlhip_weighted_kernels.h (the update bodies).
#pragma once

// THE priority formula, for every caller: (max(|e1|, |e2|) + eps)^alpha through the hardware's log2 / exp2, the two
// intrinsics is_weight() uses.  alpha == 0 gives exp2(0 * finite) = 1.0f exactly; the log stays finite because the entry
// points refuse eps == 0 together with alpha == 0 (log2(0) * 0 would be NaN).  With alpha > 0 and eps == 0 a zero TD
// error gives exp2(-inf) = 0: a priority of zero.
__device__ __forceinline__ float td_priority(float e1, float e2, float eps, float alpha) {
  return __builtin_amdgcn_exp2f(alpha * __builtin_amdgcn_logf(fmaxf(fabsf(e1), fabsf(e2)) + eps));
}

// alpha, eps of an update: by value (iqlhip_weights_update_td), or — words != nullptr — read from the device words a
// prioritised call's set-up kernel wrote: words[0] alpha, words[1] eps, words[2] != 0 "the updates of this call are
// live" (0: the rehearsal of iqlhip_train_steps_prioritized_prepare, whose update launches leave the table alone).
struct PrioArgs {
  const float* words;
  float alpha, eps;
};

// The TD source of the update bodies (iqlhip_weighted_kernels.h): entry j's weight is td_priority of td[j][0..1].  A NaN
// or an infinity in either error gives NaN, which wt_update_bad skips and flags (fmaxf alone would drop a NaN).
struct WtTd {
  const float* __restrict__ td;
  float alpha, eps;
  __device__ __forceinline__ float operator()(unsigned j) const {
    const f32x2 e = *(const f32x2*)(td + 2u * j);
    const bool finite = ((__float_as_uint(e[0]) & 0x7F800000u) != 0x7F800000u) && ((__float_as_uint(e[1]) & 0x7F800000u) != 0x7F800000u);
    return finite ? td_priority(e[0], e[1], eps, alpha) : __builtin_nanf("");
  }
};
// (uniform over the grid: every thread reads the same three words)
__device__ __forceinline__ bool prio_source(const float* td, const PrioArgs& a, WtTd* out) {
  float alpha = a.alpha, eps = a.eps;
  if (a.words) {
    if (__float_as_uint(a.words[2]) == 0u) return false;
    alpha = a.words[0];
    eps = a.words[1];
  }
  *out = WtTd{td, alpha, eps};
  return true;
}

__global__ __launch_bounds__(256) void iql_wt_update_stamp_td_kernel(const long long* __restrict__ idx, const float* __restrict__ td,
                                                                     unsigned m, long long bound, WUpd t, PrioArgs a) {
  WtTd w;
  if (prio_source(td, a, &w)) wt_update_stamp(idx, w, m, bound, t);
}
__global__ __launch_bounds__(256) void iql_wt_update_delta_td_kernel(const long long* __restrict__ idx, const float* __restrict__ td,
                                                                     unsigned m, long long bound, WUpd t,
                                                                     unsigned long long* __restrict__ delta, PrioArgs a) {
  WtTd w;
  if (prio_source(td, a, &w)) wt_update_delta(idx, w, m, bound, t, delta);
}
__global__ __launch_bounds__(256) void iql_wt_update_apply_td_kernel(const long long* __restrict__ idx, const float* __restrict__ td,
                                                                     unsigned m, long long bound, WUpd t,
                                                                     const unsigned long long* __restrict__ delta, PrioArgs a) {
  WtTd w;
  if (prio_source(td, a, &w)) wt_update_apply(idx, w, m, bound, t, delta);
}

// ---- prioritised chunk graphs (iqlhip_train_steps_prioritized) ----------------------------------------------------------
// gather_rows_drawn_weighted_q that also stages each drawn row's index at ix[r], next to its q.
__device__ __forceinline__ void gather_rows_drawn_weighted_qi(const float* rows, long long ld, float* xb, float* qf, long long* ix,
                                                              int n, const WTab& wt, unsigned long long seed,
                                                              unsigned long long ctr0, unsigned long long j0, int wave, int n_waves) {
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
      ix[r0] = i[0];
      if (two) {
        qf[r1] = (float)wt_leaf(wt, (unsigned)i[1]);
        ix[r1] = i[1];
      }
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
__device__ __forceinline__ void idle_gather_weighted_qi(const IdleWork& w, unsigned long long seed, unsigned long long ctr0,
                                                        unsigned long long j0, int blk, int nblk) {
  const WTab wt = w.wt;
  const int wave = __builtin_amdgcn_readfirstlane(blk * 4 + (int)(threadIdx.x >> 6));
  gather_rows_drawn_weighted_qi(w.rows, w.ld, w.xb_dst, w.q_dst, w.idx_dst, w.n, wt, seed, ctr0, j0, wave, nblk * 4);
}

// iql_call_setup_weighted_is_kernel that stages step 0's indices too and publishes the call's alpha, eps and whether its
// updates are live (every call, a continuation included).
__global__ __launch_bounds__(256) void iql_call_setup_prio_kernel(unsigned long long* hdr, ChunkHdr h,
                                                                  iqlhip_step_scalars* sched_call,
                                                                  const iqlhip_step_scalars* sched_src, int n_steps,
                                                                  const float* rows, long long ld, float* xb, int B,
                                                                  unsigned* drop_dst, int drop_words, unsigned drop_thresh,
                                                                  unsigned* arrivals, unsigned long long* ack,
                                                                  unsigned long long ack_val, WTab wt, float* q_dst,
                                                                  float* beta_dev, float beta, long long* idx_dst,
                                                                  float* prio_words, float alpha, float eps, unsigned live) {
  call_setup_head(hdr, h, sched_call, sched_src, n_steps, arrivals, ack, ack_val);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *beta_dev = beta;
    prio_words[0] = alpha;
    prio_words[1] = eps;
    prio_words[2] = __uint_as_float(live);
  }
  if (B > 0)
    gather_rows_drawn_weighted_qi(rows, ld, xb, q_dst, idx_dst, B, wt, h.w[HDR_SEED], h.w[HDR_OFFSET], h.w[HDR_POS],
                                  __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6))), (int)gridDim.x * 4);
  if (drop_dst)
    dropmask_words(drop_dst, drop_words, drop_thresh, h.w[HDR_DROP_SEED], h.w[HDR_DROP_STEP],
                   ((int)gridDim.x - 1 - (int)blockIdx.x) * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
}

// The training forward of such a chunk: iql_fwd_kernel's body once more, fp32, the idle blocks doing idle_block_work<4>
// (mode 3 plus the index store).
template <bool W0DMA, bool MULTI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void iql_fwd_prio_kernel(StepParams p) {
  constexpr bool BF16 = false, ONE = false, ROW_EXIT = false;
  constexpr int MIXED_IDLE = 4;
  FWD_NOT_EARLY();
#include "iqlhip_fwd_body.inc"
}
