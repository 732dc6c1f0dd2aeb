// iqlhip_online_prio_kernels.h — online prioritised replay: tables that track their largest priority, new rows entering
// at it, and the launches of iqlhip_online_step_prioritized (include/iqlhip.h "tracking tables"; DESIGN.md 6j "Online
// prioritised replay").  Included by iqlhip.hip behind every other kernel of the library (the existing kernels keep their
// places in the code object); needs iqlhip_weighted_kernels.h (the update bodies, WUpd) and iqlhip_prio_kernels.h (WtTd,
// prio_source, gather_rows_drawn_weighted_qi).
#pragma once

// The tracking instantiations of an update's second launch (wt_update_delta<WS, TRACK = true>): the table's maximum word
// q_max rises to the largest q_new among the launch's winners.  The first and the third launch are the kernels every
// updatable table uses.
__global__ __launch_bounds__(256) void iql_wt_update_delta_track_kernel(const long long* __restrict__ idx, const float* __restrict__ w,
                                                                        unsigned m, long long bound, WUpd t,
                                                                        unsigned long long* __restrict__ delta,
                                                                        unsigned long long* q_max) {
  wt_update_delta<WtVec, true>(idx, WtVec{w}, m, bound, t, delta, q_max);
}
// (a rehearsal — prio_source false — leaves q_max alone as it leaves the tree)
__global__ __launch_bounds__(256) void iql_wt_update_delta_td_track_kernel(const long long* __restrict__ idx, const float* __restrict__ td,
                                                                           unsigned m, long long bound, WUpd t,
                                                                           unsigned long long* __restrict__ delta, PrioArgs a,
                                                                           unsigned long long* q_max) {
  WtTd w;
  if (prio_source(td, a, &w)) wt_update_delta<WtTd, true>(idx, w, m, bound, t, delta, q_max);
}

// q_max of a freshly built tracking table: max(max_i q[i], q(new_row_weight)).  Quantisation is monotone, so the largest
// q is that of the largest weight, whose bit pattern the build's validation has; new_row_weight saturates like any weight.
__global__ __launch_bounds__(64) void iql_wt_qmax_init_kernel(unsigned max_bits, float new_row_weight, int sh0, unsigned sat_bits,
                                                              unsigned long long* q_max) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const unsigned long long q_w = wt_quantise(__uint_as_float(max_bits), sh0);
  const unsigned long long q_new =
      ((__float_as_uint(new_row_weight) & 0x7FFFFFFFu) >= sat_bits) ? WT_Q_SATURATED : wt_quantise(new_row_weight, sh0);
  *q_max = q_w > q_new ? q_w : q_new;
}

// table[row] <- q_max by ONE wave, all of its lanes calling with the same arguments: q_old from the row's level-0 node,
// d = q_max - q_old (two's complement), and on every level the lanes at and behind the row's position inside its node add
// d — wt_update_apply's loop.  One row: no duplicates, no stamp, and no other wave touches the tree, so plain adds do.
// row < t.n is the caller's (a host check).
__device__ __forceinline__ void wt_insert_max(const WUpd& t, const unsigned long long* q_max, unsigned row) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long upto = t.tab[row], before = (row & 63u) ? t.tab[row - 1u] : 0ull;
  const unsigned long long d = *q_max - (upto - before);
  if (!d) return;
  unsigned size = t.n, off = 0u, at = row;
#pragma unroll
  for (int l = 0; l < WT_MAX_LEVELS; ++l) {
    if (l < t.levels) {
      const unsigned first = at & ~63u, width = min(64u, size - first);
      if (lane >= (at & 63u) && lane < width) t.tab[off + first + lane] += d;
    }
    off += (size + 63u) & ~63u;
    size = (size + 63u) >> 6;
    at >>= 6;
  }
}
__global__ __launch_bounds__(64) void iql_wt_insert_max_kernel(WUpd t, const unsigned long long* q_max, unsigned row) {
  wt_insert_max(t, q_max, row);
}

// First launch of iqlhip_online_step_prioritized, one block: the new transition (host-mapped words) to ring row `pointer`
// by waves 1 .. 3, and table[pointer] <- q_max by wave 0.
__global__ __launch_bounds__(256) void iql_online_ring_insert_kernel(float* rows, long long ld, long long pointer,
                                                                     const float* __restrict__ row_pin, WUpd t,
                                                                     const unsigned long long* q_max) {
  if (threadIdx.x < 64u) {
    wt_insert_max(t, q_max, (unsigned)pointer);
  } else {
    float* dst = rows + pointer * ld;
    for (int c = (int)threadIdx.x - 64; c < (int)ld; c += 192) dst[c] = row_pin[c];
  }
}

// Second launch: indices 0 .. n - 1 of the stream (seed, offset) by the table as the first launch left it, each drawn
// row's q (fp32) at qf, its index at ix, the row itself at xb — the prioritised set-up kernel's staging
// (gather_rows_drawn_weighted_qi), a wave per two rows.
__global__ __launch_bounds__(256) void iql_online_draw_gather_kernel(const float* rows, long long ld, float* xb, float* qf,
                                                                     long long* ix, int n, WTab wt, unsigned long long seed,
                                                                     unsigned long long offset) {
  gather_rows_drawn_weighted_qi(rows, ld, xb, qf, ix, n, wt, seed, offset, 0ull,
                                __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6))), (int)gridDim.x * 4);
}
