// iqlhip_group_prio_kernels.h — trainer groups: per-row loss weights, importance-sampling weights and prioritised replay
// (include/iqlhip.h "iqlhip_group_step_rw", "iqlhip_group_train_steps_weighted_is", "iqlhip_group_train_steps_prioritized";
// DESIGN.md 6j "trainer groups").  Included by iqlhip.hip behind iqlhip_prio_kernels.h: the code object's last kernels,
// every existing kernel keeps its place and its code.  Needs iqlhip_kernels.h (GroupRec, GroupDropRec, the backward's
// body), iqlhip_weighted_kernels.h (the draw, the update bodies), iqlhip_isweight_kernels.h (is_weight, wt_leaf) and
// iqlhip_prio_kernels.h (WtTd).
#pragma once

// The row-weighted group backward's two extra arguments, one record per member: an array of its own next to the
// GroupRecs, as GroupDropRec and GroupWtRec are — GroupRec is unchanged.
struct GroupRwRec {
  const float* w;                         // [rows] the member's loss weights
  float* td;                              // [rows][2] where its TD errors go; null: nowhere
};

// iql_bwd_group_kernel with iql_bwd_rw_kernel's switch: member blockIdx.y's loss terms weighted by rws[blockIdx.y].w,
// its TD errors stored to rws[blockIdx.y].td.  fp32, one-slice (b) blocks, no argument-line prefetch, as the plain group
// backward.  A weight of 1.0f reproduces iql_bwd_group_kernel's bits (the multiply comes last: iqlhip_bwd_body.inc).
template <bool FULL>
__global__ __launch_bounds__(256) void iql_bwd_group_rw_kernel(const GroupRec* __restrict__ recs,
                                                               const GroupRwRec* __restrict__ rws) {
  constexpr bool BF16 = false;
  constexpr bool MULTI = false;
  constexpr bool KPF = false;
  constexpr bool RW = true;
  const GroupRec& r = recs[blockIdx.y];
  const float* const rw_w = rws[blockIdx.y].w;
  float* const rw_td = rws[blockIdx.y].td;
  const float* q_heads = r.q_heads; const float* q_xb = r.q_xb; const float* q_h1 = r.q_h1; const float* q_h0 = r.q_h0;
  const float* q_params = r.q_params;
  const unsigned q_dims = r.q_dims, q_ldB = r.q_ldB, q_mbc = r.q_mbc, q_rts = r.q_rts;
  const StepParams& p = r.p;
#include "iqlhip_bwd_body.inc"
}

// What a member's draws, loss weights and table updates need in a burst with importance-sampling weights, one record per
// member.  Everything a step stages exists twice: step s of the call reads half s & 1, and the gather of step s + 1 — which
// runs in front of step s — fills the other one (the solo chunk graphs' two staging parities).
struct GroupPrioRec {
  WTab wt;                                // the member's table; tab == nullptr: it draws uniformly and stages q = 1
  float* xb[2];                           // staged rows
  float* q[2];                            // [B] the staged rows' q as fp32
  long long* idx[2];                      // [B] their indices (members with a table)
  unsigned* drop_bits[2];                 // keep-bits of the two halves
  GroupDropRec drop;                      // the member's keep-bit draw (active: it draws; `bits` is not read: drop_bits is)
  float* c;                               // [B] the running step's loss weights
  float beta;                             // is_beta of the call
  int skip0;                              // 1: step 0's rows, q and indices lie staged (a continued call)
  // prioritised calls: the table update behind every step (up.tab == nullptr: none)
  WUpd up;
  unsigned long long* delta;
  const float* td;                        // [B][2] the running step's TD errors
  long long bound;
  unsigned m;                             // entries of an update: the member's batch rows
  float alpha, eps;
};

// group_gather_weighted (iqlhip_weighted_kernels.h) that also stages each drawn row's q and index — the solo
// gather_rows_drawn_weighted_qi expressions — into staging half s & 1.  A block serves one member: the branches are uniform.
__device__ __forceinline__ void group_gather_weighted_qi(const GroupRec& r, const GroupPrioRec& w, int s) {
  if (s == 0 && w.skip0) return;
  const int h = s & 1;
  const unsigned long long j0 = (unsigned long long)s * (unsigned long long)r.B;
  if (w.wt.tab) {
    // gather_rows_drawn_weighted_qi's loop with the sources and destinations read from the records BEHIND the descents:
    // two descents in flight fill the scalar registers, and with eight more pointers live across them the allocator
    // spills (the empty asm hides the record addresses from the loop-invariant hoist; the reads are cached scalar loads)
    const WTab wt = w.wt;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const int n_waves = (int)gridDim.x * 4;
    const int lane = (int)(threadIdx.x & 63);
    const int n = r.B;
    for (int r0 = wave; r0 < n; r0 += 2 * n_waves) {
      const int r1 = r0 + n_waves;
      const bool two = r1 < n;
      const unsigned long long j[2] = {j0 + (unsigned long long)r0, j0 + (unsigned long long)(two ? r1 : r0)};
      long long i[2];
      const GroupRec* rp = &r;
      asm volatile("" : "+s"(rp));      // (the stream's key and counter too: only the head of a descent reads them)
      draw_index_weighted<2>(wt, rp->seed, rp->offset, j, i);
      const GroupPrioRec* wp = &w;
      asm volatile("" : "+s"(rp), "+s"(wp));
      if (lane == 0) {
        float* qf = wp->q[h];
        long long* ix = wp->idx[h];
        qf[r0] = (float)wt_leaf(wt, (unsigned)i[0]);
        ix[r0] = i[0];
        if (two) {
          qf[r1] = (float)wt_leaf(wt, (unsigned)i[1]);
          ix[r1] = i[1];
        }
      }
      const float* rows = rp->rows;
      const long long ld = rp->ld;
      float* xb = wp->xb[h];
      const int q4 = (int)(ld >> 2);
      for (int c4 = lane; c4 < q4; c4 += 64) {
        const f32x4 a = *(const f32x4*)(rows + i[0] * ld + 4 * c4);
        f32x4 b = a;
        if (two) b = *(const f32x4*)(rows + i[1] * ld + 4 * c4);
        *(f32x4*)(xb + (long long)r0 * ld + 4 * c4) = a;
        if (two) *(f32x4*)(xb + (long long)r1 * ld + 4 * c4) = b;
      }
    }
  } else {
    const int first = (int)blockIdx.x * 256 + (int)threadIdx.x, stride = (int)gridDim.x * 256;
    gather_rows_drawn(r.rows, r.ld, w.xb[h], r.B, r.seed, r.offset, j0, (unsigned long long)r.size, first, stride);
    float* q = w.q[h];
    for (int i = first; i < r.B; i += stride) q[i] = 1.f;
  }
}

// The rows of step `step` of every member, 0 <= step <= n_steps: step n_steps is what a continuing call starts on.
__global__ __launch_bounds__(256) void iql_gather_weighted_qi_group_kernel(const GroupRec* __restrict__ recs,
                                                                           const GroupPrioRec* __restrict__ prs, int step) {
  const GroupRec& r = recs[blockIdx.y];
  const int s = min(max(step, 0), r.n_steps);
  group_gather_weighted_qi(r, prs[blockIdx.y], s);
}

// ... plus that step's keep-bit words of the members that draw some, into the same half, from the far end of the grid
// (iql_gather_weighted_drop_group_kernel's split).  The words are a function of (seed, position) alone: a continued call
// draws step 0's again.  The drop record lies inside the member's GroupPrioRec and is read behind the gather: a third
// record array would be two more scalar registers live across the descents, which have none to spare.
__global__ __launch_bounds__(256) void iql_gather_weighted_qi_drop_group_kernel(const GroupRec* __restrict__ recs,
                                                                                const GroupPrioRec* __restrict__ prs,
                                                                                int step) {
  const GroupRec& r = recs[blockIdx.y];
  const int s = min(max(step, 0), r.n_steps);
  const GroupPrioRec& w = prs[blockIdx.y];
  group_gather_weighted_qi(r, w, s);
  const GroupPrioRec* wp = &w;
  asm volatile("" : "+s"(wp));
  GroupDropRec d = wp->drop;
  if (d.active) {
    d.bits = wp->drop_bits[s & 1];
    group_drop_words(d, d.step0 + (unsigned long long)s, ((int)gridDim.x - 1 - (int)blockIdx.x) * 256 + (int)threadIdx.x,
                     (int)gridDim.x * 256);
  }
}

// c[r] = is_weight(q[r], min q, beta), r < B, of step `step` of every member (grid.y = member, one block each):
// iql_is_weights_kernel's arithmetic on the step's staged q.  A minimum of floats is the same in any order, so the result
// is idle_is_weights' (the solo chunk graphs), bit for bit.
__global__ __launch_bounds__(256) void iql_is_weights_group_kernel(const GroupRec* __restrict__ recs,
                                                                   const GroupPrioRec* __restrict__ prs, int step) {
  __shared__ float red[4];
  const GroupPrioRec& w = prs[blockIdx.y];
  const int n = recs[blockIdx.y].B;
  const float* q = w.q[step & 1];
  float* c = w.c;
  const float beta = w.beta;
  float m = __builtin_inff();
  for (int j = (int)threadIdx.x; j < n; j += 256) m = fminf(m, q[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  const float q_min = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  for (int j = (int)threadIdx.x; j < n; j += 256) c[j] = is_weight(q[j], q_min, beta);
}

// The three launches of the table update behind a prioritised group step: the shared wt_update_*<WtTd> bodies with
// grid.y = member, everything read from the member's record — table[idx of staging half `half`] <- td_priority(the step's
// TD errors).  grid.x is sized by the largest member; a body bounds its entries by the member's own m.  A member without
// an update (up.tab == nullptr) leaves at once.
__global__ __launch_bounds__(256) void iql_wt_update_stamp_td_group_kernel(const GroupPrioRec* __restrict__ prs, int half) {
  const GroupPrioRec& w = prs[blockIdx.y];
  if (!w.up.tab) return;
  const WUpd t = w.up;
  wt_update_stamp(w.idx[half & 1], WtTd{w.td, w.alpha, w.eps}, w.m, w.bound, t);
}
__global__ __launch_bounds__(256) void iql_wt_update_delta_td_group_kernel(const GroupPrioRec* __restrict__ prs, int half) {
  const GroupPrioRec& w = prs[blockIdx.y];
  if (!w.up.tab) return;
  const WUpd t = w.up;
  wt_update_delta(w.idx[half & 1], WtTd{w.td, w.alpha, w.eps}, w.m, w.bound, t, w.delta);
}
__global__ __launch_bounds__(256) void iql_wt_update_apply_td_group_kernel(const GroupPrioRec* __restrict__ prs, int half) {
  const GroupPrioRec& w = prs[blockIdx.y];
  if (!w.up.tab) return;
  const WUpd t = w.up;
  wt_update_apply(w.idx[half & 1], WtTd{w.td, w.alpha, w.eps}, w.m, w.bound, t, (const unsigned long long*)w.delta);
}
