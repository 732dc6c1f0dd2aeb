// iqlhip_variance_group_kernels.h — the variance learner's five launches for K learners at once (iqlhip_var_group;
// DESIGN.md 6l "Groups of learners").  Included by iqlhip.hip behind iqlhip_variance_kernels.h.  The arithmetic is the
// solo kernels' own text (iqlhip_var_*_body.inc): a block here finds its member, reads that member's record once, and
// runs the solo body on it.  No sum crosses a member and no atomic is used, so a member's result is its solo result bit
// for bit.
//
// The record table: one VarGroupRec per member in device memory, written by the host once per call (K records are too
// large for kernel arguments), and behind it the call's Adam scalars, [n_steps][K].  What changes from one update of a
// burst to the next — the index of the start stream, the words of the two rings, the row of the scalar table — is
// derived from the `step` argument of the launch.
//
// Block -> member.  Blocks are dealt to the 8 XCDs round-robin by their linear id, so id % 8 labels the blocks that share
// an L2.  Every group launch is one-dimensional and maps id -> (member, j) with member % 8 == id % 8: all blocks of a
// member — the 33 backward blocks that each read the member's whole H0 / H1 / dy, the forward tiles that wrote them —
// carry one label.  Within a launch this keeps a member's operand tiles in one L2; across launches it coincides only
// as far as the dispatcher starts every launch on the same XCD (observed, not promised: a speed choice, never needed
// for the result).  With more than 8 members, members m and m + 8 share a label and alternate.  Blocks whose member
// would be >= K exit at once.  The kernels read neither gridDim nor blockDim (iqlhip_variance_kernels.h: why).
#pragma once

struct VarGroupRec {
  VarPackParams pk;              // out = the member's packed-block scratch; j, start_out: update 0's
  VarFwdParams f;
  VarRowParams r;                // loss: update 0's word
  VarBwdParams b;
  float *pw, *m, *v;             // the stepped net's segment of the three arenas
  int n_adam;                    // its words
};

// id = 8 * (j * G + grp) + lab, member = 8 * grp + lab; G = (K + 7) / 8 groups of labels
__device__ __forceinline__ int var_group_member(const unsigned id, const int G, int& j) {
  const unsigned q = id >> 3;
  j = (int)(q / (unsigned)G);
  return (int)(8u * (q % (unsigned)G) + (id & 7u));
}
static unsigned var_group_grid(int K, unsigned per_member) { return 8u * (unsigned)((K + 7) / 8) * per_member; }

// j = the member's pack block.  DRAWN: the start is drawn from the member's own (seed, j + step), or picked from its
// own list by that draw.  (The record is block-uniform: one scalar read at the top, here and below.)
template <bool DRAWN> __global__ __launch_bounds__(256) void iql_var_pack_window_group_kernel(const VarGroupRec* __restrict__ recs,
                                                                                             int K, int G, int step) {
  int j;
  const int mem = var_group_member(blockIdx.x, G, j);
  if (mem >= K) return;
  VarPackParams p = recs[mem].pk;
  if (DRAWN) {
    p.j += (unsigned long long)step;
    p.start_out += step;
  }
#define VAR_PACK_ELEMENT j * 256 + (int)threadIdx.x
#include "iqlhip_var_pack_body.inc"
#undef VAR_PACK_ELEMENT
}

// j = tile * 2 + net (a tile past the net's rows returns inside the body)
template <int = 0> __global__ __launch_bounds__(256) void iql_var_fwd_group_kernel(const VarGroupRec* __restrict__ recs, int K, int G) {
  int j;
  const int mem = var_group_member(blockIdx.x, G, j);
  if (mem >= K) return;
  const VarFwdParams p = recs[mem].f;
  const int tile = j >> 1, net = j & 1;
#include "iqlhip_var_fwd_body.inc"
}

template <int = 0> __global__ __launch_bounds__(256) void iql_var_row_group_kernel(const VarGroupRec* __restrict__ recs, int K, int G,
                                                                                  int step) {
  int j;
  const int mem = var_group_member(blockIdx.x, G, j);
  if (mem >= K) return;
  VarRowParams p = recs[mem].r;
  p.loss += step;
  {      // (the body opens with its floating-point pragma: the start of a compound statement)
#include "iqlhip_var_row_body.inc"
  }
}

// j = the solo kernel's block: 0..15 dW1, 16..31 dH0 / dW0 / db0, 32 dW2 / db1 / db2
template <int = 0> __global__ __launch_bounds__(256) void iql_var_bwd_group_kernel(const VarGroupRec* __restrict__ recs, int K, int G) {
  int blk;
  const int mem = var_group_member(blockIdx.x, G, blk);
  if (mem >= K) return;
  const VarBwdParams p = recs[mem].b;
#include "iqlhip_var_bwd_body.inc"
}

// j = the member's Adam block; tab: the call's scalars [n_steps][K]
template <int = 0> __global__ __launch_bounds__(256) void iql_var_adam_group_kernel(const VarGroupRec* __restrict__ recs,
                                                                                   const iqlhip_var_scalars* __restrict__ tab, int K,
                                                                                   int G, int step) {
  int j;
  const int mem = var_group_member(blockIdx.x, G, j);
  if (mem >= K) return;
  const VarGroupRec& r = recs[mem];
  const iqlhip_var_scalars sc = tab[step * K + mem];
  float *pw = r.pw, *m = r.m, *v = r.v;
  const float* gr = r.b.grad;
  const int n = r.n_adam, i = j * 256 + (int)threadIdx.x;
  const float step_neg = -sc.step_size, bc2 = sc.bc2_sqrt, omb1 = sc.one_minus_beta1, b2 = sc.beta2, omb2 = sc.one_minus_beta2,
              eps = sc.eps;
#include "iqlhip_var_adam_body.inc"
}
