// iqlhip_variance_kernels.h — one gradient step of the JSRL variance learner (iqlhip_var_step).
// Included by iqlhip.hip behind iqlhip_kernels.h and iqlhip_score_kernels.h (HID, H0_LD, MFMA16, NetPtrs, block_sum_256,
// score_l0).  Two scalar networks S -> 256 -> 256 -> 1 — mf (the value mean, net 0) and vf (the log-variance, net 1) — over
// a rollout of B <= VAR_MAX_ROWS consecutive environment steps, fp32 throughout:
//
//   iql_var_fwd_kernel    both nets over 32-row tiles (grid.y = net): mf on B + 1 rows (the B states and the bootstrap
//                         row, the last next-state), vf on B rows; head outputs, and the H0 / H1 tiles of the net that
//                         is going to be updated
//   iql_var_row_kernel    one block: the reverse recurrence of the sampled values (one lane, the reference's order and
//                         roundings), the clip and its gate, the per-row loss terms and their sum in a fixed order,
//                         the forward scan of the bootstrap row's gradient, the output-gradient column
//   iql_var_bwd_kernel    the chosen net's gradient: blocks 0..15 dW1 (16 output units each), blocks 16..31 dH0 of 16
//                         layer-0 units over all rows and from it dW0 / db0, block 32 dW2, db1, db2.  Every sum runs
//                         over the rows in a fixed order inside one wave or one thread: no atomics
//   iql_var_adam_kernel   torch's Adam on the net's segment of the arena (iql_update_kernel's operation order)
//   iql_var_pack_window_kernel   the packed block from B consecutive rows of a packed replay buffer, the start row an
//                         argument or drawn in the kernel (iqlhip_var_train_steps; DESIGN.md 6l "From a replay buffer")
//
// The kernels are templates of one unused parameter and read neither gridDim nor blockDim, as the scoring group kernels
// (iqlhip_score_kernels.h: why): they are emitted behind every other kernel of the code object.  Their bodies are
// iqlhip_var_*_body.inc: iqlhip_variance_group_kernels.h runs the same text per member of a learner group.
#pragma once

#define VAR_MAX_ROWS 1024        // B of a step
#define VAR_LD 1040              // rows of the per-row scratch: B + 1 rounded up to whole 16-row MFMA tiles
#define VAR_GAMMA 0.99f          // variance_learner.py GAMMA
#define VAR_CLIP_LO 1e-4f
#define VAR_CLIP_HI 1e8f

struct VarFwdParams {
  NetPtrs net[2];                // mf, vf: the fp32 masters of the bound arena
  const float* x;                // the packed block's rows [B + 1][S]: B states, then the last next-state
  int S;
  int rows0, rows1;              // rows each net runs on: B + 1, B
  int keep;                      // the net whose activations are kept for the backward (-1: none)
  float* h0;                     // [VAR_LD][256] post-ReLU activations of `keep`
  float* h1;
  float* out;                    // [2][VAR_LD] head outputs
};

// blockIdx.x = 32-row tile, blockIdx.y = net.  Layer 0 and layer 1 are score_l0 (weights from the cache hierarchy, the
// rows from the packed block / the H0 tile in LDS); a lane's accumulators are 4 consecutive units of one row.  Rows past
// the net's last repeat it; their results are never stored.  The head: per lane 16 units of a row in a fixed order, then
// the row's 16 lane partials (4 waves x 4 lane groups) added in order by one thread.
template <int = 0> __global__ __launch_bounds__(256) void iql_var_fwd_kernel(VarFwdParams p) {
  const int tile = blockIdx.x, net = blockIdx.y;
#include "iqlhip_var_fwd_body.inc"
}

// ---------------------------------------------------------------------------
struct VarRowParams {
  const float* out;              // [2][VAR_LD] head outputs: pred (row B: the bootstrap value), s
  const float* rew;              // [B] rewards of the packed block
  const float* nd;               // [B] next-done flags, 0 or 1
  int B;
  int which;                     // the net whose output gradient is formed: 0 mf, 1 vf, -1 none
  int aligned;                   // 0: the reference's rewards[t - 1] (row 0 takes rewards[B - 1]); 1: rewards[t]
  float* vals;                   // samp | pred | var, each [B] at stride VAR_LD (the handle's host-mapped landing words)
  float* vals2;                  // the same at stride B for a caller's [3][B] array, or null
  float* dy;                     // [VAR_LD] the output-gradient column (mf: B + 1 rows; vf: B rows)
  float* loss;                   // [1]
};

// One block of 256 threads.  samp[t] = reward + (GAMMA * next) * (1 - next_done[t]), every operation rounded on its own,
// walked from t = B - 1 down by lane 0.  loss = mean(0.5 * (log(var) + d^2 / var)), d = pred - samp: a thread adds its
// rows t = tid, tid + 256, ... in order, the 256 sums are added by block_sum_256's fixed tree.  The total gradient on
// samp[t + 1] is its direct term -d / (var B) plus GAMMA * nnt[t] times the total on samp[t]: a forward scan by lane 0,
// whose last value times GAMMA * nnt[B - 1] is the bootstrap row's output gradient (the reference does not detach it).
template <int = 0> __global__ __launch_bounds__(256) void iql_var_row_kernel(VarRowParams p) {
#include "iqlhip_var_row_body.inc"
}

// ---------------------------------------------------------------------------
struct VarBwdParams {
  NetPtrs np;                    // the net being updated
  const float* x;                // [n][S] rows of the packed block
  int S;
  int n;                         // rows: B + 1 (mf) or B (vf)
  const float* h0;               // [VAR_LD][256]
  const float* h1;
  const float* dy;               // [VAR_LD]
  float* dh0;                    // [VAR_LD][256] scratch: dH0 (pre-activation), written and read inside one block
  float* grad;                   // the net's gradient, laid out as its segment of the arena
  unsigned g_w1, g_w0, g_b0, g_b1, g_w2, g_b2;
};

#define VAR_BWD_BLOCKS 33
// dH1 (pre-activation) of a row and a unit is never stored: dy[t] * W2[u] where H1[t][u] > 0, formed where it is an
// operand.  Rows t >= n contribute exact zeros: the gradient-side operand is zero and the other side is read at a
// clamped, valid row (finite x 0 = 0).
template <int = 0> __global__ __launch_bounds__(256) void iql_var_bwd_kernel(VarBwdParams p) {
  const int blk = blockIdx.x;
#include "iqlhip_var_bwd_body.inc"
}

// ---------------------------------------------------------------------------
// torch.optim.Adam's defaults on n words (the net's whole segment: its padding words have zero gradients and stay zero).
// step_neg = -lr / (1 - beta1^t), bc2 = sqrt(1 - beta2^t): float64 on the host; eps is added behind the division by bc2.
template <int = 0> __global__ __launch_bounds__(256) void iql_var_adam_kernel(float* pw, float* m, float* v, const float* gr, int n,
                                                                             float step_neg, float bc2, float omb1, float b2,
                                                                             float omb2, float eps) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
#include "iqlhip_var_adam_body.inc"
}

// ---------------------------------------------------------------------------
struct VarPackParams {
  const float* rows;             // packed replay rows [s | a | s' | r | d | pad] of stride ld
  long long ld;
  long long start;               // the window's first row (the eager form)
  long long last_start;          // size - B: the largest start whose window stays inside the buffer
  unsigned long long seed, j;    // DRAWN: index j of the index stream under `seed` at counter offset 0
  unsigned long long span;       // DRAWN: size - B + 1 values, or the length of `starts`
  const long long* starts;       // DRAWN: a list the draw indexes, or null
  long long* start_out;          // DRAWN: this update's word of the start ring
  int S, A, B;
  float* out;                    // the packed block: [B][S] states | [S] last next-state | [B] rewards | [B] next-dones
};

// Thread e = (t, c) of (B + 1) x (S + 2): t < B copies column c of row start + t — c < S a state word, c = S the reward,
// c = S + 1 the done flag (the buffer stores real_done: run_episodes' next_dones) —, t = B copies word c < S of the
// last row's next-state.  Consecutive lanes read consecutive words of a row.  Row offsets are 64-bit: start * ld floats
// passes 2^31 and 2^32 bytes on a 10 M-row buffer.  DRAWN: every thread draws the start itself (draw_index, as
// gather_rows_drawn: ~150 ALU instructions instead of a dependent load); an entry of `starts` is clamped into
// [0, last_start], so that no list can send a read outside the buffer.
template <bool DRAWN> __global__ __launch_bounds__(256) void iql_var_pack_window_kernel(VarPackParams p) {
#define VAR_PACK_ELEMENT (int)blockIdx.x * 256 + (int)threadIdx.x
#include "iqlhip_var_pack_body.inc"
#undef VAR_PACK_ELEMENT
}
