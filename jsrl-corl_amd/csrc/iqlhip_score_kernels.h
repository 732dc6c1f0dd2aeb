// iqlhip_score_kernels.h — scoring transitions without a step (iqlhip_score_rows).
// Included by iqlhip.hip behind iqlhip_kernels.h (HID, RT_ROWS, H0_LD, T64_LD, W2_LD, NSPLIT, HEAD_LD, MFMA16, NetPtrs,
// PIN_S / PIN_P, sum4).
//
//   iql_score_fwd_kernel     fp32 forward of the seven instances over the row tiles of a chunk: head partials only
//   iql_score_rows_kernel    per row: the eight score columns; per 32-row tile: partial sums of 3 loss numerators + 8 columns
//   iql_score_finish_kernel  one block: tile partials added in tile order, in double; the 11 summary floats
//   iql_score_check_idx_kernel  the index list against [0, n_rows), in front of everything else
//   iql_score_*_group_kernel   the four above for every member of a trainer group in one launch (grid.y = member), and
//                              iql_score_spread_group_kernel: per row, mean and deviation of the members' columns
// The bodies of the first four are iqlhip_score_{fwd,rows,finish,check}_body.inc, shared by the solo and the group kernels.
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
  constexpr bool GROUP = false;      // (p is this launch's chunk)
  constexpr int chunk_n = 0, chunk_ngrp = 0;
  constexpr long long chunk_done = 0;
#include "iqlhip_score_fwd_body.inc"
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
  constexpr bool GROUP = false;
  constexpr int chunk_n = 0;
  constexpr long long chunk_done = 0;
  float* const chunk_out = nullptr;
#include "iqlhip_score_rows_body.inc"
}

// One block.  Thread (j = tid >> 4, s = tid & 15) adds partial j of the s-th sixteenth of the chunk's tiles in tile
// order, in double; the sixteen sums are then added in order s = 0 .. 15 onto the call's running sums acc[j] (`first`:
// the call's first chunk starts them at zero).  `summary` (host-mapped; the call's last chunk): the three losses as
// means over n_total — q_loss with the reference's / 2 — then the eight column means.
__global__ __launch_bounds__(256) void iql_score_finish_kernel(const float* part, int n_tiles, double* acc, int first,
                                                               long long n_total, float* summary) {
#include "iqlhip_score_finish_body.inc"
}

// status[0] = 1 and status[1] = an offending index when some idx[i] lies outside [0, n_rows) (status is host-mapped
// and zeroed by the host before the launch; which offender is reported is not defined).
__global__ __launch_bounds__(256) void iql_score_check_idx_kernel(const long long* idx, long long n, long long n_rows,
                                                                  unsigned long long* status) {
  const long long check_first = (long long)blockIdx.x * blockDim.x + threadIdx.x, check_stride = (long long)gridDim.x * blockDim.x;
#include "iqlhip_score_check_body.inc"
}

// ---------------------------------------------------------------------------
// Trainer groups (iqlhip_group_score_rows): the same bodies on a member's record, grid.y = member.  A record describes
// the member's part of the whole CALL (its rows, its index list, where its output starts); the launch arguments name
// the chunk — rows chunk_done .. chunk_done + chunk_n of every member — so one upload of the records serves every chunk
// of the call.  heads / pi / part of a record are the member's own region of the group's scratch, laid out for a chunk.
// All members score the same number of rows, so every block of a launch has work.
// These kernels are templates (of one unused parameter) so that they are emitted with the deferred instantiations, in
// the order of their first use in iqlhip.hip — behind every other kernel of the code object, whose kernels keep their
// places (the step time is sensitive to them: see the #include of this file in iqlhip.hip).  For the same reason none
// of them reads gridDim or blockDim: a kernel with few arguments that does has its implicit arguments preloaded
// (-amdgpu-kernarg-preload-count), and the compiler re-creates such a kernel in the MIDDLE of the code object — so the
// forward gets its tile streams per member, and the index check its block count, as arguments.
struct ScoreGroupAux {
  long long n_rows;              // rows the member's buffer holds (the index check's bound)
  long long out_step;            // floats the chunk's first row lies behind r.out per row of chunk_done: IQLHIP_N_SCORE
                                 // for the caller's [n][8] array, 0 for the group's chunk-sized scratch rows
  unsigned long long* status;    // host-mapped [2]: the member's words of the index check
};

template <int = 0> __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void iql_score_fwd_group_kernel(
    const ScoreParams* __restrict__ recs, long long chunk_done, int chunk_n, int chunk_ngrp) {
  constexpr bool GROUP = true;
  const ScoreParams& p = recs[blockIdx.y];
#include "iqlhip_score_fwd_body.inc"
}

template <int = 0> __global__ __launch_bounds__(256) void iql_score_rows_group_kernel(const ScoreRowsParams* __restrict__ recs,
                                                                   const ScoreGroupAux* __restrict__ aux,
                                                                   long long chunk_done, int chunk_n) {
  constexpr bool GROUP = true;
  const ScoreRowsParams& p = recs[blockIdx.y];
  float* const chunk_out = p.out ? p.out + chunk_done * aux[blockIdx.y].out_step : nullptr;
#include "iqlhip_score_rows_body.inc"
}

// grid.y = member: the member's tile partials onto its own running sums acc + 16 y; summary (the call's last chunk):
// host-mapped [K][16].
template <int = 0> __global__ __launch_bounds__(256) void iql_score_finish_group_kernel(const ScoreRowsParams* __restrict__ recs, int n_tiles,
                                                                     double* acc_all, int first, long long n_total,
                                                                     float* summary_all) {
  const float* part = recs[blockIdx.y].part;
  double* acc = acc_all + 16 * blockIdx.y;
  float* summary = summary_all ? summary_all + 16 * blockIdx.y : nullptr;
#include "iqlhip_score_finish_body.inc"
}

// Every member's whole index list against its own buffer (grid.y = member), in front of everything else of the call.
template <int = 0> __global__ __launch_bounds__(256) void iql_score_check_idx_group_kernel(const ScoreRowsParams* __restrict__ recs,
                                                                        const ScoreGroupAux* __restrict__ aux,
                                                                        long long n, int n_blocks) {
  const long long check_first = (long long)blockIdx.x * 256 + threadIdx.x, check_stride = (long long)n_blocks * 256;
  const long long* idx = recs[blockIdx.y].idx;
  const long long n_rows = aux[blockIdx.y].n_rows;
  unsigned long long* status = aux[blockIdx.y].status;
#include "iqlhip_score_check_body.inc"
}

// Across-member spread of a chunk: a lane owns row i of the chunk and reads the K members' eight floats of that row in
// member order, from where the rows kernel has just stored them (src[k]: the caller's array at the chunk's first row,
// or the group's scratch rows).  spread[i][j] = (x_0 + x_1 + ...) / K and spread[i][8 + j] = sqrt((sum_k (x_k - mean)^2)
// / K), both in member order 0 .. K - 1, every operation rounded on its own (no fused multiply-add), division and square root
// correctly rounded: two passes over
// the K values (the second reads them again — they are in the cache), no atomics, nothing shared between lanes.
struct ScoreSpreadSrc { const float* src[IQLHIP_MAX_GROUP]; };
template <int = 0> __global__ __launch_bounds__(256) void iql_score_spread_group_kernel(ScoreSpreadSrc s, int K, int chunk_n, float* spread) {
#pragma clang fp contract(off)      // (a square and the sum it is added to stay two roundings)
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= chunk_n) return;
  const size_t at = (size_t)i * IQLHIP_N_SCORE;
  float mean[8], dev[8];
  {
    const f32x4 a = *(const f32x4*)(s.src[0] + at), b = *(const f32x4*)(s.src[0] + at + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { mean[j] = a[j]; mean[4 + j] = b[j]; }
  }
  for (int k = 1; k < K; ++k) {
    const f32x4 a = *(const f32x4*)(s.src[k] + at), b = *(const f32x4*)(s.src[k] + at + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { mean[j] = mean[j] + a[j]; mean[4 + j] = mean[4 + j] + b[j]; }
  }
  const float fk = (float)K;
#pragma unroll
  for (int j = 0; j < 8; ++j) { mean[j] = mean[j] / fk; dev[j] = 0.f; }
  for (int k = 0; k < K; ++k) {
    const f32x4 a = *(const f32x4*)(s.src[k] + at), b = *(const f32x4*)(s.src[k] + at + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float da = a[j] - mean[j], db = b[j] - mean[4 + j];
      dev[j] = dev[j] + da * da;
      dev[4 + j] = dev[4 + j] + db * db;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) dev[j] = sqrtf(dev[j] / fk);
  float* o = spread + (size_t)i * (2 * IQLHIP_N_SCORE);
  *(f32x4*)o = (f32x4){mean[0], mean[1], mean[2], mean[3]};
  *(f32x4*)(o + 4) = (f32x4){mean[4], mean[5], mean[6], mean[7]};
  *(f32x4*)(o + 8) = (f32x4){dev[0], dev[1], dev[2], dev[3]};
  *(f32x4*)(o + 12) = (f32x4){dev[4], dev[5], dev[6], dev[7]};
}
