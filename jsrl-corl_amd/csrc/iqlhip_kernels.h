// iqlhip_kernels.h — device code of the IQL step for gfx950 (MI355X, CDNA4).
//
// One step = three launches (cut at every all-to-all seam):
//   iql_fwd_kernel     7 MLP instances x row-tiles(32 rows) x 4 column slices
//   iql_bwd_kernel     (a) dW1 tiles over a 256-row chunk, (b) dH0/dW0 per row-tile
//   iql_update_kernel  slab-sum of gradients + Adam (3 lr groups) + Polyak + losses
//                      (+ extra blocks that gather the NEXT step's rows into the compact batch)
//
// The step is latency-bound at B=256 (0.54 GFLOP against ~20 dependent memory
// round trips), so every kernel is written as: issue ALL global loads of the
// block first -> one wait -> LDS staging -> MFMA phases fed from LDS/registers.
//
// All GEMMs use v_mfma_f32_16x16x4_f32 (exact fp32 fma chain).  Lane maps
// (wave64, l = lane, l15 = l&15, g = l>>4):
//   A operand: A[m=l15][k=g]      B operand: B[k=g][n=l15]
//   C/D:       D[m=4g+reg][n=l15] (reg = 0..3)
// "float4-along-k": a lane loads 4 consecutive k of its row once and feeds element t to
// the t-th of 4 MFMAs — A and B use the same (g,t)->k map, so 4 MFMAs cover 16 k once.
// "float4-along-n": a lane loads 4 consecutive output columns; MFMA t produces columns {4n+t}.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "iqlhip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte access at 4-byte alignment

#define HID 256
#define RT_ROWS 32          // rows per forward / (b) block
#define CHUNK_ROWS 256      // rows per (a) block chunk
#define H0_LD 260           // LDS row stride of a [rows][256] tile (16-B aligned, bank-shifted)
#define H0B_LD 264          // ... of the same tile kept in bf16 (bf16 path): 528-byte rows, 16 rows cover all 64 banks
#define T64_LD 68           // LDS row stride of a [rows][64] tile
#define NSPLIT 4            // column slices of the hidden layer per row tile
#define HEAD_LD 24          // scalar head partials per row: [inst 0..5][ns 0..3]
#define W0_LDS_MAX_K 64     // layer-0 weights are staged in LDS through registers when k_in <= this (64 KiB)
#define W0_DMA_MAX_K 96     // ... and by LDS-DMA up to this width, LDS permitting (host: iqlhip_create)
#define W2_LD 68            // row stride of the forward's head-weight tile in LDS (64 units + 4: bank spread)

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// bf16-operand variant of the large products (layer 0 / layer 1 forward, dW1, dH0, dW0): fp32 accumulate, fp32
// master weights / activations in memory; operands are rounded to bf16 in registers (v_cvt_pk_bf16_f32) and
// eight fp32 MFMAs (8 x 4 k) collapse into one v_mfma_f32_16x16x32_bf16 (32 k).  The operand lane map of the
// bf16 instruction is "8 k per lane"; since both operands are built from the same (lane, element) -> k
// assignment, the loads are exactly those of the fp32 path.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
#define MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)
__device__ __forceinline__ bf16x8 pack8(const f32x4 lo, const f32x4 hi) {
  bf16x8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) { r[i] = (__bf16)lo[i]; r[4 + i] = (__bf16)hi[i]; }
  return r;
}
__device__ __forceinline__ bf16x8 pack8s(const float (&v)[8]) {
  bf16x8 r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = (__bf16)v[i];
  return r;
}
// bf16 STORAGE on the bf16 path (round 3): W1 is read from a bf16 shadow of the fp32 master weights (written by the
// update kernel next to the master, refreshed from it at the start of every library call), and the activations H0 / H1
// the backward re-reads live in memory as bf16.  Every (lane, element) -> index map is that of the fp32 kernels: a
// lane's load shrinks from 16 to 8 bytes (4 elements) or from 8 to 4 (2 elements) — half the bytes through the CU's
// vector-memory pipe, which is what these kernels wait for — and the operands need no conversion any more.
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
template <bool BF16> struct Frag4 { typedef f32x4 type; };
template <> struct Frag4<true> { typedef bf16x4 type; };
template <bool BF16> struct Frag2 { typedef f32x2 type; };
template <> struct Frag2<true> { typedef bf16x2 type; };
// 4 / 2 consecutive elements at element offset `off` of an array whose element type is float (fp32 path) or __bf16
// (bf16 path; `base` then is the bf16 array's address carried in a float pointer)
template <bool BF16> __device__ __forceinline__ typename Frag4<BF16>::type ld4(const float* base, unsigned off) {
  if constexpr (BF16) return *(const bf16x4*)((const __bf16*)base + off);
  else return *(const f32x4*)(base + off);
}
template <bool BF16> __device__ __forceinline__ typename Frag2<BF16>::type ld2(const float* base, unsigned off) {
  if constexpr (BF16) return *(const bf16x2*)((const __bf16*)base + off);
  else return *(const f32x2*)(base + off);
}
template <bool BF16> __device__ __forceinline__ void st4(float* base, unsigned off, const f32x4 v) {
  if constexpr (BF16) {
    bf16x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (__bf16)v[i];
    *(bf16x4*)((__bf16*)base + off) = r;
  } else {
    *(f32x4*)(base + off) = v;
  }
}
__device__ __forceinline__ bf16x8 cat8(const bf16x4 lo, const bf16x4 hi) {
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

struct DevScratch {
  float* h0;        // [4][max_batch][256]  post-ReLU layer-0 activations of V(s),Q1,Q2,pi
  float* h1;        // [4][max_batch][256]
  float* heads;     // [max_batch][HEAD_LD] scalar partials (bias folded into slice 0), then pi: [max_batch][A][NSPLIT]
  float* slab_a;    // [n_chunk_max][n_params]  chunk slabs: w1,b1,w2,b2,log_std grads
  float* slab_b;    // per net [n_rt_max][256*k_in+256]  row-tile slabs: w0,b0 grads
  float* loss_parts;// [4][64]: value, q1, q2 (err^2 sums), actor — per chunk
  float* losses;    // [4]
  long long slab_b_off[4];  // float offset of net's region in slab_b
  int max_batch;
};

// Diagnostic build only (-DIQL_STAMPS): lane 0 of every block writes s_memtime at phase
// boundaries to a buffer of its own; no product path reads it.
#ifdef IQL_STAMPS
__device__ __forceinline__ unsigned long long iql_memtime() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
#define STAMP(p, i)                                                                        \
  do {                                                                                     \
    const unsigned long long t_ = iql_memtime();                                           \
    if (stamps_ && threadIdx.x == 0 && blockIdx.x < stamps_blocks_) stamps_[(long long)blockIdx.x * 16 + (i)] = t_; \
  } while (0)
// (stamps_ is a LOCAL copy of p.stamps: modifying the by-value kernel-argument struct itself makes the compiler
//  copy all of it to scratch at entry — 1.1 KB per thread, ~3 us — which is what an earlier stamps build measured)
// (the buffer holds 4 096 blocks x 16 stamps: a launch with more blocks than fit behind its base stamps only the first ones)
#define STAMP_BASE(p, off) unsigned long long* const stamps_ = (p).stamps ? (p).stamps + (off) : nullptr; \
  const unsigned stamps_blocks_ = (unsigned)((4096 * 16 - (off)) / 16)
// the constant 100 MHz clock shared by the whole chip (s_memtime counters are local and not comparable across blocks)
__device__ __forceinline__ unsigned long long iql_realtime() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
#define RT_ENTRY() const unsigned long long rt_entry_ = iql_realtime()
#define RT_STAMP(p, i, t)                                                                  \
  do {                                                                                     \
    if (stamps_ && threadIdx.x == 0 && blockIdx.x < stamps_blocks_) stamps_[(long long)blockIdx.x * 16 + (i)] = (t); \
  } while (0)
#else
#define STAMP(p, i) do {} while (0)
#define STAMP_BASE(p, off) do {} while (0)
#define RT_ENTRY() do {} while (0)
#define RT_STAMP(p, i, t) do {} while (0)
#define iql_realtime() 0ull
#define rt_entry_ 0ull
#endif

// Direct pointers of one MLP (host-built, so a block needs ONE scalar-load round to find its weights).
struct NetPtrs {
  const float *w0, *b0, *w1, *b1, *w2, *b2;
  int k0, d;
};
// Offsets of one net's gradient tensors inside a chunk slab (= arena layout).
struct NetGrad {
  long long w1, b1, w2, b2, log_std;
};

// The batch is ALWAYS the packed staging buffer xb: rows [s(S) | a(A) | s'(S) | r | d | pad], stride ld.
struct StepParams {
  unsigned long long* stamps;
  NetPtrs inst[8];     // forward instances 0..6: V(s'), V(s), Qt1, Qt2, Q1, Q2, pi
  int xoff[8];         // first column of the instance's input inside a packed row (0 or S+A)
  int slot[8];         // activation slot (0..3) of trainable instances, -1 otherwise
  NetPtrs net[4];      // trainable nets V, Q1, Q2, pi (backward)
  NetGrad go[4];
  const float* log_std;   // Gaussian policy log_std (A floats) or nullptr
  iqlhip_hyper hy;
  DevScratch sc;
  const float* xb;
  int ld, rows;
  int S, A, policy;
  float inv_batch;
  long long n_params;
  // actor dropout (nn.Dropout(p) after each hidden ReLU of the policy MLP, iql.py:331-333): keep-bits
  // [2 layers][max_batch][8 words] (bit j of word w = unit 32w + j), scale = 1/(1-p); null when off
  const unsigned* drop_bits;
  float drop_scale;
  // >= 0: forward ONE instance only (grid = n_rt * NSPLIT, blockIdx = row tile * NSPLIT + column slice) — the
  // policy-inference entry point iqlhip_actor_forward; -1: the training forward over all 7 instances
  int only_inst;
  int w0_lds_k;             // instances with k_in <= this stage their layer-0 weights in LDS
  // Bits 0..1: log2 of the column slices a forward block walks (0, 1, 2): grid = 8 x row tiles x (NSPLIT >> that).  Batches of
  // more row tiles than the chip has CUs take 2 or 4 slices per block: layer 0 and the block prologue are then paid
  // once per 2 / 4 slices instead of once per slice (host: launch_fwd).
  // Bits 2..3: the same for the backward's (b) blocks (dH0 / dW0 of a row tile): the dY / dH1 tile of the 32 rows is
  // built once and 2 or 4 of the 64-column slices are walked with it (host: launch_bwd).  (One word for both: a
  // second one grew the kernel-argument block past 0x478 bytes and every backward launch took 0.17 us longer.)
  int spb_l2;
  // hipGraph chunks: what the forward's idle blocks (blockIdx & 7 == 7, one per row tile and column slice) do while the 7
  // instances run — stage the NEXT step's rows (indices drawn on the spot) into the other staging buffer, copy this
  // step's optimiser scalars into place, draw the next step's dropout keep-bits.  One pointer to a device-resident
  // record (frozen per captured step) instead of the fields themselves: the kernel-argument block stays below the
  // size at which every backward launch was measured 0.17 us slower (0x480 bytes).  Null: nothing to do.
  const struct IdleWork* g_work;
};

// Force kernel-argument fields into SGPRs NOW.  hipcc sinks each s_load next to its first use, which
// turns one scalar-cache miss (~1k cycles at kernel start) into 3-5 dependent ones; an empty asm that
// "uses" the values makes the compiler issue all the loads in one batch behind a single wait.
#define PIN_S(x) asm volatile("" ::"s"(x))
#define PIN_P(x) asm volatile("" ::"s"((unsigned long long)(uintptr_t)(x)))
// For every includer of iqlhip_fwd_body.inc but iql_fwd_kernel_early: the body's EARLY flag off and its leading
// arguments null constants (no code of theirs survives `if constexpr`).
#define FWD_EARLY_MAX_K 32   // iql_fwd_kernel_early: every layer-0 input at most this wide (8 float4 of W0 per thread, 8 k-steps)
// W1 fragment loads (of a wave's 16) that iql_fwd_kernel_early requests in front of the LDS stores; the others go out
// behind layer 0's MFMA groups in fours, as in iql_fwd_kernel (measured 0 .. 16: profiles/fwd_early_w1_ab.txt)
#define FWD_EARLY_W1 4
static_assert(FWD_EARLY_W1 >= 0 && FWD_EARLY_W1 <= 16, "a wave has 16 W1 fragments");
#define FWD_NOT_EARLY()                                                                                   \
  constexpr bool EARLY = false;                                                                           \
  constexpr const float *q_params = nullptr, *q_target = nullptr, *q_xb = nullptr;                        \
  constexpr const unsigned* q_drop = nullptr;                                                             \
  constexpr unsigned q_dims = 0, q_ldB = 0, q_mb = 0

// ---------------------------------------------------------------------------
// A 32-row tile of packed rows is staged whole (flat float4 copy).  The packed stride 2S+A+2 (padded to 4)
// reaches 260 floats at the dimension limits, i.e. up to 9 float4 per thread; the common dims need 2-4, so the
// copy is instantiated for 3 / 5 / 9 (straight-line loads each: a load under a run-time trip count would be
// waited for individually).
#define XR_MAX_F4 9
#define XR_LD_MAX 260
template <int Q0, int Q1>
__device__ __forceinline__ void xr_issue(f32x4 (&xr)[XR_MAX_F4], const float* xb, int first_f4, int n_x, int x_last) {
#pragma unroll
  for (int q = Q0; q < Q1; ++q) {
    const int f = min(first_f4 + min((int)threadIdx.x + 256 * q, n_x - 1), x_last);
    xr[q] = *(const f32x4*)(xb + 4u * (unsigned)f);
  }
}
__device__ __forceinline__ void xr_load(f32x4 (&xr)[XR_MAX_F4], const float* xb, int first_f4, int n_x, int x_last) {
#pragma unroll
  for (int q = 0; q < XR_MAX_F4; ++q) xr[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
  xr_issue<0, 3>(xr, xb, first_f4, n_x, x_last);
  if (n_x > 3 * 256) {
    xr_issue<3, 5>(xr, xb, first_f4, n_x, x_last);
    if (n_x > 5 * 256) xr_issue<5, 9>(xr, xb, first_f4, n_x, x_last);
  }
}
__device__ __forceinline__ void xr_store(const f32x4 (&xr)[XR_MAX_F4], float* Xr, int n_x) {
#pragma unroll
  for (int q = 0; q < XR_MAX_F4; ++q) {
    const int f = (int)threadIdx.x + 256 * q;
    if (f < n_x) *(f32x4*)(Xr + 4 * f) = xr[q];
  }
}

__device__ __forceinline__ void lds_dma16(const float* gsrc, float* lds_wave_base) {
  // 64 lanes x 16 B: global (per-lane address) -> LDS (wave-uniform base + lane*16), no VGPR staging
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// ---------------------------------------------------------------------------
// rows[idx[r]] -> xb[r], r < n: one float4 per thread-iteration (rows are 16-B aligned, ld % 4 == 0)
// n_rows > 0: an index outside [0, n_rows) is never dereferenced — its output row is filled with NaN instead (the
// reference's torch indexing raises IndexError, iql.py:173-177; the Python shim raises it on the host before the
// launch — this guard only makes sure that a caller of the C ABI cannot fault the GPU with a bad index).
__device__ __forceinline__ void gather_rows_flat(const float* rows, long long ld, const long long* idx, float* xb,
                                                 int n, int first, int stride, long long n_rows = 0) {
  const int q = (int)(ld >> 2);
  const int total = n * q;
  for (int e = first; e < total; e += stride) {
    const int r = e / q, c4 = e - r * q;
    const long long i = idx[r];
    f32x4 v;
    if (n_rows > 0 && (i < 0 || i >= n_rows)) {
      const float nanv = __builtin_nanf("");
      v = (f32x4){nanv, nanv, nanv, nanv};
    } else {
      v = *(const f32x4*)(rows + i * ld + 4 * c4);
    }
    *(f32x4*)(xb + (long long)r * ld + 4 * c4) = v;
  }
}

// ---------------------------------------------------------------------------
// Device words a run of steps (hipGraph chunks) reads its per-launch values from: kernel arguments of a captured graph
// are frozen, these words are not.  iql_call_setup_kernel writes them ONCE per iqlhip_train_steps call; every chunk
// then advances them itself (thread 0 of its last update kernel: POS, DROP_STEP, BASE, XSTEP), so the chunks of a
// call chain on the device with no host-side launch between them.
//   SIZE      rows the index draw covers           SEED / OFFSET  Philox key / the call's first counter
//   POS       indices drawn before this chunk (index j of the call = counter OFFSET + j / 2, word pair j & 1)
//   BASE      steps of the call before this chunk (row of the call's scalar table, slot of the loss ring)
//   DROP_*    dropout stream                        XSTEP          steps exchanged before this chunk (P2P flags)
//   SIZE_ON   two-source calls (iqlhip_train_steps_mixed): rows the draw of a batch's online part covers — SIZE is
//             then the offline buffer's; a header word, so the online ring may grow between calls (0 in a plain call)
enum { HDR_SIZE = 0, HDR_SEED = 1, HDR_OFFSET = 2, HDR_DROP_STEP = 3, HDR_DROP_SEED = 4, HDR_BASE = 5, HDR_XSTEP = 6,
       HDR_POS = 7, HDR_SIZE_ON = 8, HDR_WORDS = 9 };
struct ChunkHdr { unsigned long long w[HDR_WORDS]; };

// Philox4x32-10 (Salmon et al. 2011).
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// Dropout keep-bits for one step: word w (of n_words = 2 * max_batch * 8) gets 32 independent Bernoulli(1-p)
// bits: keep iff u32 >= thresh (thresh = p * 2^32).  Stream: key = seed, counter = (word, call, step).
// (keep_word: the 32 bits of stream word w at position pos — eight counters (w, j | tag, lo32 pos, hi32 pos), bit
//  4 j + t = (output t >= thresh); the training stream's tag is "DROP", the inference stream's "ADRP")
__device__ __forceinline__ unsigned keep_word(uint32_t w, uint32_t tag, unsigned thresh, unsigned long long seed,
                                              unsigned long long pos) {
  unsigned word = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    uint32_t c[4] = {w, (uint32_t)j | tag, (uint32_t)pos, (uint32_t)(pos >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
    for (int q = 0; q < 4; ++q) word |= (c[q] >= thresh ? 1u : 0u) << (4 * j + q);
  }
  return word;
}
__device__ __forceinline__ void dropmask_words(unsigned* bits, int n_words, unsigned thresh, unsigned long long seed,
                                               unsigned long long step, int first, int stride) {
  for (int w = first; w < n_words; w += stride)
    bits[w] = keep_word((uint32_t)w, 0x44524F50u /* "DROP" */, thresh, seed, step);
}

// Index j of a call's draw: Philox4x32-10, counter = ctr0 + j / 2, key = seed; the counter's four words give two
// indices, uniform over [0, size) by multiply-high of 64 random bits (bias <= size / 2^64) — the stream
// iql_draw_indices_kernel writes out (np.random.randint's distribution, iql.py:172).
__device__ __forceinline__ long long draw_index(unsigned long long seed, unsigned long long ctr0, unsigned long long j,
                                                unsigned long long size) {
  const unsigned long long ctr = ctr0 + (j >> 1);
  uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0x49514C48u /* "IQLH" */, 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const unsigned long long r = (j & 1ull) ? (((unsigned long long)c[3] << 32) | c[2]) : (((unsigned long long)c[1] << 32) | c[0]);
  return (long long)__umul64hi(r, size);
}

// rows[draw(j0 + r)] -> xb[r], r < n: the gather of a step whose indices nobody stores — every thread of a row's
// float4s draws that row's index itself (~150 ALU instructions instead of a dependent idx -> row round trip to HBM).
__device__ __forceinline__ void gather_rows_drawn(const float* rows, long long ld, float* xb, int n, unsigned long long seed,
                                                  unsigned long long ctr0, unsigned long long j0, unsigned long long size,
                                                  int first, int stride) {
  const int q = (int)(ld >> 2);
  const int total = n * q;
  for (int e = first; e < total; e += stride) {
    const int r = e / q, c4 = e - r * q;
    const long long i = draw_index(seed, ctr0, j0 + (unsigned long long)r, size);
    *(f32x4*)(xb + (long long)r * ld + 4 * c4) = *(const f32x4*)(rows + i * ld + 4 * c4);
  }
}

// The same for a batch mixed from two buffers (iqlhip_train_steps_mixed): row r < n_off is drawn over [0, size_off) from
// rows_off, row r >= n_off over [0, size_on) from rows_on — index j0 + r of the call's one stream either way, so the
// counters a call consumes do not depend on the split.
__device__ __forceinline__ void gather_rows_drawn2(const float* rows_off, const float* rows_on, long long ld, float* xb, int n,
                                                   int n_off, unsigned long long seed, unsigned long long ctr0,
                                                   unsigned long long j0, unsigned long long size_off,
                                                   unsigned long long size_on, int first, int stride) {
  const int q = (int)(ld >> 2);
  const int total = n * q;
  for (int e = first; e < total; e += stride) {
    const int r = e / q, c4 = e - r * q;
    const bool on = r >= n_off;
    const long long i = draw_index(seed, ctr0, j0 + (unsigned long long)r, on ? size_on : size_off);
    const float* src = on ? rows_on : rows_off;
    *(f32x4*)(xb + (long long)r * ld + 4 * c4) = *(const f32x4*)(src + i * ld + 4 * c4);
  }
}

// What a kernel needs of a weighted-sampling table (iqlhip_weighted_kernels.h; by value: kernel argument, IdleWork record).
struct WTab {
  const unsigned long long* tab;          // level 0 = cum[0..n), the search levels behind it
  unsigned n;
  unsigned short levels;
  unsigned short local;                   // 1: an updatable table — every node holds the prefix sums of its own 64 children
};
static_assert(sizeof(WTab) == 16, "WTab keeps its size: it lies inside IdleWork and among kernel arguments");

// What the idle eighth of a captured step's forward grid does (StepParams::g_work; one record per step of a chunk,
// written once when the chunk is captured):
struct IdleWork {
  const float* rows;                      // replay rows the NEXT step's batch is drawn from
  long long ld;
  float* xb_dst;                          // the staging buffer the next step reads (the other one of the two)
  const unsigned long long* hdr;
  const iqlhip_step_scalars* sched_call;  // the call's scalar table (device copy)
  iqlhip_step_scalars* sched_dst;         // where THIS step's update kernel reads its scalars (frozen address)
  unsigned* drop_dst;                     // keep-bits of the next step (the other parity's buffer); null: no dropout
  int drop_words;
  unsigned drop_thresh;
  int n;                                  // rows per step
  int k;                                  // this step's number inside the chunk
  // two-source chunks only (MIXED): `rows` is the offline buffer, rows_on the online one, batch rows >= n_off are its
  const float* rows_on;
  int n_off;
  // weighted chunks only (MODE 2 and 3): the cumulative table the next step's rows are drawn by
  WTab wt;
  // weighted chunks with importance-sampling weights only (MODE 3): the next step's staged q (fp32, the
  // other parity's half), this step's (staged by the step before or by the set-up kernel), this step's c — read by its
  // row-weighted backward — and the device word that holds the call's beta
  float* q_dst;
  const float* q_src;
  float* c_dst;
  const float* is_beta;
  // prioritised chunks only (MODE 4): where the next step's drawn indices are staged, next to its q (int64,
  // the other parity's half) — what that step's in-graph table update reads
  long long* idx_dst;
};
// (defined in iqlhip_weighted_kernels.h, behind every kernel of this file)
__device__ __forceinline__ void idle_gather_weighted(const IdleWork& w, unsigned long long seed, unsigned long long ctr0,
                                                     unsigned long long j0, int blk, int nblk);
// (defined in iqlhip_isweight_kernels.h, behind every kernel of this file)
__device__ __forceinline__ void idle_gather_weighted_q(const IdleWork& w, unsigned long long seed, unsigned long long ctr0,
                                                       unsigned long long j0, int blk, int nblk);
__device__ __forceinline__ void idle_is_weights(const IdleWork& w);
// (defined in iqlhip_prio_kernels.h, behind every kernel of this file)
__device__ __forceinline__ void idle_gather_weighted_qi(const IdleWork& w, unsigned long long seed, unsigned long long ctr0,
                                                        unsigned long long j0, int blk, int nblk);
// MODE: 1 = the idle work of a two-source chunk (iql_fwd_mixed_kernel), 2 = of a weighted chunk
// (iql_fwd_weighted_kernel), 3 = of a weighted chunk with importance-sampling weights (iql_fwd_weighted_is_kernel),
// 4 = of a prioritised chunk (iql_fwd_prio_kernel: mode 3 plus the drawn indices) — a
// compile-time switch, so that the forward kernels of plain calls hold no trace of any.
template <int MODE = 0>
__device__ __forceinline__ void idle_block_work(const IdleWork* wk, int blk, int nblk) {
  constexpr bool MIXED = MODE == 1;
  const IdleWork w = *wk;
  const unsigned long long size = w.hdr[HDR_SIZE], seed = w.hdr[HDR_SEED], ctr0 = w.hdr[HDR_OFFSET], pos = w.hdr[HDR_POS];
  const unsigned long long base = w.hdr[HDR_BASE], dseed = w.hdr[HDR_DROP_SEED], dstep = w.hdr[HDR_DROP_STEP];
  // the next step's rows: index j = POS + (k + 1) n + r of the call (for the chunk's last step that is step 0 of
  // whatever runs next: the following chunk, or the next call when it continues this one's stream)
  if constexpr (MODE == 4) {
    idle_gather_weighted_qi(w, seed, ctr0, pos + (unsigned long long)(w.k + 1) * (unsigned long long)w.n, blk, nblk);
    if (blk == nblk - 1) idle_is_weights(w);
  } else if constexpr (MODE == 3) {
    idle_gather_weighted_q(w, seed, ctr0, pos + (unsigned long long)(w.k + 1) * (unsigned long long)w.n, blk, nblk);
    if (blk == nblk - 1) idle_is_weights(w);       // THIS step's c, from the q the step before staged: one block
  } else if constexpr (MODE == 2)
    idle_gather_weighted(w, seed, ctr0, pos + (unsigned long long)(w.k + 1) * (unsigned long long)w.n, blk, nblk);
  else if (MIXED)
    gather_rows_drawn2(w.rows, w.rows_on, w.ld, w.xb_dst, w.n, w.n_off, seed, ctr0,
                       pos + (unsigned long long)(w.k + 1) * (unsigned long long)w.n, size, w.hdr[HDR_SIZE_ON],
                       blk * 256 + (int)threadIdx.x, nblk * 256);
  else
    gather_rows_drawn(w.rows, w.ld, w.xb_dst, w.n, seed, ctr0, pos + (unsigned long long)(w.k + 1) * (unsigned long long)w.n,
                      size, blk * 256 + (int)threadIdx.x, nblk * 256);
  // this step's optimiser scalars: row BASE + k of the call's table -> the slot this step's update kernel reads
  if (blk == nblk - 1 && threadIdx.x < sizeof(iqlhip_step_scalars) / sizeof(float))
    ((float*)w.sched_dst)[threadIdx.x] = ((const float*)(w.sched_call + base + (unsigned long long)w.k))[threadIdx.x];
  // the next step's dropout keep-bits (the last blocks first: the gather occupies the first ones)
  if (w.drop_dst)
    dropmask_words(w.drop_dst, w.drop_words, w.drop_thresh, dseed, dstep + (unsigned long long)(w.k + 1),
                   (nblk - 1 - blk) * 256 + (int)threadIdx.x, nblk * 256);
}

// A net's tensors inside the parameter arena, from the dims alone (restates iqlhip_arena_layout; used by the kernels whose
// leading, preloaded arguments carry the arena pointer and the packed dims: iql_fwd_kernel_early, iql_bwd_kernel).
struct ArenaOff { unsigned w0, b0, b1, w2, b2, log_std; int k0, d; };
__device__ __forceinline__ ArenaOff arena_off(int net, int S, int A, bool gauss) {
  auto seg = [&](int k, int d, bool ls) -> unsigned {
    const unsigned n = 65536u + 256u * (unsigned)k + 512u + 256u * (unsigned)d + (((unsigned)d + 3u) & ~3u) + (ls ? (((unsigned)A + 3u) & ~3u) : 0u);
    return (n + 63u) & ~63u;
  };
  const unsigned sV = seg(S, 1, false), sQ = seg(S + A, 1, false);
  const unsigned begin = (net == IQLHIP_NET_V) ? 0u : ((net == IQLHIP_NET_Q1) ? sV : ((net == IQLHIP_NET_Q2) ? sV + sQ : sV + 2u * sQ));
  ArenaOff o;
  o.k0 = (net == IQLHIP_NET_Q1 || net == IQLHIP_NET_Q2) ? S + A : S;
  o.d = (net == IQLHIP_NET_PI) ? A : 1;
  o.w0 = begin + 65536u;
  o.b0 = o.w0 + 256u * (unsigned)o.k0;
  o.b1 = o.b0 + 256u;
  o.w2 = o.b1 + 256u;
  o.b2 = o.w2 + 256u * (unsigned)o.d;
  o.log_std = o.b2 + (((unsigned)o.d + 3u) & ~3u);
  return o;
}

// Forward: block = (instance, row tile of 32 rows, column slice ns of 64 hidden-1 units).
// grid = 8 * n_rt * NSPLIT; blockIdx & 7 = instance (7 = idle) so that the
// blocks of one instance share an XCD and hence one L2 copy of its weights.
// W0DMA: the variant that may stage wide layer-0 weights by LDS-DMA.  A separate instantiation because the mere
// presence of an LDS-DMA makes the compiler wait vmcnt(0) before LDS reads on every path it may reach (measured:
// +1 us on the narrow-input configs, whose W1 prefetch then no longer streams under layer 0).
// Layer 0 with bf16 operands: the 8 k-steps of a chunk (lane group g holds k = 4 ks + g, ks = 0..7, of both operands)
// are one v_mfma_f32_16x16x32_bf16 per (row tile, unit tile): 8 MFMAs of 16 cycles instead of 64 of 32.
__device__ __forceinline__ void l0_chunk_bf16(f32x4 (&acc)[2][4], const float (&bq)[8][4], const float (&aq)[8][2]) {
  bf16x8 B[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    float t8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t8[e] = aq[e][r];
    B[r] = pack8s(t8);
  }
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    float t8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t8[e] = bq[e][ct];
    const bf16x8 A = pack8s(t8);
    acc[0][ct] = MFMA_BF16(A, B[0], acc[0][ct]);
    acc[1][ct] = MFMA_BF16(A, B[1], acc[1][ct]);
  }
}

// (two waves per SIMD — 256 registers, accumulators included — so that two blocks can share a CU when LDS allows)
// ONE: the policy-inference launch (one instance, p.only_inst).  A template flag rather than a run-time test of
// p.only_inst: the test was a scalar load + wait + branch in FRONT of the argument batch below — two dependent
// scalar-cache misses at the start of every training forward instead of one.
template <bool BF16, bool W0DMA, bool MULTI, bool ONE = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void iql_fwd_kernel(StepParams p) {
  constexpr bool ROW_EXIT = false;      // (a grid of exactly this agent's row tiles)
  constexpr bool MIXED_IDLE = false;
  FWD_NOT_EARLY();
#include "iqlhip_fwd_body.inc"
}
// The one-slice fp32 training forward of a plain step when every instance stages W0 in LDS through registers
// (state_dim + action_dim <= 32; host: fwd_early_ok): iql_fwd_kernel<false, false, false>'s work with LEADING, PRELOADED
// arguments (the library is built with -mllvm -amdgpu-kernarg-preload-count=14; these are 11 dwords) that suffice to
// form every address of the block's issue section — the parameter arena, the target arena biased by the target
// segment's offset so that parameter-arena offsets hold in it, the staged batch, the dropout keep-bits (null: off) and
//   q_dims = S | A << 8 | policy << 14      q_ldB = ld | rows << 10      q_mb = max_batch
// (arena_off gives a net's tensors from the dims; W1 leads its segment).  A block therefore requests its small
// operands and the first quarter of its W1 slice in the first few hundred cycles, instead of waiting 450-700 cycles for
// the by-value `p`; the rest of W1 still goes out between layer 0's MFMAs (iqlhip_fwd_body.inc: why not all of it).
// What `p` still supplies (the instance's row offset and slot, the activation and head pointers, the idle blocks'
// record) is fetched behind the issue section.  `p` follows at byte 48: the argument block stays below
// iql_bwd_kernel's (56 + sizeof(StepParams)).
// A kernel of its own, not a flag of iql_fwd_kernel: every other instantiation keeps its symbol and its code.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void iql_fwd_kernel_early(
    const float* q_params, const float* q_target, const float* q_xb, const unsigned* q_drop, unsigned q_dims, unsigned q_ldB,
    unsigned q_mb, StepParams p) {
  constexpr bool BF16 = false, W0DMA = false, MULTI = false, ONE = false, ROW_EXIT = false, MIXED_IDLE = false;
  constexpr bool EARLY = true;
#include "iqlhip_fwd_body.inc"
}

// ---------------------------------------------------------------------------
// Loss gradients at the heads.  The per-row inputs are loaded first (RowIn, issue
// only) so that the caller can overlap them with its other loads; row_finish does
// the arithmetic.  Head = sum of the 4 column-slice partials in fixed order
// (the bias is already inside slice 0).
struct RowIn {
  f32x4 h[6];       // scalar head partials: inst 0..5 x ns 0..3
  float r, d;
};

// The scalar per-row loss inputs of one row (issue only).  The policy's per-(row, dim) inputs are loaded by the
// callers as coalesced (row, dim) work items.
// (offsets are formed as 32-bit UNSIGNED values on uniform base pointers: the load then takes the SGPR-base +
//  VGPR-offset form and needs no 64-bit address arithmetic on the vector ALU — with signed indices every load of
//  the backward's issue phase cost a sign extension and a 64-bit multiply-add, ~300 extra instructions per block)
__device__ __forceinline__ void row_issue(const StepParams& p, int row, RowIn& in) {
  const float* hb = p.sc.heads;
  const unsigned o = (unsigned)row * (unsigned)HEAD_LD;
#pragma unroll
  for (int i = 0; i < 6; ++i) in.h[i] = *(const f32x4*)(hb + (o + 4u * i));
  const float* xb = p.xb;
  const unsigned ox = (unsigned)row * (unsigned)p.ld + (unsigned)(2 * p.S + p.A);
  in.r = xb[ox];
  in.d = xb[ox + 1u];
}

// (the same with every input an explicit argument: the backward passes values that arrive preloaded in SGPRs)
__device__ __forceinline__ void row_issue_hot(const float* heads, const float* xb, int ld, int S, int A, int row, RowIn& in) {
  const unsigned o = (unsigned)row * (unsigned)HEAD_LD;
#pragma unroll
  for (int i = 0; i < 6; ++i) in.h[i] = *(const f32x4*)(heads + (o + 4u * i));
  const unsigned ox = (unsigned)row * (unsigned)ld + (unsigned)(2 * S + A);
  in.r = xb[ox];
  in.d = xb[ox + 1u];
}

__device__ __forceinline__ float sum4(const f32x4 v) { return ((v[0] + v[1]) + v[2]) + v[3]; }

// tanh(x) = 1 - 2 / (exp(2x) + 1) on the hardware transcendentals: exp2 (v_exp_f32, 1 ulp) of 2x*log2(e) and
// v_rcp_f32 (1 ulp).  Absolute error < 1e-7 (the argument rounding |2x log2e| * 6e-8 is damped by
// d tanh / d e = 2 / (e + 1)^2); saturates correctly: e -> inf gives 1, e -> 0 gives -1.  The policy blocks of the
// backward evaluate it 256 x A times EACH (every one needs every row's dY), so libm's expf + IEEE division
// (~35 instructions) were a measurable part of those blocks — the kernel's long pole.
__device__ __forceinline__ float tanh_via_exp(float x) {
  const float e = __builtin_amdgcn_exp2f(x * 2.885390081777927f);     // exp(2x)
  return 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f);
}

// row_finish: dL/d(head pre-activation) of a SCALAR net (V, Q1, Q2) for one row -> dyrow[0]; loss terms:
//   V: lossA = w*u^2     Q1/Q2: lossA = e1^2, lossB = e2^2
// (the policy's per-(row, dim) terms are formed in the callers as coalesced work items.)
// PiConst: per-action-dim constants of the Gaussian policy (clamped log_std, 1/var): lane dd holds dim dd's; callers
// fetch them with a lane shuffle, so all lanes of the wave must be active at that point.
struct PiConst { float ls, ivar; };
// The raw log_std word is loaded by pi_ls_issue() BEFORE the block's big prefetches: vmcnt retires in issue
// order, so a load issued after them would make the loss arithmetic wait for all of them.
__device__ __forceinline__ float pi_ls_issue(const StepParams& p) {
  const float* src = (p.policy == IQLHIP_POLICY_GAUSSIAN) ? p.log_std : p.xb;      // any valid address when unused
  return src[min((int)(threadIdx.x & 63), p.A - 1)];
}
__device__ __forceinline__ float pi_ls_issue_hot(const float* log_std, const float* xb, int policy, int A) {
  const float* src = (policy == IQLHIP_POLICY_GAUSSIAN) ? log_std : xb;      // any valid address when unused
  return src[min((int)(threadIdx.x & 63), A - 1)];
}
__device__ __forceinline__ PiConst pi_consts_hot(const StepParams& p, int policy, int net, float lsr) {
  PiConst c;
  c.ls = 0.f;
  c.ivar = 1.f;
  if (net == IQLHIP_NET_PI && policy == IQLHIP_POLICY_GAUSSIAN) {
    c.ls = fminf(fmaxf(lsr, p.hy.log_std_min), p.hy.log_std_max);
    const float sig = expf(c.ls);
    c.ivar = 1.f / (sig * sig);
  }
  return c;
}
__device__ __forceinline__ PiConst pi_consts(const StepParams& p, int net, float lsr) {
  PiConst c;
  c.ls = 0.f;
  c.ivar = 1.f;
  if (net == IQLHIP_NET_PI && p.policy == IQLHIP_POLICY_GAUSSIAN) {
    c.ls = fminf(fmaxf(lsr, p.hy.log_std_min), p.hy.log_std_max);
    const float sig = expf(c.ls);
    c.ivar = 1.f / (sig * sig);
  }
  return c;
}

__device__ __forceinline__ void row_finish(const StepParams& p, int net, const RowIn& in, float* dyrow,
                                           float& lossA, float& lossB) {
  const float invB = p.inv_batch;
  lossA = 0.f;
  lossB = 0.f;
  if (net == IQLHIP_NET_V) {
    const float tq = fminf(sum4(in.h[2]), sum4(in.h[3]));
    const float u = tq - sum4(in.h[1]);
    const float wgt = fabsf(p.hy.iql_tau - ((u < 0.f) ? 1.f : 0.f));
    lossA = wgt * u * u;
    dyrow[0] = (-2.f * wgt * u) * invB;
    return;
  }
  const float nv = sum4(in.h[0]);
  const float y = in.r + ((1.f - in.d) * p.hy.discount) * nv;
  const float e1 = sum4(in.h[4]) - y;
  const float e2 = sum4(in.h[5]) - y;
  lossA = e1 * e1;
  lossB = e2 * e2;
  dyrow[0] = ((net == IQLHIP_NET_Q1) ? e1 : e2) * invB;
}
// The row's TD errors (q1 - y, q2 - y) as row_finish forms them: the same expressions in the same order, so the stored
// values are the ones the loss used (row-weighted backward only: iql_bwd_rw_kernel).
__device__ __forceinline__ f32x2 row_td_errors(const StepParams& p, const RowIn& in) {
  const float nv = sum4(in.h[0]);
  const float y = in.r + ((1.f - in.d) * p.hy.discount) * nv;
  return (f32x2){sum4(in.h[4]) - y, sum4(in.h[5]) - y};
}

__device__ __forceinline__ float block_sum_256(float v, float* red /*>=4 floats*/) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------------------
// Backward.  blockIdx & 7 = x: net = x & 3, half = x >> 2 (two XCD groups per net).
// Within a net, local id < 32*n_chunk  -> (a) block: chunk c, j-tile jt (32 rows of W1), i-tile it (64 cols)
//               otherwise              -> (b) block: row tile rt (32 rows), i-slice is (64 cols)
// dH1pre tiles of one wave's 64 rows: pre[t][ta] += dY[16t.., 4 k1 + g] x W2s[4 k1 + g][2 l15 + ta], NK k-steps
// (straight-line: all LDS operands of a k-step in one batch).
template <int NK>
__device__ __forceinline__ void dh1_mfma(f32x4 (&pre)[4][2], const float* dYs, const float* W2s, int DYA, int wave,
                                         int g, int l15) {
#pragma unroll
  for (int k1 = 0; k1 < NK; ++k1) {
    float a1[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) a1[t] = dYs[(64 * wave + 16 * t + l15) * DYA + 4 * k1 + g];
    const f32x2 b1 = *(const f32x2*)(W2s + (4 * k1 + g) * 32 + 2 * l15);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      pre[t][0] = MFMA16(a1[t], b1[0], pre[t][0]);
      pre[t][1] = MFMA16(a1[t], b1[1], pre[t][1]);
    }
  }
}

// Policy loss terms of 8 (row, dim) items — one action dim, eight rows — as straight-line code: both policy kinds are
// evaluated and selected on the (uniform) kind, dims beyond A on `live`; no branch, no memory access.
//   gaussian: -log N(a; mu, sigma) = q/2 + log_sigma + log(2 pi)/2 with q = (a - mu)^2 / sigma^2   (iql.py:527)
//   deterministic: (mu - a)^2                                                                     (iql.py:531)
__device__ __forceinline__ void pi_items8(const f32x4 (&hv)[8], const float (&acv)[8], const float (&wv)[8], bool live,
                                          bool gauss, float ivar, float ls, float invB, float (&dyv)[8], float (&dlv)[8],
                                          float& lossA) {
#pragma unroll
  for (int cc = 0; cc < 8; ++cc) {
    const float w = wv[cc];
    const float mu = tanh_via_exp(sum4(hv[cc]));
    const float diff = acv[cc] - mu;
    const float q = diff * diff * ivar;
    const float l_g = w * (0.5f * q + ls + 0.918938533204672742f);
    const float l_d = w * (diff * diff);
    const float dmu_g = (-(w * diff) * ivar) * invB;
    const float dmu_d = (-2.f * w * diff) * invB;
    const float dmu = gauss ? dmu_g : dmu_d;
    lossA += live ? (gauss ? l_g : l_d) : 0.f;
    dyv[cc] = live ? dmu * (1.f - mu * mu) : 0.f;
    dlv[cc] = (live && gauss) ? w * (1.f - q) : 0.f;
  }
}

// FULL: every row of every block's tile is a row of the batch (B % 256 == 0; the host selects the instantiation):
// no row index is clamped, so consecutive loads differ by compile-time constants.
#define BROW(r) (FULL ? (r) : min((r), B - 1))
// Kernel-argument PRELOAD (library built with -mllvm -amdgpu-kernarg-preload-count=14): the first 14 dwords of the
// explicit arguments arrive in SGPRs with the wave instead of through s_load from the freshly written argument block
// (measured 450-700 cycles until a field of the by-value StepParams is usable, 40 with preloading:
// profiles/r03_kernarg_latency_microbench.txt).  They are exactly what the block needs to ISSUE its first loads — the
// four scratch / batch pointers, the parameter arena (W2 and log_std addresses follow from the dims: arena_off below
// restates iqlhip_arena_layout) and the dims; everything else still comes from `p`, whose fetch now overlaps them.
//   q_dims = S | A << 8 | policy << 14      q_ldB = ld | rows << 10      q_mbc = max_batch | n_chunk << 16
//   q_rts  = n_rt | spb_l2 word << 10
template <bool BF16, bool FULL, bool MULTI>
__global__ __launch_bounds__(256) void iql_bwd_kernel(const float* q_heads, const float* q_xb, const float* q_h1, const float* q_h0,
                                                      const float* q_params, unsigned q_dims, unsigned q_ldB, unsigned q_mbc,
                                                      unsigned q_rts, StepParams p) {
  constexpr bool KPF = true;      // (the argument-line prefetch below reads this kernel's argument block)
  constexpr bool RW = false;      // (no per-row loss weights: iql_bwd_rw_kernel below is the form with them)
  const float* const rw_w = nullptr;
  float* const rw_td = nullptr;
#include "iqlhip_bwd_body.inc"
}
// RW = true (iqlhip_step_rw): the same body, fp32 only, with every row's loss terms and head gradients
// multiplied by rw_w[row] — one multiply per row, applied LAST to the finished unweighted value, so a weight of 1.0f
// reproduces the plain kernel's bits — and, when rw_td is given, the row's TD errors (q1 - y, q2 - y) stored to
// rw_td[row][2] by the chunk's Q1 loss block (one block per row, one 8-byte vector store per row).
// A kernel of its own rather than a fourth flag of iql_bwd_kernel: the plain instantiations keep their symbols, their
// argument block and their place in the code object, so plain calls launch exactly the kernels they always did.  The two
// extra arguments follow `p`; the argument-line prefetch is left out (KPF: its safety is checked per instantiation).
template <bool FULL, bool MULTI>
__global__ __launch_bounds__(256) void iql_bwd_rw_kernel(const float* q_heads, const float* q_xb, const float* q_h1, const float* q_h0,
                                                         const float* q_params, unsigned q_dims, unsigned q_ldB, unsigned q_mbc,
                                                         unsigned q_rts, StepParams p, const float* rw_w, float* rw_td) {
  constexpr bool BF16 = false;
  constexpr bool KPF = false;
  constexpr bool RW = true;
#include "iqlhip_bwd_body.inc"
}

// ---------------------------------------------------------------------------
// bf16 OPERAND IMAGES of W1 and W0 (bf16 path; read by the large-batch forward, iqlhip_lb_kernels.h): the weights in the
// order the MFMA consumes them, so that a wave's fragment load is 1 KB of consecutive memory (with row-major weights the
// 16 lanes of a group read 16 different rows: the CU's vector-memory pipe handles about one (lane group, cache line)
// pair per cycle, and the forward's 56 fragment loads per wave cost ~14 k cycles that way).
//   fragment (slab w = unit >> 6, tile ct = (unit >> 4) & 3, k-block kb = k >> 5): 64 lanes x 8 elements,
//   lane = (unit & 15) + 16 ((k >> 3) & 3), element = k & 7
// One image per net slot (V, Q1, Q2, pi, target Q1, target Q2): [W1: 65 536 | W0: 256 x 32 ceil(k_in / 32), zero beyond k_in].
#define IMG_W0_OFF 65536
#define IMG_STRIDE (65536 + 256 * 128)
__device__ __forceinline__ unsigned img_w1_off(int unit, int k) {
  return (unsigned)((((unit >> 6) * 4 + ((unit >> 4) & 3)) * 8 + (k >> 5)) * 512 + ((unit & 15) + 16 * ((k >> 3) & 3)) * 8 + (k & 7));
}
__device__ __forceinline__ unsigned img_w0_off(int unit, int k, int nkb) {
  return (unsigned)(IMG_W0_OFF + (((unit >> 6) * 4 + ((unit >> 4) & 3)) * nkb + (k >> 5)) * 512 + ((unit & 15) + 16 * ((k >> 3) & 3)) * 8 + (k & 7));
}
// the four arena elements e .. e + 3 of a net (w1 / w0 offsets and k_in given) -> its image, if they are W1 or W0 elements
__device__ __forceinline__ void img_store4(__bf16* img, long long e, long long w1, long long w0, int k_in, const f32x4 v) {
  if (e >= w1 && e < w1 + 65536) {
    const int idx = (int)(e - w1);
    bf16x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (__bf16)v[i];
    *(bf16x4*)(img + img_w1_off(idx >> 8, idx & 255)) = r;
  } else if (e >= w0 && e < w0 + 256 * k_in) {
    const int nkb = (k_in + 31) >> 5;
    // (row / column of element idx of the [256][k_in] matrix without an integer division: idx < 2^15, so the rounded
    //  quotient is at most one off — fixed up by the remainder's sign)
    const float inv_k = __builtin_amdgcn_rcpf((float)k_in);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = (int)(e - w0) + i;
      int unit = (int)((float)idx * inv_k);
      int k = idx - unit * k_in;
      if (k < 0) { unit -= 1; k += k_in; }
      if (k >= k_in) { unit += 1; k -= k_in; }
      img[img_w0_off(unit, k, nkb)] = (__bf16)v[i];
    }
  }
}

// ---------------------------------------------------------------------------
// Gradient assembly + Adam + Polyak.  Element e (float4 granularity) of the flat arena.
struct UpdParams {
  iqlhip_layout L;
  iqlhip_step_scalars sc;
  float tau, one_minus_tau;
  float* params;
  float* target;
  float* m;
  float* v;
  const float* slab_a;
  const float* slab_b;
  long long slab_b_off[4];
  const float* flat_grads;  // when non-null: gradient already summed (DP path), n_params + 4 words
  // direct-read exchange (xGMI peer-to-peer): n_peer > 0 -> the gradient is the sum, in rank order, of the n_peer flat
  // buffers peer_flat[0..n_peer) (this rank's own buffer included; the others are IPC-mapped peer memory, read with
  // system-scope loads).  Every rank forms the same sum in the same order: replicas stay bitwise equal.
  const float* peer_flat[IQLHIP_MAX_WORLD];
  int n_peer;
  // peer_direct: no flatten kernel ran — peer_flat[r] IS rank r's chunk slab (the backward wrote w1 / b1 / w2 / b2 /
  // log_std gradients straight into the exchange block; batches of <= 256 rows have ONE chunk slab, i.e. the gradient
  // itself), the w0 / b0 gradients are still per-row-tile partial slabs in peer_slab_b[r] (summed here, slab order
  // then rank order) and the loss sums are in peer_loss[r] ([4][64] like DevScratch::loss_parts)
  int peer_direct;
  const float* peer_slab_b[IQLHIP_MAX_WORLD];
  const float* peer_loss[IQLHIP_MAX_WORLD];
  float* loss_parts;
  float* losses;            // [4]
  float* losses_mirror;     // nullable: second copy of the three losses (host-mapped pinned words: iqlhip_online_step)
  float* loss_ring;         // nullable
  int ring_slot;
  int n_chunk, n_rt;        // chunk slabs (slab_a) and row-tile slabs (slab_b) the backward wrote
  int n_loss;               // entries of loss_parts per loss: 256-row chunks of the batch (large-batch backward: its row blocks)
  // large-batch backward (iqlhip_lb_kernels.h; LB instantiations only): slab_a holds the row-contraction products (w1, w0, b0,
  // the policy's w2; n_chunk chunk-group slabs), slab_x the row blocks' partial sums of everything else (b1, scalar w2, b2,
  // log_std; n_x slabs) — both laid out like the arena
  const float* slab_x;
  int n_x;
  int batch_rows;
  const iqlhip_step_scalars* sched;  // when non-null the scalars of this launch are sched[sched_idx]
  int sched_idx;                     // (hipGraph replay: kernel arguments are frozen, the table is not)
  // chunk replay: the loss-ring slot of this launch is ring_slot + ring_hdr[HDR_BASE] (the chunk's first step inside
  // the call; a captured chunk is replayed at different positions of the ring); null = ring_slot as given
  const unsigned long long* ring_hdr;
  // the LAST update of a chunk moves the chunk header on by the chunk's adv_k steps of adv_rows rows (thread 0 of
  // block 0, the only reader of the header in this kernel — every other reader belongs to an earlier or later
  // kernel), so the next chunk of the call starts without a host-side launch in between; null elsewhere
  unsigned long long* adv_hdr;
  int adv_k, adv_rows;
  // eager steps that return the losses to the host: after the three loss words have been written to losses_mirror
  // (host-mapped pinned memory) this host-mapped word receives done_val (release, system scope) — the host spins on it
  // instead of calling a HIP synchronise (measured 12-17 us of host time after the GPU has finished).  Everything else
  // a caller can observe of the step is ordered by the stream as before.  Null elsewhere.
  unsigned long long* done_flag;
  unsigned long long done_val;
  // bf16 path: bf16 shadows of the parameter and target arenas (same element offsets), written next to the fp32
  // masters so that the following forward / backward read their W1 fragments at half the bytes; null on the fp32 path
  __bf16* wsh;
  __bf16* tsh;
  __bf16* wimg;             // bf16 path: operand images [6][IMG_STRIDE] (slots V, Q1, Q2, pi, target Q1, target Q2); nullable
};

__device__ __forceinline__ int net_of(const iqlhip_layout& L, long long e) {
  int n = 0;
#pragma unroll
  for (int i = 1; i < 4; ++i) if (e >= L.net[i].seg_begin) n = i;
  return n;
}

// The layout words of a lane's net, WITHOUT indexing the kernel-argument block by the lane's net: `u.L.net[net]` with a
// per-lane index is a vector load from the argument block — a memory round trip that the gradient loads then wait for
// (they need these words for their address), i.e. a second dependent round trip in a kernel that otherwise has one.
// All four nets' words are uniform scalar loads; the lane selects.
struct NetWords { long long w0, b0; int k_in; long long slab_b_off; };
__device__ __forceinline__ NetWords net_words(const UpdParams& u, int net) {
  NetWords r;
  r.w0 = u.L.net[0].w0; r.b0 = u.L.net[0].b0; r.k_in = u.L.net[0].k_in; r.slab_b_off = u.slab_b_off[0];
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    const bool is = (net == i);
    r.w0 = is ? u.L.net[i].w0 : r.w0;
    r.b0 = is ? u.L.net[i].b0 : r.b0;
    r.k_in = is ? u.L.net[i].k_in : r.k_in;
    r.slab_b_off = is ? u.slab_b_off[i] : r.slab_b_off;
  }
  return r;
}

template <bool LB = false>
__device__ __forceinline__ f32x4 slab_grad(const UpdParams& u, long long e, int net) {
  const NetWords nl = net_words(u, net);
  f32x4 gsum = (f32x4){0.f, 0.f, 0.f, 0.f};
  // slabs are read 8 at a time with unconditional (clamped) loads: a load inside a runtime-count loop
  // would be waited for individually — one dependent round trip per slab.
  const float* base;
  long long stride;
  int n;
  if (LB) {
    // [w1 | w0 | b0 | b1 | w2 | b2 | log_std]: the row contractions (w1, w0, the policy's w2) come from the chunk-group
    // slabs, every plain sum over rows (the rest) from the row blocks' slabs
    const long long w2b = nl.b0 + 2 * HID, b2b = w2b + (long long)HID * ((net == IQLHIP_NET_PI) ? u.L.net[IQLHIP_NET_PI].d_out : 1);
    // (the row blocks' slabs have been summed into chunk-group slab 0 by iql_bwd_gemm_kernel's reduction jobs)
    const bool in_x = (e >= nl.b0) && !(net == IQLHIP_NET_PI && e >= w2b && e < b2b);
    stride = u.L.n_params;
    base = u.slab_a + e;
    n = in_x ? 1 : u.n_chunk;
  } else if (e >= nl.w0 && e < nl.b0 + HID) {
    stride = (long long)HID * nl.k_in + HID;
    base = u.slab_b + nl.slab_b_off + (e - nl.w0);
    n = u.n_rt;
  } else {
    stride = u.L.n_params;
    base = u.slab_a + e;
    n = u.n_chunk;
  }
  if (n == 1) return *(const f32x4*)base;
  for (int r0 = 0; r0 < n; r0 += 8) {
    f32x4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = *(const f32x4*)(base + (long long)min(r0 + j, n - 1) * stride);
#pragma unroll
    for (int j = 0; j < 8; ++j) if (r0 + j < n) gsum += v[j];
  }
  return gsum;
}

__device__ __forceinline__ void loss_words(const UpdParams& u, float out[4]) {
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < u.n_loss; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += u.loss_parts[k * 64 + c];
  out[0] = s[0];   // sum_r w u^2
  out[1] = s[1];   // sum_r e1^2
  out[2] = s[2];   // sum_r e2^2
  out[3] = s[3];   // sum_r w bc
}

// `hdr` (nullable): device words {size, seed, offset, step0}: a captured graph is replayed with new values.
__global__ __launch_bounds__(256) void iql_dropmask_kernel(unsigned* bits, int n_words, unsigned thresh,
                                                           unsigned long long seed, unsigned long long step,
                                                           const unsigned long long* hdr, int k) {
  if (hdr) { seed = hdr[HDR_DROP_SEED]; step = hdr[HDR_DROP_STEP] + (unsigned long long)k; }
  dropmask_words(bits, n_words, thresh, seed, step, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// First launch of an iqlhip_train_steps call (the only one that is not part of a chunk): block 0 publishes the call's
// header words; all blocks copy the call's scalar table from the library's pinned, host-mapped slot (read over PCIe,
// n_steps x 48 B) into its device copy, and — unless the previous call left them staged (B == 0) — gather the rows
// of the call's step 0 (indices drawn on the spot from the by-value header) and draw its dropout keep-bits.
// The block that finishes last acknowledges the table read in a host-mapped word (`ack`): the host reuses the pinned
// slot once it sees the call's number there — no event record in the stream, no HIP call on the host to test it.
// (call_setup_head: the header, the table and the acknowledgement — shared with the two-source form below)
__device__ __forceinline__ void call_setup_head(unsigned long long* hdr, const ChunkHdr& h, iqlhip_step_scalars* sched_call,
                                                const iqlhip_step_scalars* sched_src, int n_steps, unsigned* arrivals,
                                                unsigned long long* ack, unsigned long long ack_val) {
  if (blockIdx.x == 0 && threadIdx.x < HDR_WORDS) hdr[threadIdx.x] = h.w[threadIdx.x];
  const f32x4* s = (const f32x4*)sched_src;
  f32x4* d = (f32x4*)sched_call;
  const int n4 = n_steps * (int)(sizeof(iqlhip_step_scalars) / sizeof(f32x4));
  for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < n4; i += (int)gridDim.x * 256) d[i] = s[i];
  // (a thread's stores carry the data its loads returned: once every thread of every block is past this point the
  //  pinned slot has been read completely)
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned prev = __hip_atomic_fetch_add(arrivals, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev + 1u == gridDim.x) {
      __hip_atomic_store(arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ack, ack_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}
__global__ __launch_bounds__(256) void iql_call_setup_kernel(unsigned long long* hdr, ChunkHdr h,
                                                             iqlhip_step_scalars* sched_call,
                                                             const iqlhip_step_scalars* sched_src, int n_steps,
                                                             const float* rows, long long ld, float* xb, int B,
                                                             unsigned* drop_dst, int drop_words, unsigned drop_thresh,
                                                             unsigned* arrivals, unsigned long long* ack,
                                                             unsigned long long ack_val) {
  call_setup_head(hdr, h, sched_call, sched_src, n_steps, arrivals, ack, ack_val);
  if (B > 0)
    gather_rows_drawn(rows, ld, xb, B, h.w[HDR_SEED], h.w[HDR_OFFSET], h.w[HDR_POS], h.w[HDR_SIZE],
                      (int)blockIdx.x * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
  if (drop_dst)
    dropmask_words(drop_dst, drop_words, drop_thresh, h.w[HDR_DROP_SEED], h.w[HDR_DROP_STEP],
                   ((int)gridDim.x - 1 - (int)blockIdx.x) * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
}
// (its two-source form, iql_call_setup_mixed_kernel, is defined with the other kernels of mixed calls: end of iqlhip.hip)
__global__ __launch_bounds__(256) void iql_call_setup_mixed_kernel(unsigned long long* hdr, ChunkHdr h,
                                                                   iqlhip_step_scalars* sched_call,
                                                                   const iqlhip_step_scalars* sched_src, int n_steps,
                                                                   const float* rows, long long ld, float* xb, int B,
                                                                   unsigned* drop_dst, int drop_words, unsigned drop_thresh,
                                                                   unsigned* arrivals, unsigned long long* ack,
                                                                   unsigned long long ack_val, const float* rows_on,
                                                                   int n_off);
// (and its weighted form: iqlhip_weighted_kernels.h, included there too)
__global__ __launch_bounds__(256) void iql_call_setup_weighted_kernel(unsigned long long* hdr, ChunkHdr h,
                                                                      iqlhip_step_scalars* sched_call,
                                                                      const iqlhip_step_scalars* sched_src, int n_steps,
                                                                      const float* rows, long long ld, float* xb, int B,
                                                                      unsigned* drop_dst, int drop_words, unsigned drop_thresh,
                                                                      unsigned* arrivals, unsigned long long* ack,
                                                                      unsigned long long ack_val, WTab wt);
// (and the weighted form that stages the rows' q and publishes the call's beta: iqlhip_isweight_kernels.h)
__global__ __launch_bounds__(256) void iql_call_setup_weighted_is_kernel(unsigned long long* hdr, ChunkHdr h,
                                                                         iqlhip_step_scalars* sched_call,
                                                                         const iqlhip_step_scalars* sched_src, int n_steps,
                                                                         const float* rows, long long ld, float* xb, int B,
                                                                         unsigned* drop_dst, int drop_words, unsigned drop_thresh,
                                                                         unsigned* arrivals, unsigned long long* ack,
                                                                         unsigned long long ack_val, WTab wt, float* q_dst,
                                                                         float* beta_dev, float beta);
// (and the prioritised form that stages the rows' indices too and publishes alpha and eps: iqlhip_prio_kernels.h)
__global__ __launch_bounds__(256) void iql_call_setup_prio_kernel(unsigned long long* hdr, ChunkHdr h,
                                                                  iqlhip_step_scalars* sched_call,
                                                                  const iqlhip_step_scalars* sched_src, int n_steps,
                                                                  const float* rows, long long ld, float* xb, int B,
                                                                  unsigned* drop_dst, int drop_words, unsigned drop_thresh,
                                                                  unsigned* arrivals, unsigned long long* ack,
                                                                  unsigned long long ack_val, WTab wt, float* q_dst,
                                                                  float* beta_dev, float beta, long long* idx_dst,
                                                                  float* prio_words, float alpha, float eps, unsigned live);

// bf16 shadows rebuilt from the fp32 masters (start of every library call on the bf16 path: the caller owns the
// masters and may have written them through its own tensors since the last update kernel ran).
__global__ __launch_bounds__(256) void iql_shadow_refresh_kernel(const float* params, const float* target, __bf16* wsh,
                                                                 __bf16* tsh, long long n_params, long long n_target,
                                                                 iqlhip_layout L, __bf16* wimg) {
  const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e < n_params) {
    const f32x4 v = *(const f32x4*)(params + e);
    st4<true>((float*)wsh, (unsigned)e, v);
    if (wimg) {
      const int net = net_of(L, e);
      img_store4(wimg + (size_t)net * IMG_STRIDE, e, L.net[net].w1, L.net[net].w0, L.net[net].k_in, v);
    }
  }
  if (e < n_target) {
    const f32x4 v = *(const f32x4*)(target + e);
    st4<true>((float*)tsh, (unsigned)e, v);
    if (wimg) {
      const long long ea = e + L.target_src;       // the element's offset in the parameter arena: nets 1 (Q1), 2 (Q2)
      const int net = net_of(L, ea);
      img_store4(wimg + (size_t)(3 + net) * IMG_STRIDE, ea, L.net[net].w1, L.net[net].w0, L.net[net].k_in, v);
    }
  }
}

// Diagnostic (tools/gpu_call_overhead.py): a host-mapped word that says "everything queued before me has run".
__global__ void iql_debug_flag_kernel(unsigned long long* flag, unsigned long long v) {
  __hip_atomic_store(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(256) void iql_gather_kernel(const float* rows, long long ld, const long long* idx,
                                                         float* xb, int n, long long n_rows) {
  gather_rows_flat(rows, ld, idx, xb, n, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256, n_rows);
}
// The same with the indices read straight from a pinned, host-mapped slot (ReplayBuffer.sample: no H2D copy, no
// event): every block first parks the indices of ITS rows in LDS, then the block that finishes last acknowledges the
// slot in a host-mapped word — the host reuses the slot once it sees the call's number there (cf. iql_call_setup_kernel).
// (n_rows: an index outside [0, n_rows) — the host checks them before the launch; this only guards a reused pinned slot —
//  is never dereferenced: its row is filled with NaN, as in gather_rows_flat)
__global__ __launch_bounds__(256) void iql_gather_hostidx_kernel(const float* rows, long long ld, const long long* idx_host,
                                                                 float* xb, int n, long long n_rows, unsigned* arrivals,
                                                                 unsigned long long* ack, unsigned long long ack_val) {
  __shared__ long long s_idx[260];
  const int q = (int)(ld >> 2);
  const int e0 = (int)blockIdx.x * 256;
  const int r_first = e0 / q;
  const int r_last = min((e0 + 255) / q, n - 1);
  if ((int)threadIdx.x <= r_last - r_first) s_idx[threadIdx.x] = idx_host[r_first + threadIdx.x];
  __syncthreads();                       // (the slot's words this block needs have been read)
  if (threadIdx.x == 0) {
    const unsigned prev = __hip_atomic_fetch_add(arrivals, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev + 1u == gridDim.x) {
      __hip_atomic_store(arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ack, ack_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  const int e = e0 + (int)threadIdx.x;
  if (e < n * q) {
    const int r = e / q, c4 = e - r * q;
    const long long i = s_idx[r - r_first];
    f32x4 v;
    if (i < 0 || i >= n_rows) {
      const float nanv = __builtin_nanf("");
      v = (f32x4){nanv, nanv, nanv, nanv};
    } else {
      v = *(const f32x4*)(rows + i * ld + 4 * c4);
    }
    *(f32x4*)(xb + (long long)r * ld + 4 * c4) = v;
  }
}

// 16-byte accesses at SYSTEM scope (sc0 sc1): the load misses every cache level that is not coherent with another
// device's writes (IPC-mapped peer memory over xGMI), the store is written through to memory.  There is no 16-byte
// atomic, so these are the instructions the memory model uses for system-scope relaxed accesses, issued by hand.
// (load and wait are ONE asm statement: the compiler does not know that the load completes asynchronously and would
//  otherwise be free to copy the destination registers before a separate s_waitcnt has run)
__device__ __forceinline__ f32x4 load16_sys(const float* p) {
  f32x4 v;
  asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(p) : "memory");
  return v;
}
// eight such loads in flight together (one fabric round trip), then one wait
__device__ __forceinline__ void load16_sys_x8(f32x4 (&v)[8], const float* const (&p)[8]) {
  asm volatile(
      "global_load_dwordx4 %0, %8, off sc0 sc1\n\t"
      "global_load_dwordx4 %1, %9, off sc0 sc1\n\t"
      "global_load_dwordx4 %2, %10, off sc0 sc1\n\t"
      "global_load_dwordx4 %3, %11, off sc0 sc1\n\t"
      "global_load_dwordx4 %4, %12, off sc0 sc1\n\t"
      "global_load_dwordx4 %5, %13, off sc0 sc1\n\t"
      "global_load_dwordx4 %6, %14, off sc0 sc1\n\t"
      "global_load_dwordx4 %7, %15, off sc0 sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
      : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]), "v"(p[6]), "v"(p[7])
      : "memory");
}
__device__ __forceinline__ void store16_sys(float* p, f32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void wait_vm0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Direct-read gradient exchange between the ranks of one node (one process per GPU, buffers mapped with hipIpc):
// after its flatten kernel (whose stores are complete at the kernel boundary) rank r stores the step number into ITS
// slot of every peer's flag block, then waits until every peer's slot of its OWN flag block has reached that number;
// the update kernel that follows reads all ranks' flat gradients.  Buffers alternate by step parity: rank r rewrites
// buffer b two steps later, i.e. after it has seen every peer's signal of the step in between, which a peer only
// sends after its own update (its reads of buffer b) has finished.
// The wait is bounded: a peer that never arrives (crashed rank) makes the lane give up after `timeout_ticks` of the
// 100 MHz wall clock, record the step in status[0] (sticky: later waits return at once) and let the stream drain —
// the host reports it (iqlhip_xch_status), the grid never hangs.
struct XchParams {
  unsigned long long* peer_flags[IQLHIP_MAX_WORLD];   // base of every rank's flag block [world][16] (own = local)
  unsigned long long* status;                          // [0] first timed-out step (0 = none), [1] polls (diagnostic)
  const unsigned long long* hdr;                       // HDR_XSTEP: steps exchanged before this chunk (chunk replay) ...
  unsigned long long xstep;                            // ... or, hdr == null, the same number as a kernel argument
  unsigned long long timeout_ticks;
  int rank, world;
};
__global__ __launch_bounds__(64) void iql_xch_signal_wait_kernel(XchParams x, int k) {
  const int t = threadIdx.x;
  const unsigned long long v = (x.hdr ? x.hdr[HDR_XSTEP] : x.xstep) + (unsigned long long)k + 1ull;
  if (t < x.world && t != x.rank) {
    // release at system scope, drained, THEN the flag (the explicit wait: hipcc may drop the one that belongs to the
    // fence when its own scoreboard is empty, and the flag must not overtake the write-back)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    wait_vm0();
    __hip_atomic_store(x.peer_flags[t] + 16 * x.rank, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const unsigned long long* mine = x.peer_flags[x.rank] + 16 * t;
    if (__hip_atomic_load(x.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull) {
      const unsigned long long t0 = wall_clock64();
      unsigned long long polls = 0;
      while (__hip_atomic_load(mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < v) {
        __builtin_amdgcn_s_sleep(4);
        if (((++polls) & 63ull) == 0ull && wall_clock64() - t0 > x.timeout_ticks) {
          __hip_atomic_store(x.status, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
      }
    }
  }
}

// Writes the summed flat gradient (+ tail: value, q, actor loss contributions, spare) for the DP exchange.
// SYS: write-through system-scope stores (the buffer is read by peer GPUs).
template <bool SYS, bool LB = false>
__global__ __launch_bounds__(256) void iql_grad_flatten_kernel(UpdParams u, float* out) {
  const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e < u.L.n_params) {
    const int net = net_of(u.L, e);
    const f32x4 gv = slab_grad<LB>(u, e, net);
    if (SYS) store16_sys(out + e, gv);
    else *(f32x4*)(out + e) = gv;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float s[4];
    loss_words(u, s);
    const float ib = u.sc.inv_batch;
    const f32x4 tail = (f32x4){s[0] * ib, (s[1] * ib + s[2] * ib) * 0.5f, s[3] * ib, 0.f};
    if (SYS) store16_sys(out + u.L.n_params, tail);
    else *(f32x4*)(out + u.L.n_params) = tail;
  }
}

// FROM_TABLE: the per-step scalars come from the device table u.sched[u.sched_idx] (hipGraph replay: kernel
// arguments are frozen, the table is not); otherwise from the kernel argument u.sc.  Two instantiations
// rather than a run-time pointer select, which would turn every access into a flat load.
// PEER: the direct-read exchange variant (gradient = rank-ordered sum over UpdParams::peer_flat).
// Leading arguments (14 dwords, PRELOADED into SGPRs with the wave, cf. iql_bwd_kernel): the three state arenas, the chunk
// slab, the four segment starts and the end of the last segment as 32-bit element offsets, and q_flags: bit 0 = "the W1
// gradient of an element is the single word slab_a[e]" (one chunk slab, no exchange, not the large-batch form).  A block
// issues its m / v / p loads — and, for the 91 % of the elements that are W1, the gradient load — ~40 cycles after it starts
// instead of behind the ~600-cycle fetch of the by-value UpdParams, which now runs under those loads' latency.
#define UPD_EARLY_G 1u
template <bool FROM_TABLE, bool PEER, bool LB = false>
__global__ __launch_bounds__(256) void iql_update_kernel(float* q_p, float* q_m, float* q_v, const float* q_slab_a, unsigned q_s0,
                                                         unsigned q_s1, unsigned q_s2, unsigned q_s3, unsigned q_end,
                                                         unsigned q_flags, UpdParams u) {
  constexpr int step = 0;         // (row of the scalar table / loss ring: group launches pass theirs)
  constexpr bool CLIP = false;
  const float* const q_clip = nullptr;
#include "iqlhip_upd_body.inc"
}
// CLIP = true (iqlhip_set_grad_clip): the same body with the gradient additionally multiplied by the
// optimizer group's clip coefficient q_clip[grp], which iql_clip_coef_kernel wrote in the launch before.  A kernel of
// its own rather than a run-time argument of iql_update_kernel: the instantiations above keep their argument block and
// their code.  q_clip follows the 14 preloaded dwords (it shares their 64-byte line of the argument block).  Only the
// plain gradient source exists in this form: clipping is refused with an exchange and on the large-batch path.
template <bool FROM_TABLE>
__global__ __launch_bounds__(256) void iql_update_clip_kernel(float* q_p, float* q_m, float* q_v, const float* q_slab_a, unsigned q_s0,
                                                              unsigned q_s1, unsigned q_s2, unsigned q_s3, unsigned q_end,
                                                              unsigned q_flags, const float* q_clip, UpdParams u) {
  constexpr int step = 0;
  constexpr bool PEER = false, LB = false, CLIP = true;
#include "iqlhip_upd_body.inc"
}

// ---------------------------------------------------------------------------
// Trainer groups (iqlhip_group_*): K agents of identical dims stepped together, one launch per kernel for all of them.
// The host writes one record per agent into device memory — exactly what the single-agent launches pass as kernel
// arguments — and the group kernels run the bodies the single-agent kernels include (iqlhip_*_body.inc) on record
// blockIdx.y.  Nothing of an agent is shared with another: each record points at that agent's own arenas, scratch and
// staging buffer.  The members' batches may differ in rows (the _mixed entry points): grid.x of every launch is the
// largest member's block count, and a record bounds its own member's work — the forward by p.rows (ROW_EXIT), the
// backward by q_ldB / q_mbc / q_rts, the gathers and keep-bit draws by B / n_rows, the update by u's chunk count.
struct GroupRec {
  StepParams p;                       // forward + backward (spb_l2: the forward's slices per block for the group grid)
  const float* q_heads; const float* q_xb; const float* q_h1; const float* q_h0; const float* q_params;
  unsigned q_dims, q_ldB, q_mbc, q_rts;   // the backward's leading arguments (iql_bwd_kernel)
  UpdParams u;                        // update (FROM_TABLE: u.sched = the agent's scalar table of the call)
  float* u_p; float* u_m; float* u_v; const float* u_slab_a;
  unsigned u_s0, u_s1, u_s2, u_s3, u_end, u_flags;   // the update's leading arguments (iql_update_kernel)
  // device-drawn batches (iqlhip_group_train_steps): index j of the call = Philox counter offset + j / 2 under `seed`
  // over [0, size), exactly iqlhip_train_steps' stream; step s of the call gathers j = s * B + r, r < B, into xb
  const float* rows;
  long long ld, size;
  unsigned long long seed, offset;
  float* xb;
  int B;
  int n_steps;                        // steps of the call: bounds every index derived from a launch's step argument
  // two-source batches (iqlhip_group_train_steps_replay2; read by the iql_gather2_*group kernels alone, null / 0 in every
  // other call): `rows` / `size` are the offline buffer, batch rows r >= n_off are drawn over [0, size_on) from rows_on
  const float* rows_on;
  long long size_on;
  int n_off;
};

template <bool BF16, bool W0DMA, bool MULTI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void iql_fwd_group_kernel(const GroupRec* __restrict__ recs) {
  constexpr bool ONE = false;
  constexpr bool ROW_EXIT = true;       // (grid.x: the member with the most row tiles — the others' extra blocks exit)
  constexpr bool MIXED_IDLE = false;
  const StepParams& p = recs[blockIdx.y].p;
  FWD_NOT_EARLY();
#include "iqlhip_fwd_body.inc"
}

// (one-slice (b) blocks only: the multi-slice form spills SGPRs once its arguments come from a record; the slice count
//  does not change results, and a group grid has blocks enough without it)
template <bool BF16, bool FULL>
__global__ __launch_bounds__(256) void iql_bwd_group_kernel(const GroupRec* __restrict__ recs) {
  constexpr bool MULTI = false;
  constexpr bool KPF = false;     // (arguments in a device record, not in the kernel-argument block)
  constexpr bool RW = false;      // (per-row loss weights: solo steps only)
  const float* const rw_w = nullptr;
  float* const rw_td = nullptr;
  const GroupRec& r = recs[blockIdx.y];
  const float* q_heads = r.q_heads; const float* q_xb = r.q_xb; const float* q_h1 = r.q_h1; const float* q_h0 = r.q_h0;
  const float* q_params = r.q_params;
  const unsigned q_dims = r.q_dims, q_ldB = r.q_ldB, q_mbc = r.q_mbc, q_rts = r.q_rts;
  const StepParams& p = r.p;
#include "iqlhip_bwd_body.inc"
}

__global__ __launch_bounds__(256) void iql_update_group_kernel(const GroupRec* __restrict__ recs, int step) {
  constexpr bool FROM_TABLE = true, PEER = false, LB = false;
  const GroupRec& r = recs[blockIdx.y];
  float* q_p = r.u_p; float* q_m = r.u_m; float* q_v = r.u_v; const float* q_slab_a = r.u_slab_a;
  const unsigned q_s0 = r.u_s0, q_s1 = r.u_s1, q_s2 = r.u_s2, q_s3 = r.u_s3, q_end = r.u_end, q_flags = r.u_flags;
  const UpdParams& u = r.u;
  step = min(max(step, 0), r.n_steps - 1);
  constexpr bool CLIP = false;
  const float* const q_clip = nullptr;
#include "iqlhip_upd_body.inc"
}

// Step `step` of a group call: every agent draws its B indices and gathers its rows into its own staging buffer
// (grid.y = agent; the same draw as iql_call_setup_kernel / idle_block_work of a single agent's call).
__global__ __launch_bounds__(256) void iql_gather_group_kernel(const GroupRec* __restrict__ recs, int step) {
  const GroupRec& r = recs[blockIdx.y];
  const int s = min(max(step, 0), r.n_steps - 1);
  gather_rows_drawn(r.rows, r.ld, r.xb, r.B, r.seed, r.offset, (unsigned long long)s * (unsigned long long)r.B,
                    (unsigned long long)r.size, (int)blockIdx.x * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
}

// Actor dropout in a group (IQLHIP_GROUP_DROPOUT): one record per member, an array of its own next to the GroupRecs.
// A member's keep-bits are the ones its solo calls draw — dropmask_words under (seed, step) with the member's
// threshold — into parity 0 of its own buffer: a group's launches are stream-ordered, so step s + 1's draw cannot
// overtake step s's backward.  Only the words a step reads are drawn: rows < n_rows of each of the two layers.
struct GroupDropRec {
  unsigned* bits;                     // the member's keep-bits [2 layers][max_batch][8]
  int n_rows;                         // rows of the call's batches
  int max_batch;                      // rows per layer of `bits`
  unsigned thresh;                    // drop_thresh(p)
  int active;                         // 0: nothing to draw (rate 0, or masks written by iqlhip_debug_write_masks)
  unsigned long long seed, step0;     // the member's stream: key, and its position at the call's step 0
};
__device__ __forceinline__ void group_drop_words(const GroupDropRec& d, unsigned long long step, int first, int stride) {
  const int per = d.n_rows * 8;
  for (int v = first; v < 2 * per; v += stride) {
    const int w = (v < per) ? v : d.max_batch * 8 + (v - per);
    dropmask_words(d.bits, w + 1, d.thresh, d.seed, step, w, w + 1);      // (word w alone)
  }
}

// iql_dropmask_kernel for every drawing member of an eager or online group call (grid.y = record; the host packs the
// drawing members' records to the front): one launch where K solo steps pay K.
__global__ __launch_bounds__(256) void iql_dropmask_group_kernel(const GroupDropRec* __restrict__ drops) {
  const GroupDropRec& d = drops[blockIdx.y];
  group_drop_words(d, d.step0, (int)blockIdx.x * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
}

// iql_gather_group_kernel plus the step's keep-bits of the members that draw some (drops[member]), in the same launch:
// the gather occupies the first blocks, the keep-bit words are taken from the far end of the grid (idle_block_work's
// split).  Launched instead of iql_gather_group_kernel only when some member of the call draws.
__global__ __launch_bounds__(256) void iql_gather_drop_group_kernel(const GroupRec* __restrict__ recs,
                                                                    const GroupDropRec* __restrict__ drops, int step) {
  const GroupRec& r = recs[blockIdx.y];
  const int s = min(max(step, 0), r.n_steps - 1);
  gather_rows_drawn(r.rows, r.ld, r.xb, r.B, r.seed, r.offset, (unsigned long long)s * (unsigned long long)r.B,
                    (unsigned long long)r.size, (int)blockIdx.x * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
  const GroupDropRec& d = drops[blockIdx.y];
  if (d.active)
    group_drop_words(d, d.step0 + (unsigned long long)s, ((int)gridDim.x - 1 - (int)blockIdx.x) * 256 + (int)threadIdx.x,
                     (int)gridDim.x * 256);
}

// ---------------------------------------------------------------------------
// Per-step training statistics (iqlhip_set_step_stats, opt-in): IQLHIP_N_STATS floats that describe the
// batch a step trained on under the parameters before its update — 13 row statistics from the head partials the forward
// left in `heads` and the batch's r / d columns, and the L2 norms of the three optimizer groups' gradients from the
// slabs the backward left.  Two launches between a step's backward and its update kernel (the backward is the last
// reader of `heads`, the update the last reader of the slabs, and — in a chunk — the kernel that moves the header word
// the ring slot is formed from); both only read step state and write only the statistics scratch / ring.
//   1. iql_stats_gradsq_kernel  block (net = blockIdx.x & 3, window w = blockIdx.x >> 2): the sum of squares of the
//      net's gradient elements [seg_begin + 1024 w, + 1024) — the elements exactly as Adam receives them (slab_grad's
//      sum, times grad_scale when that is not 1) — to gparts[net][w].
//      Accumulation structure: a thread adds its 4 squares, 64 lanes combine by 6 xor-shuffles, 4 waves through LDS
//      (block_sum_256): ONE fp32 value stands for at most m = 1024 terms, each of which passes through 11 additions.
//   2. iql_step_stats_kernel    ONE block per agent: threads walk rows t, t + 256, ... in row order, combine like
//      block_sum_256 (shuffles, then the four waves in fixed order); waves 0..2 then add the gparts of their optimizer
//      group (V | Q1, Q2 | pi) in double — lane l takes partials l, l + 64, ..., then 6 xor-shuffles — and write the
//      square roots.  No atomics, no inter-block order: the result depends on the inputs alone.
struct StatsArgs {
  const float* heads;                 // DevScratch::heads of the step
  const float* xb;                    // the packed batch the step trained on
  int ld, rows, rd_off;               // row stride, rows, column of r (d follows): 2 S + A
  float beta, discount, exp_adv_max;
  float* gparts;                      // [4 nets][n_part] sums of squares (written by launch 1, read by launch 2)
  int n_part;                         // 1024-element windows of the longest net segment
  float* last;                        // [IQLHIP_N_STATS] the last step's statistics
  float* ring;                        // nullable: [ring_cap][IQLHIP_N_STATS], slot = ring_slot + step + ring_hdr[HDR_BASE]
  int ring_slot, ring_cap;
  const unsigned long long* ring_hdr; // nullable (chunk replay, cf. UpdParams::ring_hdr)
};

template <class T, class Op>
__device__ __forceinline__ T block_reduce_256(T v, T* red /*>=4*/, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return op(op(red[0], red[1]), op(red[2], red[3]));
}

__device__ __forceinline__ void stats_gradsq_block(const UpdParams& u, int step, float* gparts, int n_part, float* red) {
  const int net = (int)(blockIdx.x & 3u), w = (int)(blockIdx.x >> 2);
  if (w >= n_part) return;                                      // (block-uniform)
  const long long seg_b = u.L.net[net].seg_begin, seg_e = u.L.net[net].seg_end;
  const long long e = seg_b + (long long)w * 1024 + 4 * (long long)threadIdx.x;
  float ss = 0.f;
  if (e < seg_e) {
    const f32x4 gr = slab_grad<false>(u, e, net);
    const float gs = u.sched ? u.sched[u.sched_idx + step].grad_scale : u.sc.grad_scale;
    float g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = (gs == 1.f) ? gr[k] : gr[k] * gs;      // (iqlhip_upd_body.inc's gk)
    // (products and sums spelled out as separately rounded operations: the solo and the group kernel must agree bit for bit)
    ss = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(g[0], g[0]), __fmul_rn(g[1], g[1])), __fmul_rn(g[2], g[2])), __fmul_rn(g[3], g[3]));
  }
  ss = block_sum_256(ss, red);
  if (threadIdx.x == 0) gparts[net * n_part + w] = ss;
}

__device__ __forceinline__ void step_stats_block(const StatsArgs& a, int step, float* red, float* outs /*16*/) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float s[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) s[k] = 0.f;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  int n_pos = 0, n_clamp = 0;
  for (int row = tid; row < a.rows; row += 256) {
    const unsigned o = (unsigned)row * (unsigned)HEAD_LD;
    f32x4 h[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) h[i] = *(const f32x4*)(a.heads + (o + 4u * i));
    const unsigned ox = (unsigned)row * (unsigned)a.ld + (unsigned)a.rd_off;
    const float r = a.xb[ox], d = a.xb[ox + 1u];
    // head = sum4 of the four slice partials, as row_finish forms it
    const float nv = sum4(h[0]), v = sum4(h[1]), q1 = sum4(h[4]), q2 = sum4(h[5]);
    const float tq = fminf(sum4(h[2]), sum4(h[3]));
    const float adv = tq - v;                                   // row_finish's u
    const float y = fmaf((1.f - d) * a.discount, nv, r);      // (one rounding; spelled out: the solo and the group kernel agree)
    const float ex = expf(a.beta * adv);
    s[0] += v; s[1] += nv; s[2] += q1; s[3] += q2; s[4] += tq; s[5] += y; s[6] += fabsf(q1 - q2); s[7] += adv;
    s[8] += fminf(ex, a.exp_adv_max);
    mn = fminf(mn, adv);
    mx = fmaxf(mx, adv);
    n_pos += (adv < 0.f) ? 0 : 1;                               // the side row_finish's weight takes (u < 0 is the other)
    n_clamp += (ex >= a.exp_adv_max) ? 1 : 0;
  }
  const float nrows = (float)a.rows;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float t = block_sum_256(s[k], red);
    if (tid == 0) outs[(k < 8) ? k : 11] = t / nrows;
  }
  mn = block_reduce_256(mn, red, [](float x, float y) { return fminf(x, y); });
  mx = block_reduce_256(mx, red, [](float x, float y) { return fmaxf(x, y); });
  int* const redi = (int*)red;
  n_pos = block_reduce_256(n_pos, redi, [](int x, int y) { return x + y; });
  n_clamp = block_reduce_256(n_clamp, redi, [](int x, int y) { return x + y; });
  if (tid == 0) {
    outs[8] = mn;
    outs[9] = mx;
    outs[10] = (float)n_pos / nrows;
    outs[12] = (float)n_clamp / nrows;
  }
  // gradient norms: wave g adds optimizer group g's block partials in double, fixed order
  if (wave < 3) {
    const int first = (wave == 0) ? 0 : ((wave == 1) ? a.n_part : 3 * a.n_part);
    const int cnt = (wave == 1) ? 2 * a.n_part : a.n_part;
    double acc = 0.0;
    for (int i = lane; i < cnt; i += 64) acc += (double)a.gparts[first + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) outs[13 + wave] = (float)sqrt(acc);
  }
  __syncthreads();
  if (tid < IQLHIP_N_STATS) {
    const float val = outs[tid];
    a.last[tid] = val;
    if (a.ring) {
      const long long slot = (long long)a.ring_slot + step + (a.ring_hdr ? (long long)a.ring_hdr[HDR_BASE] : 0ll);
      if (slot >= 0 && slot < (long long)a.ring_cap) a.ring[IQLHIP_N_STATS * slot + tid] = val;
    }
  }
}

__global__ __launch_bounds__(256) void iql_stats_gradsq_kernel(UpdParams u, float* gparts, int n_part) {
  __shared__ float red[4];
  stats_gradsq_block(u, 0, gparts, n_part, red);
}
__global__ __launch_bounds__(256) void iql_step_stats_kernel(StatsArgs a) {
  __shared__ float red[4];
  __shared__ float outs[IQLHIP_N_STATS];
  step_stats_block(a, 0, red, outs);
}

// Group forms (grid.y = member): a member that has not enabled statistics has enabled = 0 and its blocks exit; the
// others run the solo bodies on their own records — bit-identical to their solo statistics.
struct GroupStatsRec { StatsArgs a; int enabled; };
__global__ __launch_bounds__(256) void iql_stats_gradsq_group_kernel(const GroupRec* __restrict__ recs,
                                                                     const GroupStatsRec* __restrict__ srecs, int step) {
  __shared__ float red[4];
  const GroupStatsRec& s = srecs[blockIdx.y];
  if (!s.enabled) return;
  const GroupRec& r = recs[blockIdx.y];
  stats_gradsq_block(r.u, min(max(step, 0), r.n_steps - 1), s.a.gparts, s.a.n_part, red);
}
__global__ __launch_bounds__(256) void iql_step_stats_group_kernel(const GroupRec* __restrict__ recs,
                                                                   const GroupStatsRec* __restrict__ srecs, int step) {
  __shared__ float red[4];
  __shared__ float outs[IQLHIP_N_STATS];
  const GroupStatsRec& s = srecs[blockIdx.y];
  if (!s.enabled) return;
  step_stats_block(s.a, min(max(step, 0), recs[blockIdx.y].n_steps - 1), red, outs);
}

// ---------------------------------------------------------------------------
// Gradient-norm clipping per optimizer group (iqlhip_set_grad_clip, opt-in): torch's clip_grad_norm_
// (L2, error_if_nonfinite = False) for the groups V | Q1 + Q2 | pi (+ log_std).  Launches of a step:
//   backward -> iql_stats_gradsq_kernel (the block partials, shared with the statistics) -> [iql_step_stats_kernel]
//            -> iql_clip_coef_kernel -> iql_update_clip_kernel
// iql_clip_coef_kernel: ONE block; wave g adds group g's partials in double in step_stats_block's order (lane l takes
// partials l, l + 64, ..., then 6 xor-shuffles), rounds the square root to fp32 — the value statistics 13..15 hold —
// and lane 0 writes
//   coef = min(max_norm / (norm + 1e-6f), 1.0f)       (fp32, one addition, one division; NaN stays NaN, as torch.clamp)
// or exactly 1.0f for a group without a limit (+inf in `limits`).  The limits are device memory of the context: a graph
// replay reads the current ones.  No atomics: the result depends on the inputs alone.
struct ClipArgs {
  const float* gparts;                // [4 nets][n_part] (iql_stats_gradsq_kernel)
  int n_part;
  const float* limits;                // [3] V, Q, pi: max_norm, +inf = no limit
  float* coef;                        // [3] written here, read by the update kernel of the same step
  float* norm;                        // [3] the norms before clipping
};
__device__ __forceinline__ void clip_coef_block(const ClipArgs& a) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (wave < 3) {
    const int first = (wave == 0) ? 0 : ((wave == 1) ? a.n_part : 3 * a.n_part);
    const int cnt = (wave == 1) ? 2 * a.n_part : a.n_part;
    double acc = 0.0;
    for (int i = lane; i < cnt; i += 64) acc += (double)a.gparts[first + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) {
      const float nrm = (float)sqrt(acc);
      const float mx = a.limits[wave];
      float cf = 1.f;
      if (mx < __builtin_inff()) {
        const float q = __fdiv_rn(mx, __fadd_rn(nrm, 1e-6f));
        cf = (q > 1.f) ? 1.f : q;
      }
      a.coef[wave] = cf;
      a.norm[wave] = nrm;
    }
  }
}
__global__ __launch_bounds__(256) void iql_clip_coef_kernel(ClipArgs a) { clip_coef_block(a); }

// Group forms (grid.y = member).  A member with clipping off has enabled = 0: its clip block exits at once, and
// coef_rd points at three floats of exactly 1.0f (the group's), so that the group update kernel — which picks the
// member at run time and therefore always multiplies — computes x * 1.0f = x, the bits of the CLIP = false form.
struct GroupClipRec { ClipArgs a; const float* coef_rd; int enabled; };
__global__ __launch_bounds__(256) void iql_clip_coef_group_kernel(const GroupClipRec* __restrict__ crecs) {
  const GroupClipRec& c = crecs[blockIdx.y];
  if (!c.enabled) return;
  clip_coef_block(c.a);
}
__global__ __launch_bounds__(256) void iql_update_clip_group_kernel(const GroupRec* __restrict__ recs,
                                                                    const GroupClipRec* __restrict__ crecs, int step) {
  constexpr bool FROM_TABLE = true, PEER = false, LB = false, CLIP = true;
  const GroupRec& r = recs[blockIdx.y];
  float* q_p = r.u_p; float* q_m = r.u_m; float* q_v = r.u_v; const float* q_slab_a = r.u_slab_a;
  const unsigned q_s0 = r.u_s0, q_s1 = r.u_s1, q_s2 = r.u_s2, q_s3 = r.u_s3, q_end = r.u_end, q_flags = r.u_flags;
  const float* const q_clip = crecs[blockIdx.y].coef_rd;
  const UpdParams& u = r.u;
  step = min(max(step, 0), r.n_steps - 1);
#include "iqlhip_upd_body.inc"
}

// Policy inference (GaussianPolicy.act / DeterministicPolicy.act, algorithms/finetune/iql.py:371-379, 404-413):
// states -> packed rows whose first S columns are the state (the rest zero), then iql_fwd_kernel with
// only_inst = 6, then this finish kernel over the policy head partials:
//   action = clamp(max_action * (tanh(pre) [+ exp(clamp(log_std)) * noise]), -max_action, +max_action)
__device__ __forceinline__ void pack_states(float* xb, int ld, int S, int n, const float* s, long long ld_s) {
  const int total = n * ld;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int i = e / ld;
    const int c = e - i * ld;
    xb[e] = (c < S) ? s[i * ld_s + c] : 0.f;
  }
}
__global__ void iql_pack_states_kernel(float* xb, int ld, int S, int n, const float* s, long long ld_s) {
  pack_states(xb, ld, S, n, s, ld_s);
}

// Actor dropout inside policy inference (iqlhip_set_act_dropout): the keep-bits of ONE inference call, a stream of
// its own — tag "ADRP", position = the context's act_drop_calls, stream word = row * 16 + layer * 8 + q (no buffer
// size in it) — drawn into the context's act_drop_bits [2 layers][cap][8], which only the inference forward reads
// (the training steps' drop_bits are never written here: a chunk graph has pre-drawn the next step's parity there).
// Only rows < n_rows are drawn, by the launch that packs the call's states: the packing takes the first blocks, the
// words come from the far end of the grid (idle_block_work's split).
struct ActDropRec {
  unsigned* bits;                     // the context's act_drop_bits
  int n_rows;                         // rows of the call
  int cap;                            // rows per layer of `bits` (the context's act capacity)
  unsigned thresh;                    // drop_thresh(p)
  int active;                         // 0: nothing to draw (rate 0)
  unsigned long long seed, call;      // key, and the call's position in the stream
};
__device__ __forceinline__ void act_drop_words(const ActDropRec& d, int first, int stride) {
  const int per = d.n_rows * 8;
  for (int v = first; v < 2 * per; v += stride) {
    const int layer = (v >= per) ? 1 : 0, rq = v - layer * per;       // rq = row * 8 + q
    const uint32_t w = (uint32_t)((rq >> 3) * 16 + layer * 8 + (rq & 7));
    d.bits[layer * d.cap * 8 + rq] = keep_word(w, 0x41445250u /* "ADRP" */, d.thresh, d.seed, d.call);
  }
}
// iql_pack_states_kernel plus the call's keep-bits (launched instead of it only when the context's inference rate
// is > 0; the grid has a thread per packed element and per keep-bit word)
__global__ __launch_bounds__(256) void iql_pack_states_drop_kernel(float* xb, int ld, int S, int n, const float* s,
                                                                   long long ld_s, ActDropRec d) {
  pack_states(xb, ld, S, n, s, ld_s);
  act_drop_words(d, ((int)gridDim.x - 1 - (int)blockIdx.x) * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
}

// noise: caller-supplied N(0,1) values, or — rng_seed != 0 — drawn here: Philox4x32-10 keyed by the seed, counter
// (element, call), Box-Muller on two of its words (the draw of dist.sample(), iql.py:376, without a host-side
// random-number launch per env step).
__device__ __forceinline__ void actor_finish_elem(const float* heads_pi, int e, int A, float max_action, const float* log_std,
                                                  float ls_min, float ls_max, const float* noise, long long ld_noise,
                                                  unsigned long long rng_seed, unsigned long long rng_call, float* out,
                                                  long long ld_out) {
  const int row = e / A, dd = e - row * A;
  const f32x4 hp = *(const f32x4*)(heads_pi + (long long)e * NSPLIT);
  float a = tanh_via_exp(((hp[0] + hp[1]) + hp[2]) + hp[3]);      // same fixed order as the training step (sum4)
  if (noise != nullptr || rng_seed != 0ull) {
    const float sigma = (log_std != nullptr) ? expf(fminf(fmaxf(log_std[dd], ls_min), ls_max)) : 0.f;
    float z;
    if (noise != nullptr) {
      z = noise[row * ld_noise + dd];
    } else {
      uint32_t c[4] = {(uint32_t)e, (uint32_t)rng_call, (uint32_t)(rng_call >> 32), 0xAC7u};
      philox4x32_10(c, (uint32_t)rng_seed, (uint32_t)(rng_seed >> 32));
      const float u1 = ((float)(c[0] >> 8) + 0.5f) * (1.f / 16777216.f);       // (0, 1)
      const float u2 = ((float)(c[1] >> 8) + 0.5f) * (1.f / 16777216.f);
      z = sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
    }
    a = a + sigma * z;
  }
  out[row * ld_out + dd] = fminf(fmaxf(a * max_action, -max_action), max_action);
}
// done_flag (nullable; one-block launches only): after every thread's store — ordered by the system-scope fence and
// the barrier — a host-mapped word receives done_val: the host of iqlhip_online_step spins on it instead of
// synchronising the stream.
__global__ void iql_actor_finish_kernel(const float* heads_pi, int n, int A, float max_action, const float* log_std,
                                        float ls_min, float ls_max, const float* noise, long long ld_noise,
                                        unsigned long long rng_seed, unsigned long long rng_call, float* out,
                                        long long ld_out, unsigned long long* done_flag, unsigned long long done_val) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n * A) actor_finish_elem(heads_pi, e, A, max_action, log_std, ls_min, ls_max, noise, ld_noise, rng_seed, rng_call, out, ld_out);
  if (done_flag) {
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(done_flag, done_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// Five row-major arrays (any strides) -> packed rows [s | a | s' | r | d | pad] of the staging batch.
__global__ void iql_pack_kernel(float* xb, int ld, int S, int A, int n, const float* s, long long ld_s, const float* a,
                                long long ld_a, const float* r, long long ld_r, const float* ns, long long ld_ns,
                                const float* d, long long ld_d) {
  const int total = n * ld;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int i = e / ld;
    const int c = e - i * ld;
    float v = 0.f;
    if (c < S) v = s[i * ld_s + c];
    else if (c < S + A) v = a[i * ld_a + (c - S)];
    else if (c < 2 * S + A) v = ns[i * ld_ns + (c - S - A)];
    else if (c == 2 * S + A) v = r[i * ld_r];
    else if (c == 2 * S + A + 1) v = d[i * ld_d];
    xb[e] = v;
  }
}

// ---------------------------------------------------------------------------
// Replay-buffer storage kernels.  Row layout: [s(S) | a(A) | s'(S) | r | d | pad].
__global__ void iql_rows_write_kernel(float* rows, long long ld, int S, int A, long long row0, long long n,
                                      const float* s, const float* a, const float* r, const float* ns,
                                      const float* d) {
  const int W = 2 * S + A + 2;
  const long long total = n * W;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long i = e / W;
    const int c = (int)(e - i * W);
    float v;
    if (c < S) v = s[i * S + c];
    else if (c < S + A) v = a[i * A + (c - S)];
    else if (c < 2 * S + A) v = ns[i * S + (c - S - A)];
    else if (c == 2 * S + A) v = r[i];
    else v = d[i];
    rows[(row0 + i) * ld + c] = v;
  }
}

__global__ void iql_rows_gather_kernel(const float* rows, long long ld, long long n_rows, int S, int A,
                                       const long long* idx, long long n, float* s, float* a, float* r, float* ns,
                                       float* d) {
  const int W = 2 * S + A + 2;
  const long long total = n * W;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long i = e / W;
    const int c = (int)(e - i * W);
    const long long ri = idx[i];
    const float v = (n_rows > 0 && (ri < 0 || ri >= n_rows)) ? __builtin_nanf("") : rows[ri * ld + c];     // (see gather_rows_flat)
    if (c < S) s[i * S + c] = v;
    else if (c < S + A) a[i * A + (c - S)] = v;
    else if (c < 2 * S + A) ns[i * S + (c - S - A)] = v;
    else if (c == 2 * S + A) r[i] = v;
    else d[i] = v;
  }
}

// Index draw: Philox4x32-10, counter = (offset + i/2), key = seed.
// idx[i] uniform over [0,size): 64 random bits, multiply-high (bias <= size / 2^64).
// `hdr` (nullable) = device words {size, seed, offset} so that a captured graph can be replayed
// with new values.
__global__ void iql_draw_indices_kernel(long long* idx, long long n, long long size, unsigned long long seed,
                                        unsigned long long offset, const unsigned long long* hdr) {
  if (hdr) { size = (long long)hdr[HDR_SIZE]; seed = hdr[HDR_SEED]; offset = hdr[HDR_OFFSET]; }
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n + 1) / 2;
       i += (long long)gridDim.x * blockDim.x) {
    const unsigned long long ctr = offset + (unsigned long long)i;
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0x49514C48u /* "IQLH" */, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const unsigned long long r0 = ((unsigned long long)c[1] << 32) | c[0];
    const unsigned long long r1 = ((unsigned long long)c[3] << 32) | c[2];
    idx[2 * i] = (long long)__umul64hi(r0, (unsigned long long)size);
    if (2 * i + 1 < n) idx[2 * i + 1] = (long long)__umul64hi(r1, (unsigned long long)size);
  }
}

// ---------------------------------------------------------------------------
// Synthetic D4RL-shaped rows generated where they will live (bench data, SURVEY §8d's distributions, not a parity
// fixture): obs, next_obs ~ N(0,1); actions ~ U(-1,1) * 0.999; rewards ~ N(0,1) (antmaze flavour: -1 with p = 0.98,
// else 0); dones ~ Bernoulli(p_done).  One Philox4x32-10 block per element (key = seed, counter = element number):
// Box-Muller on two words for the normals.  At configs[3]'s 10 M rows the host generator of jsrl-corl_amd/synth.py takes
// ~30 s per rank (and a 1.7 GB upload); this takes milliseconds and every rank produces identical rows.
__global__ void iql_rows_fill_synth_kernel(float* rows, long long ld, int S, int A, long long row0, long long n,
                                           unsigned long long seed, float p_done, int antmaze) {
  const int W = 2 * S + A + 2;
  const long long total = n * W;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long i = e / W;
    const int c = (int)(e - i * W);
    const unsigned long long ctr = (unsigned long long)(row0 + i) * (unsigned long long)W + (unsigned long long)c;
    uint32_t k[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0x46494C4Cu /* "FILL" */, 0u};
    philox4x32_10(k, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u1 = ((float)(k[0] >> 8) + 0.5f) * (1.f / 16777216.f);       // (0, 1)
    const float u2 = ((float)(k[1] >> 8) + 0.5f) * (1.f / 16777216.f);
    float v;
    if (c < S || (c >= S + A && c < 2 * S + A)) v = sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
    else if (c < S + A) v = (2.f * u1 - 1.f) * 0.999f;
    else if (c == 2 * S + A) v = antmaze ? ((u1 < 0.98f) ? -1.f : 0.f) : sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
    else v = (u1 < p_done) ? 1.f : 0.f;
    rows[(row0 + i) * ld + c] = v;
  }
}

// ---------------------------------------------------------------------------
// Dataset ingest: column mean / std of n rows (compute_mean_std, algorithms/finetune/iql.py:77-80:
// mean = x.mean(0), std = x.std(0) + eps, population variance) and the in-place normalisation of the state columns of
// packed rows (normalize_states, :83-84: (x - mean) / std in fp32, IEEE division).  Sums are kept in float64 and
// combined in a fixed order (block partials, then one thread per column): deterministic, and closer to the exact
// value than numpy's float32 row-after-row sums — the parity statement is therefore a tolerance against numpy
// (tests: rel <= 1e-6 against a float64 numpy evaluation, <= 1e-3 against numpy's own float32 result at 1 M rows).
#define MS_BLOCKS 512
// pass 0: partial[b][c] = sum over the block's rows of x[r][c];  pass 1: sum of (x - mean[c])^2
template <int PASS>
__global__ __launch_bounds__(256) void iql_cols_moment_kernel(const float* x, long long ld, int ncols, long long n,
                                                              const double* mean, double* partial) {
  __shared__ double red[8][33];
  const int c_lane = threadIdx.x & 31, r_lane = threadIdx.x >> 5;     // 8 rows x 32 columns per pass
  for (int c0 = 0; c0 < ncols; c0 += 32) {
    const int c = c0 + c_lane;
    double acc = 0.0;
    if (c < ncols) {
      const double mu = PASS ? mean[c] : 0.0;
      for (long long r = (long long)blockIdx.x * 8 + r_lane; r < n; r += (long long)gridDim.x * 8) {
        const double v = (double)x[r * ld + c];
        acc += PASS ? (v - mu) * (v - mu) : v;
      }
    }
    red[r_lane][c_lane] = acc;
    __syncthreads();
    if (r_lane == 0 && c < ncols) {
      double s = red[0][c_lane];
#pragma unroll
      for (int k = 1; k < 8; ++k) s += red[k][c_lane];
      partial[(long long)blockIdx.x * ncols + c] = s;
    }
    __syncthreads();
  }
}
// one thread per column: fixed-order sum of the block partials -> mean (pass 0) or std + eps (pass 1)
template <int PASS>
__global__ void iql_cols_finish_kernel(const double* partial, int nblocks, int ncols, long long n, float eps,
                                       double* mean64, float* out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncols) return;
  double s = 0.0;
  for (int b = 0; b < nblocks; ++b) s += partial[(long long)b * ncols + c];
  if (PASS == 0) {
    mean64[c] = s / (double)n;
    out[c] = (float)(s / (double)n);
  } else {
    out[c] = (float)sqrt(s / (double)n) + eps;       // np.std(float32 array) returns float32, then + eps in float32
  }
}

__global__ void iql_rows_normalize_kernel(float* rows, long long ld, int S, int A, long long row0, long long n,
                                          const float* mean, const float* stdv) {
  const long long total = n * 2 * S;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long i = e / (2 * S);
    const int c2 = (int)(e - i * 2 * S);
    const int c = (c2 < S) ? c2 : c2 - S;
    float* p = rows + (row0 + i) * ld + ((c2 < S) ? c : S + A + c);
    *p = (*p - mean[c]) / stdv[c];
  }
}

// ---------------------------------------------------------------------------
// Reward ingest: return_reward_range / modify_reward (algorithms/finetune/iql.py:262-289) on n packed rows from row0,
// in storage order.  Row i (0-based in the range) ends an episode iff d[i] != 0 or its episode has reached T rows.
// With p(i) = the largest j < i with d[j] != 0 (-1 if none) and o = i - p(i) - 1:  row i ends an episode iff
// d[i] != 0 || (o + 1) % T == 0, and that episode's first row is p(i) + 1 + (o / T) * T — no sequential pass.
//   1. iql_rr_scan_{reduce,partials,apply}_kernel: prev[i] = max over j <= i of (d[j] != 0 ? j : -1), an inclusive
//      prefix max in three plain launches (a partial per 256-row tile, one block scans the partials, every tile
//      rescans itself on top of its predecessor's partial).  No block ever waits for another one: a grid may exceed
//      what the device holds at once, and a block that spins on one that is not scheduled yet never ends.
//      p(i) = prev[i - 1], and d[i] != 0 iff prev[i] == i.
//   2. iql_rr_episode_kernel: one thread per row; the thread of a row that ends an episode adds that episode's
//      float32 rewards in float64, first row to last, one after the other — the reference's `ep_ret += float(r)`, so
//      the sums (and with them min / max) are the reference's Python floats bit for bit.  The loads are one float per
//      row stride: uncoalesced by construction, n of them in all.  (min, max, count) per block.
//   3. iql_rr_finish_kernel: one block folds the block partials (min / max / integer sum: order-independent).
// A return is never -0.0 (the sum starts at +0.0, and x + (-x) = +0.0), so `<` / `>` give Python's min / max; NaN
// rewards are outside the contract (Python's min / max depend on the order there).
// Tiles are walked with a block stride, so the grids stay bounded (RR_MAX_BLOCKS) for any n.
#define RR_TILE 256
#define RR_MAX_BLOCKS 4096
struct RRResult { double min_ret, max_ret; long long episodes; };

// inclusive prefix max over the block's 256 threads of values >= -1; s_w: 4 words of LDS, reusable on return
__device__ __forceinline__ long long rr_block_scan_max(long long v, long long* s_w) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const long long u = __shfl_up(v, off, 64);
    if (lane >= off && u > v) v = u;
  }
  if (lane == 63) s_w[w] = v;
  __syncthreads();
  for (int k = 0; k < w; ++k) if (s_w[k] > v) v = s_w[k];
  __syncthreads();
  return v;
}

__device__ __forceinline__ long long rr_terminal_or_minus1(const float* rows, long long ld, int dcol, long long row0,
                                                           long long n, long long i) {
  return (i < n && rows[(row0 + i) * ld + dcol] != 0.f) ? i : -1;
}

// partial[t] = the last terminal row of tile t (-1: none)
__global__ __launch_bounds__(RR_TILE) void iql_rr_scan_reduce_kernel(const float* rows, long long ld, int dcol, long long row0,
                                                                     long long n, long long ntiles, long long* partial) {
  __shared__ long long s_w[4];
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    long long v = rr_terminal_or_minus1(rows, ld, dcol, row0, n, t * RR_TILE + threadIdx.x);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const long long u = __shfl_xor(v, o, 64); if (u > v) v = u; }
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) partial[t] = max(max(s_w[0], s_w[1]), max(s_w[2], s_w[3]));
    __syncthreads();
  }
}

// one block: partial[t] <- max over tiles <= t (in place)
__global__ __launch_bounds__(RR_TILE) void iql_rr_scan_partials_kernel(long long* partial, long long ntiles) {
  __shared__ long long s_w[4];
  __shared__ long long s_carry;
  long long carry = -1;
  for (long long base = 0; base < ntiles; base += RR_TILE) {
    const long long t = base + threadIdx.x;
    long long v = rr_block_scan_max((t < ntiles) ? partial[t] : -1, s_w);
    if (carry > v) v = carry;
    if (t < ntiles) partial[t] = v;
    if (threadIdx.x == RR_TILE - 1) s_carry = v;
    __syncthreads();
    carry = s_carry;
    __syncthreads();
  }
}

// prev[i] = the last terminal row <= i of the whole range (-1: none)
__global__ __launch_bounds__(RR_TILE) void iql_rr_scan_apply_kernel(const float* rows, long long ld, int dcol, long long row0,
                                                                    long long n, long long ntiles, const long long* partial,
                                                                    long long* prev) {
  __shared__ long long s_w[4];
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long i = t * RR_TILE + threadIdx.x;
    long long v = rr_block_scan_max(rr_terminal_or_minus1(rows, ld, dcol, row0, n, i), s_w);
    const long long carry = t ? partial[t - 1] : -1;
    if (carry > v) v = carry;
    if (i < n) prev[i] = v;
  }
}

__device__ __forceinline__ void rr_fold(double& mn, double& mx, long long& cnt, double mn2, double mx2, long long cnt2) {
  if (mn2 < mn) mn = mn2;
  if (mx2 > mx) mx = mx2;
  cnt += cnt2;
}

// (min, max, count) of the block's 256 threads -> thread 0
__device__ __forceinline__ void rr_block_fold(double& mn, double& mx, long long& cnt, RRResult* s_w) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) rr_fold(mn, mx, cnt, __shfl_xor(mn, o, 64), __shfl_xor(mx, o, 64), __shfl_xor(cnt, o, 64));
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = RRResult{mn, mx, cnt};
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < 4; ++k) rr_fold(mn, mx, cnt, s_w[k].min_ret, s_w[k].max_ret, s_w[k].episodes);
}

__global__ __launch_bounds__(RR_TILE) void iql_rr_episode_kernel(const float* rows, long long ld, int rcol, long long row0,
                                                                 long long n, long long ntiles, long long T,
                                                                 const long long* prev, RRResult* partial) {
  __shared__ RRResult s_w[4];
  double mn = __builtin_inf(), mx = -__builtin_inf();
  long long cnt = 0;
  const float* r = rows + row0 * ld + rcol;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long i = t * RR_TILE + threadIdx.x;
    if (i >= n) continue;
    const long long p = i ? prev[i - 1] : -1;
    const long long o = i - p - 1;
    if (prev[i] != i && (o + 1) % T != 0) continue;
    double ret = 0.0;
    long long j = p + 1 + (o / T) * T;
    for (; j + 8 <= i + 1; j += 8) {       // eight loads in flight (each is a cache line of its own), added in row order
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = r[(j + k) * ld];
#pragma unroll
      for (int k = 0; k < 8; ++k) ret += (double)v[k];
    }
    for (; j <= i; ++j) ret += (double)r[j * ld];       // ascending, one after another
    rr_fold(mn, mx, cnt, ret, ret, 1);
  }
  rr_block_fold(mn, mx, cnt, s_w);
  if (threadIdx.x == 0) partial[blockIdx.x] = RRResult{mn, mx, cnt};
}

__global__ __launch_bounds__(RR_TILE) void iql_rr_finish_kernel(const RRResult* partial, int nblocks, RRResult* out) {
  __shared__ RRResult s_w[4];
  double mn = __builtin_inf(), mx = -__builtin_inf();
  long long cnt = 0;
  for (int b = threadIdx.x; b < nblocks; b += RR_TILE) rr_fold(mn, mx, cnt, partial[b].min_ret, partial[b].max_ret, partial[b].episodes);
  rr_block_fold(mn, mx, cnt, s_w);
  if (threadIdx.x == 0) *out = RRResult{mn, mx, cnt};
}

// modify_reward's arithmetic on the reward column, float32 like numpy's in-place operators on a float32 array:
// SHIFT = false: r = r / divide_by, then r = r * multiply_by (two roundings, IEEE division — `rewards /= max_ret - min_ret;
// rewards *= max_episode_steps`);  SHIFT = true: r = r - a (antmaze's `rewards -= 1.0`).
template <bool SHIFT>
__global__ void iql_rows_reward_map_kernel(float* rows, long long ld, int rcol, long long row0, long long n, float a, float b) {
#pragma clang fp contract(off)
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    float* p = rows + (row0 + i) * ld + rcol;
    if (SHIFT) {
      *p = *p - a;
    } else {
      const float q = *p / a;
      *p = q * b;
    }
  }
}

// ---------------------------------------------------------------------------
// One online iteration's buffer work in one launch (iqlhip_online_step): the new transition `row_host` (pinned,
// host-mapped, ld floats) is stored at ring row `pointer`, and the batch rows[idx_host[r]] (indices in pinned,
// host-mapped memory, exactly as np.random.randint drew them) are gathered into xb.  A sampled index equal to
// `pointer` reads the new row from `row_host` itself — the ring write of block 0 may not have happened yet.
__global__ __launch_bounds__(256) void iql_online_gather_kernel(float* rows, long long ld, long long pointer,
                                                                const float* row_host, const long long* idx_host,
                                                                float* xb, int n) {
  __shared__ long long s_idx[260];
  const int q = (int)(ld >> 2);
  const int e0 = (int)blockIdx.x * 256;
  const int r_first = e0 / q;
  const int r_last = min((e0 + 255) / q, n - 1);
  if ((int)threadIdx.x <= r_last - r_first) s_idx[threadIdx.x] = idx_host[r_first + threadIdx.x];
  if (blockIdx.x == 0 && (int)threadIdx.x < q)
    *(f32x4*)(rows + pointer * ld + 4 * threadIdx.x) = *(const f32x4*)(row_host + 4 * threadIdx.x);
  __syncthreads();
  const int e = e0 + (int)threadIdx.x;
  if (e < n * q) {
    const int r = e / q, c4 = e - r * q;
    const long long i = s_idx[r - r_first];
    const float* src = (i == pointer) ? row_host : rows + i * ld;
    *(f32x4*)(xb + (long long)r * ld + 4 * c4) = *(const f32x4*)(src + 4 * c4);
  }
}

// (iql_online_gather2_kernel, the form for a batch mixed from two buffers: end of iqlhip.hip)
__global__ __launch_bounds__(256) void iql_online_gather2_kernel(float* rows, const float* rows_off, long long ld,
                                                                 long long pointer, const float* row_host,
                                                                 const long long* idx_host, float* xb, int n_off, int n);

// ---------------------------------------------------------------------------
// Trainer-group online iteration (iqlhip_group_online_step): the kernels above that a solo iqlhip_online_step
// launches, in group form (grid.y = member), with their arguments in device records the host uploads once per call.
struct GroupOnlineRec {
  float* rows;                        // the member's ring (packed rows, stride ld)
  const float* row_pin;               // its new transition (pinned, host-mapped: the context's on_row_pin)
  const long long* idx_pin;           // its sampled indices (pinned, host-mapped: on_idx_pin)
  float* xb;                          // its staging batch
  const float* act_pin;               // its next-act state (pinned: on_act_pin) or NULL: no action requested
  float* xb_act;                      // its inference staging
  long long ld, pointer;
  int n, S;
  // two-source batches (iqlhip_group_online_step_replay2; read by the iql_online_gather2_*group kernels alone): batch rows
  // [0, n_off) are rows_off[idx_pin[r]] (the member's offline buffer, read only), rows [n_off, n) come from the ring
  const float* rows_off;
  int n_off;
};
// Per requesting member: the arguments iql_actor_finish_kernel takes (one row).
struct GroupActRec {
  const float* heads;                 // the member's heads_act (policy partials of its one row)
  const float* log_std;               // NULL: deterministic policy
  float* out;                         // pinned action words (on_act_pin + IQLHIP_MAX_INPUT)
  float max_action, ls_min, ls_max;
  unsigned long long seed, call;      // seed 0: the mean action
};

// iql_online_gather_kernel per member: the ring write, the gather from pinned indices (an index equal to `pointer`
// reads the new row from the pinned copy), and — members that asked for an action — the packing of the act state into
// xb_act that iql_pack_states_kernel does for one row (block 0).  Every member has the same ld; the grid is sized for
// the largest n (a block past a member's own n reads no index and writes no row).
__device__ __forceinline__ void online_gather_member(const GroupOnlineRec& g) {
  __shared__ long long s_idx[260];
  float* rows = g.rows;
  const float* row_host = g.row_pin;
  const long long ld = g.ld, pointer = g.pointer;
  const int n = g.n;
  const int q = (int)(ld >> 2);
  const int e0 = (int)blockIdx.x * 256;
  const int r_first = e0 / q;
  const int r_last = min((e0 + 255) / q, n - 1);
  if ((int)threadIdx.x <= r_last - r_first) s_idx[threadIdx.x] = g.idx_pin[r_first + threadIdx.x];
  if (blockIdx.x == 0) {
    for (int c4 = (int)threadIdx.x; c4 < q; c4 += 256)
      *(f32x4*)(rows + pointer * ld + 4 * c4) = *(const f32x4*)(row_host + 4 * c4);
    if (g.act_pin)
      for (int c = (int)threadIdx.x; c < (int)ld; c += 256) g.xb_act[c] = (c < g.S) ? g.act_pin[c] : 0.f;
  }
  __syncthreads();
  const int e = e0 + (int)threadIdx.x;
  if (e < n * q) {
    const int r = e / q, c4 = e - r * q;
    const long long i = s_idx[r - r_first];
    const float* src = (i == pointer) ? row_host : rows + i * ld;
    *(f32x4*)(g.xb + (long long)r * ld + 4 * c4) = *(const f32x4*)(src + 4 * c4);
  }
}
__global__ __launch_bounds__(256) void iql_online_gather_group_kernel(const GroupOnlineRec* __restrict__ recs) {
  online_gather_member(recs[blockIdx.y]);
}
// ... plus the keep-bits of the act forwards that run with dropout (drops[member]; launched instead of the kernel
// above only when some requesting member's inference rate is > 0): one row's 16 words, from the far end of the grid.
__global__ __launch_bounds__(256) void iql_online_gather_drop_group_kernel(const GroupOnlineRec* __restrict__ recs,
                                                                           const ActDropRec* __restrict__ drops) {
  online_gather_member(recs[blockIdx.y]);
  const ActDropRec& d = drops[blockIdx.y];
  if (d.active)
    act_drop_words(d, ((int)gridDim.x - 1 - (int)blockIdx.x) * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
}

// (the group forms of the two-source gathers — iqlhip_group_online_step_replay2 / iqlhip_group_train_steps_replay2 — are
//  defined with the other two-source kernels: end of iqlhip.hip)
__global__ __launch_bounds__(256) void iql_online_gather2_group_kernel(const GroupOnlineRec* __restrict__ recs);
__global__ __launch_bounds__(256) void iql_online_gather2_drop_group_kernel(const GroupOnlineRec* __restrict__ recs,
                                                                            const ActDropRec* __restrict__ drops);
__global__ __launch_bounds__(256) void iql_gather2_group_kernel(const GroupRec* __restrict__ recs, int step);
__global__ __launch_bounds__(256) void iql_gather2_drop_group_kernel(const GroupRec* __restrict__ recs,
                                                                     const GroupDropRec* __restrict__ drops, int step);

// Weighted replay sampling in a group (iqlhip_group_train_steps_weighted): one record per member, an array of its own
// next to the GroupRecs as GroupDropRec is — GroupRec is unchanged.  wt.tab == nullptr: the member draws uniformly.
// (the kernels are defined with the other weighted kernels: iqlhip_weighted_kernels.h, end of iqlhip.hip)
struct GroupWtRec {
  WTab wt;
};
__global__ __launch_bounds__(256) void iql_gather_weighted_group_kernel(const GroupRec* __restrict__ recs,
                                                                        const GroupWtRec* __restrict__ wts, int step);
__global__ __launch_bounds__(256) void iql_gather_weighted_drop_group_kernel(const GroupRec* __restrict__ recs,
                                                                             const GroupWtRec* __restrict__ wts,
                                                                             const GroupDropRec* __restrict__ drops, int step);

// The policy-inference forward (iql_fwd_kernel<BF16, W0DMA, false, true>: only_inst = 6, blockIdx.x = row tile *
// NSPLIT + column slice) for the members that asked for an action: grid.y = requesting member, ps[j] its StepParams.
template <bool BF16, bool W0DMA>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void iql_act_fwd_group_kernel(const StepParams* __restrict__ ps) {
  constexpr bool MULTI = false, ONE = true, ROW_EXIT = false;      // (blocks past a member's rows store nothing)
  constexpr bool MIXED_IDLE = false;
  const StepParams& p = ps[blockIdx.y];
  FWD_NOT_EARLY();
#include "iqlhip_fwd_body.inc"
}

// iql_actor_finish_kernel for one row of each of n_req members in one block (n_req * A <= 16 * 32), then the call's
// completion word: every member's losses (written by the update before this launch) and actions are in pinned memory.
__global__ __launch_bounds__(256) void iql_actor_finish_group_kernel(const GroupActRec* __restrict__ recs, int n_req, int A,
                                                                     unsigned long long* done_flag,
                                                                     unsigned long long done_val) {
  for (int e = (int)threadIdx.x; e < n_req * A; e += 256) {
    const int j = e / A, d = e - j * A;
    const GroupActRec& r = recs[j];
    actor_finish_elem(r.heads, d, A, r.max_action, r.log_std, r.ls_min, r.ls_max, nullptr, 0, r.seed, r.call, r.out, A);
  }
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(done_flag, done_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The completion word of a group online call without actions: launched behind the update, whose blocks have stored
// every member's losses in pinned memory by then (stream order).
__global__ void iql_group_done_kernel(unsigned long long* done_flag, unsigned long long done_val) {
  if (threadIdx.x == 0) __hip_atomic_store(done_flag, done_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---------------------------------------------------------------------------
// Trainer-group policy inference (iqlhip_group_actor_forward): iqlhip_actor_forward / iqlhip_actor_sample of every
// requesting member in one set of launches — pack, iql_act_fwd_group_kernel, finish — with grid.y = requesting member
// and each member's arguments in a device record the host uploads once per call.
struct GroupPackRec {                 // iql_pack_states_kernel's arguments
  float* xb;                          // the member's xb_act
  const float* s;                     // its states (device or host-mapped memory)
  long long ld_s;
  int ld, S, n;
};
struct GroupActRowsRec {              // iql_actor_finish_kernel's arguments (no caller noise: seed or the mean)
  const float* heads;                 // the member's heads_act
  const float* log_std;               // NULL: deterministic policy
  float* out;                         // its actions (device or host-mapped memory), row stride ld_out
  long long ld_out;
  int n, A;
  float max_action, ls_min, ls_max;
  unsigned long long seed, call;      // seed 0: the mean action
};

// iql_pack_states_kernel per member (grid.y): grid.x strides over the longest member's n * ld elements.
__global__ __launch_bounds__(256) void iql_pack_states_group_kernel(const GroupPackRec* __restrict__ recs) {
  const GroupPackRec& r = recs[blockIdx.y];
  pack_states(r.xb, r.ld, r.S, r.n, r.s, r.ld_s);
}
// ... plus the call's keep-bits of the requesting members whose inference rate is > 0 (drops[j] belongs to packs[j];
// launched instead of the kernel above only when there is such a member).
__global__ __launch_bounds__(256) void iql_pack_states_drop_group_kernel(const GroupPackRec* __restrict__ recs,
                                                                         const ActDropRec* __restrict__ drops) {
  const GroupPackRec& r = recs[blockIdx.y];
  pack_states(r.xb, r.ld, r.S, r.n, r.s, r.ld_s);
  const ActDropRec& d = drops[blockIdx.y];
  if (d.active)
    act_drop_words(d, ((int)gridDim.x - 1 - (int)blockIdx.x) * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
}

// iql_actor_finish_kernel per member (grid.y) over its n rows: element e = row * A + d, numbered as there, so the
// device noise of (seed, call) is the solo call's draw element for element.
__global__ __launch_bounds__(256) void iql_actor_finish_rows_group_kernel(const GroupActRowsRec* __restrict__ recs) {
  const GroupActRowsRec& r = recs[blockIdx.y];
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < r.n * r.A)
    actor_finish_elem(r.heads, e, r.A, r.max_action, r.log_std, r.ls_min, r.ls_max, nullptr, 0, r.seed, r.call, r.out, r.ld_out);
}

// ---------------------------------------------------------------------------
// The training forward of a two-source chunk (iqlhip_train_steps_mixed): iql_fwd_kernel's body instantiated a second
// time, with the idle blocks staging the next step's rows from two buffers (idle_block_work<true>).  A kernel of its
// own rather than a run-time test in iql_fwd_kernel: the forward of plain calls stays as it is, instruction for instruction.
template <bool BF16, bool W0DMA, bool MULTI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void iql_fwd_mixed_kernel(StepParams p) {
  constexpr bool ONE = false, ROW_EXIT = false, MIXED_IDLE = true;
  FWD_NOT_EARLY();
#include "iqlhip_fwd_body.inc"
}
