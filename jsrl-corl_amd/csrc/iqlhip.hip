// iqlhip.hip — C ABI (include/iqlhip.h) of the MI355X IQL step.  Host side:
// arena layout, scratch management, launches, hipGraph capture of K-step chunks.
#include "iqlhip_kernels.h"
#include "iqlhip_lb_kernels.h"
#include "iqlhip_owned.h"
#include "iqlhip_staging.h"

#include <dlfcn.h>

#include <time.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#define GRAPH_STEPS IQLHIP_GRAPH_STEPS
// Captured chunk sizes: a call of n steps is composed of replays of these (every step runs inside a graph).  The even
// sizes start and end on staging buffer 0, so they chain in any order; the one-step chunk only ever ends a call.
static const int kChunkSizes[] = {GRAPH_STEPS, 16, 4, 2, 1};

static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(IQLHIP_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

static inline int64_t up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// Buffer and event ownership (iqlhip_owned.h) on the HIP runtime.  A context and a trainer group each have one Owned:
// it is used at create time and when an opt-in feature is first enabled, never by a step.
struct HipApi {
  using err_t = hipError_t;
  using event_t = hipEvent_t;
  using stream_t = hipStream_t;
  static constexpr err_t ok = hipSuccess;
  static constexpr unsigned event_no_timing = hipEventDisableTiming;
  static err_t dev_alloc(void** p, size_t n) { return hipMalloc(p, n); }
  static err_t dev_fill(void* p, int byte, size_t n) { return hipMemset(p, byte, n); }
  static err_t dev_free(void* p) { return hipFree(p); }
  static err_t pin_alloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
  static err_t pin_free(void* p) { return hipHostFree(p); }
  static err_t event_create(event_t* e, unsigned flags) { return hipEventCreateWithFlags(e, flags); }
  static err_t event_destroy(event_t e) { return hipEventDestroy(e); }
  static err_t copy_to_dev(void* dst, const void* src, size_t n, stream_t st) { return hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st); }
  static err_t event_record(event_t e, stream_t st) { return hipEventRecord(e, st); }
  static err_t event_wait(event_t e) { return hipEventSynchronize(e); }
};
using Owned = OwnedT<HipApi>;
using Staging = StagingT<HipApi>;                // launch records: pinned block, device block, upload event (iqlhip_staging.h)
using CachedStaging = CachedStagingT<HipApi>;    // ... uploaded only when they differ from the last upload
extern "C" int64_t iqlhip_debug_live_buffers(void) { return Owned::live().load(std::memory_order_relaxed); }
// All of `allocate`'s allocations or none: on an error what it made is freed and its pointers are null again (the
// error message stays), so the caller's "already allocated" test, whichever pointer it looks at, is false again.
template <class F> static int all_or_nothing(Owned& own, F&& allocate) {
  const size_t mark = own.mark();
  const int rc = allocate();
  if (rc) own.rollback(mark);
  return rc;
}

// Runtime flags -> template arguments: with_bools(f, a, b, ...) calls f(std::bool_constant<a>{}, std::bool_constant<b>{}, ...).
// Every kernel family with bool template parameters has ONE selector built on it (flags -> instantiation), next to its
// launcher; the solo launch, the group launch and the hipFuncSetAttribute loop (set_max_lds) all go through that selector,
// so a family's instantiation list is written once.  The selectors also fix the ORDER in which the instantiations are
// emitted (first flag outermost, false before true, selector by selector down this file), and with it where each kernel
// lies in the code object; the step time is sensitive to that (profiles/r09_host_fold_host_ab.txt), so they keep the
// order the code object has always had — which is why the flags of a selector are not always in template order.
template <class F> static auto with_bools(F&& f) { return f(); }
template <class F, class... Bs> static auto with_bools(F&& f, bool b, Bs... rest) {
  if (!b) return with_bools([&](auto... t) { return f(std::false_type{}, t...); }, rest...);
  return with_bools([&](auto... t) { return f(std::true_type{}, t...); }, rest...);
}
static auto fwd_one_kernel(bool bf, bool dma) {      // policy inference (StepParams::only_inst): its own instantiations
  return with_bools([](auto BF, auto DMA) { return &iql_fwd_kernel<BF.value, DMA.value, false, true>; }, bf, dma);
}
static auto fwd_kernel(bool bf, bool dma, bool multi) {
  return with_bools([](auto MU, auto BF, auto DMA) { return &iql_fwd_kernel<BF.value, DMA.value, MU.value>; }, multi, bf, dma);
}
static auto bwd_kernel(bool bf, bool full, bool multi) {
  return with_bools([](auto MU, auto BF, auto FU) { return &iql_bwd_kernel<BF.value, FU.value, MU.value>; }, multi, bf, full);
}
// The row-weighted fp32 backward (iqlhip_step_rw).  Its selector is DEFINED at the end of this file: the instantiations are
// then emitted behind every other kernel, and everything that existed keeps its place in the code object (see above).
using BwdRwFn = void (*)(const float*, const float*, const float*, const float*, const float*, unsigned, unsigned, unsigned,
                         unsigned, StepParams, const float*, float*);
static BwdRwFn bwd_rw_kernel(bool full, bool multi);
static auto bwd_rows_kernel(bool csplit) {
  return with_bools([](auto CS) { return &iql_bwd_rows_kernel<CS.value>; }, csplit);
}
// Allow `lds` bytes of dynamic LDS in every instantiation of a family: sel(m) = its selector called with bit i of m as flag i.
template <class Sel> static int set_max_lds(int n_flags, size_t lds, Sel sel) {
  for (unsigned m = 0; m < (1u << n_flags); ++m)
    HIPCHK(hipFuncSetAttribute((const void*)sel(m), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return IQLHIP_OK;
}

// Diagnostic (IQLHIP_TRACE=1): host timestamps inside iqlhip_train_steps, printed to stderr at the end of the call.
static inline double now_us() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}
static const bool g_trace = getenv("IQLHIP_TRACE") != nullptr;

// Host-side index check of the entry points that see the indices: the reference's `self._states[indices]` raises
// IndexError for an index outside the tensor (iql.py:173-177); here that is IQLHIP_EINDEX before anything is launched.
static int check_host_indices(const int64_t* idx_host, int64_t n, int64_t n_rows) {
  for (int64_t i = 0; i < n; ++i)
    if (idx_host[i] < 0 || idx_host[i] >= n_rows)
      return fail(IQLHIP_EINDEX, "index %lld is out of bounds for dimension 0 with size %lld", (long long)idx_host[i], (long long)n_rows);
  return IQLHIP_OK;
}

// Make the context's GPU the current HIP device for the duration of an entry point and restore the caller's
// afterwards (a trainer on cuda:1 may be driven while cuda:0 is current; the library must not change that).
struct DevGuard {
  int prev = -1;
  bool switched = false;
  explicit DevGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = (hipSetDevice(dev) == hipSuccess);
  }
  ~DevGuard() { if (switched) (void)hipSetDevice(prev); }
};

// What the table update inside a prioritised chunk needs of its updatable table beyond WTab (the launches' WUpd).
// q_max: the maximum word of a tracking table (iqlhip_weights_build_tracking), else null — the update launches of a chunk
// graph are captured as the tracking instantiations or as the plain ones, so it is part of what identifies the graph.
struct PrioSrc { unsigned* stamp = nullptr; unsigned* flags = nullptr; unsigned long long* delta = nullptr; int sh0 = 0;
                 unsigned sat_bits = 0; unsigned long long* q_max = nullptr; };
// The five kinds of chunk graph, one per pair of entry points (iqlhip_train_steps, _mixed, _weighted, _weighted_is,
// _prioritized).  The values are the kernels' too: idle_block_work<MODE> of a kind's forward is numbered the same way.
// What a kind implies for the driver stands in ONE place: kind_info(), in front of the multi-step driver.
enum class ChunkKind : int { Plain = 0, Mixed = 1, Weighted = 2, WeightedIs = 3, Prio = 4 };
constexpr int N_CHUNK_KINDS = 5;
// What a chunk graph of a kind freezes beyond a plain chunk's: part of its key.  Mixed (GraphKey::rows = the offline
// buffer): the online buffer and the batch rows that are not its; the three weighted kinds: the table the idle blocks
// draw by; Prio: what the update launches behind every step are captured with.
struct ChunkSrc {
  ChunkKind kind = ChunkKind::Plain;
  const float* rows_on = nullptr; int32_t n_off = 0; WTab wt{nullptr, 0u, 0}; PrioSrc up;
  bool operator==(const ChunkSrc& o) const {
    return kind == o.kind && rows_on == o.rows_on && n_off == o.n_off && wt.tab == o.wt.tab && wt.n == o.wt.n &&
           wt.levels == o.wt.levels && wt.local == o.wt.local && up.stamp == o.up.stamp && up.flags == o.up.flags &&
           up.delta == o.up.delta && up.sh0 == o.up.sh0 && up.sat_bits == o.up.sat_bits && up.q_max == o.up.q_max;
  }
};
// ... and the values of ONE call, which the set-up kernel writes to device words and no graph freezes: the table's
// generation and content version (what a following call must name to start on the rows this one staged:
// iqlhip_weights_update moves the version), the importance-sampling exponent, the priority's alpha and eps, and live
// (0: a rehearsal, whose update launches leave the table alone).  A mixed call's online size travels in the header
// (HDR_SIZE_ON).  Named constructors: mixed_call, weighted_call, prio_call; ChunkCall() is a plain call.
struct ChunkCall { ChunkSrc src; uint64_t wt_gen = 0, wt_ver = 0; float is_beta = 0.f, alpha = 0.f, eps = 0.f; unsigned live = 1u; };
// What a captured chunk graph depends on through frozen kernel arguments.  The number of steps of a call is NOT part
// of it: a call is composed of replays of the fixed chunk graphs (64, 16, 4, 2 steps and one), nothing is ever
// captured per call length (kernel boundaries inside a graph are ~0.5 us shorter than between directly launched kernels).
struct GraphKey {
  const float* rows = nullptr;
  int64_t ld = 0;
  int32_t B = 0;
  int32_t K = 0;      // steps in the chunk: one of kChunkSizes, never the caller's step count
  float* params = nullptr;
  float drop_p = 0.f;
  float inv_batch = 0.f;
  int xch = 0;        // exchange mode the chunk was captured with
  int parity = 0;     // P2P exchange: which flat buffer step 0 of the chunk writes
  int head = 0;       // the chunk a call starts with: its graph begins with the call's set-up kernel (arguments set per replay)
  int stats = 0;      // captured with the statistics launches (iqlhip_set_step_stats): never replayed under the other setting
  int clip = 0;       // captured with the clip launches and the CLIP update kernel (iqlhip_set_grad_clip): likewise
  ChunkSrc src;       // the chunk's kind and what it freezes: a chunk of one kind is never replayed for a call of another
  bool operator==(const GraphKey& o) const {
    return src == o.src && rows == o.rows && ld == o.ld && B == o.B && K == o.K && params == o.params && drop_p == o.drop_p &&
           inv_batch == o.inv_batch && xch == o.xch && parity == o.parity && head == o.head && stats == o.stats && clip == o.clip;
  }
};

// The few RCCL entry points the in-stream all-reduce needs, resolved at run time from the librccl.so.1 the process
// already has (PyTorch-ROCm brings one) or can load — the library has no link-time dependency on RCCL.
struct RcclId { char internal[IQLHIP_UNIQUE_ID_BYTES]; };
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, RcclId /* ncclUniqueId, by value */, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};

struct iqlhip_ctx {
  iqlhip_dims dims;
  iqlhip_hyper hyper;
  iqlhip_layout L;
  int device = 0;
  Owned own;                          // every buffer and event below that the library allocates, except where noted
  // bound (caller-owned)
  float *params = nullptr, *target = nullptr, *m = nullptr, *v = nullptr;
  // scratch (library-owned)
  DevScratch sc{};
  float* flat_tmp = nullptr;          // n_params + 4 (debug "grads")
  float* xb = nullptr;                // compact batch [max_batch][row_ld]: rows [s | a | s' | r | d | pad]
  // iqlhip_actor_forward's own staging (never aliases a training batch): packed states and policy head partials
  float* xb2 = nullptr;               // second staging batch: graph chunks alternate (step k reads one, gathers k+1 into the other)
  float* xb_act = nullptr;            // [act_cap][row_ld]
  float* heads_act = nullptr;         // [act_cap][A][NSPLIT]
  float* losses_host = nullptr;       // pinned landing pad of read_losses (a pageable D2H goes through a bounce copy)
  float* on_row_pin = nullptr;        // iqlhip_online_step: pinned, host-mapped staging of the new transition [row_ld]
  long long* on_idx_pin = nullptr;    // ... and of the sampled indices [max_batch]
  float* on_loss_pin = nullptr;       // ... and the landing words of the step's three losses [4]
  unsigned long long* done_pin = nullptr;   // host-mapped completion word of the synchronous entry points (the host spins on it)
  unsigned long long done_seq = 0;
  float* on_act_pin = nullptr;        // ... and of the follow-up act(): state in [IQLHIP_MAX_INPUT], action out [IQLHIP_MAX_ACTION]
  int act_cap = 0;
  unsigned long long act_calls = 0;   // Philox call counter of iqlhip_actor_sample
  int64_t row_ld = 0;
  // actor dropout
  unsigned* drop_bits = nullptr;      // [2 parities][2 layers][max_batch][8] keep-bits (a step reads one parity while the
                                      // forward's idle blocks draw the next step's into the other)
  float drop_p = 0.f;
  unsigned long long drop_seed = 0, drop_step = 0;
  bool drop_inject = false;           // tests: masks were written by iqlhip_debug_write_masks, do not regenerate
  // actor dropout inside policy inference (iqlhip_set_act_dropout): a rate, key, position and buffer of its own
  unsigned* act_drop_bits = nullptr;  // [2 layers][act_cap][8] keep-bits of the last inference call that drew (allocated
                                      // by the first iqlhip_set_act_dropout with p > 0)
  float act_drop_p = 0.f;
  unsigned long long act_drop_seed = 0, act_drop_calls = 0;
  int precision = 0;                  // 0: fp32 MFMA everywhere; 1: bf16 operands for the layer-0/1, dW1, dH0, dW0 products
  __bf16* wsh = nullptr;              // bf16 path: shadow of the parameter arena [n_params] (W1 is read from it) ...
  __bf16* tsh = nullptr;              // ... and of the target arena [n_target]; written by the update kernel, refreshed
                                      // from the fp32 masters at the start of every library call
  float* loss_ring = nullptr;         // [ring_cap][4], host-mapped pinned
  int ring_cap = 0;
  iqlhip_step_scalars* sched_cur = nullptr;   // [GRAPH_STEPS] device: per-step scalars of the chunk in flight
  iqlhip_step_scalars* sched_call = nullptr;  // [k_max] device copy of the scalar table of the call in flight
  iqlhip_step_scalars* sched_pin[4] = {nullptr, nullptr, nullptr, nullptr};  // pinned, host-mapped copies of a call's table [k_max]
  // a slot is free again once the set-up kernel that read it has acknowledged the call's number in sched_ack[slot]
  // (a pinned, host-mapped word the kernel writes; the host only reads memory — no event, no HIP call)
  unsigned long long* sched_ack = nullptr;      // pinned [4]
  unsigned long long sched_want[4] = {0, 0, 0, 0};
  unsigned long long call_seq = 0;
  unsigned* setup_arrivals = nullptr;           // device: block counter of iql_call_setup_kernel
  // the forward instantiations of a chunk kind have their dynamic-LDS limit (ensure_fwd_lds; Plain: at creation)
  bool fwd_lds_set[N_CHUNK_KINDS] = {false, false, false, false, false};
  // weighted calls with importance-sampling weights: [2][max_batch] staged q of the two staging parities, [max_batch] c of
  // the running step, the call's beta (one allocation, made by the first such call; addresses frozen in chunk graphs)
  float* is_buf = nullptr;
  // prioritised calls: [2][max_batch] int64 staged indices of the two staging parities, [max_batch][2] fp32 TD errors of
  // the running step, the call's alpha, eps and live word (one allocation, made by the first such call; frozen in graphs)
  char* prio_buf = nullptr;
  char* prep_save = nullptr;                    // device: prepare's copy of the four arenas, kept (freeing it at the end of prepare
                                                //   idles the GPU right in front of the caller's first steps)
  hipStream_t sched_stream[4] = {nullptr, nullptr, nullptr, nullptr};   // (the stream a slot's reader was queued on)
  int sched_slot = 0;
  unsigned long long* hdr = nullptr;  // [HDR_WORDS] per-launch values of a chunk (ChunkHdr)
  unsigned long long* stamps = nullptr;  // diagnostic builds (-DIQL_STAMPS): [4096 blocks][16]
  int k_max = 0;
  int n_chunk_max = 0, n_rt_max = 0;
  size_t lds_fwd = 0, lds_fwd_solo = 0, lds_bwd = 0;
  int n_cus = 256;                    // compute units of the device (MI355X: 256)
  int w0_lds_k = 0;                   // widest layer-0 input whose weights the forward stages in LDS
  int bwd_donate_pct = -1;            // diagnostic (IQLHIP_BWD_DONATE_PCT): share of the policy's dW1 tiles run on the other XCDs
  int bwd_spb_force = -1;             // the same for the backward's (b) blocks (IQLHIP_BWD_SPB_L2)
  int fwd_spb_force = -1;             // diagnostic (IQLHIP_FWD_SPB_L2): fixed slices-per-block exponent of the forward
  bool fwd_early = true;              // diagnostic (IQLHIP_FWD_EARLY=0): plain one-slice fp32 steps keep iql_fwd_kernel
  bool fwd_early_layout = false;      // the dims and the arena layout are what iql_fwd_kernel_early restates (fwd_early_layout_ok)
  mutable std::atomic<int64_t> fwd_early_launches{0};      // tests: forwards launched or captured as iql_fwd_kernel_early
  // large-batch bf16 path (iqlhip_lb_kernels.h): bf16 precision and more than LB_MIN_ROWS rows per step
  float* pi_t = nullptr;              // [max_batch][32] T | [max_batch][32] G | [max_batch] L: the policy's loss terms without w
  __bf16* dh1g = nullptr;             // [4][max_batch][256] dH1 rows, [4][max_batch][256] dH0 rows, [max_batch][32] policy dY (allocated
  float* slab_x = nullptr;            // with the bf16 shadows); [64][n_params] the row blocks' partial sums
  __bf16* wimg = nullptr;             // bf16 path: operand images of W1 / W0, [6][IMG_STRIDE] (iqlhip_kernels.h)
  int lb_enabled = 1;                 // diagnostic (IQLHIP_LB=0): keep the small-batch kernels at every batch size
  int lb_nbb_force = -1, lb_cpb_force = -1, lb_nbi_force = -1;   // diagnostic (IQLHIP_LB_NBB / _CPB / _NBI)
  bool lb_pi_spread = true;           // IQLHIP_LB_PI_SPREAD=0: the policy's forward tiles on its own 32 blocks only (diagnostic)
  bool lb_csplit = true;              // IQLHIP_LB_CSPLIT=0: no column split of the row kernel at <= 1 024 rows (diagnostic)
  int lb_bwd_part = 0;                // iqlhip_debug_time_kernel only: 1 = launch the row kernel alone, 2 = the GEMM kernel alone
  size_t lds_bwd_lb = 0;
  // graph cache (a few (K,B,buffer) shapes: the steady chunk, the tail chunk, ...)
  hipStream_t cap_stream = nullptr;
  struct CachedGraph { GraphKey key; hipGraph_t graph; hipGraphExec_t exec; unsigned long long stamp; hipStream_t last;
                       IdleWork* work; /* [K] device records of the chunk's idle-block work (freed with the graph, not by `own`) */
                       hipGraphNode_t setup_node; /* head chunks: the set-up kernel's node */ };
  // Continuation of the index stream across calls: the last forward of a call stages the rows (and keep-bits) of the
  // step that would come next; a following call that IS that step (same rows / size / batch / seed, counter position
  // where the previous call stopped, staging untouched in between) starts without gathering anything.
  struct { bool valid = false; const float* rows = nullptr; int64_t ld = 0, size = 0; int32_t B = 0; uint64_t seed = 0;
           uint64_t next_offset = 0; float drop_p = 0.f; uint64_t drop_seed = 0, drop_step = 0;
           uint64_t wt_gen = 0;      // the table generation of a weighted call (0: a plain call)
           int cont_class = 0;       // KindInfo::cont_class of that call: what it staged besides the rows
           uint64_t wt_ver = 0;      // ... and the table's content version at that call (iqlhip_weights_update adds 1)
           const void* owner = nullptr;      // who staged: nullptr a solo call, else the trainer group whose call did
         } cont;
  std::vector<CachedGraph> graphs;
  unsigned long long graph_clock = 0;
  // data-parallel gradient exchange
  int xch_mode = IQLHIP_XCH_NONE;
  int rank = 0, world = 1;
  float* xflat = nullptr;             // RCCL / split path: this rank's flat gradient [n_params + 4] (+ pad)
  void* nccl_comm = nullptr;
  // P2P: one exchange block per rank = [flags: IQLHIP_MAX_WORLD x 16 u64][flat 0][flat 1], exported through hipIpc
  char* xblk = nullptr;               // (freed by iqlhip_xch_shutdown, not by `own`)
  size_t xblk_bytes = 0, xflat_off[2] = {0, 0};   // per parity buffer: [flat n_params+4 | slab_b (8 row tiles) | loss_parts]
  size_t xslabb_off[2] = {0, 0}, xloss_off[2] = {0, 0};
  long long xslab_b_off[4] = {0, 0, 0, 0};        // per-net offsets inside an exchange block's slab_b region (8 row tiles)
  char* peer_blk[IQLHIP_MAX_WORLD] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool p2p_attached = false;
  unsigned long long* xstatus = nullptr;   // device: [0] first timed-out step, [1] spare
  unsigned long long* xstatus_host = nullptr;   // pinned landing pad of the status words
  unsigned long long xstep = 0;            // steps exchanged so far (the P2P flags count them)
  unsigned long long xtimeout_ticks = 500000000ull;   // 5 s of the 100 MHz wall clock
  // per-step statistics (iqlhip_set_step_stats; allocated by the first call that enables them)
  bool stats_on = false;
  float* stats_part = nullptr;        // device [4 nets][stats_n_part]: sums of squares of 1024-element gradient windows
  int stats_n_part = 0;
  float* stats_last = nullptr;        // device [IQLHIP_N_STATS]: the last step's
  float* stats_ring = nullptr;        // device [k_max][IQLHIP_N_STATS]: per step of the last iqlhip_train_steps call
  float* stats_host = nullptr;        // pinned landing pad of the two read calls [k_max][IQLHIP_N_STATS]
  // gradient-norm clipping (iqlhip_set_grad_clip; allocated by the first call that enables it; shares stats_part)
  bool clip_on = false;
  float clip_max[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};   // V, Q, pi: +inf = no limit
  float* clip_dev = nullptr;          // device [12]: limits at 0..2, the last step's coefficients at 4..6, its norms at 8..10
  float* clip_host = nullptr;         // pinned [24]: staging of an upload of clip_dev at 0..11, landing pad of iqlhip_read_grad_clip at 12..
  hipEvent_t clip_up = nullptr;       // the last upload of the limits has read clip_host
  bool clip_up_pending = false;
  // scoring without a step (iqlhip_score_rows; allocated by the first call, sized by a chunk of rows)
  float* score_heads = nullptr;       // device [SCORE_CHUNK][HEAD_LD] scalar head partials
  float* score_pi = nullptr;          // device [SCORE_CHUNK][A][NSPLIT] policy head partials
  float* score_part = nullptr;        // device [SCORE_CHUNK / 32][SCORE_N_PART] tile partials
  double* score_acc = nullptr;        // device [16]: the call's running sums
  float* score_pin = nullptr;         // pinned, host-mapped [16]: the summary's landing words
  unsigned long long* score_status = nullptr;   // pinned, host-mapped [2]: the index check's verdict, an offending index
  bool score_lds_set = false;
  // the stream of the context's last step call (note_stream): iqlhip_set_grad_clip queues the new limits there
  hipStream_t last_stream = nullptr;
  bool has_last_stream = false;
  // timing
  bool timing = false;
  std::vector<hipEvent_t> ev;         // 4 per recorded step (grown by ensure_events, destroyed by iqlhip_destroy)
  int ev_used = 0;
  float t_acc[4] = {0, 0, 0, 0};
  int t_n = 0;
  // the vector-environment online call (iqlhip_online_step_vec; allocated by the first call): pinned, host-mapped staging
  // of the new rows [IQLHIP_VEC_MAX_ENVS][row_ld], of the drawn indices [IQLHIP_VEC_MAX_UPDATES][VEC_MAX_BATCH], of the
  // steps' losses [IQLHIP_VEC_MAX_UPDATES][4] and of the act: states in [IQLHIP_VEC_MAX_ENVS][IQLHIP_MAX_INPUT], actions
  // out [IQLHIP_VEC_MAX_ENVS][IQLHIP_MAX_ACTION]
  float* vec_rows_pin = nullptr;
  long long* vec_idx_pin = nullptr;
  float* vec_loss_pin = nullptr;
  float* vec_act_pin = nullptr;
  // ... and the gathered batches of its steps, device [updates][batch_rows][row_ld]: an owner of its own, because the
  // block is freed and allocated anew when a call needs more (vec_xb_cap floats)
  Owned vec_own;
  float* vec_xb = nullptr;
  size_t vec_xb_cap = 0;
};

extern "C" int iqlhip_version(void) { return IQLHIP_VERSION; }
extern "C" const char* iqlhip_last_error(void) { return g_err.c_str(); }

static int check_dims(const iqlhip_dims* d) {
  if (!d) return fail(IQLHIP_EINVAL, "dims is NULL");
  if (d->state_dim < 1 || d->action_dim < 1) return fail(IQLHIP_EINVAL, "state_dim/action_dim must be >= 1");
  if (d->hidden_dim != IQLHIP_HIDDEN || d->n_hidden != 2)
    return fail(IQLHIP_EUNSUPPORTED, "kernels are built for hidden_dim=%d, n_hidden=2 (got %d, %d)", IQLHIP_HIDDEN,
                d->hidden_dim, d->n_hidden);
  if (d->state_dim + d->action_dim > IQLHIP_MAX_INPUT)
    return fail(IQLHIP_EUNSUPPORTED, "state_dim + action_dim > %d", IQLHIP_MAX_INPUT);
  if (d->action_dim > IQLHIP_MAX_ACTION) return fail(IQLHIP_EUNSUPPORTED, "action_dim > %d", IQLHIP_MAX_ACTION);
  if (d->policy != IQLHIP_POLICY_GAUSSIAN && d->policy != IQLHIP_POLICY_DETERMINISTIC)
    return fail(IQLHIP_EINVAL, "unknown policy kind %d", d->policy);
  if (d->max_batch < 1 || d->max_batch > 16384) return fail(IQLHIP_EINVAL, "max_batch must be in [1,16384]");
  return IQLHIP_OK;
}

extern "C" int iqlhip_arena_layout(const iqlhip_dims* d, iqlhip_layout* out) {
  int rc = check_dims(d);
  if (rc) return rc;
  if (!out) return fail(IQLHIP_EINVAL, "out is NULL");
  const int S = d->state_dim, A = d->action_dim, Hd = IQLHIP_HIDDEN;
  int64_t off = 0;
  for (int n = 0; n < 4; ++n) {
    iqlhip_net_layout& nl = out->net[n];
    nl.k_in = (n == IQLHIP_NET_Q1 || n == IQLHIP_NET_Q2) ? S + A : S;
    nl.d_out = (n == IQLHIP_NET_PI) ? A : 1;
    nl.seg_begin = off;
    nl.w1 = off; off += (int64_t)Hd * Hd;
    nl.w0 = off; off += (int64_t)Hd * nl.k_in;
    nl.b0 = off; off += Hd;
    nl.b1 = off; off += Hd;
    nl.w2 = off; off += (int64_t)nl.d_out * Hd;
    nl.b2 = off; off += up(nl.d_out, 4);
    if (n == IQLHIP_NET_PI && d->policy == IQLHIP_POLICY_GAUSSIAN) { nl.log_std = off; off += up(A, 4); }
    else nl.log_std = -1;
    off = up(off, 64);
    nl.seg_end = off;
  }
  out->n_params = off;
  out->target_src = out->net[IQLHIP_NET_Q1].seg_begin;
  out->n_target = out->net[IQLHIP_NET_Q2].seg_end - out->net[IQLHIP_NET_Q1].seg_begin;
  return IQLHIP_OK;
}

extern "C" int64_t iqlhip_row_stride(int32_t S, int32_t A) { return up(2 * (int64_t)S + A + 2, 4); }

static int xld_host(int k0) { int k0p = (k0 + 3) & ~3; return ((k0p + 29) / 32) * 32 + 2; }

extern "C" int iqlhip_destroy(iqlhip_ctx* c);
extern "C" int iqlhip_xch_shutdown(iqlhip_ctx* c);

static bool fwd_early_layout_ok(const iqlhip_ctx* c);      // (defined in front of launch_fwd_grid)
static int create_impl(iqlhip_ctx* c, const iqlhip_dims* dims, const iqlhip_hyper* hyper, int device) {
  c->dims = *dims;
  c->hyper = *hyper;
  c->device = device;
  iqlhip_arena_layout(dims, &c->L);
  const int MB = dims->max_batch, A = dims->action_dim;
  c->n_chunk_max = (MB + CHUNK_ROWS - 1) / CHUNK_ROWS;
  c->n_rt_max = (MB + RT_ROWS - 1) / RT_ROWS;
  c->sc.max_batch = MB;
  Owned& own = c->own;
  auto dalloc = [&](float** p, size_t nfloat) { return own.dev(p, nfloat * sizeof(float), 0); };
  HIPCHK(dalloc(&c->sc.h0, (size_t)4 * MB * HID));
  HIPCHK(dalloc(&c->sc.h1, (size_t)4 * MB * HID));
  HIPCHK(dalloc(&c->sc.heads, (size_t)MB * HEAD_LD + (size_t)NSPLIT * MB * A));
  c->row_ld = iqlhip_row_stride(dims->state_dim, A);
  HIPCHK(dalloc(&c->xb, (size_t)MB * c->row_ld));
  HIPCHK(dalloc(&c->xb2, (size_t)MB * c->row_ld));
  HIPCHK(own.pin(&c->losses_host, 4 * sizeof(float)));
  HIPCHK(own.pin(&c->on_row_pin, (size_t)c->row_ld * sizeof(float)));
  HIPCHK(own.pin(&c->on_idx_pin, (size_t)MB * sizeof(long long)));
  HIPCHK(own.pin(&c->on_loss_pin, 4 * sizeof(float)));
  HIPCHK(own.pin(&c->done_pin, 8 * sizeof(unsigned long long), /*zero=*/true));
  HIPCHK(own.pin(&c->on_act_pin, (size_t)(IQLHIP_MAX_INPUT + IQLHIP_MAX_ACTION) * sizeof(float)));
  c->act_cap = std::max(MB, IQLHIP_ACT_ROWS);
  HIPCHK(dalloc(&c->xb_act, (size_t)c->act_cap * c->row_ld));
  HIPCHK(dalloc(&c->heads_act, (size_t)c->act_cap * A * NSPLIT));
  HIPCHK(own.dev(&c->drop_bits, (size_t)4 * MB * 8 * sizeof(unsigned), 0xFF));
  HIPCHK(dalloc(&c->sc.slab_a, (size_t)c->n_chunk_max * c->L.n_params));
  size_t sb = 0;
  for (int n = 0; n < 4; ++n) {
    c->sc.slab_b_off[n] = (long long)sb;
    sb += (size_t)c->n_rt_max * ((size_t)HID * c->L.net[n].k_in + HID);
  }
  HIPCHK(dalloc(&c->sc.slab_b, sb));
  HIPCHK(dalloc(&c->sc.loss_parts, 2 * 4 * 64));      // [4 losses][64 chunks / row blocks] (+ a second set: the large-batch path's totals)
  HIPCHK(dalloc(&c->pi_t, (size_t)MB * 65));
  HIPCHK(dalloc(&c->sc.losses, 4));
  HIPCHK(dalloc(&c->flat_tmp, (size_t)c->L.n_params + 4));
  c->k_max = 1024;
  c->ring_cap = c->k_max;
  // the loss ring lives in host-mapped pinned memory: each step's update kernel posts its 3 words there, and the
  // end of a train_steps call is ONE stream synchronisation queued right behind the work — no device-to-host copy
  HIPCHK(own.pin(&c->loss_ring, (size_t)c->ring_cap * 4 * sizeof(float), /*zero=*/true));
  HIPCHK(own.dev(&c->sched_cur, (size_t)GRAPH_STEPS * sizeof(iqlhip_step_scalars)));
  HIPCHK(own.dev(&c->sched_call, (size_t)c->k_max * sizeof(iqlhip_step_scalars)));
  for (int i = 0; i < 4; ++i) HIPCHK(own.pin(&c->sched_pin[i], (size_t)c->k_max * sizeof(iqlhip_step_scalars)));
  HIPCHK(own.pin(&c->sched_ack, 8 * sizeof(unsigned long long), /*zero=*/true));   // [4] slots + a dummy word
  HIPCHK(own.dev(&c->setup_arrivals, 64, 0));
  HIPCHK(own.dev(&c->hdr, HDR_WORDS * sizeof(unsigned long long), 0));
  HIPCHK(own.dev(&c->xstatus, 2 * sizeof(unsigned long long), 0));
  HIPCHK(own.pin(&c->xstatus_host, 2 * sizeof(unsigned long long), /*zero=*/true));
  HIPCHK(dalloc(&c->xflat, (size_t)up(c->L.n_params + 4, 64)));
  HIPCHK(hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking));
#ifdef IQL_STAMPS
  HIPCHK(own.dev(&c->stamps, 4096 * 16 * sizeof(unsigned long long), 0));
#endif
  // LDS sizes
  const int kq = dims->state_dim + dims->action_dim;
  const int ks_ = dims->state_dim;   // V / pi layer-0 width; Q nets use kq
  // layer-0 weights are staged in LDS for every instance whose input width fits: through registers up to
  // W0_LDS_MAX_K, by LDS-DMA (no registers) above that, as far as the CU's 160 KB allow (1 KiB-float4 slack for the
  // DMA's whole-wave granularity)
  const size_t fwd_fixed = (size_t)(RT_ROWS * H0_LD + RT_ROWS * T64_LD + RT_ROWS * (int)c->row_ld +
                                    (((A + 15) & ~15) * W2_LD + 32) + 512 + 16) * sizeof(float);
  auto fits = [&](int k) { return fwd_fixed + (size_t)HID * k * sizeof(float) + 4096 <= (size_t)160 * 1024 - 1024; };
  int w0_lds_k = 0;
  if (kq <= W0_DMA_MAX_K && fits(kq)) w0_lds_k = kq;
  else if (ks_ <= W0_DMA_MAX_K && fits(ks_)) w0_lds_k = ks_;
  if (const char* ov = getenv("IQLHIP_W0_LDS_K")) w0_lds_k = std::min(w0_lds_k, atoi(ov));   // diagnostic (tools/): force a narrower staging
  c->w0_lds_k = w0_lds_k;
  if (const char* ov = getenv("IQLHIP_BWD_DONATE_PCT")) c->bwd_donate_pct = std::max(0, std::min(100, atoi(ov)));   // diagnostic (tools/)
  if (const char* ov = getenv("IQLHIP_BWD_SPB_L2")) c->bwd_spb_force = std::max(0, std::min(2, atoi(ov)));   // diagnostic (tools/)
  if (const char* ov = getenv("IQLHIP_FWD_SPB_L2")) c->fwd_spb_force = std::max(0, std::min(2, atoi(ov)));   // diagnostic (tools/)
  if (const char* ov = getenv("IQLHIP_FWD_EARLY")) c->fwd_early = atoi(ov) != 0;                             // diagnostic (tools/)
  if (const char* ov = getenv("IQLHIP_LB")) c->lb_enabled = atoi(ov) != 0;                                     // diagnostic (tools/)
  if (const char* ov = getenv("IQLHIP_LB_NBB")) c->lb_nbb_force = std::max(2, atoi(ov));
  if (const char* ov = getenv("IQLHIP_LB_CSPLIT")) c->lb_csplit = atoi(ov) != 0;
  if (const char* ov = getenv("IQLHIP_LB_PI_SPREAD")) c->lb_pi_spread = atoi(ov) != 0;
  if (const char* ov = getenv("IQLHIP_LB_CPB")) c->lb_cpb_force = std::max(1, atoi(ov));
  if (const char* ov = getenv("IQLHIP_LB_NBI")) c->lb_nbi_force = std::max(2, atoi(ov));
  c->lds_fwd = fwd_fixed + (size_t)HID * w0_lds_k * sizeof(float) + (w0_lds_k > W0_LDS_MAX_K ? 4096 : 0);
  // One block per CU while the grid fits the chip (co-resident blocks share a CU's L1 and fill rate and only slow
  // each other down); the exact size — two blocks per CU where it is <= 80 KB — once there are more blocks than CUs.
  c->lds_fwd_solo = std::max(c->lds_fwd, (size_t)(81 * 1024));
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && ncu > 0) c->n_cus = ncu;
  }
  const int dyld = ((A + 15) & ~15) + 4;     // (a) blocks: [256][Dp + 4] rows for dY and dlog_std terms
  const size_t lds_a = (size_t)(4 * 32 * T64_LD + 2 * CHUNK_ROWS * dyld + 32 * 32 + 64 + CHUNK_ROWS) * sizeof(float);
  const size_t lds_b = (size_t)(RT_ROWS * H0_LD + 4 * 32 * T64_LD + RT_ROWS * T64_LD + RT_ROWS * 36 + 4 +
                                RT_ROWS * XR_LD_MAX) * sizeof(float);
  c->lds_bwd = std::max(lds_a, lds_b);
  // large-batch backward, row blocks: [dH1 tile | H1 tile | dH0 tile | dY | dy] (iql_bwd_rows_kernel)
  c->lds_bwd_lb = (size_t)(3 * 32 * H0B_LD + 32 * LB_DYLD) * 2 + 32 * 4 + (size_t)(2 * 4 * 32 + 16) * 4;      // (+ the block sums' partials)
  int rc = set_max_lds(3, c->lds_fwd_solo, [](unsigned m) { return fwd_kernel(m & 1, m & 2, m & 4); });
  if (!rc) rc = set_max_lds(0, c->lds_fwd_solo, [](unsigned) { return &iql_fwd_kernel_early; });
  if (!rc) rc = set_max_lds(2, c->lds_fwd_solo, [](unsigned m) { return fwd_one_kernel(m & 1, m & 2); });
  if (!rc) rc = set_max_lds(3, c->lds_bwd, [](unsigned m) { return bwd_kernel(m & 1, m & 2, m & 4); });
  if (!rc) rc = set_max_lds(1, c->lds_bwd_lb, [](unsigned m) { return bwd_rows_kernel(m & 1); });
  if (!rc) rc = set_max_lds(2, c->lds_bwd, [](unsigned m) { return bwd_rw_kernel(m & 1, m & 2); });
  c->fwd_lds_set[(int)ChunkKind::Plain] = !rc;      // (the other kinds: ensure_fwd_lds, at their first call)
  c->fwd_early_layout = fwd_early_layout_ok(c);
  return rc;
}

extern "C" int iqlhip_create(const iqlhip_dims* dims, const iqlhip_hyper* hyper, int device, iqlhip_ctx** out) {
  int rc = check_dims(dims);
  if (rc) return rc;
  if (!hyper || !out) return fail(IQLHIP_EINVAL, "hyper/out is NULL");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(IQLHIP_EHIP, "device %d not available (%d visible)", device, ndev);
  DevGuard guard(device);               // the caller's current device is restored on return
  iqlhip_ctx* c = new iqlhip_ctx();
  rc = create_impl(c, dims, hyper, device);
  if (rc) {                             // free whatever was allocated before the failure (the message survives)
    const std::string msg = g_err;
    iqlhip_destroy(c);
    g_err = msg;
    return rc;
  }
  *out = c;
  return IQLHIP_OK;
}

// A cached chunk graph's three resources (their lifetime is the graph's, not the context's: the cache evicts); null
// members: a graph whose construction stopped half-way.
static void free_graph(iqlhip_ctx::CachedGraph& g) {
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.graph) (void)hipGraphDestroy(g.graph);
  if (g.work) (void)hipFree(g.work);
}
static void drop_graph(iqlhip_ctx* c) {
  for (auto& g : c->graphs) {
    if (g.last) (void)hipStreamSynchronize(g.last);   // a replay may still be executing
    free_graph(g);
  }
  c->graphs.clear();
  c->cont.valid = false;
}

extern "C" int iqlhip_destroy(iqlhip_ctx* c) {
  if (!c) return IQLHIP_OK;
  DevGuard guard(c->device);
  (void)hipDeviceSynchronize();
  drop_graph(c);
  (void)iqlhip_xch_shutdown(c);
  for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
  if (c->cap_stream) (void)hipStreamDestroy(c->cap_stream);
  c->vec_own.release_all();
  c->own.release_all();
  delete c;
  return IQLHIP_OK;
}

extern "C" int iqlhip_set_hyper(iqlhip_ctx* c, const iqlhip_hyper* h) {
  if (!c || !h) return fail(IQLHIP_EINVAL, "NULL argument");
  c->hyper = *h;
  drop_graph(c);
  return IQLHIP_OK;
}

extern "C" int iqlhip_set_precision(iqlhip_ctx* c, int mode) {
  if (!c) return fail(IQLHIP_EINVAL, "NULL ctx");
  if (mode != 0 && mode != 1) return fail(IQLHIP_EINVAL, "precision mode must be 0 (f32) or 1 (bf16 operands)");
  if (mode != c->precision) drop_graph(c);
  if (mode == 1 && !c->wsh) {
    DevGuard guard(c->device);
    const int rc = all_or_nothing(c->own, [&]() -> int {
      Owned& own = c->own;
      HIPCHK(own.dev(&c->wsh, (size_t)up(c->L.n_params, 64) * sizeof(__bf16)));
      HIPCHK(own.dev(&c->tsh, (size_t)up(c->L.n_target, 64) * sizeof(__bf16)));
      // scratch of the large-batch backward (iqlhip_lb_kernels.h)
      const size_t MB = (size_t)c->dims.max_batch;
      HIPCHK(own.dev(&c->dh1g, (8 * MB * HID + MB * 32 + MB * LB_XLD + 4 * 65536 + 8192) * sizeof(__bf16), 0));
      HIPCHK(own.dev(&c->wimg, (size_t)6 * IMG_STRIDE * sizeof(__bf16), 0));
      HIPCHK(own.dev(&c->slab_x, (size_t)64 * c->L.n_params * sizeof(float), 0));
      return IQLHIP_OK;
    });
    if (rc) return rc;
  }
  c->precision = mode;
  return IQLHIP_OK;
}

// The context's two Philox stream positions: {dropout step, act() call}.  A caller that replaces a context (the shim
// re-creates it when a larger batch arrives) carries them over so that neither stream replays from its beginning.
extern "C" int iqlhip_get_counters(const iqlhip_ctx* c, uint64_t out[2]) {
  if (!c || !out) return fail(IQLHIP_EINVAL, "NULL argument");
  out[0] = c->drop_step;
  out[1] = c->act_calls;
  return IQLHIP_OK;
}
extern "C" int iqlhip_set_counters(iqlhip_ctx* c, const uint64_t in[2]) {
  if (!c || !in) return fail(IQLHIP_EINVAL, "NULL argument");
  c->drop_step = in[0];
  c->act_calls = in[1];
  return IQLHIP_OK;
}

extern "C" int iqlhip_set_dropout(iqlhip_ctx* c, float p, uint64_t seed) {
  if (!c) return fail(IQLHIP_EINVAL, "NULL ctx");
  if (!(p >= 0.f && p < 1.f)) return fail(IQLHIP_EINVAL, "dropout probability must be in [0,1)");
  c->drop_p = p;
  c->drop_seed = seed;
  c->drop_inject = false;
  return IQLHIP_OK;
}

// The inference side of actor dropout: its own rate and key (the training rate above is untouched), position
// act_drop_calls.  The keep-bit buffer is allocated with the first rate > 0.
extern "C" int iqlhip_set_act_dropout(iqlhip_ctx* c, float p, uint64_t seed) {
  if (!c) return fail(IQLHIP_EINVAL, "NULL ctx");
  if (!(p >= 0.f && p < 1.f)) return fail(IQLHIP_EINVAL, "dropout probability must be in [0,1)");
  if (p > 0.f && !c->act_drop_bits) {
    DevGuard guard(c->device);
    HIPCHK(c->own.dev(&c->act_drop_bits, (size_t)2 * c->act_cap * 8 * sizeof(unsigned), 0xFF));      // (one allocation: made whole or not at all)
  }
  c->act_drop_p = p;
  c->act_drop_seed = seed;
  return IQLHIP_OK;
}
extern "C" int iqlhip_get_act_dropout_counter(const iqlhip_ctx* c, uint64_t* out) {
  if (!c || !out) return fail(IQLHIP_EINVAL, "NULL argument");
  *out = c->act_drop_calls;
  return IQLHIP_OK;
}
extern "C" int iqlhip_set_act_dropout_counter(iqlhip_ctx* c, uint64_t n) {
  if (!c) return fail(IQLHIP_EINVAL, "NULL ctx");
  c->act_drop_calls = n;
  return IQLHIP_OK;
}

extern "C" int iqlhip_debug_write_masks(iqlhip_ctx* c, const uint32_t* keep0, const uint32_t* keep1, int32_t rows,
                                        void* stream) {
  if (!c || !keep0 || !keep1) return fail(IQLHIP_EINVAL, "NULL argument");
  if (rows < 1 || rows > c->dims.max_batch) return fail(IQLHIP_EINVAL, "rows outside [1,max_batch]");
  hipStream_t st = (hipStream_t)stream;
  const size_t nb = (size_t)rows * 8 * sizeof(unsigned);
  HIPCHK(hipMemcpyAsync(c->drop_bits, keep0, nb, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->drop_bits + (size_t)c->dims.max_batch * 8, keep1, nb, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  c->drop_inject = true;
  c->cont.valid = false;
  return IQLHIP_OK;
}

extern "C" int iqlhip_bind(iqlhip_ctx* c, float* params, float* target, float* m, float* v) {
  if (!c || !params || !target || !m || !v) return fail(IQLHIP_EINVAL, "NULL argument");
  if (((uintptr_t)params | (uintptr_t)target | (uintptr_t)m | (uintptr_t)v) & 15)
    return fail(IQLHIP_EINVAL, "arenas must be 16-byte aligned");
  c->params = params; c->target = target; c->m = m; c->v = v;
  drop_graph(c);
  return IQLHIP_OK;
}

extern "C" int64_t iqlhip_grad_words(const iqlhip_ctx* c) { return c ? c->L.n_params + 4 : 0; }

// ---------------------------------------------------------------------------
static int check_batch(const iqlhip_ctx* c, const iqlhip_batch* b) {
  if (!c->params) return fail(IQLHIP_ENOTBOUND, "iqlhip_bind has not been called");
  if (!b) return fail(IQLHIP_EINVAL, "batch is NULL");
  if (b->rows < 1 || b->rows > c->dims.max_batch)
    return fail(IQLHIP_EINVAL, "batch rows %d outside [1, max_batch=%d]", b->rows, c->dims.max_batch);
  if (!b->s_dev || !b->a_dev || !b->r_dev || !b->ns_dev || !b->d_dev) return fail(IQLHIP_EINVAL, "NULL batch tensor");
  if (b->ld_s < c->dims.state_dim || b->ld_ns < c->dims.state_dim || b->ld_a < c->dims.action_dim || b->ld_r < 1 ||
      b->ld_d < 1)
    return fail(IQLHIP_EINVAL, "batch row strides smaller than the row widths");
  return IQLHIP_OK;
}

// True if the five arrays are views of ONE block of packed rows [s|a|s'|r|d|pad] with the library's row stride.
static bool is_packed(const iqlhip_ctx* c, const iqlhip_batch* b) {
  const int S = c->dims.state_dim, A = c->dims.action_dim;
  return b->ld_s == c->row_ld && b->ld_a == c->row_ld && b->ld_r == c->row_ld && b->ld_ns == c->row_ld &&
         b->ld_d == c->row_ld && b->a_dev == b->s_dev + S && b->ns_dev == b->s_dev + S + A &&
         b->r_dev == b->s_dev + 2 * S + A && b->d_dev == b->s_dev + 2 * S + A + 1;
}

// An indexed batch must be row-addressed storage in the packed layout (what ReplayBuffer holds).
static int check_indexed(const iqlhip_ctx* c, const iqlhip_batch* b) {
  const bool packed = is_packed(c, b);
  if (!packed) return fail(IQLHIP_EINVAL, "indexed batches must address packed rows [s|a|s'|r|d] with ld=%lld",
                           (long long)c->row_ld);
  if (((uintptr_t)b->s_dev) & 15) return fail(IQLHIP_EINVAL, "packed rows must be 16-byte aligned");
  return IQLHIP_OK;
}

static void launch_gather(const iqlhip_ctx* c, const float* rows, const long long* idx, int n, hipStream_t st) {
  const int total = n * (int)(c->row_ld / 4);
  hipLaunchKernelGGL(iql_gather_kernel, dim3((total + 255) / 256), dim3(256), 0, st, rows, (long long)c->row_ld, idx,
                     c->xb, n, 0ll);
}

// Bring the caller's batch into packed rows (the kernels read nothing else): gather by index, or pack five
// arrays into the staging buffer xb, or — when the caller's arrays already ARE one block of packed rows (what
// ReplayBuffer.sample returns) — consume them in place.  *xb_out = where the packed batch is.
static int stage_batch(const iqlhip_ctx* c, const iqlhip_batch* b, hipStream_t st, const float** xb_out) {
  *xb_out = c->xb;
  if (!b->idx_dev && is_packed(c, b) && !(((uintptr_t)b->s_dev) & 15)) {
    *xb_out = b->s_dev;
    return IQLHIP_OK;
  }
  if (b->idx_dev) {
    int rc = check_indexed(c, b);
    if (rc) return rc;
    launch_gather(c, b->s_dev, (const long long*)b->idx_dev, b->rows, st);
  } else {
    const int total = b->rows * (int)c->row_ld;
    hipLaunchKernelGGL(iql_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, st, c->xb, (int)c->row_ld,
                       c->dims.state_dim, c->dims.action_dim, b->rows, b->s_dev, (long long)b->ld_s, b->a_dev,
                       (long long)b->ld_a, b->r_dev, (long long)b->ld_r, b->ns_dev, (long long)b->ld_ns, b->d_dev,
                       (long long)b->ld_d);
  }
  return IQLHIP_OK;
}

static NetPtrs net_ptrs(const iqlhip_net_layout& nl, const float* base) {
  NetPtrs n;
  n.w0 = base + nl.w0; n.b0 = base + nl.b0; n.w1 = base + nl.w1; n.b1 = base + nl.b1;
  n.w2 = base + nl.w2; n.b2 = base + nl.b2; n.k0 = nl.k_in; n.d = nl.d_out;
  return n;
}

// ---------------------------------------------------------------------------
// Large-batch bf16 path (iqlhip_lb_kernels.h): which steps take it, and how their rows are spread over blocks.
#define LB_MIN_ROWS 512
static bool use_lb(const iqlhip_ctx* c, int rows) {
  if (c->precision != 1 || !c->lb_enabled || rows <= LB_MIN_ROWS) return false;
  if (c->fwd_spb_force >= 0 || c->bwd_spb_force >= 0) return false;      // (diagnostic layouts of the small-batch kernels)
  return c->dims.state_dim + c->dims.action_dim + 1 <= 16 * 5;           // [dW0 | db0] tiles a (b) block keeps in registers
}
struct LbGeom { int n_rt, n_chunk, nbi, nbb, cpb, n_cg, csplit; };
static LbGeom lb_geom(const iqlhip_ctx* c, int rows) {
  LbGeom g;
  g.n_rt = (rows + RT_ROWS - 1) / RT_ROWS;
  g.n_chunk = (rows + CHUNK_ROWS - 1) / CHUNK_ROWS;
  const int even_rt = (g.n_rt + 1) & ~1;
  // forward: 7 instances + the idle eighth share the chip: 32 blocks per instance, each walks ceil(n_rt / 32) row tiles
  g.nbi = std::min(even_rt, c->lb_nbi_force > 0 ? (c->lb_nbi_force + 1) & ~1 : 32);
  // backward: a net's blocks live on its two XCDs (64 CUs): (b) blocks of up to n_rt / nbb row tiles, (a) blocks of cpb chunks
  g.nbb = std::min(std::min(even_rt, 64), c->lb_nbb_force > 0 ? (c->lb_nbb_force + 1) & ~1 : 64);
  // up to 32 row tiles (1 024 rows): two blocks per tile, each half of the dH0 columns (iql_bwd_rows_kernel<true>) — a block
  // per tile would leave half the chip idle.  IQLHIP_LB_CSPLIT=0: the one-block-per-tile form at every size (diagnostic).
  g.csplit = (even_rt <= 32 && c->lb_nbb_force <= 0 && c->lb_csplit) ? 1 : 0;      // (nbb = even_rt then: one slab per tile)
  // GEMM blocks: 28 jobs per net and chunk group; about four chunk groups keep >= 400 blocks in flight
  g.cpb = c->lb_cpb_force > 0 ? std::min(c->lb_cpb_force, g.n_chunk) : std::max(1, std::min(8, g.n_chunk / 4));
  g.n_cg = (g.n_chunk + g.cpb - 1) / g.cpb;
  return g;
}
static LbArgs lb_args(const iqlhip_ctx* c, int rows) {
  const LbGeom g = lb_geom(c, rows);
  LbArgs a;
  a.pi_t = c->pi_t;
  a.pi_g = c->pi_t + (size_t)c->dims.max_batch * 32;
  a.pi_l = c->pi_t + (size_t)c->dims.max_batch * 64;
  a.n_rt = g.n_rt; a.n_chunk = g.n_chunk; a.nbi = g.nbi; a.nbb = g.nbb; a.cpb = g.cpb; a.n_cg = g.n_cg;
  const size_t MB = (size_t)c->dims.max_batch;
  a.dh1g = c->dh1g;
  a.dh0g = c->dh1g + 4 * MB * HID;
  a.dyg = c->dh1g + 8 * MB * HID;
  a.xbf = a.dyg + MB * 32;
  a.w1t = a.xbf + MB * LB_XLD;
  a.slab_x = c->slab_x;
  a.wimg = c->wimg;
  for (int n = 0; n < 4; ++n) { a.go_w0[n] = c->L.net[n].w0; a.go_b0[n] = c->L.net[n].b0; a.go_w1n[n] = c->L.net[n].seg_begin; }
  return a;
}

static StepParams make_step(const iqlhip_ctx* c, int rows, float inv_batch) {
  StepParams p;
  memset(&p, 0, sizeof p);
  p.stamps = c->stamps;
  const iqlhip_layout& L = c->L;
  const float* tb = c->target - L.target_src;
  const int S = c->dims.state_dim, A = c->dims.action_dim;
  // instances: V(s'), V(s), Qt1, Qt2, Q1, Q2, pi
  p.inst[0] = net_ptrs(L.net[IQLHIP_NET_V], c->params);  p.xoff[0] = S + A; p.slot[0] = -1;
  p.inst[1] = net_ptrs(L.net[IQLHIP_NET_V], c->params);  p.xoff[1] = 0;     p.slot[1] = 0;
  p.inst[2] = net_ptrs(L.net[IQLHIP_NET_Q1], tb);        p.xoff[2] = 0;     p.slot[2] = -1;
  p.inst[3] = net_ptrs(L.net[IQLHIP_NET_Q2], tb);        p.xoff[3] = 0;     p.slot[3] = -1;
  p.inst[4] = net_ptrs(L.net[IQLHIP_NET_Q1], c->params); p.xoff[4] = 0;     p.slot[4] = 1;
  p.inst[5] = net_ptrs(L.net[IQLHIP_NET_Q2], c->params); p.xoff[5] = 0;     p.slot[5] = 2;
  p.inst[6] = net_ptrs(L.net[IQLHIP_NET_PI], c->params); p.xoff[6] = 0;     p.slot[6] = 3;
  p.inst[7] = p.inst[6]; p.xoff[7] = 0; p.slot[7] = -1;
  if (c->precision == 1) {
    // bf16 path: the kernels read W1 from the bf16 shadows (same element offsets); the field carries that address
    const __bf16* wb = c->wsh;
    const __bf16* tbs = c->tsh - L.target_src;
    const int netof[7] = {IQLHIP_NET_V, IQLHIP_NET_V, IQLHIP_NET_Q1, IQLHIP_NET_Q2, IQLHIP_NET_Q1, IQLHIP_NET_Q2, IQLHIP_NET_PI};
    for (int i = 0; i < 7; ++i) p.inst[i].w1 = (const float*)(((i == 2 || i == 3) ? tbs : wb) + L.net[netof[i]].w1);
    p.inst[7].w1 = p.inst[6].w1;
  }
  for (int n = 0; n < 4; ++n) {
    p.net[n] = net_ptrs(L.net[n], c->params);
    if (c->precision == 1) p.net[n].w1 = (const float*)(c->wsh + L.net[n].w1);
    p.go[n].w1 = L.net[n].w1; p.go[n].b1 = L.net[n].b1; p.go[n].w2 = L.net[n].w2; p.go[n].b2 = L.net[n].b2;
    p.go[n].log_std = L.net[n].log_std;
  }
  p.log_std = (L.net[IQLHIP_NET_PI].log_std >= 0) ? c->params + L.net[IQLHIP_NET_PI].log_std : nullptr;
  p.hy = c->hyper;
  p.sc = c->sc;
  p.xb = c->xb;
  p.ld = (int)c->row_ld;
  p.rows = rows;
  p.S = S;
  p.A = A;
  p.policy = c->dims.policy;
  p.inv_batch = inv_batch;
  p.n_params = L.n_params;
  p.drop_bits = (c->drop_p > 0.f) ? c->drop_bits : nullptr;
  p.drop_scale = (c->drop_p > 0.f) ? 1.f / (1.f - c->drop_p) : 1.f;
  p.only_inst = -1;
  p.w0_lds_k = c->w0_lds_k;
  p.g_work = nullptr;
  return p;
}

// The forward record of policy inference over `rows` rows packed in xb_act (iqlhip_actor_forward, and the trainer
// groups' act launches, which pass the same record per member).
static StepParams act_step_params(const iqlhip_ctx* c, int rows) {
  StepParams p = make_step(c, rows, 1.f / (float)rows);
  p.xb = c->xb_act;
  p.only_inst = 6;
  p.slot[6] = -1;            // inference keeps no activations
  p.drop_bits = nullptr;     // the training steps' keep-bits are not the inference forward's
  p.drop_scale = 1.f;
  p.sc.heads = c->heads_act; // the policy partials of row r land at heads[max_batch * HEAD_LD + r * A * NSPLIT ...]:
  p.sc.max_batch = 0;        // with max_batch = 0 that is heads_act[r * A * NSPLIT ...]
  if (c->act_drop_p > 0.f) {
    // inference with dropout: the forward reads layer 1's keep-bits at row max_batch + r of drop_bits, so max_batch
    // is the layer stride of act_drop_bits (act_cap) and the heads pointer is moved back by what that adds
    p.drop_bits = c->act_drop_bits;
    p.drop_scale = 1.f / (1.f - c->act_drop_p);
    p.sc.max_batch = c->act_cap;
    p.sc.heads = c->heads_act - (size_t)c->act_cap * HEAD_LD;
  }
  return p;
}

static UpdParams make_upd(const iqlhip_ctx* c, const iqlhip_step_scalars* sc, int rows, const float* flat) {
  UpdParams u;
  u.L = c->L;
  u.sc = *sc;
  u.tau = c->hyper.tau;
  u.one_minus_tau = c->hyper.one_minus_tau;
  u.params = c->params; u.target = c->target; u.m = c->m; u.v = c->v;
  u.slab_a = c->sc.slab_a; u.slab_b = c->sc.slab_b;
  for (int n = 0; n < 4; ++n) u.slab_b_off[n] = c->sc.slab_b_off[n];
  u.flat_grads = flat;
  u.loss_parts = c->sc.loss_parts;
  u.losses = c->sc.losses;
  u.losses_mirror = nullptr;
  u.loss_ring = nullptr;
  u.ring_slot = 0;
  u.n_chunk = (rows + CHUNK_ROWS - 1) / CHUNK_ROWS;
  u.n_rt = (rows + RT_ROWS - 1) / RT_ROWS;
  u.n_loss = u.n_chunk;
  u.slab_x = nullptr;
  u.n_x = 0;
  if (use_lb(c, rows)) {      // the large-batch backward writes one slab per chunk group and one per row block
    const LbGeom gm = lb_geom(c, rows);
    u.n_chunk = gm.n_cg;
    u.slab_x = c->slab_x;
    u.n_x = gm.nbb;
    u.loss_parts = c->sc.loss_parts + 256;      // (entry 0 of each row: the total, summed by the GEMM launch's reduction job)
    u.n_loss = 1;
  }
  u.batch_rows = rows;
  u.sched = nullptr;
  u.sched_idx = 0;
  u.ring_hdr = nullptr;
  u.adv_hdr = nullptr; u.adv_k = 0; u.adv_rows = 0;
  u.done_flag = nullptr; u.done_val = 0;
  u.wsh = (c->precision == 1) ? c->wsh : nullptr;
  u.tsh = (c->precision == 1) ? c->tsh : nullptr;
  u.wimg = (c->precision == 1 && use_lb(c, rows)) ? c->wimg : nullptr;      // (read by the large-batch forward only)
  if (getenv("IQLHIP_LB_NOIMG")) u.wimg = nullptr;                          // timing experiment only: stale images
  u.n_peer = 0;
  u.peer_direct = 0;
  for (int r = 0; r < IQLHIP_MAX_WORLD; ++r) { u.peer_flat[r] = nullptr; u.peer_slab_b[r] = nullptr; u.peer_loss[r] = nullptr; }
  return u;
}

static size_t fwd_lds(const iqlhip_ctx* c, int n_blocks) { return (n_blocks <= c->n_cus) ? c->lds_fwd_solo : c->lds_fwd; }

// The training forward of a chunk kind: every one takes a StepParams.  Defined at the end of the file, behind the last
// kind's selector — the selectors stand where their kernels are to lie in the code object (with_bools).
static const void* fwd_kernel_of(ChunkKind kind, bool bf, bool dma, bool multi);
// iql_fwd_kernel_early takes the plain one-slice fp32 training forward whenever its premises hold: every instance
// stages W0 in LDS through registers (state_dim + action_dim <= FWD_EARLY_MAX_K and staged), a packed row tile is at most
// three float4 per thread, and the arenas are laid out as the kernel restates them from the dims.
// Once per context (iqlhip_create): the dims fit the packed words, and iqlhip_arena_layout's result is what arena_off
// (csrc/iqlhip_kernels.h) computes — W1 leads a net's segment, then W0, b0, b1, W2, b2; segments V, Q1, Q2, pi, each
// rounded up to 64 floats.  (The layout is stated three times: iqlhip_arena_layout, arena_off for the kernels with
// preloaded arguments, and here, where the first two are held against each other.)
extern "C" int64_t iqlhip_debug_fwd_early_launches(const iqlhip_ctx* ctx) {
  return ctx ? ctx->fwd_early_launches.load(std::memory_order_relaxed) : -1;
}
static bool fwd_early_layout_ok(const iqlhip_ctx* c) {
  const iqlhip_layout& L = c->L;
  const int S = c->dims.state_dim, A = c->dims.action_dim, kq = S + A;
  if (kq > FWD_EARLY_MAX_K || kq > c->w0_lds_k || c->w0_lds_k > W0_LDS_MAX_K) return false;
  if (RT_ROWS * c->row_ld / 4 > 3 * 256 || S > 255 || A > 63 || c->row_ld > 1023) return false;      // (the packed words' fields)
  long long begin = 0;
  for (int n = 0; n < 4; ++n) {
    const iqlhip_net_layout& nl = L.net[n];
    const long long k0 = nl.k_in, d = nl.d_out;
    if (k0 != ((n == IQLHIP_NET_Q1 || n == IQLHIP_NET_Q2) ? kq : S) || d != (n == IQLHIP_NET_PI ? A : 1)) return false;
    if (nl.seg_begin != begin || nl.w1 != begin || nl.w0 != begin + 65536 || nl.b0 != nl.w0 + 256 * k0 || nl.b1 != nl.b0 + 256 ||
        nl.w2 != nl.b1 + 256 || nl.b2 != nl.w2 + 256 * d)
      return false;
    const long long seg_n = (65536 + 256 * k0 + 512 + 256 * d + ((d + 3) & ~3LL) + 63) & ~63LL;      // (V, Q1, Q2: no log_std)
    if (n != IQLHIP_NET_PI && nl.seg_end != begin + seg_n) return false;
    begin = nl.seg_end;
  }
  return true;
}
// Per launch: the kind of step, and the instance table of `p` being the context's own arenas (the kernel forms every
// weight address from the two arena pointers).
static bool fwd_early_ok(const iqlhip_ctx* c, const StepParams& p, ChunkKind kind, bool bf, bool dma, bool multi) {
  if (!c->fwd_early || !c->fwd_early_layout || kind != ChunkKind::Plain || bf || dma || multi || p.only_inst >= 0) return false;
  if (p.S != c->dims.state_dim || p.A != c->dims.action_dim || p.ld != (int)c->row_ld || p.rows >= (1 << 22)) return false;
  const float* tb = c->target - c->L.target_src;
  const int netof[7] = {IQLHIP_NET_V, IQLHIP_NET_V, IQLHIP_NET_Q1, IQLHIP_NET_Q2, IQLHIP_NET_Q1, IQLHIP_NET_Q2, IQLHIP_NET_PI};
  for (int i = 0; i < 7; ++i)
    if (p.inst[i].w1 != ((i == 2 || i == 3) ? tb : c->params) + c->L.net[netof[i]].w1) return false;
  return true;
}
static void launch_fwd_grid(const iqlhip_ctx* c, const StepParams& p, int nb, hipStream_t st, ChunkKind kind = ChunkKind::Plain) {
  const bool dma = c->w0_lds_k > W0_LDS_MAX_K;       // some instance stages wide layer-0 weights by LDS-DMA
  const bool bf = c->precision == 1, multi = (p.spb_l2 & 3) > 0;
  if (fwd_early_ok(c, p, kind, bf, dma, multi)) {
    // leading arguments, preloaded into SGPRs with each wave (build: -mllvm -amdgpu-kernarg-preload-count=14)
    const float* q_params = c->params;
    const float* q_target = c->target - c->L.target_src;
    const float* q_xb = p.xb;
    const unsigned* q_drop = p.drop_bits;
    unsigned q_dims = (unsigned)p.S | ((unsigned)p.A << 8) | ((unsigned)p.policy << 14);
    unsigned q_ldB = (unsigned)p.ld | ((unsigned)p.rows << 10);
    unsigned q_mb = (unsigned)p.sc.max_batch;
    void* args[] = {&q_params, &q_target, &q_xb, &q_drop, &q_dims, &q_ldB, &q_mb, const_cast<StepParams*>(&p)};
    (void)hipLaunchKernel((const void*)&iql_fwd_kernel_early, dim3(nb), dim3(256), args, fwd_lds(c, nb), st);
    c->fwd_early_launches.fetch_add(1, std::memory_order_relaxed);
    return;
  }
  // (policy inference — iqlhip_actor_forward — has its own instantiations)
  const void* kernel = (p.only_inst >= 0) ? (const void*)fwd_one_kernel(bf, dma) : fwd_kernel_of(kind, bf, dma, multi);
  void* args[] = {const_cast<StepParams*>(&p)};
  (void)hipLaunchKernel(kernel, dim3(nb), dim3(256), args, fwd_lds(c, nb), st);
}
// The dynamic-LDS allowance of a kind's forward instantiations, once per context: at the kind's first call, from its
// argument check (the plain family has it from the context's creation).
static int ensure_fwd_lds(iqlhip_ctx* c, ChunkKind kind) {
  if (c->fwd_lds_set[(int)kind]) return IQLHIP_OK;
  DevGuard guard(c->device);
  if (int rc = set_max_lds(3, c->lds_fwd_solo, [kind](unsigned m) { return fwd_kernel_of(kind, m & 1, m & 2, m & 4); })) return rc;
  c->fwd_lds_set[(int)kind] = true;
  return IQLHIP_OK;
}

// Column slices per forward block (log2).  One block per (instance, row tile, slice) while that grid fits the chip in
// one round; beyond it every extra round costs a whole block time (prologue + layer 0 + one slice), so blocks take 2
// or 4 slices each — layer 0 and the prologue are then paid once per 2 / 4 slices (profiles/r02_slices_per_block.txt).
static int fwd_spb_l2(const iqlhip_ctx* c, int n_rt) {
  if (c->fwd_spb_force >= 0) return c->fwd_spb_force;
  // (two blocks sharing a CU each run ~1.8x slower — a second block per CU counts as no extra slot)
  if (8 * n_rt * NSPLIT <= c->n_cus) return 0;
  if (8 * n_rt * 2 <= c->n_cus) return 1;
  return 2;
}
// Blocks of a forward grid (per agent) over n_rt row tiles at 2^l2 slices per block.  (Full-width blocks: each XCD of
// a net's pair takes the row tiles of one parity — iql_fwd_kernel's block map.)
static int fwd_blocks(int n_rt, int l2) { return (l2 == 2) ? 8 * 2 * ((n_rt + 1) / 2) : 8 * n_rt * (NSPLIT >> l2); }
static void launch_fwd(const iqlhip_ctx* c, const StepParams& p_in, hipStream_t st, ChunkKind kind = ChunkKind::Plain) {
  StepParams p = p_in;
  if (p.only_inst < 0 && use_lb(c, p.rows)) {
    const LbArgs a = lb_args(c, p.rows);
    const int kq = c->dims.state_dim + c->dims.action_dim;
    const dim3 grid(8 * a.nbi);
    // (the policy's tiles over its own and the idle blocks, iql_fwd_lb_kernel: from 3 tiles per block on the idle block takes 3 / 8 of them)
    const bool spread = a.n_rt > 2 * a.nbi && c->lb_pi_spread;
    if (spread) {
      if (kq <= 32) hipLaunchKernelGGL((iql_fwd_lb_kernel<1, true>), grid, dim3(256), 0, st, p, a);
      else if (kq <= 64) hipLaunchKernelGGL((iql_fwd_lb_kernel<2, true>), grid, dim3(256), 0, st, p, a);
      else hipLaunchKernelGGL((iql_fwd_lb_kernel<3, true>), grid, dim3(256), 0, st, p, a);
    } else {
      if (kq <= 32) hipLaunchKernelGGL((iql_fwd_lb_kernel<1, false>), grid, dim3(256), 0, st, p, a);
      else if (kq <= 64) hipLaunchKernelGGL((iql_fwd_lb_kernel<2, false>), grid, dim3(256), 0, st, p, a);
      else hipLaunchKernelGGL((iql_fwd_lb_kernel<3, false>), grid, dim3(256), 0, st, p, a);
    }
    return;
  }
  const int n_rt = (p.rows + RT_ROWS - 1) / RT_ROWS;
  p.spb_l2 = fwd_spb_l2(c, n_rt);
  launch_fwd_grid(c, p, fwd_blocks(n_rt, p.spb_l2), st, kind);
}
// Column slices per (b) block of the backward (log2): one while the whole grid — 4 nets x (32 dW1 tiles per 256-row
// chunk + 4 slices per row tile) — is at most two rounds of the chip (up to 512 rows: measured equal or better), else 4:
// the row tile's dY / dH1 tile is built once and the block's W1 fragments stream in under its MFMAs
// (profiles/r02_slices_per_block.txt).
static int bwd_spb_l2(const iqlhip_ctx* c, int n_chunk, int n_rt) {
  if (c->bwd_spb_force >= 0) return c->bwd_spb_force;
  return (4 * (32 * n_chunk + 4 * n_rt) <= 2 * c->n_cus) ? 0 : 2;
}
// Blocks of a backward grid (per agent): per net 32 dW1 tiles per chunk + the (b) blocks of 2^l2 slices per row tile,
// two nets per XCD pair, + the policy's n_don donated dW1 tiles at the ends of the scalar nets' queues.
static int bwd_blocks(int n_chunk, int n_rt, int l2, int n_don) {
  const int per_net = 32 * n_chunk + (4 >> l2) * n_rt;
  return 8 * ((per_net + 1) / 2 + (n_don + 5) / 6);
}
// The backward's leading arguments: preloaded into SGPRs with each wave (build: -mllvm -amdgpu-kernarg-preload-count=14),
// what a block needs to issue its first loads, see iql_bwd_kernel.  (GroupRec carries the same words per agent.)
struct BwdWords { const float *heads, *xb, *h1, *h0, *params; unsigned dims, ldB, mbc, rts; };
static BwdWords bwd_words(const iqlhip_ctx* c, const StepParams& p, int n_chunk, int n_rt, unsigned spb_l2) {
  BwdWords w;
  w.heads = p.sc.heads; w.xb = p.xb; w.h1 = p.sc.h1; w.h0 = p.sc.h0; w.params = c->params;
  w.dims = (unsigned)p.S | ((unsigned)p.A << 8) | ((unsigned)p.policy << 14);
  w.ldB = (unsigned)p.ld | ((unsigned)p.rows << 10);
  w.mbc = (unsigned)p.sc.max_batch | ((unsigned)n_chunk << 16);
  w.rts = (unsigned)n_rt | (spb_l2 << 10);
  return w;
}
// rw (iqlhip_step_rw): the step's per-row loss weights and, nullable, where its TD errors go — the row-weighted kernel;
// its callers have refused bf16 and the large-batch path.
struct RowWeights { const float* w; float* td; };
static void launch_bwd(const iqlhip_ctx* c, const StepParams& p_in, hipStream_t st, const RowWeights* rw = nullptr) {
  StepParams p = p_in;
  if (use_lb(c, p.rows)) {
    const LbArgs a = lb_args(c, p.rows);
    const int kq = c->dims.state_dim + c->dims.action_dim;
    (void)kq;
    if (c->lb_bwd_part != 2) {
      const bool csplit = lb_geom(c, p.rows).csplit;
      hipLaunchKernelGGL(bwd_rows_kernel(csplit), dim3(8 * (csplit ? a.nbb : a.nbb / 2)), dim3(256), c->lds_bwd_lb, st, p, a);
    }
    if (c->lb_bwd_part != 1)
      hipLaunchKernelGGL(iql_bwd_gemm_kernel, dim3(8 * ((LB_NJOB * a.n_cg + 1 + 1) / 2)), dim3(256), 0, st, p, a);      // (+ 1: the reduction job)
    return;
  }
  const int n_rt = (p.rows + RT_ROWS - 1) / RT_ROWS;
  const int n_chunk = (p.rows + CHUNK_ROWS - 1) / CHUNK_ROWS;
  int l2 = bwd_spb_l2(c, n_chunk, n_rt);
  if (c->precision == 1 && l2 > 0) l2 = 2;      // bf16, large batches: a (b) block takes the whole row tile in one pass
  // multi-round launches: this many of the policy's dW1-tile blocks run at the ends of the scalar nets' XCD queues
  // (iql_bwd_kernel); share of its 32 n_chunk tiles tuned on obs 17 / act 6 and obs 39 / act 28 (profiles/r02_slices_per_block.txt)
  // Measured optimum of the share: 50 % at 28 action dims (1 024 rows 37.6 -> 30.8 us, bf16 32.7 -> 24.3; 2 048 rows
  // 76.0 -> 59.1), 30 % at 6-8 action dims (1 024 rows 28.7 -> 26.5); in between: linear in the action dims.
  int n_don = 0;
  if (l2 > 0) {
    const int pct = (c->bwd_donate_pct >= 0) ? c->bwd_donate_pct : std::max(30, std::min(50, 22 + c->dims.action_dim));
    n_don = std::min(32 * n_chunk, (32 * n_chunk * pct + 50) / 100);
  }
  p.spb_l2 = (l2 << 2) | (n_don << 8);
  const bool full = (p.rows % CHUNK_ROWS) == 0;      // every tile of every block lies inside the batch: no clamps
  const BwdWords w = bwd_words(c, p, n_chunk, n_rt, (unsigned)p.spb_l2);
  if (rw) {
    hipLaunchKernelGGL(bwd_rw_kernel(full, /*multi=*/l2 > 0), dim3(bwd_blocks(n_chunk, n_rt, l2, n_don)), dim3(256), c->lds_bwd, st,
                       w.heads, w.xb, w.h1, w.h0, w.params, w.dims, w.ldB, w.mbc, w.rts, p, rw->w, rw->td);
    return;
  }
  hipLaunchKernelGGL(bwd_kernel(c->precision == 1, full, /*multi=*/l2 > 0), dim3(bwd_blocks(n_chunk, n_rt, l2, n_don)), dim3(256),
                     c->lds_bwd, st, w.heads, w.xb, w.h1, w.h0, w.params, w.dims, w.ldB, w.mbc, w.rts, p);
}
static unsigned drop_thresh(float p) {
  const double t = (double)p * 4294967296.0;
  return t >= 4294967295.0 ? 0xFFFFFFFFu : (unsigned)t;
}

// The keep-bit draw of one inference call on `rows` rows at the context's current position (active = 0: rate 0,
// nothing is drawn and the position stays).
static ActDropRec act_drop_record(const iqlhip_ctx* c, int rows) {
  ActDropRec d;
  memset(&d, 0, sizeof d);
  d.active = (c->act_drop_p > 0.f && rows > 0) ? 1 : 0;
  if (!d.active) return d;
  d.bits = c->act_drop_bits;
  d.n_rows = rows;
  d.cap = c->act_cap;
  d.thresh = drop_thresh(c->act_drop_p);
  d.seed = c->act_drop_seed;
  d.call = c->act_drop_calls;
  return d;
}

static void launch_dropmask(const iqlhip_ctx* c, unsigned long long seed, unsigned long long step,
                            const unsigned long long* hdr, int k, hipStream_t st) {
  const int n_words = 2 * c->dims.max_batch * 8;
  hipLaunchKernelGGL(iql_dropmask_kernel, dim3((n_words + 255) / 256), dim3(256), 0, st, c->drop_bits, n_words,
                     drop_thresh(c->drop_p), seed, step, hdr, k);
}

// Blocks of an update grid (per agent): 8 x the 2 048-float windows of the longest net segment (iql_update_kernel's
// XCD-affine element map).
static int upd_blocks(const iqlhip_ctx* c) {
  long long seg_max = 0;
  for (int n = 0; n < 4; ++n) {
    const long long end = (n < 3) ? c->L.net[n + 1].seg_begin : c->L.n_params;
    seg_max = std::max(seg_max, end - c->L.net[n].seg_begin);
  }
  return 8 * (int)((seg_max + 2047) / 2048);
}
// The update's leading arguments behind its four arena pointers: preloaded into SGPRs with each wave (iql_update_kernel).
// (GroupRec carries the same words per agent.)
struct UpdWords { unsigned s0, s1, s2, s3, end, flags; };
static UpdWords upd_words(const iqlhip_ctx* c, const UpdParams& u) {
  UpdWords w;
  w.s0 = (unsigned)c->L.net[0].seg_begin; w.s1 = (unsigned)c->L.net[1].seg_begin; w.s2 = (unsigned)c->L.net[2].seg_begin;
  w.s3 = (unsigned)c->L.net[3].seg_begin; w.end = (unsigned)c->L.net[3].seg_end;
  w.flags = (u.n_peer == 0 && !u.flat_grads && !u.slab_x && u.n_chunk == 1) ? UPD_EARLY_G : 0u;
  return w;
}
// (true before false in this family and the next, LB outermost: hence the negated flags, see with_bools)
static auto upd_kernel(bool from_table, bool peer, bool lb) {
  return with_bools([](auto NLB, auto NT, auto NP) { return &iql_update_kernel<!NT.value, !NP.value, !NLB.value>; }, !lb, !from_table, !peer);
}
// clip: the step's clip coefficients (iqlhip_set_grad_clip) — the CLIP kernel; nullptr: the kernels without.
static void launch_upd(const iqlhip_ctx* c, UpdParams u, hipStream_t st, const float* clip = nullptr) {
  const UpdWords w = upd_words(c, u);
  if (clip) {       // (never with an exchange or on the large-batch path: clip_check)
    if (u.sched) hipLaunchKernelGGL(iql_update_clip_kernel<true>, dim3(upd_blocks(c)), dim3(256), 0, st, u.params, u.m, u.v, u.slab_a,
                                    w.s0, w.s1, w.s2, w.s3, w.end, w.flags, clip, u);
    else hipLaunchKernelGGL(iql_update_clip_kernel<false>, dim3(upd_blocks(c)), dim3(256), 0, st, u.params, u.m, u.v, u.slab_a,
                            w.s0, w.s1, w.s2, w.s3, w.end, w.flags, clip, u);
    return;
  }
  // (u.slab_x: a large-batch bf16 step — the LB instantiations: gradient from the chunk-group slabs unless an exchange
  //  delivered it flat; the operand images of W0 / W1 written next to the bf16 shadows)
  hipLaunchKernelGGL(upd_kernel(/*from_table=*/u.sched != nullptr, /*peer=*/u.n_peer > 0, /*lb=*/u.slab_x != nullptr), dim3(upd_blocks(c)),
                     dim3(256), 0, st, u.params, u.m, u.v, u.slab_a, w.s0, w.s1, w.s2, w.s3, w.end, w.flags, u);
}

// bf16 path: rebuild the bf16 shadows from the fp32 masters (the caller owns the masters and may have written them
// through its own tensors — load_state_dict, a broadcast — since the last update kernel kept the shadows current).
static void refresh_shadows(const iqlhip_ctx* c, hipStream_t st) {
  if (c->precision != 1) return;
  const long long n = std::max<long long>(c->L.n_params, c->L.n_target);
  hipLaunchKernelGGL(iql_shadow_refresh_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, c->params, c->target,
                     c->wsh, c->tsh, (long long)c->L.n_params, (long long)c->L.n_target, c->L, c->wimg);
}

static auto flatten_kernel(bool sys, bool lb) {
  return with_bools([](auto NLB, auto NSYS) { return &iql_grad_flatten_kernel<!NSYS.value, !NLB.value>; }, !lb, !sys);
}
static void launch_flatten(const iqlhip_ctx* c, const UpdParams& u, float* out, bool sys, hipStream_t st) {
  const int nb = (int)((c->L.n_params / 4 + 255) / 256);
  hipLaunchKernelGGL(flatten_kernel(sys, /*lb=*/u.slab_x != nullptr), dim3(nb), dim3(256), 0, st, u, out);
}

// A read-back: `bytes` from device memory into the pinned landing pad `pin` on `st`; sync: wait for the stream and, with
// dst_host, copy them out.  (sync = false queues the copy only: callers with several pieces synchronise once.)
static int read_back(void* dst_host, void* pin, const void* dev, size_t bytes, hipStream_t st, bool sync = true) {
  HIPCHK(hipMemcpyAsync(pin, dev, bytes, hipMemcpyDeviceToHost, st));
  if (!sync) return IQLHIP_OK;
  HIPCHK(hipStreamSynchronize(st));
  if (dst_host) memcpy(dst_host, pin, bytes);
  return IQLHIP_OK;
}

// ---------------------------------------------------------------------------
// Per-step statistics (include/iqlhip.h "per-step training statistics"; kernels: iqlhip_kernels.h).
static int stats_parts(const iqlhip_ctx* c) { return upd_blocks(c) / 8 * 2; }      // 1024-element windows of the longest segment
// The gradient block partials: one buffer for the statistics and the clip kernel (whoever is enabled first).
static int ensure_gparts(iqlhip_ctx* c) {
  if (c->stats_part) return IQLHIP_OK;
  c->stats_n_part = stats_parts(c);
  HIPCHK(c->own.dev(&c->stats_part, (size_t)4 * c->stats_n_part * sizeof(float), 0));
  return IQLHIP_OK;
}
extern "C" int iqlhip_set_step_stats(iqlhip_ctx* c, int enabled) {
  if (!c) return fail(IQLHIP_EINVAL, "NULL ctx");
  if (enabled && !c->stats_ring) {
    DevGuard guard(c->device);
    const int rc = all_or_nothing(c->own, [&]() -> int {
      const size_t ring = (size_t)c->k_max * IQLHIP_N_STATS * sizeof(float);
      if (int rc_g = ensure_gparts(c)) return rc_g;
      HIPCHK(c->own.dev(&c->stats_last, IQLHIP_N_STATS * sizeof(float), 0));
      HIPCHK(c->own.pin(&c->stats_host, ring));
      HIPCHK(c->own.dev(&c->stats_ring, ring, 0));
      return IQLHIP_OK;
    });
    if (rc) return rc;
  }
  c->stats_on = enabled != 0;
  return IQLHIP_OK;
}
// The two cases the opt-in features that look at a step's gradient are not built for.  Statistics: the local slabs are
// not what Adam receives after an exchange; clipping: the norm would have to be taken after it; and the large-batch
// path keeps its gradient in other slabs.
static int optional_features_check(const iqlhip_ctx* c, int rows) {
  const struct { bool on; const char* what; const char* xch_reason; } features[] = {
      {c->clip_on, "gradient clipping is", "the norm would have to be taken after the exchange"},
      {c->stats_on, "step statistics are", "the local gradient slabs are not what Adam receives"}};
  for (const auto& f : features) {
    if (!f.on) continue;
    if (c->xch_mode != IQLHIP_XCH_NONE)
      return fail(IQLHIP_EUNSUPPORTED, "%s not supported with a data-parallel exchange (%s)", f.what, f.xch_reason);
    if (use_lb(c, rows))
      return fail(IQLHIP_EUNSUPPORTED, "%s not supported on the large-batch bf16 path (more than %d rows)", f.what, LB_MIN_ROWS);
  }
  return IQLHIP_OK;
}
static int inject_check(const iqlhip_ctx* c);
// The last check of every solo step entry point, before anything is launched or any counter moves: the opt-in features
// (and, for the multi-step driver, pending injected masks); then the stream its work is queued on is remembered.
// (The group entry points: group_check_call.)
static void note_stream(iqlhip_ctx* c, void* stream) { c->last_stream = (hipStream_t)stream; c->has_last_stream = true; }
static int step_entry(iqlhip_ctx* c, int rows, void* stream, bool multi_step) {
  int rc = optional_features_check(c, rows);
  if (!rc && multi_step) rc = inject_check(c);
  if (!rc) note_stream(c, stream);
  return rc;
}
// The statistics launches' arguments for a step described by `p`; ring == nullptr: the eager steps (stats_last only).
static StatsArgs make_stats(const iqlhip_ctx* c, const StepParams& p, float* ring, int ring_slot, int ring_cap,
                            const unsigned long long* ring_hdr) {
  StatsArgs a;
  memset(&a, 0, sizeof a);
  a.heads = p.sc.heads; a.xb = p.xb; a.ld = p.ld; a.rows = p.rows; a.rd_off = 2 * p.S + p.A;
  a.beta = p.hy.beta; a.discount = p.hy.discount; a.exp_adv_max = p.hy.exp_adv_max;
  a.gparts = c->stats_part; a.n_part = c->stats_n_part;
  a.last = c->stats_last;
  a.ring = ring; a.ring_slot = ring_slot; a.ring_cap = ring_cap; a.ring_hdr = ring_hdr;
  return a;
}
static ClipArgs make_clip(const iqlhip_ctx* c) {
  ClipArgs a;
  a.gparts = c->stats_part; a.n_part = c->stats_n_part;
  a.limits = c->clip_dev; a.coef = c->clip_dev + 4; a.norm = c->clip_dev + 8;
  return a;
}
// The launches between a step's backward and its update: the block partials once for both consumers, then the
// statistics kernel (sa) and the clip coefficients (clip).
static void launch_stats(const iqlhip_ctx* c, const UpdParams& u, const StatsArgs* sa, bool clip, hipStream_t st) {
  if (!sa && !clip) return;
  hipLaunchKernelGGL(iql_stats_gradsq_kernel, dim3(4 * c->stats_n_part), dim3(256), 0, st, u, c->stats_part, c->stats_n_part);
  if (sa) hipLaunchKernelGGL(iql_step_stats_kernel, dim3(1), dim3(256), 0, st, *sa);
  if (clip) hipLaunchKernelGGL(iql_clip_coef_kernel, dim3(1), dim3(256), 0, st, make_clip(c));
}
extern "C" int iqlhip_read_step_stats(iqlhip_ctx* c, float out[IQLHIP_N_STATS], void* stream) {
  if (!c || !out) return fail(IQLHIP_EINVAL, "NULL argument");
  if (!c->stats_on) return fail(IQLHIP_EINVAL, "step statistics are off (iqlhip_set_step_stats)");
  DevGuard guard(c->device);
  return read_back(out, c->stats_host, c->stats_last, IQLHIP_N_STATS * sizeof(float), (hipStream_t)stream);
}
extern "C" int iqlhip_read_stats_ring(iqlhip_ctx* c, float* out, int32_t n_steps, void* stream) {
  if (!c || !out) return fail(IQLHIP_EINVAL, "NULL argument");
  if (!c->stats_on) return fail(IQLHIP_EINVAL, "step statistics are off (iqlhip_set_step_stats)");
  if (n_steps < 1 || n_steps > c->k_max) return fail(IQLHIP_EINVAL, "n_steps outside [1,%d]", c->k_max);
  DevGuard guard(c->device);
  return read_back(out, c->stats_host, c->stats_ring, (size_t)n_steps * IQLHIP_N_STATS * sizeof(float), (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// Gradient-norm clipping (include/iqlhip.h "gradient-norm clipping"; kernels: iqlhip_kernels.h).
extern "C" int iqlhip_set_grad_clip(iqlhip_ctx* c, const float max_norm[3]) {
  if (!c || !max_norm) return fail(IQLHIP_EINVAL, "NULL argument");
  float lim[3];
  bool on = false;
  for (int g = 0; g < 3; ++g) {
    if (max_norm[g] != max_norm[g]) return fail(IQLHIP_EINVAL, "max_norm[%d] is NaN", g);
    lim[g] = (max_norm[g] > 0.f) ? max_norm[g] : __builtin_inff();      // (<= 0 and +inf: no limit)
    on = on || lim[g] < __builtin_inff();
  }
  if (on || c->clip_dev) {
    DevGuard guard(c->device);
    const bool first = !c->clip_dev;
    if (first) {
      const int rc = all_or_nothing(c->own, [&]() -> int {
        if (int rc_g = ensure_gparts(c)) return rc_g;
        HIPCHK(c->own.pin(&c->clip_host, 24 * sizeof(float)));
        HIPCHK(c->own.dev(&c->clip_dev, 12 * sizeof(float)));
        HIPCHK(c->own.event(&c->clip_up, hipEventDisableTiming));
        return IQLHIP_OK;
      });
      if (rc) return rc;
    }
    // The limits (and, the first time, zeros for the rest of clip_dev) travel from pinned memory on the stream of the
    // context's last step call: behind the steps queued there, in front of every later one, without stalling the
    // device.  (A caller that moves to another stream orders the two itself, as for the arenas.)  No step call yet:
    // nothing of this context is queued, a blocking copy.
    if (c->clip_up_pending) HIPCHK(hipEventSynchronize(c->clip_up));      // (the staging words are free again)
    c->clip_up_pending = false;
    memset(c->clip_host, 0, 12 * sizeof(float));
    for (int g = 0; g < 3; ++g) c->clip_host[g] = lim[g];
    const size_t bytes = (first ? 12 : 3) * sizeof(float);
    if (c->has_last_stream) {
      HIPCHK(hipMemcpyAsync(c->clip_dev, c->clip_host, bytes, hipMemcpyHostToDevice, c->last_stream));
      HIPCHK(hipEventRecord(c->clip_up, c->last_stream));
      c->clip_up_pending = true;
    } else {
      HIPCHK(hipMemcpy(c->clip_dev, c->clip_host, bytes, hipMemcpyHostToDevice));
    }
  }
  for (int g = 0; g < 3; ++g) c->clip_max[g] = lim[g];
  c->clip_on = on;
  return IQLHIP_OK;
}
extern "C" int iqlhip_get_grad_clip(const iqlhip_ctx* c, float max_norm[3]) {
  if (!c || !max_norm) return fail(IQLHIP_EINVAL, "NULL argument");
  for (int g = 0; g < 3; ++g) max_norm[g] = c->clip_max[g];
  return IQLHIP_OK;
}
extern "C" int iqlhip_read_grad_clip(iqlhip_ctx* c, float out[6], void* stream) {
  if (!c || !out) return fail(IQLHIP_EINVAL, "NULL argument");
  if (!c->clip_on) return fail(IQLHIP_EINVAL, "gradient clipping is off (iqlhip_set_grad_clip)");
  DevGuard guard(c->device);
  float* land = c->clip_host + 12;
  if (int rc = read_back(nullptr, land, c->clip_dev, 12 * sizeof(float), (hipStream_t)stream)) return rc;
  for (int g = 0; g < 3; ++g) { out[g] = land[8 + g]; out[3 + g] = land[4 + g]; }
  return IQLHIP_OK;
}

// ---------------------------------------------------------------------------
// Gradient exchange between the ranks of a data-parallel group (include/iqlhip.h, "data-parallel gradient exchange").
static RcclApi g_rccl;

static int rccl_load() {
  if (g_rccl.lib) return IQLHIP_OK;
  void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);      // the copy the process already has (PyTorch-ROCm's)
  if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
  if (!h) h = dlopen("librccl.so.1", RTLD_NOW);
  if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW);
  if (!h) return fail(IQLHIP_EHIP, "librccl.so.1 not found: %s", dlerror());
  RcclApi a;
  a.lib = h;
  a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(h, "ncclGetUniqueId");
  a.CommInitRank = (decltype(a.CommInitRank))dlsym(h, "ncclCommInitRank");
  a.CommDestroy = (decltype(a.CommDestroy))dlsym(h, "ncclCommDestroy");
  a.AllReduce = (decltype(a.AllReduce))dlsym(h, "ncclAllReduce");
  a.GetErrorString = (decltype(a.GetErrorString))dlsym(h, "ncclGetErrorString");
  if (!a.GetUniqueId || !a.CommInitRank || !a.CommDestroy || !a.AllReduce)
    return fail(IQLHIP_EHIP, "librccl.so.1 lacks an expected symbol");
  g_rccl = a;
  return IQLHIP_OK;
}
#define NCCLCHK(expr)                                                                              \
  do {                                                                                             \
    int r_ = (expr);                                                                               \
    if (r_ != 0)                                                                                   \
      return fail(IQLHIP_EHIP, "%s failed: %s", #expr, g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "rccl error"); \
  } while (0)
enum { RCCL_FLOAT32 = 7, RCCL_SUM = 0 };     // ncclFloat32, ncclSum (rccl.h)

extern "C" int iqlhip_comm_unique_id(void* id_out) {
  if (!id_out) return fail(IQLHIP_EINVAL, "NULL argument");
  int rc = rccl_load();
  if (rc) return rc;
  NCCLCHK(g_rccl.GetUniqueId(id_out));
  return IQLHIP_OK;
}

extern "C" int iqlhip_allreduce_init(iqlhip_ctx* c, const void* unique_id, int rank, int world) {
  if (!c || !unique_id) return fail(IQLHIP_EINVAL, "NULL argument");
  if (world < 1 || rank < 0 || rank >= world) return fail(IQLHIP_EINVAL, "rank %d outside world %d", rank, world);
  if (c->p2p_attached && (world != c->world || rank != c->rank))
    return fail(IQLHIP_EINVAL, "rank/world differ from the attached P2P exchange");
  int rc = rccl_load();
  if (rc) return rc;
  DevGuard guard(c->device);
  if (c->nccl_comm) { (void)g_rccl.CommDestroy(c->nccl_comm); c->nccl_comm = nullptr; }
  RcclId id;
  memcpy(&id, unique_id, sizeof id);
  NCCLCHK(g_rccl.CommInitRank(&c->nccl_comm, world, id, rank));
  c->rank = rank;
  c->world = world;
  c->xch_mode = IQLHIP_XCH_RCCL;
  drop_graph(c);
  return IQLHIP_OK;
}

extern "C" int iqlhip_p2p_export(iqlhip_ctx* c, void* handle_out, int rank, int world) {
  if (!c || !handle_out) return fail(IQLHIP_EINVAL, "NULL argument");
  if (world < 1 || world > IQLHIP_MAX_WORLD || rank < 0 || rank >= world)
    return fail(IQLHIP_EINVAL, "rank %d / world %d outside [0, %d]", rank, world, IQLHIP_MAX_WORLD);
  if (c->nccl_comm && (world != c->world || rank != c->rank))
    return fail(IQLHIP_EINVAL, "rank/world differ from the RCCL communicator");
  if (getenv("IQLHIP_P2P_DISABLE"))     // diagnostic: lets the callers' fallback paths be exercised on any machine
    return fail(IQLHIP_EUNSUPPORTED, "the peer-to-peer exchange is disabled (IQLHIP_P2P_DISABLE)");
  DevGuard guard(c->device);
  if (!c->xblk) {
    const size_t flags_b = 4096;                                     // IQLHIP_MAX_WORLD x 128-B flag lines, padded
    const size_t flat_b = (size_t)up((c->L.n_params + 4) * (int64_t)sizeof(float), 4096);
    size_t sb = 0;                                                   // w0 / b0 partial slabs of <= 8 row tiles (<= 256 rows)
    for (int n = 0; n < 4; ++n) {
      c->xslab_b_off[n] = (long long)sb;
      sb += (size_t)8 * ((size_t)HID * c->L.net[n].k_in + HID);
    }
    const size_t slabb_b = (size_t)up((int64_t)(sb * sizeof(float)), 4096);
    const size_t loss_b = 4096;
    const size_t buf_b = flat_b + slabb_b + loss_b;
    for (int k = 0; k < 2; ++k) {
      c->xflat_off[k] = flags_b + (size_t)k * buf_b;
      c->xslabb_off[k] = c->xflat_off[k] + flat_b;
      c->xloss_off[k] = c->xslabb_off[k] + slabb_b;
    }
    c->xblk_bytes = flags_b + 2 * buf_b;
    // Coarse-grained device memory by default: the backward's plain stores into this block are complete AND written
    // back to the device's memory at the kernel boundary in front of the flag kernel (dirty L2 lines leave at a
    // boundary), and every peer reads them with system-scope loads that bypass its own caches — the data a peer can
    // see is in this device's HBM before the flag that announces it is stored.  IQLHIP_P2P_FINEGRAINED=1 allocates the
    // block fine-grained instead (no reliance on the boundary write-back; slower stores) where the runtime can export
    // such memory through hipIpc; the replicas-equal check of the callers is the gate either way.
    hipError_t ea = hipErrorUnknown;
    if (getenv("IQLHIP_P2P_FINEGRAINED")) ea = hipExtMallocWithFlags((void**)&c->xblk, c->xblk_bytes, hipDeviceMallocFinegrained);
    if (ea != hipSuccess) { (void)hipGetLastError(); HIPCHK(hipMalloc((void**)&c->xblk, c->xblk_bytes)); }
    HIPCHK(hipMemset(c->xblk, 0, c->xblk_bytes));
    HIPCHK(hipDeviceSynchronize());
  } else {
    // a second attach: every rank clears its OWN flag lines here, before the handles are exchanged (the callers'
    // all-gather is the barrier), so no stale flag of an earlier group satisfies the first waits of the new one
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemset(c->xblk, 0, 4096));
    HIPCHK(hipDeviceSynchronize());
  }
  hipIpcMemHandle_t h;
  static_assert(sizeof(hipIpcMemHandle_t) == IQLHIP_IPC_HANDLE_BYTES, "hipIpcMemHandle_t size");
  HIPCHK(hipIpcGetMemHandle(&h, c->xblk));
  memcpy(handle_out, &h, sizeof h);
  c->rank = rank;
  c->world = world;
  return IQLHIP_OK;
}

static void p2p_close(iqlhip_ctx* c) {
  for (int r = 0; r < IQLHIP_MAX_WORLD; ++r) {
    if (c->peer_blk[r] && c->peer_blk[r] != c->xblk) (void)hipIpcCloseMemHandle(c->peer_blk[r]);
    c->peer_blk[r] = nullptr;
  }
  c->p2p_attached = false;
}

extern "C" int iqlhip_p2p_attach(iqlhip_ctx* c, const void* handles, int timeout_ms) {
  if (!c || !handles) return fail(IQLHIP_EINVAL, "NULL argument");
  if (!c->xblk) return fail(IQLHIP_EINVAL, "iqlhip_p2p_export has not been called");
  DevGuard guard(c->device);
  p2p_close(c);
  for (int r = 0; r < c->world; ++r) {
    if (r == c->rank) { c->peer_blk[r] = c->xblk; continue; }
    hipIpcMemHandle_t h;
    memcpy(&h, (const char*)handles + (size_t)r * IQLHIP_IPC_HANDLE_BYTES, sizeof h);
    void* ptr = nullptr;
    hipError_t e = hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {
      p2p_close(c);
      return fail(IQLHIP_EHIP, "hipIpcOpenMemHandle(rank %d): %s", r, hipGetErrorString(e));
    }
    c->peer_blk[r] = (char*)ptr;
  }
  c->p2p_attached = true;
  c->xtimeout_ticks = (unsigned long long)(timeout_ms > 0 ? timeout_ms : 5000) * 100000ull;   // 100 MHz wall clock
  c->xstep = 0;
  HIPCHK(hipMemset(c->xstatus, 0, 2 * sizeof(unsigned long long)));
  c->xch_mode = IQLHIP_XCH_P2P;
  drop_graph(c);
  return IQLHIP_OK;
}

extern "C" int iqlhip_xch_select(iqlhip_ctx* c, int mode) {
  if (!c) return fail(IQLHIP_EINVAL, "NULL ctx");
  if (mode == IQLHIP_XCH_RCCL && !c->nccl_comm) return fail(IQLHIP_EINVAL, "no RCCL communicator (iqlhip_allreduce_init)");
  if (mode == IQLHIP_XCH_P2P && !c->p2p_attached) return fail(IQLHIP_EINVAL, "no P2P exchange (iqlhip_p2p_attach)");
  if (mode != IQLHIP_XCH_NONE && mode != IQLHIP_XCH_RCCL && mode != IQLHIP_XCH_P2P) return fail(IQLHIP_EINVAL, "unknown exchange mode %d", mode);
  c->xch_mode = mode;
  return IQLHIP_OK;
}

extern "C" int iqlhip_xch_status(iqlhip_ctx* c, int64_t status[3], void* stream) {
  if (!c || !status) return fail(IQLHIP_EINVAL, "NULL argument");
  DevGuard guard(c->device);
  unsigned long long h[2] = {0, 0};
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  HIPCHK(hipMemcpy(h, c->xstatus, sizeof h, hipMemcpyDeviceToHost));
  status[0] = c->xch_mode;
  status[1] = (int64_t)h[0];
  status[2] = (int64_t)c->xstep;
  return IQLHIP_OK;
}

// Forget a recorded wait timeout (after the caller has re-synchronised the replicas and chosen another exchange).
extern "C" int iqlhip_xch_clear_status(iqlhip_ctx* c, void* stream) {
  if (!c) return fail(IQLHIP_EINVAL, "NULL ctx");
  DevGuard guard(c->device);
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  HIPCHK(hipMemset(c->xstatus, 0, 2 * sizeof(unsigned long long)));
  HIPCHK(hipDeviceSynchronize());
  drop_graph(c);
  return IQLHIP_OK;
}

extern "C" int iqlhip_xch_shutdown(iqlhip_ctx* c) {
  if (!c) return IQLHIP_OK;
  DevGuard guard(c->device);
  (void)hipDeviceSynchronize();
  drop_graph(c);
  if (c->nccl_comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->nccl_comm);
  c->nccl_comm = nullptr;
  p2p_close(c);
  if (c->xblk) (void)hipFree(c->xblk);
  c->xblk = nullptr;
  c->xch_mode = IQLHIP_XCH_NONE;
  c->world = 1;
  c->rank = 0;
  return IQLHIP_OK;
}

// A P2P wait that timed out is sticky and silent on the device (later waits return at once and the update kernels sum
// whatever the peers' buffers hold): the entry points that synchronise anyway read the status word along with the
// losses and turn it into an error, so a run cannot keep training on unsynchronised gradients unnoticed.
static int xch_poisoned(iqlhip_ctx* c, const unsigned long long* status_host) {
  if (status_host[0] == 0ull) return IQLHIP_OK;
  return fail(IQLHIP_EEXCHANGE, "the peer-to-peer gradient exchange timed out at exchange step %llu: a peer rank did not arrive; "
              "the replicas are no longer synchronised", status_host[0]);
}

// Synchronise `st`; with a P2P exchange the status words come back in front of that and a recorded timeout is the result.
static bool xch_p2p(const iqlhip_ctx* c) { return c->xch_mode == IQLHIP_XCH_P2P && c->world > 1; }
static int xch_status_after_sync(iqlhip_ctx* c, hipStream_t st) {
  const bool p2p = xch_p2p(c);
  if (p2p) HIPCHK(hipMemcpyAsync(c->xstatus_host, c->xstatus, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return p2p ? xch_poisoned(c, c->xstatus_host) : IQLHIP_OK;
}

static XchParams make_xch(const iqlhip_ctx* c, bool from_hdr) {
  XchParams x;
  memset(&x, 0, sizeof x);
  for (int r = 0; r < IQLHIP_MAX_WORLD; ++r)
    x.peer_flags[r] = (unsigned long long*)c->peer_blk[std::min(r, c->world - 1)];
  x.status = c->xstatus;
  x.hdr = from_hdr ? c->hdr : nullptr;
  x.xstep = c->xstep;
  x.timeout_ticks = c->xtimeout_ticks;
  x.rank = c->rank;
  x.world = c->world;
  return x;
}

// One step's launches after the batch has been staged: forward, backward and — by exchange mode — the update, or
// flatten + all-reduce + update, or flatten + flag handshake + the update that reads every rank's buffer.
// `k` = position inside the chunk (selects the P2P buffer together with `parity`, and the flag value hdr[XSTEP]+k+1).
// `sa` (statistics enabled): the two statistics launches between the backward and the update — after the last reader
// of `heads`, before the update kernel, which is the last reader of the slabs and, in a chunk, moves the header word
// the ring slot is formed from.  `kind`: the chunk's (every kind but Plain has a forward of its own).
static int enqueue_step(iqlhip_ctx* c, const StepParams& p_in, UpdParams u, int mode, int parity, int k, bool from_hdr,
                        hipStream_t st, hipEvent_t* ev, const StatsArgs* sa = nullptr, ChunkKind kind = ChunkKind::Plain,
                        const RowWeights* rw = nullptr) {
  StepParams p = p_in;
  const int buf = (parity + k) & 1;
  // P2P with batches of <= 256 rows: no flatten kernel.  The backward writes its chunk slab (= the w1 / b1 / w2 / b2 /
  // log_std gradients themselves), its <= 8 row-tile slabs of w0 / b0 partials and its loss sums straight into this
  // rank's exchange block; they are complete and written back at the kernel boundary in front of the flag kernel, and
  // every rank's update kernel reads all ranks' blocks.
  const bool direct = (mode == IQLHIP_XCH_P2P) && (p.rows <= CHUNK_ROWS);
  if (direct) {
    p.sc.slab_a = (float*)(c->xblk + c->xflat_off[buf]);
    p.sc.slab_b = (float*)(c->xblk + c->xslabb_off[buf]);
    for (int n = 0; n < 4; ++n) p.sc.slab_b_off[n] = c->xslab_b_off[n];
    p.sc.loss_parts = (float*)(c->xblk + c->xloss_off[buf]);
  }
  launch_fwd(c, p, st, kind);
  if (ev) HIPCHK(hipEventRecord(ev[1], st));
  launch_bwd(c, p, st, rw);
  if (ev) HIPCHK(hipEventRecord(ev[2], st));
  // (clipping is refused with an exchange before any launch: below, mode is IQLHIP_XCH_NONE whenever clip_on)
  launch_stats(c, u, sa, c->clip_on, st);
  if (mode == IQLHIP_XCH_RCCL) {
    launch_flatten(c, u, c->xflat, false, st);
    NCCLCHK(g_rccl.AllReduce(c->xflat, c->xflat, (size_t)c->L.n_params + 4, RCCL_FLOAT32, RCCL_SUM, c->nccl_comm, st));
    u.flat_grads = c->xflat;
  } else if (mode == IQLHIP_XCH_P2P) {
    if (!direct) launch_flatten(c, u, (float*)(c->xblk + c->xflat_off[buf]), true, st);
    if (c->world > 1) hipLaunchKernelGGL(iql_xch_signal_wait_kernel, dim3(1), dim3(64), 0, st, make_xch(c, from_hdr), k);
    for (int r = 0; r < IQLHIP_MAX_WORLD; ++r) {
      const char* blk = c->peer_blk[std::min(r, c->world - 1)];
      u.peer_flat[r] = (const float*)(blk + c->xflat_off[buf]);
      u.peer_slab_b[r] = (const float*)(blk + c->xslabb_off[buf]);
      u.peer_loss[r] = (const float*)(blk + c->xloss_off[buf]);
    }
    u.n_peer = c->world;
    u.peer_direct = direct ? 1 : 0;
    if (direct) for (int n = 0; n < 4; ++n) u.slab_b_off[n] = c->xslab_b_off[n];
  }
  launch_upd(c, u, st, c->clip_on ? c->clip_dev + 4 : nullptr);
  if (ev) HIPCHK(hipEventRecord(ev[3], st));
  return IQLHIP_OK;
}

static int ensure_events(iqlhip_ctx* c, int n) {
  while ((int)c->ev.size() < n) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    c->ev.push_back(e);
  }
  return IQLHIP_OK;
}

static int harvest_timing(iqlhip_ctx* c) {
  for (int i = 0; i + 3 < c->ev_used; i += 4) {
    HIPCHK(hipEventSynchronize(c->ev[i + 3]));
    float a = 0, b = 0, d = 0;
    HIPCHK(hipEventElapsedTime(&a, c->ev[i], c->ev[i + 1]));
    HIPCHK(hipEventElapsedTime(&b, c->ev[i + 1], c->ev[i + 2]));
    HIPCHK(hipEventElapsedTime(&d, c->ev[i + 2], c->ev[i + 3]));
    c->t_acc[0] += a * 1e3f; c->t_acc[1] += b * 1e3f; c->t_acc[2] += d * 1e3f; c->t_acc[3] += (a + b + d) * 1e3f;
    c->t_n += 1;
  }
  c->ev_used = 0;
  return IQLHIP_OK;
}

extern "C" int iqlhip_set_timing(iqlhip_ctx* c, int enabled) {
  if (!c) return fail(IQLHIP_EINVAL, "NULL ctx");
  c->timing = enabled != 0;
  c->ev_used = 0;
  c->t_n = 0;
  for (float& t : c->t_acc) t = 0.f;
  return IQLHIP_OK;
}

extern "C" int iqlhip_get_timing(iqlhip_ctx* c, float out_us[4]) {
  if (!c || !out_us) return fail(IQLHIP_EINVAL, "NULL argument");
  int rc = harvest_timing(c);
  if (rc) return rc;
  for (int k = 0; k < 4; ++k) out_us[k] = c->t_n ? c->t_acc[k] / c->t_n : 0.f;
  return IQLHIP_OK;
}

// Wait for the completion word of a synchronous entry point: spin on host-mapped memory (no HIP call: a stream
// synchronise was measured at 12-17 us of host time AFTER the GPU had finished, profiles/r03_sync_cost.txt); bounded —
// after 2 s the stream is synchronised the ordinary way, so a lost store cannot hang the caller.
static int wait_word(const unsigned long long* f, unsigned long long val, hipStream_t st) {
  // (acquire loads: the callers read the pinned loss words right behind this — those loads must not move in front of
  //  the flag's)
  if (__atomic_load_n(f, __ATOMIC_ACQUIRE) == val) return IQLHIP_OK;
  const double t0 = now_us();
  for (;;) {
    for (int i = 0; i < 256; ++i) if (__atomic_load_n(f, __ATOMIC_ACQUIRE) == val) return IQLHIP_OK;
    if (now_us() - t0 > 2e6) break;
  }
  HIPCHK(hipStreamSynchronize(st));
  if (__atomic_load_n(f, __ATOMIC_ACQUIRE) != val) return fail(IQLHIP_EHIP, "the step's completion word was not written");
  return IQLHIP_OK;
}
// The synchronous tail of an eager step whose update mirrors its losses into on_loss_pin: with a P2P exchange the
// ordinary synchronise (the exchange's status word has to come back too), else the completion word; then the losses.
static int sync_losses(iqlhip_ctx* c, unsigned long long done_val, hipStream_t st, float out[3]) {
  const int rc = xch_p2p(c) ? xch_status_after_sync(c, st) : wait_word(c->done_pin, done_val, st);
  if (rc) return rc;
  out[0] = c->on_loss_pin[0]; out[1] = c->on_loss_pin[1]; out[2] = c->on_loss_pin[2];
  return IQLHIP_OK;
}

// The head of an eager step, once its caller has made its checks and staged or gathered the batch at `xb`: the staging
// a following train_steps call might continue from is no longer that call's, the bf16 shadows are refreshed, the
// step's keep-bits drawn (draw = false: iqlhip_debug_time_kernel, which moves no stream position), and the step's
// records built.
struct EagerStep {
  StepParams p; UpdParams u; StatsArgs sa; bool with_stats;
  const StatsArgs* stats() const { return with_stats ? &sa : nullptr; }
};
static void eager_begin(iqlhip_ctx* c, int rows, const iqlhip_step_scalars* sc, hipStream_t st, const float* xb, EagerStep& e,
                        bool draw = true) {
  c->cont.valid = false;
  refresh_shadows(c, st);
  if (draw && c->drop_p > 0.f && !c->drop_inject) launch_dropmask(c, c->drop_seed, c->drop_step++, nullptr, 0, st);
  e.p = make_step(c, rows, sc->inv_batch);
  e.p.xb = xb;
  e.u = make_upd(c, sc, rows, nullptr);
  e.with_stats = c->stats_on;
  if (e.with_stats) e.sa = make_stats(c, e.p, nullptr, 0, 0, nullptr);
}

static int step_impl(iqlhip_ctx* c, const iqlhip_batch* b, const iqlhip_step_scalars* sc, float* out_sync, void* stream,
                     bool defer_wait = false, const RowWeights* rw = nullptr);

extern "C" int iqlhip_step(iqlhip_ctx* c, const iqlhip_batch* b, const iqlhip_step_scalars* sc, void* stream) {
  return step_impl(c, b, sc, nullptr, stream);
}

// ImplicitQLearning.train(batch) WITH its host synchronisation (the three .item() calls of iql.py:491,509,535 as one):
// iqlhip_step + the losses, which land in host-mapped pinned words followed by a completion word the host spins on.
// Returns once the losses are there; everything else the step does stays ordered by the stream as usual.
extern "C" int iqlhip_step_sync(iqlhip_ctx* c, const iqlhip_batch* b, const iqlhip_step_scalars* sc, float out[3], void* stream) {
  if (!out) return fail(IQLHIP_EINVAL, "NULL argument");
  return step_impl(c, b, sc, out, stream);
}

// The two halves of iqlhip_step_sync for a host that has something to do while the GPU runs the step (the Python shim
// computes the NEXT step's float64 Adam / cosine scalars there): begin launches, wait returns the losses.
extern "C" int iqlhip_step_begin(iqlhip_ctx* c, const iqlhip_batch* b, const iqlhip_step_scalars* sc, void* stream) {
  float dummy[3];
  return step_impl(c, b, sc, dummy, stream, /*defer_wait=*/true);
}
extern "C" int iqlhip_step_wait(iqlhip_ctx* c, float out[3], void* stream) {
  if (!c || !out) return fail(IQLHIP_EINVAL, "NULL argument");
  return sync_losses(c, c->done_seq, (hipStream_t)stream, out);
}

// The cases the row-weighted backward is not built for; checked before anything is launched or any counter moves.
static int row_weights_check(const iqlhip_ctx* c, int rows, const RowWeights& rw) {
  if (!rw.w) return fail(IQLHIP_EINVAL, "NULL row weights");
  if ((((uintptr_t)rw.w) & 3) || (((uintptr_t)rw.td) & 7)) return fail(IQLHIP_EINVAL, "row weights must be 4-byte, TD errors 8-byte aligned");
  if (c->precision == 1) return fail(IQLHIP_EUNSUPPORTED, "per-row loss weights are not supported at bf16 precision");
  if (use_lb(c, rows)) return fail(IQLHIP_EUNSUPPORTED, "per-row loss weights are not supported on the large-batch path");
  if (c->xch_mode != IQLHIP_XCH_NONE) return fail(IQLHIP_EUNSUPPORTED, "per-row loss weights are not supported with a data-parallel exchange");
  return IQLHIP_OK;
}

// iqlhip_step with every row's loss terms multiplied by row_w_dev[row] (fp32, `rows` values on the device): the
// row-weighted backward, everything else the plain step's launches.  td_out_dev (nullable, [rows][2] fp32) receives the
// rows' pre-update TD errors (q1 - y, q2 - y).  NaN or negative weights are the caller's business.
extern "C" int iqlhip_step_rw(iqlhip_ctx* c, const iqlhip_batch* b, const iqlhip_step_scalars* sc, const float* row_w_dev,
                              float* td_out_dev, void* stream) {
  const RowWeights rw = {row_w_dev, td_out_dev};
  return step_impl(c, b, sc, nullptr, stream, false, &rw);
}

static int step_impl(iqlhip_ctx* c, const iqlhip_batch* b, const iqlhip_step_scalars* sc, float* out_sync, void* stream,
                     bool defer_wait, const RowWeights* rw) {
  if (!c || !sc) return fail(IQLHIP_EINVAL, "NULL argument");
  int rc = check_batch(c, b);
  if (rc) return rc;
  if (rw && (rc = row_weights_check(c, b->rows, *rw))) return rc;
  if ((rc = step_entry(c, b->rows, stream, /*multi_step=*/false))) return rc;
  DevGuard guard(c->device);
  hipStream_t st = (hipStream_t)stream;
  const float* xb_cur = nullptr;
  rc = stage_batch(c, b, st, &xb_cur);
  if (rc) return rc;
  EagerStep e;
  eager_begin(c, b->rows, sc, st, xb_cur, e);
  unsigned long long done_val = 0;
  if (out_sync) {
    e.u.losses_mirror = c->on_loss_pin;
    e.u.done_flag = c->done_pin;
    e.u.done_val = done_val = ++c->done_seq;
  }
  hipEvent_t* ev = nullptr;
  if (c->timing) {
    if (c->ev_used + 4 > 4096) { rc = harvest_timing(c); if (rc) return rc; }
    rc = ensure_events(c, c->ev_used + 4);
    if (rc) return rc;
    ev = &c->ev[c->ev_used];
    c->ev_used += 4;
    HIPCHK(hipEventRecord(ev[0], st));
  }
  rc = enqueue_step(c, e.p, e.u, c->xch_mode, (int)(c->xstep & 1ull), 0, /*from_hdr=*/false, st, ev, e.stats(), ChunkKind::Plain, rw);
  if (rc) return rc;
  if (c->xch_mode != IQLHIP_XCH_NONE) c->xstep += 1;
  HIPCHK(hipGetLastError());
  return (out_sync && !defer_wait) ? sync_losses(c, done_val, st, out_sync) : IQLHIP_OK;
}

static int actor_forward_impl(iqlhip_ctx* c, const float* states_dev, int64_t ld_s, int32_t rows, const float* noise_dev,
                              int64_t ld_noise, uint64_t rng_seed, uint64_t rng_call, float max_action,
                              float* actions_dev, int64_t ld_a, void* stream, unsigned long long* done_flag = nullptr,
                              unsigned long long done_val = 0);

// One iteration of the online loop's device work (algorithms/finetune/iql.py:741-773: add_transition -> sample ->
// train) in ONE call and four launches: ring write + gather straight from pinned host words, forward, backward, update
// with the losses landing in pinned host words; then one stream synchronisation.
// iqlhip_online_step (rows_off_dev == nullptr, n_off == 0) and iqlhip_online_step_mixed: the batch's first n_off rows
// are rows_off_dev[idx_off_host[..]] (size_off rows, read only), the n behind them come from the ring.
// The part every form of the online iteration shares (iqlhip_online_step, iqlhip_online_step_mixed,
// iqlhip_jsrl_online_step): the checks, the ring write + gather and the step, queued on `stream`.  act_follows: the
// call's completion word is left to the launch that follows the step (an act's finish); else the update stores it.
// pr != nullptr — iqlhip_online_step_prioritized (its own checks made, its buffers there): no host indices; the ring write
// carries the insert at the table's maximum, the rows are drawn by the table on the device, the step is the row-weighted
// one and the table update by its TD errors follows it (online_prio_gather / online_prio_update, defined with the
// tracking tables at the end of the file).
struct OnlinePrio { iqlhip_weights* table; uint64_t seed, offset; float is_beta, alpha, eps; };
static void online_prio_gather(iqlhip_ctx* c, float* rows_dev, int64_t ld, int64_t pointer, int32_t n, const OnlinePrio& pr,
                               hipStream_t st, RowWeights* rw);
static void online_prio_update(iqlhip_ctx* c, int32_t n, const OnlinePrio& pr, hipStream_t st);
// ns != nullptr — iqlhip_online_step_nstep (its own checks made): rows_dev is the DERIVED ring; one launch in front of the
// gather stores the host row into the raw ring, sets its end byte and refreshes the derived rows the new transition
// extends (online_nstep_refresh, defined with the n-step rows at the end of the file).  The gather's own ring write then
// stores at derived[pointer] the bytes that launch stored there (the newest derived row is the host row: k = 1).
struct OnlineNstep { float* raw_dev; unsigned char* ends_dev; unsigned char* steps_dev; int64_t size_after; int32_t horizon;
                     int32_t episode_end; double discount; };
static void online_nstep_refresh(iqlhip_ctx* c, float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer,
                                 const OnlineNstep& ns, hipStream_t st);
static int online_step_front(iqlhip_ctx* c, float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer,
                             const float* row_host, const int64_t* idx_host, int32_t n, const iqlhip_step_scalars* sc,
                             const float* out, bool act_follows, void* stream, const float* rows_off_dev,
                             int64_t size_off, const int64_t* idx_off_host, int32_t n_off,
                             unsigned long long* done_val_out, const OnlinePrio* pr = nullptr,
                             const OnlineNstep* ns = nullptr) {
  if (!c || !rows_dev || !row_host || (!idx_host && !pr) || !sc || !out) return fail(IQLHIP_EINVAL, "NULL argument");
  if (!c->params) return fail(IQLHIP_ENOTBOUND, "iqlhip_bind has not been called");
  if (ld != c->row_ld) return fail(IQLHIP_EINVAL, "row stride must be iqlhip_row_stride(S,A)=%lld", (long long)c->row_ld);
  if (((uintptr_t)rows_dev) & 15) return fail(IQLHIP_EINVAL, "packed rows must be 16-byte aligned");
  const int B = n_off + n;                // rows of the step
  if (n < 1 || n_off < 0 || n > c->dims.max_batch || n_off > c->dims.max_batch || B > c->dims.max_batch)
    return fail(IQLHIP_EINVAL, "batch rows %d (+ %d offline) outside [1, max_batch=%d]", n, n_off, c->dims.max_batch);
  if (capacity < 1 || pointer < 0 || pointer >= capacity) return fail(IQLHIP_EINVAL, "ring pointer outside the buffer");
  {                                       // (the reference's torch indexing raises on such an index; a gather would fault)
    int rc_i = pr ? IQLHIP_OK : check_host_indices(idx_host, n, capacity);      // (pr: the device draws; the descent is clamped)
    if (!rc_i && n_off) rc_i = check_host_indices(idx_off_host, n_off, size_off);
    if (rc_i) return rc_i;
    if ((rc_i = step_entry(c, B, stream, /*multi_step=*/false))) return rc_i;
  }
  DevGuard guard(c->device);
  hipStream_t st = (hipStream_t)stream;
  memcpy(c->on_row_pin, row_host, (size_t)ld * sizeof(float));
  if (n_off) memcpy(c->on_idx_pin, idx_off_host, (size_t)n_off * sizeof(long long));      // [offline | online], batch order
  if (!pr) memcpy(c->on_idx_pin + n_off, idx_host, (size_t)n * sizeof(long long));
  const int total = B * (int)(ld / 4);
  RowWeights rw = {nullptr, nullptr};
  if (ns) online_nstep_refresh(c, rows_dev, ld, capacity, pointer, *ns, st);
  if (pr)
    online_prio_gather(c, rows_dev, ld, pointer, n, *pr, st, &rw);
  else if (n_off)
    hipLaunchKernelGGL(iql_online_gather2_kernel, dim3((total + 255) / 256), dim3(256), 0, st, rows_dev, rows_off_dev,
                       (long long)ld, (long long)pointer, (const float*)c->on_row_pin, (const long long*)c->on_idx_pin,
                       c->xb, n_off, B);
  else
    hipLaunchKernelGGL(iql_online_gather_kernel, dim3((total + 255) / 256), dim3(256), 0, st, rows_dev, (long long)ld,
                       (long long)pointer, (const float*)c->on_row_pin, (const long long*)c->on_idx_pin, c->xb, n);
  EagerStep e;
  eager_begin(c, B, sc, st, c->xb, e);
  e.u.losses_mirror = c->on_loss_pin;
  const unsigned long long done_val = ++c->done_seq;
  if (!act_follows) { e.u.done_flag = c->done_pin; e.u.done_val = done_val; }      // (else the follow-up act() signals)
  int rc = enqueue_step(c, e.p, e.u, c->xch_mode, (int)(c->xstep & 1ull), 0, /*from_hdr=*/false, st, nullptr, e.stats(),
                        ChunkKind::Plain, pr ? &rw : nullptr);
  if (rc) return rc;
  if (c->xch_mode != IQLHIP_XCH_NONE) c->xstep += 1;
  if (pr) online_prio_update(c, n, *pr, st);      // table[drawn rows] <- the priorities of the step's TD errors
  *done_val_out = done_val;
  return IQLHIP_OK;
}
static int online_step(iqlhip_ctx* c, float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer,
                       const float* row_host, const int64_t* idx_host, int32_t n, const iqlhip_step_scalars* sc,
                       float out[3], const float* act_state_host, float max_action, uint64_t act_seed,
                       float* act_out_host, void* stream, const float* rows_off_dev, int64_t size_off,
                       const int64_t* idx_off_host, int32_t n_off, const OnlinePrio* pr = nullptr,
                       const OnlineNstep* ns = nullptr) {
  if (!c || !rows_dev || !row_host || (!idx_host && !pr) || !sc || !out) return fail(IQLHIP_EINVAL, "NULL argument");
  if (act_state_host && !act_out_host) return fail(IQLHIP_EINVAL, "act_state_host without act_out_host");
  unsigned long long done_val = 0;
  int rc = online_step_front(c, rows_dev, ld, capacity, pointer, row_host, idx_host, n, sc, out, act_state_host != nullptr,
                             stream, rows_off_dev, size_off, idx_off_host, n_off, &done_val, pr, ns);
  if (rc) return rc;
  DevGuard guard(c->device);
  hipStream_t st = (hipStream_t)stream;
  const int S = c->dims.state_dim, A = c->dims.action_dim;
  if (act_state_host) {
    // the NEXT iteration's actor.act(next_state) with the just-updated policy, in the same stream and under the
    // same synchronisation: state and action travel through host-mapped pinned words
    memcpy(c->on_act_pin, act_state_host, (size_t)S * sizeof(float));
    float* a_out = c->on_act_pin + IQLHIP_MAX_INPUT;
    rc = (act_seed != 0 && c->dims.policy == IQLHIP_POLICY_GAUSSIAN)
             ? actor_forward_impl(c, c->on_act_pin, S, 1, nullptr, 0, act_seed, c->act_calls++, max_action, a_out, A, stream, c->done_pin, done_val)
             : actor_forward_impl(c, c->on_act_pin, S, 1, nullptr, 0, 0, 0, max_action, a_out, A, stream, c->done_pin, done_val);
    if (rc) return rc;
  }
  // (a synchronous call: the pinned staging words are free again on return.)  Without an exchange the completion word
  // comes from the last kernel of the call; the whole call's kernels precede it in the stream EXCEPT that the update's
  // flag is stored by its first block — the ring write and the gather (first launch) are long done by then, and the
  // pinned words read below were written before the flag (release)
  rc = sync_losses(c, done_val, st, out);
  if (rc) return rc;
  if (act_state_host) memcpy(act_out_host, c->on_act_pin + IQLHIP_MAX_INPUT, (size_t)A * sizeof(float));
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}
extern "C" int iqlhip_online_step(iqlhip_ctx* c, float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer,
                                  const float* row_host, const int64_t* idx_host, int32_t n,
                                  const iqlhip_step_scalars* sc, float out[3], const float* act_state_host,
                                  float max_action, uint64_t act_seed, float* act_out_host, void* stream) {
  return online_step(c, rows_dev, ld, capacity, pointer, row_host, idx_host, n, sc, out, act_state_host, max_action,
                     act_seed, act_out_host, stream, nullptr, 0, nullptr, 0);
}
extern "C" int iqlhip_online_step_mixed(iqlhip_ctx* c, float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer,
                                        const float* row_host, const int64_t* idx_host, int32_t n,
                                        const iqlhip_step_scalars* sc, float out[3], const float* act_state_host,
                                        float max_action, uint64_t act_seed, float* act_out_host, void* stream,
                                        const float* rows_off_dev, int64_t size_off, const int64_t* idx_off_host,
                                        int32_t n_off) {
  if (!rows_off_dev || !idx_off_host) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n_off < 1) return fail(IQLHIP_EINVAL, "n_off must be at least 1 (no offline rows: iqlhip_online_step)");
  if (size_off < 1) return fail(IQLHIP_EINVAL, "empty offline buffer");
  if (rows_off_dev == rows_dev) return fail(IQLHIP_EINVAL, "the offline and the online buffer are the same rows");
  if (((uintptr_t)rows_off_dev) & 15) return fail(IQLHIP_EINVAL, "packed rows must be 16-byte aligned");
  // (the same scope as iqlhip_train_steps_mixed: no exchange, no large-batch bf16 step — before anything is launched)
  if (c && c->xch_mode != IQLHIP_XCH_NONE)
    return fail(IQLHIP_EUNSUPPORTED, "mixed batches are not supported with a data-parallel exchange");
  if (c && n > 0 && n_off <= c->dims.max_batch && n <= c->dims.max_batch && use_lb(c, n_off + n))
    return fail(IQLHIP_EUNSUPPORTED, "mixed batches are not supported on the large-batch bf16 path (more than %d rows)", LB_MIN_ROWS);
  return online_step(c, rows_dev, ld, capacity, pointer, row_host, idx_host, n, sc, out, act_state_host, max_action,
                     act_seed, act_out_host, stream, rows_off_dev, size_off, idx_off_host, n_off);
}

static int forward_backward_impl(iqlhip_ctx* c, const iqlhip_batch* b, const iqlhip_step_scalars* sc, float* grads_dev,
                                 void* stream, const RowWeights* rw);
extern "C" int iqlhip_forward_backward(iqlhip_ctx* c, const iqlhip_batch* b, const iqlhip_step_scalars* sc,
                                       float* grads_dev, void* stream) {
  return forward_backward_impl(c, b, sc, grads_dev, stream, nullptr);
}
// iqlhip_forward_backward with iqlhip_step_rw's row weights: the gradient of the weighted losses.
extern "C" int iqlhip_forward_backward_rw(iqlhip_ctx* c, const iqlhip_batch* b, const iqlhip_step_scalars* sc,
                                          const float* row_w_dev, float* td_out_dev, float* grads_dev, void* stream) {
  const RowWeights rw = {row_w_dev, td_out_dev};
  return forward_backward_impl(c, b, sc, grads_dev, stream, &rw);
}
static int forward_backward_impl(iqlhip_ctx* c, const iqlhip_batch* b, const iqlhip_step_scalars* sc, float* grads_dev,
                                 void* stream, const RowWeights* rw) {
  if (!c || !sc || !grads_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  int rc = check_batch(c, b);
  if (rc) return rc;
  if (rw && (rc = row_weights_check(c, b->rows, *rw))) return rc;
  DevGuard guard(c->device);
  hipStream_t st = (hipStream_t)stream;
  const float* xb_cur = nullptr;
  rc = stage_batch(c, b, st, &xb_cur);
  if (rc) return rc;
  EagerStep e;
  eager_begin(c, b->rows, sc, st, xb_cur, e);
  launch_fwd(c, e.p, st);
  launch_bwd(c, e.p, st, rw);
  launch_flatten(c, e.u, grads_dev, false, st);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

extern "C" int iqlhip_apply_update(iqlhip_ctx* c, const float* grads_dev, const iqlhip_step_scalars* sc, void* stream) {
  if (!c || !sc || !grads_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (!c->params) return fail(IQLHIP_ENOTBOUND, "iqlhip_bind has not been called");
  DevGuard guard(c->device);
  UpdParams u = make_upd(c, sc, 1, grads_dev);
  launch_upd(c, u, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

extern "C" int iqlhip_read_losses(iqlhip_ctx* c, float out[3], void* stream) {
  if (!c || !out) return fail(IQLHIP_EINVAL, "NULL argument");
  float* h = c->losses_host;
  HIPCHK(hipMemcpyAsync(h, c->sc.losses, 4 * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
  const int rc = xch_status_after_sync(c, (hipStream_t)stream);
  if (rc == IQLHIP_OK || rc == IQLHIP_EEXCHANGE) { out[0] = h[0]; out[1] = h[1]; out[2] = h[2]; }      // (the stream was synchronised)
  return rc;
}

extern "C" int iqlhip_read_loss_ring(iqlhip_ctx* c, float* out, int32_t n_steps, void* stream) {
  if (!c || !out) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n_steps < 1 || n_steps > c->ring_cap) return fail(IQLHIP_EINVAL, "n_steps outside [1,%d]", c->ring_cap);
  const float* h = c->loss_ring;
  const int rc = xch_status_after_sync(c, (hipStream_t)stream);
  if (rc != IQLHIP_OK && rc != IQLHIP_EEXCHANGE) return rc;
  for (int k = 0; k < n_steps; ++k)
    for (int j = 0; j < 3; ++j) out[3 * k + j] = h[4 * (size_t)k + j];
  return rc;
}

// ---------------------------------------------------------------------------
extern "C" int iqlhip_draw_indices(int64_t* idx_dev, int64_t n, int64_t size, uint64_t seed, uint64_t offset, void* stream) {
  if (!idx_dev || n < 1 || size < 1) return fail(IQLHIP_EINVAL, "bad argument");
  const int nb = (int)std::min<int64_t>((n / 2 + 255) / 256 + 1, 1024);
  hipLaunchKernelGGL(iql_draw_indices_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, (long long*)idx_dev,
                     (long long)n, (long long)size, (unsigned long long)seed, (unsigned long long)offset,
                     (const unsigned long long*)nullptr);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

// ---------------------------------------------------------------------------
// The multi-step driver.  A call of n steps = ONE directly launched set-up kernel (header words, the call's scalar
// table, step 0's rows unless the previous call left them staged) + its first 2 / 4 steps launched directly + replays
// of the fixed chunk graphs.  Everything a
// replay needs to differ in lives in device words that the set-up kernel writes once and each chunk's last update
// kernel advances, so the chunks of a call follow each other with no host-side launch in between; the rows, scalars and
// keep-bits of step k + 1 are staged by the idle eighth of step k's forward grid (IdleWork).
// The parts of iqlhip_ctx::prio_buf: the staged indices of staging parity h, the running step's TD errors, the call's words.
static long long* prio_idx(const iqlhip_ctx* c, int h) { return (long long*)c->prio_buf + (size_t)h * c->dims.max_batch; }
static float* prio_td(const iqlhip_ctx* c) { return (float*)(c->prio_buf + 16 * (size_t)c->dims.max_batch); }
static float* prio_words(const iqlhip_ctx* c) { return prio_td(c) + 2 * (size_t)c->dims.max_batch; }
// What a chunk kind implies for the driver.  A sixth kind is added HERE (and gets a forward in fwd_kernel_of, a named
// constructor and its pair of entry points); the driver below reads these fields and tests no kind itself.
//   setup, n_args   the call's set-up kernel and how many arguments it takes (fill_setup_args checks its count against it)
//   arg_groups      argument groups behind the fifteen common ones: {rows_on, n_off} (Mixed) or {wt}; {q_dst, beta_dev,
//                   beta}; {idx_dst, prio_words, alpha, eps, live}
//   rw_bwd          the row-weighted backward, its weights the c an idle block of the forward formed from the staged q
//   td_store        ... which stores the rows' TD errors;  table_update: the table update behind every step
//   wave_per_row    the set-up kernel draws step 0's rows by weight, a wave per row: its grid has a floor
//   continues       a call may start on the rows the previous one staged and stages for the next — one of the same
//   cont_class      only (what is staged besides the rows: nothing, q, q and indices)
//   moves_version   a finished call has moved its table's content version by 1
struct KindInfo { const void* setup; int n_args, arg_groups; bool rw_bwd, td_store, table_update, wave_per_row, continues;
                  int cont_class; bool moves_version; };
template <class... A> static KindInfo kind_row(void (*setup)(A...), int groups, bool rw, bool td, bool update, bool wave,
                                               bool cont, int cont_class, bool version) {
  return {(const void*)setup, (int)sizeof...(A), groups, rw, td, update, wave, cont, cont_class, version};
}
static const KindInfo& kind_info(ChunkKind kind) {
  static const KindInfo info[N_CHUNK_KINDS] = {
      //                                         groups rw_bwd td  update   wave   cont  class version
      kind_row(iql_call_setup_kernel,             0, false, false, false, false, true,  0, false),      // Plain
      kind_row(iql_call_setup_mixed_kernel,       1, false, false, false, false, false, 0, false),      // Mixed
      kind_row(iql_call_setup_weighted_kernel,    1, false, false, false, true,  true,  0, false),      // Weighted
      kind_row(iql_call_setup_weighted_is_kernel, 2, true,  false, false, true,  true,  1, false),      // WeightedIs
      kind_row(iql_call_setup_prio_kernel,        3, true,  true,  true,  true,  true,  2, true)};       // Prio
  return info[(int)kind];
}
// The table update behind step k of a prioritised chunk (end of file: its kernels are the library's last).
static void launch_prio_update(const iqlhip_ctx* c, const ChunkSrc& src, int B, int k, hipStream_t st);
static void fill_idle_work(const iqlhip_ctx* c, IdleWork* w, const float* rows_dev, int B, int K, const ChunkSrc& src) {
  const KindInfo& ki = kind_info(src.kind);
  const int MB = c->dims.max_batch;
  for (int k = 0; k < K; ++k) {
    IdleWork& i = w[k];
    memset(&i, 0, sizeof i);
    i.rows = rows_dev;
    i.ld = c->row_ld;
    i.xb_dst = (k & 1) ? c->xb : c->xb2;              // step k reads buffer k & 1, step k + 1 the other one
    i.hdr = c->hdr;
    i.sched_call = c->sched_call;
    i.sched_dst = c->sched_cur + k;
    i.drop_dst = (c->drop_p > 0.f) ? c->drop_bits + (size_t)((k + 1) & 1) * 2 * MB * 8 : nullptr;
    i.drop_words = 2 * MB * 8;
    i.drop_thresh = drop_thresh(c->drop_p);
    i.n = B;
    i.k = k;
    i.rows_on = src.rows_on; i.n_off = src.n_off; i.wt = src.wt;
    if (ki.rw_bwd) {          // step k's q lie in half k & 1 (where the step before staged them), step k + 1's go to the other
      i.q_src = c->is_buf + (size_t)(k & 1) * MB;
      i.q_dst = c->is_buf + (size_t)((k + 1) & 1) * MB;
      i.c_dst = c->is_buf + 2 * (size_t)MB;
      i.is_beta = c->is_buf + 3 * (size_t)MB;
    }
    if (ki.table_update) i.idx_dst = prio_idx(c, (k + 1) & 1);      // (as q_dst: step k + 1's half)
  }
}

static int enqueue_chunk(iqlhip_ctx* c, hipStream_t st, int B, int K, float inv_batch, int mode, int parity,
                         const IdleWork* work_dev, const ChunkSrc& src) {
  const KindInfo& ki = kind_info(src.kind);
  const int MB = c->dims.max_batch;
  iqlhip_step_scalars sc0;
  memset(&sc0, 0, sizeof sc0);
  sc0.inv_batch = inv_batch;
  for (int k = 0; k < K; ++k) {
    StepParams p = make_step(c, B, inv_batch);
    p.xb = (k & 1) ? c->xb2 : c->xb;
    if (p.drop_bits) p.drop_bits = c->drop_bits + (size_t)(k & 1) * 2 * MB * 8;
    p.g_work = work_dev + k;
    UpdParams u = make_upd(c, &sc0, B, nullptr);
    u.sched = c->sched_cur;
    u.sched_idx = k;
    u.loss_ring = c->loss_ring;
    u.ring_slot = k;
    u.ring_hdr = c->hdr;
    if (k + 1 == K) { u.adv_hdr = c->hdr; u.adv_k = K; u.adv_rows = B; }
    // (statistics: slot BASE + k of the ring, the loss ring's indexing; the chunk's key carries the setting)
    StatsArgs sa;
    if (c->stats_on) sa = make_stats(c, p, c->stats_ring, k, c->k_max, c->hdr);
    // (WeightedIs and Prio: the step's c, written by an idle block of its forward, is the row-weighted backward's weight
    //  vector; Prio: the backward stores the rows' TD errors, the new priorities of the rows staged in half k & 1 — the update's
    //  launches follow the step on the same stream, a linear chain in front of the next forward, which draws by the table)
    const RowWeights rw = {c->is_buf ? c->is_buf + 2 * (size_t)MB : nullptr, ki.td_store ? prio_td(c) : nullptr};
    int rc = enqueue_step(c, p, u, mode, parity, k, /*from_hdr=*/true, st, nullptr, c->stats_on ? &sa : nullptr, src.kind,
                          ki.rw_bwd ? &rw : nullptr);
    if (rc) return rc;
    if (ki.table_update) launch_prio_update(c, src, B, k, st);
  }
  return IQLHIP_OK;
}

// A pinned table slot that no queued set-up kernel still has to read.
static int acquire_sched_slot(iqlhip_ctx* c, int* slot_out) {
  const int slot = c->sched_slot;
  c->sched_slot = (c->sched_slot + 1) & 3;
  const volatile unsigned long long* ack = c->sched_ack + slot;
  if (*ack < c->sched_want[slot]) {
    // (four calls deep in flight: wait for that set-up kernel — it runs at the head of its call — then re-check)
    for (int spin = 0; spin < 20000 && *ack < c->sched_want[slot]; ++spin) { /* ~ a few tens of us */ }
    if (*ack < c->sched_want[slot] && c->sched_stream[slot]) HIPCHK(hipStreamSynchronize(c->sched_stream[slot]));
  }
  *slot_out = slot;
  return IQLHIP_OK;
}

// The set-up launch of a call (iql_call_setup_kernel): header, scalar table, and (gather) step 0's rows + keep-bits.
// Its arguments as values + the pointer array both launch forms take: a direct launch, or — head chunk graphs, whose
// first node is this kernel — hipGraphExecKernelNodeSetParams in front of the replay.
struct SetupArgs {
  unsigned long long* hdr; ChunkHdr h; iqlhip_step_scalars* sched_call; const iqlhip_step_scalars* sched_src; int n_steps;
  const float* rows; long long ld; float* xb; int B; unsigned* drop_dst; int drop_words; unsigned drop_thresh;
  unsigned* arrivals; unsigned long long* ack; unsigned long long ack_val;
  const float* rows_on; int n_off;        // the kinds' argument groups (KindInfo::arg_groups): Mixed's two ...
  WTab wt;                                // ... or, in their place, the table of the three weighted kinds
  float* q_dst; float* beta_dev; float beta;        // WeightedIs and Prio
  long long* idx_dst; float* prio_words; float alpha; float eps; unsigned live;      // Prio
  void* ptrs[24];
  const void* func;                       // KindInfo::setup of the call's kind
  int nb;
};
static int fill_setup_args(iqlhip_ctx* c, SetupArgs& a, const ChunkHdr& h, int slot, int n_steps, const float* rows_dev,
                           int B, bool gather, hipStream_t st, const ChunkCall& call) {
  const ChunkSrc& src = call.src;
  const KindInfo& ki = kind_info(src.kind);
  const int MB = c->dims.max_batch;
  const bool drop = gather && c->drop_p > 0.f;
  if (slot >= 0) {
    c->sched_want[slot] = ++c->call_seq;
    c->sched_stream[slot] = st;
  }
  a.hdr = c->hdr; a.h = h; a.sched_call = c->sched_call; a.sched_src = slot >= 0 ? c->sched_pin[slot] : c->sched_pin[0];
  a.n_steps = slot >= 0 ? n_steps : 0;
  a.rows = rows_dev; a.ld = (long long)c->row_ld; a.xb = c->xb; a.B = gather ? B : 0;
  a.drop_dst = drop ? c->drop_bits : nullptr; a.drop_words = 2 * MB * 8; a.drop_thresh = drop_thresh(c->drop_p);
  a.arrivals = c->setup_arrivals;
  a.ack = slot >= 0 ? c->sched_ack + slot : c->sched_ack + 4;        // (slot < 0: a capture-time placeholder, word 4 is a dummy)
  a.ack_val = slot >= 0 ? c->sched_want[slot] : 0ull;
  a.rows_on = src.rows_on; a.n_off = src.n_off; a.wt = src.wt;
  a.q_dst = c->is_buf; a.beta_dev = c->is_buf ? c->is_buf + 3 * (size_t)MB : nullptr; a.beta = call.is_beta;
  a.idx_dst = c->prio_buf ? prio_idx(c, 0) : nullptr; a.prio_words = c->prio_buf ? prio_words(c) : nullptr;
  a.alpha = call.alpha; a.eps = call.eps; a.live = call.live;
  a.func = ki.setup;
  // the pointer array: the fifteen common arguments, then the kind's groups in order
  int n = 0;
  auto append = [&](std::initializer_list<void*> group) { for (void* q : group) a.ptrs[n++] = q; };
  append({&a.hdr, &a.h, &a.sched_call, &a.sched_src, &a.n_steps, &a.rows, &a.ld, &a.xb, &a.B, &a.drop_dst, &a.drop_words,
          &a.drop_thresh, &a.arrivals, &a.ack, &a.ack_val});
  if (ki.arg_groups >= 1) src.kind == ChunkKind::Mixed ? append({&a.rows_on, &a.n_off}) : append({&a.wt});
  if (ki.arg_groups >= 2) append({&a.q_dst, &a.beta_dev, &a.beta});
  if (ki.arg_groups >= 3) append({&a.idx_dst, &a.prio_words, &a.alpha, &a.eps, &a.live});
  if (n != ki.n_args) return fail(IQLHIP_EINVAL, "set-up kernel of chunk kind %d: %d arguments appended, it takes %d", (int)src.kind, n, ki.n_args);
  long long want = ((long long)n_steps * 3 + 255) / 256;
  if (gather) want = std::max(want, ((long long)B * (c->row_ld / 4) + 255) / 256);
  if (gather && ki.wave_per_row) want = std::max(want, ((long long)B + 7) / 8);      // (a wave per row, two rows a pass)
  if (drop) want += (2 * MB * 8 + 255) / 256;
  a.nb = (int)std::max<long long>(1, std::min<long long>(want, 256));
  return IQLHIP_OK;
}
static int launch_call_setup(iqlhip_ctx* c, hipStream_t st, const ChunkHdr& h, int slot, int n_steps,
                             const float* rows_dev, int B, bool gather, const ChunkCall& call) {
  SetupArgs a;
  if (int rc = fill_setup_args(c, a, h, slot, n_steps, rows_dev, B, gather, st, call)) return rc;
  HIPCHK(hipLaunchKernel(a.func, dim3(a.nb), dim3(256), a.ptrs, 0, st));
  return IQLHIP_OK;
}

// The header a call's set-up kernel writes: what the index draw covers and where it stands, and the context's keep-bit
// and exchange positions (c == nullptr: none of them — the placeholder a head chunk graph is captured with).
static ChunkHdr call_hdr(const iqlhip_ctx* c, int64_t size, int64_t size_on, uint64_t seed, uint64_t offset) {
  ChunkHdr h;
  memset(&h, 0, sizeof h);
  h.w[HDR_SIZE] = (unsigned long long)size;
  h.w[HDR_SIZE_ON] = (unsigned long long)size_on;
  h.w[HDR_SEED] = (unsigned long long)seed;
  h.w[HDR_OFFSET] = (unsigned long long)offset;      // index j of the call = counter offset + j / 2, pair word j & 1
  if (c) { h.w[HDR_DROP_STEP] = c->drop_step; h.w[HDR_DROP_SEED] = c->drop_seed; h.w[HDR_XSTEP] = c->xstep; }
  return h;
}
// The n steps of chunk graph `cg` have been queued on `st`: the host's positions follow.  (The keep-bit position moves
// with the steps that draw: a rate of 0 leaves it alone, as iqlhip_step does — a caller that switches the actor to
// eval() for some steps finds the stream where eager steps would have left it.)
static void chunk_queued(iqlhip_ctx* c, iqlhip_ctx::CachedGraph* cg, hipStream_t st, int n) {
  cg->last = st;
  if (c->drop_p > 0.f) c->drop_step += (unsigned long long)n;
  if (c->xch_mode != IQLHIP_XCH_NONE) c->xstep += (unsigned long long)n;
}

// Capture and instantiate the chunk graph of g.key into g, member by member (a failure leaves the ones made so far).
static int build_chunk_graph(iqlhip_ctx* c, iqlhip_ctx::CachedGraph& g) {
  const GraphKey& key = g.key;
  // the chunk's idle-work records: device memory written once, here (their content is part of what the key freezes)
  {
    std::vector<IdleWork> hw((size_t)key.K);
    fill_idle_work(c, hw.data(), key.rows, key.B, key.K, key.src);
    HIPCHK(hipMalloc((void**)&g.work, hw.size() * sizeof(IdleWork)));
    hipError_t e = hipMemcpy(g.work, hw.data(), hw.size() * sizeof(IdleWork), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(IQLHIP_EHIP, "chunk_graph: hipMemcpy: %s", hipGetErrorString(e));
  }
  hipStream_t cs = c->cap_stream;
  // (relaxed: a collective library may make calls during capture that the stricter modes forbid)
  hipError_t e = hipStreamBeginCapture(cs, key.xch == IQLHIP_XCH_RCCL ? hipStreamCaptureModeRelaxed : hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) return fail(IQLHIP_EHIP, "hipStreamBeginCapture: %s", hipGetErrorString(e));
  int rc = IQLHIP_OK;
  if (key.head) {        // placeholder arguments: every replay sets the real ones (grid included)
    ChunkCall placeholder;
    placeholder.src = key.src;
    SetupArgs a;
    rc = fill_setup_args(c, a, call_hdr(nullptr, 1, 1, 0, 0), -1, 0, key.rows, key.B, true, cs, placeholder);
    if (!rc && hipLaunchKernel(a.func, dim3(a.nb), dim3(256), a.ptrs, 0, cs) != hipSuccess)
      rc = fail(IQLHIP_EHIP, "capture of the set-up kernel failed");
  }
  if (!rc) rc = enqueue_chunk(c, cs, key.B, key.K, key.inv_batch, key.xch, key.parity, g.work, key.src);
  e = hipStreamEndCapture(cs, &g.graph);
  if (rc) return rc;
  if (e != hipSuccess) return fail(IQLHIP_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
  e = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
  if (e != hipSuccess) return fail(IQLHIP_EHIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
  if (key.head) {
    size_t n_root = 1;
    e = hipGraphGetRootNodes(g.graph, &g.setup_node, &n_root);
    hipGraphNodeType ty = hipGraphNodeTypeEmpty;
    if (e == hipSuccess && n_root == 1) e = hipGraphNodeGetType(g.setup_node, &ty);
    if (e != hipSuccess || n_root != 1 || ty != hipGraphNodeTypeKernel)
      return fail(IQLHIP_EHIP, "head chunk graph: no single kernel root node");
  }
  return IQLHIP_OK;
}

static int chunk_graph(iqlhip_ctx* c, const GraphKey& key, hipGraphExec_t* out, iqlhip_ctx::CachedGraph** slot) {
  for (auto& g : c->graphs)
    if (g.key == key) { g.stamp = ++c->graph_clock; *out = g.exec; if (slot) *slot = &g; return IQLHIP_OK; }
  if (c->graphs.size() >= 12) {   // evict the least recently used — after its last replay has finished
    size_t lru = 0;
    for (size_t i = 1; i < c->graphs.size(); ++i) if (c->graphs[i].stamp < c->graphs[lru].stamp) lru = i;
    if (c->graphs[lru].last) HIPCHK(hipStreamSynchronize(c->graphs[lru].last));
    free_graph(c->graphs[lru]);
    c->graphs.erase(c->graphs.begin() + lru);
  }
  iqlhip_ctx::CachedGraph ng{key, nullptr, nullptr, 0, nullptr, nullptr, nullptr};
  if (int rc = build_chunk_graph(c, ng)) { free_graph(ng); return rc; }      // (whatever of it was made; the message stays)
  ng.stamp = ++c->graph_clock;
  c->graphs.push_back(ng);
  *out = ng.exec;
  if (slot) *slot = &c->graphs.back();
  return IQLHIP_OK;
}

static int check_train_args(const iqlhip_ctx* c, const float* rows_dev, int64_t ld, int32_t B) {
  if (!c || !rows_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (!c->params) return fail(IQLHIP_ENOTBOUND, "iqlhip_bind has not been called");
  if (B < 1 || B > c->dims.max_batch) return fail(IQLHIP_EINVAL, "batch_rows outside [1,max_batch]");
  if (ld != c->row_ld) return fail(IQLHIP_EINVAL, "row stride must be iqlhip_row_stride(S,A)=%lld", (long long)c->row_ld);
  if (((uintptr_t)rows_dev) & 15) return fail(IQLHIP_EINVAL, "packed rows must be 16-byte aligned");
  return IQLHIP_OK;
}

// Masks written by iqlhip_debug_write_masks fill one of the two keep-bit halves, and the chunks' steps alternate between
// the halves and draw the next step's bits as they go: the multi-step driver cannot honour injected masks, so it refuses
// while they are pending — before anything is launched or any position moves.
static int inject_check(const iqlhip_ctx* c) {
  if (c->drop_inject)
    return fail(IQLHIP_EUNSUPPORTED, "keep-bits injected by iqlhip_debug_write_masks are pending: iqlhip_train_steps draws "
                "its own (call iqlhip_set_dropout first, or step with iqlhip_step)");
  return IQLHIP_OK;
}

static GraphKey make_key(const iqlhip_ctx* c, const float* rows_dev, int64_t ld, int32_t B, int32_t K, float inv_batch,
                         int parity, int head, const ChunkSrc& src) {
  GraphKey key;
  key.head = head;
  key.src = src;
  key.rows = rows_dev; key.ld = ld; key.B = B; key.K = K; key.params = c->params; key.drop_p = c->drop_p;
  key.inv_batch = inv_batch; key.xch = c->xch_mode;
  key.parity = (c->xch_mode == IQLHIP_XCH_P2P) ? parity : 0;
  key.stats = c->stats_on ? 1 : 0;
  key.clip = c->clip_on ? 1 : 0;
  return key;
}

// Replay one chunk graph on `st`.  head: the call's first chunk — its set-up node gets this call's arguments first.
// How a call's first steps reach the GPU (IQLHIP_HEAD): "direct" (default) — the set-up kernel and the first 2 or 4
// steps are launched kernel by kernel, so the GPU has work ~3 us after the call instead of after a graph launch
// (~12 us), and the chunk launches that follow are hidden behind their execution; "graph" — round 3's first form, a head
// chunk graph whose first node is the set-up kernel; "plain" — set-up kernel + plain chunks only (diagnostic).
// profiles/r03_ab_experiments.txt #7: the driver's 20-step command 41.7 k -> 42.45 k steps/s with "direct".
static const int g_head_mode = [] {
  const char* e = getenv("IQLHIP_HEAD");
  if (e && !strcmp(e, "graph")) return 1;
  if (e && !strcmp(e, "plain")) return 2;
  return 0;
}();
static const bool g_direct_head = g_head_mode == 0;
static const bool g_no_head_graph = g_head_mode == 2;
static const bool g_direct_all = getenv("IQLHIP_DIRECT_ALL") != nullptr;           // diagnostic: no graph replays at all
// What is left of a call behind its head, as chunk graphs: n64 of 64 steps, and the rest in sizes 16, 4, 2 and 1,
// largest first (<= 3 + 3 + 1 + 1 entries).
struct ChunkPlan { int n64 = 0; int small[8]; int ns = 0; };
static ChunkPlan plan_chunks(int rem) {
  ChunkPlan pl;
  pl.n64 = rem / GRAPH_STEPS;
  rem %= GRAPH_STEPS;
  for (int cs_ : {16, 4, 2, 1}) while (rem >= cs_) { pl.small[pl.ns++] = cs_; rem -= cs_; }
  return pl;
}
static int n_chunks_for(int rem) { const ChunkPlan pl = plan_chunks(rem); return pl.n64 + pl.ns; }
static int replay_chunk(iqlhip_ctx* c, hipStream_t st, const float* rows_dev, int64_t ld, int B, int n, float inv_batch,
                        const SetupArgs* head_args, const ChunkSrc& src) {
  const int parity = (int)(c->xstep & 1ull);
  hipGraphExec_t gexec = nullptr;
  iqlhip_ctx::CachedGraph* cg = nullptr;
  int r = chunk_graph(c, make_key(c, rows_dev, ld, B, n, inv_batch, parity, head_args ? 1 : 0, src), &gexec, &cg);
  if (r) return r;
  if (g_direct_all && !head_args) {      // experiment: the chunk's kernels launched one by one instead of the graph replay
    r = enqueue_chunk(c, st, B, n, inv_batch, c->xch_mode, parity, cg->work, src);
    if (r) return r;
    chunk_queued(c, cg, st, n);
    return IQLHIP_OK;
  }
  if (head_args) {
    hipKernelNodeParams np;
    memset(&np, 0, sizeof np);
    np.func = const_cast<void*>(head_args->func);
    np.gridDim = dim3(head_args->nb);
    np.blockDim = dim3(256);
    np.kernelParams = const_cast<void**>(head_args->ptrs);
    HIPCHK(hipGraphExecKernelNodeSetParams(gexec, cg->setup_node, &np));
  }
  HIPCHK(hipGraphLaunch(gexec, st));
  chunk_queued(c, cg, st, n);
  return IQLHIP_OK;
}

// The five *_prepare entry points behind their argument checks: the chunk graphs of the call's kind, captured and
// rehearsed.
static int train_steps_prepare(iqlhip_ctx* c, const float* rows_dev, int64_t ld, int32_t B, float inv_batch, void* stream,
                               const ChunkCall& call) {
  int rc = IQLHIP_OK;
  if ((rc = step_entry(c, B, stream, /*multi_step=*/true))) return rc;
  DevGuard guard(c->device);
  HIPCHK(hipDeviceSynchronize());       // a one-off set-up call: ordered after everything queued on any stream
  c->cont.valid = false;
  // the rehearsal replays run on the CALLER's stream — the first replay of a graph on a stream it has not run on yet was
  // measured ~20 us slower than the following ones, rehearsed on another stream or not (capture itself happens on the
  // library's own stream: the legacy default stream cannot be captured)
  hipStream_t cs = (hipStream_t)stream;
  // Each chunk graph is captured, instantiated, uploaded AND replayed once, so that its first replay inside a caller's
  // timed region costs what every later one does (a first replay is ~50-100 us slower, and the first launch of a
  // kernel loads its code).  The rehearsal must not train: the parameter, moment and target arenas are saved before
  // and restored after it; it reads row 0 only (size = 1); scratch, loss words and ring are transient anyway.  Under
  // data parallelism the rehearsal runs the exchange too — every rank must call prepare (the same number of times).
  const size_t np_b = (size_t)c->L.n_params * sizeof(float), nt_b = (size_t)c->L.n_target * sizeof(float);
  if (!c->prep_save) HIPCHK(c->own.dev(&c->prep_save, 3 * np_b + nt_b));     // (arena sizes are fixed per context)
  char* const save = c->prep_save;
  auto copy_all = [&](bool restore) -> hipError_t {
    float* arenas[4] = {c->params, c->m, c->v, c->target};
    size_t off = 0;
    for (int i = 0; i < 4; ++i) {
      const size_t nb = (i == 3) ? nt_b : np_b;
      hipError_t e = restore ? hipMemcpyAsync(arenas[i], save + off, nb, hipMemcpyDeviceToDevice, cs)
                             : hipMemcpyAsync(save + off, arenas[i], nb, hipMemcpyDeviceToDevice, cs);
      if (e != hipSuccess) return e;
      off += nb;
    }
    return hipSuccess;
  };
  hipError_t e = copy_all(false);
  if (e != hipSuccess) return fail(IQLHIP_EHIP, "prepare: save arenas: %s", hipGetErrorString(e));
  refresh_shadows(c, cs);
  int slot = 0;
  rc = acquire_sched_slot(c, &slot);
  if (rc) return rc;
  const unsigned long long drop_step0 = c->drop_step;
  do {
    iqlhip_step_scalars benign;
    memset(&benign, 0, sizeof benign);
    benign.bc2_sqrt[0] = benign.bc2_sqrt[1] = benign.bc2_sqrt[2] = 1.f;
    benign.beta2 = 1.f; benign.eps = 1e-8f; benign.grad_scale = 1.f; benign.inv_batch = inv_batch;
    for (int k = 0; k < c->k_max; ++k) c->sched_pin[slot][k] = benign;
    // every chunk graph once: the head chunks (2 steps, and the one-step call's) with their set-up node, the plain ones
    // behind a directly launched set-up kernel.  P2P: a one-step chunk flips the buffer parity, so a second pass over
    // the same list reaches the other captured variant of each.
    const int passes = (c->xch_mode == IQLHIP_XCH_P2P) ? 2 : 1;
    struct Item { int K; int head; };
    const Item items[] = {{2, 1}, {GRAPH_STEPS, 0}, {16, 0}, {4, 0}, {2, 0}, {1, 0}};
    auto rehearse = [&](const Item& it) -> int {
      const ChunkHdr h = call_hdr(c, 1, 1, 0, 0);
      if (it.head) {
        SetupArgs a;
        if (int r = fill_setup_args(c, a, h, slot, it.K, rows_dev, B, /*gather=*/true, cs, call)) return r;
        return replay_chunk(c, cs, rows_dev, ld, B, it.K, inv_batch, &a, call.src);
      }
      int r = launch_call_setup(c, cs, h, slot, it.K, rows_dev, B, /*gather=*/true, call);
      if (r) return r;
      return replay_chunk(c, cs, rows_dev, ld, B, it.K, inv_batch, nullptr, call.src);
    };
    for (int pass = 0; pass < passes && !rc; ++pass)
      for (const Item& it : items) { if (it.head && g_head_mode != 1) continue; rc = rehearse(it); if (rc) break; }
    for (int pass = 0; pass < passes && !rc && g_head_mode == 1; ++pass) rc = rehearse(Item{1, 1});
    // Sustained replays of the 64-step chunk (benign scalars, row 0, arenas restored below like the rest of the
    // rehearsal): the chip's clocks ramp up over the first milliseconds of a workload — a timed region that starts right
    // behind a capture-heavy (GPU-idle) prepare call measured its first 20 steps ~5 % slower than the following ones
    // (profiles/r03_first_call.txt).  IQLHIP_PREPARE_WARM_CHUNKS: how many (default 16 = 1 024 steps, ~22 ms; 0 = none).
    static const int n_warm = getenv("IQLHIP_PREPARE_WARM_CHUNKS") ? std::max(0, atoi(getenv("IQLHIP_PREPARE_WARM_CHUNKS"))) : 16;
    if (!rc && n_warm > 0 && c->xch_mode == IQLHIP_XCH_NONE) {
      const ChunkHdr h = call_hdr(c, 1, 1, 0, 0);      // (no exchange here: the header's exchange step is not read)
      for (int i = 0; i < n_warm && !rc; ++i) {
        if ((i % (c->k_max / GRAPH_STEPS)) == 0) rc = launch_call_setup(c, cs, h, slot, c->k_max, rows_dev, B, /*gather=*/true, call);
        if (!rc) rc = replay_chunk(c, cs, rows_dev, ld, B, GRAPH_STEPS, inv_batch, nullptr, call.src);
      }
    }
  } while (0);
  c->drop_step = drop_step0;            // (the rehearsal drew keep-bits from the stream's current position; it is not advanced)
  e = copy_all(true);
  refresh_shadows(c, cs);
  hipError_t e2 = hipStreamSynchronize(cs);
  if (rc) return rc;
  if (e != hipSuccess || e2 != hipSuccess) return fail(IQLHIP_EHIP, "prepare: restore arenas: %s", hipGetErrorString(e != hipSuccess ? e : e2));
  return IQLHIP_OK;
}

extern "C" int iqlhip_train_steps_prepare(iqlhip_ctx* c, const float* rows_dev, int64_t ld, int32_t B, float inv_batch,
                                          void* stream) {
  int rc = check_train_args(c, rows_dev, ld, B);
  if (rc) return rc;
  return train_steps_prepare(c, rows_dev, ld, B, inv_batch, stream, ChunkCall());
}

// The five iqlhip_train_steps* entry points behind their argument checks (a mixed call: rows_dev / size are the offline
// buffer, size_on the rows the online part's draw covers; 0 for every other kind).
static int train_steps(iqlhip_ctx* c, const float* rows_dev, int64_t ld, int64_t size, int32_t B,
                       const iqlhip_step_scalars* sc, int32_t K, uint64_t seed, uint64_t stream_offset, int32_t flags,
                       void* stream, const ChunkCall& call, int64_t size_on) {
  const ChunkSrc& src = call.src;
  const KindInfo& ki = kind_info(src.kind);
  int rc = IQLHIP_OK;
  if (K < 1 || K > c->k_max) return fail(IQLHIP_EINVAL, "n_steps outside [1,%d]", c->k_max);
  if (size < 1) return fail(IQLHIP_EINVAL, "empty buffer");
  if ((rc = step_entry(c, B, stream, /*multi_step=*/true))) return rc;
  double tr_t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (g_trace) tr_t[0] = now_us();
  DevGuard guard(c->device);
  hipStream_t st = (hipStream_t)stream;
  // the call's scalar table goes into a pinned, host-mapped slot that the set-up kernel reads in place; a slot is
  // reused only after the set-up kernel that read it has run (event), so the caller's array is free on return
  int slot = 0;
  rc = acquire_sched_slot(c, &slot);
  if (rc) return rc;
  memcpy(c->sched_pin[slot], sc, (size_t)K * sizeof(iqlhip_step_scalars));
  const float inv_batch = sc[0].inv_batch;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (c->timing) {
    rc = ensure_events(c, c->ev_used + 2);
    if (rc) return rc;
    ev0 = c->ev[c->ev_used]; ev1 = c->ev[c->ev_used + 1];
    HIPCHK(hipEventRecord(ev0, st));
  }
  // does this call continue the previous one's index stream with its step 0 already staged?  (Never a mixed call: the
  // rows its last forward staged are not what a plain call would draw, so it claims nothing and leaves no token.)
  // A weighted call continues a weighted call on the same table generation only, and a plain call a plain one.
  // (the rows a call without staged q left cannot start a call that needs them, nor those of one without staged indices:
  //  cont_class; a prioritised call continues only a prioritised one: its rows were drawn one update behind, the lag-1 chain)
  const bool cont = ki.continues && (flags & IQLHIP_TS_CONTINUE) && c->cont.valid && !c->cont.owner && c->cont.wt_gen == call.wt_gen &&
                    c->cont.cont_class == ki.cont_class && c->cont.wt_ver == call.wt_ver &&
                    c->cont.rows == rows_dev && c->cont.ld == ld &&
                    c->cont.size == size && c->cont.B == B && c->cont.seed == seed && c->cont.next_offset == stream_offset &&
                    c->cont.drop_p == c->drop_p && c->cont.drop_seed == c->drop_seed && c->cont.drop_step == c->drop_step;
  c->cont.valid = false;
  const ChunkHdr h = call_hdr(c, size, size_on, seed, stream_offset);
  refresh_shadows(c, st);
  if (g_trace) tr_t[1] = now_us();
  // The call's HEAD — the set-up kernel and the first 2 or 4 steps (1 for a one-step call) — is launched kernel by
  // kernel (g_head_mode; a graph launch costs ~10 us + 0.4 us per node on the host and the GPU starts when it returns,
  // a kernel launch ~2.5 us).  The rest follows as chunk graphs, the even sizes ascending (each launch is hidden behind
  // the execution of what was launched before), the 64-step chunk as often as it fits, a one-step chunk — odd calls
  // only — last.
  int rem;
  if (g_direct_head) {
    // 2 or 4 steps (even: a chunk's step 0 reads staging buffer 0), whichever leaves fewer chunk launches behind it —
    // every launch boundary between chunks costs the GPU ~5 us (profiles/r03_train_steps_call_length.txt)
    const int head_k = (K >= 4 && n_chunks_for(K - 4) < n_chunks_for(K - 2)) ? 4 : ((K >= 2) ? 2 : 1);
    const int parity = (int)(c->xstep & 1ull);
    hipGraphExec_t gexec = nullptr;
    iqlhip_ctx::CachedGraph* cg = nullptr;
    rc = chunk_graph(c, make_key(c, rows_dev, ld, B, head_k, inv_batch, parity, 0, src), &gexec, &cg);     // (for its idle-work records)
    if (rc) return rc;
    rc = launch_call_setup(c, st, h, slot, K, rows_dev, B, /*gather=*/!cont, call);
    if (rc) return rc;
    rc = enqueue_chunk(c, st, B, head_k, inv_batch, c->xch_mode, parity, cg->work, src);
    if (rc) return rc;
    chunk_queued(c, cg, st, head_k);
    rem = K - head_k;
  } else if (g_no_head_graph) {
    rc = launch_call_setup(c, st, h, slot, K, rows_dev, B, /*gather=*/!cont, call);
    if (rc) return rc;
    rem = K;
  } else {
    const int head_k = (K >= 2) ? 2 : 1;
    SetupArgs a;
    if ((rc = fill_setup_args(c, a, h, slot, K, rows_dev, B, /*gather=*/!cont, st, call))) return rc;
    rc = replay_chunk(c, st, rows_dev, ld, B, head_k, inv_batch, &a, src);
    if (rc) return rc;
    rem = K - head_k;
  }
  if (g_trace) tr_t[2] = tr_t[3] = now_us();
  const ChunkPlan pl = plan_chunks(rem);
  for (int i = pl.ns - 1; i >= 0; --i) if (pl.small[i] != 1) { rc = replay_chunk(c, st, rows_dev, ld, B, pl.small[i], inv_batch, nullptr, src); if (rc) return rc; }
  for (int i = 0; i < pl.n64; ++i) { rc = replay_chunk(c, st, rows_dev, ld, B, GRAPH_STEPS, inv_batch, nullptr, src); if (rc) return rc; }
  if (pl.ns > 0 && pl.small[pl.ns - 1] == 1) { rc = replay_chunk(c, st, rows_dev, ld, B, 1, inv_batch, nullptr, src); if (rc) return rc; }
  // what a following call must look like to start on the rows this call's last forward has staged: an even number of
  // steps ends on staging buffer 0, where a chunk's step 0 reads; the next counter follows from the rows drawn
  if (ki.continues && (K & 1) == 0 && (((unsigned long long)K * (unsigned long long)B) & 1ull) == 0) {
    c->cont.valid = true;
    c->cont.owner = nullptr;
    // (a prioritised call moves its table's version by 1 itself: iqlhip_train_steps_prioritized)
    c->cont.wt_gen = call.wt_gen; c->cont.wt_ver = call.wt_ver + (ki.moves_version ? 1 : 0); c->cont.cont_class = ki.cont_class;
    c->cont.rows = rows_dev; c->cont.ld = ld; c->cont.size = size; c->cont.B = B; c->cont.seed = seed;
    c->cont.next_offset = stream_offset + ((unsigned long long)K * (unsigned long long)B) / 2ull;
    c->cont.drop_p = c->drop_p; c->cont.drop_seed = c->drop_seed; c->cont.drop_step = c->drop_step;
  }
  if (ev0) {
    HIPCHK(hipEventRecord(ev1, st));
    HIPCHK(hipEventSynchronize(ev1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
    c->t_acc[3] += ms * 1e3f;   // total per call; per-step = /K done by the caller
    c->t_n += 1;
  }
  HIPCHK(hipGetLastError());
  if (g_trace)
    fprintf(stderr, "[iqlhip trace] train_steps K=%d cont=%d: entry->launch %.1f us, head chunk (set-up + launch) %.1f, rest %.1f\n",
            K, (int)cont, tr_t[1] - tr_t[0], tr_t[2] - tr_t[1], now_us() - tr_t[3]);
  return IQLHIP_OK;
}

extern "C" int iqlhip_train_steps(iqlhip_ctx* c, const float* rows_dev, int64_t ld, int64_t size, int32_t B,
                                  const iqlhip_step_scalars* sc, int32_t K, uint64_t seed, uint64_t stream_offset,
                                  int32_t flags, void* stream) {
  if (!sc) return fail(IQLHIP_EINVAL, "NULL argument");
  int rc = check_train_args(c, rows_dev, ld, B);
  if (rc) return rc;
  return train_steps(c, rows_dev, ld, size, B, sc, K, seed, stream_offset, flags, stream, ChunkCall(), 0);
}

// ---------------------------------------------------------------------------
// Dataset ingest on the device.
extern "C" int iqlhip_cols_mean_std(const float* x_dev, int64_t ld, int32_t ncols, int64_t n, float eps, float* mean_dev,
                                    float* std_dev, void* stream) {
  if (!x_dev || !mean_dev || !std_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (ncols < 1 || ncols > 4096 || n < 1 || ld < ncols) return fail(IQLHIP_EINVAL, "bad cols_mean_std geometry");
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)std::min<int64_t>((n + 7) / 8, MS_BLOCKS);
  double* scratch = nullptr;                         // [nb][ncols] partials + [ncols] float64 means
  HIPCHK(hipMallocAsync((void**)&scratch, ((size_t)nb * ncols + ncols) * sizeof(double), st));
  double* mean64 = scratch + (size_t)nb * ncols;
  hipLaunchKernelGGL(iql_cols_moment_kernel<0>, dim3(nb), dim3(256), 0, st, x_dev, (long long)ld, ncols, (long long)n,
                     (const double*)nullptr, scratch);
  hipLaunchKernelGGL(iql_cols_finish_kernel<0>, dim3((ncols + 63) / 64), dim3(64), 0, st, (const double*)scratch, nb, ncols,
                     (long long)n, eps, mean64, mean_dev);
  hipLaunchKernelGGL(iql_cols_moment_kernel<1>, dim3(nb), dim3(256), 0, st, x_dev, (long long)ld, ncols, (long long)n,
                     (const double*)mean64, scratch);
  hipLaunchKernelGGL(iql_cols_finish_kernel<1>, dim3((ncols + 63) / 64), dim3(64), 0, st, (const double*)scratch, nb, ncols,
                     (long long)n, eps, mean64, std_dev);
  HIPCHK(hipFreeAsync(scratch, st));
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

extern "C" int iqlhip_rows_normalize(float* rows_dev, int64_t ld, int32_t S, int32_t A, int64_t row0, int64_t n,
                                     const float* mean_dev, const float* std_dev, void* stream) {
  if (!rows_dev || !mean_dev || !std_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n < 0 || row0 < 0 || S < 1 || A < 1 || ld < 2 * (int64_t)S + A + 2) return fail(IQLHIP_EINVAL, "bad rows_normalize geometry");
  if (n == 0) return IQLHIP_OK;
  const long long total = (long long)n * 2 * S;
  const int nb = (int)std::min<long long>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(iql_rows_normalize_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, rows_dev, (long long)ld, S, A,
                     (long long)row0, (long long)n, mean_dev, std_dev);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

// ---------------------------------------------------------------------------
// Reward ingest (return_reward_range / modify_reward, algorithms/finetune/iql.py:262-289): kernels in iqlhip_kernels.h.
static int reward_args_ok(const void* rows_dev, int64_t ld, int32_t S, int32_t A, int64_t row0, int64_t n, const char* who) {
  if (!rows_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n < 1 || row0 < 0 || S < 1 || A < 1 || ld < iqlhip_row_stride(S, A)) return fail(IQLHIP_EINVAL, "bad %s geometry", who);
  return IQLHIP_OK;
}

static int launch_return_range(const float* rows_dev, long long ld, int S, int A, long long row0, long long n, long long T,
                               char* scratch, RRResult* res_host, hipStream_t st) {
  const long long ntiles = (n + RR_TILE - 1) / RR_TILE;
  const int nb = (int)std::min<long long>(ntiles, RR_MAX_BLOCKS);
  // scratch: prev[n] | tile partials[ntiles] | block results[nb] | result
  long long* prev = (long long*)scratch;
  long long* tiles = prev + n;
  RRResult* blocks = (RRResult*)(tiles + ntiles);
  RRResult* res = blocks + nb;
  const int rcol = 2 * S + A, dcol = rcol + 1;
  hipLaunchKernelGGL(iql_rr_scan_reduce_kernel, dim3(nb), dim3(RR_TILE), 0, st, rows_dev, ld, dcol, row0, n, ntiles, tiles);
  hipLaunchKernelGGL(iql_rr_scan_partials_kernel, dim3(1), dim3(RR_TILE), 0, st, tiles, ntiles);
  hipLaunchKernelGGL(iql_rr_scan_apply_kernel, dim3(nb), dim3(RR_TILE), 0, st, rows_dev, ld, dcol, row0, n, ntiles,
                     (const long long*)tiles, prev);
  hipLaunchKernelGGL(iql_rr_episode_kernel, dim3(nb), dim3(RR_TILE), 0, st, rows_dev, ld, rcol, row0, n, ntiles, T,
                     (const long long*)prev, blocks);
  hipLaunchKernelGGL(iql_rr_finish_kernel, dim3(1), dim3(RR_TILE), 0, st, (const RRResult*)blocks, nb, res);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(res_host, res, sizeof(RRResult), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return IQLHIP_OK;
}

extern "C" int iqlhip_rows_return_range(const float* rows_dev, int64_t ld, int32_t S, int32_t A, int64_t row0, int64_t n,
                                        int32_t max_episode_steps, double out_min_max[2], int64_t* out_episodes,
                                        void* stream) {
  if (!out_min_max || !out_episodes) return fail(IQLHIP_EINVAL, "NULL argument");
  int rc = reward_args_ok(rows_dev, ld, S, A, row0, n, "rows_return_range");
  if (rc) return rc;
  if (max_episode_steps < 1) return fail(IQLHIP_EINVAL, "max_episode_steps must be at least 1");
  hipStream_t st = (hipStream_t)stream;
  const long long ntiles = ((long long)n + RR_TILE - 1) / RR_TILE;
  const size_t bytes = ((size_t)n + (size_t)ntiles) * sizeof(long long) + ((size_t)std::min<long long>(ntiles, RR_MAX_BLOCKS) + 1) * sizeof(RRResult);
  char* scratch = nullptr;
  HIPCHK(hipMallocAsync((void**)&scratch, bytes, st));
  RRResult res;
  rc = launch_return_range(rows_dev, (long long)ld, S, A, (long long)row0, (long long)n, (long long)max_episode_steps,
                           scratch, &res, st);
  const hipError_t e = hipFreeAsync(scratch, st);
  if (rc) return rc;
  HIPCHK(e);
  *out_episodes = (int64_t)res.episodes;
  if (res.episodes < 1)       // the reference's min([]) raises ValueError
    return fail(IQLHIP_EINVAL, "no complete episode in %lld rows (no terminal, and fewer than max_episode_steps = %d rows)",
                (long long)n, (int)max_episode_steps);
  out_min_max[0] = res.min_ret;
  out_min_max[1] = res.max_ret;
  return IQLHIP_OK;
}

static int launch_reward_map(bool shift, float* rows_dev, int64_t ld, int32_t S, int32_t A, int64_t row0, int64_t n, float a,
                             float b, void* stream) {
  const int nb = (int)std::min<int64_t>((n + 255) / 256, 8192);
  if (shift)
    hipLaunchKernelGGL(iql_rows_reward_map_kernel<true>, dim3(nb), dim3(256), 0, (hipStream_t)stream, rows_dev, (long long)ld,
                       2 * S + A, (long long)row0, (long long)n, a, b);
  else
    hipLaunchKernelGGL(iql_rows_reward_map_kernel<false>, dim3(nb), dim3(256), 0, (hipStream_t)stream, rows_dev, (long long)ld,
                       2 * S + A, (long long)row0, (long long)n, a, b);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

extern "C" int iqlhip_rows_reward_scale(float* rows_dev, int64_t ld, int32_t S, int32_t A, int64_t row0, int64_t n,
                                        float divide_by, float multiply_by, void* stream) {
  const int rc = reward_args_ok(rows_dev, ld, S, A, row0, n, "rows_reward_scale");
  if (rc) return rc;
  if (divide_by == 0.f) return fail(IQLHIP_EINVAL, "divide_by is zero (max_ret == min_ret)");
  return launch_reward_map(false, rows_dev, ld, S, A, row0, n, divide_by, multiply_by, stream);
}

extern "C" int iqlhip_rows_reward_shift(float* rows_dev, int64_t ld, int32_t S, int32_t A, int64_t row0, int64_t n,
                                        float subtract, void* stream) {
  const int rc = reward_args_ok(rows_dev, ld, S, A, row0, n, "rows_reward_shift");
  if (rc) return rc;
  return launch_reward_map(true, rows_dev, ld, S, A, row0, n, subtract, 0.f, stream);
}

// ---------------------------------------------------------------------------
extern "C" int iqlhip_rows_fill_synth(float* rows_dev, int64_t ld, int32_t S, int32_t A, int64_t row0, int64_t n,
                                      uint64_t seed, float p_done, int32_t antmaze_rewards, void* stream) {
  if (!rows_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n < 0 || row0 < 0 || S < 1 || A < 1 || ld < 2 * (int64_t)S + A + 2) return fail(IQLHIP_EINVAL, "bad rows_fill_synth geometry");
  if (!(p_done >= 0.f && p_done <= 1.f)) return fail(IQLHIP_EINVAL, "p_done outside [0,1]");
  if (n == 0) return IQLHIP_OK;
  const long long total = (long long)n * (2 * S + A + 2);
  const int nb = (int)std::min<long long>((total + 255) / 256, 16384);
  hipLaunchKernelGGL(iql_rows_fill_synth_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, rows_dev, (long long)ld, S, A,
                     (long long)row0, (long long)n, (unsigned long long)seed, p_done, (int)antmaze_rewards);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

// ---------------------------------------------------------------------------
extern "C" int iqlhip_rows_write(float* rows_dev, int64_t ld, int32_t S, int32_t A, int64_t row0, int64_t n,
                                 const float* s, const float* a, const float* r, const float* ns, const float* d,
                                 void* stream) {
  if (!rows_dev || !s || !a || !r || !ns || !d) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n < 0 || row0 < 0 || ld < 2 * (int64_t)S + A + 2) return fail(IQLHIP_EINVAL, "bad rows_write geometry");
  if (n == 0) return IQLHIP_OK;
  const long long total = (long long)n * (2 * S + A + 2);
  const int nb = (int)std::min<long long>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(iql_rows_write_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, rows_dev, (long long)ld, S, A,
                     (long long)row0, (long long)n, s, a, r, ns, d);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

extern "C" int iqlhip_rows_gather(const float* rows_dev, int64_t ld, int64_t n_rows, int32_t S, int32_t A,
                                  const int64_t* idx_dev, int64_t n, float* s, float* a, float* r, float* ns, float* d,
                                  void* stream) {
  if (!rows_dev || !idx_dev || !s || !a || !r || !ns || !d) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n < 0 || n_rows < 1 || ld < 2 * (int64_t)S + A + 2) return fail(IQLHIP_EINVAL, "bad rows_gather geometry");
  if (n == 0) return IQLHIP_OK;
  const long long total = (long long)n * (2 * S + A + 2);
  const int nb = (int)std::min<long long>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(iql_rows_gather_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, rows_dev, (long long)ld,
                     (long long)n_rows, S, A, (const long long*)idx_dev, (long long)n, s, a, r, ns, d);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

// ReplayBuffer.sample as ONE coalesced row gather: out[i] = rows[idx[i]] (whole packed rows).
extern "C" int iqlhip_rows_gather_packed(const float* rows_dev, int64_t ld, int64_t n_rows, const int64_t* idx_dev,
                                         int64_t n, float* out_rows_dev, void* stream) {
  if (!rows_dev || !idx_dev || !out_rows_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n < 0 || n_rows < 1 || ld < 4 || (ld & 3)) return fail(IQLHIP_EINVAL, "bad rows_gather_packed geometry");
  if ((((uintptr_t)rows_dev) | ((uintptr_t)out_rows_dev)) & 15) return fail(IQLHIP_EINVAL, "rows must be 16-byte aligned");
  if (n == 0) return IQLHIP_OK;
  const long long total = (long long)n * (ld / 4);
  if (total > 0x7fffffffLL) return fail(IQLHIP_EINVAL, "gather too large for one call");
  hipLaunchKernelGGL(iql_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rows_dev,
                     (long long)ld, (const long long*)idx_dev, out_rows_dev, (int)n, (long long)n_rows);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

extern "C" int iqlhip_stream_synchronize(void* stream) {
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return IQLHIP_OK;
}

// The same with the indices still on the host (pinned): one H2D copy into idx_scratch_dev, then the gather —
// ReplayBuffer.sample's whole device side in one call.
extern "C" int iqlhip_rows_gather_packed_h(const float* rows_dev, int64_t ld, int64_t n_rows, const int64_t* idx_host,
                                           int64_t* idx_scratch_dev, int64_t n, float* out_rows_dev, void* stream) {
  if (!idx_host || !idx_scratch_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n < 0 || n_rows < 1) return fail(IQLHIP_EINVAL, "bad rows_gather_packed_h geometry");
  if (n == 0) return IQLHIP_OK;
  int rc = check_host_indices(idx_host, n, n_rows);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(idx_scratch_dev, idx_host, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, (hipStream_t)stream));
  return iqlhip_rows_gather_packed(rows_dev, ld, n_rows, idx_scratch_dev, n, out_rows_dev, stream);
}

// ReplayBuffer.sample in one call from ORDINARY host memory (the array np.random.randint returned): the indices are
// copied into a pinned ring slot owned by the library (guarded by an event, so a slot is never rewritten while its
// H2D copy may still be queued), sent to a device scratch array on `stream`, and the rows gathered.  Per device
// state, created on first use; like the rest of the ABI not thread-safe.
namespace {
struct SampleStage {
  int device = -1;
  int64_t cap = 0;
  enum { SLOTS = 8 };
  Owned own;                             // ack and arrivals, then (from slots_mark on) the index slots: re-made when they grow
  size_t slots_mark = 0;
  int64_t* host[SLOTS] = {};             // pinned, host-mapped index slots the gather kernel reads in place
  unsigned long long want[SLOTS] = {};   // the call number whose kernel must have acknowledged the slot before reuse
  hipStream_t stream[SLOTS] = {};
  unsigned long long* ack = nullptr;     // pinned [SLOTS]: written by the gather kernels
  unsigned* arrivals = nullptr;          // device block counter
  unsigned long long seq = 0;
  int slot = 0;
};
// (process lifetime: never destroyed, so nothing is freed behind the runtime's back at exit)
SampleStage* const g_stage = new SampleStage[16];
}  // namespace

// ReplayBuffer.sample in one call from ORDINARY host memory (the array np.random.randint returned): the indices are
// copied into a pinned, host-mapped slot owned by the library and the gather kernel reads them THERE (2 KB over PCIe) —
// no H2D copy, no event; a slot is reused only after its kernel has acknowledged it in a host-mapped word.  Per-device
// state, created on first use; like the rest of the ABI not thread-safe.
extern "C" int iqlhip_rows_sample_packed(const float* rows_dev, int64_t ld, int64_t n_rows, const int64_t* idx_host,
                                         int64_t n, float* out_rows_dev, void* stream) {
  if (!rows_dev || !idx_host || !out_rows_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n < 0 || n_rows < 1 || ld < 4 || (ld & 3)) return fail(IQLHIP_EINVAL, "bad rows_sample_packed geometry");
  if ((((uintptr_t)rows_dev) | ((uintptr_t)out_rows_dev)) & 15) return fail(IQLHIP_EINVAL, "rows must be 16-byte aligned");
  if (n == 0) return IQLHIP_OK;
  {
    int rc = check_host_indices(idx_host, n, n_rows);
    if (rc) return rc;
  }
  const long long total = (long long)n * (ld / 4);
  if (total > 0x7fffffffLL) return fail(IQLHIP_EINVAL, "gather too large for one call");
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 16) return fail(IQLHIP_EUNSUPPORTED, "device index %d", dev);
  SampleStage& sg = g_stage[dev];
  if (sg.cap < n) {
    HIPCHK(hipDeviceSynchronize());          // nothing may still read the old staging
    if (!sg.ack) {
      const int rc = all_or_nothing(sg.own, [&]() -> int {
        HIPCHK(sg.own.pin(&sg.ack, SampleStage::SLOTS * sizeof(unsigned long long), /*zero=*/true));
        HIPCHK(sg.own.dev(&sg.arrivals, 64, 0));
        return IQLHIP_OK;
      });
      if (rc) return rc;
      HIPCHK(hipDeviceSynchronize());
      sg.slots_mark = sg.own.mark();
    }
    sg.own.rollback(sg.slots_mark);          // (the old slots)
    sg.cap = 0;
    const int64_t cap = std::max<int64_t>(n, 1024);
    const int rc = all_or_nothing(sg.own, [&]() -> int {
      for (int i = 0; i < SampleStage::SLOTS; ++i) {
        HIPCHK(sg.own.pin(&sg.host[i], (size_t)cap * sizeof(int64_t)));
        sg.want[i] = 0;
      }
      return IQLHIP_OK;
    });
    if (rc) return rc;
    sg.cap = cap;
    sg.device = dev;
  }
  const int k = sg.slot;
  sg.slot = (sg.slot + 1) % SampleStage::SLOTS;
  {
    const volatile unsigned long long* ack = sg.ack + k;
    if (*ack < sg.want[k]) {                 // eight samples deep in flight: wait for that slot's kernel
      for (int spin = 0; spin < 20000 && *ack < sg.want[k]; ++spin) {}
      if (*ack < sg.want[k] && sg.stream[k]) HIPCHK(hipStreamSynchronize(sg.stream[k]));
    }
  }
  memcpy(sg.host[k], idx_host, (size_t)n * sizeof(int64_t));
  sg.want[k] = ++sg.seq;
  sg.stream[k] = (hipStream_t)stream;
  hipLaunchKernelGGL(iql_gather_hostidx_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rows_dev,
                     (long long)ld, (const long long*)sg.host[k], out_rows_dev, (int)n, (long long)n_rows, sg.arrivals, sg.ack + k, sg.want[k]);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

// ---------------------------------------------------------------------------
// Policy inference: pack states -> forward of the policy instance only -> tanh / noise / scale / clamp.

extern "C" int iqlhip_actor_forward(iqlhip_ctx* c, const float* states_dev, int64_t ld_s, int32_t rows,
                                    const float* noise_dev, int64_t ld_noise, float max_action, float* actions_dev,
                                    int64_t ld_a, void* stream) {
  return actor_forward_impl(c, states_dev, ld_s, rows, noise_dev, ld_noise, 0, 0, max_action, actions_dev, ld_a, stream);
}

// dist.sample() with the noise drawn on the device: seed != 0 selects the stream, the library counts the calls.
extern "C" int iqlhip_actor_sample(iqlhip_ctx* c, const float* states_dev, int64_t ld_s, int32_t rows, uint64_t seed,
                                   float max_action, float* actions_dev, int64_t ld_a, void* stream) {
  if (!c) return fail(IQLHIP_EINVAL, "NULL argument");
  if (seed == 0) return fail(IQLHIP_EINVAL, "seed must be non-zero");
  return actor_forward_impl(c, states_dev, ld_s, rows, nullptr, 0, seed, c->act_calls++, max_action, actions_dev, ld_a,
                            stream);
}

static int actor_forward_impl(iqlhip_ctx* c, const float* states_dev, int64_t ld_s, int32_t rows, const float* noise_dev,
                              int64_t ld_noise, uint64_t rng_seed, uint64_t rng_call, float max_action,
                              float* actions_dev, int64_t ld_a, void* stream, unsigned long long* done_flag,
                              unsigned long long done_val) {
  if (!c || !states_dev || !actions_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (!c->params) return fail(IQLHIP_EINVAL, "iqlhip_bind has not been called");
  const int S = c->dims.state_dim, A = c->dims.action_dim;
  if (rows < 0 || rows > c->act_cap) return fail(IQLHIP_EINVAL, "rows %d outside [0, %d]", rows, c->act_cap);
  if (ld_s < S || ld_a < A || (noise_dev && ld_noise < A)) return fail(IQLHIP_EINVAL, "row stride smaller than the row");
  if (rows == 0) return IQLHIP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int total = rows * (int)c->row_ld;
  const ActDropRec drop = act_drop_record(c, rows);
  if (drop.active) {       // the call's keep-bits come from the packing launch; the stream moves on by one call
    hipLaunchKernelGGL(iql_pack_states_drop_kernel, dim3((total + 255) / 256 + (2 * rows * 8 + 255) / 256), dim3(256), 0, st,
                       c->xb_act, (int)c->row_ld, S, rows, states_dev, (long long)ld_s, drop);
    c->act_drop_calls += 1;
  } else {
    hipLaunchKernelGGL(iql_pack_states_kernel, dim3((total + 255) / 256), dim3(256), 0, st, c->xb_act, (int)c->row_ld, S,
                       rows, states_dev, (long long)ld_s);
  }
  refresh_shadows(c, st);
  const StepParams p = act_step_params(c, rows);
  const int n_rt = (rows + RT_ROWS - 1) / RT_ROWS;
  launch_fwd_grid(c, p, n_rt * NSPLIT, st);
  hipLaunchKernelGGL(iql_actor_finish_kernel, dim3((rows * A + 255) / 256), dim3(256), 0, st, c->heads_act, rows, A,
                     max_action, p.log_std, c->hyper.log_std_min, c->hyper.log_std_max, noise_dev, (long long)ld_noise,
                     (unsigned long long)rng_seed, (unsigned long long)rng_call, actions_dev, (long long)ld_a,
                     (rows * A <= 256) ? done_flag : (unsigned long long*)nullptr, done_val);
  if (done_flag && rows * A > 256) return fail(IQLHIP_EINVAL, "a completion flag needs a one-block finish launch");
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

// Diagnostic: queue a kernel that writes a fresh number into a host-mapped word, then spin on that word from the host
// (no HIP call): *spin_us = time until the GPU has drained `stream`, as the host sees it without any synchronise call.
extern "C" int iqlhip_debug_drain_spin(iqlhip_ctx* c, void* stream, double* spin_us) {
  if (!c || !spin_us) return fail(IQLHIP_EINVAL, "NULL argument");
  const double t0 = now_us();
  const unsigned long long v = ++c->call_seq;
  hipLaunchKernelGGL(iql_debug_flag_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, c->sched_ack + 5, v);
  const volatile unsigned long long* f = c->sched_ack + 5;
  while (*f != v) { if (now_us() - t0 > 5e6) return fail(IQLHIP_EHIP, "drain_spin: timeout"); }
  *spin_us = now_us() - t0;
  return IQLHIP_OK;
}

// ---------------------------------------------------------------------------
// Micro-benchmark hook: launch ONE kernel of the step `repeat` times back to back and return the
// average time per launch (hipEvents on `stream`).  which: 0 fwd, 1 bwd, 2 update (no-op scalars:
// step_size 0, so parameters do not move), 3 fwd+bwd+update; large-batch bf16 path: 4 = the backward's row kernel alone,
// 5 = its GEMM kernel alone.  Synchronous.
extern "C" int iqlhip_debug_time_kernel(iqlhip_ctx* c, const iqlhip_batch* b, int which, int repeat, float* avg_us,
                                        void* stream) {
  if (!c || !avg_us || repeat < 1) return fail(IQLHIP_EINVAL, "bad argument");
  int rc = check_batch(c, b);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const float* xb_cur = nullptr;
  rc = stage_batch(c, b, st, &xb_cur);
  if (rc) return rc;
  iqlhip_step_scalars sc;
  memset(&sc, 0, sizeof sc);
  sc.bc2_sqrt[0] = sc.bc2_sqrt[1] = sc.bc2_sqrt[2] = 1.f;
  sc.beta2 = 1.f; sc.eps = 1e-8f; sc.grad_scale = 1.f; sc.inv_batch = 1.f / b->rows;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  Owned events;                          // (released on every way out; declared behind the two it nulls)
  HIPCHK(events.event(&e0, hipEventDefault));
  HIPCHK(events.event(&e1, hipEventDefault));
  EagerStep e;
  eager_begin(c, b->rows, &sc, st, xb_cur, e, /*draw=*/false);
  const StepParams& p = e.p;
  UpdParams& u = e.u;
  u.tau = 0.f; u.one_minus_tau = 1.f;
  for (int w = 0; w < 3; ++w) { launch_fwd(c, p, st); launch_bwd(c, p, st); }
  HIPCHK(hipEventRecord(e0, st));
  c->lb_bwd_part = (which == 4) ? 1 : ((which == 5) ? 2 : 0);
  for (int i = 0; i < repeat; ++i) {
    if (which == 0 || which == 3) launch_fwd(c, p, st);
    if (which == 1 || which == 3 || which == 4 || which == 5) launch_bwd(c, p, st);
    if (which == 2 || which == 3) launch_upd(c, u, st);
  }
  c->lb_bwd_part = 0;
  HIPCHK(hipEventRecord(e1, st));
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  *avg_us = ms * 1e3f / repeat;
  return IQLHIP_OK;
}

// ---------------------------------------------------------------------------
extern "C" int iqlhip_debug_read(iqlhip_ctx* c, const char* name, float* host_out, int64_t max_floats, int64_t* n_out,
                                 void* stream) {
  if (!c || !name || !host_out) return fail(IQLHIP_EINVAL, "NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const float* src = nullptr;
  int64_t n = 0;
  const int MB = c->dims.max_batch;
  if (!strcmp(name, "h0")) { src = c->sc.h0; n = (int64_t)4 * MB * HID; }
  else if (!strcmp(name, "h1")) { src = c->sc.h1; n = (int64_t)4 * MB * HID; }
  else if (!strcmp(name, "heads")) { src = c->sc.heads; n = (int64_t)MB * HEAD_LD + (int64_t)NSPLIT * MB * c->dims.action_dim; }
  else if (!strcmp(name, "loss_parts")) { src = c->sc.loss_parts; n = 4 * 64; }
  else if (!strcmp(name, "xb")) { src = c->xb; n = (int64_t)MB * c->row_ld; }      // the packed batch of the last eager step
  else if (!strcmp(name, "drop_bits")) { src = (const float*)c->drop_bits; n = (int64_t)2 * MB * 8; }
  else if (!strcmp(name, "act_drop_bits")) {
    if (!c->act_drop_bits) return fail(IQLHIP_EINVAL, "no inference keep-bits: iqlhip_set_act_dropout has set no rate > 0");
    src = (const float*)c->act_drop_bits; n = (int64_t)2 * c->act_cap * 8;
  }
  else if (!strcmp(name, "stamps")) {   // 64-bit stamps returned as pairs of 32-bit words
    if (!c->stamps) return fail(IQLHIP_EINVAL, "library built without -DIQL_STAMPS");
    src = (const float*)c->stamps; n = 4096 * 16 * 2;
  }
  else if (!strcmp(name, "grads")) {
    // flatten the slabs of the LAST forward_backward/step with the batch size implied by max_batch slabs in use
    return fail(IQLHIP_EINVAL, "use iqlhip_forward_backward to obtain the flat gradient");
  } else return fail(IQLHIP_EINVAL, "unknown scratch array '%s'", name);
  if (n > max_floats) n = max_floats;
  HIPCHK(hipMemcpyAsync(host_out, src, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (n_out) *n_out = n;
  return IQLHIP_OK;
}

// ---------------------------------------------------------------------------
// Trainer groups (include/iqlhip.h): K contexts of identical dims stepped together.  Every launch of a group step covers
// all K agents (grid.y = agent); each agent's launch arguments are a device-resident GroupRec (iqlhip_kernels.h) the
// host writes once per call, together with the agents' scalar tables, in ONE host-to-device copy from pinned memory.
// A group created with IQLHIP_GROUP_DROPOUT also uploads one GroupDropRec per member in that copy: the members' actor
// dropout keep-bits are drawn by the group's own launches, each from the member's own stream (seed, rate, position).

// (Staging, Section<T>: iqlhip_staging.h.)
// The per-member records of the opt-in features that look at a step's gradient, as they lie in a staging: the
// statistics records, the clip records, and the records the block-partial launch runs under when some member clips.
struct AuxSections {
  Section<GroupStatsRec> srecs; Section<GroupClipRec> crecs; Section<GroupStatsRec> gqrecs;
  void add(Staging& s, size_t k) {
    srecs = s.add<GroupStatsRec>(k);
    crecs = s.add<GroupClipRec>(k);
    gqrecs = s.add<GroupStatsRec>(k);
  }
};
// A staging the group's training calls run from, and what every one of them has in it: the agents' records (one set,
// or one per half of the members' double-buffered rows), the dropout records, the statistics / clip records per set,
// and the scalar tables, [k][IQLHIP_GROUP_MAX_STEPS] — the staging's last section: upload_steps copies up to their
// used rows.  The owner lays it out (its other sections lie between these).
struct GroupStage {
  Staging stg;
  Section<GroupRec> recs[2]; Section<GroupDropRec> drops; AuxSections aux[2]; Section<iqlhip_step_scalars> tabs;
  // Agent i's scalar table: the host copy the caller's rows go to, and its device address.
  iqlhip_step_scalars* tab(int i) const { return stg.host(tabs) + (size_t)i * IQLHIP_GROUP_MAX_STEPS; }
  const iqlhip_step_scalars* sched(int i) const { return stg.device(tabs) + (size_t)i * IQLHIP_GROUP_MAX_STEPS; }
  // records + the first n rows of every one of the k agents' tables (the tables are strided by IQLHIP_GROUP_MAX_STEPS)
  hipError_t upload_steps(int k, int n, hipStream_t st) {
    return stg.upload(tabs.off + ((size_t)(k - 1) * IQLHIP_GROUP_MAX_STEPS + (size_t)n) * sizeof(iqlhip_step_scalars), st);
  }
};

struct ScoreParams; struct ScoreRowsParams; struct ScoreGroupAux;      // (iqlhip_score_kernels.h, included further down)
struct GroupRwRec; struct GroupPrioRec;                                // (iqlhip_group_prio_kernels.h, included further down)
struct GroupVecRec;                                                    // (iqlhip_group_online_vec_kernels.h, the file's last include)
struct iqlhip_group {
  int k = 0;
  int device = 0;
  int flags = 0;                      // IQLHIP_GROUP_*
  iqlhip_ctx* m[IQLHIP_MAX_GROUP] = {};
  Owned own;                          // every buffer and event of the group (the members own theirs)
  // iqlhip_group_step / iqlhip_group_train_steps: one record set, dropout records only with IQLHIP_GROUP_DROPOUT (no rows
  // without the flag).  (An asynchronous call: the staging waits for its upload before the next call rewrites it.)
  GroupStage train;
  Section<GroupWtRec> wts;            // iqlhip_group_train_steps_weighted: one table record per member (before the tables)
  // clip_ones: three floats of 1.0f, the coefficients a member without clipping reads (allocated by the first call
  // with a clipping member)
  float* clip_ones = nullptr;
  // per-step statistics of the members that enabled them (iqlhip_set_step_stats): [k][IQLHIP_GROUP_MAX_STEPS][IQLHIP_N_STATS],
  // allocated by the first call with such a member; stats_mask: who had them on in the last call
  float* stats_ring_dev = nullptr;
  float* stats_ring_pin = nullptr;
  bool stats_mask[IQLHIP_MAX_GROUP] = {};
  float* ring_dev = nullptr;          // [k][IQLHIP_GROUP_MAX_STEPS][4] losses of the last call
  float* ring_pin = nullptr;
  int last_n = 0;                     // steps of the last call (rows of the ring that are valid)
  // iqlhip_group_online_step: its own records (a synchronous call — the staging is free again when it returns, so it
  // has no upload event): the
  // agents' records, the act forwards' and the ring writes + gathers', the act finishes', the dropout records (as above)
  // and one row of scalars per agent
  Staging on;
  Section<GroupRec> on_recs; Section<StepParams> on_aps; Section<GroupOnlineRec> on_gathers; Section<GroupActRec> on_fins;
  Section<GroupDropRec> on_drops; Section<ActDropRec> on_adrops; Section<iqlhip_step_scalars> on_tabs;
  AuxSections on_aux;
  unsigned long long* done_pin = nullptr;   // host-mapped completion word of the call (the host spins on it)
  unsigned long long done_seq = 0;
  // iqlhip_group_actor_forward: its own records — the state packs', the forwards', the finishes' — built in the staging's
  // build buffer and uploaded only when they differ from the last upload: an evaluation loop's calls repeat theirs.
  CachedStaging act;
  Section<GroupPackRec> act_packs; Section<StepParams> act_ps; Section<GroupActRowsRec> act_fins;
  Section<ActDropRec> act_drops;      // (IQLHIP_GROUP_DROPOUT groups: the inference keep-bit draws, indexed like act_packs)
  // iqlhip_group_score_rows: the scratch of a chunk of every member — member i's regions start at i * score_chunk rows
  // (score_chunk = the largest chunk a member scores: 65 536 / k rows, so the k members together take what one solo
  // context's scratch takes) — and the call's records, which go the way the act records go.  All of it is
  // allocated by the group's first scoring call; a group that never scores holds none.
  int score_chunk = 0;
  float* score_heads = nullptr;       // device [k][score_chunk][HEAD_LD]
  float* score_pi = nullptr;          // device [k][score_chunk][A][NSPLIT]
  float* score_part = nullptr;        // device [k][score_chunk / 32][SCORE_N_PART]
  float* score_out = nullptr;         // device [k][score_chunk][IQLHIP_N_SCORE]: rows of members without an out (for the spread)
  double* score_acc = nullptr;        // device [k][16]: the call's running sums
  float* score_pin = nullptr;         // pinned, host-mapped [k][16]: the summaries' landing words
  unsigned long long* score_status = nullptr;   // pinned, host-mapped [k][2]: the index check's verdicts
  CachedStaging score;
  Section<ScoreParams> score_ps; Section<ScoreRowsParams> score_qs; Section<ScoreGroupAux> score_aux;
  // iqlhip_group_step_rw, iqlhip_group_train_steps_weighted_is / _prioritized (DESIGN.md 6j "trainer groups"): a staging
  // of their own, allocated by the group's first such call — the plain calls upload what they always did.  The agents'
  // records twice — set h has the pointers of staging half h: a burst's step s runs under set s & 1, an eager step under
  // set 0 — the dropout records (k, whatever the flags), the statistics / clip records per set, the row-weight and the
  // draw / update records (rw_rws, rw_prs), and the scalar tables last.
  // rw_ones: max over the members' max_batch floats of 1.0f, the weights of a member given none.
  GroupStage rw;
  Section<GroupRwRec> rw_rws; Section<GroupPrioRec> rw_prs;
  float* rw_ones = nullptr;
  // iqlhip_group_online_step_vec (DESIGN.md 6b "group vector-environment online step"), all of it made by the group's
  // first such call.  A staging of its own (a synchronous call: no upload event): the gather records, the inference
  // keep-bit records (both indexed by member), the act forwards' and finishes' records (packed: requesting members), then
  // one block per step — the agents' records, the packed dropout records, the statistics / clip records and one row of
  // scalars per agent — so that a call uploads the prefix its n_updates steps use (vec_end[u]: the bytes up to and
  // including step u's block; vec_head: those in front of step 0's).
  Staging vec;
  Section<GroupVecRec> vec_gathers; Section<ActDropRec> vec_adrops; Section<StepParams> vec_aps; Section<GroupActRowsRec> vec_fins;
  struct VecStep { Section<GroupRec> recs; Section<GroupDropRec> drops; AuxSections aux; Section<iqlhip_step_scalars> tabs; };
  VecStep vec_steps[IQLHIP_VEC_MAX_UPDATES];
  size_t vec_head = 0, vec_end[IQLHIP_VEC_MAX_UPDATES] = {};
  // pinned, host-mapped staging per member: the new rows [k][IQLHIP_VEC_MAX_ENVS][ld], the drawn indices
  // [k][IQLHIP_VEC_MAX_UPDATES * 512], the steps' losses [k][IQLHIP_VEC_MAX_UPDATES][4] and the act: states in
  // [k][IQLHIP_VEC_MAX_ENVS][IQLHIP_MAX_INPUT], then actions out [k][IQLHIP_VEC_MAX_ENVS][IQLHIP_MAX_ACTION]
  float* vec_rows_pin = nullptr;
  long long* vec_idx_pin = nullptr;
  float* vec_loss_pin = nullptr;
  float* vec_act_pin = nullptr;
  // ... and the gathered batches of every member's steps, device [k][updates][batch_rows[k]][ld]: an owner of its own,
  // because the block is freed and allocated anew when a call needs more (vec_xb_cap floats)
  Owned vec_own;
  float* vec_xb = nullptr;
  size_t vec_xb_cap = 0;
};

static int group_check_members(iqlhip_ctx* const* members, int k, int flags) {
  if (!members) return fail(IQLHIP_EINVAL, "members is NULL");
  if (k < 1 || k > IQLHIP_MAX_GROUP) return fail(IQLHIP_EINVAL, "group size %d outside [1,%d]", k, IQLHIP_MAX_GROUP);
  for (int i = 0; i < k; ++i) {
    if (!members[i]) return fail(IQLHIP_EINVAL, "member %d is NULL", i);
    for (int j = 0; j < i; ++j)
      if (members[j] == members[i]) return fail(IQLHIP_EINVAL, "member %d is member %d again", i, j);
  }
  const iqlhip_ctx* a = members[0];
  for (int i = 0; i < k; ++i) {
    const iqlhip_ctx* c = members[i];
    if (c->device != a->device) return fail(IQLHIP_EINVAL, "member %d is on device %d, member 0 on %d", i, c->device, a->device);
    if (c->dims.state_dim != a->dims.state_dim || c->dims.action_dim != a->dims.action_dim || c->dims.policy != a->dims.policy)
      return fail(IQLHIP_EINVAL, "member %d has other dims or policy kind than member 0", i);
    if (c->precision != a->precision) return fail(IQLHIP_EINVAL, "member %d has another precision than member 0", i);
    if (c->xch_mode != IQLHIP_XCH_NONE || c->world > 1)
      return fail(IQLHIP_EUNSUPPORTED, "member %d has data parallelism enabled (not supported in a group)", i);
    if ((c->drop_p > 0.f || c->act_drop_p > 0.f) && !(flags & IQLHIP_GROUP_DROPOUT))
      return fail(IQLHIP_EUNSUPPORTED, "member %d uses actor dropout (not supported in a group)", i);
  }
  return IQLHIP_OK;
}

// The group kernels' selectors (with_bools).
static auto fwd_group_kernel(bool bf, bool dma, bool multi) {
  return with_bools([](auto MU, auto BF, auto DMA) { return &iql_fwd_group_kernel<BF.value, DMA.value, MU.value>; }, multi, bf, dma);
}
static auto bwd_group_kernel(bool bf, bool full) {
  return with_bools([](auto BF, auto FU) { return &iql_bwd_group_kernel<BF.value, FU.value>; }, bf, full);
}
static auto act_fwd_group_kernel(bool bf, bool dma) {
  return with_bools([](auto BF, auto DMA) { return &iql_act_fwd_group_kernel<BF.value, DMA.value>; }, bf, dma);
}

extern "C" int iqlhip_group_destroy(iqlhip_group* g) {
  if (!g) return fail(IQLHIP_EINVAL, "NULL group");
  DevGuard guard(g->device);
  (void)hipDeviceSynchronize();       // a group call may still be running on some stream
  g->vec_own.release_all();
  g->own.release_all();
  delete g;
  return IQLHIP_OK;
}

extern "C" int iqlhip_group_create_flags(iqlhip_ctx* const* members, int k, int32_t flags, iqlhip_group** out) {
  if (!out) return fail(IQLHIP_EINVAL, "out is NULL");
  if (flags & ~IQLHIP_GROUP_DROPOUT) return fail(IQLHIP_EINVAL, "unknown flags 0x%x", (unsigned)flags);
  int rc = group_check_members(members, k, flags);
  if (rc) return rc;
  iqlhip_group* g = new iqlhip_group();
  g->k = k;
  g->flags = flags;
  g->device = members[0]->device;
  for (int i = 0; i < k; ++i) g->m[i] = members[i];
  DevGuard guard(g->device);
  auto setup = [&]() -> int {
    const size_t n_drop = (flags & IQLHIP_GROUP_DROPOUT) ? k : 0;      // (without the flag: the layouts of a plain group)
    GroupStage& tr = g->train;
    tr.recs[0] = tr.stg.add<GroupRec>(k);
    tr.drops = tr.stg.add<GroupDropRec>(n_drop);
    tr.aux[0].add(tr.stg, k);
    g->wts = tr.stg.add<GroupWtRec>(k);
    tr.tabs = tr.stg.add<iqlhip_step_scalars>((size_t)k * IQLHIP_GROUP_MAX_STEPS);
    g->on_recs = g->on.add<GroupRec>(k);
    g->on_aps = g->on.add<StepParams>(k);
    g->on_gathers = g->on.add<GroupOnlineRec>(k);
    g->on_fins = g->on.add<GroupActRec>(k);
    g->on_drops = g->on.add<GroupDropRec>(n_drop);
    g->on_adrops = g->on.add<ActDropRec>(n_drop);
    g->on_tabs = g->on.add<iqlhip_step_scalars>(k);
    g->on_aux.add(g->on, k);
    g->act_packs = g->act.add<GroupPackRec>(k);
    g->act_ps = g->act.add<StepParams>(k);
    g->act_fins = g->act.add<GroupActRowsRec>(k);
    g->act_drops = g->act.add<ActDropRec>(n_drop);
    HIPCHK(tr.stg.alloc(g->own));
    HIPCHK(g->on.alloc(g->own, /*with_event=*/false));
    HIPCHK(g->act.alloc(g->own));
    const size_t ring = (size_t)k * IQLHIP_GROUP_MAX_STEPS * 4 * sizeof(float);
    HIPCHK(g->own.dev(&g->ring_dev, ring, 0));
    HIPCHK(g->own.pin(&g->ring_pin, ring));
    HIPCHK(g->own.pin(&g->done_pin, 8 * sizeof(unsigned long long), /*zero=*/true));
    const iqlhip_ctx* c = members[0];
    int rc_a = set_max_lds(3, c->lds_fwd_solo, [](unsigned m) { return fwd_group_kernel(m & 1, m & 2, m & 4); });
    if (!rc_a) rc_a = set_max_lds(2, c->lds_bwd, [](unsigned m) { return bwd_group_kernel(m & 1, m & 2); });
    if (!rc_a) rc_a = set_max_lds(2, c->lds_fwd_solo, [](unsigned m) { return act_fwd_group_kernel(m & 1, m & 2); });
    return rc_a;
  };
  rc = setup();
  if (rc) {
    const std::string msg = g_err;
    iqlhip_group_destroy(g);
    g_err = msg;
    return rc;
  }
  *out = g;
  return IQLHIP_OK;
}

extern "C" int iqlhip_group_create(iqlhip_ctx* const* members, int k, iqlhip_group** out) {
  return iqlhip_group_create_flags(members, k, 0, out);
}

// One row count per member: what the step entry points work on.  The uniform entry points pass one count k times.
struct GroupRows { int32_t v[IQLHIP_MAX_GROUP]; };
static GroupRows group_rows_all(int32_t rows) {
  GroupRows r;
  for (int i = 0; i < IQLHIP_MAX_GROUP; ++i) r.v[i] = rows;
  return r;
}

// Geometry of a group step.  Per member: its row tiles and chunks (its record carries them: a block beyond a member's
// own count exits).  Per launch: grid.x is the largest member's block count, grid.y the member.  The forward's slices
// per block are chosen for the whole group grid (the single-agent rule applied to the sum of the members' row tiles);
// the backward's (b) blocks take one slice each (iql_bwd_group_kernel).  Results do not depend on either (bit-identical
// for every slice count).  full: every member's rows fill whole chunks (the backward's FULL instantiation).
struct GroupGeom {
  int n_rt[IQLHIP_MAX_GROUP], n_chunk[IQLHIP_MAX_GROUP];
  int max_rows, fwd_l2, fwd_nb, fwd_work, bwd_nb, upd_nb;      // fwd_work: the forward blocks that have a row tile
  bool full;
};
static GroupGeom group_geom(const iqlhip_group* g, const int32_t* rows) {
  const iqlhip_ctx* c = g->m[0];
  GroupGeom q;
  memset(&q, 0, sizeof q);
  int rt_sum = 0;
  q.full = true;
  for (int i = 0; i < g->k; ++i) {
    q.n_rt[i] = (rows[i] + RT_ROWS - 1) / RT_ROWS;
    q.n_chunk[i] = (rows[i] + CHUNK_ROWS - 1) / CHUNK_ROWS;
    q.max_rows = std::max(q.max_rows, (int)rows[i]);
    q.full = q.full && (rows[i] % CHUNK_ROWS) == 0;
    rt_sum += q.n_rt[i];
  }
  q.fwd_l2 = fwd_spb_l2(c, rt_sum);
  for (int i = 0; i < g->k; ++i) {
    const int nb = fwd_blocks(q.n_rt[i], q.fwd_l2);
    q.fwd_nb = std::max(q.fwd_nb, nb);
    q.fwd_work += nb;
    q.bwd_nb = std::max(q.bwd_nb, bwd_blocks(q.n_chunk[i], q.n_rt[i], 0, 0));
  }
  q.upd_nb = upd_blocks(c);
  return q;
}

// Per-member checks the entry points share (before any device work): bound arenas ...
static int group_check_bound(const iqlhip_group* g, int i) {
  return g->m[i]->params ? IQLHIP_OK : fail(IQLHIP_ENOTBOUND, "member %d: iqlhip_bind has not been called", i);
}
// ... and, for the step entry points, a batch of rows[i] rows for member i.
static int group_check_call(iqlhip_group* g, const int32_t* rows) {
  if (!g) return fail(IQLHIP_EINVAL, "NULL group");
  int rc = group_check_members(g->m, g->k, g->flags);
  if (rc) return rc;
  for (int i = 0; i < g->k; ++i) {
    if ((rc = group_check_bound(g, i))) return rc;
    if (rows[i] < 1 || rows[i] > g->m[i]->dims.max_batch)
      return fail(IQLHIP_EINVAL, "member %d: batch rows %d outside [1, max_batch=%d]", i, rows[i], g->m[i]->dims.max_batch);
  }
  for (int i = 0; i < g->k; ++i)
    if (g->m[0]->precision == 1 && rows[i] > LB_MIN_ROWS)
      return fail(IQLHIP_EUNSUPPORTED, "bf16 groups take batches of at most %d rows (the large-batch kernels have no group form)", LB_MIN_ROWS);
  for (int i = 0; i < g->k; ++i)
    if ((rc = optional_features_check(g->m[i], rows[i]))) return rc;
  return IQLHIP_OK;
}

// Write agent i's record r (host side) for a call of n steps on batches of `rows` rows staged at xb; sched: the
// device address of the agent's scalar table.  The leading-argument words are the solo launchers' (bwd_words, upd_words).
static void group_record(iqlhip_group* g, GroupRec& r, int i, const GroupGeom& q, int rows, int n, const float* xb,
                         const iqlhip_step_scalars* sc0, const iqlhip_step_scalars* sched) {
  iqlhip_ctx* c = g->m[i];
  memset(&r, 0, sizeof r);
  r.p = make_step(c, rows, sc0->inv_batch);
  r.p.xb = xb;
  r.p.spb_l2 = q.fwd_l2;
  const BwdWords b = bwd_words(c, r.p, q.n_chunk[i], q.n_rt[i], 0u);      // (one-slice backward: no slice or donation word)
  r.q_heads = b.heads; r.q_xb = b.xb; r.q_h1 = b.h1; r.q_h0 = b.h0; r.q_params = b.params;
  r.q_dims = b.dims; r.q_ldB = b.ldB; r.q_mbc = b.mbc; r.q_rts = b.rts;
  r.u = make_upd(c, sc0, rows, nullptr);
  r.u.sched = sched;
  r.u.sched_idx = 0;
  r.u.loss_ring = g->ring_dev + (size_t)i * IQLHIP_GROUP_MAX_STEPS * 4;
  r.u.ring_slot = 0;
  const UpdWords w = upd_words(c, r.u);
  r.u_p = r.u.params; r.u_m = r.u.m; r.u_v = r.u.v; r.u_slab_a = r.u.slab_a;
  r.u_s0 = w.s0; r.u_s1 = w.s1; r.u_s2 = w.s2; r.u_s3 = w.s3; r.u_end = w.end; r.u_flags = w.flags;
  r.n_steps = n;
  r.xb = (float*)xb;
  r.B = rows;
}

// Actor dropout (IQLHIP_GROUP_DROPOUT): does member c draw keep-bits in a group call?  (a rate of 0 reads none;
// injected masks stay as they were written)
static bool group_draws(const iqlhip_ctx* c) { return c->drop_p > 0.f && !c->drop_inject; }

// A drawing member's record (host side) for a call on batches of `rows` rows (<= max_batch: group_check_call) that
// starts at the member's current stream position.  (GroupRec::p already carries drop_bits — parity 0 — and drop_scale
// of a member with a rate: make_step.)
static GroupDropRec group_drop_record(const iqlhip_ctx* c, int rows) {
  GroupDropRec d;
  memset(&d, 0, sizeof d);
  d.bits = c->drop_bits;
  d.n_rows = rows;
  d.max_batch = c->dims.max_batch;
  d.thresh = drop_thresh(c->drop_p);
  d.active = 1;
  d.seed = c->drop_seed;
  d.step0 = c->drop_step;
  return d;
}

// One-step calls (iqlhip_group_step, iqlhip_group_online_step): the drawing members' records packed at the front of
// `d` (iql_dropmask_group_kernel's grid.y).  Returns their number.
static int group_drop_records_packed(const iqlhip_group* g, GroupDropRec* d, const int32_t* rows) {
  int n = 0;
  if (!(g->flags & IQLHIP_GROUP_DROPOUT)) return 0;
  for (int i = 0; i < g->k; ++i)
    if (group_draws(g->m[i])) d[n++] = group_drop_record(g->m[i], rows[i]);
  return n;
}

// ... their draw at drop_step (one launch for all of them, where the solo steps launch iql_dropmask_kernel each), and
// drop_step += 1 as the solo step's.  `drops`: the device copy of the packed records; max_rows: the largest member's
// rows (each record bounds its own member's words).
static void group_launch_dropmask(iqlhip_group* g, const GroupDropRec* drops, int n_draw, int max_rows, hipStream_t st) {
  if (n_draw == 0) return;
  hipLaunchKernelGGL(iql_dropmask_group_kernel, dim3((2 * max_rows * 8 + 255) / 256, n_draw), dim3(256), 0, st, drops);
  for (int i = 0; i < g->k; ++i)
    if (group_draws(g->m[i])) g->m[i]->drop_step += 1;
}

// The device copies of a call's per-member statistics / clip records; nullptr: no member has the feature on.
struct GroupAux { const GroupStatsRec* srecs = nullptr; const GroupClipRec* crecs = nullptr; const GroupStatsRec* gqrecs = nullptr; };
// Build them in staging `s` at sections `x` from the members' step records (host side) and point `aux` at their device
// copies.  Statistics: enabled = the member has them on, its rows going to (member, step) of the group's statistics
// ring; stats_mask remembers who.  Clipping: a member with it off reads the group's 1.0f coefficients; the
// block-partial launch's records are enabled for a member with either feature.  A feature no member has on leaves its
// records alone (nothing of it is launched).
static int group_aux(iqlhip_group* g, const Staging& s, const AuxSections& x, const GroupRec* recs_host, GroupAux* aux) {
  bool stats = false, clip = false;
  for (int i = 0; i < g->k; ++i) { stats = stats || g->m[i]->stats_on; clip = clip || g->m[i]->clip_on; }
  if (stats && !g->stats_ring_dev) {
    const int rc = all_or_nothing(g->own, [&]() -> int {
      const size_t ring = (size_t)g->k * IQLHIP_GROUP_MAX_STEPS * IQLHIP_N_STATS * sizeof(float);
      HIPCHK(g->own.dev(&g->stats_ring_dev, ring, 0));
      HIPCHK(g->own.pin(&g->stats_ring_pin, ring));
      return IQLHIP_OK;
    });
    if (rc) return rc;
  }
  if (clip && !g->clip_ones) {
    const int rc = all_or_nothing(g->own, [&]() -> int {
      const float ones[4] = {1.f, 1.f, 1.f, 1.f};
      HIPCHK(g->own.dev(&g->clip_ones, sizeof ones));
      HIPCHK(hipMemcpy(g->clip_ones, ones, sizeof ones, hipMemcpyHostToDevice));
      return IQLHIP_OK;
    });
    if (rc) return rc;
  }
  GroupStatsRec* sr = s.host(x.srecs);
  GroupClipRec* cr = s.host(x.crecs);
  GroupStatsRec* gq = s.host(x.gqrecs);
  for (int i = 0; i < g->k; ++i) {
    const iqlhip_ctx* c = g->m[i];
    memset(&sr[i], 0, sizeof sr[i]);
    g->stats_mask[i] = c->stats_on;
    if (c->stats_on) {
      sr[i].a = make_stats(c, recs_host[i].p, g->stats_ring_dev + (size_t)i * IQLHIP_GROUP_MAX_STEPS * IQLHIP_N_STATS, 0,
                           IQLHIP_GROUP_MAX_STEPS, nullptr);
      sr[i].enabled = 1;
    }
    if (!clip) continue;
    memset(&cr[i], 0, sizeof cr[i]);
    memset(&gq[i], 0, sizeof gq[i]);
    cr[i].coef_rd = g->clip_ones;
    if (c->clip_on) {
      cr[i].a = make_clip(c);
      cr[i].coef_rd = cr[i].a.coef;
      cr[i].enabled = 1;
    }
    if (c->clip_on || c->stats_on) {
      gq[i].a.gparts = c->stats_part; gq[i].a.n_part = c->stats_n_part;
      gq[i].enabled = 1;
    }
  }
  *aux = GroupAux();
  if (stats) aux->srecs = s.device(x.srecs);
  if (clip) { aux->crecs = s.device(x.crecs); aux->gqrecs = s.device(x.gqrecs); }
  return IQLHIP_OK;
}
// rws != nullptr: the row-weighted backward under those records (end of file: its instantiations are the library's last).
static void launch_bwd_group_rw(const iqlhip_ctx* c, const GroupRec* recs, const GroupRwRec* rws, const GroupGeom& q, int K,
                                hipStream_t st);
static void group_launch_step(iqlhip_group* g, const GroupRec* recs, const GroupGeom& q, int s, hipStream_t st,
                              const GroupAux& aux, const GroupRwRec* rws = nullptr) {
  const GroupStatsRec* srecs = aux.srecs;
  const iqlhip_ctx* c = g->m[0];
  const int K = g->k;
  const bool bf = c->precision == 1, dma = c->w0_lds_k > W0_LDS_MAX_K;
  hipLaunchKernelGGL(fwd_group_kernel(bf, dma, /*multi=*/q.fwd_l2 > 0), dim3(q.fwd_nb, K), dim3(256), fwd_lds(c, q.fwd_work), st, recs);
  if (rws) launch_bwd_group_rw(c, recs, rws, q, K, st);
  else hipLaunchKernelGGL(bwd_group_kernel(bf, q.full), dim3(q.bwd_nb, K), dim3(256), c->lds_bwd, st, recs);
  // (between the backward and the update, as in a solo step: enqueue_step; the block partials once for both consumers)
  if (srecs || aux.crecs)
    hipLaunchKernelGGL(iql_stats_gradsq_group_kernel, dim3(4 * stats_parts(c), K), dim3(256), 0, st, recs,
                       aux.crecs ? aux.gqrecs : srecs, s);
  if (srecs) hipLaunchKernelGGL(iql_step_stats_group_kernel, dim3(1, K), dim3(256), 0, st, recs, srecs, s);
  if (aux.crecs) {
    hipLaunchKernelGGL(iql_clip_coef_group_kernel, dim3(1, K), dim3(256), 0, st, aux.crecs);
    hipLaunchKernelGGL(iql_update_clip_group_kernel, dim3(q.upd_nb, K), dim3(256), 0, st, recs, aux.crecs, s);
  } else {
    hipLaunchKernelGGL(iql_update_group_kernel, dim3(q.upd_nb, K), dim3(256), 0, st, recs, s);
  }
}

// The policy forward of n_req requesting members (both act paths): record j of `ps` on grid.y = j, `lds` from fwd_lds.
static void group_launch_act_fwd(const iqlhip_ctx* c0, const StepParams* ps, int nbx, int n_req, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL(act_fwd_group_kernel(c0->precision == 1, c0->w0_lds_k > W0_LDS_MAX_K), dim3(nbx, n_req), dim3(256), lds, st, ps);
}

static int group_losses_out(iqlhip_group* g, float* out, int n, hipStream_t st) {
  if (!out) return IQLHIP_OK;
  const size_t row = (size_t)IQLHIP_GROUP_MAX_STEPS * 4;
  for (int i = 0; i < g->k; ++i)
    if (int rc = read_back(nullptr, g->ring_pin + i * row, g->ring_dev + i * row, (size_t)n * 4 * sizeof(float), st, /*sync=*/false)) return rc;
  HIPCHK(hipStreamSynchronize(st));
  for (int i = 0; i < g->k; ++i)
    for (int s = 0; s < n; ++s)
      for (int j = 0; j < 3; ++j) out[((size_t)i * n + s) * 3 + j] = g->ring_pin[i * row + (size_t)s * 4 + j];
  return IQLHIP_OK;
}

// The row-weighted calls (defined with their entry points at the end of the file, where GroupRwRec / GroupPrioRec are
// complete): their staging (iqlhip_group::rw) and everything else they need beyond the members' own buffers, made by the
// group's first such call; the eager call's checks; and the step's row-weight records from the caller's arrays.
struct GroupRwArgs { const float* const* w; float* const* td; };
static int group_rw_ready(iqlhip_group* g);
static int group_rw_check_eager(const iqlhip_group* g, const int32_t* rows, const GroupRwArgs& a);
static const GroupRwRec* group_rw_records(iqlhip_group* g, const GroupRwArgs& a);

// iqlhip_group_step (mixed = false: every batch has batches[0]'s rows) and iqlhip_group_step_mixed.
// iqlhip_group_step_rw (rwa != nullptr; mixed): the same step from the row-weighted calls' staging, its backward the
// row-weighted one.  `stage`: the staging the step runs from (record set 0).
static int group_step(iqlhip_group* g, GroupStage iqlhip_group::* stage, const iqlhip_batch* batches, const iqlhip_step_scalars* sc,
                      float* out, void* stream, bool mixed, const GroupRwArgs* rwa = nullptr) {
  if (!g || !batches || !sc) return fail(IQLHIP_EINVAL, "NULL argument");
  GroupRows rows = group_rows_all(batches[0].rows);
  if (mixed)
    for (int i = 0; i < g->k && i < IQLHIP_MAX_GROUP; ++i) rows.v[i] = batches[i].rows;
  int rc = group_check_call(g, rows.v);
  if (rc) return rc;
  for (int i = 0; i < g->k; ++i) {
    rc = check_batch(g->m[i], &batches[i]);
    if (rc) return rc;
    if (!mixed && batches[i].rows != rows.v[0]) return fail(IQLHIP_EINVAL, "member %d: batch of %d rows, member 0: %d (one batch size per group)", i, batches[i].rows, rows.v[0]);
    if (batches[i].idx_dev && (rc = check_indexed(g->m[i], &batches[i]))) return rc;
  }
  if (rwa && (rc = group_rw_check_eager(g, rows.v, *rwa))) return rc;
  DevGuard guard(g->device);
  if (rwa && (rc = group_rw_ready(g))) return rc;
  for (int i = 0; i < g->k; ++i) note_stream(g->m[i], stream);
  hipStream_t st = (hipStream_t)stream;
  GroupStage& sg = g->*stage;
  Staging& stg = sg.stg;
  HIPCHK(stg.wait_free());
  const GroupGeom q = group_geom(g, rows.v);
  for (int i = 0; i < g->k; ++i) {
    iqlhip_ctx* c = g->m[i];
    c->cont.valid = false;
    const float* xb = nullptr;
    rc = stage_batch(c, &batches[i], st, &xb);
    if (rc) return rc;
    refresh_shadows(c, st);
    group_record(g, stg.host(sg.recs[0])[i], i, q, rows.v[i], 1, xb, &sc[i], sg.sched(i));
    sg.tab(i)[0] = sc[i];
  }
  const int n_draw = group_drop_records_packed(g, stg.host(sg.drops), rows.v);
  GroupAux aux;
  if ((rc = group_aux(g, stg, sg.aux[0], stg.host(sg.recs[0]), &aux))) return rc;
  const GroupRwRec* rws = rwa ? group_rw_records(g, *rwa) : nullptr;
  HIPCHK(sg.upload_steps(g->k, 1, st));
  group_launch_dropmask(g, stg.device(sg.drops), n_draw, q.max_rows, st);
  group_launch_step(g, stg.device(sg.recs[0]), q, 0, st, aux, rws);
  HIPCHK(hipGetLastError());
  g->last_n = 1;
  return group_losses_out(g, out, 1, st);
}
extern "C" int iqlhip_group_step(iqlhip_group* g, const iqlhip_batch* batches, const iqlhip_step_scalars* sc, float* out,
                                 void* stream) {
  return group_step(g, &iqlhip_group::train, batches, sc, out, stream, /*mixed=*/false);
}
extern "C" int iqlhip_group_step_mixed(iqlhip_group* g, const iqlhip_batch* batches, const iqlhip_step_scalars* sc,
                                       float* out, void* stream) {
  return group_step(g, &iqlhip_group::train, batches, sc, out, stream, /*mixed=*/true);
}

// The second source of a two-source group call, per member (the group form of a Mixed ChunkSrc): iqlhip_group_train_steps_replay2
// draws batch rows >= n_off[i] over [0, size[i]) from rows[i] — the online buffers; iqlhip_group_online_step_replay2
// reads batch rows < n_off[i] from rows[i] — the offline buffers of size[i] rows.
struct GroupMixSrc { const float* const* rows; const int64_t* size; const int32_t* n_off; };
// What both two-source group calls check per member (before any device work): the other buffer's rows, its size, and a
// split that leaves both parts of a batch of B rows non-empty.
static int group_check_mix(const GroupMixSrc* mx, int i, int32_t B, const char* what) {
  if (!mx->rows[i]) return fail(IQLHIP_EINVAL, "member %d: NULL %s buffer", i, what);
  if (((uintptr_t)mx->rows[i]) & 15) return fail(IQLHIP_EINVAL, "member %d: packed rows must be 16-byte aligned", i);
  if (mx->size[i] < 1) return fail(IQLHIP_EINVAL, "member %d: empty %s buffer", i, what);
  if (mx->n_off[i] < 1 || mx->n_off[i] >= B)
    return fail(IQLHIP_EINVAL, "member %d: n_off %d outside [1, batch_rows - 1 = %d]", i, mx->n_off[i], B - 1);
  return IQLHIP_OK;
}

// Weighted draws in a group call (iqlhip_group_train_steps_weighted): member i's table, wtabs[i] — NULL: it draws
// uniformly.  (iqlhip_weights is defined with the weighted-sampling code at the end of the file.)
static WTab weights_tab(const iqlhip_weights* t);
static int weights_check_member(const iqlhip_weights* t, int member, int64_t size, int device);
// Rows a wave of the weighted group gather resolves and copies per pass of its grid (gather_rows_drawn_weighted keeps
// two descents in flight per wave): 2 = a wave per two rows of the largest member, 1 = a wave per row.
#ifndef IQL_GROUP_WT_ROWS_PER_WAVE
#define IQL_GROUP_WT_ROWS_PER_WAVE 2
#endif

// iqlhip_group_train_steps (B: one count k times) and iqlhip_group_train_steps_mixed: member i draws B[i] rows a step.
// iqlhip_group_train_steps_replay2 (mx != nullptr): rows / size are the offline buffers, mx the online ones.
// iqlhip_group_train_steps_weighted (wtabs != nullptr; never together with mx): member i's rows are drawn by wtabs[i].
static int group_train_steps(iqlhip_group* g, const float* const* rows, int64_t ld, const int64_t* size, const int32_t* B,
                             const void* const* tables, int32_t n, const uint64_t* seeds, const uint64_t* offsets,
                             void* stream, const GroupMixSrc* mx = nullptr, const iqlhip_weights* const* wtabs = nullptr) {
  if (!g || !rows || !size || !B || !tables || !seeds || !offsets) return fail(IQLHIP_EINVAL, "NULL argument");
  if (mx && wtabs) return fail(IQLHIP_EUNSUPPORTED, "weighted draws from two buffers are not supported");
  int rc = group_check_call(g, B);
  if (rc) return rc;
  if (n < 1 || n > IQLHIP_GROUP_MAX_STEPS) return fail(IQLHIP_EINVAL, "n_steps outside [1,%d]", IQLHIP_GROUP_MAX_STEPS);
  for (int i = 0; i < g->k; ++i) {
    rc = check_train_args(g->m[i], rows[i], ld, B[i]);
    if (rc) return rc;
    if (size[i] < 1) return fail(IQLHIP_EINVAL, "member %d: empty buffer", i);
    if (!tables[i]) return fail(IQLHIP_EINVAL, "member %d: NULL scalar table", i);
    if (wtabs && wtabs[i] && (rc = weights_check_member(wtabs[i], i, size[i], g->device))) return rc;
    if (!mx) continue;
    if ((rc = group_check_mix(mx, i, B[i], "online"))) return rc;
    if (mx->rows[i] == rows[i]) return fail(IQLHIP_EINVAL, "member %d: the offline and the online buffer are the same rows", i);
  }
  for (int i = 0; i < g->k; ++i) note_stream(g->m[i], stream);
  DevGuard guard(g->device);
  hipStream_t st = (hipStream_t)stream;
  GroupStage& sg = g->train;
  Staging& stg = sg.stg;
  HIPCHK(stg.wait_free());
  const GroupGeom q = group_geom(g, B);
  for (int i = 0; i < g->k; ++i) {
    iqlhip_ctx* c = g->m[i];
    c->cont.valid = false;             // the staging buffer is overwritten: a later solo call must gather its own rows
    refresh_shadows(c, st);
    const iqlhip_step_scalars* tab = (const iqlhip_step_scalars*)tables[i];
    GroupRec& r = stg.host(sg.recs[0])[i];
    group_record(g, r, i, q, B[i], n, c->xb, &tab[0], sg.sched(i));
    r.rows = rows[i]; r.ld = ld; r.size = size[i]; r.seed = seeds[i]; r.offset = offsets[i];
    if (mx) { r.rows_on = mx->rows[i]; r.size_on = mx->size[i]; r.n_off = mx->n_off[i]; }
    memcpy(sg.tab(i), tab, (size_t)n * sizeof(iqlhip_step_scalars));
    if (wtabs) stg.host(g->wts)[i].wt = wtabs[i] ? weights_tab(wtabs[i]) : WTab{nullptr, 0u, 0};
  }
  // actor dropout: one record per member (indexed like the GroupRecs; active = the member draws), step s at drop_step + s
  bool draws = false;
  if (g->flags & IQLHIP_GROUP_DROPOUT) {
    GroupDropRec* d = stg.host(sg.drops);
    for (int i = 0; i < g->k; ++i) {
      d[i] = group_drop_record(g->m[i], B[i]);
      d[i].active = group_draws(g->m[i]) ? 1 : 0;
      draws = draws || d[i].active;
    }
  }
  GroupAux aux;
  if ((rc = group_aux(g, stg, sg.aux[0], stg.host(sg.recs[0]), &aux))) return rc;
  HIPCHK(sg.upload_steps(g->k, n, st));
  const iqlhip_ctx* c0 = g->m[0];
  // (grids sized by the largest member: every record bounds its own member's rows and words)
  const int gather_nb = (int)std::min<int64_t>(((int64_t)q.max_rows * (c0->row_ld / 4) + 255) / 256, 1024);
  // (a grid with a thread per gathered float4 and per keep-bit word: the words come from its far end)
  const int drop_nb = gather_nb + (2 * q.max_rows * 8 + 255) / 256;
  const GroupRec* recs = stg.device(sg.recs[0]);
  // weighted: a wave resolves an index and copies that row — a wave per IQL_GROUP_WT_ROWS_PER_WAVE rows of the largest
  // member, four waves a block; with keep-bits, their words fit behind the gather at the far end as above
  const int wt_nb = (q.max_rows + 4 * IQL_GROUP_WT_ROWS_PER_WAVE - 1) / (4 * IQL_GROUP_WT_ROWS_PER_WAVE);
  const int wt_drop_nb = wt_nb + (2 * q.max_rows * 8 + 255) / 256;
  const GroupWtRec* wts = stg.device(g->wts);
  for (int s = 0; s < n; ++s) {
    if (wtabs && draws)
      hipLaunchKernelGGL(iql_gather_weighted_drop_group_kernel, dim3(wt_drop_nb, g->k), dim3(256), 0, st, recs, wts,
                         stg.device(sg.drops), s);
    else if (wtabs)
      hipLaunchKernelGGL(iql_gather_weighted_group_kernel, dim3(wt_nb, g->k), dim3(256), 0, st, recs, wts, s);
    else if (draws)
      hipLaunchKernelGGL(mx ? iql_gather2_drop_group_kernel : iql_gather_drop_group_kernel, dim3(drop_nb, g->k), dim3(256), 0,
                         st, recs, stg.device(sg.drops), s);
    else
      hipLaunchKernelGGL(mx ? iql_gather2_group_kernel : iql_gather_group_kernel, dim3(gather_nb, g->k), dim3(256), 0, st,
                         recs, s);
    group_launch_step(g, recs, q, s, st, aux);
  }
  if (g->flags & IQLHIP_GROUP_DROPOUT)      // (as iqlhip_train_steps: the position of every context with a rate above 0)
    for (int i = 0; i < g->k; ++i) if (g->m[i]->drop_p > 0.f) g->m[i]->drop_step += (unsigned long long)n;
  HIPCHK(hipGetLastError());
  g->last_n = n;
  return IQLHIP_OK;
}
extern "C" int iqlhip_group_train_steps(iqlhip_group* g, const float* const* rows, int64_t ld, const int64_t* size,
                                        int32_t B, const void* const* tables, int32_t n, const uint64_t* seeds,
                                        const uint64_t* offsets, int32_t flags, void* stream) {
  (void)flags;
  const GroupRows b = group_rows_all(B);
  return group_train_steps(g, rows, ld, size, b.v, tables, n, seeds, offsets, stream);
}
extern "C" int iqlhip_group_train_steps_mixed(iqlhip_group* g, const float* const* rows, int64_t ld, const int64_t* size,
                                              const int32_t* B, const void* const* tables, int32_t n, const uint64_t* seeds,
                                              const uint64_t* offsets, int32_t flags, void* stream) {
  (void)flags;
  return group_train_steps(g, rows, ld, size, B, tables, n, seeds, offsets, stream);
}
extern "C" int iqlhip_group_train_steps_replay2(iqlhip_group* g, const float* const* rows_off, const int64_t* size_off,
                                                const float* const* rows_on, const int64_t* size_on, int64_t ld,
                                                const int32_t* B, const int32_t* n_off, const void* const* tables, int32_t n,
                                                const uint64_t* seeds, const uint64_t* offsets, void* stream) {
  if (!rows_on || !size_on || !n_off) return fail(IQLHIP_EINVAL, "NULL argument");
  const GroupMixSrc mx{rows_on, size_on, n_off};
  return group_train_steps(g, rows_off, ld, size_off, B, tables, n, seeds, offsets, stream, &mx);
}
extern "C" int iqlhip_group_train_steps_weighted(iqlhip_group* g, const float* const* rows, int64_t ld, const int64_t* size,
                                                 const int32_t* B, const void* const* tables, int32_t n,
                                                 const uint64_t* seeds, const uint64_t* offsets, int32_t flags, void* stream,
                                                 const iqlhip_weights* const* wtabs) {
  (void)flags;
  if (!wtabs) return fail(IQLHIP_EINVAL, "NULL argument");
  return group_train_steps(g, rows, ld, size, B, tables, n, seeds, offsets, stream, nullptr, wtabs);
}

extern "C" int iqlhip_group_read_losses(iqlhip_group* g, float* out, int32_t n, void* stream) {
  if (!g || !out) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n < 1 || n > g->last_n) return fail(IQLHIP_EINVAL, "n_steps %d outside [1,%d] (steps of the last group call)", n, g->last_n);
  DevGuard guard(g->device);
  return group_losses_out(g, out, n, (hipStream_t)stream);
}

extern "C" int iqlhip_group_read_step_stats(iqlhip_group* g, float* out, int32_t n, void* stream) {
  if (!g || !out) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n < 1 || n > g->last_n) return fail(IQLHIP_EINVAL, "n_steps %d outside [1,%d] (steps of the last group call)", n, g->last_n);
  DevGuard guard(g->device);
  hipStream_t st = (hipStream_t)stream;
  const size_t row = (size_t)IQLHIP_GROUP_MAX_STEPS * IQLHIP_N_STATS;
  for (int i = 0; i < g->k; ++i)
    if (g->stats_mask[i])
      if (int rc = read_back(nullptr, g->stats_ring_pin + i * row, g->stats_ring_dev + i * row,
                             (size_t)n * IQLHIP_N_STATS * sizeof(float), st, /*sync=*/false)) return rc;
  HIPCHK(hipStreamSynchronize(st));
  for (int s = 0; s < n; ++s)
    for (int i = 0; i < g->k; ++i)
      for (int j = 0; j < IQLHIP_N_STATS; ++j)
        out[((size_t)s * g->k + i) * IQLHIP_N_STATS + j] =
            g->stats_mask[i] ? g->stats_ring_pin[i * row + (size_t)s * IQLHIP_N_STATS + j] : __builtin_nanf("");
  return IQLHIP_OK;
}

// One online iteration of every member (iqlhip_online_step for each, include/iqlhip.h) in one set of launches: ring
// writes + gathers (+ the act states' packing), forward, backward, update with each member's losses landing in its own
// pinned words, then — members that asked for one — the next action with the updated policy, and one completion word
// the host spins on.  Everything is checked before any device work and before any counter moves.
// iqlhip_group_online_step (n: one count k times) and iqlhip_group_online_step_mixed: member i steps on n[i] rows, its
// indices at idx_host[n[0] + ... + n[i - 1]].  iqlhip_group_online_step_replay2 (mx != nullptr): the first mx->n_off[i] of
// member i's n[i] indices address its offline buffer mx->rows[i], the others its ring.
static int group_online_step(iqlhip_group* g, float* const* rows_dev, int64_t ld, const int64_t* capacity,
                             const int64_t* pointer, const float* row_host, const int64_t* idx_host, const int32_t* n,
                             const iqlhip_step_scalars* sc, float* out, const float* act_state_host,
                             const int32_t* act_mask, const float* max_action, const uint64_t* act_seed,
                             float* act_out_host, void* stream, const GroupMixSrc* mx = nullptr) {
  if (!g || !rows_dev || !capacity || !pointer || !row_host || !idx_host || !n || !sc || !out) return fail(IQLHIP_EINVAL, "NULL argument");
  if (act_state_host && (!max_action || !act_seed || !act_out_host))
    return fail(IQLHIP_EINVAL, "act_state_host without max_action, act_seed or act_out_host");
  int rc = group_check_call(g, n);
  if (rc) return rc;
  const int K = g->k;
  size_t idx0[IQLHIP_MAX_GROUP];      // where member i's indices start in idx_host
  for (int i = 0; i < K; ++i) idx0[i] = i ? idx0[i - 1] + (size_t)n[i - 1] : 0;
  for (int i = 0; i < K; ++i) {
    const iqlhip_ctx* c = g->m[i];
    if (ld != c->row_ld) return fail(IQLHIP_EINVAL, "row stride must be iqlhip_row_stride(S,A)=%lld", (long long)c->row_ld);
    if (!rows_dev[i]) return fail(IQLHIP_EINVAL, "member %d: NULL ring", i);
    if (((uintptr_t)rows_dev[i]) & 15) return fail(IQLHIP_EINVAL, "member %d: packed rows must be 16-byte aligned", i);
    if (capacity[i] < 1 || pointer[i] < 0 || pointer[i] >= capacity[i])
      return fail(IQLHIP_EINVAL, "member %d: ring pointer outside the buffer", i);
    for (int j = 0; j < i; ++j) {      // (two members writing one ring would race on its rows)
      const uintptr_t a0 = (uintptr_t)rows_dev[i], a1 = a0 + (uintptr_t)(capacity[i] * ld) * sizeof(float);
      const uintptr_t b0 = (uintptr_t)rows_dev[j], b1 = b0 + (uintptr_t)(capacity[j] * ld) * sizeof(float);
      if (a0 < b1 && b0 < a1) return fail(IQLHIP_EINVAL, "members %d and %d share ring rows (one buffer per member)", j, i);
    }
    const int n_off = mx ? mx->n_off[i] : 0;
    if (mx && (rc = group_check_mix(mx, i, n[i], "offline"))) return rc;
    if (n_off && (rc = check_host_indices(idx_host + idx0[i], n_off, mx->size[i]))) return rc;
    rc = check_host_indices(idx_host + idx0[i] + n_off, n[i] - n_off, capacity[i]);
    if (rc) return rc;
  }
  if (mx)      // (a ring is written by the launch that reads the offline rows: no member's ring may lie in an offline buffer)
    for (int i = 0; i < K; ++i)
      for (int j = 0; j < K; ++j) {
        const uintptr_t a0 = (uintptr_t)rows_dev[i], a1 = a0 + (uintptr_t)(capacity[i] * ld) * sizeof(float);
        const uintptr_t b0 = (uintptr_t)mx->rows[j], b1 = b0 + (uintptr_t)(mx->size[j] * ld) * sizeof(float);
        if (a0 < b1 && b0 < a1)
          return fail(IQLHIP_EINVAL, "member %d's ring overlaps member %d's offline buffer (the offline rows are read only)", i, j);
      }
  for (int i = 0; i < g->k; ++i) note_stream(g->m[i], stream);
  DevGuard guard(g->device);
  hipStream_t st = (hipStream_t)stream;
  const iqlhip_ctx* c0 = g->m[0];
  const int S = c0->dims.state_dim, A = c0->dims.action_dim;
  const bool gauss = c0->dims.policy == IQLHIP_POLICY_GAUSSIAN;
  const GroupGeom q = group_geom(g, n);
  const Staging& on = g->on;
  GroupRec* recs = on.host(g->on_recs);
  StepParams* aps = on.host(g->on_aps);
  GroupOnlineRec* ons = on.host(g->on_gathers);
  GroupActRec* fins = on.host(g->on_fins);
  iqlhip_step_scalars* tab = on.host(g->on_tabs);
  auto act_requested = [&](int i) { return act_state_host && (!act_mask || act_mask[i]); };
  // inference keep-bits of the requesting members whose act forward runs with dropout (one record per member)
  const bool with_adrops = (g->flags & IQLHIP_GROUP_DROPOUT) != 0;
  ActDropRec* adrops = with_adrops ? on.host(g->on_adrops) : nullptr;
  bool act_draws = false;
  int n_req = 0;
  for (int i = 0; i < K; ++i) {
    iqlhip_ctx* c = g->m[i];
    c->cont.valid = false;             // the staging buffer is overwritten: a later solo call must gather its own rows
    memcpy(c->on_row_pin, row_host + (size_t)i * ld, (size_t)ld * sizeof(float));
    memcpy(c->on_idx_pin, idx_host + idx0[i], (size_t)n[i] * sizeof(long long));
    tab[i] = sc[i];
    group_record(g, recs[i], i, q, n[i], 1, c->xb, &sc[i], on.device(g->on_tabs) + i);
    recs[i].u.losses_mirror = c->on_loss_pin;
    const bool req = act_requested(i);
    GroupOnlineRec& o = ons[i];
    o.rows = rows_dev[i]; o.row_pin = c->on_row_pin; o.idx_pin = c->on_idx_pin; o.xb = c->xb;
    o.act_pin = req ? c->on_act_pin : nullptr; o.xb_act = c->xb_act;
    o.ld = ld; o.pointer = pointer[i]; o.n = n[i]; o.S = S;
    o.rows_off = mx ? mx->rows[i] : nullptr; o.n_off = mx ? mx->n_off[i] : 0;
    if (with_adrops) adrops[i] = act_drop_record(c, req ? 1 : 0);
    if (!req) continue;
    memcpy(c->on_act_pin, act_state_host + (size_t)i * S, (size_t)S * sizeof(float));
    aps[n_req] = act_step_params(c, 1);
    if (with_adrops && adrops[i].active) { act_draws = true; c->act_drop_calls += 1; }
    GroupActRec& f = fins[n_req];
    const bool noise = act_seed[i] != 0 && gauss;      // (the call counter moves only when noise is drawn, as solo)
    f.heads = c->heads_act; f.log_std = aps[n_req].log_std; f.out = c->on_act_pin + IQLHIP_MAX_INPUT;
    f.max_action = max_action[i]; f.ls_min = c->hyper.log_std_min; f.ls_max = c->hyper.log_std_max;
    f.seed = noise ? act_seed[i] : 0ull;
    f.call = noise ? c->act_calls++ : 0ull;
    ++n_req;
  }
  const int n_draw = group_drop_records_packed(g, on.host(g->on_drops), n);
  GroupAux aux;
  if ((rc = group_aux(g, on, g->on_aux, recs, &aux))) return rc;
  // (a synchronous call: the previous one's upload has been read long ago)
  HIPCHK(g->on.upload(on.bytes, st));
  const int gather_nb = (int)((q.max_rows * (ld / 4) + 255) / 256);      // (the largest member's: a record bounds its own)
  if (act_draws)
    hipLaunchKernelGGL(mx ? iql_online_gather2_drop_group_kernel : iql_online_gather_drop_group_kernel, dim3(gather_nb, K),
                       dim3(256), 0, st, on.device(g->on_gathers), on.device(g->on_adrops));
  else
    hipLaunchKernelGGL(mx ? iql_online_gather2_group_kernel : iql_online_gather_group_kernel, dim3(gather_nb, K), dim3(256), 0,
                       st, on.device(g->on_gathers));
  for (int i = 0; i < K; ++i) refresh_shadows(g->m[i], st);
  group_launch_dropmask(g, on.device(g->on_drops), n_draw, q.max_rows, st);
  group_launch_step(g, on.device(g->on_recs), q, 0, st, aux);
  const unsigned long long done_val = ++g->done_seq;
  if (n_req > 0) {
    // (bf16: the update has just rewritten the shadows from the new masters — the conversion refresh_shadows makes)
    group_launch_act_fwd(c0, on.device(g->on_aps), NSPLIT, n_req, fwd_lds(c0, NSPLIT), st);
    hipLaunchKernelGGL(iql_actor_finish_group_kernel, dim3(1), dim3(256), 0, st, on.device(g->on_fins), n_req, A, g->done_pin,
                       done_val);
  } else {
    hipLaunchKernelGGL(iql_group_done_kernel, dim3(1), dim3(64), 0, st, g->done_pin, done_val);
  }
  HIPCHK(hipGetLastError());
  g->last_n = 1;
  rc = wait_word(g->done_pin, done_val, st);
  if (rc) return rc;
  for (int i = 0; i < K; ++i) {
    const iqlhip_ctx* c = g->m[i];
    for (int j = 0; j < 3; ++j) out[3 * i + j] = c->on_loss_pin[j];
    if (act_requested(i)) memcpy(act_out_host + (size_t)i * A, c->on_act_pin + IQLHIP_MAX_INPUT, (size_t)A * sizeof(float));
  }
  return IQLHIP_OK;
}
extern "C" int iqlhip_group_online_step(iqlhip_group* g, float* const* rows_dev, int64_t ld, const int64_t* capacity,
                                        const int64_t* pointer, const float* row_host, const int64_t* idx_host, int32_t n,
                                        const iqlhip_step_scalars* sc, float* out, const float* act_state_host,
                                        const int32_t* act_mask, const float* max_action, const uint64_t* act_seed,
                                        float* act_out_host, void* stream) {
  const GroupRows r = group_rows_all(n);
  return group_online_step(g, rows_dev, ld, capacity, pointer, row_host, idx_host, r.v, sc, out, act_state_host, act_mask,
                           max_action, act_seed, act_out_host, stream);
}
extern "C" int iqlhip_group_online_step_mixed(iqlhip_group* g, float* const* rows_dev, int64_t ld, const int64_t* capacity,
                                              const int64_t* pointer, const float* row_host, const int64_t* idx_host,
                                              const int32_t* n, const iqlhip_step_scalars* sc, float* out,
                                              const float* act_state_host, const int32_t* act_mask,
                                              const float* max_action, const uint64_t* act_seed, float* act_out_host,
                                              void* stream) {
  return group_online_step(g, rows_dev, ld, capacity, pointer, row_host, idx_host, n, sc, out, act_state_host, act_mask,
                           max_action, act_seed, act_out_host, stream);
}
extern "C" int iqlhip_group_online_step_replay2(iqlhip_group* g, float* const* rows_dev, int64_t ld, const int64_t* capacity,
                                                const int64_t* pointer, const float* row_host, const int64_t* idx_host,
                                                const int32_t* n, const iqlhip_step_scalars* sc, float* out,
                                                const float* act_state_host, const int32_t* act_mask,
                                                const float* max_action, const uint64_t* act_seed, float* act_out_host,
                                                void* stream, const float* const* rows_off_dev, const int64_t* size_off,
                                                const int32_t* n_off) {
  if (!rows_off_dev || !size_off || !n_off) return fail(IQLHIP_EINVAL, "NULL argument");
  const GroupMixSrc mx{rows_off_dev, size_off, n_off};
  return group_online_step(g, rows_dev, ld, capacity, pointer, row_host, idx_host, n, sc, out, act_state_host, act_mask,
                           max_action, act_seed, act_out_host, stream, &mx);
}

// Policy inference of every member (iqlhip_actor_forward / iqlhip_actor_sample for each, include/iqlhip.h) in one set
// of launches: the members' states packed into their xb_act, the policy forward (iql_act_fwd_group_kernel, grid.y =
// requesting member, grid.x = the longest member's row tiles x NSPLIT — a block past a shorter member's rows loads its
// last row again, clamped, and stores nothing: every store of the body is guarded by row < p.rows), and the finish over
// each member's rows.  Everything is checked before any device work and before any counter moves.
extern "C" int iqlhip_group_actor_forward(iqlhip_group* g, const float* const* states, int64_t ld_s, const int32_t* rows,
                                          const uint64_t* seeds, const float* max_action, float* const* actions,
                                          int64_t ld_a, int32_t flags, void* stream) {
  if (!g || !states || !rows || !seeds || !max_action || !actions) return fail(IQLHIP_EINVAL, "NULL argument");
  int rc = group_check_members(g->m, g->k, g->flags);
  if (rc) return rc;
  const int K = g->k;
  const iqlhip_ctx* c0 = g->m[0];
  const int S = c0->dims.state_dim, A = c0->dims.action_dim;
  for (int i = 0; i < K; ++i) {
    if ((rc = group_check_bound(g, i))) return rc;
    if (rows[i] < 0 || rows[i] > g->m[i]->act_cap)
      return fail(IQLHIP_EINVAL, "member %d: rows %d outside [0, %d]", i, rows[i], g->m[i]->act_cap);
    if (rows[i] > 0 && (!states[i] || !actions[i])) return fail(IQLHIP_EINVAL, "member %d: NULL states or actions", i);
  }
  if (ld_s < S || ld_a < A) return fail(IQLHIP_EINVAL, "row stride smaller than the row");
  if (flags & ~IQLHIP_GROUP_ACT_WAIT) return fail(IQLHIP_EINVAL, "unknown flags 0x%x", (unsigned)flags);
  int n_req = 0, max_rows = 0;
  for (int i = 0; i < K; ++i) {
    if (rows[i] > 0) ++n_req;
    max_rows = std::max(max_rows, (int)rows[i]);
  }
  if (n_req == 0) return IQLHIP_OK;
  DevGuard guard(g->device);
  hipStream_t st = (hipStream_t)stream;
  CachedStaging& act = g->act;
  // (records are written field by field into the build buffer, whose padding bytes stay zero, or copied whole from a
  //  record make_step has zeroed: upload_if_changed sees equal bytes for equal records)
  GroupPackRec* packs = act.build(g->act_packs);
  StepParams* ps = act.build(g->act_ps);
  GroupActRowsRec* fins = act.build(g->act_fins);
  const bool with_drops = (g->flags & IQLHIP_GROUP_DROPOUT) != 0;
  ActDropRec* drops = with_drops ? act.build(g->act_drops) : nullptr;
  bool act_draws = false;
  int j = 0;
  for (int i = 0; i < K; ++i) {
    if (rows[i] == 0) continue;        // (no launch, no counter: the solo caller makes no call for no rows)
    iqlhip_ctx* c = g->m[i];
    const int n = rows[i];
    GroupPackRec& pk = packs[j];
    pk.xb = c->xb_act; pk.s = states[i]; pk.ld_s = (long long)ld_s; pk.ld = (int)c->row_ld; pk.S = S; pk.n = n;
    ps[j] = act_step_params(c, n);
    if (with_drops) {
      drops[j] = act_drop_record(c, n);
      if (drops[j].active) { act_draws = true; c->act_drop_calls += 1; }
    }
    GroupActRowsRec& f = fins[j];
    f.heads = c->heads_act; f.log_std = ps[j].log_std; f.out = actions[i]; f.ld_out = (long long)ld_a; f.n = n; f.A = A;
    f.max_action = max_action[i]; f.ls_min = c->hyper.log_std_min; f.ls_max = c->hyper.log_std_max;
    f.seed = seeds[i];
    f.call = seeds[i] != 0 ? c->act_calls++ : 0ull;      // (iqlhip_actor_sample: one call number per call)
    ++j;
  }
  HIPCHK(act.upload_if_changed(act.bytes, st));
  const int pack_nb = (int)std::min<int64_t>(((int64_t)max_rows * c0->row_ld + 255) / 256, 1024);
  if (act_draws)           // (a grid with blocks for the longest member's keep-bit words at its far end)
    hipLaunchKernelGGL(iql_pack_states_drop_group_kernel, dim3(pack_nb + (2 * max_rows * 8 + 255) / 256, n_req), dim3(256), 0,
                       st, act.device(g->act_packs), act.device(g->act_drops));
  else
    hipLaunchKernelGGL(iql_pack_states_group_kernel, dim3(pack_nb, n_req), dim3(256), 0, st, act.device(g->act_packs));
  for (int i = 0; i < K; ++i)
    if (rows[i] > 0) refresh_shadows(g->m[i], st);
  const int nbx = (max_rows + RT_ROWS - 1) / RT_ROWS * NSPLIT;
  group_launch_act_fwd(c0, act.device(g->act_ps), nbx, n_req, fwd_lds(c0, nbx * n_req), st);
  hipLaunchKernelGGL(iql_actor_finish_rows_group_kernel, dim3((max_rows * A + 255) / 256, n_req), dim3(256), 0, st,
                     act.device(g->act_fins));
  if (!(flags & IQLHIP_GROUP_ACT_WAIT)) {
    HIPCHK(hipGetLastError());
    return IQLHIP_OK;
  }
  // synchronous: a completion word behind the finish (stream order: every action is stored by then), the host spins
  // on it instead of synchronising the stream
  const unsigned long long done_val = ++g->done_seq;
  hipLaunchKernelGGL(iql_group_done_kernel, dim3(1), dim3(64), 0, st, g->done_pin, done_val);
  HIPCHK(hipGetLastError());
  return wait_word(g->done_pin, done_val, st);
}

// ---------------------------------------------------------------------------
// Two-source multi-step calls (include/iqlhip.h "mixed offline / online batches"): iqlhip_train_steps with every batch's
// first n_off rows drawn from one buffer and the rest from another.  The driver above does the work (ChunkKind::Mixed); here are
// the forward instantiations of such chunks — selected and emitted behind every other kernel of the library, so the
// code object of the plain calls' kernels lies where it always has (with_bools) — and the entry points' checks.
// (The two kernels below are declared in iqlhip_kernels.h and defined here for the same reason.)
// First launch of an iqlhip_train_steps_mixed call: the same, with step 0's rows drawn from the two buffers (a mixed
// call always gathers them: B > 0; `rows` is the offline buffer).
__global__ __launch_bounds__(256) void iql_call_setup_mixed_kernel(unsigned long long* hdr, ChunkHdr h,
                                                                   iqlhip_step_scalars* sched_call,
                                                                   const iqlhip_step_scalars* sched_src, int n_steps,
                                                                   const float* rows, long long ld, float* xb, int B,
                                                                   unsigned* drop_dst, int drop_words, unsigned drop_thresh,
                                                                   unsigned* arrivals, unsigned long long* ack,
                                                                   unsigned long long ack_val, const float* rows_on,
                                                                   int n_off) {
  call_setup_head(hdr, h, sched_call, sched_src, n_steps, arrivals, ack, ack_val);
  gather_rows_drawn2(rows, rows_on, ld, xb, B, n_off, h.w[HDR_SEED], h.w[HDR_OFFSET], h.w[HDR_POS], h.w[HDR_SIZE],
                     h.w[HDR_SIZE_ON], (int)blockIdx.x * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
  if (drop_dst)
    dropmask_words(drop_dst, drop_words, drop_thresh, h.w[HDR_DROP_SEED], h.w[HDR_DROP_STEP],
                   ((int)gridDim.x - 1 - (int)blockIdx.x) * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
}

// The same for a batch mixed from two buffers (iqlhip_online_step_mixed): batch rows [0, n_off) are
// rows_off[idx_host[r]] (the offline buffer, read only), rows [n_off, n) come from the ring as above — idx_host holds the
// n_off offline indices followed by the n - n_off online ones, the order the host drew them in.  A row's float4 count
// does not divide 256, so a block may straddle n_off: its index cache holds indices of both kinds, and the row number
// decides which buffer an index belongs to (an offline index that happens to equal `pointer` is an ordinary row).
__global__ __launch_bounds__(256) void iql_online_gather2_kernel(float* rows, const float* rows_off, long long ld,
                                                                 long long pointer, const float* row_host,
                                                                 const long long* idx_host, float* xb, int n_off, int n) {
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
    const float* src = (r < n_off) ? rows_off + i * ld : ((i == pointer) ? row_host : rows + i * ld);
    *(f32x4*)(xb + (long long)r * ld + 4 * c4) = *(const f32x4*)(src + 4 * c4);
  }
}

static auto fwd_mixed_kernel(bool bf, bool dma, bool multi) {
  return with_bools([](auto MU, auto BF, auto DMA) { return &iql_fwd_mixed_kernel<BF.value, DMA.value, MU.value>; }, multi, bf, dma);
}
static int check_mixed_args(iqlhip_ctx* c, const float* rows_off_dev, const float* rows_on_dev, int64_t ld, int32_t B,
                            int32_t n_off) {
  int rc = check_train_args(c, rows_off_dev, ld, B);
  if (rc) return rc;
  if (!rows_on_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (((uintptr_t)rows_on_dev) & 15) return fail(IQLHIP_EINVAL, "packed rows must be 16-byte aligned");
  if (rows_on_dev == rows_off_dev) return fail(IQLHIP_EINVAL, "the offline and the online buffer are the same rows");
  if (n_off < 1 || n_off >= B) return fail(IQLHIP_EINVAL, "n_off %d outside [1, batch_rows - 1] (one buffer only: iqlhip_train_steps)", n_off);
  if (c->xch_mode != IQLHIP_XCH_NONE)
    return fail(IQLHIP_EUNSUPPORTED, "mixed batches are not supported with a data-parallel exchange");
  if (use_lb(c, B))
    return fail(IQLHIP_EUNSUPPORTED, "mixed batches are not supported on the large-batch bf16 path (more than %d rows)", LB_MIN_ROWS);
  return ensure_fwd_lds(c, ChunkKind::Mixed);
}
static ChunkCall mixed_call(const float* rows_on_dev, int32_t n_off) {
  ChunkCall call;
  call.src.kind = ChunkKind::Mixed; call.src.rows_on = rows_on_dev; call.src.n_off = n_off;
  return call;
}
extern "C" int iqlhip_train_steps_mixed_prepare(iqlhip_ctx* c, const float* rows_off_dev, const float* rows_on_dev, int64_t ld,
                                                int32_t B, int32_t n_off, float inv_batch, void* stream) {
  int rc = check_mixed_args(c, rows_off_dev, rows_on_dev, ld, B, n_off);
  if (rc) return rc;
  return train_steps_prepare(c, rows_off_dev, ld, B, inv_batch, stream, mixed_call(rows_on_dev, n_off));
}
extern "C" int iqlhip_train_steps_mixed(iqlhip_ctx* c, const float* rows_off_dev, int64_t size_off, const float* rows_on_dev,
                                        int64_t size_on, int64_t ld, int32_t B, int32_t n_off,
                                        const iqlhip_step_scalars* sc, int32_t K, uint64_t seed, uint64_t stream_offset,
                                        void* stream) {
  if (!sc) return fail(IQLHIP_EINVAL, "NULL argument");
  int rc = check_mixed_args(c, rows_off_dev, rows_on_dev, ld, B, n_off);
  if (rc) return rc;
  if (size_on < 1) return fail(IQLHIP_EINVAL, "empty online buffer");
  return train_steps(c, rows_off_dev, ld, size_off, B, sc, K, seed, stream_offset, 0, stream, mixed_call(rows_on_dev, n_off), size_on);
}

// ---------------------------------------------------------------------------
// The two-source gathers in group form (iqlhip_group_online_step_replay2 / iqlhip_group_train_steps_replay2; grid.y =
// member, the arguments in the member's record).  Everything behind them is the group launch sequence of the plain calls.
// iql_online_gather2_kernel per member, as online_gather_member is iql_online_gather_kernel per member: the ring write,
// the act state's packing, and the gather — batch rows [0, n_off) from the member's offline buffer, rows [n_off, n) from
// its ring, by the member's pinned indices (its n_off offline ones first).  A block's 256 float4 slots cover several rows
// and may straddle n_off: the index cache holds both kinds, and the ROW decides which buffer an index addresses — only an
// online index equal to `pointer` reads the pinned row.  The grid is sized for the largest n: a block past a member's own
// n reads no index and writes no row.
__device__ __forceinline__ void online_gather2_member(const GroupOnlineRec& g) {
  __shared__ long long s_idx[260];
  float* rows = g.rows;
  const float* row_host = g.row_pin;
  const long long ld = g.ld, pointer = g.pointer;
  const int n = g.n, n_off = g.n_off;
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
    const float* src = (r < n_off) ? g.rows_off + i * ld : ((i == pointer) ? row_host : rows + i * ld);
    *(f32x4*)(g.xb + (long long)r * ld + 4 * c4) = *(const f32x4*)(src + 4 * c4);
  }
}
__global__ __launch_bounds__(256) void iql_online_gather2_group_kernel(const GroupOnlineRec* __restrict__ recs) {
  online_gather2_member(recs[blockIdx.y]);
}
// ... plus the act forwards' keep-bits from the far end of the grid (iql_online_gather_drop_group_kernel's split).
__global__ __launch_bounds__(256) void iql_online_gather2_drop_group_kernel(const GroupOnlineRec* __restrict__ recs,
                                                                            const ActDropRec* __restrict__ drops) {
  online_gather2_member(recs[blockIdx.y]);
  const ActDropRec& d = drops[blockIdx.y];
  if (d.active)
    act_drop_words(d, ((int)gridDim.x - 1 - (int)blockIdx.x) * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
}

// iql_gather_group_kernel / iql_gather_drop_group_kernel with every member's step drawn from its two buffers: index
// j = s * B + r of the member's one stream, mapped over `size` into `rows` (offline) for r < n_off and over size_on into
// rows_on for the others — gather_rows_drawn2, the draw of iqlhip_train_steps_mixed.
__global__ __launch_bounds__(256) void iql_gather2_group_kernel(const GroupRec* __restrict__ recs, int step) {
  const GroupRec& r = recs[blockIdx.y];
  const int s = min(max(step, 0), r.n_steps - 1);
  gather_rows_drawn2(r.rows, r.rows_on, r.ld, r.xb, r.B, r.n_off, r.seed, r.offset,
                     (unsigned long long)s * (unsigned long long)r.B, (unsigned long long)r.size,
                     (unsigned long long)r.size_on, (int)blockIdx.x * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
}
__global__ __launch_bounds__(256) void iql_gather2_drop_group_kernel(const GroupRec* __restrict__ recs,
                                                                     const GroupDropRec* __restrict__ drops, int step) {
  const GroupRec& r = recs[blockIdx.y];
  const int s = min(max(step, 0), r.n_steps - 1);
  gather_rows_drawn2(r.rows, r.rows_on, r.ld, r.xb, r.B, r.n_off, r.seed, r.offset,
                     (unsigned long long)s * (unsigned long long)r.B, (unsigned long long)r.size,
                     (unsigned long long)r.size_on, (int)blockIdx.x * 256 + (int)threadIdx.x, (int)gridDim.x * 256);
  const GroupDropRec& d = drops[blockIdx.y];
  if (d.active)
    group_drop_words(d, d.step0 + (unsigned long long)s, ((int)gridDim.x - 1 - (int)blockIdx.x) * 256 + (int)threadIdx.x,
                     (int)gridDim.x * 256);
}

// ---------------------------------------------------------------------------
// Scoring transitions without a step (include/iqlhip.h "scoring transitions without a step"; kernels:
// iqlhip_score_kernels.h).  The host walks the call in chunks of rows: forward (head partials into the scoring
// scratch), row kernel (the eight columns, tile partials), finish kernel (running sums in double; the last chunk
// writes the summary into host-mapped words).
// (the kernels are included HERE, behind every other kernel of the file: the existing kernels keep their places in the
//  code object, which the step time is sensitive to — see with_bools above)
#include "iqlhip_score_kernels.h"
#define SCORE_CHUNK 65536
static size_t score_lds(const iqlhip_ctx* c) {
  const int A = c->dims.action_dim, kq = c->dims.state_dim + A;
  const size_t w0 = (kq <= W0_LDS_MAX_K) ? kq : ((c->dims.state_dim <= W0_LDS_MAX_K) ? c->dims.state_dim : 0);
  return (size_t)(RT_ROWS * H0_LD + RT_ROWS * T64_LD + RT_ROWS * SCORE_XLD_MAX + (((A + 15) & ~15) * W2_LD + 32) + HID +
                  (size_t)HID * w0) * sizeof(float);
}
static int ensure_score(iqlhip_ctx* c) {
  if (!c->score_heads) {
    const int rc = all_or_nothing(c->own, [&]() -> int {
      Owned& own = c->own;
      HIPCHK(own.dev(&c->score_heads, (size_t)SCORE_CHUNK * HEAD_LD * sizeof(float), 0));
      HIPCHK(own.dev(&c->score_pi, (size_t)SCORE_CHUNK * c->dims.action_dim * NSPLIT * sizeof(float), 0));
      HIPCHK(own.dev(&c->score_part, (size_t)(SCORE_CHUNK / RT_ROWS) * SCORE_N_PART * sizeof(float), 0));
      HIPCHK(own.dev(&c->score_acc, 16 * sizeof(double), 0));
      HIPCHK(own.pin(&c->score_pin, 16 * sizeof(float), /*zero=*/true));
      HIPCHK(own.pin(&c->score_status, 2 * sizeof(unsigned long long), /*zero=*/true));
      return IQLHIP_OK;
    });
    if (rc) return rc;
  }
  if (!c->score_lds_set) {
    HIPCHK(hipFuncSetAttribute((const void*)&iql_score_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)score_lds(c)));
    c->score_lds_set = true;
  }
  return IQLHIP_OK;
}

extern "C" int iqlhip_score_rows(iqlhip_ctx* c, const float* rows_dev, int64_t ld, int64_t n_rows, int64_t row0, int64_t n,
                                 const int64_t* idx_dev, float* out_dev, int32_t chunk_rows, float* summary, void* stream) {
  if (!c || !rows_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (!c->params) return fail(IQLHIP_ENOTBOUND, "iqlhip_bind has not been called");
  if (!out_dev && !summary) return fail(IQLHIP_EINVAL, "nothing to write: out_dev and summary are both NULL");
  if (n < 1) return fail(IQLHIP_EINVAL, "n = %lld rows to score", (long long)n);
  if (n_rows < 1) return fail(IQLHIP_EINVAL, "n_rows = %lld", (long long)n_rows);
  if (ld < c->row_ld || (ld & 3)) return fail(IQLHIP_EINVAL, "row stride %lld: need a multiple of 4 >= %lld", (long long)ld, (long long)c->row_ld);
  if ((((uintptr_t)rows_dev) | ((uintptr_t)out_dev)) & 15) return fail(IQLHIP_EINVAL, "rows and out must be 16-byte aligned");
  if (!idx_dev && (row0 < 0 || row0 > n_rows || n > n_rows - row0))
    return fail(IQLHIP_EINVAL, "rows [%lld, %lld) outside the buffer's [0, %lld)", (long long)row0, (long long)(row0 + n), (long long)n_rows);
  if (chunk_rows < 0 || (chunk_rows % RT_ROWS)) return fail(IQLHIP_EINVAL, "chunk_rows %d: need 0 or a positive multiple of %d", chunk_rows, RT_ROWS);
  const int64_t chunk = (chunk_rows == 0) ? SCORE_CHUNK : std::min<int64_t>(chunk_rows, SCORE_CHUNK);
  DevGuard guard(c->device);
  int rc = ensure_score(c);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (idx_dev) {      // the whole list, in front of any forward: nothing reads a row before the verdict is in
    c->score_status[0] = 0; c->score_status[1] = 0;
    const int nb = (int)std::min<int64_t>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(iql_score_check_idx_kernel, dim3(nb), dim3(256), 0, st, (const long long*)idx_dev, (long long)n,
                       (long long)n_rows, c->score_status);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    if (((volatile unsigned long long*)c->score_status)[0])
      return fail(IQLHIP_EINDEX, "index %lld is out of bounds for dimension 0 with size %lld",
                  (long long)((volatile unsigned long long*)c->score_status)[1], (long long)n_rows);
  }
  const iqlhip_layout& L = c->L;
  const float* tb = c->target - L.target_src;
  const int S = c->dims.state_dim, A = c->dims.action_dim;
  ScoreParams p;
  memset(&p, 0, sizeof p);
  // instances: V(s'), V(s), Qt1, Qt2, Q1, Q2, pi (make_step's order) — the fp32 masters whatever the context's precision
  p.inst[0] = net_ptrs(L.net[IQLHIP_NET_V], c->params);  p.xoff[0] = S + A;
  p.inst[1] = net_ptrs(L.net[IQLHIP_NET_V], c->params);
  p.inst[2] = net_ptrs(L.net[IQLHIP_NET_Q1], tb);
  p.inst[3] = net_ptrs(L.net[IQLHIP_NET_Q2], tb);
  p.inst[4] = net_ptrs(L.net[IQLHIP_NET_Q1], c->params);
  p.inst[5] = net_ptrs(L.net[IQLHIP_NET_Q2], c->params);
  p.inst[6] = net_ptrs(L.net[IQLHIP_NET_PI], c->params);
  p.rows = rows_dev; p.ld = ld; p.A = A;
  p.heads = c->score_heads; p.pi = c->score_pi;
  ScoreRowsParams q;
  memset(&q, 0, sizeof q);
  q.rows = rows_dev; q.ld = ld; q.S = S; q.A = A; q.policy = c->dims.policy; q.hy = c->hyper;
  q.log_std = (L.net[IQLHIP_NET_PI].log_std >= 0) ? c->params + L.net[IQLHIP_NET_PI].log_std : nullptr;
  q.heads = c->score_heads; q.pi = c->score_pi; q.part = c->score_part;
  const size_t lds = score_lds(c);
  // two blocks per CU where their LDS allows it; a group = the 28 (instance, column slice) blocks of one tile stream
  const int slots = c->n_cus * ((lds <= (size_t)80 * 1024) ? 2 : 1);
  for (int64_t done = 0; done < n; done += chunk) {
    const int m = (int)std::min<int64_t>(chunk, n - done);
    const int n_tiles = (m + RT_ROWS - 1) / RT_ROWS;
    p.idx = idx_dev ? (const long long*)idx_dev + done : nullptr;
    p.row0 = row0 + done; p.n = m; p.n_tiles = n_tiles;
    const int ngrp = std::max(1, std::min(n_tiles, slots / 28));
    hipLaunchKernelGGL(iql_score_fwd_kernel, dim3(28 * ngrp), dim3(256), lds, st, p);
    q.idx = p.idx; q.row0 = p.row0; q.n = m; q.n_tiles = n_tiles;
    q.out = out_dev ? out_dev + (size_t)done * IQLHIP_N_SCORE : nullptr;
    hipLaunchKernelGGL(iql_score_rows_kernel, dim3((n_tiles + 3) / 4), dim3(256), 0, st, q);
    if (summary) {
      const bool last = done + chunk >= n;
      hipLaunchKernelGGL(iql_score_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)c->score_part, n_tiles, c->score_acc,
                         done == 0 ? 1 : 0, (long long)n, last ? c->score_pin : (float*)nullptr);
    }
  }
  HIPCHK(hipGetLastError());
  if (summary) {
    HIPCHK(hipStreamSynchronize(st));
    for (int j = 0; j < 11; ++j) summary[j] = ((volatile float*)c->score_pin)[j];
  }
  return IQLHIP_OK;
}

// ---------------------------------------------------------------------------
// iqlhip_score_rows for every member of a trainer group in one set of launches (include/iqlhip.h "group scoring").
// Per chunk: one forward (a few for large chunks, see the loop), one row kernel, one spread kernel (when asked for) and one finish kernel (when a summary is
// asked for), each with grid.y = member.  The members' records describe the whole call and are uploaded once; the
// launches name the chunk.  Nothing of a member is written: parameters and targets are read, every intermediate lies
// in the group's own scratch.
static int64_t group_score_cap(int k) { return (int64_t)(SCORE_CHUNK / k / RT_ROWS) * RT_ROWS; }
// what one more forward launch costs, in tiles of one block: about 12 us of launch and weight staging against 4.4 us a
// tile (solo calls cut into smaller chunks, profiles/group_score_bench.txt)
#define SCORE_LAUNCH_TILES 3
static int ensure_group_score(iqlhip_group* g) {
  const iqlhip_ctx* c0 = g->m[0];
  if (!g->score_heads) {
    const size_t K = (size_t)g->k, cap = (size_t)group_score_cap(g->k);
    const size_t b_heads = K * cap * HEAD_LD * sizeof(float), b_pi = K * cap * c0->dims.action_dim * NSPLIT * sizeof(float),
                 b_part = K * (cap / RT_ROWS) * SCORE_N_PART * sizeof(float), b_out = K * cap * IQLHIP_N_SCORE * sizeof(float);
    CachedStaging& stg = g->score;      // (laid out and allocated in place: the owner keeps the addresses of its members)
    const int rc = all_or_nothing(g->own, [&]() -> int {
      Owned& own = g->own;
      HIPCHK(own.dev(&g->score_heads, b_heads, 0));
      HIPCHK(own.dev(&g->score_pi, b_pi, 0));
      HIPCHK(own.dev(&g->score_part, b_part, 0));
      HIPCHK(own.dev(&g->score_out, b_out, 0));
      HIPCHK(own.dev(&g->score_acc, K * 16 * sizeof(double), 0));
      HIPCHK(own.pin(&g->score_pin, K * 16 * sizeof(float), /*zero=*/true));
      HIPCHK(own.pin(&g->score_status, K * 2 * sizeof(unsigned long long), /*zero=*/true));
      g->score_ps = stg.add<ScoreParams>(K);
      g->score_qs = stg.add<ScoreRowsParams>(K);
      g->score_aux = stg.add<ScoreGroupAux>(K);
      HIPCHK(stg.alloc(own));
      return IQLHIP_OK;
    });
    if (rc) {
      stg.bytes = 0;      // (a retry lays out again)
      return rc;
    }
    g->score_chunk = (int)cap;
  }
  // every call: the limit belongs to the kernel, not to the group, and another live group of other dims may have set its own
  HIPCHK(hipFuncSetAttribute((const void*)&iql_score_fwd_group_kernel<>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)score_lds(c0)));
  return IQLHIP_OK;
}

extern "C" int iqlhip_group_score_rows(iqlhip_group* g, const float* const* rows_dev, int64_t ld, const int64_t* n_rows,
                                       int64_t row0, int64_t n, const int64_t* const* idx_dev, float* const* out_dev,
                                       float* spread_dev, int32_t chunk_rows, float* summary, void* stream) {
  if (!g || !rows_dev || !n_rows) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n < 1) return fail(IQLHIP_EINVAL, "n = %lld rows to score", (long long)n);
  if (chunk_rows < 0 || (chunk_rows % RT_ROWS)) return fail(IQLHIP_EINVAL, "chunk_rows %d: need 0 or a positive multiple of %d", chunk_rows, RT_ROWS);
  if (((uintptr_t)spread_dev) & 15) return fail(IQLHIP_EINVAL, "spread must be 16-byte aligned");
  int rc = group_check_members(g->m, g->k, g->flags);
  if (rc) return rc;
  const int K = g->k;
  const iqlhip_ctx* c0 = g->m[0];
  bool any_out = false;
  for (int i = 0; i < K; ++i) {
    if (!rows_dev[i]) return fail(IQLHIP_EINVAL, "member %d: NULL rows", i);
    if (idx_dev && !idx_dev[i]) return fail(IQLHIP_EINVAL, "member %d: NULL index list", i);
    float* o = out_dev ? out_dev[i] : nullptr;
    if ((((uintptr_t)rows_dev[i]) | ((uintptr_t)o)) & 15) return fail(IQLHIP_EINVAL, "member %d: rows and out must be 16-byte aligned", i);
    any_out = any_out || o;
    if (n_rows[i] < 1) return fail(IQLHIP_EINVAL, "member %d: n_rows = %lld", i, (long long)n_rows[i]);
    if (!idx_dev && (row0 < 0 || row0 > n_rows[i] || n > n_rows[i] - row0))
      return fail(IQLHIP_EINVAL, "member %d: rows [%lld, %lld) outside the buffer's [0, %lld)", i, (long long)row0, (long long)(row0 + n), (long long)n_rows[i]);
  }
  if (!any_out && !spread_dev && !summary) return fail(IQLHIP_EINVAL, "nothing to write: out_dev, spread_dev and summary are all NULL");
  if (ld < c0->row_ld || (ld & 3)) return fail(IQLHIP_EINVAL, "row stride %lld: need a multiple of 4 >= %lld", (long long)ld, (long long)c0->row_ld);
  for (int i = 0; i < K; ++i)
    if ((rc = group_check_bound(g, i))) return rc;
  DevGuard guard(g->device);
  if ((rc = ensure_group_score(g))) return rc;
  const int64_t chunk = (chunk_rows == 0) ? g->score_chunk : std::min<int64_t>(chunk_rows, g->score_chunk);
  hipStream_t st = (hipStream_t)stream;
  const int S = c0->dims.state_dim, A = c0->dims.action_dim;
  const size_t cap = (size_t)g->score_chunk;

  // the members' records (written whole into the build buffer, whose padding bytes stay zero: equal records compare equal)
  ScoreParams* ps = g->score.build(g->score_ps);
  ScoreRowsParams* qs = g->score.build(g->score_qs);
  ScoreGroupAux* aux = g->score.build(g->score_aux);
  ScoreSpreadSrc src;
  long long src_step[IQLHIP_MAX_GROUP];
  memset(&src, 0, sizeof src);
  for (int i = 0; i < K; ++i) {
    const iqlhip_ctx* c = g->m[i];
    const iqlhip_layout& L = c->L;
    const float* tb = c->target - L.target_src;
    float* heads = g->score_heads + (size_t)i * cap * HEAD_LD;
    float* pi = g->score_pi + (size_t)i * cap * A * NSPLIT;
    ScoreParams& p = ps[i];
    memset(&p, 0, sizeof p);
    // instances: V(s'), V(s), Qt1, Qt2, Q1, Q2, pi (iqlhip_score_rows) — the fp32 masters whatever the members' precision
    p.inst[0] = net_ptrs(L.net[IQLHIP_NET_V], c->params);  p.xoff[0] = S + A;
    p.inst[1] = net_ptrs(L.net[IQLHIP_NET_V], c->params);
    p.inst[2] = net_ptrs(L.net[IQLHIP_NET_Q1], tb);
    p.inst[3] = net_ptrs(L.net[IQLHIP_NET_Q2], tb);
    p.inst[4] = net_ptrs(L.net[IQLHIP_NET_Q1], c->params);
    p.inst[5] = net_ptrs(L.net[IQLHIP_NET_Q2], c->params);
    p.inst[6] = net_ptrs(L.net[IQLHIP_NET_PI], c->params);
    p.rows = rows_dev[i]; p.ld = ld; p.A = A;
    p.idx = idx_dev ? (const long long*)idx_dev[i] : nullptr;
    p.row0 = row0;
    p.heads = heads; p.pi = pi;
    ScoreRowsParams& q = qs[i];
    memset(&q, 0, sizeof q);
    q.rows = rows_dev[i]; q.ld = ld; q.idx = p.idx; q.row0 = row0;
    q.S = S; q.A = A; q.policy = c->dims.policy; q.hy = c->hyper;
    q.log_std = (L.net[IQLHIP_NET_PI].log_std >= 0) ? c->params + L.net[IQLHIP_NET_PI].log_std : nullptr;
    q.heads = heads; q.pi = pi;
    q.part = g->score_part + (size_t)i * (cap / RT_ROWS) * SCORE_N_PART;
    float* o = out_dev ? out_dev[i] : nullptr;
    ScoreGroupAux& a = aux[i];
    memset(&a, 0, sizeof a);
    a.n_rows = n_rows[i];
    a.status = g->score_status + 2 * i;
    if (o) { q.out = o; a.out_step = IQLHIP_N_SCORE; }
    else if (spread_dev) { q.out = g->score_out + (size_t)i * cap * IQLHIP_N_SCORE; a.out_step = 0; }
    src.src[i] = q.out;
    src_step[i] = a.out_step;
  }
  HIPCHK(g->score.upload_if_changed(g->score.bytes, st));
  const ScoreParams* d_ps = g->score.device(g->score_ps);
  const ScoreRowsParams* d_qs = g->score.device(g->score_qs);
  const ScoreGroupAux* d_aux = g->score.device(g->score_aux);
  if (idx_dev) {      // every member's whole list, in front of any forward: nothing reads a row before the verdict is in
    memset(g->score_status, 0, (size_t)K * 2 * sizeof(unsigned long long));
    const int nb = (int)std::min<int64_t>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(iql_score_check_idx_group_kernel<>, dim3(nb, K), dim3(256), 0, st, d_qs, d_aux, (long long)n, nb);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < K; ++i)
      if (((volatile unsigned long long*)g->score_status)[2 * i])
        return fail(IQLHIP_EINDEX, "member %d: index %lld is out of bounds for dimension 0 with size %lld", i,
                    (long long)((volatile unsigned long long*)g->score_status)[2 * i + 1], (long long)n_rows[i]);
  }
  const size_t lds = score_lds(c0);
  // two blocks per CU where their LDS allows it: `streams` tile streams of 28 blocks fill the device, as in the solo call
  const int slots = c0->n_cus * ((lds <= (size_t)80 * 1024) ? 2 : 1);
  const int streams = std::max(1, slots / 28);
  for (int64_t done = 0; done < n; done += chunk) {
    const int m = (int)std::min<int64_t>(chunk, n - done);
    const int n_tiles = (m + RT_ROWS - 1) / RT_ROWS;
    // The chunk's forward: ONE launch over all K members (streams / K tile streams each, rounded down) where that is
    // cheapest — small chunks —, otherwise several launches over d members each, d dividing `streams`, so that every
    // launch fills the device (K = 2 with 9 streams: 4 + 4 of them in one launch leave an eighth of the device idle,
    // 9 and then 9 do not).  Costs in tile times of the slowest block; a launch's ramp is worth about
    // SCORE_LAUNCH_TILES of them (profiles/group_score_bench.txt).  Any cut gives the same bits.
    const int one_ngrp = std::max(1, std::min(n_tiles, streams / K));
    const int64_t one_cost = (int64_t)((n_tiles + one_ngrp - 1) / one_ngrp) * ((28 * one_ngrp * K + slots - 1) / slots) + SCORE_LAUNCH_TILES;
    int64_t cut_cost = 0;
    for (int i0 = 0, d; i0 < K; i0 += d) {
      for (d = std::min(K - i0, streams); streams % d; --d) {}
      const int ngrp = std::min(n_tiles, streams / d);
      cut_cost += (n_tiles + ngrp - 1) / ngrp + SCORE_LAUNCH_TILES;
    }
    const bool cut = cut_cost < one_cost;
    for (int i0 = 0, d; i0 < K; i0 += d) {
      d = K - i0;
      if (cut)
        for (d = std::min(d, streams); streams % d; --d) {}
      const int ngrp = std::max(1, std::min(n_tiles, streams / d));
      hipLaunchKernelGGL(iql_score_fwd_group_kernel<>, dim3(28 * ngrp, d), dim3(256), lds, st, d_ps + i0, (long long)done, m, ngrp);
    }
    hipLaunchKernelGGL(iql_score_rows_group_kernel<>, dim3((n_tiles + 3) / 4, K), dim3(256), 0, st, d_qs, d_aux, (long long)done, m);
    if (spread_dev) {
      ScoreSpreadSrc at = src;
      for (int i = 0; i < K; ++i) at.src[i] = src.src[i] + done * src_step[i];
      hipLaunchKernelGGL(iql_score_spread_group_kernel<>, dim3((m + 255) / 256), dim3(256), 0, st, at, K, m,
                         spread_dev + (size_t)done * (2 * IQLHIP_N_SCORE));
    }
    if (summary) {
      const bool last = done + chunk >= n;
      hipLaunchKernelGGL(iql_score_finish_group_kernel<>, dim3(1, K), dim3(256), 0, st, d_qs, n_tiles, g->score_acc,
                         done == 0 ? 1 : 0, (long long)n, last ? g->score_pin : (float*)nullptr);
    }
  }
  HIPCHK(hipGetLastError());
  if (summary) {
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < K; ++i)
      for (int j = 0; j < 11; ++j) summary[11 * i + j] = ((volatile float*)g->score_pin)[16 * i + j];
  }
  return IQLHIP_OK;
}

extern "C" int iqlhip_pack_rows(iqlhip_ctx* c, const iqlhip_batch* b, float* rows_out_dev, void* stream) {
  if (!c || !b || !rows_out_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (b->rows < 1) return fail(IQLHIP_EINVAL, "batch rows %d", b->rows);
  if (b->idx_dev) return fail(IQLHIP_EINVAL, "iqlhip_pack_rows takes no index list");
  if (!b->s_dev || !b->a_dev || !b->r_dev || !b->ns_dev || !b->d_dev) return fail(IQLHIP_EINVAL, "NULL batch tensor");
  if (b->ld_s < c->dims.state_dim || b->ld_ns < c->dims.state_dim || b->ld_a < c->dims.action_dim || b->ld_r < 1 || b->ld_d < 1)
    return fail(IQLHIP_EINVAL, "batch row strides smaller than the row widths");
  if (((uintptr_t)rows_out_dev) & 15) return fail(IQLHIP_EINVAL, "packed rows must be 16-byte aligned");
  DevGuard guard(c->device);
  const int64_t ld = c->row_ld;
  const int64_t slice = 1 << 20;        // rows per launch: iql_pack_kernel counts elements in 32 bits
  for (int64_t r0 = 0; r0 < b->rows; r0 += slice) {
    const int m = (int)std::min<int64_t>(slice, b->rows - r0);
    const int64_t total = (int64_t)m * ld;
    hipLaunchKernelGGL(iql_pack_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 65536)), dim3(256), 0,
                       (hipStream_t)stream, rows_out_dev + r0 * ld, (int)ld, c->dims.state_dim, c->dims.action_dim, m,
                       b->s_dev + r0 * b->ld_s, (long long)b->ld_s, b->a_dev + r0 * b->ld_a, (long long)b->ld_a,
                       b->r_dev + r0 * b->ld_r, (long long)b->ld_r, b->ns_dev + r0 * b->ld_ns, (long long)b->ld_ns,
                       b->d_dev + r0 * b->ld_d, (long long)b->ld_d);
  }
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

// ---------------------------------------------------------------------------
// Weighted replay sampling (include/iqlhip.h "weighted replay sampling"; kernels: iqlhip_weighted_kernels.h, included
// HERE, behind every other kernel of the file, as the scoring kernels are).  A table is an object of its own, not part
// of a context: a replay buffer owns it, any context on its device may draw by it.  The multi-step driver above does
// the rest (ChunkSrc::wt).
#include "iqlhip_weighted_kernels.h"
struct iqlhip_weights {
  Owned own;                              // the table, and the build's scratch
  int device = 0;
  unsigned long long* tab = nullptr;      // level 0 = cum[0..n), then the search levels, each from a multiple of 64 entries
  unsigned long long* tile_sums = nullptr;
  unsigned* verdict = nullptr;            // iql_wt_validate_kernel's two words
  int64_t n = 0;
  int levels = 0;
  uint64_t total = 0;
  uint64_t gen = 0;                       // unique per built table: what IQLHIP_TS_CONTINUE compares
  // updatable tables (iqlhip_weights_build_updatable): node-local prefix sums, a scale fixed for the table's life
  bool local = false;
  int sh0 = 0;                            // 38 - e
  unsigned sat_bits = 0;                  // the bit pattern of 2^(e + 1)
  unsigned* stamp = nullptr;              // [n]: which entry of the running update sets a row (zero between updates)
  unsigned* flags = nullptr;              // the sticky flag word
  unsigned long long* delta = nullptr;    // [WT_UPDATE_SLICE]: q_new - q_old of a slice's entries
  uint64_t version = 0;                   // content version: every iqlhip_weights_update adds 1
  // tracking tables (iqlhip_weights_build_tracking): the largest q an applied update or the build has seen; never falls
  unsigned long long* q_max = nullptr;    // one device word at the table's scale; null: the table does not track
};
#define WT_UPDATE_SLICE 65536             // entries of an update handled per set of launches (the delta scratch: 512 KB)
static std::atomic<uint64_t> g_weights_gen{0};

// Sizes and offsets (in entries) of a table's levels over n rows; returns the level count.
static int weights_levels(int64_t n, unsigned size[WT_MAX_LEVELS], unsigned off[WT_MAX_LEVELS], size_t* entries) {
  unsigned s = (unsigned)n, o = 0;
  int levels = 0;
  for (int l = 0; l < WT_MAX_LEVELS; ++l) {
    size[l] = s; off[l] = o;
    o += (s + 63u) & ~63u;
    if (!levels && s <= 64u) levels = l + 1;
    s = (s + 63u) >> 6;
  }
  if (entries) *entries = o;
  return levels;
}
static WTab weights_tab(const iqlhip_weights* t) {
  return WTab{t->tab, (unsigned)t->n, (unsigned short)t->levels, (unsigned short)(t->local ? 1 : 0)};
}
// A group member's table (iqlhip_group_train_steps_weighted): on the group's device, and weighing exactly the size[k]
// rows the member draws over — every index the descent can resolve is then < size[k].
static int weights_check_member(const iqlhip_weights* t, int member, int64_t size, int device) {
  if (t->device != device) return fail(IQLHIP_EINVAL, "member %d: the table lives on device %d, the group on %d", member, t->device, device);
  if (size != t->n) return fail(IQLHIP_EINVAL, "member %d: size %lld, but the table weighs %lld rows", member, (long long)size, (long long)t->n);
  return IQLHIP_OK;
}

// The validation both builds start with — nothing but its two words exists until the weights have passed; synchronises
// st.  max_bits: the largest bit pattern among the weights (all finite, none negative, one at least above zero).
static int weights_validate(iqlhip_weights* t, const float* w_dev, int64_t n, hipStream_t st, unsigned* max_bits) {
  HIPCHK(t->own.dev(&t->verdict, 2 * sizeof(unsigned), 0));
  hipLaunchKernelGGL(iql_wt_validate_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1024)), dim3(256), 0, st, w_dev,
                     (long long)n, t->verdict);
  HIPCHK(hipGetLastError());
  unsigned verdict[2] = {0u, 0u};
  HIPCHK(hipMemcpyAsync(verdict, t->verdict, sizeof verdict, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (verdict[1] & 1u) return fail(IQLHIP_EINVAL, "weights hold a NaN or an infinity");
  if (verdict[1] & 2u) return fail(IQLHIP_EINVAL, "weights hold a negative value");
  if (!verdict[0]) return fail(IQLHIP_EINVAL, "all weights are zero");
  *max_bits = verdict[0];
  return IQLHIP_OK;
}
// e = floor(log2(x)) of the positive finite float with these bits; every q is a weight's significand shifted by (its
// exponent + 38 - e).
static int weights_exponent(unsigned bits) {
  const unsigned ex = bits >> 23, frac = bits & 0x7FFFFFu;
  const unsigned m = ex ? (frac | 0x800000u) : frac;
  return (ex ? (int)ex - 150 : -149) + (31 - __builtin_clz(m));
}

extern "C" int iqlhip_weights_build(const float* w_dev, int64_t n, void* stream, iqlhip_weights** out) {
  if (!w_dev || !out) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n < 1 || n > IQLHIP_WEIGHTS_MAX_ROWS) return fail(IQLHIP_EINVAL, "n = %lld weights outside [1, 2^24]", (long long)n);
  if (((uintptr_t)w_dev) & 3) return fail(IQLHIP_EINVAL, "weights must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  std::unique_ptr<iqlhip_weights> t(new iqlhip_weights);
  HIPCHK(hipGetDevice(&t->device));
  unsigned size[WT_MAX_LEVELS], off[WT_MAX_LEVELS];
  size_t entries = 0;
  t->n = n;
  t->levels = weights_levels(n, size, off, &entries);
  if (t->levels < 1) return fail(IQLHIP_EINVAL, "n = %lld weights need more than %d levels", (long long)n, WT_MAX_LEVELS);
  const int n_tiles = (int)((n + WT_SCAN_TILE - 1) / WT_SCAN_TILE);        // <= WT_SCAN_TILE: one block scans their sums
  unsigned max_bits = 0;
  int rc = weights_validate(t.get(), w_dev, n, st, &max_bits);
  if (rc) return rc;
  const int sh0 = 38 - weights_exponent(max_bits);      // e = floor(log2(max w))
  HIPCHK(t->own.dev(&t->tab, entries * sizeof(unsigned long long), 0));
  HIPCHK(t->own.dev(&t->tile_sums, (size_t)n_tiles * sizeof(unsigned long long)));
  hipLaunchKernelGGL(iql_wt_tile_sums_kernel, dim3(n_tiles), dim3(256), 0, st, w_dev, (long long)n, sh0, t->tile_sums);
  hipLaunchKernelGGL(iql_wt_scan_sums_kernel, dim3(1), dim3(256), 0, st, t->tile_sums, n_tiles);
  hipLaunchKernelGGL(iql_wt_tile_scan_kernel, dim3(n_tiles), dim3(256), 0, st, w_dev, (long long)n, sh0,
                     (const unsigned long long*)t->tile_sums, t->tab);
  for (int l = 1; l < t->levels; ++l)
    hipLaunchKernelGGL(iql_wt_level_kernel, dim3((size[l] + 255u) / 256u), dim3(256), 0, st,
                       (const unsigned long long*)(t->tab + off[l - 1]), size[l - 1], t->tab + off[l], size[l]);
  HIPCHK(hipGetLastError());
  unsigned long long total = 0;
  HIPCHK(hipMemcpyAsync(&total, t->tab + (n - 1), sizeof total, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  t->total = total;
  t->gen = ++g_weights_gen;
  *out = t.release();
  return IQLHIP_OK;
}

extern "C" int iqlhip_weights_free(iqlhip_weights* t) {
  if (!t) return IQLHIP_OK;
  DevGuard guard(t->device);
  (void)hipDeviceSynchronize();           // a draw or a chunk that reads the table may still be queued
  delete t;
  return IQLHIP_OK;
}

extern "C" int iqlhip_weights_info(const iqlhip_weights* t, int64_t* n, uint64_t* total, int32_t* levels, uint64_t* generation,
                                   uint64_t* cum_host) {
  if (!t) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n) *n = t->n;
  if (total) *total = t->total;
  if (levels) *levels = t->levels;
  if (generation) *generation = t->gen;
  if (cum_host) {
    DevGuard guard(t->device);
    HIPCHK(hipMemcpy(cum_host, t->tab, (size_t)t->n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  return IQLHIP_OK;
}

// ---- updatable tables: node-local prefix sums, changed in place (DESIGN.md 6i "updatable tables")
// What a tracking table adds (iqlhip_weights_build_tracking; their kernels are the code object's last, so these are
// defined behind them, at the end of the file): the maximum word and its first value; the tracking instantiation of an
// update's second launch.
static int weights_track_init(iqlhip_weights* t, unsigned max_bits, float new_row_weight, hipStream_t st);
static void launch_update_delta_track(const long long* idx, const float* w, unsigned m, long long bound, const WUpd& u,
                                      unsigned long long* delta, unsigned long long* q_max, hipStream_t st);
// track: iqlhip_weights_build_tracking (new_row_weight checked there); else the table iqlhip_weights_build_updatable always built.
static int weights_build_local(const float* w_dev, int64_t n, int64_t capacity, float max_weight, bool track, float new_row_weight,
                               void* stream, iqlhip_weights** out) {
  if (!w_dev || !out) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n < 1 || capacity < n || capacity > IQLHIP_WEIGHTS_MAX_ROWS)
    return fail(IQLHIP_EINVAL, "n = %lld weights, capacity = %lld: need 1 <= n <= capacity <= 2^24", (long long)n, (long long)capacity);
  if (((uintptr_t)w_dev) & 3) return fail(IQLHIP_EINVAL, "weights must be 4-byte aligned");
  if (!(max_weight >= 0.f) || std::isinf(max_weight)) return fail(IQLHIP_EINVAL, "max_weight must be finite and not negative");
  hipStream_t st = (hipStream_t)stream;
  std::unique_ptr<iqlhip_weights> t(new iqlhip_weights);
  HIPCHK(hipGetDevice(&t->device));
  unsigned size[WT_MAX_LEVELS], off[WT_MAX_LEVELS];
  size_t entries = 0;
  t->n = capacity;
  t->local = true;
  t->levels = weights_levels(capacity, size, off, &entries);
  if (t->levels < 1) return fail(IQLHIP_EINVAL, "capacity = %lld needs more than %d levels", (long long)capacity, WT_MAX_LEVELS);
  unsigned max_bits = 0, given_bits = 0;
  int rc = weights_validate(t.get(), w_dev, n, st, &max_bits);
  if (rc) return rc;
  memcpy(&given_bits, &max_weight, sizeof given_bits);
  // the scale, fixed for the table's life: e = floor(log2(max(max_weight, max w))) (bit patterns of floats >= 0 order as they do)
  const int e = weights_exponent(std::max(max_bits, given_bits & 0x7FFFFFFFu));
  t->sh0 = 38 - e;
  t->sat_bits = (e + 1 >= -126) ? ((unsigned)(e + 1 + 127) << 23) : (1u << (e + 1 + 149));      // 2^(e + 1); e = 127: infinity's
  HIPCHK(t->own.dev(&t->tab, entries * sizeof(unsigned long long), 0));
  HIPCHK(t->own.dev(&t->stamp, (size_t)capacity * sizeof(unsigned), 0));
  HIPCHK(t->own.dev(&t->flags, sizeof(unsigned), 0));
  HIPCHK(t->own.dev(&t->delta, (size_t)WT_UPDATE_SLICE * sizeof(unsigned long long)));
  hipLaunchKernelGGL(iql_wt_local_leaves_kernel, dim3((((unsigned)capacity + 63u) / 64u + 3u) / 4u), dim3(256), 0, st, w_dev,
                     (long long)n, (unsigned)capacity, t->sh0, t->tab);
  for (int l = 1; l < t->levels; ++l)
    hipLaunchKernelGGL(iql_wt_local_level_kernel, dim3(((size[l] + 63u) / 64u + 3u) / 4u), dim3(256), 0, st,
                       (const unsigned long long*)(t->tab + off[l - 1]), size[l - 1], t->tab + off[l], size[l]);
  if (track && (rc = weights_track_init(t.get(), max_bits, new_row_weight, st))) return rc;
  HIPCHK(hipGetLastError());
  unsigned long long total = 0;
  HIPCHK(hipMemcpyAsync(&total, t->tab + off[t->levels - 1] + size[t->levels - 1] - 1, sizeof total, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  t->total = total;                       // (at build: iqlhip_weights_state reads the current one)
  t->gen = ++g_weights_gen;
  *out = t.release();
  return IQLHIP_OK;
}
extern "C" int iqlhip_weights_build_updatable(const float* w_dev, int64_t n, int64_t capacity, float max_weight, void* stream,
                                              iqlhip_weights** out) {
  return weights_build_local(w_dev, n, capacity, max_weight, /*track=*/false, 0.f, stream, out);
}
extern "C" int iqlhip_weights_build_tracking(const float* w_dev, int64_t n, int64_t capacity, float max_weight,
                                             float new_row_weight, void* stream, iqlhip_weights** out) {
  if (!(new_row_weight > 0.f) || std::isinf(new_row_weight)) return fail(IQLHIP_EINVAL, "new_row_weight must be finite and > 0");
  return weights_build_local(w_dev, n, capacity, max_weight, /*track=*/true, new_row_weight, stream, out);
}

extern "C" int iqlhip_weights_update(iqlhip_weights* t, const int64_t* idx_dev, const float* w_dev, int64_t m, int64_t bound,
                                     void* stream) {
  if (!t || (m > 0 && (!idx_dev || !w_dev))) return fail(IQLHIP_EINVAL, "NULL argument");
  if (!t->local) return fail(IQLHIP_EINVAL, "the table is not updatable (iqlhip_weights_build_updatable)");
  if (m < 0) return fail(IQLHIP_EINVAL, "m = %lld entries", (long long)m);
  if (bound < 0 || bound > t->n) return fail(IQLHIP_EINVAL, "bound = %lld outside [0, %lld]", (long long)bound, (long long)t->n);
  if ((((uintptr_t)idx_dev) & 7) || (((uintptr_t)w_dev) & 3)) return fail(IQLHIP_EINVAL, "indices must be 8-byte, weights 4-byte aligned");
  DevGuard guard(t->device);
  hipStream_t st = (hipStream_t)stream;
  const WUpd u{t->tab, t->stamp, t->flags, (unsigned)t->n, t->levels, t->sh0, t->sat_bits};
  // slice by slice, in order: a later slice's entry overrides an earlier one's as a later position does inside a slice
  for (int64_t j0 = 0; j0 < m; j0 += WT_UPDATE_SLICE) {
    const unsigned k = (unsigned)std::min<int64_t>(WT_UPDATE_SLICE, m - j0);
    const long long* idx = (const long long*)idx_dev + j0;
    const float* w = w_dev + j0;
    hipLaunchKernelGGL(iql_wt_update_stamp_kernel, dim3((k + 255u) / 256u), dim3(256), 0, st, idx, w, k, (long long)bound, u);
    if (t->q_max)
      launch_update_delta_track(idx, w, k, (long long)bound, u, t->delta, t->q_max, st);
    else
      hipLaunchKernelGGL(iql_wt_update_delta_kernel, dim3((k + 255u) / 256u), dim3(256), 0, st, idx, w, k, (long long)bound, u, t->delta);
    hipLaunchKernelGGL(iql_wt_update_apply_kernel, dim3((k + 3u) / 4u), dim3(256), 0, st, idx, w, k, (long long)bound, u,
                       (const unsigned long long*)t->delta);
  }
  HIPCHK(hipGetLastError());
  ++t->version;
  return IQLHIP_OK;
}

extern "C" int iqlhip_weights_clear_flags(iqlhip_weights* t, void* stream) {
  if (!t) return fail(IQLHIP_EINVAL, "NULL argument");
  if (!t->local) return IQLHIP_OK;        // (a static table has no flag word: its build refuses bad weights)
  DevGuard guard(t->device);
  HIPCHK(hipMemsetAsync(t->flags, 0, sizeof(unsigned), (hipStream_t)stream));
  return IQLHIP_OK;
}

extern "C" int iqlhip_weights_state(const iqlhip_weights* t, uint64_t* total, uint32_t* flags, uint64_t* version, uint64_t* q_out) {
  if (!t) return fail(IQLHIP_EINVAL, "NULL argument");
  DevGuard guard(t->device);
  HIPCHK(hipDeviceSynchronize());         // an update may be queued on any stream
  unsigned size[WT_MAX_LEVELS], off[WT_MAX_LEVELS];
  (void)weights_levels(t->n, size, off, nullptr);
  if (total)
    HIPCHK(hipMemcpy(total, t->local ? t->tab + off[t->levels - 1] + size[t->levels - 1] - 1 : t->tab + (t->n - 1), sizeof(uint64_t),
                     hipMemcpyDeviceToHost));
  if (flags) {
    *flags = 0u;
    if (t->local) HIPCHK(hipMemcpy(flags, t->flags, sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  if (version) *version = t->version;
  if (q_out) {
    unsigned long long* q = nullptr;
    HIPCHK(hipMalloc((void**)&q, (size_t)t->n * sizeof(unsigned long long)));
    hipLaunchKernelGGL(iql_wt_leaves_kernel, dim3(((unsigned)t->n + 255u) / 256u), dim3(256), 0, (hipStream_t) nullptr,
                       (const unsigned long long*)t->tab, (unsigned)t->n, t->local ? 1 : 0, q);
    const hipError_t e = hipMemcpy(q_out, q, (size_t)t->n * sizeof(uint64_t), hipMemcpyDeviceToHost);
    (void)hipFree(q);
    HIPCHK(e);
  }
  return IQLHIP_OK;
}

extern "C" int iqlhip_draw_indices_weighted(int64_t* idx_dev, int64_t n_idx, const iqlhip_weights* table, uint64_t seed,
                                            uint64_t offset, void* stream) {
  if (!idx_dev || !table || n_idx < 1) return fail(IQLHIP_EINVAL, "bad argument");
  const int nb = (int)std::min<int64_t>((n_idx + 7) / 8, 1024);      // a wave per index, two indices a pass
  hipLaunchKernelGGL(iql_draw_indices_weighted_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, (long long*)idx_dev,
                     (long long)n_idx, weights_tab(table), (unsigned long long)seed, (unsigned long long)offset);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

static auto fwd_weighted_kernel(bool bf, bool dma, bool multi) {
  return with_bools([](auto MU, auto BF, auto DMA) { return &iql_fwd_weighted_kernel<BF.value, DMA.value, MU.value>; }, multi, bf, dma);
}
// Everything a weighted multi-step call is refused for, before anything is launched or any counter moves (pending
// injected keep-bits: step_entry, as for iqlhip_train_steps).
static int check_weighted_args(iqlhip_ctx* c, const float* rows_dev, int64_t ld, int64_t size, int32_t B,
                               const iqlhip_weights* table) {
  int rc = check_train_args(c, rows_dev, ld, B);
  if (rc) return rc;
  if (!table) return fail(IQLHIP_EINVAL, "NULL argument");
  if (table->device != c->device) return fail(IQLHIP_EINVAL, "the table lives on device %d, the context on %d", table->device, c->device);
  if (size != table->n) return fail(IQLHIP_EINVAL, "size %lld, but the table weighs %lld rows", (long long)size, (long long)table->n);
  if (c->xch_mode != IQLHIP_XCH_NONE)
    return fail(IQLHIP_EUNSUPPORTED, "weighted sampling is not supported with a data-parallel exchange");
  if (use_lb(c, B))
    return fail(IQLHIP_EUNSUPPORTED, "weighted sampling is not supported on the large-batch bf16 path (more than %d rows)", LB_MIN_ROWS);
  if ((rc = inject_check(c))) return rc;
  return ensure_fwd_lds(c, ChunkKind::Weighted);
}
// A call of one of the three kinds that draw by `t`: Weighted, WeightedIs (is_beta its exponent) or — prio_call — Prio.
static ChunkCall weighted_call(const iqlhip_weights* t, ChunkKind kind = ChunkKind::Weighted, float is_beta = 0.f) {
  ChunkCall call;
  call.src.kind = kind; call.src.wt = weights_tab(t);
  call.wt_gen = t->gen; call.wt_ver = t->version; call.is_beta = is_beta;
  return call;
}
extern "C" int iqlhip_train_steps_weighted_prepare(iqlhip_ctx* c, const float* rows_dev, int64_t ld, int32_t B, float inv_batch,
                                                   void* stream, const iqlhip_weights* table) {
  int rc = check_weighted_args(c, rows_dev, ld, table ? table->n : 0, B, table);
  if (rc) return rc;
  return train_steps_prepare(c, rows_dev, ld, B, inv_batch, stream, weighted_call(table));
}
extern "C" int iqlhip_train_steps_weighted(iqlhip_ctx* c, const float* rows_dev, int64_t ld, int64_t size, int32_t B,
                                           const iqlhip_step_scalars* sc, int32_t K, uint64_t seed, uint64_t stream_offset,
                                           int32_t flags, void* stream, const iqlhip_weights* table) {
  if (!sc) return fail(IQLHIP_EINVAL, "NULL argument");
  int rc = check_weighted_args(c, rows_dev, ld, size, B, table);
  if (rc) return rc;
  return train_steps(c, rows_dev, ld, size, B, sc, K, seed, stream_offset, flags, stream, weighted_call(table), 0);
}

// ... with importance-sampling weights (include/iqlhip.h iqlhip_train_steps_weighted_is): chunk graphs of a
// kind of their own — iql_fwd_weighted_is_kernel, whose idle blocks also stage the drawn rows' q and form the step's c,
// and the row-weighted backward.  The kernels: iqlhip_isweight_kernels.h, behind every other kernel (end of file).
// What such a call needs beyond check_weighted_args, before anything is launched or any counter moves: fp32, a valid
// exponent, the staging buffers and the forward's LDS allowance.
static int weighted_is_setup(iqlhip_ctx* c, float is_beta) {
  if (!(is_beta >= 0.f) || !std::isfinite(is_beta)) return fail(IQLHIP_EINVAL, "is_beta must be finite and >= 0");
  if (c->precision == 1) return fail(IQLHIP_EUNSUPPORTED, "per-row loss weights are not supported at bf16 precision");
  DevGuard guard(c->device);
  if (!c->is_buf) HIPCHK(c->own.dev(&c->is_buf, (3 * (size_t)c->dims.max_batch + 4) * sizeof(float), 0));
  return ensure_fwd_lds(c, ChunkKind::WeightedIs);
}
extern "C" int iqlhip_train_steps_weighted_is_prepare(iqlhip_ctx* c, const float* rows_dev, int64_t ld, int32_t B,
                                                      float inv_batch, void* stream, const iqlhip_weights* table) {
  int rc = check_weighted_args(c, rows_dev, ld, table ? table->n : 0, B, table);
  if (!rc) rc = weighted_is_setup(c, 0.f);
  if (rc) return rc;
  return train_steps_prepare(c, rows_dev, ld, B, inv_batch, stream, weighted_call(table, ChunkKind::WeightedIs));
}
extern "C" int iqlhip_train_steps_weighted_is(iqlhip_ctx* c, const float* rows_dev, int64_t ld, int64_t size, int32_t B,
                                              const iqlhip_step_scalars* sc, int32_t K, uint64_t seed, uint64_t stream_offset,
                                              int32_t flags, void* stream, const iqlhip_weights* table, float is_beta) {
  if (!sc) return fail(IQLHIP_EINVAL, "NULL argument");
  int rc = check_weighted_args(c, rows_dev, ld, size, B, table);
  if (!rc) rc = weighted_is_setup(c, is_beta);
  if (rc) return rc;
  return train_steps(c, rows_dev, ld, size, B, sc, K, seed, stream_offset, flags, stream,
                     weighted_call(table, ChunkKind::WeightedIs, is_beta), 0);
}

// ---------------------------------------------------------------------------
// Per-row episode spans, returns and return-to-go (include/iqlhip.h iqlhip_rows_episode_returns; DESIGN.md 6c-2;
// kernels: iqlhip_episode_kernels.h, included HERE, behind every other kernel of the file, as the scoring and the
// weighted-sampling kernels are).  Scratch lives for the call alone, like launch_return_range's.
#include "iqlhip_episode_kernels.h"
static_assert(EP_KEEP_TAIL == IQLHIP_EP_KEEP_TAIL, "kernel and header disagree on the tail flag");

extern "C" int iqlhip_rows_episode_returns(const float* rows_dev, int64_t ld, int32_t S, int32_t A, int64_t row0, int64_t n,
                                           int64_t max_episode_steps, double discount, double state_break_tol, int32_t flags,
                                           const double* sparse_value, double* ep_return_dev, double* return_to_go_dev,
                                           int64_t* ep_first_dev, int64_t* ep_last_dev, int64_t* episodes_out, void* stream) {
  int rc = reward_args_ok(rows_dev, ld, S, A, row0, n, "rows_episode_returns");
  if (rc) return rc;
  if (max_episode_steps < 1) return fail(IQLHIP_EINVAL, "max_episode_steps must be at least 1");
  if (!(discount >= 0.0) || std::isinf(discount)) return fail(IQLHIP_EINVAL, "discount must be finite and not negative");
  if (std::isnan(state_break_tol)) return fail(IQLHIP_EINVAL, "state_break_tol is NaN");
  if (flags & ~IQLHIP_EP_KEEP_TAIL) return fail(IQLHIP_EINVAL, "unknown flag bits 0x%x", (unsigned)(flags & ~IQLHIP_EP_KEEP_TAIL));
  if (!ep_return_dev && !return_to_go_dev && !ep_first_dev && !ep_last_dev && !episodes_out)
    return fail(IQLHIP_EINVAL, "no output requested");
  if (sparse_value && discount == 1.0) return fail(IQLHIP_EINVAL, "the sparse option divides by 1 - discount: discount must not be 1");
  hipStream_t st = (hipStream_t)stream;
  const long long N = (long long)n, T = (long long)max_episode_steps;
  const long long ntiles = (N + RR_TILE - 1) / RR_TILE;
  const int nb = (int)std::min<long long>(ntiles, RR_MAX_BLOCKS);
  const bool rule = state_break_tol >= 0.0;
  const int keep_tail = flags & IQLHIP_EP_KEEP_TAIL;
  // scratch: prev[n] | tile partials[ntiles] | episode count | flag bytes[n]
  const size_t bytes = ((size_t)N + (size_t)ntiles + 1) * sizeof(long long) + (size_t)N;
  char* scratch = nullptr;
  HIPCHK(hipMallocAsync((void**)&scratch, bytes, st));
  long long* prev = (long long*)scratch;
  long long* tiles = prev + N;
  unsigned long long* count = (unsigned long long*)(tiles + ntiles);
  unsigned char* flag = (unsigned char*)(count + 1);
  hipError_t e = hipMemsetAsync(count, 0, sizeof *count, st);
  if (e == hipSuccess) {
    if (rule)
      hipLaunchKernelGGL(iql_ep_break_kernel<true>, dim3((unsigned)std::min<long long>((N + RR_TILE / EP_LANES - 1) / (RR_TILE / EP_LANES), EP_BREAK_MAX_BLOCKS)),
                         dim3(RR_TILE), 0, st, rows_dev, (long long)ld, (int)S, (int)A, (long long)row0, N,
                         state_break_tol * state_break_tol, flag);
    else
      hipLaunchKernelGGL(iql_ep_break_kernel<false>, dim3(nb), dim3(RR_TILE), 0, st, rows_dev, (long long)ld, (int)S, (int)A,
                         (long long)row0, N, 0.0, flag);
    hipLaunchKernelGGL(iql_ep_scan_reduce_kernel, dim3(nb), dim3(RR_TILE), 0, st, (const unsigned char*)flag, N, ntiles, tiles);
    hipLaunchKernelGGL(iql_rr_scan_partials_kernel, dim3(1), dim3(RR_TILE), 0, st, tiles, ntiles);
    hipLaunchKernelGGL(iql_ep_scan_apply_kernel, dim3(nb), dim3(RR_TILE), 0, st, (const unsigned char*)flag, N, ntiles,
                       (const long long*)tiles, prev);
    if (ep_return_dev || return_to_go_dev || episodes_out)
      hipLaunchKernelGGL(iql_ep_walk_kernel, dim3(nb), dim3(RR_TILE), 0, st, rows_dev, (long long)ld, 2 * (int)S + (int)A,
                         (long long)row0, N, ntiles, T, keep_tail, discount, sparse_value ? 1 : 0,
                         sparse_value ? *sparse_value : 0.0, (const long long*)prev, ep_return_dev, return_to_go_dev, count);
    if (ep_return_dev || return_to_go_dev || ep_first_dev || ep_last_dev)
      hipLaunchKernelGGL(iql_ep_rows_kernel, dim3(nb), dim3(RR_TILE), 0, st, N, T, keep_tail, (const long long*)prev,
                         ep_return_dev, return_to_go_dev, (long long*)ep_first_dev, (long long*)ep_last_dev);
    e = hipGetLastError();
  }
  unsigned long long episodes = 0;
  if (e == hipSuccess && episodes_out) {
    e = hipMemcpyAsync(&episodes, count, sizeof episodes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  const hipError_t e_free = hipFreeAsync(scratch, st);
  HIPCHK(e);
  HIPCHK(e_free);
  if (episodes_out) *episodes_out = (int64_t)episodes;
  return IQLHIP_OK;
}

// ---------------------------------------------------------------------------
// JSRL action selection (include/iqlhip.h iqlhip_jsrl_act; the finish kernels: iqlhip_jsrl_kernels.h,
// included HERE, behind every other kernel of the file).  Pack (iql_pack_states_group_kernel), forward
// (iql_act_fwd_group_kernel over the call's records) and finish, with the records uploaded as the group act uploads its.
#include "iqlhip_jsrl_kernels.h"
#include "iqlhip_jsrl_q_kernels.h"

struct iqlhip_jsrl {
  int k = 0;
  int device = 0;
  iqlhip_ctx* l[IQLHIP_MAX_GROUP] = {};      // learners
  iqlhip_ctx* g[IQLHIP_MAX_GROUP] = {};      // guides
  iqlhip_ctx* v[IQLHIP_MAX_GROUP] = {};      // gates (entries may be NULL)
  iqlhip_ctx* c[IQLHIP_MAX_GROUP] = {};      // critics of who == 3 (iqlhip_jsrl_set_critics; NULL: the member's learner)
  int cap[IQLHIP_MAX_GROUP] = {};            // the smallest act capacity of the triple
  Owned own;
  // per member: the packed states (the learner's row stride; xb_v: the gate's own copy where its stride differs, else
  // xb) and the head partials of the three roles
  float* xb[IQLHIP_MAX_GROUP] = {};
  float* xb_v[IQLHIP_MAX_GROUP] = {};
  float* heads_l[IQLHIP_MAX_GROUP] = {};
  float* heads_g[IQLHIP_MAX_GROUP] = {};
  float* heads_v[IQLHIP_MAX_GROUP] = {};
  // who == 3 (allocated by the first call that has one): the critic's packed act rows [cap][row_ld] — row r the guide's
  // candidate, row n + r the learner's — and its scalar head partials [cap][HEAD_LD]
  float* xq[IQLHIP_MAX_GROUP] = {};
  float* heads_q[IQLHIP_MAX_GROUP] = {};
  // the call's records (built in the staging's build buffer, uploaded when their used part differs from the last upload's):
  // packs [4 k], forwards [5 k], finishes [k], critic records [k], then the members' who bytes, back to back from `who`
  CachedStaging act;
  Section<GroupPackRec> packs; Section<StepParams> ps; Section<JsrlFinRec> fins; Section<JsrlQRec> qrecs;
  Section<signed char> who;
  unsigned long long* done_pin = nullptr;    // completion word of IQLHIP_GROUP_ACT_WAIT calls
  unsigned long long done_seq = 0;
  float* on_pin = nullptr;                   // iqlhip_jsrl_online_step: host-mapped [0] the flag (an int), [1] h
};

extern "C" int iqlhip_jsrl_destroy(iqlhip_jsrl* j) {
  if (!j) return fail(IQLHIP_EINVAL, "NULL handle");
  DevGuard guard(j->device);
  (void)hipDeviceSynchronize();       // a call may still be running on some stream
  j->own.release_all();
  delete j;
  return IQLHIP_OK;
}

static int jsrl_check_triples(iqlhip_ctx* const* learners, iqlhip_ctx* const* guides, iqlhip_ctx* const* gates, int k) {
  if (!learners || !guides) return fail(IQLHIP_EINVAL, "NULL learner or guide table");
  if (k < 1 || k > IQLHIP_MAX_GROUP) return fail(IQLHIP_EINVAL, "member count %d outside [1,%d]", k, IQLHIP_MAX_GROUP);
  for (int i = 0; i < k; ++i) {
    const iqlhip_ctx* l = learners[i];
    const iqlhip_ctx* g = guides[i];
    const iqlhip_ctx* v = gates ? gates[i] : nullptr;
    if (!l || !g) return fail(IQLHIP_EINVAL, "member %d: NULL learner or guide", i);
    if (l->device != learners[0]->device || g->device != l->device || (v && v->device != l->device))
      return fail(IQLHIP_EINVAL, "member %d: contexts on different devices", i);
    if (g->dims.state_dim != l->dims.state_dim || (v && v->dims.state_dim != l->dims.state_dim))
      return fail(IQLHIP_EINVAL, "member %d: state_dim differs between learner, guide and gate", i);
    if (g->dims.action_dim != l->dims.action_dim)
      return fail(IQLHIP_EINVAL, "member %d: action_dim differs between learner and guide", i);
  }
  return IQLHIP_OK;
}

extern "C" int iqlhip_jsrl_create(iqlhip_ctx* const* learners, iqlhip_ctx* const* guides, iqlhip_ctx* const* gates, int k,
                                  iqlhip_jsrl** out) {
  if (!out) return fail(IQLHIP_EINVAL, "out is NULL");
  int rc = jsrl_check_triples(learners, guides, gates, k);
  if (rc) return rc;
  iqlhip_jsrl* j = new iqlhip_jsrl();
  j->k = k;
  j->device = learners[0]->device;
  DevGuard guard(j->device);
  auto setup = [&]() -> int {
    size_t who_bytes = 0, lds = 0;
    for (int i = 0; i < k; ++i) {
      iqlhip_ctx* l = j->l[i] = learners[i];
      iqlhip_ctx* g = j->g[i] = guides[i];
      iqlhip_ctx* v = j->v[i] = gates ? gates[i] : nullptr;
      const int cap = j->cap[i] = std::min(std::min(l->act_cap, g->act_cap), v ? v->act_cap : l->act_cap);
      const int A = l->dims.action_dim;
      HIPCHK(j->own.dev(&j->xb[i], (size_t)cap * l->row_ld * sizeof(float), 0));
      HIPCHK(j->own.dev(&j->heads_l[i], (size_t)cap * A * NSPLIT * sizeof(float), 0));
      HIPCHK(j->own.dev(&j->heads_g[i], (size_t)cap * A * NSPLIT * sizeof(float), 0));
      j->xb_v[i] = j->xb[i];
      if (v) {
        HIPCHK(j->own.dev(&j->heads_v[i], (size_t)cap * HEAD_LD * sizeof(float), 0));
        if (v->row_ld != l->row_ld) HIPCHK(j->own.dev(&j->xb_v[i], (size_t)cap * v->row_ld * sizeof(float), 0));
      }
      who_bytes += (size_t)up(cap, 16);
      for (const iqlhip_ctx* c : {(const iqlhip_ctx*)l, (const iqlhip_ctx*)g, (const iqlhip_ctx*)v})
        if (c) lds = std::max(lds, c->lds_fwd_solo);
    }
    j->packs = j->act.add<GroupPackRec>(4 * (size_t)k);
    j->ps = j->act.add<StepParams>(5 * (size_t)k);
    j->fins = j->act.add<JsrlFinRec>(k);
    j->qrecs = j->act.add<JsrlQRec>(k);
    j->who = j->act.add<signed char>(who_bytes);
    HIPCHK(j->act.alloc(j->own));
    HIPCHK(j->own.pin(&j->done_pin, 8 * sizeof(unsigned long long), /*zero=*/true));
    HIPCHK(j->own.pin(&j->on_pin, 8 * sizeof(float), /*zero=*/true));
    return set_max_lds(2, lds, [](unsigned m) { return act_fwd_group_kernel(m & 1, m & 2); });
  };
  rc = setup();
  if (rc) {
    const std::string msg = g_err;
    iqlhip_jsrl_destroy(j);
    g_err = msg;
    return rc;
  }
  *out = j;
  return IQLHIP_OK;
}

// What the host reads out of `who` before anything is launched: which forwards member i needs.
// need_q: the member has a `3` (iqlhip_jsrl_act_q only): both policy forwards, then the critic's stage.
struct JsrlPlan { bool need_l[IQLHIP_MAX_GROUP], need_g[IQLHIP_MAX_GROUP], need_v[IQLHIP_MAX_GROUP], need_q[IQLHIP_MAX_GROUP]; };
// What iqlhip_jsrl_act_q adds to a call's arguments.
struct JsrlQArgs { const float* inv_temp; float* const* q_out; };

// Every check of iqlhip_jsrl_act; moves and launches nothing.  who_max: the largest byte the entry point accepts.
static int jsrl_check(const iqlhip_jsrl* j, const float* const* states, int64_t ld_s, const int32_t* rows,
                      const int8_t* const* who, const float* gate_max, const uint64_t* seeds, const float* max_l,
                      const float* max_g, float* const* actions, int64_t ld_a, float* const* gate_out, int32_t flags,
                      JsrlPlan* plan, int who_max = 2) {
  if (!j) return fail(IQLHIP_EINVAL, "NULL handle");
  if (!states || !rows || !who || !seeds || !max_l || !max_g || !actions) return fail(IQLHIP_EINVAL, "NULL argument");
  int rc = jsrl_check_triples(j->l, j->g, j->v, j->k);
  if (rc) return rc;
  if (flags & ~IQLHIP_GROUP_ACT_WAIT) return fail(IQLHIP_EINVAL, "unknown flags 0x%x", (unsigned)flags);
  for (int i = 0; i < j->k; ++i) {
    const iqlhip_ctx* l = j->l[i];
    const iqlhip_ctx* g = j->g[i];
    const iqlhip_ctx* v = j->v[i];
    if (!l->params || !g->params || (v && !v->params))
      return fail(IQLHIP_ENOTBOUND, "member %d: iqlhip_bind has not been called on its learner, guide or gate", i);
    if (l->act_drop_p > 0.f || g->act_drop_p > 0.f)
      return fail(IQLHIP_EUNSUPPORTED, "member %d: inference dropout (iqlhip_set_act_dropout) is not supported here", i);
    if (rows[i] < 0 || rows[i] > j->cap[i]) return fail(IQLHIP_EINVAL, "member %d: rows %d outside [0, %d]", i, rows[i], j->cap[i]);
    plan->need_l[i] = plan->need_g[i] = plan->need_v[i] = plan->need_q[i] = false;
    if (rows[i] == 0) continue;
    if (!states[i] || !who[i] || !actions[i]) return fail(IQLHIP_EINVAL, "member %d: NULL states, who or actions", i);
    if (ld_s < l->dims.state_dim || ld_a < l->dims.action_dim) return fail(IQLHIP_EINVAL, "row stride smaller than the row");
    bool two = false;
    for (int r = 0; r < rows[i]; ++r) {
      const int w = who[i][r];
      if (w < 0 || w > who_max) return fail(IQLHIP_EINVAL, "member %d: who[%d] = %d outside 0..%d", i, r, w, who_max);
      if (w != 0) plan->need_l[i] = true;
      if (w != 1) plan->need_g[i] = true;
      if (w == 2) two = true;
      if (w == 3) plan->need_q[i] = true;
    }
    const bool wants_h = gate_out && gate_out[i];
    if ((two || wants_h) && !v) return fail(IQLHIP_EINVAL, "member %d: who == 2 or a gate_out entry on a member without a gate", i);
    if (two && !gate_max) return fail(IQLHIP_EINVAL, "who == 2 without gate_max");
    plan->need_v[i] = two || wants_h;
  }
  return IQLHIP_OK;
}

// The launches of a checked call.  done_flag: the completion word the finish stores behind its outputs (one member,
// one block: iqlhip_jsrl_online_step); else IQLHIP_GROUP_ACT_WAIT's own word, or none.
static int jsrl_enqueue(iqlhip_jsrl* j, const JsrlPlan& plan, const float* const* states, int64_t ld_s, const int32_t* rows,
                        const int8_t* const* who, const float* gate_max, const uint64_t* seeds, const float* max_l,
                        const float* max_g, float* const* actions, int64_t ld_a, int32_t* const* use_learner,
                        float* const* gate_out, int32_t flags, hipStream_t st, unsigned long long* done_flag,
                        unsigned long long done_val, const JsrlQArgs* qa = nullptr) {
  const int K = j->k;
  CachedStaging& act = j->act;
  GroupPackRec* packs = act.build(j->packs);
  StepParams* ps = act.build(j->ps);
  JsrlFinRec* fins = act.build(j->fins);
  JsrlQRec* qrecs = act.build(j->qrecs);
  signed char* who_host = act.build(j->who);
  const signed char* who_dev = act.device(j->who);
  // forward records sorted by kernel variant (bit 0: bf16, bit 1: wide layer-0 staging by LDS-DMA): one launch each
  struct Fwd { StepParams p; int variant; size_t lds; int rows; };
  Fwd fwd[3 * IQLHIP_MAX_GROUP], fwd_q[2 * IQLHIP_MAX_GROUP];      // fwd_q: the critics' Q1 and Q2 records (a later launch)
  int n_fwd = 0, n_fwd_q = 0, n_pack = 0, n_req = 0, max_rows = 0, max_pack = 0, max_fin = 0;
  size_t who_off = 0;
  auto add_fwd = [&](const iqlhip_ctx* c, int n, const float* xb, float* heads, int inst) {
    Fwd& f = (inst == 4 || inst == 5) ? fwd_q[n_fwd_q++] : fwd[n_fwd++];
    f.p = act_step_params(c, n);
    f.p.xb = xb;
    f.p.only_inst = inst;
    f.p.slot[inst] = -1;
    f.p.drop_bits = nullptr; f.p.drop_scale = 1.f;
    f.p.sc.heads = heads; f.p.sc.max_batch = 0;
    f.variant = (c->precision == 1 ? 1 : 0) | (c->w0_lds_k > W0_LDS_MAX_K ? 2 : 0);
    f.lds = c->lds_fwd_solo;
    f.rows = n;
  };
  for (int i = 0; i < K; ++i) {
    if (rows[i] == 0) continue;
    iqlhip_ctx* l = j->l[i];
    const iqlhip_ctx* g = j->g[i];
    const iqlhip_ctx* v = j->v[i];
    const int n = rows[i], S = l->dims.state_dim, A = l->dims.action_dim;
    GroupPackRec& pk = packs[n_pack++];
    pk.xb = j->xb[i]; pk.s = states[i]; pk.ld_s = (long long)ld_s; pk.ld = (int)l->row_ld; pk.S = S; pk.n = n;
    max_pack = std::max(max_pack, n * (int)l->row_ld);
    if (plan.need_v[i] && j->xb_v[i] != j->xb[i]) {
      GroupPackRec& pv = packs[n_pack++];
      pv = pk; pv.xb = j->xb_v[i]; pv.ld = (int)v->row_ld;
      max_pack = std::max(max_pack, n * (int)v->row_ld);
    }
    if (plan.need_l[i]) add_fwd(l, n, j->xb[i], j->heads_l[i], 6);
    if (plan.need_g[i]) add_fwd(g, n, j->xb[i], j->heads_g[i], 6);
    if (plan.need_v[i]) add_fwd(v, n, j->xb_v[i], j->heads_v[i], 1);
    JsrlQRec& qr = qrecs[n_req];
    qr = JsrlQRec{};
    if (plan.need_q[i]) {
      // both halves of the critic's rows get the states from the same pack launch (columns past S zeroed), then the
      // candidates launch fills the action columns of the `3` rows; Q1 and Q2 are two records over the 2 n rows
      const iqlhip_ctx* cq = j->c[i] ? j->c[i] : l;
      for (int half = 0; half < 2; ++half) {
        GroupPackRec& pq = packs[n_pack++];
        pq = pk; pq.xb = j->xq[i] + (size_t)half * n * l->row_ld;
      }
      add_fwd(cq, 2 * n, j->xq[i], j->heads_q[i], 4);
      add_fwd(cq, 2 * n, j->xq[i], j->heads_q[i], 5);
      qr.xq = j->xq[i]; qr.heads_q = j->heads_q[i];
      qr.q_out = qa->q_out ? qa->q_out[i] : nullptr;
      qr.inv_temp = qa->inv_temp[i];
      qr.ld_q = (int)l->row_ld; qr.S = S;
    }
    memcpy(who_host + who_off, who[i], (size_t)n);
    JsrlFinRec& f = fins[n_req++];
    f.heads_l = plan.need_l[i] ? j->heads_l[i] : nullptr;
    f.heads_g = plan.need_g[i] ? j->heads_g[i] : nullptr;
    f.heads_v = plan.need_v[i] ? j->heads_v[i] : nullptr;
    f.log_std = (l->L.net[IQLHIP_NET_PI].log_std >= 0) ? l->params + l->L.net[IQLHIP_NET_PI].log_std : nullptr;
    f.who = who_dev + who_off;
    f.out = actions[i];
    f.use_learner = use_learner ? use_learner[i] : nullptr;
    f.gate_out = gate_out ? gate_out[i] : nullptr;
    f.ld_out = (long long)ld_a; f.n = n; f.A = A;
    f.gate_max = gate_max ? gate_max[i] : 0.f;
    f.max_l = max_l[i]; f.max_g = max_g[i]; f.ls_min = l->hyper.log_std_min; f.ls_max = l->hyper.log_std_max;
    f.seed = seeds[i];
    f.call = seeds[i] != 0 ? l->act_calls++ : 0ull;      // (one call number per call, whatever the rows choose)
    who_off += (size_t)up(n, 16);
    max_rows = std::max(max_rows, n);
    max_fin = std::max(max_fin, n * A);
  }
  if (n_req == 0) return IQLHIP_OK;
  std::stable_sort(fwd, fwd + n_fwd, [](const Fwd& a, const Fwd& b) { return a.variant < b.variant; });
  std::stable_sort(fwd_q, fwd_q + n_fwd_q, [](const Fwd& a, const Fwd& b) { return a.variant < b.variant; });
  for (int q = 0; q < n_fwd; ++q) ps[q] = fwd[q].p;
  for (int q = 0; q < n_fwd_q; ++q) ps[n_fwd + q] = fwd_q[q].p;
  HIPCHK(act.upload_if_changed(j->who.off + who_off, st));
  const int pack_nb = std::min((max_pack + 255) / 256, 1024);
  hipLaunchKernelGGL(iql_pack_states_group_kernel, dim3(pack_nb, n_pack), dim3(256), 0, st, act.device(j->packs));
  for (int i = 0; i < K; ++i) {
    if (rows[i] == 0) continue;
    if (plan.need_l[i]) refresh_shadows(j->l[i], st);
    if (plan.need_g[i] && j->g[i] != j->l[i]) refresh_shadows(j->g[i], st);
    if (plan.need_v[i]) refresh_shadows(j->v[i], st);
    if (plan.need_q[i] && j->c[i] && j->c[i] != j->l[i]) refresh_shadows(j->c[i], st);
  }
  // one launch per kernel variant over records [first, first + count) of the uploaded table
  auto launch_fwds = [&](const Fwd* fw, int count, int first) {
    for (int q0 = 0; q0 < count;) {
      int q1 = q0, fr = 0;
      size_t lds = 0;
      for (; q1 < count && fw[q1].variant == fw[q0].variant; ++q1) { fr = std::max(fr, fw[q1].rows); lds = std::max(lds, fw[q1].lds); }
      const int nbx = (fr + RT_ROWS - 1) / RT_ROWS * NSPLIT;
      hipLaunchKernelGGL(act_fwd_group_kernel(fw[q0].variant & 1, fw[q0].variant & 2), dim3(nbx, q1 - q0), dim3(256), lds, st,
                         act.device(j->ps) + first + q0);
      q0 = q1;
    }
  };
  launch_fwds(fwd, n_fwd, 0);
  if (done_flag) {
    if (n_req != 1 || max_fin > 256 || n_fwd_q) return fail(IQLHIP_EINVAL, "a completion flag needs a one-block finish launch");
    hipLaunchKernelGGL(iql_jsrl_finish_done_kernel, dim3(1), dim3(256), 0, st, act.device(j->fins), done_flag, done_val);
    HIPCHK(hipGetLastError());
    return IQLHIP_OK;
  }
  if (n_fwd_q == 0) {
    hipLaunchKernelGGL(iql_jsrl_finish_kernel, dim3((max_fin + 255) / 256, n_req), dim3(256), 0, st, act.device(j->fins));
  } else {      // candidates, the critics' Q forward over them, select (include/iqlhip.h iqlhip_jsrl_act_q)
    const dim3 grid((max_fin + 255) / 256, n_req);
    hipLaunchKernelGGL(iql_jsrl_q_cand_kernel, grid, dim3(256), 0, st, act.device(j->fins), act.device(j->qrecs));
    launch_fwds(fwd_q, n_fwd_q, n_fwd);
    hipLaunchKernelGGL(iql_jsrl_q_select_kernel, grid, dim3(256), 0, st, act.device(j->fins), act.device(j->qrecs));
  }
  if (!(flags & IQLHIP_GROUP_ACT_WAIT)) {
    HIPCHK(hipGetLastError());
    return IQLHIP_OK;
  }
  const unsigned long long wait_val = ++j->done_seq;
  hipLaunchKernelGGL(iql_group_done_kernel, dim3(1), dim3(64), 0, st, j->done_pin, wait_val);
  HIPCHK(hipGetLastError());
  return wait_word(j->done_pin, wait_val, st);
}

extern "C" int iqlhip_jsrl_act(iqlhip_jsrl* j, const float* const* states, int64_t ld_s, const int32_t* rows,
                               const int8_t* const* who, const float* gate_max, const uint64_t* seeds,
                               const float* max_action_learner, const float* max_action_guide, float* const* actions,
                               int64_t ld_a, int32_t* const* use_learner, float* const* gate_out, int32_t flags,
                               void* stream) {
  JsrlPlan plan;
  int rc = jsrl_check(j, states, ld_s, rows, who, gate_max, seeds, max_action_learner, max_action_guide, actions, ld_a,
                      gate_out, flags, &plan);
  if (rc) return rc;
  DevGuard guard(j->device);
  return jsrl_enqueue(j, plan, states, ld_s, rows, who, gate_max, seeds, max_action_learner, max_action_guide, actions,
                      ld_a, use_learner, gate_out, flags, (hipStream_t)stream, nullptr, 0);
}

extern "C" int iqlhip_jsrl_set_critics(iqlhip_jsrl* j, iqlhip_ctx* const* critics) {
  if (!j) return fail(IQLHIP_EINVAL, "NULL handle");
  size_t lds = 0;
  for (int i = 0; i < j->k && critics; ++i) {
    const iqlhip_ctx* c = critics[i];
    const iqlhip_ctx* l = j->l[i];
    if (!c) continue;
    if (c->device != l->device) return fail(IQLHIP_EINVAL, "member %d: critic on another device", i);
    if (c->dims.state_dim != l->dims.state_dim || c->dims.action_dim != l->dims.action_dim)
      return fail(IQLHIP_EINVAL, "member %d: state_dim or action_dim differs between learner and critic", i);
    if (!c->params) return fail(IQLHIP_ENOTBOUND, "member %d: iqlhip_bind has not been called on its critic", i);
    lds = std::max(lds, c->lds_fwd_solo);
  }
  DevGuard guard(j->device);
  if (lds) {
    const int rc = set_max_lds(2, lds, [](unsigned m) { return act_fwd_group_kernel(m & 1, m & 2); });
    if (rc) return rc;
  }
  for (int i = 0; i < j->k; ++i) j->c[i] = (critics && critics[i] != j->l[i]) ? critics[i] : nullptr;
  return IQLHIP_OK;
}

extern "C" int iqlhip_jsrl_act_q(iqlhip_jsrl* j, const float* const* states, int64_t ld_s, const int32_t* rows,
                                 const int8_t* const* who, const float* gate_max, const uint64_t* seeds,
                                 const float* max_action_learner, const float* max_action_guide, float* const* actions,
                                 int64_t ld_a, int32_t* const* use_learner, float* const* gate_out, const float* q_inv_temp,
                                 float* const* q_out, int32_t flags, void* stream) {
  JsrlPlan plan;
  int rc = jsrl_check(j, states, ld_s, rows, who, gate_max, seeds, max_action_learner, max_action_guide, actions, ld_a,
                      gate_out, flags, &plan, /*who_max=*/3);
  if (rc) return rc;
  bool any = false;
  for (int i = 0; i < j->k; ++i) {
    const iqlhip_ctx* c = j->c[i];
    if (c && !c->params) return fail(IQLHIP_ENOTBOUND, "member %d: iqlhip_bind has not been called on its critic", i);
    if (q_inv_temp && !(q_inv_temp[i] >= 0.f)) return fail(IQLHIP_EINVAL, "member %d: q_inv_temp must be >= 0 (infinite: argmax)", i);
    if (rows[i] == 0) continue;
    if (q_out && q_out[i] && !plan.need_q[i]) return fail(IQLHIP_EINVAL, "member %d: a q_out entry on a member without who == 3", i);
    if (!plan.need_q[i]) continue;
    if (!q_inv_temp) return fail(IQLHIP_EINVAL, "who == 3 without q_inv_temp");
    const int cap = std::min(j->cap[i], c ? c->act_cap : j->cap[i]);
    if (2 * (int64_t)rows[i] > cap)
      return fail(IQLHIP_EINVAL, "member %d: who == 3 needs 2 * rows (%d) within the act capacity %d", i, rows[i], cap);
    any = true;
  }
  DevGuard guard(j->device);
  if (any) {      // the critic stage's scratch, made whole or not at all, by the first call that needs it
    const size_t mark = j->own.mark();
    for (int i = 0; i < j->k; ++i) {
      if (!plan.need_q[i] || j->xq[i]) continue;
      hipError_t e = j->own.dev(&j->xq[i], (size_t)j->cap[i] * j->l[i]->row_ld * sizeof(float), 0);
      if (e == hipSuccess) e = j->own.dev(&j->heads_q[i], (size_t)j->cap[i] * HEAD_LD * sizeof(float), 0);
      if (e != hipSuccess) {
        j->own.rollback(mark);
        HIPCHK(e);
      }
    }
  }
  const JsrlQArgs qa{q_inv_temp, q_out};
  return jsrl_enqueue(j, plan, states, ld_s, rows, who, gate_max, seeds, max_action_learner, max_action_guide, actions,
                      ld_a, use_learner, gate_out, flags, (hipStream_t)stream, nullptr, 0, &qa);
}

extern "C" int iqlhip_jsrl_online_step(iqlhip_jsrl* j, float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer,
                                       const float* row_host, const int64_t* idx_host, int32_t n,
                                       const iqlhip_step_scalars* sc, float out[3], const float* act_state_host,
                                       int8_t who, float gate_max, uint64_t act_seed, float max_action_learner,
                                       float max_action_guide, float* act_out_host, int32_t* use_learner_out,
                                       float* gate_out, void* stream) {
  if (!j || !act_state_host || !act_out_host) return fail(IQLHIP_EINVAL, "NULL argument");
  if (j->k != 1) return fail(IQLHIP_EINVAL, "the fused online step takes a handle of one member (this one has %d)", j->k);
  iqlhip_ctx* c = j->l[0];
  const int S = c->dims.state_dim, A = c->dims.action_dim;
  // the selection's arguments: state, action, flag and h in host-mapped words
  const float* states[1] = {c->on_act_pin};
  float* actions[1] = {c->on_act_pin + IQLHIP_MAX_INPUT};
  int32_t* flag[1] = {(int32_t*)j->on_pin};
  float* hout[1] = {gate_out ? j->on_pin + 1 : nullptr};
  const int32_t one[1] = {1};
  const int8_t* whos[1] = {&who};
  const uint64_t seeds[1] = {act_seed};
  JsrlPlan plan;
  int rc = jsrl_check(j, states, S, one, whos, &gate_max, seeds, &max_action_learner, &max_action_guide, actions, A, hout, 0,
                      &plan);
  if (rc) return rc;
  unsigned long long done_val = 0;
  rc = online_step_front(c, rows_dev, ld, capacity, pointer, row_host, idx_host, n, sc, out, /*act_follows=*/true, stream,
                         nullptr, 0, nullptr, 0, &done_val);
  if (rc) return rc;
  DevGuard guard(c->device);
  hipStream_t st = (hipStream_t)stream;
  memcpy(c->on_act_pin, act_state_host, (size_t)S * sizeof(float));
  rc = jsrl_enqueue(j, plan, states, S, one, whos, &gate_max, seeds, &max_action_learner, &max_action_guide, actions, A, flag,
                    hout, 0, st, c->done_pin, done_val);
  if (rc) return rc;
  rc = sync_losses(c, done_val, st, out);
  if (rc) return rc;
  memcpy(act_out_host, c->on_act_pin + IQLHIP_MAX_INPUT, (size_t)A * sizeof(float));
  if (use_learner_out) *use_learner_out = *(const int32_t*)j->on_pin;
  if (gate_out) *gate_out = j->on_pin[1];
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

// ---------------------------------------------------------------------------
// Importance-sampling weights of a weighted draw (include/iqlhip.h "iqlhip_draw_indices_weighted_is").
#include "iqlhip_isweight_kernels.h"

extern "C" int iqlhip_draw_indices_weighted_is(int64_t* idx_dev, float* c_dev, int64_t n_idx, const iqlhip_weights* table,
                                               uint64_t seed, uint64_t offset, int64_t batch_rows, float is_beta, void* stream) {
  if (!idx_dev || !c_dev || !table || n_idx < 1) return fail(IQLHIP_EINVAL, "bad argument");
  if (batch_rows < 1) return fail(IQLHIP_EINVAL, "batch_rows %lld < 1", (long long)batch_rows);
  if (!(is_beta >= 0.f) || !std::isfinite(is_beta)) return fail(IQLHIP_EINVAL, "is_beta must be finite and >= 0");
  const int64_t n_groups = (n_idx + batch_rows - 1) / batch_rows;
  if (n_groups > 0x7FFFFFFF) return fail(IQLHIP_EINVAL, "more than 2^31 - 1 batches in one draw");
  const int nb = (int)std::min<int64_t>((n_idx + 7) / 8, 1024);      // a wave per index, two indices a pass
  hipLaunchKernelGGL(iql_draw_indices_weighted_q_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, (long long*)idx_dev, c_dev,
                     (long long)n_idx, weights_tab(table), (unsigned long long)seed, (unsigned long long)offset);
  hipLaunchKernelGGL(iql_is_weights_kernel, dim3((unsigned)n_groups), dim3(256), 0, (hipStream_t)stream, c_dev, (long long)n_idx,
                     (long long)batch_rows, is_beta);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

static auto fwd_weighted_is_kernel(bool dma, bool multi) {      // (fp32 only: the row-weighted backward is)
  return with_bools([](auto MU, auto DMA) { return &iql_fwd_weighted_is_kernel<DMA.value, MU.value>; }, multi, dma);
}

// ---------------------------------------------------------------------------
// (declared next to the other selectors; here so that its instantiations are the code object's last)
static BwdRwFn bwd_rw_kernel(bool full, bool multi) {
  return with_bools([](auto MU, auto FU) -> BwdRwFn { return &iql_bwd_rw_kernel<FU.value, MU.value>; }, multi, full);
}

// ---------------------------------------------------------------------------
// Prioritised replay (include/iqlhip.h "iqlhip_weights_update_td", "iqlhip_train_steps_prioritized"; DESIGN.md 6j
// "Prioritised replay inside the chunk graphs"; kernels: iqlhip_prio_kernels.h, the code object's last).
#include "iqlhip_prio_kernels.h"

// alpha and eps of a priority: finite, not negative, and not both zero (a zero TD error would then give log2(0) * 0, a NaN
// — the row would be skipped and flagged instead of getting the priority 1 that alpha = 0 means).
static int prio_exponents_check(float alpha, float eps) {
  if (!(alpha >= 0.f) || !std::isfinite(alpha)) return fail(IQLHIP_EINVAL, "alpha must be finite and >= 0");
  if (!(eps >= 0.f) || !std::isfinite(eps)) return fail(IQLHIP_EINVAL, "eps must be finite and >= 0");
  if (alpha == 0.f && eps == 0.f) return fail(IQLHIP_EINVAL, "alpha = 0 needs eps > 0 (a zero TD error would give log2(0) * 0)");
  return IQLHIP_OK;
}
// The three launches of an update of m entries with TD errors as the weight source.
// q_max != nullptr (a tracking table): the second launch is its tracking instantiation (defined behind its kernel, at the
// end of the file).
static void launch_update_delta_td_track(const long long* idx, const float* td, unsigned m, long long bound, const WUpd& u,
                                         unsigned long long* delta, const PrioArgs& a, unsigned long long* q_max, hipStream_t st);
static void launch_update_td(const WUpd& u, const long long* idx, const float* td, unsigned m, long long bound,
                             unsigned long long* delta, const PrioArgs& a, hipStream_t st, unsigned long long* q_max = nullptr) {
  hipLaunchKernelGGL(iql_wt_update_stamp_td_kernel, dim3((m + 255u) / 256u), dim3(256), 0, st, idx, td, m, bound, u, a);
  if (q_max)
    launch_update_delta_td_track(idx, td, m, bound, u, delta, a, q_max, st);
  else
    hipLaunchKernelGGL(iql_wt_update_delta_td_kernel, dim3((m + 255u) / 256u), dim3(256), 0, st, idx, td, m, bound, u, delta, a);
  hipLaunchKernelGGL(iql_wt_update_apply_td_kernel, dim3((m + 3u) / 4u), dim3(256), 0, st, idx, td, m, bound, u,
                     (const unsigned long long*)delta, a);
}

extern "C" int iqlhip_weights_update_td(iqlhip_weights* t, const int64_t* idx_dev, const float* td_dev, int64_t m, int64_t bound,
                                        float alpha, float eps, void* stream) {
  if (!t || (m > 0 && (!idx_dev || !td_dev))) return fail(IQLHIP_EINVAL, "NULL argument");
  if (!t->local) return fail(IQLHIP_EINVAL, "the table is not updatable (iqlhip_weights_build_updatable)");
  if (m < 0) return fail(IQLHIP_EINVAL, "m = %lld entries", (long long)m);
  if (bound < 0 || bound > t->n) return fail(IQLHIP_EINVAL, "bound = %lld outside [0, %lld]", (long long)bound, (long long)t->n);
  if ((((uintptr_t)idx_dev) & 7) || (((uintptr_t)td_dev) & 7)) return fail(IQLHIP_EINVAL, "indices and TD errors must be 8-byte aligned");
  if (int rc = prio_exponents_check(alpha, eps)) return rc;
  DevGuard guard(t->device);
  hipStream_t st = (hipStream_t)stream;
  const WUpd u{t->tab, t->stamp, t->flags, (unsigned)t->n, t->levels, t->sh0, t->sat_bits};
  const PrioArgs a{nullptr, alpha, eps};
  // slice by slice, in order, as iqlhip_weights_update
  for (int64_t j0 = 0; j0 < m; j0 += WT_UPDATE_SLICE) {
    const unsigned k = (unsigned)std::min<int64_t>(WT_UPDATE_SLICE, m - j0);
    launch_update_td(u, (const long long*)idx_dev + j0, td_dev + 2 * j0, k, (long long)bound, t->delta, a, st, t->q_max);
  }
  HIPCHK(hipGetLastError());
  ++t->version;
  return IQLHIP_OK;
}

static auto fwd_prio_kernel(bool dma, bool multi) {      // (fp32 only: the row-weighted backward is)
  return with_bools([](auto MU, auto DMA) { return &iql_fwd_prio_kernel<DMA.value, MU.value>; }, multi, dma);
}
// (declared in front of launch_fwd_grid; here, behind the last kind's selector)
static const void* fwd_kernel_of(ChunkKind kind, bool bf, bool dma, bool multi) {
  switch (kind) {
    case ChunkKind::Plain: return (const void*)fwd_kernel(bf, dma, multi);
    case ChunkKind::Mixed: return (const void*)fwd_mixed_kernel(bf, dma, multi);
    case ChunkKind::Weighted: return (const void*)fwd_weighted_kernel(bf, dma, multi);
    case ChunkKind::WeightedIs: return (const void*)fwd_weighted_is_kernel(dma, multi);      // (fp32 only, as Prio)
    case ChunkKind::Prio: return (const void*)fwd_prio_kernel(dma, multi);
  }
  return nullptr;
}
// Step k of a prioritised chunk has run: table[idx of staging half k & 1] <- td_priority(its TD errors), alpha, eps and the
// live word read from the call's device words.  m, bound and every pointer are constants of the chunk graph.
static void launch_prio_update(const iqlhip_ctx* c, const ChunkSrc& src, int B, int k, hipStream_t st) {
  const WUpd u{const_cast<unsigned long long*>(src.wt.tab), src.up.stamp, src.up.flags, src.wt.n, (int)src.wt.levels, src.up.sh0,
               src.up.sat_bits};
  const PrioArgs a{prio_words(c), 0.f, 0.f};
  launch_update_td(u, prio_idx(c, k & 1), prio_td(c), (unsigned)B, (long long)src.wt.n, src.up.delta, a, st, src.up.q_max);
}
// What a prioritised call needs beyond check_weighted_args and weighted_is_setup, before anything is launched or any
// counter moves: an updatable table, valid exponents, the staging buffer and the forward's LDS allowance.
static int prio_setup(iqlhip_ctx* c, const iqlhip_weights* table, int32_t B, float alpha, float eps) {
  if (!table->local) return fail(IQLHIP_EINVAL, "the table is not updatable (iqlhip_weights_build_updatable)");
  if (int rc = prio_exponents_check(alpha, eps)) return rc;
  if (B > WT_UPDATE_SLICE) return fail(IQLHIP_EUNSUPPORTED, "prioritised calls take batches of at most %d rows", WT_UPDATE_SLICE);
  DevGuard guard(c->device);
  if (!c->prio_buf) HIPCHK(c->own.dev(&c->prio_buf, 24 * (size_t)c->dims.max_batch + 4 * sizeof(float), 0));
  return ensure_fwd_lds(c, ChunkKind::Prio);
}
static ChunkCall prio_call(const iqlhip_weights* t, float is_beta, float alpha, float eps, unsigned live) {
  ChunkCall call = weighted_call(t, ChunkKind::Prio, is_beta);
  call.src.up = PrioSrc{t->stamp, t->flags, t->delta, t->sh0, t->sat_bits, t->q_max};
  call.alpha = alpha; call.eps = eps; call.live = live;
  return call;
}
extern "C" int iqlhip_train_steps_prioritized_prepare(iqlhip_ctx* c, const float* rows_dev, int64_t ld, int32_t B,
                                                      float inv_batch, void* stream, iqlhip_weights* table) {
  int rc = check_weighted_args(c, rows_dev, ld, table ? table->n : 0, B, table);
  if (!rc) rc = weighted_is_setup(c, 0.f);
  if (!rc) rc = prio_setup(c, table, B, 1.f, 1.f);
  if (rc) return rc;
  // (live = 0: the rehearsal's updates leave the table alone)
  return train_steps_prepare(c, rows_dev, ld, B, inv_batch, stream, prio_call(table, 0.f, 1.f, 1.f, /*live=*/0u));
}
extern "C" int iqlhip_train_steps_prioritized(iqlhip_ctx* c, const float* rows_dev, int64_t ld, int64_t size, int32_t B,
                                              const iqlhip_step_scalars* sc, int32_t K, uint64_t seed, uint64_t stream_offset,
                                              int32_t flags, void* stream, iqlhip_weights* table, float is_beta, float alpha,
                                              float eps) {
  if (!sc) return fail(IQLHIP_EINVAL, "NULL argument");
  int rc = check_weighted_args(c, rows_dev, ld, size, B, table);
  if (!rc) rc = weighted_is_setup(c, is_beta);
  if (!rc) rc = prio_setup(c, table, B, alpha, eps);
  if (rc) return rc;
  rc = train_steps(c, rows_dev, ld, size, B, sc, K, seed, stream_offset, flags, stream,
                   prio_call(table, is_beta, alpha, eps, /*live=*/1u), 0);
  if (!rc) ++table->version;      // the table's content has moved (a failed call leaves no continuation behind anyway)
  return rc;
}

// ---------------------------------------------------------------------------
// Trainer groups: per-row loss weights, importance-sampling weights and prioritised replay (include/iqlhip.h
// "iqlhip_group_step_rw", "iqlhip_group_train_steps_weighted_is", "iqlhip_group_train_steps_prioritized"; DESIGN.md 6j
// "trainer groups"; kernels: iqlhip_group_prio_kernels.h, the code object's last).
#include "iqlhip_group_prio_kernels.h"

static auto bwd_group_rw_kernel(bool full) {      // (fp32 only, one-slice (b) blocks: iql_bwd_group_kernel's form)
  return with_bools([](auto FU) { return &iql_bwd_group_rw_kernel<FU.value>; }, full);
}
static void launch_bwd_group_rw(const iqlhip_ctx* c, const GroupRec* recs, const GroupRwRec* rws, const GroupGeom& q, int K,
                                hipStream_t st) {
  hipLaunchKernelGGL(bwd_group_rw_kernel(q.full), dim3(q.bwd_nb, K), dim3(256), c->lds_bwd, st, recs, rws);
}

static int group_rw_ready(iqlhip_group* g) {
  GroupStage& rw = g->rw;
  Staging& s = rw.stg;
  if (s.dev) return IQLHIP_OK;
  const int k = g->k;
  for (int h = 0; h < 2; ++h) rw.recs[h] = s.add<GroupRec>(k);
  rw.drops = s.add<GroupDropRec>(k);
  for (int h = 0; h < 2; ++h) rw.aux[h].add(s, k);
  g->rw_rws = s.add<GroupRwRec>(k);
  g->rw_prs = s.add<GroupPrioRec>(k);
  rw.tabs = s.add<iqlhip_step_scalars>((size_t)k * IQLHIP_GROUP_MAX_STEPS);
  int max_batch = 0;
  for (int i = 0; i < k; ++i) max_batch = std::max(max_batch, (int)g->m[i]->dims.max_batch);
  const int rc = all_or_nothing(g->own, [&]() -> int {
    HIPCHK(s.alloc(g->own));
    HIPCHK(g->own.dev(&g->rw_ones, (size_t)max_batch * sizeof(float)));
    const std::vector<float> ones((size_t)max_batch, 1.f);
    HIPCHK(hipMemcpy(g->rw_ones, ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice));
    return set_max_lds(1, g->m[0]->lds_bwd, [](unsigned m) { return bwd_group_rw_kernel(m & 1); });
  });
  if (rc) s.bytes = 0;      // (the rollback has nulled the blocks and the event; a retry lays out again)
  return rc;
}

// `rc` of a solo check as member i's refusal: the message names the member.
static int member_fail(int i, int rc) {
  if (!rc) return rc;
  const std::string msg = g_err;
  return fail(rc, "member %d: %s", i, msg.c_str());
}
// What no row-weighted group call is built for (the solo refusals, row_weights_check): bf16.  (An exchange and the
// large-batch path: the group rules, group_check_call.)
static int group_rw_check_member(const iqlhip_group* g, int i) {
  if (g->m[i]->precision == 1) return fail(IQLHIP_EUNSUPPORTED, "member %d: per-row loss weights are not supported at bf16 precision", i);
  return IQLHIP_OK;
}
static int group_rw_check_eager(const iqlhip_group* g, const int32_t* rows, const GroupRwArgs& a) {
  (void)rows;
  if (!a.w || !a.td) return fail(IQLHIP_EINVAL, "NULL argument");
  for (int i = 0; i < g->k; ++i) {
    if (int rc = group_rw_check_member(g, i)) return rc;
    if ((((uintptr_t)a.w[i]) & 3) || (((uintptr_t)a.td[i]) & 7))
      return fail(IQLHIP_EINVAL, "member %d: row weights must be 4-byte, TD errors 8-byte aligned", i);
  }
  return IQLHIP_OK;
}
static const GroupRwRec* group_rw_records(iqlhip_group* g, const GroupRwArgs& a) {
  GroupRwRec* r = g->rw.stg.host(g->rw_rws);
  for (int i = 0; i < g->k; ++i) r[i] = GroupRwRec{a.w[i] ? a.w[i] : g->rw_ones, a.td[i]};
  return g->rw.stg.device(g->rw_rws);
}

extern "C" int iqlhip_group_step_rw(iqlhip_group* g, const iqlhip_batch* batches, const iqlhip_step_scalars* sc,
                                    const float* const* row_w_dev, float* const* td_out_dev, float* out, void* stream) {
  if (!row_w_dev || !td_out_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  const GroupRwArgs a{row_w_dev, td_out_dev};
  return group_step(g, &iqlhip_group::rw, batches, sc, out, stream, /*mixed=*/true, &a);
}

// iqlhip_group_train_steps_weighted_is (alpha == nullptr) and iqlhip_group_train_steps_prioritized.  Per call: the rows of
// step 0 (members that continue have theirs staged), then per step s: the rows, q and indices of step s + 1 into the other
// staging half, the loss weights of step s from its half's q, the step under record set s & 1 with the row-weighted
// backward, and — prioritised — the table updates from its TD errors.  One linear chain on `stream` (the
// hazard table).
static int group_train_steps_rw(iqlhip_group* g, const float* const* rows, int64_t ld, const int64_t* size, const int32_t* B,
                                const void* const* tables, int32_t n, const uint64_t* seeds, const uint64_t* offsets,
                                int32_t flags, void* stream, iqlhip_weights* const* wtabs, const float* is_beta,
                                const float* alpha, const float* eps) {
  const bool prio = alpha != nullptr;
  if (!g || !rows || !size || !B || !tables || !seeds || !offsets || !wtabs || !is_beta || (prio && !eps))
    return fail(IQLHIP_EINVAL, "NULL argument");
  if (flags & ~IQLHIP_GROUP_TS_CONTINUE) return fail(IQLHIP_EINVAL, "unknown flags 0x%x", (unsigned)flags);
  int rc = group_check_call(g, B);
  if (rc) return rc;
  if (n < 1 || n > IQLHIP_GROUP_MAX_STEPS) return fail(IQLHIP_EINVAL, "n_steps outside [1,%d]", IQLHIP_GROUP_MAX_STEPS);
  for (int i = 0; i < g->k; ++i) {
    const iqlhip_ctx* c = g->m[i];
    if ((rc = member_fail(i, check_train_args(c, rows[i], ld, B[i])))) return rc;
    if (size[i] < 1) return fail(IQLHIP_EINVAL, "member %d: empty buffer", i);
    if (!tables[i]) return fail(IQLHIP_EINVAL, "member %d: NULL scalar table", i);
    if ((rc = group_rw_check_member(g, i))) return rc;
    if ((rc = member_fail(i, inject_check(c)))) return rc;
    if (!(is_beta[i] >= 0.f) || !std::isfinite(is_beta[i])) return fail(IQLHIP_EINVAL, "member %d: is_beta must be finite and >= 0", i);
    const iqlhip_weights* t = wtabs[i];
    if (!t) {
      if (prio) return fail(IQLHIP_EINVAL, "member %d: NULL table (a prioritised call updates every member's table)", i);
      continue;
    }
    if ((rc = weights_check_member(t, i, size[i], g->device))) return rc;
    if (!prio) continue;
    if (!t->local) return fail(IQLHIP_EINVAL, "member %d: the table is not updatable (iqlhip_weights_build_updatable)", i);
    if (t->q_max)
      return fail(IQLHIP_EUNSUPPORTED, "member %d: a table that tracks its maximum (iqlhip_weights_build_tracking) is not "
                  "supported in trainer groups", i);
    if ((rc = member_fail(i, prio_exponents_check(alpha[i], eps[i])))) return rc;
    if (B[i] > WT_UPDATE_SLICE) return fail(IQLHIP_EUNSUPPORTED, "member %d: prioritised calls take batches of at most %d rows", i, WT_UPDATE_SLICE);
    for (int j = 0; j < i; ++j)
      if (wtabs[j] == t)
        return fail(IQLHIP_EINVAL, "member %d: the table of member %d again (a prioritised call updates a table per member; "
                    "their updates would race)", i, j);
  }
  DevGuard guard(g->device);
  if ((rc = group_rw_ready(g))) return rc;
  for (int i = 0; i < g->k; ++i) {      // the members' staging halves: the buffers their solo calls of these kinds use
    iqlhip_ctx* c = g->m[i];
    if (!c->is_buf) HIPCHK(c->own.dev(&c->is_buf, (3 * (size_t)c->dims.max_batch + 4) * sizeof(float), 0));
    if (wtabs[i] && !c->prio_buf) HIPCHK(c->own.dev(&c->prio_buf, 24 * (size_t)c->dims.max_batch + 4 * sizeof(float), 0));
  }
  for (int i = 0; i < g->k; ++i) note_stream(g->m[i], stream);
  hipStream_t st = (hipStream_t)stream;
  GroupStage& sg = g->rw;
  Staging& stg = sg.stg;
  HIPCHK(stg.wait_free());
  const GroupGeom q = group_geom(g, B);
  const int cont_class = prio ? 2 : 1;      // (KindInfo::cont_class of the solo kinds: what lies staged besides the rows)
  GroupRec* recs_host[2] = {stg.host(sg.recs[0]), stg.host(sg.recs[1])};
  bool all_cont = true;
  for (int i = 0; i < g->k; ++i) {
    iqlhip_ctx* c = g->m[i];
    const iqlhip_weights* t = wtabs[i];
    const int MB = c->dims.max_batch;
    // does member i start on the rows this group's previous call staged for it?  (the solo rules: train_steps)
    const bool cont = (flags & IQLHIP_GROUP_TS_CONTINUE) && t && c->cont.valid && c->cont.owner == g &&
                      c->cont.cont_class == cont_class && c->cont.wt_gen == t->gen && c->cont.wt_ver == t->version &&
                      c->cont.rows == rows[i] && c->cont.ld == ld && c->cont.size == size[i] && c->cont.B == B[i] &&
                      c->cont.seed == seeds[i] && c->cont.next_offset == offsets[i] && c->cont.drop_p == c->drop_p &&
                      c->cont.drop_seed == c->drop_seed && c->cont.drop_step == c->drop_step;
    c->cont.valid = false;
    all_cont = all_cont && cont;
    refresh_shadows(c, st);
    const iqlhip_step_scalars* tab = (const iqlhip_step_scalars*)tables[i];
    GroupRec& r = recs_host[0][i];
    group_record(g, r, i, q, B[i], n, c->xb, &tab[0], sg.sched(i));
    r.rows = rows[i]; r.ld = ld; r.size = size[i]; r.seed = seeds[i]; r.offset = offsets[i];
    GroupRec& r1 = recs_host[1][i];      // the other half's set: the rows and the keep-bits the odd steps read
    r1 = r;
    r1.p.xb = c->xb2; r1.q_xb = c->xb2; r1.xb = c->xb2;
    if (r1.p.drop_bits) r1.p.drop_bits = c->drop_bits + (size_t)2 * MB * 8;
    memcpy(sg.tab(i), tab, (size_t)n * sizeof(iqlhip_step_scalars));
    GroupPrioRec& w = stg.host(g->rw_prs)[i];
    memset(&w, 0, sizeof w);
    w.wt = t ? weights_tab(t) : WTab{nullptr, 0u, 0, 0};
    w.xb[0] = c->xb; w.xb[1] = c->xb2;
    w.q[0] = c->is_buf; w.q[1] = c->is_buf + MB;
    if (t) { w.idx[0] = prio_idx(c, 0); w.idx[1] = prio_idx(c, 1); }
    w.drop_bits[0] = c->drop_bits; w.drop_bits[1] = c->drop_bits + (size_t)2 * MB * 8;
    w.c = c->is_buf + 2 * (size_t)MB;
    w.beta = is_beta[i];
    w.skip0 = cont ? 1 : 0;
    if (prio) {
      w.up = WUpd{t->tab, t->stamp, t->flags, (unsigned)t->n, t->levels, t->sh0, t->sat_bits};
      w.delta = t->delta;
      w.td = prio_td(c);
      w.bound = (long long)t->n;
      w.m = (unsigned)B[i];
      w.alpha = alpha[i]; w.eps = eps[i];
    }
    stg.host(g->rw_rws)[i] = GroupRwRec{w.c, prio ? prio_td(c) : nullptr};
  }
  // actor dropout: every member's record inside its GroupPrioRec (active = the member draws), step s at drop_step + s into
  // half s & 1 (GroupPrioRec::drop_bits)
  bool draws = false;
  for (int i = 0; i < g->k; ++i) {
    GroupDropRec& d = stg.host(g->rw_prs)[i].drop;
    d = group_drop_record(g->m[i], B[i]);
    d.active = ((g->flags & IQLHIP_GROUP_DROPOUT) && group_draws(g->m[i])) ? 1 : 0;
    draws = draws || d.active;
  }
  GroupAux aux[2];
  for (int h = 0; h < 2; ++h)
    if ((rc = group_aux(g, stg, sg.aux[h], recs_host[h], &aux[h]))) return rc;
  HIPCHK(sg.upload_steps(g->k, n, st));
  const GroupRec* recs[2] = {stg.device(sg.recs[0]), stg.device(sg.recs[1])};
  const GroupPrioRec* prs = stg.device(g->rw_prs);
  const GroupRwRec* rws = stg.device(g->rw_rws);
  // (grids sized by the largest member, as iqlhip_group_train_steps_weighted's: a wave per IQL_GROUP_WT_ROWS_PER_WAVE rows,
  //  the keep-bit words behind the gather at the far end; every record bounds its own member's rows and words)
  const int wt_nb = (q.max_rows + 4 * IQL_GROUP_WT_ROWS_PER_WAVE - 1) / (4 * IQL_GROUP_WT_ROWS_PER_WAVE);
  const int wt_drop_nb = wt_nb + (2 * q.max_rows * 8 + 255) / 256;
  auto gather = [&](int s) {
    if (draws)
      hipLaunchKernelGGL(iql_gather_weighted_qi_drop_group_kernel, dim3(wt_drop_nb, g->k), dim3(256), 0, st, recs[0], prs, s);
    else
      hipLaunchKernelGGL(iql_gather_weighted_qi_group_kernel, dim3(wt_nb, g->k), dim3(256), 0, st, recs[0], prs, s);
  };
  const unsigned upd_nb = ((unsigned)q.max_rows + 255u) / 256u, apply_nb = ((unsigned)q.max_rows + 3u) / 4u;
  if (!all_cont || draws) gather(0);
  for (int s = 0; s < n; ++s) {
    if (s + 1 < n || (n & 1) == 0) gather(s + 1);      // (step n of an even call: what a continuing call starts on)
    hipLaunchKernelGGL(iql_is_weights_group_kernel, dim3(1, g->k), dim3(256), 0, st, recs[0], prs, s);
    group_launch_step(g, recs[s & 1], q, s, st, aux[s & 1], rws);
    if (prio) {
      hipLaunchKernelGGL(iql_wt_update_stamp_td_group_kernel, dim3(upd_nb, g->k), dim3(256), 0, st, prs, s & 1);
      hipLaunchKernelGGL(iql_wt_update_delta_td_group_kernel, dim3(upd_nb, g->k), dim3(256), 0, st, prs, s & 1);
      hipLaunchKernelGGL(iql_wt_update_apply_td_group_kernel, dim3(apply_nb, g->k), dim3(256), 0, st, prs, s & 1);
    }
  }
  if (g->flags & IQLHIP_GROUP_DROPOUT)      // (as iqlhip_train_steps: the position of every context with a rate above 0)
    for (int i = 0; i < g->k; ++i) if (g->m[i]->drop_p > 0.f) g->m[i]->drop_step += (unsigned long long)n;
  for (int i = 0; i < g->k; ++i) {
    iqlhip_ctx* c = g->m[i];
    iqlhip_weights* t = wtabs[i];
    if (t && (n & 1) == 0) {        // an even call ends on staging half 0, where a call's step 0 reads
      c->cont.valid = true;
      c->cont.owner = g;
      c->cont.wt_gen = t->gen; c->cont.wt_ver = t->version + (prio ? 1 : 0); c->cont.cont_class = cont_class;
      c->cont.rows = rows[i]; c->cont.ld = ld; c->cont.size = size[i]; c->cont.B = B[i]; c->cont.seed = seeds[i];
      c->cont.next_offset = offsets[i] + ((unsigned long long)n * (unsigned long long)B[i]) / 2ull;
      c->cont.drop_p = c->drop_p; c->cont.drop_seed = c->drop_seed; c->cont.drop_step = c->drop_step;
    }
    if (prio) ++t->version;         // the table's content has moved (iqlhip_train_steps_prioritized)
  }
  HIPCHK(hipGetLastError());
  g->last_n = n;
  return IQLHIP_OK;
}

extern "C" int iqlhip_group_train_steps_weighted_is(iqlhip_group* g, const float* const* rows, int64_t ld, const int64_t* size,
                                                    const int32_t* B, const void* const* tables, int32_t n,
                                                    const uint64_t* seeds, const uint64_t* offsets, int32_t flags,
                                                    void* stream, const iqlhip_weights* const* wtabs, const float* is_beta) {
  return group_train_steps_rw(g, rows, ld, size, B, tables, n, seeds, offsets, flags, stream,
                              const_cast<iqlhip_weights* const*>(wtabs), is_beta, nullptr, nullptr);
}
extern "C" int iqlhip_group_train_steps_prioritized(iqlhip_group* g, const float* const* rows, int64_t ld, const int64_t* size,
                                                    const int32_t* B, const void* const* tables, int32_t n,
                                                    const uint64_t* seeds, const uint64_t* offsets, int32_t flags,
                                                    void* stream, iqlhip_weights* const* wtabs, const float* is_beta,
                                                    const float* alpha, const float* eps) {
  if (!alpha || !eps) return fail(IQLHIP_EINVAL, "NULL argument");
  return group_train_steps_rw(g, rows, ld, size, B, tables, n, seeds, offsets, flags, stream, wtabs, is_beta, alpha, eps);
}

// ---------------------------------------------------------------------------
// Online prioritised replay: tables that track their maximum, new rows entering at it, and the prioritised online
// iteration in one call (include/iqlhip.h "tracking tables", "iqlhip_online_step_prioritized"; DESIGN.md 6j "Online
// prioritised replay"; kernels: iqlhip_online_prio_kernels.h, the code object's last).
#include "iqlhip_online_prio_kernels.h"

static WUpd weights_upd(const iqlhip_weights* t) {
  return WUpd{t->tab, t->stamp, t->flags, (unsigned)t->n, t->levels, t->sh0, t->sat_bits};
}
static int weights_track_init(iqlhip_weights* t, unsigned max_bits, float new_row_weight, hipStream_t st) {
  HIPCHK(t->own.dev(&t->q_max, sizeof(unsigned long long), 0));
  hipLaunchKernelGGL(iql_wt_qmax_init_kernel, dim3(1), dim3(64), 0, st, max_bits, new_row_weight, t->sh0, t->sat_bits, t->q_max);
  return IQLHIP_OK;
}
static void launch_update_delta_track(const long long* idx, const float* w, unsigned m, long long bound, const WUpd& u,
                                      unsigned long long* delta, unsigned long long* q_max, hipStream_t st) {
  hipLaunchKernelGGL(iql_wt_update_delta_track_kernel, dim3((m + 255u) / 256u), dim3(256), 0, st, idx, w, m, bound, u, delta, q_max);
}
static void launch_update_delta_td_track(const long long* idx, const float* td, unsigned m, long long bound, const WUpd& u,
                                         unsigned long long* delta, const PrioArgs& a, unsigned long long* q_max, hipStream_t st) {
  hipLaunchKernelGGL(iql_wt_update_delta_td_track_kernel, dim3((m + 255u) / 256u), dim3(256), 0, st, idx, td, m, bound, u, delta, a,
                     q_max);
}

extern "C" int iqlhip_weights_max(const iqlhip_weights* t, uint64_t* q_max, float* w_max) {
  if (!t) return fail(IQLHIP_EINVAL, "NULL argument");
  if (!t->q_max) return fail(IQLHIP_EINVAL, "the table does not track its maximum (iqlhip_weights_build_tracking)");
  DevGuard guard(t->device);
  HIPCHK(hipDeviceSynchronize());         // an update may be queued on any stream
  unsigned long long q = 0;
  HIPCHK(hipMemcpy(&q, t->q_max, sizeof q, hipMemcpyDeviceToHost));
  if (q_max) *q_max = q;
  if (w_max) *w_max = (float)std::ldexp((double)q, -t->sh0);      // q = floor(w * 2^sh0): exact in a double (q < 2^39)
  return IQLHIP_OK;
}

extern "C" int iqlhip_weights_insert_max(iqlhip_weights* t, int64_t row, int64_t bound, void* stream) {
  if (!t) return fail(IQLHIP_EINVAL, "NULL argument");
  if (!t->q_max) return fail(IQLHIP_EINVAL, "the table does not track its maximum (iqlhip_weights_build_tracking)");
  if (bound < 0 || bound > t->n) return fail(IQLHIP_EINVAL, "bound = %lld outside [0, %lld]", (long long)bound, (long long)t->n);
  if (row < 0 || row >= bound) return fail(IQLHIP_EINVAL, "row = %lld outside [0, %lld)", (long long)row, (long long)bound);
  DevGuard guard(t->device);
  hipLaunchKernelGGL(iql_wt_insert_max_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, weights_upd(t),
                     (const unsigned long long*)t->q_max, (unsigned)row);
  HIPCHK(hipGetLastError());
  ++t->version;
  return IQLHIP_OK;
}

// The launches of iqlhip_online_step_prioritized in front of the step (online_step_front): the ring write with the insert,
// the draw with the gather, and the batch's loss weights — iqlhip_draw_indices_weighted_is's second kernel on the staged
// q, in place.  Indices: prio_buf's first staging half; c: is_buf's c region; TD errors: prio_buf's.
static void online_prio_gather(iqlhip_ctx* c, float* rows_dev, int64_t ld, int64_t pointer, int32_t n, const OnlinePrio& pr,
                               hipStream_t st, RowWeights* rw) {
  const iqlhip_weights* t = pr.table;
  float* cw = c->is_buf + 2 * (size_t)c->dims.max_batch;
  hipLaunchKernelGGL(iql_online_ring_insert_kernel, dim3(1), dim3(256), 0, st, rows_dev, (long long)ld, (long long)pointer,
                     (const float*)c->on_row_pin, weights_upd(t), (const unsigned long long*)t->q_max);
  hipLaunchKernelGGL(iql_online_draw_gather_kernel, dim3((unsigned)(n + 7) / 8u), dim3(256), 0, st, (const float*)rows_dev,
                     (long long)ld, c->xb, cw, prio_idx(c, 0), (int)n, weights_tab(t), (unsigned long long)pr.seed,
                     (unsigned long long)pr.offset);
  hipLaunchKernelGGL(iql_is_weights_kernel, dim3(1), dim3(256), 0, st, cw, (long long)n, (long long)n, pr.is_beta);
  *rw = RowWeights{cw, prio_td(c)};
}
// ... and behind it: iqlhip_weights_update_td's launches on the staged indices and the step's TD errors.
static void online_prio_update(iqlhip_ctx* c, int32_t n, const OnlinePrio& pr, hipStream_t st) {
  const iqlhip_weights* t = pr.table;
  const PrioArgs a{nullptr, pr.alpha, pr.eps};
  launch_update_td(weights_upd(t), prio_idx(c, 0), prio_td(c), (unsigned)n, (long long)t->n, t->delta, a, st, t->q_max);
}

extern "C" int iqlhip_online_step_prioritized(iqlhip_ctx* c, float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer,
                                              const float* row_host, int32_t n, const iqlhip_step_scalars* sc, float out[3],
                                              const float* act_state_host, float max_action, uint64_t act_seed,
                                              float* act_out_host, void* stream, iqlhip_weights* table, uint64_t seed,
                                              uint64_t stream_offset, float is_beta, float alpha, float eps) {
  if (!c || !table) return fail(IQLHIP_EINVAL, "NULL argument");
  if (!table->local) return fail(IQLHIP_EINVAL, "the table is not updatable (iqlhip_weights_build_tracking)");
  if (!table->q_max) return fail(IQLHIP_EINVAL, "the table does not track its maximum (iqlhip_weights_build_tracking)");
  if (table->device != c->device) return fail(IQLHIP_EINVAL, "the table lives on device %d, the context on %d", table->device, c->device);
  if (capacity != table->n) return fail(IQLHIP_EINVAL, "capacity %lld, but the table weighs %lld rows", (long long)capacity, (long long)table->n);
  if (int rc = prio_exponents_check(alpha, eps)) return rc;
  if (!(is_beta >= 0.f) || !std::isfinite(is_beta)) return fail(IQLHIP_EINVAL, "is_beta must be finite and >= 0");
  if (c->precision == 1) return fail(IQLHIP_EUNSUPPORTED, "per-row loss weights are not supported at bf16 precision");
  if (c->xch_mode != IQLHIP_XCH_NONE)
    return fail(IQLHIP_EUNSUPPORTED, "the prioritised online step is not supported with a data-parallel exchange");
  if (n > WT_UPDATE_SLICE) return fail(IQLHIP_EUNSUPPORTED, "prioritised calls take batches of at most %d rows", WT_UPDATE_SLICE);
  if (int rc = inject_check(c)) return rc;
  {                                       // the staging buffers of the prioritised calls (prio_setup's)
    DevGuard guard(c->device);
    if (!c->is_buf) HIPCHK(c->own.dev(&c->is_buf, (3 * (size_t)c->dims.max_batch + 4) * sizeof(float), 0));
    if (!c->prio_buf) HIPCHK(c->own.dev(&c->prio_buf, 24 * (size_t)c->dims.max_batch + 4 * sizeof(float), 0));
  }
  const OnlinePrio pr{table, seed, stream_offset, is_beta, alpha, eps};
  const int rc = online_step(c, rows_dev, ld, capacity, pointer, row_host, nullptr, n, sc, out, act_state_host, max_action, act_seed,
                             act_out_host, stream, nullptr, 0, nullptr, 0, &pr);
  if (!rc) table->version += 2;           // the insert and the update: what the two eager calls add
  return rc;
}

// The batch of the context's last prioritised online step, copied on `stream`: its n drawn indices and its rows' TD errors
// ([n][2]); either pointer may be null.
extern "C" int iqlhip_online_prioritized_batch(iqlhip_ctx* c, int32_t n, int64_t* idx_out_dev, float* td_out_dev, void* stream) {
  if (!c) return fail(IQLHIP_EINVAL, "NULL argument");
  if (!c->prio_buf) return fail(IQLHIP_EINVAL, "no prioritised step has run on this context");
  if (n < 1 || n > c->dims.max_batch) return fail(IQLHIP_EINVAL, "n outside [1, max_batch]");
  DevGuard guard(c->device);
  if (idx_out_dev)
    HIPCHK(hipMemcpyAsync(idx_out_dev, prio_idx(c, 0), (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (td_out_dev)
    HIPCHK(hipMemcpyAsync(td_out_dev, prio_td(c), (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return IQLHIP_OK;
}

// ---------------------------------------------------------------------------
// The JSRL variance learner's gradient step (include/iqlhip.h "the JSRL variance learner"; kernels:
// iqlhip_variance_kernels.h, the code object's last).  A handle of its own: two scalar nets in one arena, scratch sized
// by max_rows, nothing shared with a context.  A step is four launches: forward, row kernel, backward, Adam.
#include "iqlhip_variance_kernels.h"

struct iqlhip_var {
  int S = 0, max_rows = 0, device = 0;
  iqlhip_net_layout L[2];
  int64_t n_params = 0;
  Owned own;
  float *params = nullptr, *m = nullptr, *v = nullptr;      // bound (caller-owned)
  float *h0 = nullptr, *h1 = nullptr, *dh0 = nullptr;       // [VAR_LD][256]
  float *out = nullptr;                                     // [2][VAR_LD] head outputs
  float *dy = nullptr;                                      // [VAR_LD]
  float *grad = nullptr;                                    // the stepped net's gradient (the longer segment's words)
  float *land = nullptr;                                    // pinned, host-mapped: [4] loss | [3][VAR_LD] samp, pred, var
  // windows of a replay buffer (iqlhip_var_train_steps, iqlhip_var_values_window): taken on first use
  float *wblk = nullptr;                                    // the packed block of the current update
  float *wvals = nullptr;                                   // [3][VAR_LD] samp, pred, var of a burst's updates (not read back)
  float *loss_ring = nullptr;                               // pinned, host-mapped: [IQLHIP_VAR_TRAIN_MAX_STEPS] losses
  long long *start_ring = nullptr;                          // pinned, host-mapped: [IQLHIP_VAR_TRAIN_MAX_STEPS] start rows
};

static int var_check_dim(int32_t S) {
  if (S < 1) return fail(IQLHIP_EINVAL, "state_dim must be >= 1");
  if (S + 1 > IQLHIP_MAX_INPUT) return fail(IQLHIP_EUNSUPPORTED, "state_dim > %d", IQLHIP_MAX_INPUT - 1);
  return IQLHIP_OK;
}

extern "C" int iqlhip_var_layout(int32_t state_dim, iqlhip_net_layout out[2], int64_t* n_params) {
  if (int rc = var_check_dim(state_dim)) return rc;
  if (!out || !n_params) return fail(IQLHIP_EINVAL, "NULL argument");
  // the per-net rule of iqlhip_arena_layout at k_in = S, d_out = 1: a V net's segment, twice
  iqlhip_dims d{state_dim, 1, IQLHIP_HIDDEN, 2, IQLHIP_POLICY_DETERMINISTIC, 1};
  iqlhip_layout L;
  if (int rc = iqlhip_arena_layout(&d, &L)) return rc;
  const iqlhip_net_layout& v = L.net[IQLHIP_NET_V];
  const int64_t seg = v.seg_end - v.seg_begin;
  for (int k = 0; k < 2; ++k) {
    const int64_t sh = k * seg - v.seg_begin;
    out[k] = v;
    out[k].seg_begin += sh; out[k].seg_end += sh;
    out[k].w0 += sh; out[k].b0 += sh; out[k].w1 += sh; out[k].b1 += sh; out[k].w2 += sh; out[k].b2 += sh;
    out[k].log_std = -1;
  }
  *n_params = 2 * seg;
  return IQLHIP_OK;
}

extern "C" int iqlhip_var_destroy(iqlhip_var* s) {
  if (!s) return IQLHIP_OK;
  {
    DevGuard guard(s->device);
    (void)hipDeviceSynchronize();
    s->own.release_all();
  }
  delete s;
  return IQLHIP_OK;
}

extern "C" int iqlhip_var_create(int32_t state_dim, int32_t max_rows, int device, iqlhip_var** out) {
  if (!out) return fail(IQLHIP_EINVAL, "out is NULL");
  *out = nullptr;
  if (int rc = var_check_dim(state_dim)) return rc;
  if (max_rows < 1 || max_rows > VAR_MAX_ROWS) return fail(IQLHIP_EINVAL, "max_rows must be in [1,%d]", VAR_MAX_ROWS);
  int n_dev = 0;
  HIPCHK(hipGetDeviceCount(&n_dev));
  if (device < 0 || device >= n_dev) return fail(IQLHIP_EINVAL, "device %d out of range (%d devices)", device, n_dev);
  std::unique_ptr<iqlhip_var> s(new iqlhip_var);
  s->S = state_dim; s->max_rows = max_rows; s->device = device;
  if (int rc = iqlhip_var_layout(state_dim, s->L, &s->n_params)) return rc;
  DevGuard guard(device);
  auto dalloc = [&](float** p, size_t nfloat) { return s->own.dev(p, nfloat * sizeof(float), 0); };
  HIPCHK(dalloc(&s->h0, (size_t)VAR_LD * HID));
  HIPCHK(dalloc(&s->h1, (size_t)VAR_LD * HID));
  HIPCHK(dalloc(&s->dh0, (size_t)VAR_LD * HID));
  HIPCHK(dalloc(&s->out, (size_t)2 * VAR_LD));
  HIPCHK(dalloc(&s->dy, (size_t)VAR_LD));
  HIPCHK(dalloc(&s->grad, (size_t)(s->L[0].seg_end - s->L[0].seg_begin)));
  HIPCHK(s->own.pin(&s->land, (size_t)(4 + 3 * VAR_LD) * sizeof(float), /*zero=*/true));
  *out = s.release();
  return IQLHIP_OK;
}

extern "C" int iqlhip_var_bind(iqlhip_var* s, float* params, float* exp_avg, float* exp_avg_sq) {
  if (!s || !params || !exp_avg || !exp_avg_sq) return fail(IQLHIP_EINVAL, "NULL argument");
  if (((uintptr_t)params | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return fail(IQLHIP_EINVAL, "arenas must be 16-byte aligned");
  s->params = params; s->m = exp_avg; s->v = exp_avg_sq;
  return IQLHIP_OK;
}

static NetPtrs var_net_ptrs(const iqlhip_var* s, int k) {
  const iqlhip_net_layout& l = s->L[k];
  const float* p = s->params;
  return NetPtrs{p + l.w0, p + l.b0, p + l.w1, p + l.b1, p + l.w2, p + l.b2, s->S, 1};
}

static int var_check_call(const iqlhip_var* s, const float* batch_dev, int32_t B, int32_t which, bool need_net, int32_t aligned) {
  if (!s || !batch_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (!s->params) return fail(IQLHIP_ENOTBOUND, "iqlhip_var_bind has not been called");
  if (B < 1 || B > s->max_rows) return fail(IQLHIP_EINVAL, "B = %d outside [1, max_rows = %d]", B, s->max_rows);
  if (need_net && which != 0 && which != 1) return fail(IQLHIP_EINVAL, "which_net must be 0 (mf) or 1 (vf), got %d", which);
  if (aligned != 0 && aligned != 1) return fail(IQLHIP_EINVAL, "aligned_rewards must be 0 or 1, got %d", aligned);
  if ((uintptr_t)batch_dev & 3) return fail(IQLHIP_EINVAL, "the packed block must be 4-byte aligned");
  return IQLHIP_OK;
}

// The three launches' arguments (the solo launches pass them by value, a learner group writes them into its records).
// vals / loss: where the row kernel leaves samp | pred | var and the loss; null: the handle's host-mapped landing words
static VarFwdParams var_fwd_params(const iqlhip_var* s, const float* batch_dev, int B, int which) {
  VarFwdParams f{};
  f.net[0] = var_net_ptrs(s, 0); f.net[1] = var_net_ptrs(s, 1);
  f.x = batch_dev; f.S = s->S; f.rows0 = B + 1; f.rows1 = B; f.keep = which;
  f.h0 = s->h0; f.h1 = s->h1; f.out = s->out;
  return f;
}
static VarRowParams var_row_params(const iqlhip_var* s, const float* batch_dev, int B, int which, int aligned, float* vals2,
                                   float* vals, float* loss) {
  VarRowParams r{};
  r.out = s->out; r.rew = batch_dev + (size_t)(B + 1) * s->S; r.nd = r.rew + B; r.B = B; r.which = which; r.aligned = aligned;
  r.vals = vals ? vals : s->land + 4; r.vals2 = vals2; r.dy = s->dy; r.loss = loss ? loss : s->land;
  return r;
}
static VarBwdParams var_bwd_params(const iqlhip_var* s, const float* batch_dev, int B, int which) {
  const iqlhip_net_layout& l = s->L[which];
  VarBwdParams b{};
  b.np = var_net_ptrs(s, which); b.x = batch_dev; b.S = s->S; b.n = which == 0 ? B + 1 : B;
  b.h0 = s->h0; b.h1 = s->h1; b.dy = s->dy; b.dh0 = s->dh0; b.grad = s->grad;
  const int64_t sb = l.seg_begin;
  b.g_w1 = (unsigned)(l.w1 - sb); b.g_w0 = (unsigned)(l.w0 - sb); b.g_b0 = (unsigned)(l.b0 - sb);
  b.g_b1 = (unsigned)(l.b1 - sb); b.g_w2 = (unsigned)(l.w2 - sb); b.g_b2 = (unsigned)(l.b2 - sb);
  return b;
}

// forward + row kernel (which = -1: values only), then the backward of `which` into s->grad
static void var_launch(iqlhip_var* s, const float* batch_dev, int B, int which, int aligned, float* vals2, hipStream_t st,
                       float* vals = nullptr, float* loss = nullptr) {
  const VarFwdParams f = var_fwd_params(s, batch_dev, B, which);
  hipLaunchKernelGGL(iql_var_fwd_kernel<>, dim3((unsigned)(B + 1 + 31) / 32u, 2), dim3(256), 0, st, f);
  const VarRowParams r = var_row_params(s, batch_dev, B, which, aligned, vals2, vals, loss);
  hipLaunchKernelGGL(iql_var_row_kernel<>, dim3(1), dim3(256), 0, st, r);
  if (which < 0) return;
  const VarBwdParams b = var_bwd_params(s, batch_dev, B, which);
  hipLaunchKernelGGL(iql_var_bwd_kernel<>, dim3(VAR_BWD_BLOCKS), dim3(256), 0, st, b);
}

static void var_launch_adam(iqlhip_var* s, int which, const iqlhip_var_scalars* sc, hipStream_t st) {
  const iqlhip_net_layout& l = s->L[which];
  const int n = (int)(l.seg_end - l.seg_begin);
  hipLaunchKernelGGL(iql_var_adam_kernel<>, dim3((unsigned)(n + 255) / 256u), dim3(256), 0, st, s->params + l.seg_begin,
                     s->m + l.seg_begin, s->v + l.seg_begin, (const float*)s->grad, n, -sc->step_size, sc->bc2_sqrt,
                     sc->one_minus_beta1, sc->beta2, sc->one_minus_beta2, sc->eps);
}

extern "C" int iqlhip_var_step(iqlhip_var* s, const float* batch_dev, int32_t B, int32_t which_net, const iqlhip_var_scalars* sc,
                               void* stream) {
  if (!sc) return fail(IQLHIP_EINVAL, "NULL argument");
  if (int rc = var_check_call(s, batch_dev, B, which_net, true, sc->aligned_rewards)) return rc;
  DevGuard guard(s->device);
  hipStream_t st = (hipStream_t)stream;
  var_launch(s, batch_dev, B, which_net, sc->aligned_rewards, nullptr, st);
  var_launch_adam(s, which_net, sc, st);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

extern "C" int iqlhip_var_values(iqlhip_var* s, const float* batch_dev, int32_t B, int32_t aligned_rewards, float* out_dev,
                                 void* stream) {
  if (int rc = var_check_call(s, batch_dev, B, -1, false, aligned_rewards)) return rc;
  if (!out_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  DevGuard guard(s->device);
  var_launch(s, batch_dev, B, -1, aligned_rewards, out_dev, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

extern "C" int iqlhip_var_forward_backward(iqlhip_var* s, const float* batch_dev, int32_t B, int32_t which_net,
                                           int32_t aligned_rewards, float* grad_out_dev, void* stream) {
  if (int rc = var_check_call(s, batch_dev, B, which_net, true, aligned_rewards)) return rc;
  if (!grad_out_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  DevGuard guard(s->device);
  hipStream_t st = (hipStream_t)stream;
  var_launch(s, batch_dev, B, which_net, aligned_rewards, nullptr, st);
  HIPCHK(hipGetLastError());
  const iqlhip_net_layout& l = s->L[which_net];
  HIPCHK(hipMemcpyAsync(grad_out_dev, s->grad, (size_t)(l.seg_end - l.seg_begin) * sizeof(float), hipMemcpyDeviceToDevice, st));
  return IQLHIP_OK;
}

extern "C" int iqlhip_var_read_loss(iqlhip_var* s, float* loss, float* head, int32_t n_head, void* stream) {
  if (!s || !loss) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n_head < 0 || n_head > s->max_rows) return fail(IQLHIP_EINVAL, "n_head outside [0, max_rows]");
  DevGuard guard(s->device);
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  *loss = s->land[0];
  if (head)
    for (int k = 0; k < 3; ++k) memcpy(head + (size_t)k * n_head, s->land + 4 + (size_t)k * VAR_LD, (size_t)n_head * sizeof(float));
  return IQLHIP_OK;
}

// ---- windows of a packed replay buffer (include/iqlhip.h "from a replay buffer") ----
static int var_window_scratch(iqlhip_var* s) {
  if (s->wblk) return IQLHIP_OK;
  return all_or_nothing(s->own, [&]() -> int {
    HIPCHK(s->own.dev(&s->wblk, ((size_t)s->max_rows * s->S + s->S + 2 * (size_t)s->max_rows) * sizeof(float), 0));
    HIPCHK(s->own.dev(&s->wvals, (size_t)3 * VAR_LD * sizeof(float), 0));
    HIPCHK(s->own.pin(&s->loss_ring, (size_t)IQLHIP_VAR_TRAIN_MAX_STEPS * sizeof(float), /*zero=*/true));
    HIPCHK(s->own.pin(&s->start_ring, (size_t)IQLHIP_VAR_TRAIN_MAX_STEPS * sizeof(long long), /*zero=*/true));
    return IQLHIP_OK;
  });
}

// What every window call checks, before a launch and before anything is allocated.
static int var_check_window(const iqlhip_var* s, const float* rows_dev, int64_t ld, int64_t size, int32_t state_dim,
                            int32_t action_dim, int32_t B) {
  if (!s || !rows_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (state_dim != s->S) return fail(IQLHIP_EINVAL, "state_dim = %d, the handle's is %d", state_dim, s->S);
  if (action_dim < 1) return fail(IQLHIP_EINVAL, "action_dim must be >= 1");
  if (B < 1 || B > s->max_rows) return fail(IQLHIP_EINVAL, "B = %d outside [1, max_rows = %d]", B, s->max_rows);
  if (size < B) return fail(IQLHIP_EINVAL, "the buffer holds %lld rows, a window takes B = %d", (long long)size, B);
  if (ld < iqlhip_row_stride(state_dim, action_dim))
    return fail(IQLHIP_EINVAL, "ld = %lld below iqlhip_row_stride = %lld", (long long)ld, (long long)iqlhip_row_stride(state_dim, action_dim));
  if ((uintptr_t)rows_dev & 3) return fail(IQLHIP_EINVAL, "rows must be 4-byte aligned");
  return IQLHIP_OK;
}

static VarPackParams var_pack_params(const iqlhip_var* s, const float* rows_dev, int64_t ld, int64_t size, int32_t action_dim,
                                     int32_t B, float* out) {
  VarPackParams p{};
  p.rows = rows_dev; p.ld = ld; p.last_start = size - B; p.S = s->S; p.A = action_dim; p.B = B; p.out = out;
  return p;
}
static unsigned var_pack_blocks(int S, int B) { return (unsigned)((B + 1) * (S + 2) + 255) / 256u; }

extern "C" int iqlhip_var_pack_window(iqlhip_var* s, const float* rows_dev, int64_t ld, int64_t n_rows, int32_t state_dim,
                                      int32_t action_dim, int64_t start, int32_t B, float* block_out_dev, void* stream) {
  if (int rc = var_check_window(s, rows_dev, ld, n_rows, state_dim, action_dim, B)) return rc;
  if (!block_out_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (start < 0 || start > n_rows - B) return fail(IQLHIP_EINVAL, "rows %lld .. %lld outside the buffer's %lld", (long long)start,
                                                   (long long)start + B - 1, (long long)n_rows);
  if ((uintptr_t)block_out_dev & 3) return fail(IQLHIP_EINVAL, "the packed block must be 4-byte aligned");
  DevGuard guard(s->device);
  VarPackParams p = var_pack_params(s, rows_dev, ld, n_rows, action_dim, B, block_out_dev);
  p.start = start;
  hipLaunchKernelGGL(iql_var_pack_window_kernel<false>, dim3(var_pack_blocks(s->S, B)), dim3(256), 0, (hipStream_t)stream, p);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

extern "C" int iqlhip_var_values_window(iqlhip_var* s, const float* rows_dev, int64_t ld, int64_t n_rows, int32_t state_dim,
                                        int32_t action_dim, int64_t start, int32_t B, int32_t aligned_rewards, float* out_dev,
                                        void* stream) {
  if (int rc = var_check_window(s, rows_dev, ld, n_rows, state_dim, action_dim, B)) return rc;
  if (start < 0 || start > n_rows - B) return fail(IQLHIP_EINVAL, "rows %lld .. %lld outside the buffer's %lld", (long long)start,
                                                   (long long)start + B - 1, (long long)n_rows);
  if (int rc = var_check_call(s, rows_dev, B, -1, false, aligned_rewards)) return rc;
  if (!out_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  DevGuard guard(s->device);
  if (int rc = var_window_scratch(s)) return rc;
  VarPackParams p = var_pack_params(s, rows_dev, ld, n_rows, action_dim, B, s->wblk);
  p.start = start;
  hipLaunchKernelGGL(iql_var_pack_window_kernel<false>, dim3(var_pack_blocks(s->S, B)), dim3(256), 0, (hipStream_t)stream, p);
  var_launch(s, s->wblk, B, -1, aligned_rewards, out_dev, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

extern "C" int iqlhip_var_train_steps(iqlhip_var* s, const float* rows_dev, int64_t ld, int64_t size, int32_t action_dim, int32_t B,
                                      int32_t n_steps, int32_t which_net, const iqlhip_var_scalars* scalars, uint64_t seed,
                                      uint64_t stream_offset, const int64_t* starts_dev, int64_t n_starts, void* stream) {
  if (!s || !scalars) return fail(IQLHIP_EINVAL, "NULL argument");
  if (int rc = var_check_window(s, rows_dev, ld, size, s->S, action_dim, B)) return rc;
  if (n_steps < 1 || n_steps > IQLHIP_VAR_TRAIN_MAX_STEPS)
    return fail(IQLHIP_EINVAL, "n_steps = %d outside [1, %d]", n_steps, IQLHIP_VAR_TRAIN_MAX_STEPS);
  if (starts_dev && n_starts < 1) return fail(IQLHIP_EINVAL, "a starts list needs n_starts >= 1, got %lld", (long long)n_starts);
  if ((uintptr_t)starts_dev & 7) return fail(IQLHIP_EINVAL, "the starts list must be 8-byte aligned");
  for (int k = 0; k < n_steps; ++k)
    if (scalars[k].aligned_rewards != scalars[0].aligned_rewards) return fail(IQLHIP_EINVAL, "aligned_rewards differs inside a call");
  if (int rc = var_check_call(s, rows_dev, B, which_net, true, scalars[0].aligned_rewards)) return rc;
  DevGuard guard(s->device);
  if (int rc = var_window_scratch(s)) return rc;
  hipStream_t st = (hipStream_t)stream;
  VarPackParams p = var_pack_params(s, rows_dev, ld, size, action_dim, B, s->wblk);
  p.seed = seed;
  p.span = starts_dev ? (unsigned long long)n_starts : (unsigned long long)(size - B + 1);
  p.starts = (const long long*)starts_dev;
  const unsigned blocks = var_pack_blocks(s->S, B);
  for (int k = 0; k < n_steps; ++k) {
    p.j = stream_offset + (uint64_t)k;
    p.start_out = s->start_ring + k;
    hipLaunchKernelGGL(iql_var_pack_window_kernel<true>, dim3(blocks), dim3(256), 0, st, p);
    var_launch(s, s->wblk, B, which_net, scalars[k].aligned_rewards, nullptr, st, s->wvals, s->loss_ring + k);
    var_launch_adam(s, which_net, &scalars[k], st);
  }
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

extern "C" int iqlhip_var_read_train_ring(iqlhip_var* s, float* losses_out, int64_t* starts_out, int32_t n_steps, void* stream) {
  if (!s || !losses_out || !starts_out) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n_steps < 1 || n_steps > IQLHIP_VAR_TRAIN_MAX_STEPS)
    return fail(IQLHIP_EINVAL, "n_steps = %d outside [1, %d]", n_steps, IQLHIP_VAR_TRAIN_MAX_STEPS);
  if (!s->loss_ring) return fail(IQLHIP_EINVAL, "iqlhip_var_train_steps has not been called");
  DevGuard guard(s->device);
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  memcpy(losses_out, s->loss_ring, (size_t)n_steps * sizeof(float));
  memcpy(starts_out, s->start_ring, (size_t)n_steps * sizeof(int64_t));
  return IQLHIP_OK;
}

// ---------------------------------------------------------------------------
// Groups of variance learners (include/iqlhip.h "groups of variance learners"; DESIGN.md 6l "Groups of learners";
// kernels: iqlhip_variance_group_kernels.h, behind the solo kernels in the code object).  K bound iqlhip_var handles of
// one state_dim on one device, every launch of an update covering all of them.  The group owns the record table, the
// scalar table behind it (one staging, ONE host-to-device copy per call) and the K loss / start rings; a member keeps
// its arenas, its scratch and its landing words, and stays a solo handle.  Records are written anew by every call from
// what the members hold then, so nothing a solo call does in between can make them stale.
#include "iqlhip_variance_group_kernels.h"

struct iqlhip_var_group {
  int k = 0, device = 0, S = 0;
  iqlhip_var* m[IQLHIP_MAX_GROUP] = {};
  Owned own;
  Staging stg;
  Section<VarGroupRec> recs; Section<iqlhip_var_scalars> tab;      // tab [IQLHIP_VAR_TRAIN_MAX_STEPS][k], the staging's last
  float* loss_ring = nullptr;         // pinned, host-mapped [k][IQLHIP_VAR_TRAIN_MAX_STEPS]
  long long* start_ring = nullptr;
};

extern "C" int iqlhip_var_group_destroy(iqlhip_var_group* g) {
  if (!g) return IQLHIP_OK;
  {
    DevGuard guard(g->device);
    (void)hipDeviceSynchronize();
    g->own.release_all();
  }
  delete g;
  return IQLHIP_OK;
}

extern "C" int iqlhip_var_group_create(iqlhip_var* const* members, int k, iqlhip_var_group** out) {
  if (!out) return fail(IQLHIP_EINVAL, "out is NULL");
  *out = nullptr;
  if (!members) return fail(IQLHIP_EINVAL, "NULL argument");
  if (k < 1 || k > IQLHIP_MAX_GROUP) return fail(IQLHIP_EINVAL, "k = %d outside [1, %d]", k, IQLHIP_MAX_GROUP);
  for (int i = 0; i < k; ++i) {
    if (!members[i]) return fail(IQLHIP_EINVAL, "member %d: NULL handle", i);
    for (int j = 0; j < i; ++j)
      if (members[j] == members[i]) return fail(IQLHIP_EINVAL, "member %d: the handle is member %d too", i, j);
    if (members[i]->S != members[0]->S)
      return fail(IQLHIP_EINVAL, "member %d: state_dim = %d, member 0's is %d", i, members[i]->S, members[0]->S);
    if (members[i]->device != members[0]->device)
      return fail(IQLHIP_EINVAL, "member %d: device %d, member 0's is %d", i, members[i]->device, members[0]->device);
  }
  std::unique_ptr<iqlhip_var_group> g(new iqlhip_var_group);
  g->k = k; g->device = members[0]->device; g->S = members[0]->S;
  for (int i = 0; i < k; ++i) g->m[i] = members[i];
  DevGuard guard(g->device);
  g->recs = g->stg.add<VarGroupRec>(k);
  g->tab = g->stg.add<iqlhip_var_scalars>((size_t)k * IQLHIP_VAR_TRAIN_MAX_STEPS);
  HIPCHK(g->stg.alloc(g->own));
  HIPCHK(g->own.pin(&g->loss_ring, (size_t)k * IQLHIP_VAR_TRAIN_MAX_STEPS * sizeof(float), /*zero=*/true));
  HIPCHK(g->own.pin(&g->start_ring, (size_t)k * IQLHIP_VAR_TRAIN_MAX_STEPS * sizeof(long long), /*zero=*/true));
  *out = g.release();
  return IQLHIP_OK;
}

// What a call asks of every member's window, with the solo calls' checks and messages (start: null for a burst).
struct VarGroupWin { const float* const* rows; const int64_t* ld; const int64_t* size; const int32_t* action_dim; const int64_t* start; };
static int var_group_check_windows(const iqlhip_var_group* g, const VarGroupWin& w, int32_t B) {
  if (!g || !w.rows || !w.ld || !w.size || !w.action_dim) return fail(IQLHIP_EINVAL, "NULL argument");
  for (int i = 0; i < g->k; ++i) {
    if (int rc = var_check_window(g->m[i], w.rows[i], w.ld[i], w.size[i], g->S, w.action_dim[i], B)) return member_fail(i, rc);
    if (!g->m[i]->params) return fail(IQLHIP_ENOTBOUND, "member %d: iqlhip_var_bind has not been called", i);
    if (w.start && (w.start[i] < 0 || w.start[i] > w.size[i] - B))
      return fail(IQLHIP_EINVAL, "member %d: rows %lld .. %lld outside the buffer's %lld", i, (long long)w.start[i],
                  (long long)w.start[i] + B - 1, (long long)w.size[i]);
  }
  return IQLHIP_OK;
}
static int var_group_check_blocks(const iqlhip_var_group* g, const float* const* blocks_dev, int32_t B, int32_t which, bool need_net,
                                  const int32_t* aligned, int64_t aligned_stride) {
  if (!g || !blocks_dev || !aligned) return fail(IQLHIP_EINVAL, "NULL argument");
  for (int i = 0; i < g->k; ++i)
    if (int rc = var_check_call(g->m[i], blocks_dev[i], B, which, need_net, aligned[i * aligned_stride])) return member_fail(i, rc);
  return IQLHIP_OK;
}
static int var_group_window_scratch(iqlhip_var_group* g) {
  for (int i = 0; i < g->k; ++i)
    if (int rc = var_window_scratch(g->m[i])) return member_fail(i, rc);
  return IQLHIP_OK;
}

// Member i's record of a call: the solo launches' arguments on its block.
static void var_group_record(iqlhip_var_group* g, int i, const float* blk, int B, int which, int aligned, float* vals2, float* vals,
                             float* loss) {
  iqlhip_var* s = g->m[i];
  VarGroupRec& r = g->stg.host(g->recs)[i];
  memset(&r, 0, sizeof r);
  r.f = var_fwd_params(s, blk, B, which);
  r.r = var_row_params(s, blk, B, which, aligned, vals2, vals, loss);
  if (which < 0) return;
  r.b = var_bwd_params(s, blk, B, which);
  const iqlhip_net_layout& l = s->L[which];
  r.pw = s->params + l.seg_begin; r.m = s->m + l.seg_begin; r.v = s->v + l.seg_begin;
  r.n_adam = (int)(l.seg_end - l.seg_begin);
}
// ... and of its window: into the member's packed-block scratch, or `out`
static void var_group_record_pack(iqlhip_var_group* g, int i, const VarGroupWin& w, int B, float* out) {
  VarPackParams& p = g->stg.host(g->recs)[i].pk;
  p = var_pack_params(g->m[i], w.rows[i], w.ld[i], w.size[i], w.action_dim[i], B, out);
  if (w.start) p.start = w.start[i];
}
// the records and the first n_steps rows of the scalar table, in one copy (n_steps == 0: the records only)
static hipError_t var_group_upload(iqlhip_var_group* g, int n_steps, hipStream_t st) {
  const size_t bytes = n_steps ? g->tab.off + (size_t)n_steps * g->k * sizeof(iqlhip_var_scalars) : (size_t)g->k * sizeof(VarGroupRec);
  return g->stg.upload(bytes, st);
}

enum VarGroupPack { VG_NO_PACK, VG_PACK_AT, VG_PACK_DRAWN };
// One update's launches for all members: [pack,] forward, recurrence[, backward, Adam with row `step` of the table].
static void var_group_launch(const iqlhip_var_group* g, int B, int which, int step, VarGroupPack pack, hipStream_t st) {
  const int K = g->k, G = (K + 7) / 8;
  const VarGroupRec* recs = g->stg.device(g->recs);
  if (pack == VG_PACK_AT)
    hipLaunchKernelGGL(iql_var_pack_window_group_kernel<false>, dim3(var_group_grid(K, var_pack_blocks(g->S, B))), dim3(256), 0, st,
                       recs, K, G, step);
  else if (pack == VG_PACK_DRAWN)
    hipLaunchKernelGGL(iql_var_pack_window_group_kernel<true>, dim3(var_group_grid(K, var_pack_blocks(g->S, B))), dim3(256), 0, st,
                       recs, K, G, step);
  hipLaunchKernelGGL(iql_var_fwd_group_kernel<>, dim3(var_group_grid(K, 2u * ((unsigned)(B + 1 + 31) / 32u))), dim3(256), 0, st, recs, K, G);
  hipLaunchKernelGGL(iql_var_row_group_kernel<>, dim3(var_group_grid(K, 1)), dim3(256), 0, st, recs, K, G, step);
  if (which < 0) return;
  hipLaunchKernelGGL(iql_var_bwd_group_kernel<>, dim3(var_group_grid(K, VAR_BWD_BLOCKS)), dim3(256), 0, st, recs, K, G);
  const iqlhip_net_layout& l = g->m[0]->L[which];      // (one state_dim: every member's segment has these words)
  const unsigned nb = (unsigned)((l.seg_end - l.seg_begin + 255) / 256);
  hipLaunchKernelGGL(iql_var_adam_group_kernel<>, dim3(var_group_grid(K, nb)), dim3(256), 0, st, recs, g->stg.device(g->tab), K, G, step);
}

// The eager forms: blocks_dev null = every member's window (packed by the first launch into its scratch, or into
// blocks_out), else K packed blocks.  which = -1: values only.
static int var_group_eager(iqlhip_var_group* g, const float* const* blocks_dev, const VarGroupWin* w, int32_t B, int32_t which,
                           const iqlhip_var_scalars* scalars, const int32_t* aligned, float* const* outs_dev, void* stream) {
  DevGuard guard(g->device);
  if (w)
    if (int rc = var_group_window_scratch(g)) return rc;
  HIPCHK(g->stg.wait_free());
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < g->k; ++i) {
    const float* blk = w ? g->m[i]->wblk : blocks_dev[i];
    var_group_record(g, i, blk, B, which, scalars ? scalars[i].aligned_rewards : aligned[i], outs_dev ? outs_dev[i] : nullptr, nullptr,
                     nullptr);
    if (w) var_group_record_pack(g, i, *w, B, g->m[i]->wblk);
    if (scalars) g->stg.host(g->tab)[i] = scalars[i];
  }
  HIPCHK(var_group_upload(g, scalars ? 1 : 0, st));
  var_group_launch(g, B, which, 0, w ? VG_PACK_AT : VG_NO_PACK, st);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

extern "C" int iqlhip_var_group_step(iqlhip_var_group* g, const float* const* blocks_dev, int32_t B, int32_t which_net,
                                     const iqlhip_var_scalars* scalars, void* stream) {
  if (!g || !scalars) return fail(IQLHIP_EINVAL, "NULL argument");
  if (int rc = var_group_check_blocks(g, blocks_dev, B, which_net, true, &scalars[0].aligned_rewards,
                                      sizeof(iqlhip_var_scalars) / sizeof(int32_t)))
    return rc;
  return var_group_eager(g, blocks_dev, nullptr, B, which_net, scalars, nullptr, nullptr, stream);
}

extern "C" int iqlhip_var_group_values(iqlhip_var_group* g, const float* const* blocks_dev, int32_t B, const int32_t* aligned_rewards,
                                       float* const* outs_dev, void* stream) {
  if (!g || !outs_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (int rc = var_group_check_blocks(g, blocks_dev, B, -1, false, aligned_rewards, 1)) return rc;
  for (int i = 0; i < g->k; ++i)
    if (!outs_dev[i]) return fail(IQLHIP_EINVAL, "member %d: NULL argument", i);
  return var_group_eager(g, blocks_dev, nullptr, B, -1, nullptr, aligned_rewards, outs_dev, stream);
}

extern "C" int iqlhip_var_group_pack_windows(iqlhip_var_group* g, const float* const* rows_dev, const int64_t* ld, const int64_t* size,
                                             const int32_t* action_dim, const int64_t* start, int32_t B, float* const* blocks_out_dev,
                                             void* stream) {
  if (!start || !blocks_out_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  const VarGroupWin w{rows_dev, ld, size, action_dim, start};
  if (int rc = var_group_check_windows(g, w, B)) return rc;
  for (int i = 0; i < g->k; ++i) {
    if (!blocks_out_dev[i]) return fail(IQLHIP_EINVAL, "member %d: NULL argument", i);
    if ((uintptr_t)blocks_out_dev[i] & 3) return fail(IQLHIP_EINVAL, "member %d: the packed block must be 4-byte aligned", i);
  }
  DevGuard guard(g->device);
  HIPCHK(g->stg.wait_free());
  for (int i = 0; i < g->k; ++i) {
    memset(&g->stg.host(g->recs)[i], 0, sizeof(VarGroupRec));
    var_group_record_pack(g, i, w, B, blocks_out_dev[i]);
  }
  HIPCHK(var_group_upload(g, 0, (hipStream_t)stream));
  hipLaunchKernelGGL(iql_var_pack_window_group_kernel<false>, dim3(var_group_grid(g->k, var_pack_blocks(g->S, B))), dim3(256), 0,
                     (hipStream_t)stream, g->stg.device(g->recs), g->k, (g->k + 7) / 8, 0);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

extern "C" int iqlhip_var_group_step_windows(iqlhip_var_group* g, const float* const* rows_dev, const int64_t* ld, const int64_t* size,
                                             const int32_t* action_dim, const int64_t* start, int32_t B, int32_t which_net,
                                             const iqlhip_var_scalars* scalars, void* stream) {
  if (!start || !scalars) return fail(IQLHIP_EINVAL, "NULL argument");
  const VarGroupWin w{rows_dev, ld, size, action_dim, start};
  if (int rc = var_group_check_windows(g, w, B)) return rc;
  if (int rc = var_group_check_blocks(g, rows_dev, B, which_net, true, &scalars[0].aligned_rewards,
                                      sizeof(iqlhip_var_scalars) / sizeof(int32_t)))
    return rc;
  return var_group_eager(g, nullptr, &w, B, which_net, scalars, nullptr, nullptr, stream);
}

extern "C" int iqlhip_var_group_values_windows(iqlhip_var_group* g, const float* const* rows_dev, const int64_t* ld,
                                               const int64_t* size, const int32_t* action_dim, const int64_t* start, int32_t B,
                                               const int32_t* aligned_rewards, float* const* outs_dev, void* stream) {
  if (!start || !outs_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  const VarGroupWin w{rows_dev, ld, size, action_dim, start};
  if (int rc = var_group_check_windows(g, w, B)) return rc;
  if (int rc = var_group_check_blocks(g, rows_dev, B, -1, false, aligned_rewards, 1)) return rc;
  for (int i = 0; i < g->k; ++i)
    if (!outs_dev[i]) return fail(IQLHIP_EINVAL, "member %d: NULL argument", i);
  return var_group_eager(g, nullptr, &w, B, -1, nullptr, aligned_rewards, outs_dev, stream);
}

extern "C" int iqlhip_var_group_read_loss(iqlhip_var_group* g, float* losses, float* heads, int32_t n_head, void* stream) {
  if (!g || !losses) return fail(IQLHIP_EINVAL, "NULL argument");
  for (int i = 0; i < g->k; ++i)
    if (n_head < 0 || n_head > g->m[i]->max_rows) return fail(IQLHIP_EINVAL, "member %d: n_head outside [0, max_rows]", i);
  DevGuard guard(g->device);
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  for (int i = 0; i < g->k; ++i) {
    losses[i] = g->m[i]->land[0];
    if (heads)
      for (int k = 0; k < 3; ++k)
        memcpy(heads + ((size_t)i * 3 + k) * n_head, g->m[i]->land + 4 + (size_t)k * VAR_LD, (size_t)n_head * sizeof(float));
  }
  return IQLHIP_OK;
}

extern "C" int iqlhip_var_group_train_steps(iqlhip_var_group* g, const float* const* rows_dev, const int64_t* ld, const int64_t* size,
                                            const int32_t* action_dim, int32_t B, int32_t n_steps, int32_t which_net,
                                            const iqlhip_var_scalars* scalars, const uint64_t* seeds, const uint64_t* stream_offsets,
                                            const int64_t* const* starts_dev, const int64_t* n_starts, void* stream) {
  if (!scalars || !seeds || !stream_offsets || !starts_dev || !n_starts) return fail(IQLHIP_EINVAL, "NULL argument");
  const VarGroupWin w{rows_dev, ld, size, action_dim, nullptr};
  if (int rc = var_group_check_windows(g, w, B)) return rc;
  if (n_steps < 1 || n_steps > IQLHIP_VAR_TRAIN_MAX_STEPS)
    return fail(IQLHIP_EINVAL, "n_steps = %d outside [1, %d]", n_steps, IQLHIP_VAR_TRAIN_MAX_STEPS);
  const int K = g->k;
  for (int i = 0; i < K; ++i) {
    if (starts_dev[i] && n_starts[i] < 1)
      return fail(IQLHIP_EINVAL, "member %d: a starts list needs n_starts >= 1, got %lld", i, (long long)n_starts[i]);
    if ((uintptr_t)starts_dev[i] & 7) return fail(IQLHIP_EINVAL, "member %d: the starts list must be 8-byte aligned", i);
    for (int s = 0; s < n_steps; ++s)
      if (scalars[(size_t)s * K + i].aligned_rewards != scalars[i].aligned_rewards)
        return fail(IQLHIP_EINVAL, "member %d: aligned_rewards differs inside a call", i);
  }
  if (int rc = var_group_check_blocks(g, rows_dev, B, which_net, true, &scalars[0].aligned_rewards,
                                      sizeof(iqlhip_var_scalars) / sizeof(int32_t)))
    return rc;
  DevGuard guard(g->device);
  if (int rc = var_group_window_scratch(g)) return rc;
  HIPCHK(g->stg.wait_free());
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < K; ++i) {
    iqlhip_var* s = g->m[i];
    var_group_record(g, i, s->wblk, B, which_net, scalars[i].aligned_rewards, nullptr, s->wvals,
                     g->loss_ring + (size_t)i * IQLHIP_VAR_TRAIN_MAX_STEPS);
    var_group_record_pack(g, i, w, B, s->wblk);
    VarPackParams& p = g->stg.host(g->recs)[i].pk;
    p.seed = seeds[i];
    p.j = stream_offsets[i];
    p.span = starts_dev[i] ? (unsigned long long)n_starts[i] : (unsigned long long)(size[i] - B + 1);
    p.starts = (const long long*)starts_dev[i];
    p.start_out = g->start_ring + (size_t)i * IQLHIP_VAR_TRAIN_MAX_STEPS;
  }
  memcpy(g->stg.host(g->tab), scalars, (size_t)n_steps * K * sizeof(iqlhip_var_scalars));
  HIPCHK(var_group_upload(g, n_steps, st));
  for (int s = 0; s < n_steps; ++s) var_group_launch(g, B, which_net, s, VG_PACK_DRAWN, st);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

extern "C" int iqlhip_var_group_read_train_ring(iqlhip_var_group* g, float* losses_out, int64_t* starts_out, int32_t n_steps,
                                                void* stream) {
  if (!g || !losses_out || !starts_out) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n_steps < 1 || n_steps > IQLHIP_VAR_TRAIN_MAX_STEPS)
    return fail(IQLHIP_EINVAL, "n_steps = %d outside [1, %d]", n_steps, IQLHIP_VAR_TRAIN_MAX_STEPS);
  DevGuard guard(g->device);
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  for (int i = 0; i < g->k; ++i) {
    memcpy(losses_out + (size_t)i * n_steps, g->loss_ring + (size_t)i * IQLHIP_VAR_TRAIN_MAX_STEPS, (size_t)n_steps * sizeof(float));
    memcpy(starts_out + (size_t)i * n_steps, g->start_ring + (size_t)i * IQLHIP_VAR_TRAIN_MAX_STEPS, (size_t)n_steps * sizeof(int64_t));
  }
  return IQLHIP_OK;
}

// ---------------------------------------------------------------------------
// N-step rows (include/iqlhip.h "n-step rows"; kernels: iqlhip_nstep_kernels.h, the code object's
// last).  Nothing is allocated and nothing stays attached to a context: a build is one launch, a ring refresh one
// launch of at most four blocks.
#include "iqlhip_nstep_kernels.h"
static_assert(NS_MAX_HORIZON == IQLHIP_NSTEP_MAX_HORIZON, "kernel and header disagree on the largest horizon");

static int nstep_args_ok(int32_t horizon, double discount) {
  if (horizon < 1 || horizon > IQLHIP_NSTEP_MAX_HORIZON)
    return fail(IQLHIP_EINVAL, "horizon = %d outside [1, %d]", horizon, IQLHIP_NSTEP_MAX_HORIZON);
  if (!std::isfinite(discount) || !(discount > 0.0) || discount > 1.0)
    return fail(IQLHIP_EINVAL, "discount must be finite and in (0, 1]");
  return IQLHIP_OK;
}
static int nstep_store_ok(const float* src, int64_t src_ld, const float* dst, int64_t dst_ld, int32_t S, int32_t A, int64_t row0,
                          int64_t n, const char* who) {
  if (!dst) return fail(IQLHIP_EINVAL, "NULL argument");
  if (dst_ld < iqlhip_row_stride(S, A)) return fail(IQLHIP_EINVAL, "bad %s geometry", who);
  if ((src_ld & 3) || (dst_ld & 3)) return fail(IQLHIP_EINVAL, "row strides must be multiples of 4 floats");
  if ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) return fail(IQLHIP_EINVAL, "packed rows must be 16-byte aligned");
  if (src == dst) return fail(IQLHIP_EINVAL, "source and derived rows are the same buffer: n-step rows are not built in place");
  const uintptr_t s0 = (uintptr_t)(src + row0 * src_ld), s1 = (uintptr_t)(src + (row0 + n) * src_ld);
  const uintptr_t d0 = (uintptr_t)(dst + row0 * dst_ld), d1 = (uintptr_t)(dst + (row0 + n) * dst_ld);
  if (s0 < d1 && d0 < s1) return fail(IQLHIP_EINVAL, "source and derived rows overlap: n-step rows are not built in place");
  return IQLHIP_OK;
}
static NstepArgs nstep_kernel_args(const float* src, int64_t src_ld, float* dst, int64_t dst_ld, int32_t S, int32_t A,
                                   int32_t horizon, double discount, uint8_t* steps) {
  return NstepArgs{src, dst, (long long)src_ld, (long long)dst_ld, (int)S, (int)A, (int)(iqlhip_row_stride(S, A) / 4), (int)horizon,
                   (int)((horizon + NS_LANES - 1) / NS_LANES), discount, steps};
}

extern "C" int iqlhip_rows_nstep(const float* src_dev, int64_t src_ld, float* dst_dev, int64_t dst_ld, int32_t S, int32_t A,
                                 int64_t row0, int64_t n, int32_t horizon, double discount, const int64_t* ep_last_dev,
                                 uint8_t* steps_dev, void* stream) {
  int rc = reward_args_ok(src_dev, src_ld, S, A, row0, n, "rows_nstep");
  if (!rc) rc = nstep_store_ok(src_dev, src_ld, dst_dev, dst_ld, S, A, row0, n, "rows_nstep");
  if (!rc) rc = nstep_args_ok(horizon, discount);
  if (rc) return rc;
  if (((uintptr_t)ep_last_dev) & 7) return fail(IQLHIP_EINVAL, "ep_last must be 8-byte aligned");
  const long long rounds = ((long long)n + NS_ROWS_PER_BLOCK - 1) / NS_ROWS_PER_BLOCK;
  const dim3 grid((unsigned)std::min<long long>(rounds, NS_MAX_BLOCKS));
  const NstepArgs a = nstep_kernel_args(src_dev, src_ld, dst_dev, dst_ld, S, A, horizon, discount, steps_dev);
  if (ep_last_dev)
    hipLaunchKernelGGL(iql_nstep_build_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a, (long long)row0, (long long)n,
                       (const long long*)ep_last_dev);
  else
    hipLaunchKernelGGL(iql_nstep_build_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a, (long long)row0, (long long)n,
                       (const long long*)nullptr);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

static int nstep_ring_ok(const float* src, const float* dst, int64_t ld, int32_t S, int32_t A, int64_t capacity, int64_t size,
                         int64_t newest, const uint8_t* ends, int32_t horizon, double discount) {
  if (!src || !ends) return fail(IQLHIP_EINVAL, "NULL argument");
  if (S < 1 || A < 1 || ld < iqlhip_row_stride(S, A)) return fail(IQLHIP_EINVAL, "bad rows_nstep_ring geometry");
  if (capacity < 1 || size < 1 || size > capacity) return fail(IQLHIP_EINVAL, "ring size %lld outside [1, capacity=%lld]", (long long)size, (long long)capacity);
  if (newest < 0 || newest >= capacity) return fail(IQLHIP_EINVAL, "newest row outside the ring");
  if (size < capacity && newest >= size) return fail(IQLHIP_EINVAL, "newest row %lld beyond the %lld rows of a ring that has not wrapped", (long long)newest, (long long)size);
  int rc = nstep_store_ok(src, ld, dst, ld, S, A, 0, capacity, "rows_nstep_ring");
  if (!rc) rc = nstep_args_ok(horizon, discount);
  return rc;
}
static void launch_nstep_ring(const NstepArgs& a, int64_t capacity, int64_t size, int64_t newest, uint8_t* ends,
                              const float* newest_row, int newest_end, float* raw_out, hipStream_t st) {
  const int todo = (int)std::min<int64_t>(a.horizon, size);
  const dim3 grid((unsigned)(todo + NS_ROWS_PER_BLOCK - 1) / NS_ROWS_PER_BLOCK);
  if (newest_row)
    hipLaunchKernelGGL(iql_nstep_ring_kernel<true>, grid, dim3(256), 0, st, a, (long long)capacity, (long long)size,
                       (long long)newest, todo, ends, newest_row, newest_end, raw_out);
  else
    hipLaunchKernelGGL(iql_nstep_ring_kernel<false>, grid, dim3(256), 0, st, a, (long long)capacity, (long long)size,
                       (long long)newest, todo, ends, newest_row, newest_end, raw_out);
}

extern "C" int iqlhip_rows_nstep_ring(const float* src_dev, float* dst_dev, int64_t ld, int32_t S, int32_t A, int64_t capacity,
                                      int64_t size, int64_t newest, const uint8_t* ends_dev, int32_t horizon, double discount,
                                      uint8_t* steps_dev, void* stream) {
  const int rc = nstep_ring_ok(src_dev, dst_dev, ld, S, A, capacity, size, newest, ends_dev, horizon, discount);
  if (rc) return rc;
  launch_nstep_ring(nstep_kernel_args(src_dev, ld, dst_dev, ld, S, A, horizon, discount, steps_dev), capacity, size, newest,
                    const_cast<uint8_t*>(ends_dev), nullptr, 0, nullptr, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

// The launch of iqlhip_online_step_nstep in front of the step (online_step_front): ring write, end byte and refresh.
static void online_nstep_refresh(iqlhip_ctx* c, float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer,
                                 const OnlineNstep& ns, hipStream_t st) {
  launch_nstep_ring(nstep_kernel_args(ns.raw_dev, ld, rows_dev, ld, c->dims.state_dim, c->dims.action_dim, ns.horizon, ns.discount,
                                      ns.steps_dev),
                    capacity, ns.size_after, pointer, ns.ends_dev, (const float*)c->on_row_pin, ns.episode_end, ns.raw_dev, st);
}

extern "C" int iqlhip_online_step_nstep(iqlhip_ctx* c, float* raw_dev, float* rows_dev, int64_t ld, int64_t capacity,
                                        int64_t pointer, const float* row_host, const int64_t* idx_host, int32_t n,
                                        const iqlhip_step_scalars* sc, float out[3], const float* act_state_host,
                                        float max_action, uint64_t act_seed, float* act_out_host, void* stream,
                                        uint8_t* ends_dev, int32_t episode_end, int64_t size_after, int32_t horizon,
                                        double discount, uint8_t* steps_dev) {
  if (!c || !raw_dev || !rows_dev || !ends_dev) return fail(IQLHIP_EINVAL, "NULL argument");
  if (c->xch_mode != IQLHIP_XCH_NONE)
    return fail(IQLHIP_EUNSUPPORTED, "the n-step online step is not supported with a data-parallel exchange");
  const int rc = nstep_ring_ok(raw_dev, rows_dev, ld, c->dims.state_dim, c->dims.action_dim, capacity, size_after, pointer,
                               ends_dev, horizon, discount);
  if (rc) return rc;
  const OnlineNstep ns{raw_dev, ends_dev, steps_dev, size_after, horizon, episode_end, discount};
  return online_step(c, rows_dev, ld, capacity, pointer, row_host, idx_host, n, sc, out, act_state_host, max_action, act_seed,
                     act_out_host, stream, nullptr, 0, nullptr, 0, nullptr, &ns);
}

// ---------------------------------------------------------------------------
// The vector-environment online step (include/iqlhip.h "vector-environment online step"; kernel:
// iqlhip_online_vec_kernels.h, the code object's last): E ring writes, the batches of U steps gathered in the same
// launch, the U eager steps back to back and the act forward on E2 states, under one synchronisation.
#include "iqlhip_online_vec_kernels.h"
constexpr int VEC_MAX_BATCH = 512;      // rows per step: the small-batch kernels, fp32 or bf16
static_assert(VEC_MAX_BATCH == LB_MIN_ROWS, "the vector online step stays below the large-batch path");
static_assert(IQLHIP_VEC_MAX_UPDATES <= 1024, "the steps' statistics go to the first slots of the statistics ring");

// What the multi-row ring write asks of its arguments, with or without a context.
static int vec_ring_ok(const float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer, int32_t n_rows) {
  if (ld < 8 || (ld & 3)) return fail(IQLHIP_EINVAL, "row stride must be a multiple of 4 floats and at least 8");
  if (((uintptr_t)rows_dev) & 15) return fail(IQLHIP_EINVAL, "packed rows must be 16-byte aligned");
  if (capacity < 1 || pointer < 0 || pointer >= capacity) return fail(IQLHIP_EINVAL, "ring pointer outside the buffer");
  if (n_rows < 1 || n_rows > IQLHIP_VEC_MAX_ENVS || n_rows > capacity)
    return fail(IQLHIP_EINVAL, "%d new rows outside [1, min(capacity=%lld, %d)]", n_rows, (long long)capacity, IQLHIP_VEC_MAX_ENVS);
  return IQLHIP_OK;
}
static void launch_vec_gather(float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer, const float* rows_pin,
                              int32_t n_rows, const long long* idx_pin, float* xb, int n, hipStream_t st) {
  const int total = std::max((int)n_rows, n) * (int)(ld / 4);
  hipLaunchKernelGGL(iql_online_vec_gather_kernel, dim3((total + 255) / 256), dim3(256), 0, st, rows_dev, (long long)ld,
                     (long long)capacity, (long long)pointer, rows_pin, (int)n_rows, idx_pin, xb, n);
}

extern "C" int iqlhip_rows_write_ring(float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer, const float* rows_pin,
                                      int32_t n_rows, void* stream) {
  if (!rows_dev || !rows_pin) return fail(IQLHIP_EINVAL, "NULL argument");
  if (int rc = vec_ring_ok(rows_dev, ld, capacity, pointer, n_rows)) return rc;
  if (((uintptr_t)rows_pin) & 15) return fail(IQLHIP_EINVAL, "the new rows must be 16-byte aligned");
  launch_vec_gather(rows_dev, ld, capacity, pointer, rows_pin, n_rows, nullptr, nullptr, 0, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

// The call's buffers: the pinned blocks once, the device staging whenever a call needs more than there is.
static int vec_buffers(iqlhip_ctx* c, size_t stage_floats) {
  if (!c->vec_rows_pin) {
    const int rc = all_or_nothing(c->own, [&]() -> int {
      HIPCHK(c->own.pin(&c->vec_rows_pin, (size_t)IQLHIP_VEC_MAX_ENVS * c->row_ld * sizeof(float)));
      HIPCHK(c->own.pin(&c->vec_idx_pin, (size_t)IQLHIP_VEC_MAX_UPDATES * VEC_MAX_BATCH * sizeof(long long)));
      HIPCHK(c->own.pin(&c->vec_loss_pin, (size_t)IQLHIP_VEC_MAX_UPDATES * 4 * sizeof(float)));
      HIPCHK(c->own.pin(&c->vec_act_pin, (size_t)IQLHIP_VEC_MAX_ENVS * (IQLHIP_MAX_INPUT + IQLHIP_MAX_ACTION) * sizeof(float)));
      return IQLHIP_OK;
    });
    if (rc) return rc;
  }
  if (c->vec_xb_cap < stage_floats) {
    HIPCHK(hipDeviceSynchronize());          // (an earlier call's steps may still read the old block)
    c->vec_own.release_all();
    c->vec_xb_cap = 0;
    HIPCHK(c->vec_own.dev(&c->vec_xb, stage_floats * sizeof(float)));
    c->vec_xb_cap = stage_floats;
  }
  return IQLHIP_OK;
}

extern "C" int iqlhip_online_step_vec(iqlhip_ctx* c, float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer,
                                      const float* rows_host, int32_t n_rows, const int64_t* idx_host, int32_t batch_rows,
                                      int32_t n_updates, const iqlhip_step_scalars* sc, float* out,
                                      const float* act_states_host, int32_t act_rows, float max_action, uint64_t act_seed,
                                      float* act_out_host, void* stream) {
  if (!c || !rows_dev || !rows_host) return fail(IQLHIP_EINVAL, "NULL argument");
  if (n_updates > 0 && (!idx_host || !sc || !out)) return fail(IQLHIP_EINVAL, "NULL argument");
  if (act_states_host && !act_out_host) return fail(IQLHIP_EINVAL, "act_states_host without act_out_host");
  if (!c->params) return fail(IQLHIP_ENOTBOUND, "iqlhip_bind has not been called");
  if (ld != c->row_ld) return fail(IQLHIP_EINVAL, "row stride must be iqlhip_row_stride(S,A)=%lld", (long long)c->row_ld);
  if (int rc = vec_ring_ok(rows_dev, ld, capacity, pointer, n_rows)) return rc;
  const int U = n_updates, B = batch_rows;
  if (U < 0 || U > IQLHIP_VEC_MAX_UPDATES) return fail(IQLHIP_EINVAL, "n_updates = %d outside [0, %d]", U, IQLHIP_VEC_MAX_UPDATES);
  if (act_states_host && (act_rows < 1 || act_rows > IQLHIP_VEC_MAX_ENVS))
    return fail(IQLHIP_EINVAL, "act_rows = %d outside [1, %d]", act_rows, IQLHIP_VEC_MAX_ENVS);
  if (c->xch_mode != IQLHIP_XCH_NONE)
    return fail(IQLHIP_EUNSUPPORTED, "the vector online step is not supported with a data-parallel exchange");
  if (c->drop_inject)
    return fail(IQLHIP_EUNSUPPORTED, "keep-bits injected by iqlhip_debug_write_masks are pending: the vector online step draws "
                "every step's own (call iqlhip_set_dropout first, or step with iqlhip_step)");
  if (B >= 1 && use_lb(c, B))
    return fail(IQLHIP_EUNSUPPORTED, "the vector online step is not supported on the large-batch bf16 path (more than %d rows)", LB_MIN_ROWS);
  if (B < 1 || B > VEC_MAX_BATCH || B > c->dims.max_batch)
    return fail(IQLHIP_EINVAL, "batch rows %d outside [1, min(%d, max_batch=%d)]", B, VEC_MAX_BATCH, c->dims.max_batch);
  if (U > 0) {
    if (int rc = check_host_indices(idx_host, (int64_t)U * B, capacity)) return rc;
    if (int rc = step_entry(c, B, stream, /*multi_step=*/false)) return rc;
  }
  DevGuard guard(c->device);
  hipStream_t st = (hipStream_t)stream;
  const int S = c->dims.state_dim, A = c->dims.action_dim;
  if (int rc = vec_buffers(c, (size_t)std::max(U, 1) * B * (size_t)ld)) return rc;
  memcpy(c->vec_rows_pin, rows_host, (size_t)n_rows * ld * sizeof(float));
  if (U > 0) memcpy(c->vec_idx_pin, idx_host, (size_t)U * B * sizeof(long long));
  launch_vec_gather(rows_dev, ld, capacity, pointer, c->vec_rows_pin, n_rows, c->vec_idx_pin, c->vec_xb, U * B, st);
  const unsigned long long done_val = ++c->done_seq;
  for (int u = 0; u < U; ++u) {
    EagerStep e;
    eager_begin(c, B, sc + u, st, c->vec_xb + (size_t)u * B * ld, e);
    if (e.with_stats) e.sa = make_stats(c, e.p, c->stats_ring, u, c->k_max, nullptr);      // (and stats_last, as every step)
    e.u.losses_mirror = c->vec_loss_pin + 4 * u;
    if (u == U - 1 && !act_states_host) { e.u.done_flag = c->done_pin; e.u.done_val = done_val; }
    if (int rc = enqueue_step(c, e.p, e.u, IQLHIP_XCH_NONE, 0, 0, /*from_hdr=*/false, st, nullptr, e.stats())) return rc;
  }
  float* a_out = c->vec_act_pin + (size_t)IQLHIP_VEC_MAX_ENVS * IQLHIP_MAX_INPUT;
  if (act_states_host) {
    // the next iteration's actions by the policy the U steps left: states and actions travel through host-mapped pinned words
    memcpy(c->vec_act_pin, act_states_host, (size_t)act_rows * S * sizeof(float));
    const bool noisy = act_seed != 0 && c->dims.policy == IQLHIP_POLICY_GAUSSIAN;
    const bool one_block = act_rows * A <= 256;      // (the finish launch stores the completion word only when it is one block)
    const int rc = actor_forward_impl(c, c->vec_act_pin, S, act_rows, nullptr, 0, noisy ? act_seed : 0, noisy ? c->act_calls++ : 0,
                                      max_action, a_out, A, stream, one_block ? c->done_pin : nullptr, done_val);
    if (rc) return rc;
    if (!one_block) hipLaunchKernelGGL(iql_group_done_kernel, dim3(1), dim3(64), 0, st, c->done_pin, done_val);
  }
  // (a synchronous call: the pinned staging is free again on return)
  if (U > 0 || act_states_host) {
    if (int rc = wait_word(c->done_pin, done_val, st)) return rc;
  } else {
    HIPCHK(hipStreamSynchronize(st));
  }
  for (int u = 0; u < U; ++u)
    for (int k = 0; k < 3; ++k) out[3 * u + k] = c->vec_loss_pin[4 * u + k];
  if (act_states_host) memcpy(act_out_host, a_out, (size_t)act_rows * A * sizeof(float));
  HIPCHK(hipGetLastError());
  return IQLHIP_OK;
}

// ---------------------------------------------------------------------------
// The vector-environment online step of a trainer group (include/iqlhip.h "group vector-environment online step";
// DESIGN.md 6b; kernels: iqlhip_group_online_vec_kernels.h, the code object's last): iqlhip_online_step_vec for every
// member in one set of launches — one launch for all members' ring writes, gathers and act-state packing, n_updates
// times the group step launches on the slices of a group-owned staging block, the group inference launches over the
// requesting members' act_rows rows, and one completion word.
#include "iqlhip_group_online_vec_kernels.h"

// The call's buffers.  Once: the staging's layout and blocks and the pinned blocks; whenever a call needs more than
// there is: the device staging of the gathered batches.
static int group_vec_buffers(iqlhip_group* g, size_t stage_floats) {
  const size_t K = (size_t)g->k;
  if (g->vec.bytes == 0) {
    const size_t n_drop = (g->flags & IQLHIP_GROUP_DROPOUT) ? K : 0;
    Staging& s = g->vec;
    g->vec_gathers = s.add<GroupVecRec>(K);
    g->vec_adrops = s.add<ActDropRec>(n_drop);
    g->vec_aps = s.add<StepParams>(K);
    g->vec_fins = s.add<GroupActRowsRec>(K);
    g->vec_head = s.bytes;
    for (int u = 0; u < IQLHIP_VEC_MAX_UPDATES; ++u) {
      iqlhip_group::VecStep& v = g->vec_steps[u];
      v.recs = s.add<GroupRec>(K);
      v.drops = s.add<GroupDropRec>(n_drop);
      v.aux.add(s, K);
      v.tabs = s.add<iqlhip_step_scalars>(K);
      g->vec_end[u] = s.bytes;
    }
  }
  if (!g->vec_rows_pin) {
    const size_t ld = (size_t)g->m[0]->row_ld;
    const int rc = all_or_nothing(g->own, [&]() -> int {
      HIPCHK(g->vec.alloc(g->own, /*with_event=*/false));
      HIPCHK(g->own.pin(&g->vec_idx_pin, K * IQLHIP_VEC_MAX_UPDATES * VEC_MAX_BATCH * sizeof(long long)));
      HIPCHK(g->own.pin(&g->vec_loss_pin, K * IQLHIP_VEC_MAX_UPDATES * 4 * sizeof(float)));
      HIPCHK(g->own.pin(&g->vec_act_pin, K * IQLHIP_VEC_MAX_ENVS * (IQLHIP_MAX_INPUT + IQLHIP_MAX_ACTION) * sizeof(float)));
      HIPCHK(g->own.pin(&g->vec_rows_pin, K * IQLHIP_VEC_MAX_ENVS * ld * sizeof(float)));
      return IQLHIP_OK;
    });
    if (rc) return rc;
  }
  if (g->vec_xb_cap < stage_floats) {
    HIPCHK(hipDeviceSynchronize());          // (an earlier call's steps may still read the old block)
    g->vec_own.release_all();
    g->vec_xb_cap = 0;
    HIPCHK(g->vec_own.dev(&g->vec_xb, stage_floats * sizeof(float)));
    g->vec_xb_cap = stage_floats;
  }
  return IQLHIP_OK;
}

extern "C" int iqlhip_group_online_step_vec(iqlhip_group* g, float* const* rows_dev, int64_t ld, const int64_t* capacity,
                                            const int64_t* pointer, const float* rows_host, const int32_t* n_rows,
                                            const int64_t* idx_host, const int32_t* batch_rows, int32_t n_updates,
                                            const iqlhip_step_scalars* sc, float* out, const float* act_states_host,
                                            const int32_t* act_rows, const float* max_action, const uint64_t* act_seed,
                                            float* act_out_host, void* stream) {
  if (!g || !rows_dev || !capacity || !pointer || !rows_host || !n_rows || !batch_rows) return fail(IQLHIP_EINVAL, "NULL argument");
  const int U = n_updates;
  if (U < 0 || U > IQLHIP_VEC_MAX_UPDATES) return fail(IQLHIP_EINVAL, "n_updates = %d outside [0, %d]", U, IQLHIP_VEC_MAX_UPDATES);
  if (U > 0 && (!idx_host || !sc || !out)) return fail(IQLHIP_EINVAL, "NULL argument");
  if (act_states_host && (!act_rows || !max_action || !act_seed || !act_out_host))
    return fail(IQLHIP_EINVAL, "act_states_host without act_rows, max_action, act_seed or act_out_host");
  // (the warm-up takes no step: as the solo call with n_updates = 0, it asks what the steps' optional features need of
  //  no member — the members, their arenas and the batch size are checked all the same)
  int rc = U > 0 ? group_check_call(g, batch_rows) : group_check_members(g->m, g->k, g->flags);
  if (rc) return rc;
  const int K = g->k;
  for (int i = 0; i < K && U == 0; ++i) {
    if ((rc = group_check_bound(g, i))) return rc;
    if (batch_rows[i] < 1 || batch_rows[i] > g->m[i]->dims.max_batch)
      return fail(IQLHIP_EINVAL, "member %d: batch rows %d outside [1, max_batch=%d]", i, batch_rows[i], g->m[i]->dims.max_batch);
  }
  size_t idx0[IQLHIP_MAX_GROUP], row0[IQLHIP_MAX_GROUP], act0[IQLHIP_MAX_GROUP];      // where member i's indices, new rows and act rows start
  auto n_act = [&](int i) { return act_states_host ? (int)act_rows[i] : 0; };
  for (int i = 0; i < K; ++i) {
    const iqlhip_ctx* c = g->m[i];
    if (batch_rows[i] > VEC_MAX_BATCH)
      return fail(IQLHIP_EINVAL, "member %d: batch rows %d outside [1, %d]", i, batch_rows[i], VEC_MAX_BATCH);
    if (ld != c->row_ld) return fail(IQLHIP_EINVAL, "row stride must be iqlhip_row_stride(S,A)=%lld", (long long)c->row_ld);
    if (!rows_dev[i]) return fail(IQLHIP_EINVAL, "member %d: NULL ring", i);
    if (((uintptr_t)rows_dev[i]) & 15) return fail(IQLHIP_EINVAL, "member %d: packed rows must be 16-byte aligned", i);
    if (capacity[i] < 1 || pointer[i] < 0 || pointer[i] >= capacity[i])
      return fail(IQLHIP_EINVAL, "member %d: ring pointer outside the buffer", i);
    if (n_rows[i] < 1 || n_rows[i] > IQLHIP_VEC_MAX_ENVS || n_rows[i] > capacity[i])
      return fail(IQLHIP_EINVAL, "member %d: %d new rows outside [1, min(capacity=%lld, %d)]", i, n_rows[i],
                  (long long)capacity[i], IQLHIP_VEC_MAX_ENVS);
    if (n_act(i) < 0 || n_act(i) > IQLHIP_VEC_MAX_ENVS)
      return fail(IQLHIP_EINVAL, "member %d: act_rows = %d outside [0, %d]", i, n_act(i), IQLHIP_VEC_MAX_ENVS);
    if (c->drop_inject)
      return fail(IQLHIP_EUNSUPPORTED, "member %d: keep-bits injected by iqlhip_debug_write_masks are pending: the vector online "
                  "step draws every step's own (call iqlhip_set_dropout first)", i);
    for (int j = 0; j < i; ++j) {      // (two members writing one ring would race on its rows)
      const uintptr_t a0 = (uintptr_t)rows_dev[i], a1 = a0 + (uintptr_t)(capacity[i] * ld) * sizeof(float);
      const uintptr_t b0 = (uintptr_t)rows_dev[j], b1 = b0 + (uintptr_t)(capacity[j] * ld) * sizeof(float);
      if (a0 < b1 && b0 < a1) return fail(IQLHIP_EINVAL, "members %d and %d share ring rows (one buffer per member)", j, i);
    }
    idx0[i] = i ? idx0[i - 1] + (size_t)U * batch_rows[i - 1] : 0;
    row0[i] = i ? row0[i - 1] + (size_t)n_rows[i - 1] : 0;
    act0[i] = i ? act0[i - 1] + (size_t)n_act(i - 1) : 0;
  }
  for (int i = 0; i < K && U > 0; ++i)
    if ((rc = check_host_indices(idx_host + idx0[i], (int64_t)U * batch_rows[i], capacity[i]))) return rc;
  for (int i = 0; i < K; ++i) note_stream(g->m[i], stream);
  DevGuard guard(g->device);
  hipStream_t st = (hipStream_t)stream;
  const iqlhip_ctx* c0 = g->m[0];
  const int S = c0->dims.state_dim, A = c0->dims.action_dim;
  const bool gauss = c0->dims.policy == IQLHIP_POLICY_GAUSSIAN;
  size_t xb0[IQLHIP_MAX_GROUP], stage_floats = 0;      // where member i's slices start in the staging block
  for (int i = 0; i < K; ++i) {
    xb0[i] = stage_floats;
    stage_floats += (size_t)std::max(U, 1) * batch_rows[i] * (size_t)ld;
  }
  if ((rc = group_vec_buffers(g, stage_floats))) return rc;
  const GroupGeom q = group_geom(g, batch_rows);
  const Staging& vs = g->vec;
  GroupVecRec* gathers = vs.host(g->vec_gathers);
  StepParams* aps = vs.host(g->vec_aps);
  GroupActRowsRec* fins = vs.host(g->vec_fins);
  const bool with_drops = (g->flags & IQLHIP_GROUP_DROPOUT) != 0;
  ActDropRec* adrops = with_drops ? vs.host(g->vec_adrops) : nullptr;
  const size_t act_pin_k = (size_t)IQLHIP_VEC_MAX_ENVS * (IQLHIP_MAX_INPUT + IQLHIP_MAX_ACTION);
  auto act_out_pin = [&](int i) { return g->vec_act_pin + (size_t)i * act_pin_k + (size_t)IQLHIP_VEC_MAX_ENVS * IQLHIP_MAX_INPUT; };
  bool act_draws = false;
  int n_req = 0, max_act = 0, max_work = 0;
  for (int i = 0; i < K; ++i) {
    iqlhip_ctx* c = g->m[i];
    const int B = batch_rows[i], E = n_rows[i], E2 = n_act(i);
    float* rows_pin = g->vec_rows_pin + (size_t)i * IQLHIP_VEC_MAX_ENVS * ld;
    long long* idx_pin = g->vec_idx_pin + (size_t)i * IQLHIP_VEC_MAX_UPDATES * VEC_MAX_BATCH;
    float* act_pin = g->vec_act_pin + (size_t)i * act_pin_k;
    memcpy(rows_pin, rows_host + row0[i] * ld, (size_t)E * ld * sizeof(float));
    if (U > 0) memcpy(idx_pin, idx_host + idx0[i], (size_t)U * B * sizeof(long long));
    GroupVecRec& o = gathers[i];
    memset(&o, 0, sizeof o);
    o.rows = rows_dev[i]; o.rows_pin = rows_pin; o.idx_pin = idx_pin; o.xb = g->vec_xb + xb0[i];
    o.act_pin = E2 ? act_pin : nullptr; o.xb_act = c->xb_act;
    o.ld = ld; o.capacity = capacity[i]; o.pointer = pointer[i];
    o.n_new = E; o.n = U * B; o.act_rows = E2; o.S = S;
    max_work = std::max(max_work, std::max(std::max(E, U * B), E2));
    if (with_drops) adrops[i] = act_drop_record(c, E2);
    if (!E2) continue;
    memcpy(act_pin, act_states_host + act0[i] * S, (size_t)E2 * S * sizeof(float));
    aps[n_req] = act_step_params(c, E2);
    if (with_drops && adrops[i].active) act_draws = true;
    GroupActRowsRec& f = fins[n_req];
    const bool noise = act_seed[i] != 0 && gauss;      // (the call counter moves only when noise is drawn, as solo)
    f.heads = c->heads_act; f.log_std = aps[n_req].log_std; f.out = act_out_pin(i); f.ld_out = (long long)A; f.n = E2; f.A = A;
    f.max_action = max_action[i]; f.ls_min = c->hyper.log_std_min; f.ls_max = c->hyper.log_std_max;
    f.seed = noise ? act_seed[i] : 0ull;
    f.call = noise ? c->act_calls : 0ull;              // (the counters move behind the upload, below)
    max_act = std::max(max_act, E2);
    ++n_req;
  }
  // the steps' records: step u is a one-step group call on slice u of every member's staging, its scalars in the
  // block's own row, its losses and statistics in slot u of the members' rings and mirrors
  GroupAux aux[IQLHIP_VEC_MAX_UPDATES];
  int n_draw = 0;
  for (int u = 0; u < U; ++u) {
    const iqlhip_group::VecStep& v = g->vec_steps[u];
    GroupRec* recs = vs.host(v.recs);
    iqlhip_step_scalars* tab = vs.host(v.tabs);
    for (int i = 0; i < K; ++i) {
      const int B = batch_rows[i];
      tab[i] = sc[(size_t)i * U + u];
      group_record(g, recs[i], i, q, B, 1, g->vec_xb + xb0[i] + (size_t)u * B * ld, &tab[i], vs.device(v.tabs) + i);
      recs[i].u.ring_slot = u;
      recs[i].u.losses_mirror = g->vec_loss_pin + ((size_t)i * IQLHIP_VEC_MAX_UPDATES + u) * 4;
    }
    if ((rc = group_aux(g, vs, v.aux, recs, &aux[u]))) return rc;
    if (aux[u].srecs)
      for (int i = 0; i < K; ++i) vs.host(v.aux.srecs)[i].a.ring_slot = u;
    if (with_drops) {      // (the drawing members' records at the front, step u's draw at the member's position + u)
      GroupDropRec* d = vs.host(v.drops);
      n_draw = group_drop_records_packed(g, d, batch_rows);
      for (int j = 0; j < n_draw; ++j) d[j].step0 += (unsigned long long)u;
    }
  }
  // (a synchronous call: the previous one's upload has been read long ago)
  HIPCHK(g->vec.upload(U > 0 ? g->vec_end[U - 1] : g->vec_head, st));
  // nothing below returns before the launches are queued: only now do the members' counters move — the noise and the
  // inference keep-bit position of every requesting member by one call, and the staged rows of a solo continuation go
  for (int i = 0; i < K; ++i) {
    iqlhip_ctx* c = g->m[i];
    if (U > 0) c->cont.valid = false;      // (as after any group step: a later solo call gathers its own rows)
    if (!n_act(i)) continue;
    if (with_drops && adrops[i].active) c->act_drop_calls += 1;
    if (act_seed[i] != 0 && gauss) c->act_calls += 1;
  }
  const int gather_nb = (int)(((long long)max_work * (ld / 4) + 255) / 256);      // (the largest member's: a record bounds its own)
  if (act_draws)
    hipLaunchKernelGGL(iql_online_vec_gather_drop_group_kernel, dim3(gather_nb + (2 * max_act * 8 + 255) / 256, K), dim3(256), 0, st,
                       vs.device(g->vec_gathers), vs.device(g->vec_adrops));
  else
    hipLaunchKernelGGL(iql_online_vec_gather_group_kernel, dim3(gather_nb, K), dim3(256), 0, st, vs.device(g->vec_gathers));
  for (int i = 0; i < K; ++i)
    if (U > 0 || n_act(i)) refresh_shadows(g->m[i], st);
  for (int u = 0; u < U; ++u) {
    const iqlhip_group::VecStep& v = g->vec_steps[u];
    group_launch_dropmask(g, vs.device(v.drops), n_draw, q.max_rows, st);      // (every drawing member's position moves by one)
    group_launch_step(g, vs.device(v.recs), q, 0, st, aux[u]);
  }
  const unsigned long long done_val = ++g->done_seq;
  if (n_req > 0) {
    // (bf16: the last update has rewritten the shadows from the new masters — the conversion refresh_shadows makes)
    const int nbx = (max_act + RT_ROWS - 1) / RT_ROWS * NSPLIT;
    group_launch_act_fwd(c0, vs.device(g->vec_aps), nbx, n_req, fwd_lds(c0, nbx * n_req), st);
    hipLaunchKernelGGL(iql_actor_finish_rows_group_kernel, dim3((max_act * A + 255) / 256, n_req), dim3(256), 0, st,
                       vs.device(g->vec_fins));
  }
  // (the rows finish stores no completion word: the one-block launch behind it does)
  if (U > 0 || n_req > 0) hipLaunchKernelGGL(iql_group_done_kernel, dim3(1), dim3(64), 0, st, g->done_pin, done_val);
  HIPCHK(hipGetLastError());
  g->last_n = U;
  if (U > 0 || n_req > 0) {
    if ((rc = wait_word(g->done_pin, done_val, st))) return rc;
  } else {
    HIPCHK(hipStreamSynchronize(st));
  }
  for (int i = 0; i < K; ++i) {
    for (int u = 0; u < U; ++u)
      for (int j = 0; j < 3; ++j)
        out[((size_t)i * U + u) * 3 + j] = g->vec_loss_pin[((size_t)i * IQLHIP_VEC_MAX_UPDATES + u) * 4 + j];
    if (n_act(i)) memcpy(act_out_host + act0[i] * A, act_out_pin(i), (size_t)n_act(i) * A * sizeof(float));
  }
  return IQLHIP_OK;
}
