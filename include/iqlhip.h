/*
 * iqlhip.h — C ABI of libiqlhip.so: the MI355X (gfx950) implementation of the
 * IQL gradient step of LaurenYTaylor/jsrl-CORL.
 *
 * The reference has no FFI: its boundary is the Python class surface of
 * algorithms/finetune/iql.py (ReplayBuffer :122-197, ImplicitQLearning :445-606).
 * Each entry point below names the reference method whose device work it
 * replaces; jsrl-corl_amd/iql.py is the Python shim that keeps those classes'
 * signatures and calls these symbols through ctypes.  INTEGRATION.md shows the
 * binding a reference maintainer would add.
 *
 * Conventions
 *  - plain C types only; every pointer named *_dev is device memory owned by the
 *    CALLER (torch tensors in the shim); the library never frees it.
 *  - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *    all calls are asynchronous on it unless stated otherwise.
 *  - return 0 on success, negative IQLHIP_E* otherwise; iqlhip_last_error() gives
 *    the message (thread-local).  No C++ exception crosses the boundary.
 *  - a context is not thread-safe; one context per (process, GPU).
 *  - all arithmetic is fp32 ("f32" in bench.py's dtype); GEMMs run on
 *    v_mfma_f32_16x16x4_f32 (exact fp32 fma chains).
 */
#ifndef IQLHIP_H
#define IQLHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IQLHIP_VERSION 410          /* 0.4.1 */
#define IQLHIP_HIDDEN 256           /* hidden width the kernels are tiled for (reference default, iql.py:352) */
#define IQLHIP_MAX_INPUT 128        /* max state_dim + action_dim */
#define IQLHIP_MAX_ACTION 32        /* max action_dim */
#define IQLHIP_MAX_WORLD 8          /* ranks of one data-parallel group (the GPUs of one node) */
#define IQLHIP_GRAPH_STEPS 64       /* steps per captured hipGraph chunk of iqlhip_train_steps */
#define IQLHIP_N_SCORE 8            /* floats per row of iqlhip_score_rows: v, next_v, q1, q2, target_q, adv, exp_adv, bc */
#define IQLHIP_N_STATS 16           /* floats per step of the opt-in training statistics (iqlhip_set_step_stats) */

enum {
  IQLHIP_OK = 0,
  IQLHIP_EINVAL = -1,    /* bad argument (maps to ValueError in the shim) */
  IQLHIP_EHIP = -2,      /* a HIP runtime call failed (RuntimeError) */
  IQLHIP_ENOTBOUND = -3, /* step before iqlhip_bind */
  IQLHIP_EUNSUPPORTED = -4, /* dims the kernels are not built for (NotImplementedError) */
  IQLHIP_EINDEX = -5,    /* a row index outside the buffer (IndexError, like the reference's tensor indexing iql.py:173-177) */
  IQLHIP_EEXCHANGE = -6  /* a peer of the P2P gradient exchange did not arrive in time: replicas out of sync (RuntimeError) */
};

enum { IQLHIP_NET_V = 0, IQLHIP_NET_Q1 = 1, IQLHIP_NET_Q2 = 2, IQLHIP_NET_PI = 3 };
enum { IQLHIP_POLICY_GAUSSIAN = 0, IQLHIP_POLICY_DETERMINISTIC = 1 };

/* ---- dimensions -------------------------------------------------------- */
typedef struct {
  int32_t state_dim;     /* S */
  int32_t action_dim;    /* A */
  int32_t hidden_dim;    /* must be IQLHIP_HIDDEN */
  int32_t n_hidden;      /* must be 2 (MLP [in,256,256,out], iql.py:351-356) */
  int32_t policy;        /* IQLHIP_POLICY_* (GaussianPolicy :347 / DeterministicPolicy :382) */
  int32_t max_batch;     /* largest batch a step will be called with */
} iqlhip_dims;

/* Offsets (in floats) of one MLP's tensors inside the flat parameter arena.
 * Weights keep torch.nn.Linear's [out,in] row-major layout. */
typedef struct {
  int64_t seg_begin, seg_end;  /* [begin,end) of this net's segment, multiples of 64 */
  int64_t w0, b0, w1, b1, w2, b2, log_std;  /* log_std = -1 when absent */
  int32_t k_in;    /* input width of layer 0: S (V, pi) or S+A (Q) */
  int32_t d_out;   /* 1 (V, Q) or A (pi) */
} iqlhip_net_layout;

typedef struct {
  iqlhip_net_layout net[4];   /* IQLHIP_NET_* order: V, Q1, Q2, PI */
  int64_t n_params;           /* floats in the trainable arena (= Adam exp_avg / exp_avg_sq arenas) */
  int64_t n_target;           /* floats in the target arena: copy of the [Q1,Q2] segments */
  int64_t target_src;         /* arena offset of Q1's segment: target[i] mirrors params[target_src+i] */
} iqlhip_layout;

/* Pure host function (no GPU needed).  Replaces nothing in the reference: the
 * reference keeps one tensor per nn.Parameter; the shim re-homes them as views
 * into ONE arena laid out by this function so a step touches three flat buffers. */
int iqlhip_arena_layout(const iqlhip_dims* dims, iqlhip_layout* out);

/* ---- hyper-parameters and per-step scalars ------------------------------ */
typedef struct {
  float iql_tau;    /* expectile, ImplicitQLearning(iql_tau)  iql.py:454,490 */
  float beta;       /* inverse temperature                    iql.py:455,524 */
  float discount;   /* gamma                                  iql.py:457,506 */
  float tau;        /* Polyak rate, cast of the python float  iql.py:458,515 */
  float one_minus_tau; /* (float)(1.0 - tau) formed in float64 first (iql.py:74) */
  float exp_adv_max;   /* EXP_ADV_MAX = 100                   iql.py:26 */
  float log_std_min, log_std_max; /* -20, 2                  iql.py:27-28 */
} iqlhip_hyper;

/* Host-computed (float64 -> float32) scalars of torch.optim.Adam's
 * _single_tensor_adam for THIS step; group order V, Q, PI. */
typedef struct {
  float step_size[3];   /* lr_g / (1 - beta1^t_g) */
  float bc2_sqrt[3];    /* sqrt(1 - beta2^t_g) */
  float beta2;          /* (float)beta2 */
  float one_minus_beta1;/* (float)(1 - beta1) : lerp weight */
  float one_minus_beta2;/* (float)(1 - beta2) */
  float eps;
  float grad_scale;     /* 1 for single GPU; 1/world after a summed all-reduce */
  float inv_batch;      /* 1 / (rows the batch means divide by): 1/B, or 1/(B*world) under DP */
} iqlhip_step_scalars;

/* One batch, either gathered already (idx_dev == NULL; five separate row-major
 * tensors as returned by ReplayBuffer.sample, iql.py:171-178) or addressed
 * through int64 row indices into buffer storage (ld_* = row strides in floats). */
typedef struct {
  const float* s_dev; const float* a_dev; const float* r_dev; const float* ns_dev; const float* d_dev;
  int64_t ld_s, ld_a, ld_r, ld_ns, ld_d;
  const int64_t* idx_dev;
  int32_t rows;
} iqlhip_batch;

typedef struct iqlhip_ctx iqlhip_ctx;

/* ---- life cycle --------------------------------------------------------- */
int iqlhip_version(void);
const char* iqlhip_last_error(void);

/* ImplicitQLearning.__init__ (iql.py:446-480): allocates library-owned scratch
 * (activations, gradient slabs, loss words) on `device`. */
int iqlhip_create(const iqlhip_dims* dims, const iqlhip_hyper* hyper, int device, iqlhip_ctx** out);
int iqlhip_destroy(iqlhip_ctx* ctx);
int iqlhip_set_hyper(iqlhip_ctx* ctx, const iqlhip_hyper* hyper);

/* Arithmetic of the large matrix products (layer 0 and layer 1 forward, dW1, dH0, dW0): 0 = fp32 MFMA (default; the
 * parity path), 1 = operands rounded to bf16, fp32 accumulate (v_mfma_f32_16x16x32_bf16).  The heads, master weights,
 * activations in memory, losses, Adam and Polyak stay fp32.  The reference has no reduced-precision mode; this
 * is BASELINE config 5's "MFMA bf16 path" and is checked against the fp32 fixtures at 2e-2. */
int iqlhip_set_precision(iqlhip_ctx* ctx, int mode);

/* Actor dropout (GaussianPolicy/DeterministicPolicy(..., dropout=p) -> nn.Dropout(p) after each hidden ReLU,
 * iql.py:331-333, active while the actor is in train mode): p in [0,1), 0 = off.  Keep-masks are drawn on
 * the device (Philox4x32-10 keyed by `seed` and a per-step counter). */
int iqlhip_set_dropout(iqlhip_ctx* ctx, float p, uint64_t seed);
/* The context's Philox stream positions {dropout step, act() call}: read them from a context that is about to be
 * replaced and set them on its successor, so that neither random stream restarts mid-run. */
int iqlhip_get_counters(const iqlhip_ctx* ctx, uint64_t out[2]);
int iqlhip_set_counters(iqlhip_ctx* ctx, const uint64_t in[2]);
/* Actor dropout INSIDE policy inference (the online loop asks a training-mode actor for its next action, algorithms/
 * finetune/iql.py:725-738: the nn.Dropout layers are live): p in [0,1), 0 = off (the default: every inference entry
 * point then behaves and launches exactly as without this call).  Independent of iqlhip_set_dropout — the training
 * rate stays what it is.  With p > 0, iqlhip_actor_forward, iqlhip_actor_sample, the act forward of iqlhip_online_step,
 * and — member by member, each with its own rate, key and position — iqlhip_group_actor_forward and the act forward of
 * iqlhip_group_online_step draw the call's keep-bits on the device and run the policy forward with them (keep scale
 * 1.f / (1.f - p)).  A stream of its own: Philox4x32-10, key `seed`, counter words (w, j | 0x41445250 "ADRP", lo32 n,
 * hi32 n), j = 0..7, w = row * 16 + layer * 8 + q (rows restart at 0 with every library call), bit 4 j + t of the word
 * = (output t >= p * 2^32), bit b = hidden unit 32 q + b; n = the context's position, which moves by one with every
 * library inference call that draws (rate > 0, rows > 0, arguments accepted).  The bits live in a buffer of their own
 * (never the training steps'); allocated by the first call with p > 0. */
int iqlhip_set_act_dropout(iqlhip_ctx* ctx, float p, uint64_t seed);
/* That stream's position n (iqlhip_get_counters / iqlhip_set_counters keep their two words). */
int iqlhip_get_act_dropout_counter(const iqlhip_ctx* ctx, uint64_t* out);
int iqlhip_set_act_dropout_counter(iqlhip_ctx* ctx, uint64_t n);
/* Tests: inject keep-bits for the next steps instead of drawing them ([rows][8] uint32 per layer, bit j of
 * word w = hidden unit 32w + j); cleared by the next iqlhip_set_dropout.  The single-step entry points (iqlhip_step and
 * its forms, iqlhip_online_step, iqlhip_forward_backward) and the group calls use them.  iqlhip_train_steps and
 * iqlhip_train_steps_prepare cannot (their steps alternate between two keep-bit halves and draw the next step's bits as
 * they go): while injected masks are pending they return IQLHIP_EUNSUPPORTED before anything is launched or any
 * position moves. */
int iqlhip_debug_write_masks(iqlhip_ctx* ctx, const uint32_t* keep0_host, const uint32_t* keep1_host, int32_t rows,
                             void* stream);

/* Bind the caller-owned arenas: params (n_params), target (n_target; the
 * deepcopy q_target of iql.py:461), Adam exp_avg / exp_avg_sq (n_params each). */
int iqlhip_bind(iqlhip_ctx* ctx, float* params_dev, float* target_dev, float* exp_avg_dev, float* exp_avg_sq_dev);

/* ---- the step ----------------------------------------------------------- */
/* ImplicitQLearning.train(batch) (iql.py:542-563) minus the host syncs: forward
 * of V(s'), V(s), Qt1, Qt2, Q1, Q2, pi; the three losses; backward; Adam on the
 * three groups; Polyak.  Losses land in device words read by iqlhip_read_losses. */
int iqlhip_step(iqlhip_ctx* ctx, const iqlhip_batch* batch, const iqlhip_step_scalars* sc, void* stream);

/* iqlhip_step with per-row loss weights c = row_w_dev[0 .. rows) (fp32, device; importance-sampling correction of a
 * weighted or prioritised draw):
 *   value_loss = 1/B sum_r c_r |tau - 1(u_r < 0)| u_r^2     q_loss = 1/B sum_r c_r (e1_r^2 + e2_r^2) / 2
 *   actor_loss = 1/B sum_r c_r exp_adv_r bc_r
 * and every gradient follows from these.  A row-weighted variant of the fp32 backward forms them: each row's finished
 * unweighted terms are multiplied by c_r last, so weights of exactly 1.0f give iqlhip_step's bits.  The forward and the
 * update are iqlhip_step's; actor dropout, step statistics (unweighted definitions) and gradient clipping (norms of the
 * weighted gradient) apply as there.  td_out_dev: NULL, or [rows][2] fp32 (8-byte aligned) that receives the rows'
 * TD errors (q1 - y, q2 - y) — the pre-update values the loss used.  Asynchronous like iqlhip_step; the (weighted)
 * losses are read through iqlhip_read_losses.
 * IQLHIP_EINVAL: row_w_dev NULL.  IQLHIP_EUNSUPPORTED, before anything is launched or any counter moves: bf16 precision
 * (and with it the large-batch path), a data-parallel exchange attached.  The weights' VALUES are not inspected: NaN
 * or negative weights are the caller's business. */
int iqlhip_step_rw(iqlhip_ctx* ctx, const iqlhip_batch* batch, const iqlhip_step_scalars* sc, const float* row_w_dev,
                   float* td_out_dev, void* stream);

/* The same step WITH the host synchronisation train() ends on (the three .item() calls of iql.py:491,509,535 as one):
 * the losses land in host-mapped pinned words followed by a completion word the host spins on — no stream synchronise
 * (12-17 us of host time after the GPU has finished, profiles/r03_sync_cost.txt).  Returns when out[3] = {value, q, actor}
 * is there; the parameter update itself stays ordered by `stream` like after iqlhip_step. */
int iqlhip_step_sync(iqlhip_ctx* ctx, const iqlhip_batch* batch, const iqlhip_step_scalars* sc, float out[3], void* stream);
/* ... in two halves, for a host that has work to do while the GPU runs the step: begin launches, wait returns the
 * losses of the step begun last. */
int iqlhip_step_begin(iqlhip_ctx* ctx, const iqlhip_batch* batch, const iqlhip_step_scalars* sc, void* stream);
int iqlhip_step_wait(iqlhip_ctx* ctx, float out[3], void* stream);

/* One iteration of the online fine-tuning loop's device work (algorithms/finetune/iql.py:741-773, jsrl_w_iql.py:
 * 512-548: add_transition -> sample -> train) in one call: the new packed transition row_host[ld] is stored at ring
 * row `pointer` of rows_dev (capacity rows), the batch rows_dev[idx_host[0..n)] (indices as np.random.randint drew them,
 * AFTER the insert, iql.py:172) is gathered and one IQL step runs on it.  row_host / idx_host are ordinary host
 * memory (copied into pinned staging inside the call).  Synchronous: returns the three losses in out[3].
 * act_state_host != NULL additionally evaluates the NEXT iteration's actor.act(state) (iql.py:371-379) with the
 * just-updated policy before the call's one synchronisation: state_dim floats in, action_dim floats out
 * (act_out_host); act_seed != 0 draws the training-mode noise on the device like iqlhip_actor_sample. */
int iqlhip_online_step(iqlhip_ctx* ctx, float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer,
                       const float* row_host, const int64_t* idx_host, int32_t n, const iqlhip_step_scalars* sc,
                       float out[3], const float* act_state_host, float max_action, uint64_t act_seed,
                       float* act_out_host, void* stream);

/* ---- mixed offline / online batches -------------------------------------------------------------------------
 * The batch of an online fine-tuning step mixed from two buffers, as the reference's Cal-QL loop builds it
 * (algorithms/finetune/cal_ql.py: vstack(offline_buffer.sample(n_off), online_buffer.sample(n_on))): batch rows
 * [0, n_off) come from the offline buffer, rows [n_off, n_off + n) from the online ring.  1 <= n_off and 1 <= n; both
 * buffers have the same row stride and are different allocations.
 *
 * iqlhip_online_step_mixed: iqlhip_online_step's arguments and meaning — rows_dev / capacity / pointer / row_host are
 * the online ring and its new transition, idx_host[0..n) the online indices, drawn over the ring's size AFTER the insert
 * (an index equal to `pointer` reads the new row) — plus the offline part: rows_off_dev (size_off rows, read only) and
 * idx_off_host[0..n_off).  The host draws the offline indices FIRST, then the online ones (the order of the two
 * sample() calls).  Both arrays are range-checked on the host before anything is launched (IQLHIP_EINDEX; online
 * indices against `capacity`, offline ones against size_off).  One step on n_off + n <= max_batch rows; sc->inv_batch
 * is 1 / (n_off + n).  Bit for bit what add_transition, the two gathers, a concatenation and iqlhip_step give.
 * IQLHIP_EUNSUPPORTED with a data-parallel exchange attached and for bf16 batches of more than 512 rows, like
 * iqlhip_train_steps_mixed, before anything is launched. */
int iqlhip_online_step_mixed(iqlhip_ctx* ctx, float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer,
                             const float* row_host, const int64_t* idx_host, int32_t n, const iqlhip_step_scalars* sc,
                             float out[3], const float* act_state_host, float max_action, uint64_t act_seed,
                             float* act_out_host, void* stream, const float* rows_off_dev, int64_t size_off,
                             const int64_t* idx_off_host, int32_t n_off);

/* iqlhip_train_steps_mixed: iqlhip_train_steps with every step's batch mixed the same way.  The index stream is
 * iqlhip_train_steps' own — index j = k * batch_rows + r of the call (step k, batch row r) takes the 64 random bits of
 * counter stream_offset + j / 2, word pair j & 1, under `seed`, and a call consumes ceil(n_steps * batch_rows / 2)
 * counters whatever n_off is — and only the mapping depends on the row: r < n_off gives floor(bits * size_off / 2^64) into
 * rows_off_dev, r >= n_off gives floor(bits * size_on / 2^64) into rows_on_dev.  1 <= n_off <= batch_rows - 1.  Both sizes
 * are per-call values (device header words), so the online ring may grow between calls; the captured chunk graphs
 * depend on the two row pointers, batch_rows and n_off.  A mixed call neither continues a previous call's stream nor
 * leaves rows staged for the next one (there is no flags argument): the plain call that follows gathers its own step 0.
 * IQLHIP_EUNSUPPORTED with a data-parallel exchange attached, for bf16 batches of more than 512 rows, and with injected
 * keep-bits pending.  Losses and statistics come from the rings as after iqlhip_train_steps.
 * iqlhip_train_steps_mixed_prepare: iqlhip_train_steps_prepare for the chunk graphs of such calls. */
int iqlhip_train_steps_mixed(iqlhip_ctx* ctx, const float* rows_off_dev, int64_t size_off, const float* rows_on_dev,
                             int64_t size_on, int64_t ld, int32_t batch_rows, int32_t n_off,
                             const iqlhip_step_scalars* sc, int32_t n_steps, uint64_t seed, uint64_t stream_offset,
                             void* stream);
int iqlhip_train_steps_mixed_prepare(iqlhip_ctx* ctx, const float* rows_off_dev, const float* rows_on_dev, int64_t ld,
                                     int32_t batch_rows, int32_t n_off, float inv_batch, void* stream);

/* ---- weighted replay sampling ---------------------------------------------------------------------------------
 * Rows drawn by weight instead of uniformly, on the device, from the index stream of iqlhip_train_steps unchanged.
 * The distribution is defined in integers, so the device and a CPU restatement agree to the bit:
 *   w[0..n) float32, all finite, all >= 0, at least one > 0, 1 <= n <= IQLHIP_WEIGHTS_MAX_ROWS;
 *   e = floor(log2(max w)); q[i] = floor(w[i] * 2^(38 - e)) as uint64, taken from the fp32 bit pattern by shifts, so
 *   max q lies in [2^38, 2^39) and a weight below max w * 2^-39 becomes 0: such a row is never drawn;
 *   cum[i] = q[0] + ... + q[i]; total = cum[n - 1] < 2^63;
 *   index j of a call takes the 64 random bits r of counter stream_offset + j / 2, word pair j & 1, under `seed` — what
 *   iqlhip_draw_indices gives it — then t = mulhi64(r, total) and the index is the smallest i with cum[i] > t.
 * With all weights equal that is floor(r * n / 2^64): the plain stream bit for bit.
 *
 * iqlhip_weights_build: validates w_dev[0..n) (device memory) and builds the table — cum plus the 64-ary search levels
 * above it, 8 bytes per row plus 1/63 — in device memory of the current device; synchronises `stream`.  IQLHIP_EINVAL
 * for a NaN, an infinity, a negative weight, all zeros or n out of range; nothing is returned then, and any table built
 * before is untouched.  Every table gets a generation number no other table of the process has.
 * iqlhip_weights_free: waits for the device, then frees the table (NULL: nothing).
 * iqlhip_weights_info: n, total, the level count, the generation and — tests — a synchronous copy of cum[0..n) into
 * cum_host (each may be NULL). */
#define IQLHIP_WEIGHTS_MAX_ROWS (1 << 24)
typedef struct iqlhip_weights iqlhip_weights;
int iqlhip_weights_build(const float* w_dev, int64_t n, void* stream, iqlhip_weights** out);
int iqlhip_weights_free(iqlhip_weights* table);
int iqlhip_weights_info(const iqlhip_weights* table, int64_t* n, uint64_t* total, int32_t* levels, uint64_t* generation,
                        uint64_t* cum_host);
/* ---- updatable tables: weights changed in place ---------------------------------------------------------------
 * A second kind of table with the same 64-ary geometry (every level starts on a multiple of 64 entries, a node is one
 * aligned 512-byte read, at most 4 levels) and other contents: every node holds the inclusive prefix sums of its OWN 64
 * children's subtree totals — level-0 node k, entry l: q[64 k] + ... + q[64 k + l]; level l + 1, entry c of a node: the
 * totals of that node's children 0 .. c; the top level is one node, its last entry is `total`.  The descent subtracts
 * the chosen child's left neighbour from t at every level and so returns the smallest i with cum[i] > t, what a static
 * table returns: for equal q[] both kinds give the same index for every (seed, offset, j).  Every call that takes a
 * table takes either kind.  Changing q[i] touches one node per level.
 *
 * iqlhip_weights_build_updatable: a table over `capacity` rows (its n), 1 <= n <= capacity <= 2^24; rows n .. capacity
 * weigh 0.  The scale is fixed for the table's life: e = floor(log2(max(max_weight, max w))), q = floor(w * 2^(38 - e));
 * max_weight = 0 means the largest weight present, which gives the static table's q[].  Validation and errors as
 * iqlhip_weights_build; synchronises `stream`.  12 bytes per row plus 1/63 of 8 (the tree, and a 4-byte stamp per row).
 * iqlhip_weights_update: w[idx_dev[j]] = w_dev[j], j < m (int64 indices, float32 weights, device memory), queued on
 * `stream` with no read-back, in integers throughout:
 *   - q_new = floor(w * 2^(38 - e)) at the table's scale; a weight >= 2^(e + 1) saturates to 2^39 - 1;
 *   - a NaN, an infinity, a negative weight (-0.0 is zero) or an index outside [0, bound), bound <= n, is skipped — its
 *     row stays as it was — and leaves a bit in the table's sticky flag word: 1 non-finite, 2 negative, 4 index;
 *   - of several valid entries for one row the one at the largest position j wins;
 *   - afterwards every entry of the tree equals what a fresh build over the changed weights at the same scale holds
 *     (integer adds commute: exact in any order).  total may reach 0: draws then stay inside [0, n) and mean nothing.
 * An update is ordered on its stream against draws and steps queued there; a draw running concurrently on another
 * stream is the caller's error.  Address, n and level count stay, so captured chunk graphs stay valid; the table's
 * content VERSION (0 after the build) grows by 1 per call, and IQLHIP_TS_CONTINUE is honoured only behind a call on the
 * same generation AND version (the rows staged for the next step were drawn by the old weights).
 * iqlhip_weights_clear_flags: zeroes the flag word, on `stream`.
 * iqlhip_weights_state: waits for the device, then reads the current total, the flag word, the version and — q_out
 * not NULL — the n leaf values q[] rebuilt from the tree (either kind of table; each pointer may be NULL).
 * iqlhip_weights_info on an updatable table: n = capacity; total is the one at build; cum_host receives level 0 as
 * stored (node-local prefixes). */
int iqlhip_weights_build_updatable(const float* w_dev, int64_t n, int64_t capacity, float max_weight, void* stream,
                                   iqlhip_weights** out);
int iqlhip_weights_update(iqlhip_weights* table, const int64_t* idx_dev, const float* w_dev, int64_t m, int64_t bound,
                          void* stream);
int iqlhip_weights_clear_flags(iqlhip_weights* table, void* stream);
int iqlhip_weights_state(const iqlhip_weights* table, uint64_t* total, uint32_t* flags, uint64_t* version, uint64_t* q_out);
#define IQLHIP_WEIGHTS_FLAG_NONFINITE 1
#define IQLHIP_WEIGHTS_FLAG_NEGATIVE 2
#define IQLHIP_WEIGHTS_FLAG_INDEX 4
/* iqlhip_draw_indices with the weighted mapping: idx_dev[j], j < n_idx, of the stream (seed, offset).  One wave resolves
 * one index by a 64-ary descent through the table. */
int iqlhip_draw_indices_weighted(int64_t* idx_dev, int64_t n_idx, const iqlhip_weights* table, uint64_t seed,
                                 uint64_t offset, void* stream);
/* The same indices, bit for bit, plus the importance-sampling weights of the drawn rows for iqlhip_step_rw (DESIGN.md
 * §6j): c_dev[j] = (q_min / q_j)^is_beta, q_j the quantised weight of row idx_dev[j] (the table integer
 * iqlhip_weights_state returns) and q_min the smallest q among the batch_rows consecutive indices j belongs to (groups
 * [k batch_rows, (k + 1) batch_rows); a short last group is normalised over the rows it has).  Per-batch max
 * normalisation: the table total and the row count cancel, c in (0, 1], the rarest row of every batch has c = 1.0f and
 * is_beta = 0 gives 1.0f throughout.  Computed in fp32 through log2 / exp2 (relative error about 2e-6 at a 2^20 weight
 * range).  IQLHIP_EINVAL: a NULL pointer, n_idx or batch_rows < 1, is_beta negative or not finite. */
int iqlhip_draw_indices_weighted_is(int64_t* idx_dev, float* c_dev, int64_t n_idx, const iqlhip_weights* table, uint64_t seed,
                                    uint64_t offset, int64_t batch_rows, float is_beta, void* stream);
/* iqlhip_train_steps with every step's rows drawn by `table` (size must be the table's n): the idle blocks of each
 * forward draw and gather the next step's rows, so a weighted call consumes exactly the counters a plain call does.
 * IQLHIP_TS_CONTINUE is honoured only behind a weighted call on the same table GENERATION (and the conditions of
 * iqlhip_train_steps); a plain call never continues a weighted one, nor the reverse.  The chunk graphs of weighted
 * calls are a kind of their own, keyed by the table's address, n and level count as well.  IQLHIP_EUNSUPPORTED, before
 * anything is launched or any counter moves: a data-parallel exchange attached, bf16 batches of more than 512 rows,
 * injected keep-bits pending.  The table must outlive the call's queued work (iqlhip_weights_free waits for it).
 * iqlhip_train_steps_weighted_prepare: iqlhip_train_steps_prepare for the chunk graphs of such calls. */
int iqlhip_train_steps_weighted(iqlhip_ctx* ctx, const float* rows_dev, int64_t ld, int64_t size, int32_t batch_rows,
                                const iqlhip_step_scalars* sc, int32_t n_steps, uint64_t seed, uint64_t stream_offset,
                                int32_t flags, void* stream, const iqlhip_weights* table);
int iqlhip_train_steps_weighted_prepare(iqlhip_ctx* ctx, const float* rows_dev, int64_t ld, int32_t batch_rows,
                                        float inv_batch, void* stream, const iqlhip_weights* table);
/* iqlhip_train_steps_weighted with the importance-sampling correction of iqlhip_step_rw applied inside the chunk graphs
 * (DESIGN.md §6j): every step's loss terms are weighted by c_r = (q_min / q_r)^is_beta over that step's batch — bit for
 * bit the c that iqlhip_draw_indices_weighted_is(..., batch_rows, is_beta) returns for the same indices, so a call equals
 * the eager loop draw -> gather -> iqlhip_step_rw bit for bit, and is_beta = 0 equals iqlhip_train_steps_weighted.  The
 * idle blocks and the set-up kernel stage each drawn row's q next to the rows; one idle block of step t's forward forms
 * c before backward t (the row-weighted kernel) reads it: no launch more than a weighted call has.  is_beta is a value of
 * the CALL: the set-up kernel writes it to a device word, so another is_beta neither re-captures a chunk nor ends a
 * continuation.  The chunk graphs are a kind of their own (their own _prepare); such a call continues only such a call.
 * Everything iqlhip_train_steps_weighted refuses, and: IQLHIP_EINVAL for an is_beta that is negative or not finite,
 * IQLHIP_EUNSUPPORTED at bf16 precision. */
int iqlhip_train_steps_weighted_is(iqlhip_ctx* ctx, const float* rows_dev, int64_t ld, int64_t size, int32_t batch_rows,
                                   const iqlhip_step_scalars* sc, int32_t n_steps, uint64_t seed, uint64_t stream_offset,
                                   int32_t flags, void* stream, const iqlhip_weights* table, float is_beta);
int iqlhip_train_steps_weighted_is_prepare(iqlhip_ctx* ctx, const float* rows_dev, int64_t ld, int32_t batch_rows,
                                           float inv_batch, void* stream, const iqlhip_weights* table);
/* ---- prioritised replay: TD errors as new priorities (DESIGN.md §6j "Prioritised replay inside the chunk graphs") ----
 * The priority of a row with TD errors (e1, e2) = (q1 - y, q2 - y) is
 *     td_priority = (max(|e1|, |e2|) + eps)^alpha = exp2(alpha * log2(max(|e1|, |e2|) + eps)),
 * one device function for every caller, computed in fp32 through the hardware's log2 / exp2 (the intrinsics of the
 * importance-sampling weights); alpha = 0 gives 1.0f exactly.
 * iqlhip_weights_update_td: iqlhip_weights_update with w[j] = td_priority(td_dev[j][0], td_dev[j][1]) formed on the fly
 * (td_dev: [m][2] fp32 on the device, 8-byte aligned — what iqlhip_step_rw's td_out_dev receives; no intermediate weight
 * array).  Everything else is iqlhip_weights_update's: the last duplicate wins; a NaN or an infinity in either TD error
 * (flag 1) or an index outside [0, bound) (flag 4) is skipped; a priority beyond the table's scale saturates; slices of
 * 65 536 entries in order; asynchronous; the version grows by 1.  IQLHIP_EINVAL: a static table, alpha or eps negative or
 * not finite, and alpha = 0 together with eps = 0 — a zero TD error would give log2(0) * 0 = NaN and the row would be
 * skipped and flagged instead of getting the priority 1 that alpha = 0 means (eps = 0 with alpha > 0 is fine: a zero TD
 * error gives priority 0).
 * iqlhip_train_steps_prioritized: iqlhip_train_steps_weighted_is whose steps write their TD errors back into `table` (an
 * updatable one) as new priorities, inside the chunk graphs.  Per call:
 *     idx_0 = draw of step 0 by the table as it stands (the set-up kernel)
 *     for t = 0 .. n_steps - 1:
 *         idx_{t+1} = draw of step t + 1 (the idle blocks of forward t: it sees the updates of steps < t)
 *         step t on rows idx_t, loss terms weighted by c_t = (q_min / q_r)^is_beta with the q read at the draw
 *         table[idx_t] <- td_priority(TD errors of step t)              (in front of forward t + 1)
 * — bit for bit the eager loop iqlhip_draw_indices_weighted_is (step t + 1) -> iqlhip_step_rw with td_out (step t) ->
 * iqlhip_weights_update_td (step t), in this order.  The one-step lag keeps the draw off the critical path: the
 * priorities of step t first affect the draw of step t + 2.  The update is three more launches per step on the same
 * stream (a linear chain; m = batch_rows, bound = n).  alpha, eps and is_beta are values of the call (device words the
 * set-up kernel writes): changing them re-captures nothing.  IQLHIP_TS_CONTINUE: honoured only behind a prioritised call
 * (same table generation and version, and the conditions of iqlhip_train_steps) and means "this call goes on with that
 * call's lag-1 chain": its step 0 runs on the rows that call's last forward drew, one update behind.  A caller that wants
 * a call's result to depend on the table alone passes it only between the pieces of one burst (the Python layer does).
 * The call moves the table's version by 1: a weighted call that follows gathers afresh.  Everything
 * iqlhip_train_steps_weighted_is refuses, and IQLHIP_EINVAL for a static table and for alpha / eps as above — all before
 * anything is launched or any counter moves.  _prepare rehearses the chunk graphs with their update launches switched
 * off by the call's device word: it neither trains nor touches the table. */
int iqlhip_weights_update_td(iqlhip_weights* table, const int64_t* idx_dev, const float* td_dev, int64_t m, int64_t bound,
                             float alpha, float eps, void* stream);
int iqlhip_train_steps_prioritized(iqlhip_ctx* ctx, const float* rows_dev, int64_t ld, int64_t size, int32_t batch_rows,
                                   const iqlhip_step_scalars* sc, int32_t n_steps, uint64_t seed, uint64_t stream_offset,
                                   int32_t flags, void* stream, iqlhip_weights* table, float is_beta, float alpha, float eps);
int iqlhip_train_steps_prioritized_prepare(iqlhip_ctx* ctx, const float* rows_dev, int64_t ld, int32_t batch_rows,
                                           float inv_batch, void* stream, iqlhip_weights* table);
/* ---- tracking tables: new rows enter at the largest priority seen (DESIGN.md §6j "Online prioritised replay") ----
 * iqlhip_weights_build_tracking: iqlhip_weights_build_updatable plus one device word q_max (uint64, at the table's fixed
 * scale), max(max_i q[i], q(new_row_weight)) after the build; new_row_weight finite and > 0 (IQLHIP_EINVAL otherwise), it
 * saturates like any weight.  Every update that is APPLIED raises q_max to max(q_max, q_new): iqlhip_weights_update,
 * iqlhip_weights_update_td and the update launches of iqlhip_train_steps_prioritized's chunk graphs (their second
 * launch is then a tracking instantiation; "tracking or not" is part of what identifies such a chunk graph).  An entry
 * that lost to a later duplicate or was skipped (non-finite, negative, out of bound) raises nothing; q_max never falls;
 * an integer maximum, so the order of application does not matter.  _prepare's rehearsal leaves q_max as it leaves the
 * tree.  Whether a table tracks is fixed at its build; tables built by iqlhip_weights_build_updatable launch the kernels
 * they always did.  The group calls refuse a tracking table (IQLHIP_EUNSUPPORTED, naming the member).
 * iqlhip_weights_max: waits for the device, then reads q_max and w_max = q_max * 2^(e - 38) (each pointer may be NULL).
 * iqlhip_weights_insert_max: q[row] = q_max in one launch of one wave, queued on `stream` with no read-back; afterwards
 * every entry of the tree equals a fresh build over the changed weights at the same scale; the version grows by 1.
 * IQLHIP_EINVAL (both): a table that does not track; (insert) bound outside [0, n] or row outside [0, bound). */
int iqlhip_weights_build_tracking(const float* w_dev, int64_t n, int64_t capacity, float max_weight, float new_row_weight,
                                  void* stream, iqlhip_weights** out);
int iqlhip_weights_max(const iqlhip_weights* table, uint64_t* q_max, float* w_max);
int iqlhip_weights_insert_max(iqlhip_weights* table, int64_t row, int64_t bound, void* stream);
/* iqlhip_online_step with prioritised replay, one call per iteration of the online loop, everything queued on `stream`
 * and one synchronisation at the end:
 *   1. row_host -> ring row `pointer`, and table[pointer] <- q_max (one launch: iqlhip_weights_insert_max's wave in it);
 *   2. n indices of the stream (seed, stream_offset) by the table — behind the insert, so the new row can be drawn —, the
 *      rows gathered, c = (q_min / q_row)^is_beta over the n rows (iqlhip_draw_indices_weighted_is's arithmetic);
 *   3. iqlhip_step_rw on those rows with row weights c, TD errors kept;
 *   4. iqlhip_weights_update_td on the drawn indices with those TD errors (m = n, bound = capacity);
 *   5. act_state_host != NULL: the next action by the updated policy, as iqlhip_online_step.
 * Bit for bit the sequence ring write + iqlhip_weights_insert_max(pointer), iqlhip_draw_indices_weighted_is(n indices,
 * batch_rows = n), gather, iqlhip_step_rw, iqlhip_weights_update_td, act — parameters, Adam state, losses, statistics, TD
 * errors, action, and the table's leaves, total, flags, q_max; its version grows by 2.  The stream consumes
 * ceil(n / 2) counters from stream_offset.  Before anything is launched or any counter moves: IQLHIP_EINVAL for a static or
 * non-tracking table, a table whose n is not `capacity` or on another device, alpha / eps / is_beta as
 * iqlhip_train_steps_prioritized, and iqlhip_online_step's own; IQLHIP_EUNSUPPORTED at bf16 precision, with a data-parallel
 * exchange, with injected keep-bits pending.
 * iqlhip_online_prioritized_batch: the last such step's n drawn indices and TD errors ([n][2]) copied to device memory
 * on `stream` (either pointer may be NULL). */
int iqlhip_online_step_prioritized(iqlhip_ctx* ctx, float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer,
                                   const float* row_host, int32_t n, const iqlhip_step_scalars* sc, float out[3],
                                   const float* act_state_host, float max_action, uint64_t act_seed, float* act_out_host,
                                   void* stream, iqlhip_weights* table, uint64_t seed, uint64_t stream_offset, float is_beta,
                                   float alpha, float eps);
int iqlhip_online_prioritized_batch(iqlhip_ctx* ctx, int32_t n, int64_t* idx_out_dev, float* td_out_dev, void* stream);
/* iqlhip_online_step for a raw ring and the n-step ring derived from it ("n-step rows" below), in one
 * call and under one synchronisation.  One launch of at most four blocks in front of iqlhip_online_step's own: it stores
 * row_host at raw_dev[pointer], stores episode_end != 0 at ends_dev[pointer] and refreshes the min(horizon, size_after)
 * derived rows that end at `pointer` — iqlhip_rows_nstep_ring with newest = pointer, reading the new row from the host
 * words.  Then iqlhip_online_step's launches run on the DERIVED ring rows_dev: its gather stores row_host at
 * rows_dev[pointer], which is what the refresh stored there (the newest derived row has k = 1), and the step trains on
 * rows_dev[idx_host[..]].  size_after: the ring's size with the new row.  steps_dev (uint8 [capacity]) may be NULL.
 * Bit for bit: the ring write, iqlhip_rows_nstep_ring, iqlhip_rows_sample_packed on rows_dev and iqlhip_step_sync.
 * Refuses what iqlhip_online_step and iqlhip_rows_nstep_ring refuse, and a data-parallel exchange
 * (IQLHIP_EUNSUPPORTED), before anything is launched. */
int iqlhip_online_step_nstep(iqlhip_ctx* ctx, float* raw_dev, float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer,
                             const float* row_host, const int64_t* idx_host, int32_t n, const iqlhip_step_scalars* sc,
                             float out[3], const float* act_state_host, float max_action, uint64_t act_seed,
                             float* act_out_host, void* stream, uint8_t* ends_dev, int32_t episode_end, int64_t size_after,
                             int32_t horizon, double discount, uint8_t* steps_dev);

/* ---- vector-environment online step --------------------------------------------------------------------------
 * One agent, E environments and an update-to-data ratio of U: E transitions into the ring, U gradient steps and the
 * next actions of E2 states in one call and under one synchronisation.
 * IQLHIP_VEC_MAX_ENVS bounds E and E2: one pinned staging block of 64 rows of at most iqlhip_row_stride(S, A) floats,
 * under 70 KB at IQLHIP_MAX_INPUT.  IQLHIP_VEC_MAX_UPDATES bounds U.
 *
 * iqlhip_rows_write_ring: the n_rows packed rows rows_pin[j][ld] — pinned, host-mapped memory (or device memory) that the
 * caller leaves untouched until the launch has run — are stored at ring rows (pointer + j) mod capacity of rows_dev, in
 * one launch on `stream`; no context.  1 <= n_rows <= min(capacity, IQLHIP_VEC_MAX_ENVS), ld a multiple of 4 and >= 8,
 * both blocks 16-byte aligned, 0 <= pointer < capacity (IQLHIP_EINVAL otherwise, before the launch).
 *
 * iqlhip_online_step_vec, queued on `stream`:
 *   1. one launch stores the n_rows new rows rows_host[j][ld] at ring rows (pointer + j) mod capacity and gathers the
 *      n_updates * batch_rows rows rows_dev[idx_host[..]] — the indices of n_updates consecutive sample() draws over the
 *      size after all inserts — into a staging block [n_updates][batch_rows][ld] the context owns (sized on first use,
 *      grown when a call needs more).  A drawn index i with (i - pointer) mod capacity < n_rows reads new row j from
 *      the host words: the ring write of another block may not have landed.  No other ring row is written;
 *   2. n_updates eager steps back to back, the launches of iqlhip_step each: step u trains on slice u of the staging
 *      block with the scalars sc[u]; its losses land in out[3 * u ..]; with statistics enabled its 16 numbers go to slot
 *      u of the ring iqlhip_read_stats_ring reads; actor dropout draws its keep-bits per step as iqlhip_step does;
 *      iqlhip_read_grad_clip reports the last step;
 *   3. act_states_host != NULL: the actions of act_rows states [act_rows][state_dim] by the updated policy —
 *      iqlhip_actor_sample's launches over act_rows rows when act_seed != 0 and the policy is Gaussian (the noise call
 *      counter advances by one), else iqlhip_actor_forward's; the inference keep-bit stream advances by one call as
 *      theirs does — into act_out_host [act_rows][action_dim].
 * The call's last launch stores the completion word the host spins on (an act over more than 256 action words adds a
 * one-thread launch for it); n_updates = 0 without an act ends on a stream synchronisation.  Launches: 1 + 3 n_updates
 * + the act's, plus per step the keep-bit launch with actor dropout, the two or three statistics / clip launches when
 * those are on, and the shadow refresh at bf16 precision — what iqlhip_step itself launches.
 * rows_host, idx_host, sc, act_states_host are ordinary host memory (copied into pinned staging inside the call);
 * idx_host, sc and out may be NULL when n_updates = 0.  Bit for bit what n_rows single ring writes, n_updates times
 * iqlhip_rows_sample_packed + iqlhip_step_sync, and the actor call give.
 * Refused before anything is launched or any counter moves — IQLHIP_EINVAL: a NULL argument, ld other than the context's
 * row stride, misaligned rows, pointer outside the ring, n_rows outside [1, min(capacity, IQLHIP_VEC_MAX_ENVS)],
 * n_updates outside [0, IQLHIP_VEC_MAX_UPDATES], act_rows outside [1, IQLHIP_VEC_MAX_ENVS], batch_rows outside
 * [1, min(512, max_batch)]; IQLHIP_EINDEX: an index outside [0, capacity); IQLHIP_EUNSUPPORTED: a data-parallel exchange
 * attached, injected keep-bits pending, bf16 batches of more than 512 rows, and what statistics and clipping refuse. */
#define IQLHIP_VEC_MAX_ENVS 64
#define IQLHIP_VEC_MAX_UPDATES 32
int iqlhip_rows_write_ring(float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer, const float* rows_pin,
                           int32_t n_rows, void* stream);
int iqlhip_online_step_vec(iqlhip_ctx* ctx, float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer,
                           const float* rows_host, int32_t n_rows, const int64_t* idx_host, int32_t batch_rows,
                           int32_t n_updates, const iqlhip_step_scalars* sc, float* out, const float* act_states_host,
                           int32_t act_rows, float max_action, uint64_t act_seed, float* act_out_host, void* stream);

/* Data-parallel split of the same step: forward+backward, then the
 * flat gradient (n_params floats + 4 tail words: 3 loss sums and a spare) is
 * written to grads_dev for the caller's all-reduce, then the update consumes it. */
int iqlhip_forward_backward(iqlhip_ctx* ctx, const iqlhip_batch* batch, const iqlhip_step_scalars* sc,
                            float* grads_dev, void* stream);
int iqlhip_apply_update(iqlhip_ctx* ctx, const float* grads_dev, const iqlhip_step_scalars* sc, void* stream);
/* Tests and debugging: iqlhip_forward_backward with iqlhip_step_rw's row weights (same arguments, same refusals) — the
 * flat gradient of the weighted losses, the tail words their sums; what the parity tests compare per tensor. */
int iqlhip_forward_backward_rw(iqlhip_ctx* ctx, const iqlhip_batch* batch, const iqlhip_step_scalars* sc,
                               const float* row_w_dev, float* td_out_dev, float* grads_dev, void* stream);
int64_t iqlhip_grad_words(const iqlhip_ctx* ctx);   /* n_params + 4 */

/* n_steps consecutive `sample -> train` iterations without host round trips: row indices are drawn on the device
 * (Philox4x32-10, uniform with replacement over [0,size) like np.random.randint at iql.py:172; index j of the call comes
 * from counter stream_offset + j / 2, modulo 2^64: counter words (lo32, hi32, 0x49514C48, 0), key (lo32 seed, hi32 seed);
 * an even j takes output words o1:o0, an odd j o3:o2 as 64 random bits r, index = floor(r * size / 2^64); step k of the
 * call trains on indices k * batch_rows .. (k + 1) * batch_rows - 1.  A call consumes ceil(n_steps * batch_rows / 2)
 * counters.  With an odd batch_rows a step's first index alternates between a counter's two word pairs, and a caller
 * that starts every call on a fresh counter — the Python shim passes stream_offset = total_it * ceil(batch_rows / 2) —
 * does not continue the previous call's stream: the rows drawn then depend on how the steps are split into calls (with
 * an even batch_rows they do not).  DESIGN.md "Random streams" has all four device streams),
 * per-step scalars come from `sc` (host array of n_steps, free again on return).
 * The loss of every step is kept in a device ring read by iqlhip_read_loss_ring.
 * Replaces the offline loop body sample()->train() (algorithms/offline/iql.py:631-635).
 * A call = one set-up launch + replays of fixed chunk graphs (IQLHIP_GRAPH_STEPS = 64 steps, 16, 4, 2, 1) that chain on
 * the device; nothing is captured per value of n_steps.
 * flags: IQLHIP_TS_CONTINUE — the caller states that the replay rows have not been written since the previous
 * iqlhip_train_steps call; if that call ended where this one starts (same rows / size / batch_rows / seed,
 * stream_offset = its offset + n_steps * batch_rows / 2 exactly, an even n_steps (so that n_steps * batch_rows is even
 * and the previous call ended on a whole counter), no other step entry point in between — the library checks all of
 * that) the rows its last forward staged for "the next step" ARE this call's step 0 and nothing is gathered up front.
 * Results are identical with and without the flag: it never changes which rows a (seed, stream_offset) pair draws. */
#define IQLHIP_TS_CONTINUE 1
int iqlhip_train_steps(iqlhip_ctx* ctx, const float* rows_dev, int64_t ld, int64_t size, int32_t batch_rows,
                       const iqlhip_step_scalars* sc, int32_t n_steps, uint64_t seed, uint64_t stream_offset,
                       int32_t flags, void* stream);

/* Capture, instantiate, upload AND rehearse (arenas saved and restored) every chunk graph iqlhip_train_steps replays for
 * this (buffer, batch_rows, inv_batch) — and, with an exchange attached, this exchange mode — so that no later
 * iqlhip_train_steps call pays for a capture or a first replay (bench.py calls it before its timed region).  The
 * rehearsal replays run on `stream` (pass the stream the later calls will use); synchronous. */
int iqlhip_train_steps_prepare(iqlhip_ctx* ctx, const float* rows_dev, int64_t ld, int32_t batch_rows, float inv_batch,
                               void* stream);

/* ---- data-parallel gradient exchange (the reference has no multi-device code) ----------------
 * One process per GPU.  With an exchange attached, iqlhip_step and iqlhip_train_steps run, per step:
 * forward, backward, flatten (this rank's flat gradient: n_params floats + 4 tail words with the loss
 * contributions; batch means divided by the GLOBAL row count: sc->inv_batch = 1 / (batch_rows * world)), the
 * exchange, and the fused Adam / Polyak update on the summed gradient — all on `stream`, inside the captured chunk
 * graphs too.  Two exchanges:
 *   RCCL  ncclAllReduce(sum, fp32) of the flat buffer, in place, in-stream (iqlhip_allreduce_init).
 *   P2P   every rank's flat buffers are mapped into every other rank (hipIpc); after a flag handshake in device
 *         memory the update kernel reads all ranks' buffers directly over xGMI and sums them in rank order
 *         (iqlhip_p2p_export + iqlhip_p2p_attach).  No collective library call per step. */
enum { IQLHIP_XCH_NONE = 0, IQLHIP_XCH_RCCL = 1, IQLHIP_XCH_P2P = 2 };
#define IQLHIP_UNIQUE_ID_BYTES 128  /* = NCCL_UNIQUE_ID_BYTES */
#define IQLHIP_IPC_HANDLE_BYTES 64  /* = sizeof(hipIpcMemHandle_t) */
/* ncclGetUniqueId: called by ONE rank; the caller ships the 128 bytes to the others (any channel). */
int iqlhip_comm_unique_id(void* id_out);
/* ncclCommInitRank on the context's device; collective over the `world` ranks.  Selects the RCCL exchange. */
int iqlhip_allreduce_init(iqlhip_ctx* ctx, const void* unique_id, int rank, int world);
/* P2P exchange, step 1: allocate this rank's exchange block (flags + two flat buffers) and export it
 * (hipIpcGetMemHandle) into handle_out[IQLHIP_IPC_HANDLE_BYTES]; the caller all-gathers the handles. */
int iqlhip_p2p_export(iqlhip_ctx* ctx, void* handle_out, int rank, int world);
/* step 2: map the peers' blocks (handles = world x IQLHIP_IPC_HANDLE_BYTES in rank order; the own slot is ignored).
 * Selects the P2P exchange.  timeout_ms bounds every in-stream wait for a peer (0 = 5000). */
int iqlhip_p2p_attach(iqlhip_ctx* ctx, const void* handles, int timeout_ms);
/* Switch between attached exchanges (IQLHIP_XCH_*); NONE detaches nothing, it only runs steps locally. */
int iqlhip_xch_select(iqlhip_ctx* ctx, int mode);
/* status[0] = mode in use, status[1] = first step at which a P2P wait timed out (0 = never), status[2] = steps
 * exchanged so far.  Synchronises `stream`. */
int iqlhip_xch_status(iqlhip_ctx* ctx, int64_t status[3], void* stream);
/* Forget a recorded P2P wait timeout (status[1] back to 0) once the caller has re-synchronised the replicas and
 * selected another exchange.  Until then iqlhip_read_losses / iqlhip_read_loss_ring / iqlhip_online_step — the entry
 * points that synchronise — return IQLHIP_EEXCHANGE; fully asynchronous callers poll iqlhip_xch_status. */
int iqlhip_xch_clear_status(iqlhip_ctx* ctx, void* stream);
/* Release communicator / peer mappings (also done by iqlhip_destroy). */
int iqlhip_xch_shutdown(iqlhip_ctx* ctx);

/* The three .item() calls of iql.py:491,509,535: synchronises `stream`. out = {value,q,actor}. */
int iqlhip_read_losses(iqlhip_ctx* ctx, float out[3], void* stream);
int iqlhip_read_loss_ring(iqlhip_ctx* ctx, float* out, int32_t n_steps, void* stream);

/* ---- per-step training statistics (opt-in) ----------------------------------------------------
 * IQLHIP_N_STATS floats per step that describe the batch the step trained on, evaluated with the parameters BEFORE
 * that step's update (the convention of the three losses).  With tq = min(tQ1, tQ2), adv = tq - V(s),
 * y = r + (1 - d) * discount * V(s'), in this order:
 *    0 v_mean          mean V(s)            1 next_v_mean     mean V(s')          2 q1_mean   mean Q1(s,a)
 *    3 q2_mean         mean Q2(s,a)         4 target_q_mean   mean tq             5 td_target_mean   mean y
 *    6 q_gap_mean      mean |Q1 - Q2|       7 adv_mean        8 adv_min           9 adv_max
 *   10 adv_pos_frac    share of rows on the expectile's upper side (every row but those with adv < 0: the comparison
 *                      the value loss makes)
 *   11 exp_adv_mean    mean of min(exp(beta * adv), EXP_ADV_MAX), the actor loss's row weights
 *   12 exp_adv_clamped_frac   share of rows whose weight sits on that clamp
 *   13 grad_norm_vf / 14 grad_norm_qf (both Q nets) / 15 grad_norm_actor (+ log_std): L2 norms of the gradients as Adam
 *      receives them
 * Head values are the fixed-order sums of the four slice partials the step itself uses; sums run in a fixed order
 * (deterministic).  Default off: nothing is launched, captured or allocated, and every result is bit-identical to a
 * library without this feature.  Enabled, every entry point that runs a step records them (two extra launches per
 * step between its backward and its update; iqlhip_train_steps keeps chunk graphs of their own per setting, and a
 * ring indexed like the loss ring); parameters, losses and random streams do not change.  Not supported
 * (IQLHIP_EUNSUPPORTED from the step entry points, before anything is launched): a context with a data-parallel
 * exchange selected (the local slabs are not what Adam receives there), and steps that take the large-batch bf16
 * path (more than 512 rows in bf16). */
int iqlhip_set_step_stats(iqlhip_ctx* ctx, int enabled);
/* The last step's statistics; synchronises `stream`.  IQLHIP_EINVAL when statistics are off. */
int iqlhip_read_step_stats(iqlhip_ctx* ctx, float out[IQLHIP_N_STATS], void* stream);
/* out[n_steps][IQLHIP_N_STATS]: the statistics of the first n_steps steps of the last iqlhip_train_steps call (like
 * iqlhip_read_loss_ring); synchronises `stream`. */
int iqlhip_read_stats_ring(iqlhip_ctx* ctx, float* out, int32_t n_steps, void* stream);

/* ---- gradient-norm clipping per optimizer group (opt-in) ---------------------------------------
 * torch.nn.utils.clip_grad_norm_ (L2, error_if_nonfinite = False) between a step's backward and its Adam update,
 * independently for the three optimizer groups, in this order: V | Q1 + Q2 | pi (with log_std).  Per group, in fp32:
 *    total_norm = sqrt(sum of squares of the group's gradient as Adam would receive it)    (statistics 13..15)
 *    coef       = min(max_norm / (total_norm + 1e-6f), 1.0f)
 *    grad      *= coef            (one multiply per element, also when coef is 1)
 * max_norm[g] <= 0 or +inf: no limit for that group (its coefficient is exactly 1); NaN: IQLHIP_EINVAL.  All three
 * without a limit: the feature is off — nothing is allocated, launched or captured and every result is bit-identical
 * to a library without it.  On, every entry point that runs a step clips (iqlhip_step and its forms,
 * iqlhip_online_step, iqlhip_train_steps — which keeps chunk graphs of their own per on/off setting — and the group
 * calls, where it is a per-member setting).  The limits live in device memory: changing them needs no re-capture; the
 * new limits are queued (an asynchronous copy from pinned memory) on the stream of the context's last step call, so
 * steps already queued there keep the old limits and every later one reads the new ones; a caller that moves to
 * another stream orders the two itself, as for the arenas.
 * The sum of squares runs in a fixed order (deterministic; the block partials are shared with the statistics).
 * iqlhip_forward_backward keeps returning the UNCLIPPED gradient, and iqlhip_apply_update applies the caller's
 * gradient as given.  Not supported (IQLHIP_EUNSUPPORTED from the step entry points, before anything is launched or
 * any counter moves): a context with a data-parallel exchange selected (the norm would have to be taken after the
 * exchange), and steps that take the large-batch bf16 path (more than 512 rows in bf16). */
int iqlhip_set_grad_clip(iqlhip_ctx* ctx, const float max_norm[3]);
/* The limits as the context holds them (+inf = no limit). */
int iqlhip_get_grad_clip(const iqlhip_ctx* ctx, float max_norm[3]);
/* {norm_v, norm_q, norm_pi, coef_v, coef_q, coef_pi} of the last step (the norms before clipping); synchronises
 * `stream`.  IQLHIP_EINVAL when clipping is off. */
int iqlhip_read_grad_clip(iqlhip_ctx* ctx, float out[6], void* stream);

/* ---- replay buffer storage (packed rows [s | a | s' | r | d | pad]) ------ */
/* Row stride in floats for given dims (multiple of 4 floats = 16 B). */
int64_t iqlhip_row_stride(int32_t state_dim, int32_t action_dim);
/* ReplayBuffer.load_d4rl_dataset / add_transition (iql.py:153-169,180-196): write n
 * rows starting at row0 from five contiguous device arrays. */
int iqlhip_rows_write(float* rows_dev, int64_t ld, int32_t state_dim, int32_t action_dim, int64_t row0, int64_t n,
                      const float* s_dev, const float* a_dev, const float* r_dev, const float* ns_dev,
                      const float* d_dev, void* stream);
/* Synthetic D4RL-shaped rows written where they live (bench data of SURVEY §8d's distributions: obs / next_obs ~ N(0,1),
 * actions ~ U(-1,1) * 0.999, rewards ~ N(0,1) or the antmaze flavour {-1, 0}, dones ~ Bernoulli(p_done); Philox4x32-10
 * keyed by `seed`, counter = element number, so every rank of a data-parallel run fills identical rows without a
 * host-side generator or an upload).  Replaces nothing in the reference (its data come from d4rl.qlearning_dataset). */
int iqlhip_rows_fill_synth(float* rows_dev, int64_t ld, int32_t state_dim, int32_t action_dim, int64_t row0, int64_t n,
                           uint64_t seed, float p_done, int32_t antmaze_rewards, void* stream);
/* ReplayBuffer.sample's five advanced-index gathers (iql.py:173-177) in one launch.  n_rows = rows the buffer holds
 * (its capacity): the reference's indexing raises IndexError for an index outside the tensors; the entry points that
 * see the indices on the host return IQLHIP_EINDEX before anything is launched, the ones that take device indices never
 * dereference such an index (its output row is filled with NaN instead of faulting the GPU) — a caller that wants the
 * exception checks device indices itself, as the Python shim's ReplayBuffer.gather does. */
int iqlhip_rows_gather(const float* rows_dev, int64_t ld, int64_t n_rows, int32_t state_dim, int32_t action_dim,
                       const int64_t* idx_dev, int64_t n, float* s_dev, float* a_dev, float* r_dev, float* ns_dev,
                       float* d_dev, void* stream);
/* The same sample as whole packed rows: out[i] = rows[idx[i]] (one coalesced row copy per sample).  A batch whose
 * five pointers are the packed offsets of such a block (a = s + S, s' = s + S + A, r = s + 2S + A, d = r + 1, all
 * strides = iqlhip_row_stride, 16-byte aligned) is consumed IN PLACE by iqlhip_step / iqlhip_forward_backward. */
int iqlhip_rows_gather_packed(const float* rows_dev, int64_t ld, int64_t n_rows, const int64_t* idx_dev, int64_t n,
                              float* out_rows_dev, void* stream);
/* ... with the indices still in (pinned) host memory, as np.random.randint leaves them (iql.py:172): copies them to
 * idx_scratch_dev on `stream`, then gathers.  idx_host must stay untouched until that copy has run. */
int iqlhip_rows_gather_packed_h(const float* rows_dev, int64_t ld, int64_t n_rows, const int64_t* idx_host,
                                int64_t* idx_scratch_dev, int64_t n, float* out_rows_dev, void* stream);
/* ... or in ordinary host memory: the library stages them through its own pinned ring (event-guarded) — the whole
 * device side of ReplayBuffer.sample(batch_size) after the np.random.randint draw, in one call. */
int iqlhip_rows_sample_packed(const float* rows_dev, int64_t ld, int64_t n_rows, const int64_t* idx_host, int64_t n,
                              float* out_rows_dev, void* stream);
/* ---- dataset ingest on the device -------------------------------------------------------------
 * compute_mean_std (algorithms/finetune/iql.py:77-80): mean[c] = mean_r x[r][c], std[c] = sqrt(mean_r (x - mean)^2) + eps
 * over n rows of ncols columns (row stride ld floats; e.g. the state columns of packed replay rows: x = rows_dev,
 * ncols = state_dim).  Sums in float64, fixed order (deterministic); results are float32 like numpy's. */
int iqlhip_cols_mean_std(const float* x_dev, int64_t ld, int32_t ncols, int64_t n, float eps, float* mean_dev,
                         float* std_dev, void* stream);
/* normalize_states (:83-84) applied in place to the s and s' columns of n packed rows from row0:
 * x = (x - mean[c]) / std[c] in fp32 — bit-identical to numpy given the same mean / std. */
int iqlhip_rows_normalize(float* rows_dev, int64_t ld, int32_t state_dim, int32_t action_dim, int64_t row0, int64_t n,
                          const float* mean_dev, const float* std_dev, void* stream);
/* return_reward_range (:262-274) over n packed rows from row0, in storage order: min and max of the episode returns,
 * and the number of complete episodes.  Row i ends an episode iff its done column is non-zero or its episode has
 * reached max_episode_steps rows; a trailing run that ends neither way is no episode (the reference keeps only its
 * length).  A return is the float64 sum of the episode's float32 rewards, added in ascending row order one after the
 * other (one thread walks one episode), so out_min_max is bit-identical to the reference's Python floats.  No complete
 * episode (the reference's min([]) raises ValueError): IQLHIP_EINVAL, *out_episodes = 0, out_min_max untouched.  NaN
 * rewards are outside the contract (Python's min / max depend on the order of their arguments there).  Device scratch
 * (8 B per row) is allocated and freed on `stream`.  Synchronises `stream`. */
int iqlhip_rows_return_range(const float* rows_dev, int64_t ld, int32_t state_dim, int32_t action_dim, int64_t row0,
                             int64_t n, int32_t max_episode_steps, double out_min_max[2], int64_t* out_episodes,
                             void* stream);
/* modify_reward's rescaling (:280-281) applied in place to the reward column of n packed rows from row0, in fp32 as two
 * separately rounded operations: r = r / divide_by (IEEE division), then r = r * multiply_by — what numpy's
 * `rewards /= max_ret - min_ret; rewards *= max_episode_steps` does to a float32 array, with
 * divide_by = (float)(max_ret - min_ret) (subtracted in double) and multiply_by = (float)max_episode_steps.
 * divide_by == 0: IQLHIP_EINVAL.  No other column is written. */
int iqlhip_rows_reward_scale(float* rows_dev, int64_t ld, int32_t state_dim, int32_t action_dim, int64_t row0, int64_t n,
                             float divide_by, float multiply_by, void* stream);
/* modify_reward's antmaze branch (:287-288): r = r - subtract in fp32 on the same column. */
int iqlhip_rows_reward_shift(float* rows_dev, int64_t ld, int32_t state_dim, int32_t action_dim, int64_t row0, int64_t n,
                             float subtract, void* stream);
/* The three calls above refuse, before any device work, with IQLHIP_EINVAL: a NULL pointer, n < 1, row0 < 0,
 * max_episode_steps < 1, ld < iqlhip_row_stride(state_dim, action_dim). */
/* Per-row episode spans, returns and discounted return-to-go of n packed rows from row0, in storage order (a loaded
 * dataset, not a wrapped ring) — get_return_to_go of the reference's finetune/cal_ql.py and the episode returns behind
 * keep_best_trajectories of offline/any_percent_bc.py, as device arrays ([n] each; any may be NULL).  i is 0-based in
 * the range; everything is integers and float64, so a CPU restatement (tests/returns_ref.py) agrees to the bit.
 *   break        row i is a break iff d[i] != 0, or state_break_tol >= 0 and i + 1 < n and ss > tol * tol, where
 *                ss = sum over columns c, ascending, of (double)dlt_c * (double)dlt_c, dlt_c = s[i+1][c] - s'[i][c] in
 *                float32 (one rounding), the product and every addition rounded on its own (Cal-QL's
 *                norm(obs[t+1] - next_obs[t]) > 1e-6; state_break_tol < 0: rule off)
 *   episode end  with p(i) = the largest break j < i (-1 if none) and o = i - p(i) - 1: row i ends an episode iff it is a
 *                break, or (o + 1) % max_episode_steps == 0, or IQLHIP_EP_KEEP_TAIL is set and i == n - 1; its episode
 *                starts at p(i) + 1 + (o / max_episode_steps) * max_episode_steps.  Rule off and flag clear: exactly
 *                iqlhip_rows_return_range's episodes.
 *   tail rows    of a trailing run that ends no episode: ep_first = ep_last = -1, ep_return = return_to_go = 0.0
 *   ep_first / ep_last   the row's episode, relative to row0
 *   ep_return    the episode's float32 rewards added in float64 from 0.0, first row to last, one after another
 *                (iqlhip_rows_return_range's value), on every row of the episode
 *   return_to_go G[last] = (double)r[last]; G[i] = (double)r[i] + discount * G[i+1] down the episode, the product
 *                rounded, then the sum: Cal-QL's recurrence bit for bit (a last reward of -0.0 stays -0.0)
 *   sparse_value (host pointer; NULL: off) an episode whose (double)r[last] == *sparse_value gets
 *                return_to_go = (double)r[last] / (1.0 - discount) on all its rows (ours: not claimed bit-equal to the
 *                reference, whose branch mixes numpy scalar types)
 *   episodes_out (host; may be NULL) the number of episodes; zero episodes is a result, not an error
 * NaN rewards and NaN states are outside the contract.  One thread walks one episode in order; the spans and the
 * ep_return broadcast are row-parallel.  Device scratch (9 B per row) is allocated and freed on `stream`; nothing stays
 * attached to any context.  Synchronises `stream` only when episodes_out is given.  No column of the rows is written.
 * IQLHIP_EINVAL before any device work: what the reward calls above refuse, max_episode_steps < 1, a NaN, infinite or
 * negative discount, a NaN state_break_tol, unknown flag bits, all five outputs NULL, sparse_value with discount == 1. */
#define IQLHIP_EP_KEEP_TAIL 1
int iqlhip_rows_episode_returns(const float* rows_dev, int64_t ld, int32_t state_dim, int32_t action_dim, int64_t row0,
                                int64_t n, int64_t max_episode_steps, double discount, double state_break_tol,
                                int32_t flags, const double* sparse_value, double* ep_return_dev,
                                double* return_to_go_dev, int64_t* ep_first_dev, int64_t* ep_last_dev,
                                int64_t* episodes_out, void* stream);

/* ---- n-step rows --------------------------------------------------------------------------------
 * A DERIVED row store: one-step packed rows rewritten so that the unchanged step kernels, which all form
 *   y = r + ((1.f - d) * discount) * next_v,
 * compute a k-step target from them: r holds the discounted reward sum of k rows, s' the state k rows ahead and
 * d = 1 - discount^(k - 1) * (1 - d_last), so that (1 - d) * discount = discount^k * (1 - d_last).  Every call that takes
 * packed rows takes a derived store as it is.  The d column of a derived store therefore holds fractions by design.
 * Arithmetic (integers and float64, fp contract off; tests/nstep_ref.py restates it and agrees to the bit), for row i of
 * a range, horizon N in [1, IQLHIP_NSTEP_MAX_HORIZON]:
 *   limit L(i)  build form: min(i + N - 1, end(i)); end(i) = ep_last[i] when a table is given and the entry is >= 0 (an
 *               entry outside [i, n - 1] is clamped into it), else n - 1, the last row of the range.
 *               ring form: rows in ring order (oldest first, positions modulo the capacity); the chain also stops at a
 *               row whose end byte is not 0, and at the newest row: it never passes the newest row.
 *   chain       m = the first row j in [i, L(i)] with d[j] != 0, or L(i) if there is none; k = m - i + 1.
 *   r           G = (double)r[m]; for j = m - 1 down to i: G = (double)r[j] + discount * G, the product rounded, then
 *               the sum; the row stores (float)G.
 *   d           d[m] itself if d[m] != 0; else c = 1.0, (k - 1) times c = c * discount, and the row stores
 *               (float)(1.0 - c): +0.0 for k = 1.  (A stored done of -0.0 is outside the contract.)
 *   columns     s, a and the pad columns below iqlhip_row_stride of row i, s' of row m; steps[i] = k (uint8).
 * So N = 1 copies the rows bit for bit.  NaN rewards are outside the contract.  Row-parallel, one launch, 64-bit row
 * offsets; the source rows are only read.  Nothing is allocated; nothing stays attached to a context. */
#define IQLHIP_NSTEP_MAX_HORIZON 64
/* Build form: rows [row0, row0 + n) of src_dev -> the same rows of dst_dev.  ep_last_dev (int64 [n], may be NULL) and
 * steps_dev (uint8 [n], may be NULL) are indexed from 0 in the range; ep_last is iqlhip_rows_episode_returns' column,
 * relative to row0.  IQLHIP_EINVAL before any device work: a NULL store, n < 1, row0 < 0, a stride below
 * iqlhip_row_stride or no multiple of 4, a store not 16-byte aligned, src_dev == dst_dev or overlapping ranges (the
 * rows are not built in place), a horizon outside [1, 64], a discount that is not finite or outside (0, 1]. */
int iqlhip_rows_nstep(const float* src_dev, int64_t src_ld, float* dst_dev, int64_t dst_ld, int32_t state_dim,
                      int32_t action_dim, int64_t row0, int64_t n, int32_t horizon, double discount,
                      const int64_t* ep_last_dev, uint8_t* steps_dev, void* stream);
/* Ring form: src_dev and dst_dev are rings of `capacity` rows of stride ld that hold `size` rows, the newest at position
 * `newest` (the oldest at (newest - size + 1) mod capacity); ends_dev[capacity] holds one byte per position, not 0
 * where the stored row ends an episode (a terminal state or a time limit).  Recomputes the min(horizon, size) derived
 * rows that end at `newest` — the only rows whose chains a new transition can extend — in one launch of at most four
 * blocks; steps_dev (uint8 [capacity], may be NULL) is indexed by position.  Invariant: a derived ring refreshed after
 * every insert equals the build form applied to the ring unrolled into time order, ep_last taken from the end bytes.
 * IQLHIP_EINVAL before any device work: what the build form refuses, size outside [1, capacity], newest outside the
 * ring (or beyond size in a ring that has not wrapped), a NULL ends_dev. */
int iqlhip_rows_nstep_ring(const float* src_dev, float* dst_dev, int64_t ld, int32_t state_dim, int32_t action_dim,
                           int64_t capacity, int64_t size, int64_t newest, const uint8_t* ends_dev, int32_t horizon,
                           double discount, uint8_t* steps_dev, void* stream);
/* Device-side index draw used by iqlhip_train_steps, exposed for tests. */
int iqlhip_draw_indices(int64_t* idx_dev, int64_t n, int64_t size, uint64_t seed, uint64_t offset, void* stream);

/* ---- scoring transitions without a step ----------------------------------------------------------
 * What the networks think of n transitions, with no gradient step: per row IQLHIP_N_SCORE floats
 *   v  next_v  q1  q2  target_q = min(qt1, qt2)  adv = target_q - v  exp_adv = min(exp(beta adv), exp_adv_max)
 *   bc = the row's behaviour-cloning term (Gaussian policy: sum over action dims of -log_prob(a) with the clamped
 *        log_std; deterministic: sum of (a - mu)^2)
 * and over all n rows summary[11]: value_loss, q_loss (with the reference's / 2), actor_loss — the three losses of
 * _update_v / _update_q / _update_policy (iql.py:482-534) as means over n — then the eight column means.
 * Rows: packed replay rows [s | a | s' | r | d | pad] of stride ld (a multiple of 4, >= iqlhip_row_stride; 16-byte
 * aligned), n_rows of them; either the range [row0, row0 + n) (idx_dev NULL) or the n rows idx_dev[0 .. n) names, in
 * that order (row0 ignored).  out_dev: [n][IQLHIP_N_SCORE] floats, 16-byte aligned, or NULL (summary only); summary: 11
 * host floats or NULL; not both NULL.  The policy is evaluated without dropout (actor.eval()).  Parameters are always
 * the fp32 masters and the arithmetic fp32 MFMA, also in a context set to bf16 operands: a row's eight floats depend on
 * the row and the parameters alone — not on n, chunk_rows, the row's place in the call or range / index addressing.
 * The summary's sums are added per 32-row tile in fp32 and over tiles in double; they depend on how the call groups
 * rows into tiles and chunks only in the last bits.
 * chunk_rows: rows scored per launch sequence (0: the library's 65 536; larger values are cut to that; the scratch —
 * head partials of one chunk — is allocated by the context's first call and sized by it, never by n).
 * Before anything is launched: IQLHIP_EINVAL for n < 1, NULL rows, a range outside [0, n_rows], a negative chunk_rows
 * or one that is no multiple of 32, misaligned pointers or stride, both outputs NULL; IQLHIP_ENOTBOUND before
 * iqlhip_bind.  An index list is range-checked on the device in front of the forward (one small launch, then the call
 * waits for its verdict): IQLHIP_EINDEX when an index lies outside [0, n_rows), and no row has been read.
 * The call writes its own scratch, out_dev and summary — no parameter, moment or target, nothing of the step's
 * staging, activations, slabs, chunk header, graph cache, random-stream counters, loss / statistics / clip rings.
 * Legal on a data-parallel context (local, no exchange) and on a trainer group's member.  Synchronises `stream` when
 * idx_dev or summary is given; otherwise it only queues work.  (All members of a group: iqlhip_group_score_rows.) */
int iqlhip_score_rows(iqlhip_ctx* ctx, const float* rows_dev, int64_t ld, int64_t n_rows, int64_t row0, int64_t n,
                      const int64_t* idx_dev, float* out_dev, int32_t chunk_rows, float summary[11], void* stream);
/* Five row-major device arrays (any row strides; b->rows of any size >= 1, b->idx_dev NULL) -> packed rows of stride
 * iqlhip_row_stride at rows_out_dev, pad columns zero: what iqlhip_step does to a batch in front of its forward, into
 * the caller's block — the way a five-tensor batch reaches iqlhip_score_rows. */
int iqlhip_pack_rows(iqlhip_ctx* ctx, const iqlhip_batch* b, float* rows_out_dev, void* stream);

/* ---- trainer groups -------------------------------------------------------------------------------------------
 * K independent agents (contexts) of the same shape stepped together: every kernel launch of a group step covers all
 * K agents (seed sweeps and hyper-parameter sweeps of one configuration on one GPU).  Each agent keeps its own arenas,
 * Adam state, target nets, scratch, scalars and batches; after a group call every member is exactly where the same
 * steps run alone (iqlhip_step / iqlhip_train_steps) would have left it, bit for bit.
 * Members: 1..IQLHIP_MAX_GROUP distinct contexts on one device with equal state / action dims, policy kind and
 * precision; no data-parallel exchange; actor dropout (iqlhip_set_dropout with p > 0) only in a group created with
 * IQLHIP_GROUP_DROPOUT (IQLHIP_EUNSUPPORTED otherwise).  Batches: one size for all members through iqlhip_group_step /
 * _train_steps / _online_step, a size per member through their _mixed forms (the same launches: each launch's grid is
 * the largest member's, a member's record bounds its own work); small-batch kernels only (bf16: at most 512 rows per
 * member).  A group call invalidates each member's train_steps continuation
 * (the staging buffer is overwritten); the group's own bursts with importance-sampling weights may continue each other
 * (IQLHIP_GROUP_TS_CONTINUE).  Per-row loss weights, importance-sampling weights and prioritised replay are fp32 only, in
 * a group as alone.  The members must outlive the group; a context that is destroyed or re-created
 * means a new group. */
#define IQLHIP_MAX_GROUP 16
#define IQLHIP_GROUP_MAX_STEPS 1024   /* steps per iqlhip_group_train_steps call */
typedef struct iqlhip_group iqlhip_group;
/* iqlhip_group_create_flags with flags = 0. */
int iqlhip_group_create(iqlhip_ctx* const* members, int k, iqlhip_group** out);
/* flags & IQLHIP_GROUP_DROPOUT: members may train with actor dropout, each with its own rate (0 included), seed and
 * stream position.  Every training call draws member k's keep-bits exactly as its solo call would — key drop_seed,
 * the member's threshold, position drop_step — in the group's own launches, and moves the position as the solo call
 * does: iqlhip_group_step / iqlhip_group_online_step by one for a member that draws, iqlhip_group_train_steps by n
 * for every member with a rate above 0 (a rate of 0 never moves a position).  Masks written by
 * iqlhip_debug_write_masks are kept (no draw for that member).  The inference
 * forwards are eval-mode for every member without an inference rate (iqlhip_set_act_dropout; a member with one needs
 * this flag too).  Unknown flag bits: IQLHIP_EINVAL, checked before any member is looked at; *out is
 * written on success only. */
#define IQLHIP_GROUP_DROPOUT 1
int iqlhip_group_create_flags(iqlhip_ctx* const* members, int k, int32_t flags, iqlhip_group** out);
int iqlhip_group_destroy(iqlhip_group* group);
/* One step per member on caller-given batches (batches[k], sc[k]); out[3k] (value, q, actor per member) or NULL.
 * With out != NULL the call synchronises `stream`. */
int iqlhip_group_step(iqlhip_group* group, const iqlhip_batch* batches, const iqlhip_step_scalars* sc, float* out,
                      void* stream);
/* iqlhip_group_step where batches[k].rows may differ from member to member (1 <= rows <= member k's max_batch; bf16:
 * <= 512): member k ends exactly where iqlhip_step on batches[k] leaves it.  Any group takes it; with equal rows it
 * is iqlhip_group_step.  Everything is checked, per member, before any device work or counter change. */
int iqlhip_group_step_mixed(iqlhip_group* group, const iqlhip_batch* batches, const iqlhip_step_scalars* sc, float* out,
                            void* stream);
/* n steps per member with row indices drawn on the device: member k draws from rows[k] (packed rows, stride ld,
 * size[k] rows) under (seeds[k], offsets[k]) exactly as iqlhip_train_steps(..., seed, stream_offset) does, and takes
 * its per-step scalars from tables[k] (n x iqlhip_step_scalars, host memory, free again on return).  The losses of
 * every step go to a per-member ring read by iqlhip_group_read_losses.  flags: reserved (0). */
int iqlhip_group_train_steps(iqlhip_group* group, const float* const* rows, int64_t ld, const int64_t* size, int32_t B,
                             const void* const* tables, int32_t n, const uint64_t* seeds, const uint64_t* offsets,
                             int32_t flags, void* stream);
/* iqlhip_group_train_steps with a batch size per member, B[k] (NULL: IQLHIP_EINVAL): step s of member k draws the
 * indices j = s * B[k] + r, r < B[k], of its own stream — exactly what iqlhip_train_steps with batch B[k] draws; n is
 * common to the call.  The checks of iqlhip_group_train_steps apply per member, before any device work. */
int iqlhip_group_train_steps_mixed(iqlhip_group* group, const float* const* rows, int64_t ld, const int64_t* size,
                                   const int32_t* B, const void* const* tables, int32_t n, const uint64_t* seeds,
                                   const uint64_t* offsets, int32_t flags, void* stream);
/* out[k][n][3]: the losses of the first n steps of the last group call; synchronises `stream`. */
int iqlhip_group_read_losses(iqlhip_group* group, float* out, int32_t n, void* stream);
/* out[n][K][IQLHIP_N_STATS]: the statistics of the first n steps of the last group step / train_steps / online_step
 * call (iqlhip_set_step_stats is a per-member setting: the rows of members that had it off are NaN); a member's
 * statistics are bit-identical to those of the same steps run alone.  Synchronises `stream`. */
int iqlhip_group_read_step_stats(iqlhip_group* group, float* out, int32_t n, void* stream);
/* One online-loop iteration per member (iqlhip_online_step for each member k, in one set of launches and one
 * synchronisation): row_host[k][ld] is stored at ring row pointer[k] of rows_dev[k] (capacity[k] rows, stride ld; no
 * two members' rings may overlap), the rows rows_dev[k][idx_host[k][0..n)] are gathered and one step runs on them with
 * scalars sc[k]; out[k][3] receives the losses.  act_state_host != NULL ([k][state_dim]) additionally evaluates
 * actor.act(state) with member k's updated policy for every k with act_mask[k] != 0 (act_mask == NULL: every
 * member) into act_out_host[k][action_dim], with max_action[k] and the device noise of act_seed[k] (0: the mean
 * action) as in iqlhip_online_step.  Host arrays are ordinary memory.  Everything is checked before any device work:
 * the iqlhip_online_step checks per member, the group checks, indices within capacity[k] (IQLHIP_EINDEX).
 * Synchronous. */
int iqlhip_group_online_step(iqlhip_group* group, float* const* rows_dev, int64_t ld, const int64_t* capacity,
                             const int64_t* pointer, const float* row_host, const int64_t* idx_host, int32_t n,
                             const iqlhip_step_scalars* sc, float* out, const float* act_state_host,
                             const int32_t* act_mask, const float* max_action, const uint64_t* act_seed,
                             float* act_out_host, void* stream);
/* iqlhip_group_online_step with a batch size per member, n[k] (NULL: IQLHIP_EINVAL): idx_host holds the members' index
 * lists one after another, member k's n[k] indices starting at n[0] + ... + n[k-1].  The same checks, per member. */
int iqlhip_group_online_step_mixed(iqlhip_group* group, float* const* rows_dev, int64_t ld, const int64_t* capacity,
                                   const int64_t* pointer, const float* row_host, const int64_t* idx_host,
                                   const int32_t* n, const iqlhip_step_scalars* sc, float* out,
                                   const float* act_state_host, const int32_t* act_mask, const float* max_action,
                                   const uint64_t* act_seed, float* act_out_host, void* stream);
/* ---- group vector-environment online step ----------------------------------------------------------------------
 * iqlhip_online_step_vec ("vector-environment online step" above) for each member k, in one set of launches, one upload
 * and one synchronisation: member k's n_rows[k] new rows go to ring rows (pointer[k] + j) mod capacity[k]
 * of rows_dev[k], n_updates steps run on batches of batch_rows[k] rows, and its policy, as the steps left it, acts on
 * act_rows[k] states.  n_updates is common to the call: the members' steps run in lockstep.
 *   rows_host        the members' new rows one member after another, n_rows[k] rows of ld floats each
 *   idx_host         the members' n_updates * batch_rows[k] indices one member after another, step by step (each step's
 *                    batch_rows[k] indices a sample() draw over the member's size after all its inserts)
 *   sc[k][u]         step u's scalars of member k (sc[k * n_updates + u]);  out[k][u][3]: its losses
 *   act_states_host  NULL: no member acts; else the members' act states one member after another, act_rows[k] rows of
 *                    state_dim floats each (act_rows[k] = 0: none for member k), with max_action[k] and the device noise
 *                    of act_seed[k] (0: the mean action) as in iqlhip_online_step_vec, into act_out_host, packed alike
 *                    with action_dim floats a row
 * Launches, whatever the group's size: one (iql_online_vec_gather_group_kernel, grid.y = member: the ring writes, the
 * gathers into a staging block [k][n_updates][batch_rows[k]][ld] the group owns — sized on first use, grown when a call
 * needs more — and the act states' packing; a drawn index i with (i - pointer[k]) mod capacity[k] < n_rows[k] is read
 * from the host words, never from the ring), then n_updates times the launches of iqlhip_group_step_mixed — step u on
 * slice u of every member's staging, its statistics in slot u of what iqlhip_group_read_step_stats reads, the clip record
 * the last step's — then iqlhip_group_actor_forward's policy forward and rows finish over the requesting members and a
 * one-block launch that stores the completion word the host spins on; n_updates = 0 with no act ends on a stream
 * synchronisation.  Every requesting member's noise and inference keep-bit counters advance once, every drawing
 * member's keep-bit position by n_updates.  Host arrays are ordinary memory (copied into pinned staging inside the
 * call); idx_host, sc and out may be NULL when n_updates = 0.  Member k ends bit for bit where its iqlhip_online_step_vec
 * call leaves it.  Synchronous.
 * Refused before anything is launched or any counter moves, naming the member — IQLHIP_EINVAL: a NULL argument, a NULL or
 * misaligned ring, ld other than the row stride, a pointer outside its ring, rings that overlap, n_rows[k] outside
 * [1, min(capacity[k], IQLHIP_VEC_MAX_ENVS)], n_updates outside [0, IQLHIP_VEC_MAX_UPDATES], act_rows[k] outside
 * [0, IQLHIP_VEC_MAX_ENVS], batch_rows[k] outside [1, min(512, max_batch)]; IQLHIP_EINDEX: an index outside
 * [0, capacity[k]); IQLHIP_EUNSUPPORTED: the group rules (an exchange, bf16 batches of more than 512 rows, dropout
 * without IQLHIP_GROUP_DROPOUT), injected keep-bits pending, and — n_updates > 0 only, as in the solo call — what
 * statistics and clipping refuse. */
int iqlhip_group_online_step_vec(iqlhip_group* group, float* const* rows_dev, int64_t ld, const int64_t* capacity,
                                 const int64_t* pointer, const float* rows_host, const int32_t* n_rows,
                                 const int64_t* idx_host, const int32_t* batch_rows, int32_t n_updates,
                                 const iqlhip_step_scalars* sc, float* out, const float* act_states_host,
                                 const int32_t* act_rows, const float* max_action, const uint64_t* act_seed,
                                 float* act_out_host, void* stream);
/* Group calls on batches mixed from two replay buffers ("mixed offline / online batches" above, for every member in one
 * set of launches; "replay2" because _mixed already names the per-member batch sizes above).  One pair serves equal
 * and unequal batch sizes: every count is per member.
 * iqlhip_group_online_step_replay2 is iqlhip_online_step_mixed for each member k: n[k] is the step's whole row count,
 * the first n_off[k] of member k's n[k] indices (idx_host, laid out as for iqlhip_group_online_step_mixed) address
 * rows_off_dev[k] (size_off[k] rows, stride ld, read only; members may share one), the other n[k] - n_off[k] its ring.
 * Checked before any device work, per member, on top of iqlhip_group_online_step_mixed's checks: NULL or misaligned
 * offline rows, size_off[k] < 1, n_off[k] outside [1, n[k] - 1], a ring that overlaps any member's offline rows
 * (IQLHIP_EINVAL); offline indices within size_off[k], online ones within capacity[k] (IQLHIP_EINDEX); an exchange or
 * more than 512 bf16 rows (IQLHIP_EUNSUPPORTED, the group rules). */
int iqlhip_group_online_step_replay2(iqlhip_group* group, float* const* rows_dev, int64_t ld, const int64_t* capacity,
                                     const int64_t* pointer, const float* row_host, const int64_t* idx_host,
                                     const int32_t* n, const iqlhip_step_scalars* sc, float* out,
                                     const float* act_state_host, const int32_t* act_mask, const float* max_action,
                                     const uint64_t* act_seed, float* act_out_host, void* stream,
                                     const float* const* rows_off_dev, const int64_t* size_off, const int32_t* n_off);
/* iqlhip_group_train_steps_replay2 is iqlhip_train_steps_mixed for each member k: step s draws the indices j = s * B[k]
 * + r, r < B[k], of the member's stream (seeds[k], offsets[k]); row r < n_off[k] maps its bits over size_off[k] into
 * rows_off[k], the others over size_on[k] into rows_on[k].  Losses, statistics and scalar tables as
 * iqlhip_group_train_steps.  Checked before any device work, per member, on top of iqlhip_group_train_steps_mixed's
 * checks: NULL or misaligned rows_on[k], rows_on[k] == rows_off[k], an empty buffer, n_off[k] outside [1, B[k] - 1]
 * (IQLHIP_EINVAL). */
int iqlhip_group_train_steps_replay2(iqlhip_group* group, const float* const* rows_off, const int64_t* size_off,
                                     const float* const* rows_on, const int64_t* size_on, int64_t ld, const int32_t* B,
                                     const int32_t* n_off, const void* const* tables, int32_t n, const uint64_t* seeds,
                                     const uint64_t* offsets, void* stream);
/* iqlhip_group_train_steps_mixed with member k's rows drawn by wtabs[k] ("weighted replay sampling" above; a NULL
 * entry: that member draws uniformly, exactly as iqlhip_group_train_steps_mixed would): iqlhip_train_steps_weighted for
 * each member with a table, in the group's launches.  B is per member: one entry point serves equal and unequal batch
 * sizes.  Members may share one table.  A weighted draw consumes the counters a plain one does: stream positions,
 * dropout positions, losses, statistics and scalar tables all as iqlhip_group_train_steps_mixed; every member's solo
 * continuation (IQLHIP_TS_CONTINUE) is invalidated, as after any group call.  Each step's rows are gathered by a launch
 * of its own between the steps (one wave resolves an index and copies that row).  Checked before any device work or
 * counter change, on top of iqlhip_group_train_steps_mixed's checks: wtabs == NULL, a table whose n differs from
 * size[k] (so that every index it can resolve is < size[k]), a table on another device than the group (IQLHIP_EINVAL,
 * naming the member); an exchange or more than 512 bf16 rows (IQLHIP_EUNSUPPORTED, the group rules).  Two-source
 * (replay2) weighted batches do not exist.  Every table must outlive the call's queued work (iqlhip_weights_free waits
 * for the device before it frees).  flags: reserved (0). */
int iqlhip_group_train_steps_weighted(iqlhip_group* group, const float* const* rows, int64_t ld, const int64_t* size,
                                      const int32_t* B, const void* const* tables, int32_t n, const uint64_t* seeds,
                                      const uint64_t* offsets, int32_t flags, void* stream,
                                      const iqlhip_weights* const* wtabs);
/* Per-row loss weights, importance-sampling weights and prioritised replay for every member in the group's launches
 * (DESIGN.md 6j "trainer groups").  fp32 only; everything below is refused before anything is launched and before any
 * counter moves, the message naming the member.
 * iqlhip_group_step_rw is iqlhip_group_step_mixed with member k's loss terms weighted by row_w_dev[k][0 .. rows_k) and
 * its TD errors (q1 - y, q2 - y) stored to td_out_dev[k] ([rows_k][2] fp32, 8-byte aligned): member k ends bit for bit
 * where iqlhip_step_rw leaves it.  row_w_dev[k] == NULL: weights of 1.0f (a vector the group keeps); td_out_dev[k] ==
 * NULL: nothing is stored for that member.  Both ARRAYS must be given (IQLHIP_EINVAL); a bf16 member: IQLHIP_EUNSUPPORTED.
 * iqlhip_group_train_steps_weighted_is is iqlhip_group_train_steps_weighted whose steps weight member k's loss terms by
 * c = (q_min / q_row)^is_beta[k] — iqlhip_train_steps_weighted_is for each member with a table.  A member without one
 * (wtabs[k] == NULL) draws uniformly with c = 1 and ends where iqlhip_train_steps leaves it.
 * iqlhip_group_train_steps_prioritized is iqlhip_train_steps_prioritized for each member, lag of one step included.  Per
 * call: the rows of step 0 by every member's table as it stands; then per step s: the rows of step s + 1 into the members'
 * other staging halves (they see the updates of steps < s), step s with its loss weights, and wtabs[k][rows of s] <-
 * td_priority(TD errors of s; alpha[k], eps[k]) for all members in three launches.  One linear chain on `stream`.
 * flags: IQLHIP_GROUP_TS_CONTINUE — the call may start on the rows this group's previous call staged.  It is honoured
 * per member under the rules of IQLHIP_TS_CONTINUE: the previous call on the member was this group's, of the same kind
 * and of an even number of steps, on the same rows / size / B[k] / seed with offsets[k] where it stopped (an odd B[k]
 * never is: the member draws afresh), its table at the generation and version that call left, dropout settings and
 * position unchanged.  Any other group or solo call on a member invalidates its staged rows.  At most
 * IQLHIP_GROUP_MAX_STEPS steps per call; a caller that wants a result to depend on the tables alone passes the flag only
 * between the pieces of one burst (the Python layer does).  A prioritised call moves every table's version by 1.
 * Refused on top of iqlhip_group_train_steps_weighted's checks: unknown flag bits, a NULL is_beta / alpha / eps array, an
 * is_beta[k] that is negative or not finite (IQLHIP_EINVAL); a bf16 member, pending injected keep-bits
 * (IQLHIP_EUNSUPPORTED).  The prioritised call also: a NULL wtabs[k], a static table, alpha[k] / eps[k] negative, not
 * finite or both 0, one table given to two members — their updates would race, and "what the solo call leaves" would mean
 * nothing; sharing the ROWS is fine — (IQLHIP_EINVAL); more than 65 536 rows per batch (IQLHIP_EUNSUPPORTED). */
#define IQLHIP_GROUP_TS_CONTINUE 1
int iqlhip_group_step_rw(iqlhip_group* group, const iqlhip_batch* batches, const iqlhip_step_scalars* sc,
                         const float* const* row_w_dev, float* const* td_out_dev, float* out, void* stream);
int iqlhip_group_train_steps_weighted_is(iqlhip_group* group, const float* const* rows, int64_t ld, const int64_t* size,
                                         const int32_t* B, const void* const* tables, int32_t n, const uint64_t* seeds,
                                         const uint64_t* offsets, int32_t flags, void* stream,
                                         const iqlhip_weights* const* wtabs, const float* is_beta);
int iqlhip_group_train_steps_prioritized(iqlhip_group* group, const float* const* rows, int64_t ld, const int64_t* size,
                                         const int32_t* B, const void* const* tables, int32_t n, const uint64_t* seeds,
                                         const uint64_t* offsets, int32_t flags, void* stream,
                                         iqlhip_weights* const* wtabs, const float* is_beta, const float* alpha,
                                         const float* eps);
/* Policy inference for every member of a group in one set of launches.  Member k maps its rows[k] states
 * (row stride ld_s) to rows[k] actions (row stride ld_a), exactly as iqlhip_actor_forward (seeds[k] == 0: the mean)
 * or iqlhip_actor_sample (seeds[k] != 0: device N(0,1) noise, member k's act() call counter advances by one) on that
 * member would, with max_action[k].  rows[k] == 0 skips member k and leaves its counter alone.  rows[k] <=
 * max(max_batch_k, IQLHIP_ACT_ROWS).  states / actions may be device memory or host-mapped pinned memory.  Eval-mode
 * forward, except for members with an inference rate (iqlhip_set_act_dropout): those draw their keep-bits as their solo
 * call would, in the same launches.  Checked before any device work or counter change: NULL arguments, unbound members, row
 * counts, strides, NULL pointers of members with rows, the group rules, unknown flags.  Asynchronous on `stream`
 * (successive calls of one group on one stream); flags & IQLHIP_GROUP_ACT_WAIT: returns once every action is written
 * (the host spins on a completion word instead of synchronising the stream: the form for host-mapped actions). */
#define IQLHIP_GROUP_ACT_WAIT 1
int iqlhip_group_actor_forward(iqlhip_group* group, const float* const* states, int64_t ld_s, const int32_t* rows,
                               const uint64_t* seeds, const float* max_action, float* const* actions, int64_t ld_a,
                               int32_t flags, void* stream);

/* ---- group scoring (DESIGN.md 6h "group scoring") -----------------------------------------------------------------
 * iqlhip_score_rows for every member of a group in one set of launches (grid.y = member): per chunk one forward, one
 * row kernel, one spread kernel (spread_dev given) and one finish kernel (summary given), whatever K is (chunks of a
 * few thousand rows and more: the forward as a few launches over some of the members each, where that fills the device).
 * Rows: member k scores the n rows [row0, row0 + n) of rows_dev[k] (n_rows[k] packed rows of stride ld, as
 * iqlhip_score_rows), or, with idx_dev, the n rows idx_dev[k][0 .. n) names, in that order.  rows_dev, n_rows, idx_dev
 * and out_dev are host tables of K entries; pointers may repeat across members (one shared buffer, one shared index
 * list).  One n for all members.
 * Outputs: out_dev NULL, or K pointers, each NULL (no per-row store for that member) or a 16-byte aligned
 * [n][IQLHIP_N_SCORE] array; summary NULL, or K x 11 host floats, member k's at summary + 11 k in iqlhip_score_rows'
 * order; spread_dev NULL, or [n][2 * IQLHIP_N_SCORE] floats, 16-byte aligned.  At least one of the three (an out_dev
 * table of K NULLs counts as none).
 * Spread: spread[i][j] = the mean over members of member k's column j of ITS i-th row, spread[i][8 + j] the population
 * standard deviation of the same K values, in fixed fp32 arithmetic, members in order 0 .. K - 1:
 *   mean = (x_0 + x_1 + ...) / K        dev = sqrtf((sum_k (x_k - mean)^2) / K)       (two passes, no fused multiply-add)
 * Meaningful when all members score the same rows; that is not checked.  Available with every out_dev entry NULL.
 * Which groups: every kind — plain, IQLHIP_GROUP_DROPOUT, members of different batch sizes, bf16 members.  As in the
 * solo call the policy runs without dropout, parameters are the fp32 masters, the arithmetic is fp32 MFMA; each member
 * uses its own hyper (beta, iql_tau, discount, exp_adv_max).
 * Bitwise: member k's eight floats of a row are those iqlhip_score_rows on member k's context writes for that row —
 * whatever K, the member's place in the group, n, chunk_rows, the grid, range or index addressing.  Member k's summary
 * is bit for bit the solo call's over the same rows cut into the same chunks (other cuts: the last bits, as there).
 * chunk_rows: rows of a member per launch sequence; 0 = the cap floor(65 536 / K / 32) * 32, larger values are cut to
 * it.  The scratch belongs to the group, is sized by that cap (the K members together take what one solo context's
 * scratch takes, plus [K][cap][8] floats for the rows of members without an out), is allocated whole or not at all by
 * the group's first scoring call and released by iqlhip_group_destroy.  The members' own scoring scratch, and
 * everything else iqlhip_score_rows leaves alone, is left alone here too.
 * Before anything is launched: IQLHIP_EINVAL for a NULL group, table or entry, n < 1, a range outside any member's
 * [0, n_rows[k]], a bad ld, chunk_rows or alignment, nothing to write; IQLHIP_ENOTBOUND for an unbound member.  Index
 * lists are checked on the device by ONE launch over all members and one host wait, no row read: IQLHIP_EINDEX, and
 * iqlhip_last_error names the member and the index.
 * Synchronises `stream` when idx_dev or summary is given; otherwise it only queues work.  The call's records travel in
 * stream order, and an upload is skipped when they equal the last one's: a group's asynchronous scoring calls must all
 * be queued on ONE stream (back to back they each use their own records); a call on another stream has no order
 * against an upload still in flight, so synchronise before changing streams. */
int iqlhip_group_score_rows(iqlhip_group* group, const float* const* rows_dev, int64_t ld, const int64_t* n_rows,
                            int64_t row0, int64_t n, const int64_t* const* idx_dev, float* const* out_dev,
                            float* spread_dev, int32_t chunk_rows, float* summary /* [K][11] or NULL */, void* stream);

/* ---- policy inference ---------------------------------------------------- */
/* GaussianPolicy.act (algorithms/finetune/iql.py:371-379), DeterministicPolicy.act (:404-413) and the batched policy
 * forward of evaluation loops (eval_actor, jsrl_w_iql.py:62-179):
 *   actions[r] = clamp(max_action * (tanh(MLP_pi(states[r])) + exp(clamp(log_std)) * noise[r]), -max_action, max_action)
 * noise_dev == NULL gives the mean (eval mode, or the deterministic policy); with a Gaussian policy in training mode
 * the caller passes standard-normal noise [rows][action_dim] (dist.sample() of iql.py:376).  Dropout is applied only at
 * the rate iqlhip_set_act_dropout has set (default 0: eval-mode forward).  rows <= max(max_batch, IQLHIP_ACT_ROWS) per call.  Uses the bound parameter arena;
 * asynchronous on `stream`.  states / noise / actions may be device memory or host-mapped (pinned) memory. */
#define IQLHIP_ACT_ROWS 4096
int iqlhip_actor_forward(iqlhip_ctx* ctx, const float* states_dev, int64_t ld_s, int32_t rows, const float* noise_dev,
                         int64_t ld_noise, float max_action, float* actions_dev, int64_t ld_a, void* stream);

/* The training-mode act() of a Gaussian policy with the N(0,1) draw of dist.sample() (iql.py:376) made on the device
 * (Philox4x32-10 keyed by `seed` != 0, counter = (element, call number kept by the context), Box-Muller). */
int iqlhip_actor_sample(iqlhip_ctx* ctx, const float* states_dev, int64_t ld_s, int32_t rows, uint64_t seed,
                        float max_action, float* actions_dev, int64_t ld_a, void* stream);

/* Block the host until everything queued on `stream` has finished (hipStreamSynchronize): the completion point of
 * iqlhip_actor_forward when its buffers are host-mapped, i.e. the `.cpu()` of the reference's act() (iql.py:379). */
int iqlhip_stream_synchronize(void* stream);

/* ---- JSRL action selection (DESIGN.md 6k "JSRL action selection") ----------------------------------------------------
 * jsrl_utils.learner_or_guide_action for K >= 1 (learner, guide, gate) triples of bound contexts in one set of launches:
 * member k's states are packed once, ONE forward launch runs the policy instance of the learners and the guides and
 * the value instance V(s) of the gates the call needs (the existing forward body behind a record table, as
 * iqlhip_group_actor_forward runs it; contexts of different precision take one launch per precision), and ONE finish
 * launch decides per row and writes action, flag and gate value.  Three launches for any K.
 * A handle ties the triples together.  1 <= k <= IQLHIP_MAX_GROUP; all contexts on one device; learner and guide of a
 * member have equal state_dim and action_dim (the policy kind may differ), its gate (gates == NULL or gates[k] == NULL:
 * none) the same state_dim.  Learner and guide may be the same context, and a context may serve several members.  The
 * handle owns the packed states and the head partials of every member (sized by the smallest act capacity of its
 * triple), so the contexts' own inference scratch is left alone.  The contexts must outlive the handle.
 * Selection, per row r of member k:  who[k][r] = 0: the guide acts; 1: the learner acts; 2: the gate decides,
 *   h = V_gate(states[k][r])  (the value network of the gate context),   use_learner = (h <= gate_max[k])  in fp32.
 * Every host-known part of the reference's horizon rules (time step against stage, goal distance, ep_agent_type <=
 * agent_type_stage, the last stage, a NaN stage, the agent_type rule's host random draw) is folded into `who` by the
 * caller; the device evaluates only the state-dependent gate.  who and gate_max are HOST arrays, read during the call.
 * Actions: a learner row is exactly what iqlhip_actor_forward (seeds[k] == 0) or iqlhip_actor_sample (seeds[k] != 0) on
 * the learner writes for that row of the same states array, with max_action_learner[k]; a guide row is the guide's
 * eval-mode mean (iqlhip_actor_forward without noise) with max_action_guide[k].
 * Counters: with seeds[k] != 0 and rows[k] > 0 the LEARNER's act() call counter advances by one per call, whatever the
 * rows chose — also when `who` is 0 for every row: the gate's outcome is not known to the host, so "one call, one
 * number" is the only rule that can be kept for all `who` alike.  The guide's and the gate's counters never move.
 * use_learner[k] (NULL table or entry: not written) receives 0 / 1 per row.  gate_out[k] (NULL: not written) receives h
 * for every row of a member with a gate.  The gate forward runs for a member that has a `2` or a gate_out entry; the
 * learner forward for one that has a `1` or a `2`; the guide forward for one that has a `0` or a `2`.
 * rows[k] == 0 skips member k (no launch, no counter).  Each context runs at its own precision, as in its solo call;
 * the shadows of bf16 contexts are refreshed first.  flags & IQLHIP_GROUP_ACT_WAIT as in iqlhip_group_actor_forward;
 * without it the call is asynchronous on `stream` (successive calls of one handle on one stream).
 * Checked before any launch or counter change: IQLHIP_EINVAL for a NULL handle, table or entry (of a member with
 * rows), dims that differ as said above, rows[k] above the smallest act capacity of the triple, a stride smaller than
 * the row, a who value outside 0..2, who == 2 (or a gate_out entry) on a member without a gate, unknown flags;
 * IQLHIP_ENOTBOUND for an unbound context; IQLHIP_EUNSUPPORTED when a learner or guide has an inference dropout rate
 * (iqlhip_set_act_dropout): compose the solo calls for those. */
typedef struct iqlhip_jsrl iqlhip_jsrl;
int iqlhip_jsrl_create(iqlhip_ctx* const* learners, iqlhip_ctx* const* guides, iqlhip_ctx* const* gates, int k,
                       iqlhip_jsrl** out);
int iqlhip_jsrl_destroy(iqlhip_jsrl* jsrl);
int iqlhip_jsrl_act(iqlhip_jsrl* jsrl, const float* const* states, int64_t ld_s, const int32_t* rows,
                    const int8_t* const* who, const float* gate_max, const uint64_t* seeds,
                    const float* max_action_learner, const float* max_action_guide, float* const* actions, int64_t ld_a,
                    int32_t* const* use_learner, float* const* gate_out, int32_t flags, void* stream);
/* Selection by the critic (DESIGN.md 6k "who == 3"): iqlhip_jsrl_act plus one more byte.  A row of member k with
 * who[k][r] = 3 takes whichever of the two proposed actions the member's twin critic values more:
 *   a_g = the guide's eval-mode mean for the row (bit for bit a who == 0 row), a_l = the learner's action (bit for bit
 *   a who == 1 row of the same call, device noise of (seeds[k], call) at element r * A + d included), both after the
 *   scale by max_action and the clamp;
 *   qg = min(Q1, Q2)(s, a_g), ql = min(Q1, Q2)(s, a_l)  in fp32, head partials summed in the step's fixed order;
 *   q_inv_temp[k] infinite, or seeds[k] == 0:  use_learner = (ql >= qg)   (a tie goes to the learner);
 *   else  p = 1 / (1 + expf(-(ql - qg) * q_inv_temp[k])),  use_learner = (u < p),  u = ((c[2] >> 8) + 0.5) * 2^-24 of
 *   the Philox block the act() noise stream already draws for element r * A (key, counter and tag 0xAC7 unchanged;
 *   words 0 and 1 are its Box-Muller pair) — no new stream, no new counter.
 * The output row is the chosen candidate, bit for bit.  The critic is the twin Q of the context set by
 * iqlhip_jsrl_set_critics — critics == NULL or critics[k] == NULL: the member's learner; otherwise a bound context on
 * the learner's device with its state_dim and action_dim (IQLHIP_EINVAL / IQLHIP_ENOTBOUND), e.g. a frozen offline
 * critic.  It runs at its own precision.  The contexts must outlive the handle.
 * Launches: a call without a `3` launches exactly what iqlhip_jsrl_act launches.  With one, five for any K: pack (the
 * states also into both halves of the critic's rows), the policy and gate forwards, candidates (the finish launch,
 * which finishes rows with 0..2 as before and writes [s | a_g] to row r and [s | a_l] to row n + r of the critic's
 * packed act rows), ONE Q forward per precision kind (two records per member, instances Q1 and Q2, over 2 n rows),
 * select.  The handle owns those rows and partials (allocated by the first call that has a `3`).
 * q_out[k] (NULL table or entry: not written) receives [rows[k]][4] floats (Q1g, Q2g, Q1l, Q2l) per row, NaN on rows
 * whose byte is not 3.  Counters as in iqlhip_jsrl_act; the critic's never move.
 * Checked before any launch or counter change, on top of iqlhip_jsrl_act's checks (who in 0..3 here): IQLHIP_EINVAL for
 * q_inv_temp[k] negative or NaN, a `3` with q_inv_temp == NULL, a q_out entry on a member without a `3`, 2 * rows[k]
 * above the smallest act capacity of learner, guide, gate and critic for a member with a `3`; IQLHIP_ENOTBOUND for an
 * unbound critic.  iqlhip_jsrl_act and iqlhip_jsrl_online_step still refuse a `3`. */
int iqlhip_jsrl_set_critics(iqlhip_jsrl* jsrl, iqlhip_ctx* const* critics);
int iqlhip_jsrl_act_q(iqlhip_jsrl* jsrl, const float* const* states, int64_t ld_s, const int32_t* rows,
                      const int8_t* const* who, const float* gate_max, const uint64_t* seeds,
                      const float* max_action_learner, const float* max_action_guide, float* const* actions, int64_t ld_a,
                      int32_t* const* use_learner, float* const* gate_out, const float* q_inv_temp, float* const* q_out,
                      int32_t flags, void* stream);
/* One online iteration of a K = 1 handle's learner plus the next action's selection, under ONE synchronisation: the
 * ring write, gather and step of iqlhip_online_step without an act (same arguments, same checks), then the one-row
 * selection above with the just-updated learner — state, action, flag and h travel through host-mapped words.  Losses
 * and everything the learner holds are bit for bit what iqlhip_online_step without act_state_host leaves; action,
 * *use_learner_out and *gate_out (NULL: not returned, and no gate forward unless who == 2) are what iqlhip_jsrl_act
 * gives when called afterwards with the same arguments.  act_seed != 0 advances the learner's act() counter by one (the
 * rule above).  who == 2 or gate_out on a handle without a gate, K != 1, and every check of the two calls it stands
 * for: before any launch or counter change. */
int iqlhip_jsrl_online_step(iqlhip_jsrl* jsrl, float* rows_dev, int64_t ld, int64_t capacity, int64_t pointer,
                            const float* row_host, const int64_t* idx_host, int32_t n, const iqlhip_step_scalars* sc,
                            float out[3], const float* act_state_host, int8_t who, float gate_max, uint64_t act_seed,
                            float max_action_learner, float max_action_guide, float* act_out_host,
                            int32_t* use_learner_out, float* gate_out, void* stream);

/* ---- introspection (tests, profiling) ----------------------------------- */
/* Copy a named library-owned scratch array to host (synchronous).  Names:
 * "h0","h1" (activations [4][max_batch][256]), "heads" (partial head sums),
 * "grads" (flat summed gradient, n_params), "loss_parts", "xb" (the library's packed staging batch [max_batch][row
 * stride]: the rows of the last step that did not consume a packed block in place), "drop_bits" (the training steps' keep-bit words,
 * [2 layers][max_batch][8]), "act_drop_bits" (the last inference call's, [2 layers][max(max_batch, IQLHIP_ACT_ROWS)][8];
 * only after iqlhip_set_act_dropout with p > 0). */
int iqlhip_debug_read(iqlhip_ctx* ctx, const char* name, float* host_out, int64_t max_floats, int64_t* n_out,
                      void* stream);
/* Micro-benchmark hook: `repeat` back-to-back launches of one kernel of the step (0 fwd, 1 bwd,
 * 2 update with zero step size, 3 all three); average microseconds per launch.  Synchronous. */
int iqlhip_debug_time_kernel(iqlhip_ctx* ctx, const iqlhip_batch* batch, int which, int repeat, float* avg_us,
                             void* stream);
/* Diagnostic: queue a flag kernel on `stream` and spin on its host-mapped word (no synchronise call): microseconds
 * until the host sees the stream drained. */
int iqlhip_debug_drain_spin(iqlhip_ctx* ctx, void* stream, double* spin_us);
/* Tests: the device buffers, pinned buffers and events this process's contexts and groups hold right now (what
 * iqlhip_destroy / iqlhip_group_destroy release; cached graphs and the P2P exchange block are not counted). */
int64_t iqlhip_debug_live_buffers(void);
/* Tests: how many training forwards this context has LAUNCHED OR CAPTURED as iql_fwd_kernel_early (the one-slice fp32
 * forward with preloaded arguments; every other forward is iql_fwd_kernel or a chunk kind's kernel).  -1: null context. */
int64_t iqlhip_debug_fwd_early_launches(const iqlhip_ctx* ctx);
/* Average device time (microseconds) of the kernels of the last iqlhip_step /
 * train_steps call measured with hipEvents on `stream`; 0 when timing is off. */
int iqlhip_set_timing(iqlhip_ctx* ctx, int enabled);
int iqlhip_get_timing(iqlhip_ctx* ctx, float out_us[4]); /* fwd, bwd, update, total */

/* ---- the JSRL variance learner (variance_learner.py VarianceLearner._update_v) ----
 * Two scalar networks S -> 256 -> 256 -> 1 behind an opaque handle of their own, independent of any iqlhip_ctx: net 0
 * is mf (the value mean), net 1 is vf (the log-variance, the `variance` horizon's gate).  fp32 only.
 *
 * The arena holds the two nets one behind the other, each laid out by iqlhip_arena_layout's per-net rule with
 * k_in = state_dim, d_out = 1 (W1, W0, b0, b1, W2, b2 padded to 4 words, the segment rounded up to 64 words).
 *
 * A step reads ONE packed device block of B * S + S + 2 B floats: B states [B][S], the last next-state [S], B rewards,
 * B next-done flags (0 or 1).  With samp[t] = reward(t) + (0.99 * next) * (1 - next_done[t]) walked from t = B - 1 down
 * (next = mf of the last next-state at t = B - 1, else samp[t + 1]; every operation rounded on its own), pred = mf(s),
 * var = clip(exp(vf(s)), 1e-4, 1e8), the loss is mean(0.5 * (log(var) + (pred - samp)^2 / var)).  reward(t) is the
 * reference's rewards[t - 1] (row 0 takes rewards[B - 1]) unless aligned_rewards is 1: then rewards[t].  The bootstrap
 * value keeps its gradient, as in the reference.  which_net names the net that is differentiated and stepped with
 * torch.optim.Adam's defaults; the other net's parameters and moments are not touched.  1 <= B <= max_rows <= 1024. */
typedef struct iqlhip_var iqlhip_var;
typedef struct iqlhip_var_scalars {
  float step_size;         /* lr / (1 - beta1^t): t the stepped net's own step count, float64 on the host */
  float bc2_sqrt;          /* sqrt(1 - beta2^t) */
  float beta2, one_minus_beta1, one_minus_beta2, eps;
  int32_t aligned_rewards; /* 0: the reference's rewards[t - 1]; 1: rewards[t] */
  int32_t reserved;
} iqlhip_var_scalars;
/* out[0], out[1]: the layouts of mf and vf inside the arena; n_params: the arena's words. */
int iqlhip_var_layout(int32_t state_dim, iqlhip_net_layout out[2], int64_t* n_params);
int iqlhip_var_create(int32_t state_dim, int32_t max_rows, int device, iqlhip_var** out);
int iqlhip_var_destroy(iqlhip_var* var);
/* The caller's arenas (device, n_params floats each): parameters and Adam's two moments. */
int iqlhip_var_bind(iqlhip_var* var, float* params, float* exp_avg, float* exp_avg_sq);
/* Forward, recurrence, backward of which_net and its Adam step, queued on `stream` (four launches). */
int iqlhip_var_step(iqlhip_var* var, const float* batch_dev, int32_t B, int32_t which_net, const iqlhip_var_scalars* sc,
                    void* stream);
/* Forward and recurrence only: samp | pred | var, [B] each, into out_dev [3][B]. */
int iqlhip_var_values(iqlhip_var* var, const float* batch_dev, int32_t B, int32_t aligned_rewards, float* out_dev,
                      void* stream);
/* Tests: the flat gradient of which_net (its segment's words, arena order, padding zero) into grad_out_dev; no update. */
int iqlhip_var_forward_backward(iqlhip_var* var, const float* batch_dev, int32_t B, int32_t which_net,
                                int32_t aligned_rewards, float* grad_out_dev, void* stream);
/* Waits for `stream`; then the loss of the last step / forward_backward / values call and, when head is not NULL, the
 * first n_head (<= B of that call) entries of its samp, pred and var: head[3][n_head]. */
int iqlhip_var_read_loss(iqlhip_var* var, float* loss, float* head, int32_t n_head, void* stream);

/* ---- the variance learner from a replay buffer (DESIGN.md 6l "From a replay buffer") ----
 * A dataset is stored in trajectory order and an online ring fills in time order, so B consecutive rows of a packed
 * replay buffer ([s | a | s' | r | d | pad], stride ld >= iqlhip_row_stride) are a rollout: the window that starts at
 * row `start` gives the packed block of a step as state t = columns [0, S) of row start + t, the last next-state =
 * columns [S + A, 2 S + A) of row start + B - 1, rewards[t] = that row's r, next_dones[t] = that row's d.  A window
 * never wraps: 0 <= start <= size - B.  Row offsets are 64-bit.
 *
 * Refused before any launch, with nothing changed (IQLHIP_EINVAL): a NULL argument, state_dim other than the handle's,
 * B outside [1, max_rows], a buffer of fewer than B rows, start < 0 or start + B beyond the buffer,
 * ld < iqlhip_row_stride(state_dim, action_dim), n_steps outside [1, IQLHIP_VAR_TRAIN_MAX_STEPS], a starts list with
 * n_starts < 1.  The handle takes the scratch of these calls (a packed block, the two rings) on first use and releases
 * it with iqlhip_var_destroy. */
#define IQLHIP_VAR_TRAIN_MAX_STEPS 1024 /* updates per iqlhip_var_train_steps call = words of the loss and start rings */
/* One launch: the packed block (B * S + S + 2 B floats) of the window at `start` into block_out_dev. */
int iqlhip_var_pack_window(iqlhip_var* var, const float* rows_dev, int64_t ld, int64_t n_rows, int32_t state_dim,
                           int32_t action_dim, int64_t start, int32_t B, float* block_out_dev, void* stream);
/* iqlhip_var_values on the window at `start` (packed into the handle's scratch): samp | pred | var into out_dev [3][B]. */
int iqlhip_var_values_window(iqlhip_var* var, const float* rows_dev, int64_t ld, int64_t n_rows, int32_t state_dim,
                             int32_t action_dim, int64_t start, int32_t B, int32_t aligned_rewards, float* out_dev,
                             void* stream);
/* n_steps updates of which_net queued on `stream` as plain launches, five per update (pack, forward, recurrence,
 * backward, Adam); no synchronisation and no host work between them.  scalars[k] are update k's (all with the same
 * aligned_rewards).  Update k draws its start row inside the pack kernel from the 64 random bits of INDEX
 * j = stream_offset + k of the index stream under `seed` at counter offset 0 — what
 * iqlhip_draw_indices(idx, n, span, seed, 0) writes to idx[j]: stream_offset counts indices, not counters, so that a
 * call may be split at any update —: start = floor(bits * span / 2^64) with span = size - B + 1, or, with a list of
 * n_starts int64 device entries, starts_dev[floor(bits * n_starts / 2^64)] (entries are the caller's to keep inside
 * [0, size - B]; the kernel clamps them there).  Word k of the start ring takes the start used, word k of the loss ring
 * the update's loss.  iqlhip_var_read_loss's words are not written by this call. */
int iqlhip_var_train_steps(iqlhip_var* var, const float* rows_dev, int64_t ld, int64_t size, int32_t action_dim, int32_t B,
                           int32_t n_steps, int32_t which_net, const iqlhip_var_scalars* scalars, uint64_t seed,
                           uint64_t stream_offset, const int64_t* starts_dev, int64_t n_starts, void* stream);
/* Waits for `stream`; then the first n_steps words of the loss ring and of the start ring of the last
 * iqlhip_var_train_steps call. */
int iqlhip_var_read_train_ring(iqlhip_var* var, float* losses_out, int64_t* starts_out, int32_t n_steps, void* stream);

/* ---- groups of variance learners (DESIGN.md 6l "Groups of learners") ----
 * K <= IQLHIP_MAX_GROUP bound iqlhip_var handles of one state_dim on one device, updated by one set of launches: every
 * launch of an update covers all members, a member's arithmetic is the solo call's (no sum crosses a member), and its
 * result is the solo call's bit for bit.  The group owns its launch records, the scalar table and K loss / start rings;
 * a member keeps its arenas, scratch and landing words, and may be stepped by the solo calls before and after a group
 * call (the group's records are written anew by every call).  Destroy the group before its members.
 *
 * Arguments with [K] are host arrays with one entry per member, in member order.  B and which_net are per call, the
 * same for every member.  Refused before any launch, with nothing changed (IQLHIP_EINVAL): NULL, K outside
 * [1, IQLHIP_MAX_GROUP], a member named twice, members of different state_dim or on different devices (create); and
 * whatever the solo call of the same name refuses, for any member — the message then starts with "member <i>: ". */
typedef struct iqlhip_var_group iqlhip_var_group;
int iqlhip_var_group_create(iqlhip_var* const* members, int k, iqlhip_var_group** out);
int iqlhip_var_group_destroy(iqlhip_var_group* group);
/* iqlhip_var_step for every member: blocks_dev[K] packed device blocks of B rows, scalars[K].  One host-to-device copy
 * of the records and scalars, then four launches.  A member's loss and samp | pred | var land in its own host-mapped
 * words: iqlhip_var_group_read_loss (or the member's iqlhip_var_read_loss) reads them. */
int iqlhip_var_group_step(iqlhip_var_group* group, const float* const* blocks_dev, int32_t B, int32_t which_net,
                          const iqlhip_var_scalars* scalars, void* stream);
/* iqlhip_var_values for every member: samp | pred | var into outs_dev[i] [3][B]. */
int iqlhip_var_group_values(iqlhip_var_group* group, const float* const* blocks_dev, int32_t B, const int32_t* aligned_rewards,
                            float* const* outs_dev, void* stream);
/* Waits for `stream` once; then every member's loss into losses[K] and, when heads is not NULL, the first n_head
 * entries of its samp, pred and var into heads[K][3][n_head]. */
int iqlhip_var_group_read_loss(iqlhip_var_group* group, float* losses, float* heads, int32_t n_head, void* stream);
/* The window forms (iqlhip_var_pack_window, the step and iqlhip_var_values_window on it): member i reads the window at
 * start[i] of the buffer rows_dev[i] (ld[i], size[i] rows, action_dim[i]); rows_dev may name one buffer K times or K
 * buffers.  One launch packs every member's window (into blocks_out_dev[i], or the member's scratch). */
int iqlhip_var_group_pack_windows(iqlhip_var_group* group, const float* const* rows_dev, const int64_t* ld, const int64_t* size,
                                  const int32_t* action_dim, const int64_t* start, int32_t B, float* const* blocks_out_dev,
                                  void* stream);
int iqlhip_var_group_step_windows(iqlhip_var_group* group, const float* const* rows_dev, const int64_t* ld, const int64_t* size,
                                  const int32_t* action_dim, const int64_t* start, int32_t B, int32_t which_net,
                                  const iqlhip_var_scalars* scalars, void* stream);
int iqlhip_var_group_values_windows(iqlhip_var_group* group, const float* const* rows_dev, const int64_t* ld, const int64_t* size,
                                    const int32_t* action_dim, const int64_t* start, int32_t B, const int32_t* aligned_rewards,
                                    float* const* outs_dev, void* stream);
/* iqlhip_var_train_steps for every member: n_steps x five group launches queued on `stream`, no synchronisation and no
 * host work between them.  scalars[n_steps][K] (update-major) travel with the records in one host-to-device copy before
 * the first launch; the kernels index the table by the update number.  Member i draws update s's start from index
 * stream_offsets[i] + s of the stream under seeds[i] — over size[i] - B + 1 values, or, where starts_dev[i] is not NULL,
 * over its n_starts[i] entries (entries of starts_dev may be NULL: that member draws from the whole buffer). */
int iqlhip_var_group_train_steps(iqlhip_var_group* group, const float* const* rows_dev, const int64_t* ld, const int64_t* size,
                                 const int32_t* action_dim, int32_t B, int32_t n_steps, int32_t which_net,
                                 const iqlhip_var_scalars* scalars, const uint64_t* seeds, const uint64_t* stream_offsets,
                                 const int64_t* const* starts_dev, const int64_t* n_starts, void* stream);
/* Waits for `stream`; then the first n_steps words of every member's loss ring and start ring of the last
 * iqlhip_var_group_train_steps call: losses_out[K][n_steps], starts_out[K][n_steps]. */
int iqlhip_var_group_read_train_ring(iqlhip_var_group* group, float* losses_out, int64_t* starts_out, int32_t n_steps,
                                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IQLHIP_H */
