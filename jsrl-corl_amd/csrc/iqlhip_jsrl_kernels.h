// JSRL action selection (include/iqlhip.h iqlhip_jsrl_act): guide or learner per row.  Included at the
// end of iqlhip.hip, behind every other kernel of the file (helpers in scope: actor_finish_elem, sum4, f32x4, NSPLIT,
// HEAD_LD).  The states are packed by iql_pack_states_group_kernel and the forwards run as iql_act_fwd_group_kernel
// over a record table — one record per (member, role) the call needs: the learner's and the guide's policy instance
// (only_inst = 6), the gate's value instance V(s) (only_inst = 1) — so only the finish is new.
#pragma once

// Per requesting member: what the finish reads and writes.
struct JsrlFinRec {
  const float* heads_l;               // the learner's policy partials [n][A][NSPLIT]; NULL: no row can choose it
  const float* heads_g;               // the guide's; NULL: no row can choose it
  const float* heads_v;               // the gate's scalar partials [n][HEAD_LD] (instance 1); NULL: no gate forward
  const float* log_std;               // the learner's; NULL: deterministic policy
  const signed char* who;             // [n]: 0 guide, 1 learner, 2 the gate decides (the device copy of the call's bytes)
  float* out;                         // actions (device or host-mapped memory), row stride ld_out
  int* use_learner;                   // nullable [n]
  float* gate_out;                    // nullable [n]
  long long ld_out;
  int n, A;
  float gate_max, max_l, max_g, ls_min, ls_max;
  unsigned long long seed, call;      // seed 0: the learner's mean action
};

// Element e = row * A + d of member r, numbered as iql_actor_finish_kernel numbers it: a learner row is
// actor_finish_elem with the learner's arguments (so the device noise of (seed, call) is the solo call's draw element
// for element), a guide row the same with no noise.  h = the gate's V(s) in the step's fixed order of partial sums.
__device__ __forceinline__ void jsrl_finish_elem(const JsrlFinRec& r, int e) {
  const int row = e / r.A;
  const int w = r.who[row];
  float h = 0.f;
  if (r.heads_v) h = sum4(*(const f32x4*)(r.heads_v + (long long)row * HEAD_LD + 1 * NSPLIT));
  const bool learner = (w == 1) || (w == 2 && h <= r.gate_max);
  if (learner)
    actor_finish_elem(r.heads_l, e, r.A, r.max_l, r.log_std, r.ls_min, r.ls_max, nullptr, 0, r.seed, r.call, r.out, r.ld_out);
  else
    actor_finish_elem(r.heads_g, e, r.A, r.max_g, nullptr, 0.f, 0.f, nullptr, 0, 0ull, 0ull, r.out, r.ld_out);
  if (e - row * r.A == 0) {
    if (r.use_learner) r.use_learner[row] = learner ? 1 : 0;
    if (r.gate_out && r.heads_v) r.gate_out[row] = h;
  }
}

// grid.y = requesting member, grid.x over the longest member's n * A elements.
__global__ __launch_bounds__(256) void iql_jsrl_finish_kernel(const JsrlFinRec* __restrict__ recs) {
  const JsrlFinRec& r = recs[blockIdx.y];
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < r.n * r.A) jsrl_finish_elem(r, e);
}

// One member, at most 256 elements, in one block, then the call's completion word (iqlhip_jsrl_online_step: action, flag
// and h travel through host-mapped words, as iql_actor_finish_kernel's done_flag form does it).
__global__ __launch_bounds__(256) void iql_jsrl_finish_done_kernel(const JsrlFinRec* __restrict__ recs,
                                                                   unsigned long long* done_flag,
                                                                   unsigned long long done_val) {
  const JsrlFinRec& r = recs[0];
  const int e = threadIdx.x;
  if (e < r.n * r.A) jsrl_finish_elem(r, e);
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(done_flag, done_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
