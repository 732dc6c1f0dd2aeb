// JSRL selection by the critic (include/iqlhip.h iqlhip_jsrl_act_q; DESIGN.md 6k "who == 3"): a row whose byte is 3
// takes whichever of the two proposed actions the member's twin critic values more.  Included behind
// iqlhip_jsrl_kernels.h (helpers in scope: JsrlFinRec, jsrl_finish_elem, actor_finish_elem, philox4x32_10, sum4, f32x4,
// NSPLIT, HEAD_LD).  Two launches around a Q forward (iql_act_fwd_group_kernel, only_inst = 4 and 5 over 2 n rows):
//   candidates: the finish launch that also writes the critic's packed act rows — row r = [s_r | a_g], row n + r =
//               [s_r | a_l]; the states of both halves were packed by the call's pack launch, which zeroes the rest;
//   select:     the four head sums of a row, the rule, the chosen candidate copied out of the device rows.
#pragma once

// Per requesting member, next to its JsrlFinRec.  xq == NULL: the member has no `3` in this call.
struct JsrlQRec {
  float* xq;                          // candidate rows [2 n][ld_q] of the handle (the step's packed layout: [s | a | 0 ...])
  const float* heads_q;               // the critic's scalar partials [2 n][HEAD_LD] (instances 4 and 5)
  float* q_out;                       // nullable [n][4]: Q1g, Q2g, Q1l, Q2l (NaN on rows whose byte is not 3)
  float inv_temp;                     // +inf: argmax; else the Boltzmann draw's inverse temperature (>= 0)
  int ld_q, S;
};

// Candidates: element e = row * A + d, numbered as jsrl_finish_elem numbers it.  A row with a byte in 0..2 is finished
// exactly as iql_jsrl_finish_kernel finishes it; a `3` row writes both candidates — each by the same actor_finish_elem
// call a who == 0 / who == 1 row makes, only the destination differs — into the critic's rows and nothing into `out`.
__global__ __launch_bounds__(256) void iql_jsrl_q_cand_kernel(const JsrlFinRec* __restrict__ recs,
                                                              const JsrlQRec* __restrict__ qrecs) {
  const JsrlFinRec& r = recs[blockIdx.y];
  const JsrlQRec& q = qrecs[blockIdx.y];
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= r.n * r.A) return;
  if (q.xq == nullptr || r.who[e / r.A] != 3) {
    jsrl_finish_elem(r, e);
    return;
  }
  actor_finish_elem(r.heads_g, e, r.A, r.max_g, nullptr, 0.f, 0.f, nullptr, 0, 0ull, 0ull, q.xq + q.S, (long long)q.ld_q);
  actor_finish_elem(r.heads_l, e, r.A, r.max_l, r.log_std, r.ls_min, r.ls_max, nullptr, 0, r.seed, r.call,
                    q.xq + (long long)r.n * q.ld_q + q.S, (long long)q.ld_q);
}

// Select: qg = min(Q1, Q2)(s, a_g), ql = min(Q1, Q2)(s, a_l), each head the sum4 of its four slice partials.
//   inv_temp infinite or seed == 0:  use_learner = (ql >= qg)
//   else:  p = 1 / (1 + expf(-(ql - qg) * inv_temp)),  use_learner = (u < p),  u = the 24-bit unit float of word 2 of
//          the Philox block actor_finish_elem draws for element row * A (same key, counter and tag; words 0 and 1 are
//          its Box-Muller pair).
// Every element of a row forms the row's decision itself and copies its own component of the chosen candidate.
__global__ __launch_bounds__(256) void iql_jsrl_q_select_kernel(const JsrlFinRec* __restrict__ recs,
                                                                const JsrlQRec* __restrict__ qrecs) {
  const JsrlFinRec& r = recs[blockIdx.y];
  const JsrlQRec& q = qrecs[blockIdx.y];
  if (q.xq == nullptr) return;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= r.n * r.A) return;
  const int row = e / r.A, dd = e - row * r.A;
  if (r.who[row] != 3) {
    if (dd == 0 && q.q_out) {
      const float nan = __builtin_nanf("");
      float* qo = q.q_out + (long long)row * 4;
      qo[0] = nan; qo[1] = nan; qo[2] = nan; qo[3] = nan;
    }
    return;
  }
  const float* hg = q.heads_q + (long long)row * HEAD_LD;
  const float* hl = q.heads_q + (long long)(r.n + row) * HEAD_LD;
  const float q1g = sum4(*(const f32x4*)(hg + 4 * NSPLIT)), q2g = sum4(*(const f32x4*)(hg + 5 * NSPLIT));
  const float q1l = sum4(*(const f32x4*)(hl + 4 * NSPLIT)), q2l = sum4(*(const f32x4*)(hl + 5 * NSPLIT));
  const float qg = fminf(q1g, q2g), ql = fminf(q1l, q2l);
  bool learner;
  if (r.seed == 0ull || isinf(q.inv_temp)) {
    learner = ql >= qg;
  } else {
    const float p = 1.f / (1.f + expf(-(ql - qg) * q.inv_temp));
    uint32_t c[4] = {(uint32_t)(row * r.A), (uint32_t)r.call, (uint32_t)(r.call >> 32), 0xAC7u};
    philox4x32_10(c, (uint32_t)r.seed, (uint32_t)(r.seed >> 32));
    const float u = ((float)(c[2] >> 8) + 0.5f) * (1.f / 16777216.f);
    learner = u < p;
  }
  r.out[row * r.ld_out + dd] = q.xq[(long long)(learner ? r.n + row : row) * q.ld_q + q.S + dd];
  if (dd == 0) {
    if (r.use_learner) r.use_learner[row] = learner ? 1 : 0;
    if (r.gate_out && r.heads_v) r.gate_out[row] = sum4(*(const f32x4*)(r.heads_v + (long long)row * HEAD_LD + 1 * NSPLIT));
    if (q.q_out) {
      float* qo = q.q_out + (long long)row * 4;
      qo[0] = q1g; qo[1] = q2g; qo[2] = q1l; qo[3] = q2l;
    }
  }
}
