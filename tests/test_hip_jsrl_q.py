"""GPU tests of the JSRL critic selection (who == 3: iqlhip_jsrl_act_q, JsrlActors(..., critics=...)): the candidates
bit for bit against who == 0 / who == 1 calls, the decision exactly self-consistent with the returned Q values (argmax
and Boltzmann, the latter against tests/jsrl_q_ref.py), the Q values against the critic's PyTorch TwinQ in float64,
nothing else moved, the launch shape without a 3, refusals, and lockstep evaluation.

Bounds.  Q_TOL["f32"] is 4 x the largest fp32 error this file measured (rel_err: max abs error over max abs value; the
MARGIN lines it prints, kept in profiles/jsrl_q_parity_margins.txt) — summation order is the only difference — and must
not exceed the 2e-5 tests/test_hip_score.py holds q1 and q2 to; bf16 is the project's 5e-3."""
import ctypes as C
import functools
import math
import types

import numpy as np
import pytest
import torch

import jsrl_q_ref as R
import synth
import value_edges as ve
from helpers import rel_err

pytestmark = pytest.mark.gpu

# S, A, Gaussian learner, Gaussian guide: 39/28 takes the wide layer-0 staging (S + A = 67 input columns)
SHAPES = [(17, 6, True, True), (29, 8, True, False), (39, 28, True, True)]
ROWS = [1, 17, 33, 256]      # 17: 2 n = 34 crosses a 32-row tile inside the learner half; 33: that half starts mid-tile
SCORE_Q_TOL = 2e-5           # what tests/test_hip_score.py holds q1 / q2 to
F32_MEASURED = 8.8e-7        # the largest fp32 rel_err of profiles/jsrl_q_parity_margins.txt
Q_TOL = {"f32": 4 * F32_MEASURED, "bf16": 5e-3}
Q_W2_SCALE = ve.QT_W2_SCALE  # the critics' output layer, scaled as trained_like scales the target critics'
# ... and its action columns of layer 0: a critic that tells actions apart.  Chosen on the float64 reference alone: with
# 12 and 4 the two candidates' min-Q lie further apart than 1 % of the largest |Q| (twice the bf16 bound) on 95 % of rows
Q_ACTION_SCALE = 4.0
CALL0 = 41                  # the act() call number every compared call is made at


def _hip():
    import iql
    import iqlhip_binding as hb
    from hip_helpers import build_hip_trainer
    return iql, hb, build_hip_trainer


def tl_params(S, A, gaussian, seed):
    """synth_params made trained-like (value_edges.trained_like: saturated policy head, log_std over both clamps), and
    the online critics' output layer scaled like the targets', so that Q differs visibly between two actions."""
    params = synth.synth_params(S, A, seed=seed, gaussian=gaussian)
    ve.trained_like(params, synth.synth_transitions(64, S, A, seed=seed + 1), {"B": 64, "A": A, "gaussian": gaussian})
    for n in ("q1", "q2"):
        params[n]["w2"] = params[n]["w2"] * np.float32(Q_W2_SCALE)
        params[n]["w0"] = params[n]["w0"].copy()
        params[n]["w0"][:, S:] *= np.float32(Q_ACTION_SCALE)
    return params


def _trainer(S, A, gaussian, seed, max_action=1.0, precision="f32", dropout=0.0):
    t = _hip()[2](tl_params(S, A, gaussian, seed), S, A, gaussian, ve.HYPER, ve.LRS, 1000, max_action=max_action, dropout=dropout)
    if precision != "f32":
        t.set_precision(precision)
    # the act() noise key is derived from torch's seed at first use: pinned here (the key torch.manual_seed(7700 + seed)
    # would give), so that the rows and the recorded margins do not depend on what ran before
    t._act_key = ((7700 + seed) * 0x9E3779B97F4A7C15 + 0xAC7) & 0xFFFFFFFFFFFFFFFF
    return t


def _counters(t):
    hb = _hip()[1]
    c = (C.c_uint64 * 2)()
    hb.check(hb.lib().iqlhip_get_counters(t._ctx, c))
    return int(c[0]), int(c[1])


def _set_act_calls(t, n):
    hb = _hip()[1]
    hb.check(hb.lib().iqlhip_set_counters(t._ctx, (C.c_uint64 * 2)(_counters(t)[0], n)))


def _states(n, S, seed):
    return np.random.default_rng(seed).standard_normal((n, S)).astype(np.float32)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def q64(params, s, a):
    """(Q1, Q2) of the PyTorch TwinQ holding `params`, evaluated in float64."""
    from hip_helpers import _load_mlp
    qf = _hip()[0].TwinQ(s.shape[1], a.shape[1])
    _load_mlp(qf.q1, params["q1"])
    _load_mlp(qf.q2, params["q2"])
    with torch.no_grad():
        q1, q2 = qf.double().both(torch.from_numpy(s).double(), torch.from_numpy(a).double())
    return q1.numpy(), q2.numpy()


def _fwd(j, x, who, sample, **kw):
    """One actor_forward of a K = 1 handle at call number CALL0: numpy (actions, flags, h, q)."""
    _set_act_calls(j.learners[0], CALL0)
    got = j.actor_forward([torch.from_numpy(x).cuda()], [who], sample=sample, **kw)[0]
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in got)


def check_q(q, params, x, a_g, a_l, flags, precision, tag):
    """Returned q against the float64 TwinQ on (s, candidate): every value within Q_TOL, and the decision equal to the
    float64 decision wherever the float64 values are further apart than twice the bound."""
    g1, g2 = q64(params, x, a_g)
    l1, l2 = q64(params, x, a_l)
    want = np.stack([g1, g2, l1, l2], axis=1)
    tol = Q_TOL[precision]
    e_abs, e_rel = np.max(np.abs(q.astype(np.float64) - want)), rel_err(q, want)
    print(f"MARGIN jsrl_q {tag} {precision} max_abs {e_abs:.3e} rel_err {e_rel:.3e} bound {tol:.1e}")
    assert e_rel <= tol, (tag, e_rel)
    gap = np.minimum(l1, l2) - np.minimum(g1, g2)
    comparable = np.abs(gap) > 2 * tol * np.abs(want).max()
    assert comparable.mean() >= 0.9, (tag, comparable.mean())
    assert np.array_equal(flags[comparable] != 0, gap[comparable] >= 0), tag
    return want


@functools.lru_cache(maxsize=None)
def _solo(S, A, gl, gg):
    """(JsrlActors with the learner as its own critic, learner parameters): learner and guide differ in max_action."""
    iql = _hip()[0]
    learner, guide = _trainer(S, A, gl, 800 + S, 1.5), _trainer(S, A, gg, 801 + S, 1.25)
    return iql.JsrlActors(learner, guide, critics=True), tl_params(S, A, gl, 800 + S)


@pytest.mark.parametrize("S,A,gl,gg", SHAPES)
@pytest.mark.parametrize("n", ROWS)
def test_candidates_decision_and_q(S, A, gl, gg, n):
    j, params = _solo(S, A, gl, gg)
    learner, guide = j.learners[0], j.guides[0]
    x = _states(256, S, 50 + S)[:n]
    three = np.full(n, 3, np.int8)
    a_g, f0, _, q0 = _fwd(j, x, np.zeros(n, np.int8), True)
    a_l, f1, _, q1 = _fwd(j, x, np.ones(n, np.int8), True)
    assert not f0.any() and f1.all() and np.isnan(q0).all() and np.isnan(q1).all()
    assert not _same(a_l, _fwd(j, x, np.ones(n, np.int8), False)[0])      # the learner's rows carry the call's noise
    # ---- argmax: candidates, self-consistency, counters
    before = _counters(guide)
    a, f, h, q = _fwd(j, x, three, True)
    assert h is None and q.shape == (n, 4) and q.dtype == np.float32 and np.isfinite(q).all()
    assert _same(a, R.assemble(a_g, a_l, f))
    assert np.array_equal(f != 0, np.minimum(q[:, 2], q[:, 3]) >= np.minimum(q[:, 0], q[:, 1]))
    assert np.array_equal(f != 0, R.decide(q, math.inf))
    assert _counters(learner)[1] == CALL0 + 1 and _counters(guide) == before
    check_q(q, params, x, a_g, a_l, f, "f32", f"S{S}A{A}_n{n}")
    # ---- Boltzmann at the scale of the rows' own gaps: the flag is the CPU rule on the returned q
    qg, ql = R.q_min(q)
    inv_t = float(1.0 / max(np.median(np.abs(ql - qg)), 1e-3))
    ab, fb, _, qb = _fwd(j, x, three, True, q_inv_temp=inv_t)
    assert _same(qb, q) and _same(ab, R.assemble(a_g, a_l, fb))
    seed = learner._act_seed()
    close = R.margin(qb, inv_t, seed, CALL0, A) < 1e-6
    assert close.sum() <= (1 if n == 256 else 0)
    assert np.array_equal((fb != 0)[~close], R.decide(qb, inv_t, seed, CALL0, A)[~close])
    if n == 256:
        assert 0 < fb.sum() < n and not np.array_equal(fb, f)             # both act, and the draw really decides
    # ---- eval mode (seed 0): the argmax whatever the temperature, on the mean action
    am, fm, _, qm = _fwd(j, x, three, False, q_inv_temp=inv_t)
    mean = _fwd(j, x, np.ones(n, np.int8), False)[0]
    assert _same(am, R.assemble(a_g, mean, fm)) and np.array_equal(fm != 0, R.decide(qm, math.inf))
    assert _counters(learner)[1] == CALL0


def test_mixed_call_with_a_gate_equals_act_on_rows_0_to_2():
    iql = _hip()[0]
    S, A, n = 17, 6, 33
    learner, guide, gate = _trainer(S, A, True, 810, 1.5), _trainer(S, A, True, 811, 1.25), _trainer(S, A, True, 812)
    jq, jo = iql.JsrlActors(learner, guide, gate, critics=True), iql.JsrlActors(learner, guide, gate)
    x = _states(n, S, 61)
    who = (np.arange(n) % 4).astype(np.int8)
    gm = float(np.median(_fwd(jo, x, np.zeros(n, np.int8), False, gate_max=[0.0])[2]))
    a, f, h, q = _fwd(jq, x, who, True, gate_max=[gm])
    old = who != 3
    ao, fo, ho = _fwd(jo, x, np.where(old, who, 0).astype(np.int8), True, gate_max=[gm])
    assert _same(a[old], ao[old]) and np.array_equal(f[old], fo[old]) and _same(h, ho)
    assert 0 < f[who == 2].sum() < (who == 2).sum()
    assert np.isnan(q[old]).all() and np.isfinite(q[~old]).all()
    a3, f3, _, q3 = _fwd(jq, x, np.full(n, 3, np.int8), True, gate_max=[gm])
    assert _same(a[~old], a3[~old]) and np.array_equal(f[~old], f3[~old]) and _same(q[~old], q3[~old])


def test_three_members_without_a_3_equal_act_bit_for_bit():
    """Rows [33, 3, 0]: a member with a critic but no 3, one without a critic, one skipped — through act_q."""
    iql = _hip()[0]
    S, A = 17, 6
    ls = [_trainer(S, A, True, 820 + k, 1.0 + 0.5 * k) for k in range(3)]
    guide, gate = _trainer(S, A, True, 824, 1.25), _trainer(S, A, True, 825)
    for t in ls:
        t.actor.eval()
    xs = [_states(33, S, 62), _states(3, S, 63), None]
    whos = [(np.arange(33) % 3).astype(np.int8), np.array([0, 1, 1], np.int8), 0]
    jq = iql.JsrlActors(ls, guide, [gate, None, gate], critics=[True, None, True])
    jo = iql.JsrlActors(ls, guide, [gate, None, gate])
    got, want = jq.act(xs, whos, gate_max=[0.0, 0.0, 0.0]), jo.act(xs, whos, gate_max=[0.0, 0.0, 0.0])
    assert got[2] is None and want[2] is None and len(got[0]) == 4 and len(got[1]) == 3
    for k in range(2):
        assert _same(got[k][0], want[k][0]) and np.array_equal(got[k][1], want[k][1])
    assert _same(got[0][2], want[0][2]) and got[1][2] is None and np.isnan(got[0][3]).all()
    # the host-memory form with a 3: the chosen rows come from the device-side candidates
    whos[0] = np.where(np.arange(33) % 2 == 0, 3, whos[0]).astype(np.int8)
    a, f, h, q = jq.act(xs, whos, gate_max=[0.0, 0.0, 0.0])[0]
    dev = jq.actor_forward([torch.from_numpy(xs[0]).cuda(), torch.from_numpy(xs[1]).cuda(), torch.zeros((0, S)).cuda()],
                           [whos[0], whos[1], np.zeros(0, np.int8)], gate_max=[0.0, 0.0, 0.0])[0]
    assert _same(a, dev[0].cpu().numpy()) and np.array_equal(f, dev[1].cpu().numpy()) and _same(h, dev[2].cpu().numpy())
    three = whos[0] == 3
    assert _same(q[three], dev[3].cpu().numpy()[three]) and np.isnan(q[~three]).all()
    assert np.array_equal(f[three] != 0, R.decide(q[three], math.inf))


def test_bf16_learner_next_to_an_fp32_one():
    iql = _hip()[0]
    S, A, n = 17, 6, 33
    pb = tl_params(S, A, True, 830)
    lb, lf = _trainer(S, A, True, 830, 1.5, precision="bf16"), _trainer(S, A, True, 830, 1.5)
    guide = _trainer(S, A, True, 831, 1.25)
    x = _states(n, S, 64)
    j = iql.JsrlActors([lb, lf], guide, critics=True)
    out = {}
    for who in (0, 1, 3):
        for t in (lb, lf):
            _set_act_calls(t, CALL0)
        got = j.actor_forward([torch.from_numpy(x).cuda()] * 2, [np.full(n, who, np.int8)] * 2, sample=True)
        out[who] = [tuple(None if t is None else t.cpu().numpy() for t in g) for g in got]
    for k, precision in enumerate(("bf16", "f32")):
        a, f, _, q = out[3][k]
        a_g, a_l = out[0][k][0], out[1][k][0]
        assert _same(a, R.assemble(a_g, a_l, f)) and np.array_equal(f != 0, R.decide(q, math.inf))
        check_q(q, pb, x, a_g, a_l, f, precision, f"pair_member{k}")
    assert not _same(out[3][0][3], out[3][1][3])          # each critic really ran at its own precision


def test_a_third_trainer_as_the_critic_and_nothing_else_moves():
    from hip_helpers import arenas, to_torch_batch
    iql = _hip()[0]
    S, A, n = 29, 8, 33
    pc = tl_params(S, A, True, 842)
    learner, twin = _trainer(S, A, True, 840, 1.5), _trainer(S, A, True, 840, 1.5)
    guide, critic = _trainer(S, A, False, 841, 1.25), _trainer(S, A, True, 842)
    j, own = iql.JsrlActors(learner, guide, critics=[critic]), iql.JsrlActors(learner, guide, critics=True)
    x = _states(n, S, 65)
    a_g = _fwd(j, x, np.zeros(n, np.int8), True)[0]
    a_l = _fwd(j, x, np.ones(n, np.int8), True)[0]
    before = [arenas(t) for t in (learner, guide, critic)]
    counters = [_counters(t) for t in (guide, critic)]
    a, f, _, q = _fwd(j, x, np.full(n, 3, np.int8), True, q_inv_temp=0.5)
    for t, b in zip((learner, guide, critic), before):
        assert np.array_equal(arenas(t).view(np.uint32), b.view(np.uint32))
    assert _counters(learner)[1] == CALL0 + 1 and [_counters(t) for t in (guide, critic)] == counters
    assert _same(a, R.assemble(a_g, a_l, f))
    check_q(q, pc, x, a_g, a_l, R.decide(q, math.inf), "f32", "third_trainer")
    assert not _same(q, _fwd(own, x, np.full(n, 3, np.int8), True)[3])      # (the learner's own critic values differ)
    # a plain train() afterwards: the losses of a twin that never made the call
    data = synth.synth_transitions(64, S, A, seed=66)
    batch = {"s": data["observations"], "a": data["actions"], "r": data["rewards"], "ns": data["next_observations"],
             "d": data["terminals"]}
    la, lb = learner.train(to_torch_batch(batch)), twin.train(to_torch_batch(batch))
    assert all(la[k] == lb[k] for k in ("value_loss", "q_loss", "actor_loss"))


def _raw_q(j, x, who, q_inv_temp=(math.inf,), want_q=True, seed=0, entry="iqlhip_jsrl_act_q"):
    """One K = 1 call of a C entry point on device tensors: its return code."""
    hb = _hip()[1]
    l = j.learners[0]
    S, A, n = l._S, l._A, x.shape[0]
    xd = torch.from_numpy(x).cuda()
    out = torch.zeros((n, A), dtype=torch.float32, device="cuda")
    use = torch.zeros(n, dtype=torch.int32, device="cuda")
    q = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    who = np.ascontiguousarray(who, dtype=np.int8)
    one = lambda v: (C.c_void_p * 1)(v)
    args = [j._handle(), one(xd.data_ptr()), S, (C.c_int32 * 1)(n), one(who.ctypes.data), (C.c_float * 1)(0.0),
            (C.c_uint64 * 1)(seed), (C.c_float * 1)(float(l.actor.max_action)),
            (C.c_float * 1)(float(j.guides[0].actor.max_action)), one(out.data_ptr()), A, one(use.data_ptr()), one(None)]
    if entry == "iqlhip_jsrl_act_q":
        args += [None if q_inv_temp is None else (C.c_float * 1)(*q_inv_temp), one(q.data_ptr() if want_q else None)]
    rc = getattr(hb.lib(), entry)(*args, 0, l._stream())
    torch.cuda.synchronize()
    return rc


def test_refusals_launch_and_count_nothing():
    iql, hb, _ = _hip()
    S, A = 17, 6
    learner, guide = _trainer(S, A, True, 850), _trainer(S, A, True, 851)
    j = iql.JsrlActors(learner, guide, critics=True)
    x, three = _states(3, S, 67), np.full(3, 3, np.int8)
    _set_act_calls(learner, CALL0)
    seed = learner._act_seed()
    bad = [(_raw_q(j, x, three, (-1.0,), seed=seed), hb.E_INVAL), (_raw_q(j, x, three, (math.nan,), seed=seed), hb.E_INVAL),
           (_raw_q(j, x, three, None, seed=seed), hb.E_INVAL),
           (_raw_q(j, x, np.array([0, 1, 1], np.int8), seed=seed), hb.E_INVAL),           # q_out without a 3
           (_raw_q(j, x, np.array([0, 4, 3], np.int8), seed=seed), hb.E_INVAL),
           (_raw_q(j, _states(2049, S, 68), np.full(2049, 3, np.int8), seed=seed), hb.E_INVAL),      # 2 n > 4096
           (_raw_q(j, x, three, seed=seed, entry="iqlhip_jsrl_act"), hb.E_INVAL)]          # the old entry point
    for i, (rc, code) in enumerate(bad):
        assert rc == code and hb.last_error(), i
    assert _raw_q(j, _states(2049, S, 68), np.ones(2049, np.int8), want_q=False) == 0       # (without a 3 the rows fit)
    # an unbound context as the critic
    d = hb.Dims(S, A, hb.IQLHIP_HIDDEN, 2, hb.POLICY_GAUSSIAN, 256)
    raw_ctx = C.c_void_p()
    hb.check(hb.lib().iqlhip_create(C.byref(d), C.byref(learner._hyper_struct()), learner._dev.index, C.byref(raw_ctx)))
    assert hb.lib().iqlhip_jsrl_set_critics(j._handle(), (C.c_void_p * 1)(raw_ctx)) == hb.E_NOTBOUND
    hb.check(hb.lib().iqlhip_destroy(raw_ctx))
    other = _trainer(S + 1, A, True, 852)
    assert hb.lib().iqlhip_jsrl_set_critics(j._handle(), (C.c_void_p * 1)(other._ctx)) == hb.E_INVAL
    assert _counters(learner)[1] == CALL0
    assert _raw_q(j, x, three, seed=seed) == 0 and _counters(learner)[1] == CALL0 + 1
    # inference dropout: the library refuses, and the Python fall-back has no critic stage
    dl = _trainer(S, A, True, 853, dropout=0.1)
    dl.set_act_dropout(True)
    dl.actor.train()
    jd = iql.JsrlActors(dl, guide, critics=True)
    dl._prepare_act()
    assert _raw_q(jd, x, three) == hb.E_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="who == 3"):
        jd.act([x], [three])
    a, f, h, q = jd.act([x], [np.array([0, 1, 1], np.int8)])[0]
    assert a.shape == (3, A) and list(f) == [0, 1, 1] and h is None and np.isnan(q).all()


def test_lockstep_evaluation_equals_each_members_solo_run():
    from test_group_act_cpu import RecEnv
    iql = _hip()[0]
    S, A, n_ep = 17, 6, 2
    ls = [_trainer(S, A, True, 860 + k, 1.0) for k in range(2)]
    gs = [_trainer(S, A, True, 870 + k, 1.0) for k in range(2)]
    cfg = lambda: types.SimpleNamespace(curriculum_stage=3.0, curriculum_stage_idx=1, n_curriculum_stages=5, ep_agent_type=0,
                                        agent_type_stage=1.0, max_init_horizon=False, discrete=False)
    envs = lambda: [RecEnv(S, A, base=3 + 2 * k) for k in range(2)]
    got = iql.eval_actors_jsrl(envs(), iql.JsrlActors(ls, gs, critics=True), [cfg(), cfg()], "time_step", n_ep, [5, 6],
                               who=[3, 3], q_inv_temp=2.0)
    for k in range(2):
        solo = iql.eval_actors_jsrl(envs()[k:k + 1], iql.JsrlActors(ls[k], gs[k], critics=True), [cfg()], "time_step", n_ep,
                                    [5 + k], who=[3])[0]
        assert np.array_equal(got[k][0], solo[0]) and got[k][1:] == solo[1:], k
    assert any(0.0 < g[3] < 1.0 for g in got)       # guide and learner really mix within the episodes
