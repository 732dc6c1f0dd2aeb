"""GPU tests of the JSRL action selection (iqlhip_jsrl_act / iqlhip_jsrl_online_step, JsrlActors): per-row choice of
guide or learner bit for bit against the solo calls, the device gate against the fp32 oracle's value forward, the
recorded reference decisions (g19), member count and place, a bf16 learner, the fused online iteration, rejections."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import synth
from helpers import load_golden, rel_err

pytestmark = pytest.mark.gpu

DIMS = [(17, 6, True), (29, 8, False)]
ROWS = [1, 3, 33]                     # 33: one more than the forward's 32-row tile
V_TOL = 2e-5                          # the bound tests/test_hip_score.py holds `v` to (profiles/score_parity_margins.txt)
_HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
_LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}


def _hip():
    import iql
    import iqlhip_binding as hb
    from hip_helpers import build_hip_trainer
    return iql, hb, build_hip_trainer


def _trainer(S, A, gaussian, seed, max_action=1.0, precision="f32", params=None, dropout=0.0):
    params = params or synth.synth_params(S, A, seed=seed, gaussian=gaussian)
    t = _hip()[2](params, S, A, gaussian, _HYPER, _LRS, 1000, max_action=max_action, dropout=dropout)
    if precision != "f32":
        t.set_precision(precision)
    return t


def _act_calls(t):
    hb = _hip()[1]
    c = (C.c_uint64 * 2)()
    hb.check(hb.lib().iqlhip_get_counters(t._ctx, c))
    return int(c[1])


def _states(n, S, seed):
    return np.random.default_rng(seed).standard_normal((n, S)).astype(np.float32)


def _oracle_v(params, x):
    from oracle import iql_oracle as O
    return O.mlp_forward(params["vf"], x.astype(np.float32))[0].reshape(-1).astype(np.float32)


def _gate_max_of(v):
    """The midpoint of the widest gap between consecutive sorted oracle values; the gap is at least 100 tolerances."""
    s = np.sort(v.astype(np.float64))
    g = int(np.argmax(np.diff(s)))
    assert s[g + 1] - s[g] >= 100 * V_TOL * np.abs(s).max(), (s[g + 1] - s[g], np.abs(s).max())
    return float(np.float32(0.5 * (s[g] + s[g + 1])))


def _expected(twin, guide, x, use, sample):
    """Rows of the solo calls over the same states array: the twin learner's where `use`, else the guide's mean."""
    xd = torch.from_numpy(x).cuda()
    a_l = twin.actor_forward(xd, sample=sample).cpu().numpy()
    a_g = guide.actor_forward(xd).cpu().numpy()
    return np.where(np.asarray(use, bool)[:, None], a_l, a_g)


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("S,A,gaussian", DIMS)
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("sample", [False, True])
def test_selection_bit_for_bit(S, A, gaussian, n, sample):
    iql = _hip()[0]
    learner, twin = _trainer(S, A, gaussian, 700, 1.5), _trainer(S, A, gaussian, 700, 1.5)
    guide = _trainer(S, A, gaussian, 701, 1.25)
    j = iql.JsrlActors(learner, guide)
    x = _states(n, S, 3)
    draws = sample and gaussian
    for who in (np.zeros(n, np.int8), np.ones(n, np.int8), (np.arange(n) % 2).astype(np.int8)):
        c_l, c_t, c_g = _act_calls(learner), _act_calls(twin), _act_calls(guide)
        (a, use, h), = j.actor_forward([torch.from_numpy(x).cuda()], [who], sample=sample)
        want = _expected(twin, guide, x, who, sample)
        assert _same(a.cpu().numpy(), want), who
        assert np.array_equal(use.cpu().numpy(), who.astype(np.int32)) and h is None
        # one call, one number — whatever the rows chose; the twin's solo call moved its counter the same way
        assert _act_calls(learner) - c_l == (1 if draws else 0) == _act_calls(twin) - c_t
        assert _act_calls(guide) == c_g
    if draws:
        ones = np.ones(n, np.int8)
        (a1, _, _), = j.actor_forward([torch.from_numpy(x).cuda()], [ones], sample=True)
        (a2, _, _), = j.actor_forward([torch.from_numpy(x).cuda()], [ones], sample=True)
        assert not _same(a1.cpu().numpy(), a2.cpu().numpy())


@pytest.mark.parametrize("S,A,gaussian", DIMS)
def test_gate_against_the_oracle(S, A, gaussian):
    iql = _hip()[0]
    gparams = synth.synth_params(S, A, seed=712, gaussian=gaussian)
    learner, twin = _trainer(S, A, gaussian, 710), _trainer(S, A, gaussian, 710)
    guide, gate = _trainer(S, A, gaussian, 711, 2.0), _trainer(S, A, gaussian, 712, params=gparams)
    j = iql.JsrlActors(learner, guide, gate)
    x_all = _states(max(ROWS), S, 5)
    v_all = _oracle_v(gparams, x_all)
    for n in ROWS:
        x, v = x_all[:n], v_all[:n]
        gm = _gate_max_of(v_all) if n == 1 else _gate_max_of(v)      # (one value has no gap of its own)
        want_use = (v <= np.float32(gm)).astype(np.int32)
        (a, use, h), = j.actor_forward([torch.from_numpy(x).cuda()], [np.full(n, 2, np.int8)], gate_max=[gm])
        h = h.cpu().numpy()
        print("gate", (S, A), n, "rel_err", rel_err(h, v), "learner rows", int(want_use.sum()))
        assert np.max(np.abs(h.astype(np.float64) - v)) <= V_TOL * np.abs(v_all).max()
        assert np.array_equal(use.cpu().numpy(), want_use)
        assert _same(a.cpu().numpy(), _expected(twin, guide, x, want_use, False))
        # mixed 0 / 1 / 2 in one call
        who = (np.arange(n) % 3).astype(np.int8)
        mixed = np.where(who == 2, want_use, who).astype(np.int32)
        (a, use, h2), = j.actor_forward([torch.from_numpy(x).cuda()], [who], gate_max=[gm])
        assert np.array_equal(use.cpu().numpy(), mixed) and _same(h2.cpu().numpy(), h)
        assert _same(a.cpu().numpy(), _expected(twin, guide, x, mixed, False))
    if max(ROWS) > 1:
        assert 0 < int((v_all <= _gate_max_of(v_all)).sum()) < len(v_all)


def test_g19_end_to_end():
    """JsrlActors.act with who_from_config against the reference's recorded actions (the g10 bound: 2e-6 * max_action),
    flags exact, the variance horizon within the v bound."""
    iql = _hip()[0]
    z, meta = load_golden("g19_jsrl_selection")
    fns = meta["horizon_fns"]
    for st in meta["sets"]:
        tag, S, A, gaussian = st["tag"], st["S"], st["A"], st["gaussian"]
        learner = _trainer(S, A, gaussian, st["seed_learner"], st["max_action_learner"])
        guide = _trainer(S, A, gaussian, st["seed_guide"], st["max_action_guide"])
        gate = _trainer(S, A, gaussian, st["seed_gate"])
        learner.actor.eval()
        with_guide, alone = iql.JsrlActors(learner, guide, gate), iql.JsrlActors(learner, None, gate)
        rows, states = z[tag + ".rows"], z[tag + ".states"]
        var_h = z[tag + ".horizon"][rows[:, 0] == 2]
        for i, row in enumerate(rows):
            fn = fns[int(row[0])]
            cfg = types.SimpleNamespace(curriculum_stage=row[2], curriculum_stage_idx=int(row[3]),
                                        n_curriculum_stages=int(row[4]), ep_agent_type=row[5], agent_type_stage=row[6])
            env = types.SimpleNamespace(dist=row[8])
            who, hz = iql.who_from_config(cfg, fn, [int(row[1])], [states[i]], [env], goal_dist=lambda s, e: e.dist)
            if int(who[0][0]) == 2:      # the gap condition, on the recorded horizons
                assert abs(z[tag + ".horizon"][i] - row[2]) >= 50 * V_TOL * np.abs(var_h).max()
            j = alone if row[7] else with_guide
            (a, use, h), = j.act([states[i]], who, gate_max=None if np.isnan(row[2]) else [row[2]])
            ma = st["max_action_learner"] if use[0] else st["max_action_guide"]
            assert int(use[0]) == int(z[tag + ".use_learner"][i]), (tag, i, fn)
            assert np.max(np.abs(a[0] - z[tag + ".actions"][i])) <= 2e-6 * ma, (tag, i, fn)
            if fn == "variance":
                assert abs(float(h[0]) - z[tag + ".horizon"][i]) <= V_TOL * np.abs(var_h).max(), (tag, i)
            else:
                assert float(hz[0]) == z[tag + ".horizon"][i]


@pytest.mark.parametrize("S,A,gaussian", DIMS)
def test_three_members_share_a_guide_and_one_has_no_gate(S, A, gaussian):
    iql = _hip()[0]
    learners = [_trainer(S, A, gaussian, 720 + k, 1.0 + 0.5 * k) for k in range(3)]
    guide, gates = _trainer(S, A, gaussian, 730, 1.75), [_trainer(S, A, gaussian, 731), None, _trainer(S, A, gaussian, 732)]
    xs = [_states(n, S, 40 + n) for n in (33, 3, 1)]
    whos = [(np.arange(33) % 3).astype(np.int8), np.array([0, 1, 1], np.int8), np.array([2], np.int8)]
    gms = [0.0, 0.0, 0.1]
    solo = []
    for k in range(3):
        (a, u, h), = iql.JsrlActors(learners[k], guide, gates[k]).actor_forward([torch.from_numpy(xs[k]).cuda()], [whos[k]], gate_max=[gms[k]])
        solo.append((a.cpu().numpy(), u.cpu().numpy(), None if h is None else h.cpu().numpy()))
    for order in ((0, 1, 2), (2, 0, 1)):
        j = iql.JsrlActors([learners[k] for k in order], guide, [gates[k] for k in order])
        got = j.actor_forward([torch.from_numpy(xs[k]).cuda() for k in order], [whos[k] for k in order],
                              gate_max=[gms[k] for k in order])
        for (a, u, h), k in zip(got, order):
            assert _same(a.cpu().numpy(), solo[k][0]) and np.array_equal(u.cpu().numpy(), solo[k][1]), (order, k)
            assert (h is None) == (solo[k][2] is None) and (h is None or _same(h.cpu().numpy(), solo[k][2]))
    assert 0 < solo[0][1].sum() < 33
    # the host-memory form, with a skipped member (eval mode: act() samples as actor.act does, the calls above did not)
    for t in learners:
        t.actor.eval()
    got =iql.JsrlActors(learners, guide, gates).act([xs[0], None, xs[2]], whos, gate_max=gms)
    assert got[1] is None and _same(got[0][0], solo[0][0]) and _same(got[2][0], solo[2][0]) and _same(got[2][2], solo[2][2])


@pytest.mark.parametrize("n", ROWS)
def test_bf16_learner_rows_are_its_solo_rows(n):
    iql = _hip()[0]
    S, A, gaussian = 17, 6, True
    learner, twin = (_trainer(S, A, gaussian, 740, precision="bf16") for _ in range(2))
    guide, gate = _trainer(S, A, gaussian, 741), _trainer(S, A, gaussian, 742)
    x = _states(n, S, 9)
    who = (np.arange(n) % 3).astype(np.int8)
    (a, use, h), = iql.JsrlActors(learner, guide, gate).actor_forward([torch.from_numpy(x).cuda()], [who], gate_max=[0.05], sample=True)
    use = use.cpu().numpy()
    assert _same(a.cpu().numpy(), _expected(twin, guide, x, use, True))
    f32 = _trainer(S, A, gaussian, 740).actor_forward(torch.from_numpy(x).cuda()).cpu().numpy()
    mean = twin.actor_forward(torch.from_numpy(x).cuda()).cpu().numpy()
    assert not _same(mean, f32)          # the learner really ran at its own precision


def test_online_step_jsrl_equals_online_step_then_act():
    from hip_helpers import assert_same_trainer_state
    iql = _hip()[0]
    S, A, gaussian, cap, B = 17, 6, True, 64, 16
    guide, gate = _trainer(S, A, gaussian, 751, 1.5), _trainer(S, A, gaussian, 752)
    data = synth.synth_transitions(cap + 8, S, A, seed=31)
    runs = []
    for fused in (True, False):
        t = _trainer(S, A, gaussian, 750)
        j = iql.JsrlActors(t, guide, gate)
        buf = iql.ReplayBuffer(S, A, cap, "cuda")
        buf.load_d4rl_dataset({k: v[:cap - 2].copy() for k, v in data.items()})
        np.random.seed(17)
        rec = []
        for it in range(5):
            i = cap - 2 + it
            tr = (data["observations"][i], data["actions"][i], float(data["rewards"][i]), data["next_observations"][i],
                  bool(data["terminals"][i]))
            who, gm = it % 3, 0.02
            if fused:
                log, a, use, h = t.online_step_jsrl(j, buf, *tr, B, tr[3], who, gate_max=gm)
            else:
                log = t.online_step(buf, *tr, B)
                (acts, u, hh), = j.act([tr[3]], [who], gate_max=[gm])
                a, use, h = acts[0], int(u[0]), float(hh[0])
            rec.append((np.float32([log["value_loss"], log["q_loss"], log["actor_loss"]]), np.float32(a), use, np.float32(h)))
        runs.append((t, buf, rec))
    (ta, ba, ra), (tb, bb, rb) = runs
    for it, (x, y) in enumerate(zip(ra, rb)):
        assert _same(x[0], y[0]) and _same(x[1], y[1]) and x[2] == y[2] and _same(x[3], y[3]), it
    assert_same_trainer_state(ta, tb)
    assert torch.equal(ba._rows, bb._rows) and ba._pointer == bb._pointer and ba._size == bb._size
    assert _act_calls(ta) == _act_calls(tb) == 5
    assert len({r[2] for r in ra}) == 2  # both the guide and the learner acted


def _raw(j, x, who, n=None, ld_s=None, ld_a=None, gate_max=0.0, want_h=False, flags=0, seed=0, handle=None):
    """One K = 1 call of the C entry point on device tensors; returns (rc, actions, use_learner, h)."""
    hb = _hip()[1]
    l = j.learners[0]
    S, A = l._S, l._A
    n = x.shape[0] if n is None else n
    xd = torch.from_numpy(x).cuda()
    out = torch.zeros((max(x.shape[0], 1), A), dtype=torch.float32, device="cuda")
    use = torch.zeros(max(x.shape[0], 1), dtype=torch.int32, device="cuda")
    h = torch.zeros(max(x.shape[0], 1), dtype=torch.float32, device="cuda")
    who = np.ascontiguousarray(who, dtype=np.int8)
    rc = hb.lib().iqlhip_jsrl_act(
        j._handle() if handle is None else handle, (C.c_void_p * 1)(xd.data_ptr()), S if ld_s is None else ld_s,
        (C.c_int32 * 1)(n), (C.c_void_p * 1)(who.ctypes.data), (C.c_float * 1)(gate_max), (C.c_uint64 * 1)(seed),
        (C.c_float * 1)(float(l.actor.max_action)), (C.c_float * 1)(float((j.guides[0] or l).actor.max_action)),
        (C.c_void_p * 1)(out.data_ptr()), A if ld_a is None else ld_a, (C.c_void_p * 1)(use.data_ptr()),
        (C.c_void_p * 1)(h.data_ptr() if want_h else None), flags, l._stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), use.cpu().numpy(), h.cpu().numpy()


def test_rejections_launch_and_count_nothing():
    iql, hb, _ = _hip()
    S, A, gaussian = 17, 6, True
    learner, twin = _trainer(S, A, gaussian, 760), _trainer(S, A, gaussian, 760)
    guide, gate = _trainer(S, A, gaussian, 761), _trainer(S, A, gaussian, 762)
    j, jn = iql.JsrlActors(learner, guide, gate), iql.JsrlActors(learner, guide)
    x = _states(3, S, 11)
    who = np.array([0, 1, 2], np.int8)
    lib = hb.lib()
    before = _act_calls(learner)
    bad = [(_raw(j, x, who, handle=C.c_void_p(None)), hb.E_INVAL), (_raw(j, x, who, n=4097), hb.E_INVAL),
           (_raw(j, x, who, ld_s=S - 1), hb.E_INVAL), (_raw(j, x, who, ld_a=A - 1), hb.E_INVAL),
           (_raw(j, x, np.array([0, 3, 1], np.int8)), hb.E_INVAL), (_raw(j, x, np.array([0, -1, 1], np.int8)), hb.E_INVAL),
           (_raw(jn, x, who), hb.E_INVAL), (_raw(jn, x, np.array([0, 1, 1], np.int8), want_h=True), hb.E_INVAL),
           (_raw(j, x, who, flags=8), hb.E_INVAL)]
    for i, ((rc, *_), code) in enumerate(bad):
        assert rc == code and hb.last_error(), i
    h = C.c_void_p()
    ctx = lambda t: (C.c_void_p * 1)(t._ctx)
    other_s, other_a = _trainer(S + 1, A, gaussian, 763), _trainer(S, A + 1, gaussian, 764)
    assert lib.iqlhip_jsrl_create(ctx(learner), ctx(other_s), None, 1, C.byref(h)) == hb.E_INVAL
    assert lib.iqlhip_jsrl_create(ctx(learner), ctx(guide), ctx(other_s), 1, C.byref(h)) == hb.E_INVAL
    assert lib.iqlhip_jsrl_create(ctx(learner), ctx(other_a), None, 1, C.byref(h)) == hb.E_INVAL
    assert lib.iqlhip_jsrl_create(None, ctx(guide), None, 1, C.byref(h)) == hb.E_INVAL
    assert lib.iqlhip_jsrl_create(ctx(learner), ctx(guide), None, 17, C.byref(h)) == hb.E_INVAL
    # an unbound context as the gate
    d = hb.Dims(S, A, hb.IQLHIP_HIDDEN, 2, hb.POLICY_GAUSSIAN, 256)
    raw_ctx = C.c_void_p()
    hb.check(lib.iqlhip_create(C.byref(d), C.byref(learner._hyper_struct()), learner._dev.index, C.byref(raw_ctx)))
    hb.check(lib.iqlhip_jsrl_create(ctx(learner), ctx(guide), (C.c_void_p * 1)(raw_ctx), 1, C.byref(h)))
    assert _raw(j, x, who, handle=h)[0] == hb.E_NOTBOUND
    hb.check(lib.iqlhip_jsrl_destroy(h))
    hb.check(lib.iqlhip_destroy(raw_ctx))
    # inference dropout on the learner: refused by the library, composed from separate calls by the Python layer
    dl = _trainer(S, A, gaussian, 765, dropout=0.1)
    dl.set_act_dropout(True)
    dl.actor.train()
    jd = iql.JsrlActors(dl, guide, gate)
    dl._prepare_act()
    assert _raw(jd, x, who)[0] == hb.E_UNSUPPORTED
    (a, use, hh), = jd.act([x], [who], gate_max=[0.0])
    assert a.shape == (3, A) and list(use[:2]) == [0, 1] and hh.shape == (3,)
    # nothing was launched or counted: the next valid call gives the bitwise result of a fresh pair
    assert _act_calls(learner) == before
    rc, a, use, hv = _raw(j, x, who, gate_max=0.0, want_h=True, seed=learner._act_seed())
    assert rc == 0
    want = _expected(twin, guide, x, use, True)
    assert _same(a, want) and list(use[:2]) == [0, 1] and use[2] == int(hv[2] <= 0.0)
    assert _act_calls(learner) == before + 1 == _act_calls(twin)
