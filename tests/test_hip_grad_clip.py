"""GPU tests of gradient-norm clipping per optimizer (ImplicitQLearning.set_grad_clip / iqlhip_set_grad_clip; DESIGN.md
6e): the coefficient formula bit for bit against the step's own norms, the Adam moments of a first step against the
device's own flat gradient, that an off or never-binding limit changes nothing, graph replays across changed limits,
trainer groups against solo twins, the two refusals, and the setting surviving a re-created context.

Parameters after ONE step from fresh Adam state are never compared on their own: Adam's first update
lr * g / (|g| + eps') hardly depends on the scale of g.  The moments do (exp_avg ~ coef, exp_avg_sq ~ coef^2)."""
import os

import numpy as np
import pytest
import torch

import synth
from helpers import step_batch

pytestmark = pytest.mark.gpu

HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
GROUPS = ("vf", "qf", "actor")
# (S, A, gaussian, rows, precision): the clip kernels walk the parameter segments, not the batch — one row, one row past
# a 32-row tile, a full 256-row chunk; the smallest dims, a deterministic policy, the door dims; bf16 below 512 rows
CASES = {"S17A6_B1": (17, 6, True, 1, "f32"), "S29A8_det_B33": (29, 8, False, 33, "f32"),
         "S39A28_B256": (39, 28, True, 256, "f32"), "S17A6_B256_bf16": (17, 6, True, 256, "bf16")}
SCALES = (0.125, 0.999, 2.0)          # clipped hard, barely, not at all


def _hip():
    import iql
    import iqlhip_binding as hb
    import hip_helpers as hh
    return iql, hb, hh


def _build(name, seed=0):
    _, _, hh = _hip()
    S, A, gaussian, B, precision = CASES[name]
    tr = hh.build_hip_trainer(synth.synth_params(S, A, seed=70 + B + seed, gaussian=gaussian), S, A, gaussian, HYPER, LRS, 1000)
    if precision != "f32":
        tr.set_precision(precision)
    return tr


def _norms(log):
    return np.array([log["stats/grad_norm_" + g] for g in GROUPS], dtype=np.float32)


def _probe(tr, tb):
    """The three gradient norms of `tb` under tr's current parameters (tr takes the step: use a throw-away twin)."""
    tr.set_step_stats(True)
    return _norms(tr.train(tb))


def _clip_vec(tr):
    c = tr.last_grad_clip()
    return (np.array([c["norm_" + g] for g in GROUPS], dtype=np.float32),
            np.array([c["coef_" + g] for g in GROUPS], dtype=np.float32))


def _want_coef(m, norm):
    return np.float32(min(np.float32(m) / (np.float32(norm) + np.float32(1e-6)), np.float32(1.0)))


def _segs(tr):
    """Flat-arena element ranges of the three optimizer groups."""
    L = tr._layout
    b = [int(L.net[i].seg_begin) for i in range(4)] + [int(L.net[3].seg_end)]
    return {"vf": (b[0], b[1]), "qf": (b[1], b[3]), "actor": (b[3], b[4])}


# --------------------------------------------------------------------------------------- 1. the coefficient, exactly
@pytest.mark.parametrize("name", list(CASES))
def test_coefficients_are_the_formula_on_the_steps_own_norms(name):
    _, _, hh = _hip()
    S, A, _, B, _ = CASES[name]
    tb = hh.to_torch_batch(step_batch(S, A, B, seed=800 + B))
    probe = _probe(_build(name), tb)
    rot = list(CASES).index(name) % 3                  # which group gets which scale differs from case to case
    scale = [SCALES[(g + rot) % 3] for g in range(3)]
    M = [float(probe[g]) * scale[g] for g in range(3)]
    tr = _build(name)
    tr.set_step_stats(True)
    tr.set_grad_clip(M)
    assert tr.grad_clip == tuple(M)
    log = tr.train(tb)
    norm, coef = _clip_vec(tr)
    print(name, "norms", norm, "limits", M, "coefs", coef)
    assert np.array_equal(norm, _norms(log)) and np.array_equal(norm, probe)        # statistics 13..15, bit for bit
    for g in range(3):
        assert coef[g] == _want_coef(M[g], norm[g]), (name, g, coef[g], _want_coef(M[g], norm[g]))
        assert (coef[g] == 1.0) == (scale[g] == 2.0), (name, g, coef[g])
    assert coef[scale.index(0.125)] < 0.126 and 0.99 < coef[scale.index(0.999)] < 1.0


# ------------------------------------------------------------------- 2. first-step moments, the device's own gradient
def _ulp_err(got, want):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(want), np.float32(1e-37)))


def _moment_err(tr, tb, coef_of):
    """(worst ulp error of exp_avg, of exp_avg_sq) of tr's first step on tb against f32((1-b1) f32(g c)) and
    f32(f32((1-b2) f32(g c)) f32(g c)), g = flat_gradient(tb), c = coef_of(tr) per optimizer group."""
    n = int(tr._layout.n_params)
    g = tr.flat_gradient(tb)[:n].astype(np.float32)
    assert tr.total_it == 0
    tr.train(tb)
    c = coef_of(tr)
    gc = g.copy()
    for i, grp in enumerate(GROUPS):
        lo, hi = _segs(tr)[grp]
        gc[lo:hi] = g[lo:hi] * np.float32(c[i])
    want_m = np.float32(1.0 - 0.9) * gc
    want_v = (np.float32(1.0 - 0.999) * gc) * gc
    m, v = tr._m_arena.cpu().numpy()[:n], tr._v_arena.cpu().numpy()[:n]
    return float(_ulp_err(m, want_m).max()), float(_ulp_err(v, want_v).max()), m, v


@pytest.mark.parametrize("name", ["S17A6_B1", "S39A28_B256"])
def test_first_step_moments_scale_with_the_coefficient(name):
    """Baseline (clipping off, c = 1) measured on an MI355X: 0 ulp for both moments in both cases — the step's gradient
    is flat_gradient's bit for bit and the expected roundings are the kernel's.  The clipped step is held to that
    baseline plus 4 ulp (the coefficient multiply adds one rounding in front of two, respectively three)."""
    _, _, hh = _hip()
    S, A, _, B, _ = CASES[name]
    tb = hh.to_torch_batch(step_batch(S, A, B, seed=810 + B))
    probe = _probe(_build(name), tb)
    off, on = _build(name), _build(name)
    base_m, base_v, m_off, v_off = _moment_err(off, tb, lambda t: (1.0, 1.0, 1.0))
    on.set_grad_clip({"vf": float(probe[0]) / 8, "actor": float(probe[2]) * 0.999})      # qf: no limit
    err_m, err_v, m_on, v_on = _moment_err(on, tb, lambda t: _clip_vec(t)[1])
    _, coef = _clip_vec(on)
    print(name, "baseline ulp", base_m, base_v, "clipped ulp", err_m, err_v, "coef", coef)
    assert coef[0] < 0.126 and coef[1] == 1.0 and 0.99 < coef[2] < 1.0
    assert err_m <= base_m + 4 and err_v <= base_v + 4, (name, base_m, base_v, err_m, err_v)
    lo, hi = _segs(on)["qf"]
    assert np.array_equal(m_on[lo:hi], m_off[lo:hi]) and np.array_equal(v_on[lo:hi], v_off[lo:hi])
    lo, hi = _segs(on)["vf"]                           # ... and the clipped group's did move: by coef and coef^2
    nz = np.abs(m_off[lo:hi]) > 0
    assert nz.any() and np.allclose(m_on[lo:hi][nz] / m_off[lo:hi][nz], coef[0], rtol=1e-5)
    assert np.allclose(v_on[lo:hi][nz] / v_off[lo:hi][nz], float(coef[0]) ** 2, rtol=1e-5)


# -------------------------------------------------------------------------------- 3. the oracle, over several steps
ORACLE_STEPS = 5
ORACLE_LIMITS = {"vf": 0.3, "qf": 0.1, "actor": 0.4}
# the oracle's own clip pattern under these limits (asserted below from the oracle alone): V is clipped on the first two
# steps and no longer from the third on, both Q nets and the policy on every step
ORACLE_PATTERN = {"vf": (True, True, False, False, False), "qf": (True,) * 5, "actor": (True,) * 5}
MOMENT_STEP_RTOL = 1e-5        # tests/test_hip_parity.py's moment tolerance of ONE step, relative to the tensor's largest value
NORM_RTOL = 1024 * 2.0 ** -24  # the proven bound on a device norm (6.1e-5); twice for exp_avg_sq


def _oracle_run(limits):
    """5 free-running oracle steps on fixed batches, each step's gradient scaled by clip_ref (limits None: unclipped)."""
    import clip_ref
    from oracle import iql_oracle as O
    S, A, B = 17, 6, 33
    hyper = dict(HYPER, deterministic=False)
    params = synth.synth_params(S, A, seed=91)
    start = params
    opt = O.new_opt_state(params)
    batches = [step_batch(S, A, B, seed=600 + k) for k in range(ORACLE_STEPS)]
    norms, coefs = [], []
    for b in batches:
        grads = O.iql_losses_and_grads(params, b, hyper)["grads"]
        if limits is not None:
            grads, n, c = clip_ref.clip_coefs(grads, limits)
            norms.append([float(n[g]) for g in GROUPS]), coefs.append([float(c[g]) for g in GROUPS])
        params, opt, _ = O.iql_step(params, opt, b, hyper, LRS, grads_override=grads)
    return {"S": S, "A": A, "start": start, "batches": batches, "params": params, "opt": opt,
            "norms": np.array(norms), "coefs": np.array(coefs)}


def test_five_clipped_steps_match_the_oracle():
    """Free-running: the device's 5 clipped steps against 5 oracle steps whose gradients tests/clip_ref.py scaled.
    Parameters and targets: tests/test_hip_parity.py's free-run bound (helpers.assert_params_after_free_run).  Moments:
    parity holds one step's moments to 1e-5 of the tensor's largest value; a moment after n steps is a weighted sum of
    n gradients with weights summing to less than 1, so n such allowances bound it, plus — per element — the device
    norm's proven relative bound once for exp_avg (it scales with coef) and twice for exp_avg_sq (coef^2)."""
    from helpers import assert_params_after_free_run
    _, _, hh = _hip()
    ref = _oracle_run(ORACLE_LIMITS)
    # the property that makes the test mean something, from the oracle alone: who is clipped when, with a margin that a
    # device norm within NORM_RTOL of the oracle's cannot cross
    for gi, grp in enumerate(GROUPS):
        assert tuple(bool(c < 1.0) for c in ref["coefs"][:, gi]) == ORACLE_PATTERN[grp], (grp, ref["coefs"][:, gi])
        assert np.all(np.abs(ref["norms"][:, gi] / ORACLE_LIMITS[grp] - 1.0) > 0.05), (grp, ref["norms"][:, gi])
    assert all(any(ORACLE_PATTERN[g][k] for g in GROUPS) for k in range(ORACLE_STEPS))
    assert ORACLE_PATTERN["vf"][0] and not ORACLE_PATTERN["vf"][-1]
    S, A = ref["S"], ref["A"]
    trainers = {}
    for which, limits in (("clipped", ORACLE_LIMITS), ("off", None)):
        tr = hh.build_hip_trainer(ref["start"], S, A, True, HYPER, LRS, None)
        tr.set_grad_clip(limits)
        coefs = []
        for b in ref["batches"]:
            tr.train(hh.to_torch_batch(b))
            if limits is not None:
                coefs.append(_clip_vec(tr)[1])
        trainers[which] = (hh.read_params(tr), hh.read_moments(tr), np.array(coefs))
    got_p, got_o, coefs = trainers["clipped"]
    print("oracle coefs", ref["coefs"].tolist(), "device coefs", coefs.tolist())
    assert np.array_equal(coefs < 1.0, ref["coefs"] < 1.0)
    for net, tensors in got_p.items():
        lr = LRS["pi" if net == "pi" else ("v" if net == "vf" else "q")]
        for k, p in tensors.items():
            assert_params_after_free_run(p, ref["params"][net][k], ORACLE_STEPS, lr, (net, k))
    worst = {"m": 0.0, "v": 0.0}
    for mv, widen in (("m", NORM_RTOL), ("v", 2 * NORM_RTOL)):
        for net in got_o[mv]:
            for k, got in got_o[mv][net].items():
                want = ref["opt"][mv][net][k].astype(np.float64)
                tol = ORACLE_STEPS * MOMENT_STEP_RTOL * np.max(np.abs(want)) + widen * np.abs(want)
                err = np.abs(got.astype(np.float64) - want)
                worst[mv] = max(worst[mv], float(np.max(err / tol)))
                print(mv, net, k, "max err / tol", float(np.max(err / tol)))
                assert np.all(err <= tol), (mv, net, k, float(np.max(err / tol)))
                if mv == "m" and net != "vf":        # the groups clipped on every step: the unclipped twin is far away
                    apart = float(np.max(np.abs(trainers["off"][1]["m"][net][k].astype(np.float64) - want)))
                    print("  unclipped twin apart by", apart, "tolerance", float(np.max(tol)))
                    assert apart > 10 * float(np.max(tol)), (net, k, apart, float(np.max(tol)))
    print("worst err / tol", worst)


# ------------------------------------------------------------------------------ 4. off and "never binds" change nothing
def _twins(i, n=2, S=17, A=6, **kw):
    from test_hip_group_online import _pair
    out = []
    while len(out) < n:
        out += _pair(i, S, A, True, **kw)
    return out[:n]


def _losses_of(log):
    return [log["value_loss"], log["q_loss"], log["actor_loss"]]


def test_off_and_never_binding_limits_change_nothing():
    from test_hip_group import _buffer
    _, _, hh = _hip()
    S, A, B = 17, 6, 100
    never, toggled, huge = _twins(0, 3)
    toggled.set_grad_clip(0.01)
    toggled.set_grad_clip(None)
    huge.set_grad_clip(1e30)
    assert never.grad_clip is None and toggled.grad_clip is None and huge.grad_clip == (1e30, 1e30, 1e30)
    buf = _buffer(3000, 31)
    for step in range(8):
        tb = hh.to_torch_batch(step_batch(S, A, B, seed=400 + step))
        logs = [t.train(tb) for t in (never, toggled, huge)]
        assert logs[0] == logs[1] == logs[2] and list(logs[0]) == ["value_loss", "q_loss", "actor_loss"], step
    losses = [t.train_steps(buf, 40, B, seed=3) for t in (never, toggled, huge)]
    assert np.array_equal(losses[0], losses[1]) and np.array_equal(losses[0], losses[2])
    assert np.array_equal(_clip_vec(huge)[1], np.ones(3, dtype=np.float32))
    for other, what in ((toggled, "set then None"), (huge, "max_norm 1e30")):
        hh.assert_same_trainer_state(never, other, what)
        assert np.array_equal(hh.arenas(never), hh.arenas(other)), what


# ---------------------------------------------------------------------------- 5. graphs and changes between the calls
def test_limits_changed_between_graph_calls_equal_eager_steps():
    from test_hip_group import _buffer
    iql, _, hh = _hip()
    S, A, B, n = 17, 6, 100, 20
    tb = hh.to_torch_batch(step_batch(S, A, B, seed=420))
    probe = _probe(_twins(1, 1)[0], tb)
    M1 = tuple(float(x) / 16 for x in probe)
    M2 = (float(probe[0]) / 8, float("inf"), float(probe[2]) / 10)
    g, e = _twins(1)
    buf = _buffer(3000, 32)
    seed = 0
    for rounds in range(2):                            # second round: each setting's graphs replayed after the other's
        for limit in (M1, M2, None, M1):
            seed += 1
            for t in (g, e):
                t.set_grad_clip(limit)
            want = hh.eager_segment(e, buf, n, B, seed)
            got = g.train_steps(buf, n, B, seed=seed)
            assert np.array_equal(got, want), (rounds, limit)
            if limit is not None:
                ng, cg = _clip_vec(g)
                ne, ce = _clip_vec(e)
                assert np.array_equal(ng, ne) and np.array_equal(cg, ce), (rounds, limit)
                assert cg.min() < 1.0 and (limit is not M2 or cg[1] == 1.0), (rounds, limit, cg)
            hh.assert_same_trainer_state(g, e, f"round {rounds} limit {limit}")
    # an online iteration with clipping on against add_transition + sample + train
    st = synth.synth_transitions(4, S, A, seed=77, antmaze_rewards=True)
    rings = [iql.ReplayBuffer(S, A, 64, "cuda") for _ in range(2)]
    for it in range(3):
        tr_ = (st["observations"][it], st["actions"][it], float(st["rewards"][it]), st["next_observations"][it],
               bool(st["terminals"][it]))
        np.random.seed(50 + it)
        la = g.online_step(rings[0], *tr_, 32)
        np.random.seed(50 + it)
        rings[1].add_transition(*tr_)
        lb = e.train(rings[1].sample(32))
        assert la == lb, it
        assert np.array_equal(_clip_vec(g)[1], _clip_vec(e)[1]) and _clip_vec(g)[1].min() < 1.0
    hh.assert_same_trainer_state(g, e, "online")
    assert np.array_equal(hh.arenas(g), hh.arenas(e))


# ------------------------------------------------------------------------------------------------------- 6. groups
def _group_limits(K, probe_of):
    """Member 0 clips all three groups, member 1 only the actor, member 2 (if any) nothing."""
    out = []
    for i in range(K):
        p = probe_of(i)
        out.append([tuple(float(x) / 16 for x in p), {"actor": float(p[2]) / 16}, None][i % 3])
    return out


def _check_members(members, twins, limits, what):
    from test_hip_group import _assert_same_state
    for i, (a, b) in enumerate(zip(members, twins)):
        _assert_same_state(a, b, f"{what}: member {i} against its solo twin")
        assert np.array_equal(_arenas(a), _arenas(b)), (what, i)
        if limits[i] is not None:
            (na, ca), (nb, cb) = _clip_vec(a), _clip_vec(b)
            assert np.array_equal(na, nb) and np.array_equal(ca, cb), (what, i, ca, cb)
            assert ca[2] < 1.0 and (ca[0] < 1.0) == isinstance(limits[i], tuple), (what, i, ca)


def _arenas(t):
    return _hip()[2].arenas(t)


def test_group_members_equal_their_solo_twins():
    from test_hip_group import _buffer
    from test_hip_group_online import _streams, _tr
    iql, _, hh = _hip()
    S, A, K, B = 17, 6, 3, 100
    first = [hh.to_torch_batch(step_batch(S, A, B, seed=50 * i)) for i in range(K)]
    limits = _group_limits(K, lambda i: _probe(_twins(i, 1)[0], first[i]))
    members, twins = [], []
    for i in range(K):
        a, b = _twins(i)
        for t in (a, b):
            t.set_grad_clip(limits[i])
        members.append(a), twins.append(b)
    group = iql.ImplicitQLearningGroup(members)
    for step in range(2):
        batches = first if step == 0 else [hh.to_torch_batch(step_batch(S, A, B, seed=50 * i + step)) for i in range(K)]
        logs = group.train(batches)
        assert logs == [twins[i].train(batches[i]) for i in range(K)], step
        _check_members(members, twins, limits, f"train {step}")
    buf, seeds, n = _buffer(3000, 33), [7, 8, 9], 12
    got = group.train_steps(buf, n, B, seeds)
    for i in range(K):
        assert np.array_equal(got[i], twins[i].train_steps(buf, n, B, seed=seeds[i])), i
    _check_members(members, twins, limits, "train_steps")
    rings = [[iql.ReplayBuffer(S, A, 40, "cuda") for _ in range(K)] for _ in range(2)]
    streams = _streams(K, 2, S, A)
    for it in range(2):
        args = [list(x) for x in zip(*[_tr(streams[k], it) for k in range(K)])]
        np.random.seed(60 + it)
        logs = group.online_step(rings[0], *args, 32)
        np.random.seed(60 + it)
        assert logs == [twins[k].online_step(rings[1][k], *_tr(streams[k], it), 32) for k in range(K)], it
    _check_members(members, twins, limits, "online_step")


def test_mixed_batch_group_members_equal_their_solo_twins():
    from test_hip_group import _buffer
    iql, _, hh = _hip()
    S, A, K, sizes = 17, 6, 3, (33, 64, 256)
    batches = [hh.to_torch_batch(step_batch(S, A, B, seed=80 + i)) for i, B in enumerate(sizes)]
    limits = _group_limits(K, lambda i: _probe(_twins(i, 1)[0], batches[i]))
    members, twins = [], []
    for i in range(K):
        a, b = _twins(i)
        for t in (a, b):
            t.set_grad_clip(limits[i])
        members.append(a), twins.append(b)
    group = iql.ImplicitQLearningGroup(members, mixed_batch=True)
    assert group.train(batches) == [twins[i].train(batches[i]) for i in range(K)]
    _check_members(members, twins, limits, "mixed train")
    buf, seeds, n = _buffer(3000, 34), [3, 4, 5], 12
    got = group.train_steps(buf, n, list(sizes), seeds)
    for i in range(K):
        assert np.array_equal(got[i], twins[i].train_steps(buf, n, sizes[i], seed=seeds[i])), i
    _check_members(members, twins, limits, "mixed train_steps")


def test_dropout_group_members_equal_their_solo_twins():
    from test_hip_group_dropout import _assert_same_state, _buffer, _pair
    iql, _, hh = _hip()
    S, A, K, B = 17, 6, 2, 100
    batches = [hh.to_torch_batch(step_batch(S, A, B, seed=90 + i)) for i in range(K)]
    limits = _group_limits(K, lambda i: _probe(_pair(i, True, 0.1, seed=100 + i)[0], batches[i]))
    pairs = [_pair(i, True, 0.1, seed=100 + i) for i in range(K)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    for i in range(K):
        for t in pairs[i]:
            t.set_grad_clip(limits[i])
    group = iql.ImplicitQLearningGroup(members, actor_dropout=True)
    assert group.train(batches) == [twins[i].train(batches[i]) for i in range(K)]
    buf, seeds, n = _buffer(3000, 35), [5, 6], 12
    got = group.train_steps(buf, n, B, seeds)
    for i in range(K):
        assert np.array_equal(got[i], twins[i].train_steps(buf, n, B, seed=seeds[i])), i
        _assert_same_state(members[i], twins[i], f"dropout member {i}")
    _check_members(members, twins, limits, "dropout group")


# ---------------------------------------------------------------------------------------------------- 7. refusals
def _untouched(tr, before, arenas_before):
    _, _, hh = _hip()
    torch.cuda.synchronize()
    assert np.array_equal(hh.arenas(tr), arenas_before)
    assert tr.total_it == 0 and tr._adam_t == before["adam_t"]
    assert tr.actor_optimizer.param_groups[0]["lr"] == before["lr"]


def test_large_batch_bf16_is_refused_before_any_launch():
    from test_hip_group import _buffer
    _, _, hh = _hip()
    S, A, B = 17, 6, 1024
    tr = hh.build_hip_trainer(synth.synth_params(S, A, seed=3), S, A, True, HYPER, LRS, 1000)
    tr.set_precision("bf16")
    tr.reserve_batch(B)
    tr.set_grad_clip(0.5)
    before = {"adam_t": dict(tr._adam_t), "lr": tr.actor_optimizer.param_groups[0]["lr"]}
    arenas_before = hh.arenas(tr)
    tb = hh.to_torch_batch(step_batch(S, A, B, seed=4))
    buf = _buffer(3000, 36)
    with pytest.raises(NotImplementedError, match="512 rows"):
        tr.train(tb)
    with pytest.raises(NotImplementedError, match="512 rows"):
        tr.train_steps(buf, 4, B, seed=1)
    _untouched(tr, before, arenas_before)
    # ... and by the library itself, for a caller of the C ABI (the Python check stepped over: the shim's own step
    # count is then no longer meaningful, the device state is)
    tr._check_grad_clip = lambda rows: None
    with pytest.raises(NotImplementedError, match="large-batch"):
        tr.train(tb)
    with pytest.raises(NotImplementedError, match="large-batch"):
        tr.train_steps(buf, 4, B, seed=1)
    torch.cuda.synchronize()
    assert np.array_equal(hh.arenas(tr), arenas_before)
    tr.total_it, tr._adam_t = 0, dict(before["adam_t"])
    del tr._check_grad_clip
    tr.train(hh.to_torch_batch(step_batch(S, A, 512, seed=5)))       # 512 rows in bf16 are supported
    assert _clip_vec(tr)[1].min() < 1.0 and np.all(np.isfinite(hh.arenas(tr)))


@pytest.fixture
def gloo_world1():
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(29600 + os.getpid() % 1000)
    dist.init_process_group("gloo", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


def test_an_exchange_is_refused_before_any_launch(gloo_world1):
    _, _, hh = _hip()
    S, A, B = 17, 6, 100
    tr = hh.build_hip_trainer(synth.synth_params(S, A, seed=6), S, A, True, HYPER, LRS, 1000)
    tr.set_grad_clip(0.5)
    tr.enable_data_parallel(exchange="p2p")
    before = {"adam_t": dict(tr._adam_t), "lr": tr.actor_optimizer.param_groups[0]["lr"]}
    arenas_before = hh.arenas(tr)
    tb = hh.to_torch_batch(step_batch(S, A, B, seed=7))
    with pytest.raises(NotImplementedError, match="data parallelism"):
        tr.train(tb)
    _untouched(tr, before, arenas_before)
    tr._check_grad_clip = lambda rows: None            # the library's own check
    with pytest.raises(NotImplementedError, match="data-parallel exchange"):
        tr.train(tb)
    torch.cuda.synchronize()
    assert np.array_equal(hh.arenas(tr), arenas_before)


# ------------------------------------------------------------------------------------------ 8. context re-creation
def test_the_setting_survives_a_recreated_context():
    _, _, hh = _hip()
    S, A, B = 17, 6, 300
    tb = hh.to_torch_batch(step_batch(S, A, B, seed=430))
    small = hh.to_torch_batch(step_batch(S, A, 64, seed=431))
    a, b = _twins(2)
    probe = _probe(_twins(2, 1)[0], small)
    M = (float(probe[0]) / 4, float("inf"), float(probe[2]) / 2)
    a.set_grad_clip(M)
    a.train(small)                                     # the first context holds the limits ...
    a.reserve_batch(512)                               # ... and is replaced
    b.reserve_batch(512)
    b.set_grad_clip({"vf": M[0], "actor": M[2]})
    b.train(small)
    assert a.grad_clip == b.grad_clip == M
    assert a.train(tb) == b.train(tb)
    (na, ca), (nb, cb) = _clip_vec(a), _clip_vec(b)
    assert np.array_equal(na, nb) and np.array_equal(ca, cb) and ca[1] == 1.0 and ca.min() < 1.0, (ca, cb)
    hh.assert_same_trainer_state(a, b, "after reserve_batch")
    assert np.array_equal(hh.arenas(a), hh.arenas(b))
