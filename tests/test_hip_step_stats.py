"""GPU tests of the per-step training statistics (ImplicitQLearning.set_step_stats / iqlhip_set_step_stats; DESIGN.md
6d): the 13 row statistics against the float64 restatement (tests/stats_ref.py) fed with the step's own head partials
and packed batch, the head values against the CPU port, the gradient norms against the flat gradient, and — the
feature is opt-in — that nothing else moves: parameters, moments, losses, actions and random-stream counters are
bit-identical with statistics on and off, solo and in groups, across the chunk-graph cache.

Tolerances.  Means: B * 2^-24 * max|x| (recursive fp32 summation of the B per-row terms x, computed from the data).
exp_adv_mean additionally EXPF_MARGIN * mean(w): four times the largest relative deviation of the device's
expf(beta * adv) from the float64 exp measured over single-row steps on rows of these cases (EXPF_MEASURED below).
Gradient norms: GRADSQ_TERMS * 2^-24 relative, GRADSQ_TERMS = 1024 being the terms one fp32 accumulator of
iql_stats_gradsq_kernel stands for (its comment in csrc/iqlhip_kernels.h).  Min, max and the two shares are exact."""
import functools

import numpy as np
import pytest
import torch

import stats_ref
import synth
from helpers import check_step_against_golden, step_batch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EXPF_MEASURED = 2.13e-7        # largest relative deviation seen: 297 single-row steps, beta * adv in [-4.1, 8.1]
EXPF_MARGIN = 4 * EXPF_MEASURED
GRADSQ_TERMS = 1024
HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
# (S, A, gaussian, B, precision): fewer rows than a wave; ragged, no multiple of 64; across the 256-row chunk with
# several rows per thread (this case's advantages are spread until some rows' weights sit on the clamp, not all); bf16
CASES = {"S17A6_B3": (17, 6, True, 3, "f32"), "S29A8_det_B100": (29, 8, False, 100, "f32"),
         "S39A28_B300": (39, 28, True, 300, "f32"), "S17A6_B256_bf16": (17, 6, True, 256, "bf16")}
CLAMP_CASE = "S39A28_B300"
FP32_CASES = [n for n, c in CASES.items() if c[4] == "f32"]


def _hip():
    import iql
    import iqlhip_binding as hb
    from hip_helpers import build_hip_trainer, head_values, read_moments, read_params, to_torch_batch
    return iql, hb, build_hip_trainer, head_values, read_moments, read_params, to_torch_batch


def _params_for(name):
    S, A, gaussian, B, precision = CASES[name]
    params = synth.synth_params(S, A, seed=40 + B, gaussian=gaussian)
    if name == CLAMP_CASE:
        # statistic 12 away from 0: the rewards do not enter adv = min(tQ1, tQ2) - V(s), so it is the target critics'
        # output layer that is scaled and shifted until beta * adv straddles log(EXP_ADV_MAX) (CPU port: 35 of the
        # 300 rows above it, the nearest 1.3e-2 away; asserted from the device's heads in the test)
        params["qt1"]["w2"] = params["qt1"]["w2"] * np.float32(12.0)
        params["qt2"]["w2"] = params["qt2"]["w2"] * np.float32(12.0)
        params["qt1"]["b2"] = params["qt1"]["b2"] + np.float32(1.2)
        params["qt2"]["b2"] = params["qt2"]["b2"] + np.float32(1.2)
    return params


@functools.lru_cache(maxsize=None)
def _case(name):
    """One train() with statistics on: everything the tests 1-3 compare, computed once and left unchanged."""
    _, hb, build, head_values, _, _, to_tb = _hip()
    S, A, gaussian, B, precision = CASES[name]
    params = _params_for(name)
    batch = step_batch(S, A, B, seed=900 + B)
    tr = build(params, S, A, gaussian, HYPER, LRS, 1000)
    if precision != "f32":
        tr.set_precision(precision)
    tr.set_step_stats(True)
    tb = to_tb(batch)
    flat = tr.flat_gradient(tb)                       # same batch, same (pre-update) parameters as the step below
    log = tr.train(tb)
    hv = head_values(tr, params, B)                   # fp32 sum4 of the step's head partials, the step's own order
    xb = tr.debug_read("xb")
    ld = hb.row_stride(S, A)
    rows = xb[: B * ld].reshape(B, ld)
    L = tr._layout
    segs = [(int(L.net[i].seg_begin), int(L.net[i].seg_end)) for i in range(4)]
    return {"log": log, "stats": np.array([log["stats/" + n] for n in hb.STAT_NAMES], dtype=np.float32), "hv": hv,
            "r": rows[:, 2 * S + A].copy(), "d": rows[:, 2 * S + A + 1].copy(), "flat": flat, "segs": segs,
            "batch": batch, "params": params, "n_params": int(L.n_params)}


# ------------------------------------------------------------------------------------------- 1. the row statistics
@pytest.mark.parametrize("name", list(CASES))
def test_row_statistics_match_the_restatement(name):
    S, A, gaussian, B, precision = CASES[name]
    c = _case(name)
    hv, got = c["hv"], c["stats"]
    assert np.array_equal(c["r"], c["batch"]["r"]) and np.array_equal(c["d"], c["batch"]["d"])   # the packed columns
    heads = (hv["next_v"], hv["v"], hv["qt1"], hv["qt2"], hv["q1"], hv["q2"])
    t = stats_ref.row_terms(*heads, c["r"], c["d"], HYPER["beta"], HYPER["discount"])
    want = stats_ref.row_stats(*heads, c["r"], c["d"], HYPER["beta"], HYPER["discount"])
    adv = t["adv"]
    # the counts are only comparable away from their thresholds
    assert np.min(np.abs(HYPER["beta"] * adv - np.log(stats_ref.EXP_ADV_MAX))) > 1e-4, name
    assert np.min(np.abs(adv)) > 1e-6, name
    if name == CLAMP_CASE:
        assert 0 < int(t["clamped"].sum()) < B, int(t["clamped"].sum())
    terms = {0: t["v"], 1: t["next_v"], 2: t["q1"], 3: t["q2"], 4: t["tq"], 5: t["y"], 6: np.abs(t["q1"] - t["q2"]),
             7: adv, 11: t["w"]}
    for i, x in terms.items():
        tol = B * U * float(np.max(np.abs(x)))
        if i == 11:
            tol += EXPF_MARGIN * float(np.mean(x))
        err = abs(float(got[i]) - want[i])
        print(f"{name} {stats_ref.STAT_NAMES[i]}: got {got[i]!r} want {want[i]!r} err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (name, stats_ref.STAT_NAMES[i], float(got[i]), want[i], err, tol)
    # exact: min / max (the fp32 difference of two fp32 heads is the rounded exact difference) and the two shares
    assert got[8] == np.float32(want[8]) and got[9] == np.float32(want[9]), (name, got[8:10], want[8:10])
    n_pos, n_clamp = int(np.sum(~(adv < 0))), int(t["clamped"].sum())
    assert got[10] == np.float32(n_pos) / np.float32(B), (name, got[10], n_pos)
    assert got[12] == np.float32(n_clamp) / np.float32(B), (name, got[12], n_clamp)
    assert np.all(np.isfinite(got))


# ---------------------------------------------------------------------------------------------- 2. the head meaning
@pytest.mark.parametrize("name", FP32_CASES)
def test_head_values_are_the_cpu_ports(name):
    """Which instance is which: the six head values the statistics rest on against the CPU port's V(s'), V(s), target
    Q1 / Q2, Q1, Q2 for the same batch and parameters, at the bound tests/test_hip_parity.py holds forward outputs to
    (helpers.check_step_against_golden's `inter.*` check, applied to each value in turn).  fp32 cases: that bound is
    the fp32 kernels' (the bf16 path is held to its own, looser, bounds in tests/test_hip_parity.py)."""
    from oracle import iql_torch_port as port
    S, A, gaussian, B, _ = CASES[name]
    c = _case(name)
    params, batch, hv = c["params"], c["batch"], c["hv"]
    torch.set_num_threads(1)
    cpu = port.CpuIQL(S, A, params=params, gaussian=gaussian, iql_tau=HYPER["iql_tau"], beta=HYPER["beta"],
                      discount=HYPER["discount"], tau=HYPER["tau"], lrs=LRS, max_steps=1000)
    s, a, ns = (torch.from_numpy(batch[k]) for k in ("s", "a", "ns"))
    with torch.no_grad():
        want = {"v": cpu.vf(s).numpy(), "next_v": cpu.vf(ns).numpy()}
        want["q1"], want["q2"] = (x.numpy() for x in cpu.qf.both(s, a))
        want["qt1"], want["qt2"] = (x.numpy() for x in cpu.q_target.both(s, a))
    losses = np.array([c["log"]["value_loss"], c["log"]["q_loss"], c["log"]["actor_loss"]])
    for trio in (("next_v", "v", "q1"), ("q2", "qt1", "qt2")):
        z = {"losses": losses, "inter.next_v": want[trio[0]], "inter.target_q": want[trio[1]], "inter.adv": want[trio[2]]}
        info = {"value_loss": losses[0], "q_loss": losses[1], "actor_loss": losses[2], "next_v": hv[trio[0]],
                "target_q": hv[trio[1]], "adv": hv[trio[2]]}
        check_step_against_golden(z, {"stride": 1}, info, None, None)
    # ... and the twins are told apart by the data (an exchanged pair would sit far outside that bound)
    assert np.max(np.abs(want["q1"] - want["q2"])) > 1e-3 and np.max(np.abs(want["qt1"] - want["qt2"])) > 1e-3
    assert np.max(np.abs(want["v"] - want["next_v"])) > 1e-3


# ------------------------------------------------------------------------------------------- 3. the gradient norms
@pytest.mark.parametrize("name", list(CASES))
def test_gradient_norms_match_the_flat_gradient(name):
    rtol = GRADSQ_TERMS * U
    assert rtol < 1e-4
    c = _case(name)
    want = stats_ref.grad_norms(c["flat"][: c["n_params"]], c["segs"])
    got = c["stats"][13:16].astype(np.float64)
    rel = np.abs(got - want) / want
    print(f"{name} grad norms got {got} want {want} rel err {rel} (tol {rtol:.3e})")
    assert np.all(want > 0) and np.all(rel <= rtol), (name, got, want, rel)


# ---------------------------------------------------------------------------------------------- 4. nothing else moves
def _twins(i=0, S=17, A=6, gaussian=True, precision="f32"):
    from test_hip_group_online import _pair
    return _pair(i, S, A, gaussian, precision)


def _stat_vec(log):
    import iqlhip_binding as hb
    return np.array([log["stats/" + n] for n in hb.STAT_NAMES], dtype=np.float32)


def _losses_of(log):
    return [log["value_loss"], log["q_loss"], log["actor_loss"]]


def test_statistics_change_nothing_else():
    from test_hip_group import _buffer
    from test_hip_group_online import _assert_same, _streams, _tr
    iql, hb, _, _, _, _, to_tb = _hip()
    S, A, B = 17, 6, 256
    on, off = _twins()
    on.set_step_stats(True)
    for t in (on, off):
        t.actor.train()                               # (device noise in the returned actions: the act() counter moves)
    for step in range(8):
        tb = to_tb(step_batch(S, A, B, seed=300 + step))
        a, b = on.train(tb), off.train(tb)
        assert list(b) == ["value_loss", "q_loss", "actor_loss"] and _losses_of(a) == _losses_of(b), step
        assert len(a) == 19 and np.all(np.isfinite(_stat_vec(a)))
    rings = [iql.ReplayBuffer(S, A, 64, "cuda") for _ in range(2)]
    stream = _streams(1, 8, S, A)[0]
    for t, ring in ((on, rings[0]), (off, rings[1])):
        np.random.seed(11)
        t._online = [t.online_step(ring, *_tr(stream, it), 32, act_next=_tr(stream, it)[3]) for it in range(8)]
    for (la, aa), (lb, ab) in zip(on._online, off._online):
        assert _losses_of(la) == _losses_of(lb) and len(la) == 19 and len(lb) == 3
        assert np.array_equal(aa, ab)
    buf = _buffer(5000, 22)
    n = 130                                            # the direct head + two 64-step chunk graphs
    la, sa = on.train_steps(buf, n, B, seed=5, return_stats=True)
    lb = off.train_steps(buf, n, B, seed=5)
    assert np.array_equal(la, lb) and sa.shape == (n, 16) and np.all(np.isfinite(sa))
    _assert_same(on, off, rings[0], rings[1], "statistics on against off")


def test_ring_rows_equal_the_same_steps_taken_one_by_one():
    from test_hip_group import _buffer
    S, A, B, n = 17, 6, 256, 130
    ring_tr, eager = _twins(1)
    for t in (ring_tr, eager):
        t.set_step_stats(True)
    buf = _buffer(5000, 23)
    losses, stats = ring_tr.train_steps(buf, n, B, seed=9, return_stats=True)
    for k in range(n):
        log = eager.train_on_buffer(buf, B, seed=9, sync=True)        # the same indices, drawn the same way
        assert _losses_of(log) == [float(x) for x in losses[k]], k
        assert np.array_equal(_stat_vec(log), stats[k]), (k, _stat_vec(log), stats[k])
    assert len({tuple(r) for r in stats.tolist()}) == n               # every step wrote its own row


# ------------------------------------------------------------------------------------------------------- 5. toggle
def test_toggling_between_calls_keeps_the_graph_caches_apart():
    from test_hip_group import _buffer
    from test_hip_group_online import _assert_same
    S, A, B, n = 17, 6, 100, 70                        # head + a 64-step and a 4-step chunk graph per setting
    t, ref = _twins(2)
    buf = _buffer(3000, 24)
    want = [ref.train_steps(buf, n, B, seed=s) for s in (1, 2, 3)]
    first = t.train_steps(buf, n, B, seed=1)
    t.set_step_stats(True)
    mid, stats = t.train_steps(buf, n, B, seed=2, return_stats=True)
    t.set_step_stats(False)
    last = t.train_steps(buf, n, B, seed=3)
    assert np.array_equal(first, want[0]) and np.array_equal(mid, want[1]) and np.array_equal(last, want[2])
    assert stats.shape == (n, 16) and np.all(np.isfinite(stats))
    with pytest.raises(ValueError, match="set_step_stats"):
        t.train_steps(buf, 2, B, seed=4, return_stats=True)
    _assert_same(t, ref, None, None, "off / on / off against off only")


# ------------------------------------------------------------------------------------------------------- 6. groups
def _group_members(K, enabled):
    """K (member, solo twin, member of a statistics-off group) triples; `enabled`: who has statistics on."""
    from test_hip_group_online import _pair
    members, twins, plain = [], [], []
    for i in range(K):
        a, b = _pair(i, 17, 6, True)
        c = _pair(i, 17, 6, True)[0]
        for t in (a, b):
            t.set_step_stats(bool(enabled[i]))
        members.append(a), twins.append(b), plain.append(c)
    return members, twins, plain


def _check_group_logs(logs, twin_logs, enabled, what):
    for i, (lg, lt) in enumerate(zip(logs, twin_logs)):
        assert lg == lt, (what, i, lg, lt)                              # losses and statistics, bit for bit
        assert len(lg) == (19 if enabled[i] else 3), (what, i)


def test_group_statistics_equal_solo_statistics():
    from test_hip_group import _assert_same_state, _buffer
    from test_hip_group_online import _assert_same, _streams, _tr
    iql, hb, _, _, _, _, to_tb = _hip()
    S, A, K, B = 17, 6, 3, 100
    enabled = (True, False, True)
    members, twins, plain = _group_members(K, enabled)
    group, group_off = iql.ImplicitQLearningGroup(members), iql.ImplicitQLearningGroup(plain)
    for step in range(2):
        batches = [to_tb(step_batch(S, A, B, seed=50 * i + step)) for i in range(K)]
        logs = group.train(batches)
        _check_group_logs(logs, [twins[i].train(batches[i]) for i in range(K)], enabled, f"train {step}")
        off_logs = group_off.train(batches)
        assert [_losses_of(x) for x in off_logs] == [_losses_of(x) for x in logs]
    buf, seeds, n = _buffer(3000, 25), [7, 8, 9], 5
    stats = group.train_steps(buf, n, B, seeds, return_stats=True)
    assert stats.shape == (n, K, 16)
    group_off.train_steps(buf, n, B, seeds)
    with pytest.raises(ValueError, match="set_step_stats"):
        group_off.train_steps(buf, n, B, seeds, return_stats=True)
    for i in range(K):
        if enabled[i]:
            _, want = twins[i].train_steps(buf, n, B, seed=seeds[i], return_stats=True)
            assert np.array_equal(stats[:, i], want), i
        else:
            twins[i].train_steps(buf, n, B, seed=seeds[i])
            assert np.all(np.isnan(stats[:, i])), i
    rings = [[iql.ReplayBuffer(S, A, 40, "cuda") for _ in range(K)] for _ in range(3)]
    streams = _streams(K, 2, S, A)
    for it in range(2):
        args = [list(x) for x in zip(*[_tr(streams[k], it) for k in range(K)])]
        np.random.seed(60 + it)
        logs = group.online_step(rings[0], *args, 32)
        np.random.seed(60 + it)
        want = [twins[k].online_step(rings[1][k], *_tr(streams[k], it), 32) for k in range(K)]
        _check_group_logs(logs, want, enabled, f"online {it}")
        np.random.seed(60 + it)
        group_off.online_step(rings[2], *args, 32)
    # (state against the solo twin as tests/test_hip_group.py compares it: a plain group's train_steps leaves the
    #  members' keep-bit stream positions alone; against the statistics-off group every counter is compared too)
    for i in range(K):
        _assert_same_state(members[i], twins[i], f"member {i} against its solo twin")
        assert torch.equal(rings[0][i]._rows, rings[1][i]._rows), i
        _assert_same(members[i], plain[i], rings[0][i], rings[2][i], f"member {i} against the statistics-off group")


def test_mixed_batch_group_statistics_equal_solo_statistics():
    from test_hip_group import _assert_same_state, _buffer
    from test_hip_group_online import _assert_same
    iql, hb, _, _, _, _, to_tb = _hip()
    S, A, K, sizes = 17, 6, 3, (64, 128, 256)
    enabled = (True, False, True)
    members, twins, plain = _group_members(K, enabled)
    group = iql.ImplicitQLearningGroup(members, mixed_batch=True)
    group_off = iql.ImplicitQLearningGroup(plain, mixed_batch=True)
    batches = [to_tb(step_batch(S, A, B, seed=80 + i)) for i, B in enumerate(sizes)]
    _check_group_logs(group.train(batches), [twins[i].train(batches[i]) for i in range(K)], enabled, "mixed train")
    group_off.train(batches)
    buf, seeds, n = _buffer(3000, 26), [3, 4, 5], 5
    stats = group.train_steps(buf, n, list(sizes), seeds, return_stats=True)
    group_off.train_steps(buf, n, list(sizes), seeds)
    for i in range(K):
        if enabled[i]:
            _, want = twins[i].train_steps(buf, n, sizes[i], seed=seeds[i], return_stats=True)
            assert np.array_equal(stats[:, i], want), i
        else:
            twins[i].train_steps(buf, n, sizes[i], seed=seeds[i])
            assert np.all(np.isnan(stats[:, i])), i
        _assert_same_state(members[i], twins[i], f"member {i} against its solo twin")
        _assert_same(members[i], plain[i], None, None, f"member {i} against the statistics-off group")


# ---------------------------------------------------------------------------------------------------- 7. refusals
def test_large_batch_bf16_is_refused_before_any_launch():
    from test_hip_group import _buffer
    _, hb, build, _, _, read_params, to_tb = _hip()
    S, A, B = 17, 6, 1024
    tr = build(synth.synth_params(S, A, seed=3), S, A, True, HYPER, LRS, 1000)
    tr.set_precision("bf16")
    tr.reserve_batch(B)
    tr.set_step_stats(True)
    before = read_params(tr)
    tb = to_tb(step_batch(S, A, B, seed=4))
    buf = _buffer(3000, 27)
    with pytest.raises(NotImplementedError, match="512 rows"):
        tr.train(tb)
    with pytest.raises(NotImplementedError, match="512 rows"):
        tr.train_steps(buf, 4, B, seed=1, return_stats=True)
    assert tr.total_it == 0
    # ... and by the library itself, for a caller of the C ABI (the Python check stepped over)
    tr._check_step_stats = lambda rows: None
    with pytest.raises(NotImplementedError, match="large-batch"):
        tr.train(tb)
    with pytest.raises(NotImplementedError, match="large-batch"):
        tr.train_steps(buf, 4, B, seed=1)
    torch.cuda.synchronize()
    after = read_params(tr)
    for n in before:
        for k in before[n]:
            assert np.array_equal(before[n][k], after[n][k]), (n, k)
    # 512 rows in bf16 are supported
    del tr._check_step_stats
    log = tr.train(to_tb(step_batch(S, A, 512, seed=5)))
    assert len(log) == 19 and np.all(np.isfinite(list(log.values())))
