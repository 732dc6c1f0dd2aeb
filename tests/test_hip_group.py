"""GPU tests of trainer groups (ImplicitQLearningGroup / iqlhip_group_*): every member of a group ends exactly — bit
for bit — where a twin (a trainer built identically that runs the same steps alone) ends, for eager steps on
caller-given batches and for device-drawn steps; a member built from a reference fixture reproduces its free-run
losses while it trains next to two other agents; a member handed back to solo training continues correctly; bad
groups are rejected before anything is launched."""
import numpy as np
import pytest
import torch

import synth
from helpers import assert_losses, batch_from, fwd_spb_l2, load_golden, step_batch, w0_lds_k

pytestmark = pytest.mark.gpu

S, A = 17, 6


def _hip():
    import iql
    from hip_helpers import build_hip_trainer, read_moments, read_params, to_torch_batch
    return iql, build_hip_trainer, read_moments, read_params, to_torch_batch


def _spec(i, gaussian, S_=S, A_=A):
    """Member i: its own synthetic parameters, expectile, temperature and learning rates."""
    params = synth.synth_params(S_, A_, seed=300 + i, gaussian=gaussian)
    hyper = {"iql_tau": 0.6 + 0.1 * i, "beta": 2.0 + i, "discount": 0.99, "tau": 0.005 * (1 + i)}
    lrs = {"v": 3e-4 * (1 + i), "q": 2e-4 * (1 + i), "pi": 1e-4 * (1 + i)}
    return params, hyper, lrs


def _pair(i, gaussian, max_steps=1000, precision="f32", S_=S, A_=A):
    _, build, _, _, _ = _hip()
    params, hyper, lrs = _spec(i, gaussian, S_, A_)
    out = []
    for _ in range(2):
        t = build(params, S_, A_, gaussian, hyper, lrs, max_steps)
        if precision != "f32":
            t.set_precision(precision)
        out.append(t)
    return out


def _assert_same_state(a, b, what=""):
    _, _, read_moments, read_params, _ = _hip()
    pa, pb = read_params(a), read_params(b)
    for n in pa:
        for k in pa[n]:
            assert np.array_equal(pa[n][k], pb[n][k]), (what, "param", n, k)
    ma, mb = read_moments(a), read_moments(b)
    for which in ("m", "v"):
        for n in ma[which]:
            for k in ma[which][n]:
                assert np.array_equal(ma[which][n][k], mb[which][n][k]), (what, which, n, k)
    assert a.total_it == b.total_it, what
    assert a.actor_optimizer.param_groups[0]["lr"] == b.actor_optimizer.param_groups[0]["lr"], what
    sa, sb = a.state_dict(), b.state_dict()
    for opt in ("v_optimizer", "q_optimizer", "actor_optimizer"):
        assert float(sa[opt]["state"][0]["step"]) == float(sb[opt]["state"][0]["step"]), (what, opt)


def _buffer(N, seed, S_=S, A_=A):
    iql = _hip()[0]
    buf = iql.ReplayBuffer(S_, A_, N, "cuda")
    data = synth.synth_transitions(N, S_, A_, seed=seed)
    buf.load_d4rl_dataset({k: v.copy() for k, v in data.items()})
    return buf


@pytest.mark.parametrize("gaussian,B,precision", [(True, 256, "f32"), (False, 256, "f32"), (True, 100, "f32"),
                                                  (False, 100, "f32"), (True, 600, "f32"), (False, 600, "f32"),
                                                  (True, 256, "bf16")])
def test_eager_group_steps_equal_solo_steps_bitwise(gaussian, B, precision):
    iql, _, _, _, to_tb = _hip()
    K = 3
    pairs = [_pair(i, gaussian, precision=precision) for i in range(K)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    group = iql.ImplicitQLearningGroup(members)
    for step in range(3):
        batches = [to_tb(step_batch(S, A, B, seed=1000 * i + step)) for i in range(K)]
        logs = group.train(batches)
        for i in range(K):
            want = twins[i].train(batches[i])
            assert logs[i] == want, (step, i, logs[i], want)
    for i in range(K):
        _assert_same_state(members[i], twins[i], f"member {i}")


@pytest.mark.parametrize("shared", [True, False])
def test_device_drawn_group_steps_equal_solo_train_steps_bitwise(shared):
    iql = _hip()[0]
    K, n, B = 3, 7, 256
    # member 2 follows a cosine schedule over 40 steps: its per-step learning-rate table changes every step
    pairs = [_pair(0, True, max_steps=None), _pair(1, True, max_steps=None), _pair(2, True, max_steps=40)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    bufs = _buffer(5000, 22) if shared else [_buffer(3000, 23), _buffer(4100, 24), _buffer(5000, 25)]
    seeds = [77, 78, 79]
    group = iql.ImplicitQLearningGroup(members)
    for rnd in range(2):
        got = group.train_steps(bufs, n, B, seeds)
        assert got.shape == (K, n, 3) and np.all(np.isfinite(got))
        for i in range(K):
            want = twins[i].train_steps(bufs if shared else bufs[i], n, B, seed=seeds[i])
            assert np.array_equal(got[i], want), (rnd, i)
    for i in range(K):
        _assert_same_state(members[i], twins[i], f"member {i}")


def test_group_member_reproduces_reference_free_run_next_to_other_agents():
    iql, build, _, read_params, to_tb = _hip()
    z, meta = load_golden("g2_freerun_S17A6")
    Sg, Ag, B = meta["S"], meta["A"], meta["B"]
    params = synth.synth_params(Sg, Ag, seed=meta["seed"], gaussian=meta["gaussian"])
    data = synth.synth_transitions(meta["N"], Sg, Ag, seed=2000 + meta["seed"])
    anchor = build(params, Sg, Ag, meta["gaussian"], dict(meta["hyper"]), meta["lrs"], meta["max_steps"])
    others = [_pair(i, meta["gaussian"], S_=Sg, A_=Ag)[0] for i in (1, 2)]
    group = iql.ImplicitQLearningGroup([others[0], anchor, others[1]])
    for k in range(meta["n_steps"]):
        batches = [to_tb(step_batch(Sg, Ag, B, seed=500 + k)), to_tb(batch_from(data, z["indices"][k])),
                   to_tb(step_batch(Sg, Ag, B, seed=600 + k))]
        log = group.train(batches)[1]
        assert_losses([log["value_loss"], log["q_loss"], log["actor_loss"]], z["losses"][k], 1e-5, what=f"step {k}")


def test_member_handed_back_to_solo_training_continues_exactly():
    iql, _, _, _, to_tb = _hip()
    m, twin = _pair(0, True)
    other = _pair(1, True)[0]
    buf = _buffer(5000, 31)
    group = iql.ImplicitQLearningGroup([m, other])
    # the group overwrites the member's staging rows: a solo call right behind it must draw its own
    group.train_steps(buf, 4, 256, [5, 6])
    twin.train_steps(buf, 4, 256, seed=5)
    a = m.train_steps(buf, 6, 256, seed=5)
    b = twin.train_steps(buf, 6, 256, seed=5)
    assert np.array_equal(a, b)
    batches = [to_tb(step_batch(S, A, 256, seed=40 + i)) for i in range(2)]
    la = group.train(batches)[0]
    assert la == twin.train(batches[0])
    a = m.train_steps(buf, 3, 256, seed=9)
    b = twin.train_steps(buf, 3, 256, seed=9)
    assert np.array_equal(a, b)
    _assert_same_state(m, twin)


def test_group_of_one_equals_solo_path():
    """(the Python group of one delegates to the solo calls; the library's own one-member group is checked too)"""
    iql, _, _, _, to_tb = _hip()
    m, twin = _pair(0, True)
    buf = _buffer(5000, 41)
    group = iql.ImplicitQLearningGroup([m])
    b = to_tb(step_batch(S, A, 256, seed=3))
    assert group.train([b])[0] == twin.train(b)
    got = group.train_steps(buf, 5, 256, [11])
    assert np.array_equal(got[0], twin.train_steps(buf, 5, 256, seed=11))
    _assert_same_state(m, twin)
    # the library's group of one (iqlhip_group_* with k = 1), driven the way ImplicitQLearningGroup drives K >= 2
    import ctypes as C
    import iqlhip_binding as hb
    g = C.c_void_p()
    hb.check(hb.lib().iqlhip_group_create((C.c_void_p * 1)(m._ctx.value), 1, C.byref(g)))
    try:
        m._prepare(256)
        tab = np.ascontiguousarray(m._scalar_table(5, 1.0 / 256))
        stream = torch.cuda.current_stream().cuda_stream
        hb.check(hb.lib().iqlhip_group_train_steps(g, (C.c_void_p * 1)(buf._rows.data_ptr()), buf._ld,
                                                   (C.c_int64 * 1)(buf._index_bound()), 256,
                                                   (C.c_void_p * 1)(tab.ctypes.data), 5, (C.c_uint64 * 1)(12),
                                                   (C.c_uint64 * 1)(m.total_it * 128), 0, stream))
        m.total_it += 5
        m._ts_token = None
        out = (C.c_float * 15)()
        hb.check(hb.lib().iqlhip_group_read_losses(g, out, 5, stream))
    finally:
        hb.check(hb.lib().iqlhip_group_destroy(g))
    want = twin.train_steps(buf, 5, 256, seed=12)
    assert np.array_equal(np.frombuffer(out, dtype=np.float32).reshape(5, 3), want)
    _assert_same_state(m, twin)


def test_bad_groups_are_rejected_before_anything_is_launched():
    iql, build, _, read_params, to_tb = _hip()
    a, b = _pair(0, True)[0], _pair(1, True)[0]
    before = read_params(a)
    small = _pair(2, True, S_=11, A_=6)[0]
    with pytest.raises(ValueError):
        iql.ImplicitQLearningGroup([a, small])                    # mismatched dims
    with pytest.raises(ValueError):
        iql.ImplicitQLearningGroup([a, b, a])                     # a duplicate member
    params, hyper, lrs = _spec(3, True)
    cpu = build(params, S, A, True, hyper, lrs, 1000, device="cpu")
    with pytest.raises(RuntimeError):
        iql.ImplicitQLearningGroup([a, cpu])                      # a member on the CPU
    drop = build(params, S, A, True, hyper, lrs, 1000, dropout=0.1)
    with pytest.raises(NotImplementedError):
        iql.ImplicitQLearningGroup([a, drop])                     # actor dropout
    b._dp_world = 2                                               # (what enable_data_parallel sets for world > 1)
    try:
        with pytest.raises(NotImplementedError):
            iql.ImplicitQLearningGroup([a, b])                    # data parallelism
    finally:
        b._dp_world = 1
    group = iql.ImplicitQLearningGroup([a, b])
    drop.actor.eval()                                             # dropout inactive in eval mode: accepted
    iql.ImplicitQLearningGroup([drop])
    for t in (a, b):
        t.set_precision("bf16")
    big = [to_tb(step_batch(S, A, 1024, seed=i)) for i in range(2)]
    with pytest.raises(NotImplementedError):
        group.train(big)                                          # bf16 beyond the small-batch kernels
    with pytest.raises(NotImplementedError):
        group.train_steps(_buffer(5000, 51), 2, 1024, [1, 2])
    with pytest.raises(ValueError):
        group.train([to_tb(step_batch(S, A, 256, seed=1)), to_tb(step_batch(S, A, 128, seed=2))])   # two batch sizes
    torch.cuda.synchronize()
    assert a.total_it == 0 and b.total_it == 0
    after = read_params(a)
    for n in before:
        for k in before[n]:
            assert np.array_equal(before[n][k], after[n][k]), (n, k)


def _first_step_against_oracle(member, i, gaussian, S_, A_, batch, log, precision):
    """Member i's first step (fresh Adam state) against the float64 oracle: its losses, and its gradient read back from
    Adam's first moment (m = (1 - beta1) g after one step) — test_edge_shapes_match_oracle's bounds in fp32,
    tests/test_hip_lb.py's in bf16."""
    from oracle import iql_oracle as O
    from test_hip_lb import LOSS_RTOL, _check_grads
    _, _, read_moments, _, _ = _hip()
    params, hyper, _ = _spec(i, gaussian, S_, A_)
    ref = O.iql_losses_and_grads(params, batch, dict(hyper, deterministic=not gaussian), dtype=np.float64)
    want_l = [ref["value_loss"], ref["q_loss"], ref["actor_loss"]]
    got_l = [log["value_loss"], log["q_loss"], log["actor_loss"]]
    m = read_moments(member)["m"]
    grads = {n: {k: m[n][k].astype(np.float64) / (1.0 - 0.9) for k in m[n]} for n in m}
    if precision == "bf16":
        for got, want in zip(got_l, want_l):
            assert abs(got - want) <= LOSS_RTOL * abs(want), (got_l, want_l)
        _check_grads(grads, ref["grads"])
        return
    assert_losses(got_l, want_l, 1e-5)
    for n, ts in ref["grads"].items():
        for k, want in ts.items():
            gmax = float(np.max(np.abs(want)))
            err = float(np.max(np.abs(grads[n][k].reshape(want.shape) - want)))
            assert err <= 1e-5 * max(1.0, gmax), (n, k, err, gmax)
            if batch["s"].shape[0] <= 2048:
                assert err <= 2e-5 * max(gmax, 1e-30), (n, k, err / max(gmax, 1e-30))


# (K, S, A, gaussian, B, precision, DMA, MULTI): the group kernels each case launches — iql_fwd_group_kernel<BF16, DMA,
# MULTI> with DMA = w0_lds_k > 64 and MULTI = fwd_spb_l2(K x row tiles) > 0 (both checked against helpers' restatements
# of the host rules), iql_bwd_group_kernel<BF16, FULL> with FULL = (B % 256 == 0)
GROUP_EDGE_CASES = [
    (2, 65, 31, True, 70, "f32", True, False),      # kq = 96 does not fit LDS: V / pi W0 (65 wide) by LDS-DMA; bwd ragged
    (3, 52, 28, False, 256, "f32", True, True),     # kq = 80: every W0 by LDS-DMA; bwd full
    (3, 64, 32, False, 256, "f32", False, True),    # w0_lds_k = 64, the register-staged limit; A = 32: two head tiles
    (2, 100, 28, True, 64, "f32", False, False),    # kq = 128, S = 100: every W0 read from global
    (2, 80, 30, True, 100, "f32", False, False),    # kq = 110 > 96 and S = 80 does not fit LDS either: W0 from global
    (3, 40, 17, True, 257, "f32", False, True),     # A = 17 padded to 32; one row past a chunk
    (2, 2, 1, True, 1, "f32", False, False),        # smallest dims, one row
    (2, 17, 6, True, 64, "f32", False, False),      # K >= 2 at fwd_spb_l2 = 0
    (2, 17, 6, False, 16384, "f32", False, True),   # 64 chunks: the loss-partials table is full
    (16, 17, 6, True, 256, "f32", False, True),     # IQLHIP_MAX_GROUP members
    (16, 17, 6, False, 256, "f32", False, True),
    (2, 17, 6, False, 256, "bf16", False, True),    # bwd <bf16, full>; deterministic policy
    (2, 17, 6, True, 64, "bf16", False, False),     # bwd <bf16, ragged>
    (2, 39, 28, True, 512, "bf16", True, True),     # the largest bf16 group batch; kq = 67 by LDS-DMA
    (3, 17, 6, True, 100, "bf16", False, True),     # bwd <bf16, ragged>
    (2, 65, 31, True, 70, "bf16", True, False),
]


@pytest.mark.parametrize("K,S_,A_,gaussian,B,precision,dma,multi", GROUP_EDGE_CASES)
def test_eager_group_steps_at_edge_shapes_equal_solo_steps_and_the_oracle(K, S_, A_, gaussian, B, precision, dma,
                                                                          multi):
    iql, _, _, _, to_tb = _hip()
    assert (w0_lds_k(S_, A_) > 64, fwd_spb_l2(K * ((B + 31) // 32)) > 0) == (dma, multi)
    pairs = [_pair(i, gaussian, precision=precision, S_=S_, A_=A_) for i in range(K)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    group = iql.ImplicitQLearningGroup(members)
    for step in range(2):
        raw = [step_batch(S_, A_, B, seed=1000 * i + 10 * step + S_ + A_) for i in range(K)]
        batches = [to_tb(b) for b in raw]
        logs = group.train(batches)
        for i in range(K):
            want = twins[i].train(batches[i])
            assert logs[i] == want, (step, i, logs[i], want)
        if step == 0:
            _first_step_against_oracle(members[0], 0, gaussian, S_, A_, raw[0], logs[0], precision)
    for i in range(K):
        _assert_same_state(members[i], twins[i], f"member {i}")


@pytest.mark.parametrize("gaussian,precision,S_,A_,B", [
    (False, "f32", 17, 6, 256),     # deterministic policy
    (True, "bf16", 17, 6, 256),     # bf16: fwd <bf16, noDMA, MULTI>, bwd <bf16, full>
    (True, "f32", 65, 31, 70),      # 164-float rows (S = 17, A = 6: 44) through iql_gather_group_kernel; DMA forward
])
def test_device_drawn_group_steps_at_other_shapes_and_precisions(gaussian, precision, S_, A_, B):
    iql = _hip()[0]
    K, n = 3, 5
    pairs = [_pair(i, gaussian, max_steps=None, precision=precision, S_=S_, A_=A_) for i in range(K)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    bufs = [_buffer(3000 + 700 * i, 60 + i, S_, A_) for i in range(K)]
    seeds = [5, 6, 7]
    group = iql.ImplicitQLearningGroup(members)
    got = group.train_steps(bufs, n, B, seeds)
    assert got.shape == (K, n, 3) and np.all(np.isfinite(got))
    for i in range(K):
        assert np.array_equal(got[i], twins[i].train_steps(bufs[i], n, B, seed=seeds[i])), i
        _assert_same_state(members[i], twins[i], f"member {i}")


def test_group_train_steps_split_into_several_library_calls():
    """chunk=16 over 40 steps: three library calls (16 + 16 + 8 steps) across which total_it, the Philox offsets and the
    scalar tables carry on; member 1's cosine schedule (30 steps) ends inside the run."""
    iql = _hip()[0]
    K, n, B = 3, 40, 256
    pairs = [_pair(0, True, max_steps=None), _pair(1, True, max_steps=30), _pair(2, True, max_steps=1000)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    buf = _buffer(5000, 71)
    seeds = [3, 4, 5]
    group = iql.ImplicitQLearningGroup(members)
    got = group.train_steps(buf, n, B, seeds, chunk=16)
    assert got.shape == (K, n, 3)
    for i in range(K):
        assert np.array_equal(got[i], twins[i].train_steps(buf, n, B, seed=seeds[i])), i
        _assert_same_state(members[i], twins[i], f"member {i}")


def test_members_with_different_context_sizes_and_a_growing_batch():
    """Member 0 trained alone on 2 048 rows first (a context for 2 048 rows) next to two fresh members (256); the group's
    batch then grows to 1 024 rows: members 1 and 2 re-attach and the library group is re-created."""
    iql, _, _, _, to_tb = _hip()
    pairs = [_pair(i, True) for i in range(3)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    big = to_tb(step_batch(S, A, 2048, seed=90))
    assert members[0].train(big) == twins[0].train(big)
    group = iql.ImplicitQLearningGroup(members)
    before = None
    for step, B in enumerate((256, 256, 1024, 1024)):
        if step == 2:
            before = group._ctxs
            assert [t._max_batch for t in members] == [2048, 256, 256]
        batches = [to_tb(step_batch(S, A, B, seed=95 + 10 * step + i)) for i in range(3)]
        logs = group.train(batches)
        for i in range(3):
            assert logs[i] == twins[i].train(batches[i]), (step, i)
    assert [t._max_batch for t in members] == [2048, 1024, 1024]
    assert group._ctxs != before
    buf = _buffer(5000, 97)
    got = group.train_steps(buf, 3, 1024, [1, 2, 3])
    for i in range(3):
        assert np.array_equal(got[i], twins[i].train_steps(buf, 3, 1024, seed=i + 1)), i
        _assert_same_state(members[i], twins[i], f"member {i}")


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_group_step_ignores_rows_of_an_earlier_larger_batch(precision):
    """Each member's staging and scratch rows hold a 512-row batch (a solo forward/backward) before the group steps
    over 100 rows: bit for bit the steps of twins that never held 512 rows (same context size).  Then a group step at
    512 rows and one at 100 again."""
    iql, _, _, _, to_tb = _hip()
    K = 3
    pairs = [_pair(i, True, precision=precision) for i in range(K)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    for t in members + twins:
        t._prepare(512)
    for i, t in enumerate(members):
        t.flat_gradient(to_tb(step_batch(S, A, 512, seed=120 + i)))
    group = iql.ImplicitQLearningGroup(members)
    for B in (100, 512, 100):
        batches = [to_tb(step_batch(S, A, B, seed=130 + B + i)) for i in range(K)]
        logs = group.train(batches)
        for i in range(K):
            assert logs[i] == twins[i].train(batches[i]), (B, i)
    for i in range(K):
        _assert_same_state(members[i], twins[i], f"member {i}")
