"""GPU tests of trainer groups (ImplicitQLearningGroup / iqlhip_group_*): every member of a group ends exactly — bit
for bit — where a twin (a trainer built identically that runs the same steps alone) ends, for eager steps on
caller-given batches and for device-drawn steps; a member built from a reference fixture reproduces its free-run
losses while it trains next to two other agents; a member handed back to solo training continues correctly; bad
groups are rejected before anything is launched."""
import numpy as np
import pytest
import torch

import synth
from helpers import assert_losses, batch_from, load_golden, step_batch

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


def _buffer(N, seed):
    iql = _hip()[0]
    buf = iql.ReplayBuffer(S, A, N, "cuda")
    data = synth.synth_transitions(N, S, A, seed=seed)
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
