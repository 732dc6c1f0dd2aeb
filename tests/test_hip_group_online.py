"""GPU tests of the group online step (ImplicitQLearningGroup.online_step / iqlhip_group_online_step): after every
iteration each member is exactly — bit for bit — where a solo twin (same initial parameters, same buffer contents) is
after ImplicitQLearning.online_step with the same arguments: losses, ring rows, pointer and size, parameters, Adam
moments, targets, the next actions and the library's random-stream counters.  Bad calls are refused before anything
moves."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu


def _hip():
    import iql
    from hip_helpers import build_hip_trainer, read_moments, read_params
    return iql, build_hip_trainer, read_moments, read_params


def _pair(i, S, A, gaussian, precision="f32", dropout=0.0):
    _, build, _, _ = _hip()
    params = synth.synth_params(S, A, seed=500 + i, gaussian=gaussian)
    hyper = {"iql_tau": 0.6 + 0.05 * i, "beta": 2.0 + i, "discount": 0.99, "tau": 0.005 * (1 + i % 3)}
    lrs = {"v": 3e-4 * (1 + i % 4), "q": 2e-4 * (1 + i % 4), "pi": 1e-4 * (1 + i % 4)}
    out = []
    for _ in range(2):
        t = build(params, S, A, gaussian, hyper, lrs, 1000, dropout=dropout)
        if precision != "f32":
            t.set_precision(precision)
        out.append(t)
    return out


def _setup(K, S, A, gaussian, cap, precision="f32", dropout=0.0):
    iql = _hip()[0]
    pairs = [_pair(i, S, A, gaussian, precision, dropout) for i in range(K)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    bufs = [iql.ReplayBuffer(S, A, cap, "cuda") for _ in range(K)]
    tbufs = [iql.ReplayBuffer(S, A, cap, "cuda") for _ in range(K)]
    return members, twins, bufs, tbufs


def _streams(K, n, S, A, seed=700):
    return [synth.synth_transitions(n, S, A, seed=seed + k, antmaze_rewards=True) for k in range(K)]


def _tr(st, i):
    return (st["observations"][i], st["actions"][i], float(st["rewards"][i]), st["next_observations"][i],
            bool(st["terminals"][i]))


def _counters(t):
    import iqlhip_binding as hb
    c = (C.c_uint64 * 2)()
    hb.check(hb.lib().iqlhip_get_counters(t._ctx, c))
    return int(c[0]), int(c[1])


def _assert_same(a, b, buf_a, buf_b, what=""):
    _, _, read_moments, read_params = _hip()
    pa, pb = read_params(a), read_params(b)
    for n in pa:                                  # (qt1 / qt2: the targets)
        for k in pa[n]:
            assert np.array_equal(pa[n][k], pb[n][k]), (what, "param", n, k)
    ma, mb = read_moments(a), read_moments(b)
    for which in ("m", "v"):
        for n in ma[which]:
            for k in ma[which][n]:
                assert np.array_equal(ma[which][n][k], mb[which][n][k]), (what, which, n, k)
    assert a.total_it == b.total_it, what
    assert a.actor_optimizer.param_groups[0]["lr"] == b.actor_optimizer.param_groups[0]["lr"], what
    assert {g: int(t) for g, t in a._adam_t.items()} == {g: int(t) for g, t in b._adam_t.items()}, what
    assert _counters(a) == _counters(b), what
    if buf_a is not None:
        assert (buf_a._pointer, buf_a._size, buf_a._writes) == (buf_b._pointer, buf_b._size, buf_b._writes), what
        assert torch.equal(buf_a._rows, buf_b._rows), what


def _run_pair(group, members, twins, bufs, tbufs, streams, iters, B, act_pattern=None, rngs_seeds=None, start=0):
    """`iters` group online steps against the twins' solo steps (member order, or — rngs_seeds — each twin on its own
    seeded global stream, replayed per twin afterwards).  act_pattern(it, k) -> bool: member k asks for an action."""
    K = len(members)
    logs_g, acts_g = [], []
    rngs = None if rngs_seeds is None else [np.random.RandomState(s) for s in rngs_seeds]
    if rngs is None:
        np.random.seed(5)
    for it in range(start, start + iters):
        trs = [_tr(streams[k], it) for k in range(K)]
        args = [list(x) for x in zip(*trs)]
        an = None if act_pattern is None else [trs[k][3] if act_pattern(it, k) else None for k in range(K)]
        res = group.online_step(bufs, *args, B, act_next=an, rngs=rngs)
        if an is None:
            logs_g.append(res)
            acts_g.append([None] * K)
        else:
            logs_g.append(res[0])
            acts_g.append(res[1])
    logs_t = [[None] * K for _ in range(iters)]
    acts_t = [[None] * K for _ in range(iters)]

    def solo(k, j, it):
        s, a, r, ns, d = _tr(streams[k], it)
        want = act_pattern is not None and act_pattern(it, k)
        res = twins[k].online_step(tbufs[k], s, a, r, ns, d, B, act_next=ns if want else None)
        logs_t[j][k], acts_t[j][k] = (res[0], res[1]) if want else (res, None)

    if rngs_seeds is None:
        np.random.seed(5)
        for j, it in enumerate(range(start, start + iters)):
            for k in range(K):
                solo(k, j, it)
    else:
        for k in range(K):
            np.random.seed(rngs_seeds[k])
            for j, it in enumerate(range(start, start + iters)):
                solo(k, j, it)
    for j in range(iters):
        for k in range(K):
            assert logs_g[j][k] == logs_t[j][k], (j, k)
            if acts_t[j][k] is None:
                assert acts_g[j][k] is None, (j, k)
            else:
                assert acts_g[j][k].shape == acts_t[j][k].shape and np.array_equal(acts_g[j][k], acts_t[j][k]), (j, k)
    for k in range(K):
        _assert_same(members[k], twins[k], bufs[k], tbufs[k], f"member {k}")


def test_k4_gaussian_fp32_wrapping_rings_with_device_noise_actions():
    """configs[2]'s dims; 50-row rings wrap twice in 130 iterations; the first draws come from a 1-row buffer, so
    indices equal to the ring pointer occur; every iteration asks for a training-mode action (device noise)."""
    iql = _hip()[0]
    K, S, A, B, cap, n = 4, 29, 8, 256, 50, 130
    members, twins, bufs, tbufs = _setup(K, S, A, True, cap)
    group = iql.ImplicitQLearningGroup(members)
    for t in members + twins:
        t.actor.train()
    streams = _streams(K, n, S, A)
    _run_pair(group, members, twins, bufs, tbufs, streams, n, B, act_pattern=lambda it, k: True)
    assert all((b._pointer, b._size) == (n % cap, cap) for b in bufs)
    assert all(_counters(t)[1] == n for t in members)          # one noise draw per action


def test_k3_deterministic_bf16_b512_with_mixed_act_requests():
    iql = _hip()[0]
    K, S, A, B, cap, n = 3, 17, 6, 512, 40, 24
    members, twins, bufs, tbufs = _setup(K, S, A, False, cap, precision="bf16")
    group = iql.ImplicitQLearningGroup(members)
    streams = _streams(K, n, S, A, seed=800)
    _run_pair(group, members, twins, bufs, tbufs, streams, n, B, act_pattern=lambda it, k: (it + k) % 3 != 0 and it % 5 != 4)
    assert all(_counters(t)[1] == 0 for t in members)          # deterministic policy: no noise stream


def test_per_member_rngs_equal_separately_seeded_runs():
    iql = _hip()[0]
    K, S, A, B, cap, n = 3, 17, 6, 64, 30, 40
    members, twins, bufs, tbufs = _setup(K, S, A, True, cap)
    group = iql.ImplicitQLearningGroup(members)
    for t in members + twins:
        t.actor.train()
    streams = _streams(K, n, S, A, seed=900)
    _run_pair(group, members, twins, bufs, tbufs, streams, n, B, act_pattern=lambda it, k: (it * (k + 1)) % 4 != 1,
              rngs_seeds=[11, 12, 13])


@pytest.mark.parametrize("B", [1, 33])
def test_k16_small_batches(B):
    iql = _hip()[0]
    K, S, A, cap, n = 16, 17, 6, 20, 8
    members, twins, bufs, tbufs = _setup(K, S, A, True, cap)
    group = iql.ImplicitQLearningGroup(members)
    streams = _streams(K, n, S, A, seed=1000 + B)
    _run_pair(group, members, twins, bufs, tbufs, streams, n, B, act_pattern=lambda it, k: (it + k) % 2 == 0)


def test_hand_off_to_solo_and_group_train_steps():
    iql = _hip()[0]
    K, S, A, B, cap, n = 3, 17, 6, 128, 300, 12
    members, twins, bufs, tbufs = _setup(K, S, A, True, cap)
    group = iql.ImplicitQLearningGroup(members)
    streams = _streams(K, n + 2, S, A, seed=1100)
    _run_pair(group, members, twins, bufs, tbufs, streams, n, B)
    # member 0 continues with a solo online step, member 1 with solo train_steps; then all three in a group train_steps
    np.random.seed(21)
    l0 = members[0].online_step(bufs[0], *_tr(streams[0], n), B)
    np.random.seed(21)
    assert l0 == twins[0].online_step(tbufs[0], *_tr(streams[0], n), B)
    assert np.array_equal(members[1].train_steps(bufs[1], 5, B, seed=3), twins[1].train_steps(tbufs[1], 5, B, seed=3))
    lg = group.train_steps(bufs, 4, B, seeds=[7, 8, 9])
    tw = iql.ImplicitQLearningGroup(twins)
    assert np.array_equal(lg, tw.train_steps(tbufs, 4, B, seeds=[7, 8, 9]))
    for k in range(K):
        _assert_same(members[k], twins[k], bufs[k], tbufs[k], f"member {k} after the hand-off")
    # ... and back to group online steps
    _run_pair(group, members, twins, bufs, tbufs, streams, 2, B, act_pattern=lambda it, k: k != 1, start=n)


@pytest.mark.parametrize("with_rngs", [False, True])
def test_group_of_one(with_rngs):
    iql = _hip()[0]
    S, A, B, cap, n = 29, 8, 256, 50, 60
    members, twins, bufs, tbufs = _setup(1, S, A, True, cap)
    group = iql.ImplicitQLearningGroup(members)
    streams = _streams(1, n, S, A, seed=1200)
    _run_pair(group, members, twins, bufs, tbufs, streams, n, B, act_pattern=lambda it, k: it % 2 == 0,
              rngs_seeds=[31] if with_rngs else None)


def _snapshot(members, bufs):
    read_params = _hip()[3]
    return ([(b._pointer, b._size, b._writes, b._rows.clone()) for b in bufs],
            [(t.total_it, dict(t._adam_t), read_params(t)) for t in members])


def _unchanged(before, members, bufs):
    after = _snapshot(members, bufs)
    for (p0, s0, w0, r0), (p1, s1, w1, r1) in zip(before[0], after[0]):
        assert (p0, s0, w0) == (p1, s1, w1) and torch.equal(r0, r1)
    for (i0, a0, q0), (i1, a1, q1) in zip(before[1], after[1]):
        assert i0 == i1 and a0 == a1
        for n in q0:
            for k in q0[n]:
                assert np.array_equal(q0[n][k], q1[n][k]), (n, k)


def test_rejections_leave_everything_unmoved():
    import iqlhip_binding as hb
    iql = _hip()[0]
    K, S, A, B, cap = 3, 17, 6, 64, 30
    members, _, bufs, _ = _setup(K, S, A, True, cap)
    group = iql.ImplicitQLearningGroup(members)
    streams = _streams(K, 3, S, A, seed=1300)
    args = [list(x) for x in zip(*[_tr(streams[k], 0) for k in range(K)])]
    np.random.seed(1)
    group.online_step(bufs, *args, B)            # one good step first: the rings are non-empty
    before = _snapshot(members, bufs)

    def refused(exc, bufs_=bufs, B_=B, **kw):
        with pytest.raises(exc):
            group.online_step(bufs_, *args, B_, **kw)
        _unchanged(before, members, bufs)

    refused(ValueError, bufs_=[bufs[0], bufs[1], bufs[0]])                       # a shared buffer
    alias = iql.ReplayBuffer(S, A, cap, "cuda")
    alias._rows = bufs[1]._rows                                                  # a distinct object on the same rows
    refused(ValueError, bufs_=[bufs[0], bufs[1], alias])
    refused(NotImplementedError, bufs_=[bufs[0], bufs[1], iql.OfflineReplayBuffer(S, A, cap, "cuda")])
    refused(ValueError, bufs_=[bufs[0], bufs[1], iql.ReplayBuffer(S, A, cap, "cpu")])
    refused(ValueError, bufs_=bufs[:2])                                          # K - 1 buffers
    refused(ValueError, act_next=[None, None])
    # the library's own checks (what a direct C caller could pass)
    lib, st = hb.lib(), members[0]._stream()
    g = group._group()
    ld = bufs[0]._ld
    rows = np.zeros((K, ld), dtype=np.float32)
    idx = np.zeros((K, B), dtype=np.int64)
    scs = (hb.StepScalars * K)()
    for k, t in enumerate(members):
        t._fill_scalars(scs[k], {"v": 9, "q": 9, "pi": 9}, t._current_lrs(), 1.0 / B)
    out = (C.c_float * (3 * K))()

    def c_call(rings=None, ld_=ld, caps=None, ptrs=None, idx_=idx, n=B):
        rings = rings or [b._rows.data_ptr() for b in bufs]
        caps = caps or [cap] * K
        ptrs = ptrs or [b._pointer for b in bufs]
        return lib.iqlhip_group_online_step(g, (C.c_void_p * K)(*rings), ld_, (C.c_int64 * K)(*caps),
                                            (C.c_int64 * K)(*ptrs), rows.ctypes.data, idx_.ctypes.data, n, scs, out,
                                            None, None, None, None, None, st)

    bad = idx.copy()
    bad[2, 7] = cap                                                              # outside member 2's ring
    for exc, kw in ((ValueError, dict(rings=[bufs[0]._rows.data_ptr()] * 2 + [bufs[2]._rows.data_ptr()])),
                    (ValueError, dict(ld_=ld + 4)), (ValueError, dict(ptrs=[0, cap, 0])),
                    (ValueError, dict(caps=[cap, 0, cap])), (ValueError, dict(n=0)), (IndexError, dict(idx_=bad))):
        with pytest.raises(exc):
            hb.check(c_call(**kw))
        _unchanged(before, members, bufs)
    assert [_counters(t) for t in members] == [(0, 0)] * K
    # bf16 batches above 512 rows
    b16 = _setup(2, S, A, True, cap, precision="bf16")
    g16 = iql.ImplicitQLearningGroup(b16[0])
    a2 = [x[:2] for x in args]
    with pytest.raises(NotImplementedError):
        g16.online_step(b16[2], *a2, 513)
    assert all(t.total_it == 0 for t in b16[0]) and all(b._size == 0 for b in b16[2])
    # actor dropout (a member switched back to training mode after the group was formed)
    dm, _, dbufs, _ = _setup(2, S, A, True, cap, dropout=0.1)
    for t in dm:
        t.actor.eval()
    gd = iql.ImplicitQLearningGroup(dm)
    dm[1].actor.train()
    with pytest.raises(NotImplementedError):
        gd.online_step(dbufs, *a2, B)
    assert all(t.total_it == 0 for t in dm) and all(b._size == 0 for b in dbufs)
