"""GPU tests of the trainer groups' replay-mix calls (ImplicitQLearningGroup.online_step_replay_mix /
train_steps_replay_mix): every member's batch is mixed from an offline buffer and its online ring, in one
set of launches for the group.  After every call each member is exactly — bit for bit — where a solo twin (same
initial parameters, same buffer contents) is after ImplicitQLearning.online_step_mixed / train_steps_mixed with the
member's arguments: losses, statistics, clip record, parameters, targets, Adam moments, schedule, step counts, actions,
the random-stream counters and the ring.  Bad calls are refused before anything moves."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mixed_ref
import synth

pytestmark = pytest.mark.gpu

DIMS = [(17, 6), (39, 28)]          # packed strides 44 and 108: 11 and 27 float4 per row (27 does not divide 256)
N_OFF_ROWS = 300


def _hip():
    import hip_helpers as H
    import iql
    import iqlhip_binding as hb
    return iql, hb, H


@functools.lru_cache(maxsize=None)
def _params(S, A, i):
    return synth.synth_params(S, A, seed=500 + i)


@functools.lru_cache(maxsize=None)
def _offline(S, A, which=0):
    """Offline buffers: never written by a test.  which = 0 is the one the members share; the others differ in size."""
    iql = _hip()[0]
    n = N_OFF_ROWS + 41 * which
    buf = iql.ReplayBuffer(S, A, n, "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in synth.synth_transitions(n, S, A, seed=22 + which).items()})
    return buf


@functools.lru_cache(maxsize=None)
def _stream(S, A, k, n=24):
    d = synth.synth_transitions(n, S, A, seed=700 + k)
    return [(d["observations"][i], d["actions"][i], float(d["rewards"][i]), d["next_observations"][i],
             bool(d["terminals"][i])) for i in range(n)]


def _build(S, A, i, bf16=False, stats=False, clip=None, dropout=0.0, train_mode=True, act_dropout=False):
    """Member i (or its twin): its own parameters, hyper-parameters and learning rates."""
    hyper = {"iql_tau": 0.6 + 0.05 * (i % 4), "beta": 2.0 + (i % 5), "discount": 0.99, "tau": 0.005 * (1 + i % 3)}
    lrs = {"v": 3e-4 * (1 + i % 4), "q": 2e-4 * (1 + i % 4), "pi": 1e-4 * (1 + i % 4)}
    tr = _hip()[2].build_hip_trainer(_params(S, A, i), S, A, True, hyper, lrs, 1000, dropout=dropout)
    if dropout:
        tr.set_dropout_seed(40 + i)
    if bf16:
        tr.set_precision("bf16")
    tr.set_step_stats(stats)
    tr.set_grad_clip(clip)
    tr.set_act_dropout(act_dropout)
    tr.actor.train(train_mode)
    return tr


def _ring(S, A, k, cap, prefill):
    iql = _hip()[0]
    ring = iql.ReplayBuffer(S, A, cap, "cuda")
    for t in _stream(S, A, k)[12:12 + prefill]:
        ring.add_transition(*t)
    return ring


def _counters(t):
    hb = _hip()[1]
    c = (C.c_uint64 * 2)()
    hb.check(hb.lib().iqlhip_get_counters(t._ctx, c))
    return int(c[0]), int(c[1]), t.act_dropout_calls()


def _assert_same(a, b, ring_a=None, ring_b=None, what=""):
    _hip()[2].assert_same_trainer_state(a, b, what)
    assert _counters(a) == _counters(b), what          # (keep-bit stream, act noise calls, inference keep-bit calls)
    if a._grad_clip is not None:
        assert a.last_grad_clip() == b.last_grad_clip(), what
    if ring_a is not None:
        assert (ring_a._pointer, ring_a._size, ring_a._writes) == (ring_b._pointer, ring_b._size, ring_b._writes), what
        assert torch.equal(ring_a._rows, ring_b._rows), what


def _per(v, K):
    return list(v) if isinstance(v, (list, tuple)) else [v] * K


def _members(K, S, A, member_kw=None, **kw):
    member_kw = member_kw or [{}] * K
    return ([_build(S, A, i, **dict(kw, **member_kw[i])) for i in range(K)],
            [_build(S, A, i, **dict(kw, **member_kw[i])) for i in range(K)])


def _online(K, S, A, B, ratio=0.5, iters=6, cap=64, prefill=0, own_offline=False, global_rng=False, act=None,
            group_kw=None, member_kw=None, **kw):
    """`iters` group calls against the twins' solo online_step_mixed calls.  B / ratio / prefill: one value, or one per
    member.  act(it, k) -> bool: member k asks for an action.  global_rng: rngs=None under one global seed against the
    solo calls interleaved in member order; else member k draws from RandomState(s_k) and its twin runs under
    np.random.seed(s_k)."""
    iql = _hip()[0]
    Bs, ratios, fills = _per(B, K), _per(ratio, K), _per(prefill, K)
    members, twins = _members(K, S, A, member_kw, **kw)
    group = iql.ImplicitQLearningGroup(members, **(group_kw or {}))
    offs = [_offline(S, A, k + 1) for k in range(K)] if own_offline else [_offline(S, A)] * K
    rings = [_ring(S, A, k, cap, fills[k]) for k in range(K)]
    trings = [_ring(S, A, k, cap, fills[k]) for k in range(K)]
    seeds = [90 + k for k in range(K)]
    rngs = None if global_rng else [np.random.RandomState(s) for s in seeds]
    want = lambda it, k: act is not None and act(it, k)
    logs_g, acts_g = [], []
    np.random.seed(5)
    for it in range(iters):
        trs = [_stream(S, A, k)[it] for k in range(K)]
        an = None if act is None else [trs[k][3] if want(it, k) else None for k in range(K)]
        res = group.online_step_replay_mix(offs if own_offline else offs[0], rings, *[list(x) for x in zip(*trs)], B, ratio,
                                           act_next=an, rngs=rngs)
        logs_g.append(res if an is None else res[0])
        acts_g.append([None] * K if an is None else res[1])

    def solo(k, it):
        tr = _stream(S, A, k)[it]
        res = twins[k].online_step_mixed(offs[k], trings[k], *tr, Bs[k], ratios[k], act_next=tr[3] if want(it, k) else None)
        log, a = res if want(it, k) else (res, None)
        assert logs_g[it][k] == log, (it, k, logs_g[it][k], log)
        assert all(np.isfinite(v) for v in log.values())
        if a is None:
            assert acts_g[it][k] is None, (it, k)
        else:
            assert acts_g[it][k].shape == (A,) and np.array_equal(acts_g[it][k], a), (it, k)

    if global_rng:
        np.random.seed(5)
        for it in range(iters):
            for k in range(K):
                solo(k, it)
    else:
        for k in range(K):
            np.random.seed(seeds[k])
            for it in range(iters):
                solo(k, it)
    for k in range(K):
        _assert_same(members[k], twins[k], rings[k], trings[k], f"member {k}")
        assert members[k].total_it == iters
    return group, members, logs_g


# ------------------------------------------------------------------------------------------------ the online call
@pytest.mark.parametrize("S,A", DIMS)
@pytest.mark.parametrize("B", [8, 256])
def test_online_k3_six_iterations_equal_the_solo_twins(S, A, B):
    """B = 8: one block holds rows of both kinds; B = 256: 11 / 27 blocks per member, one of which straddles n_off.
    Every ring is empty before the first call: its new size is 1 and every online index equals `pointer`."""
    _online(3, S, A, B)


def test_online_global_stream_in_member_order():
    _online(3, 39, 28, 8, global_rng=True, prefill=(0, 2, 5))


@pytest.mark.parametrize("ratio", [0.125, 0.875], ids=["n_off=1", "n_off=B-1"])
def test_online_smallest_and_largest_split(ratio):
    _online(2, 39, 28, 8, ratio=ratio, prefill=3)


def test_online_rings_of_capacity_4_wrap():
    _, members, _ = _online(2, 39, 28, 8, ratio=0.4, cap=4, prefill=(2, 3))


@pytest.mark.parametrize("S,A", DIMS)
def test_online_one_offline_buffer_per_member(S, A):
    _online(3, S, A, 8, own_offline=True, prefill=(0, 1, 4))


def test_online_k16():
    _online(16, 17, 6, 8, iters=3, prefill=2)


def test_online_unequal_batch_sizes_and_ratios():
    """The grid is the largest member's: the blocks past the 8- and 64-row members' rows read no index, write nothing."""
    _online(3, 39, 28, (8, 64, 256), ratio=(0.25, 0.5, 0.75), group_kw={"mixed_batch": True}, prefill=(0, 3, 6))


def test_online_per_member_ratios_in_an_equal_size_group():
    _online(2, 39, 28, 64, ratio=(0.25, 0.75), prefill=2)


def test_online_act_next_eval_and_sampling_members_one_passing_none():
    _online(3, 17, 6, 8, ratio=0.4, prefill=3, act=lambda it, k: k != 2 or it % 2 == 0,
            member_kw=[{"train_mode": False}, {"train_mode": True}, {"train_mode": True}])


def test_online_statistics_and_clipping_on_a_subset():
    _, members, logs = _online(3, 39, 28, 256, prefill=5,
                               member_kw=[{"stats": True}, {"clip": 0.05}, {"stats": True, "clip": 0.05}])
    assert [len(log) for log in logs[0]] == [19, 3, 19]
    assert min(members[1].last_grad_clip()[k] for k in ("coef_vf", "coef_qf", "coef_actor")) < 1.0      # the limit did clip


def test_online_actor_dropout_two_rates():
    _, members, _ = _online(3, 39, 28, 8, ratio=0.4, prefill=3, group_kw={"actor_dropout": True},
                            member_kw=[{"dropout": 0.1}, {"dropout": 0.25}, {"dropout": 0.0}])
    assert [_counters(t)[0] for t in members] == [6, 6, 0]


def test_online_act_dropout():
    _, members, _ = _online(2, 17, 6, 8, ratio=0.4, prefill=3, group_kw={"actor_dropout": True}, act=lambda it, k: True,
                            member_kw=[{"dropout": 0.1, "act_dropout": True}, {"dropout": 0.0}])
    assert [t.act_dropout_calls() for t in members] == [6, 0]


def test_online_bf16_256_rows():
    _online(2, 39, 28, 256, bf16=True, prefill=5)


def test_online_k1_is_the_solo_call():
    _online(1, 17, 6, 8, global_rng=True, prefill=2, act=lambda it, k: it % 2 == 0)


# ------------------------------------------------------------------------------------------------ the burst call
def _filled(S, A, n, seed, cap):
    iql = _hip()[0]
    buf = iql.ReplayBuffer(S, A, cap, "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in synth.synth_transitions(n, S, A, seed=seed).items()})
    return buf


@functools.lru_cache(maxsize=None)
def _online_buffers(S, A):
    """Online buffers of different sizes, only read by the burst tests."""
    return tuple(_filled(S, A, n, 30 + k, 64) for k, n in enumerate((37, 5, 64)))


def _burst(K, S, A, B, ratio=0.5, n_steps=5, chunk=2, stats=False, group_kw=None, member_kw=None, **kw):
    iql = _hip()[0]
    Bs, ratios = _per(B, K), _per(ratio, K)
    members, twins = _members(K, S, A, member_kw, **kw)
    group = iql.ImplicitQLearningGroup(members, **(group_kw or {}))
    off, ons = _offline(S, A), list(_online_buffers(S, A)[:K])
    seeds = [5 + k for k in range(K)]
    for call in range(2):      # (the second call starts at total_it = n_steps: another Philox offset per member)
        got = group.train_steps_replay_mix(off, ons, n_steps, B, seeds, ratio, chunk=chunk, return_stats=stats)
        for k in range(K):
            res = twins[k].train_steps_mixed(off, ons[k], n_steps, Bs[k], ratios[k], seed=seeds[k], chunk=chunk,
                                             return_stats=members[k]._step_stats and stats)
            if not stats:
                assert got.shape == (K, n_steps, 3) and np.all(np.isfinite(got[k])) and np.array_equal(got[k], res), (call, k)
            elif members[k]._step_stats:
                assert got.shape == (n_steps, K, 16) and np.array_equal(got[:, k], res[1]), (call, k)
            else:
                assert np.all(np.isnan(got[:, k])), (call, k)
    assert all(t._ts_token is None for t in members)
    # nothing staged was left behind: plain calls follow as if the bursts had not happened
    lg = group.train_steps(off, 3, B, seeds)
    for k in range(K):
        assert np.array_equal(lg[k], twins[k].train_steps(off, 3, Bs[k], seed=seeds[k])), k
        _assert_same(members[k], twins[k], what=f"member {k}")
        assert members[k].total_it == 2 * n_steps + 3
    return members


@pytest.mark.parametrize("S,A", DIMS)
@pytest.mark.parametrize("B", [8, 256])
def test_burst_k3_equals_the_solo_twins(S, A, B):
    """5 steps in chunks of 2: chunk boundaries are crossed; the members' online buffers hold 37, 5 and 64 rows."""
    _burst(3, S, A, B)


def test_burst_unequal_batch_sizes_and_ratios():
    _burst(3, 39, 28, (8, 64, 256), ratio=(0.25, 0.5, 0.75), group_kw={"mixed_batch": True})


def test_burst_per_member_ratios_statistics_and_clipping():
    _burst(3, 39, 28, 64, ratio=(0.25, 0.75, 0.5), stats=True, member_kw=[{"stats": True}, {"clip": 0.05}, {"stats": True, "clip": 0.05}])
    _burst(2, 17, 6, 8, member_kw=[{"clip": 0.05}, {"stats": True}])


def test_burst_actor_dropout_two_rates():
    members = _burst(3, 39, 28, 8, ratio=0.4, group_kw={"actor_dropout": True},
                     member_kw=[{"dropout": 0.1}, {"dropout": 0.25}, {"dropout": 0.0}])
    assert [_counters(t)[0] for t in members] == [13, 13, 0]


def test_burst_bf16_256_rows():
    _burst(2, 39, 28, 256, bf16=True)


def test_burst_k1_is_the_solo_call():
    _burst(1, 17, 6, 8, stats=True, member_kw=[{"stats": True}])


def test_burst_equals_eager_steps_on_the_cpu_reference_indices():
    """Member 1 of a group burst against eager train() steps on rows gathered on the host by the indices of
    tests/mixed_ref.py (the CPU Philox reference)."""
    iql, hb, H = _hip()
    S, A, B, n_off, n_steps = 17, 6, 8, 3, 5
    members = [_build(S, A, i) for i in range(2)]
    e = _build(S, A, 1)
    group = iql.ImplicitQLearningGroup(members)
    off, ons = _offline(S, A), list(_online_buffers(S, A)[:2])
    got = group.train_steps_replay_mix(off, ons, n_steps, B, [5, 6], 0.4, chunk=2)
    idx_off, idx_on = mixed_ref.mixed_indices(n_steps, B, n_off, off._size, ons[1]._size, 6, mixed_ref.call_offset(0, B))
    rows_off, rows_on = off._rows.cpu(), ons[1]._rows.cpu()
    for s in range(n_steps):
        block = torch.cat([rows_off[torch.from_numpy(idx_off[s])], rows_on[torch.from_numpy(idx_on[s])]]).cuda()
        log = e.train([block[:, :S], block[:, S: S + A], block[:, 2 * S + A: 2 * S + A + 1], block[:, S + A: 2 * S + A],
                       block[:, 2 * S + A + 1: 2 * S + A + 2]])
        assert [log["value_loss"], log["q_loss"], log["actor_loss"]] == got[1, s].tolist(), s
    H.assert_same_trainer_state(members[1], e, "burst vs eager on the reference indices")


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_move_nothing():
    iql, hb, H = _hip()
    S, A, B, K = 17, 6, 8, 2
    off = _offline(S, A)
    members = [_build(S, A, i) for i in range(K)]
    group = iql.ImplicitQLearningGroup(members)
    rings = [_ring(S, A, k, 16, 4) for k in range(K)]
    trs = [_stream(S, A, k)[0] for k in range(K)]
    tr = [list(x) for x in zip(*trs)]
    np.random.seed(9)

    def state(ms=members, rs=rings):
        return ([(t.total_it, dict(t._adam_t), t.actor_optimizer.param_groups[0]["lr"]) for t in ms],
                [(r._pointer, r._size, r._writes) for r in rs], [r._rows.clone() for r in rs], [H.arenas(t) for t in ms],
                np.random.get_state()[1].copy(), np.random.get_state()[2])

    def same(a, b):
        return a[0] == b[0] and a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[2], b[2])) and \
            all(np.array_equal(x, y) for x, y in zip(a[3], b[3])) and np.array_equal(a[4], b[4]) and a[5] == b[5]

    def refused(exc, match=None, g=group, ms=members, off_=off, rings_=rings, B_=B, ratio=0.5, online=True, burst=True, **kw):
        before = state(ms, rings)
        if online:
            with pytest.raises(exc, match=match):
                g.online_step_replay_mix(off_, rings_, *tr, B_, ratio, **kw)
        if burst and not kw:
            with pytest.raises(exc, match=match):
                g.train_steps_replay_mix(off_, rings_, 3, B_, [1, 2], ratio)
        torch.cuda.synchronize()
        assert same(before, state(ms, rings))

    refused(ValueError, "n_off", ratio=0.0)
    refused(ValueError, "n_off", ratio=[0.5, 1.0])
    refused(ValueError, "state_dim", rings_=[rings[0], iql.ReplayBuffer(S + 1, A, 16, "cuda")])
    refused(ValueError, "GPU", rings_=[rings[0], iql.ReplayBuffer(S, A, 16, "cpu")])
    refused(ValueError, "GPU", off_=iql.ReplayBuffer(S, A, 16, "cpu"))
    refused(ValueError, "distinct", off_=[off, rings[1]])
    refused(ValueError, "empty", off_=iql.ReplayBuffer(S, A, 16, "cuda"))
    refused(ValueError, "empty", rings_=[rings[0], iql.ReplayBuffer(S, A, 16, "cuda")], online=False)
    refused(ValueError, "finetune", off_=iql.OfflineReplayBuffer(S, A, 16, "cuda"))
    refused(ValueError, "finetune", rings_=[rings[0], iql.OfflineReplayBuffer(S, A, 16, "cuda")])
    refused(ValueError, "shares an online", rings_=[rings[0], rings[0]])
    refused(ValueError, "offline buffer", off_=[rings[1], off])
    refused(ValueError, "list of 2", rings_=rings[:1])
    refused(ValueError, "mixing ratios", ratio=[0.5, 0.5, 0.5])
    refused(ValueError, "mixed_batch", B_=[8, 16])
    refused(ValueError, "rngs", burst=False, rngs=[np.random.RandomState(0)])
    wide = iql.ReplayBuffer(S, A, 16, "cuda")
    wide._size, wide._ld = 4, wide._ld + 4
    refused(ValueError, "row strides", rings_=[rings[0], wide])
    # data-parallel members (the setting alone: no process group is needed to be refused)
    members[1]._dp_exchange = "p2p"
    refused(NotImplementedError, "data parallelism")
    members[1]._dp_exchange = None
    # bf16 beyond 512 rows
    bf = [_build(S, A, i, bf16=True) for i in range(K)]
    refused(NotImplementedError, "512", g=iql.ImplicitQLearningGroup(bf), ms=bf, B_=600)
    # training-mode dropout members in a group built without actor_dropout=True
    dr = [_build(S, A, i, dropout=0.1) for i in range(K)]
    for t in dr:
        t.actor.eval()
    plain = iql.ImplicitQLearningGroup(dr)
    for t in dr:
        t.actor.train()
    refused(NotImplementedError, "actor_dropout=True", g=plain, ms=dr)
    # act_next for a training-mode dropout member that has not called set_act_dropout(True); pending injected masks
    gd = iql.ImplicitQLearningGroup(dr, actor_dropout=True)
    refused(NotImplementedError, "set_act_dropout", g=gd, ms=dr, burst=False, act_next=[trs[0][3], None])
    dr[1].inject_dropout_masks(np.ones((8, 256), dtype=bool), np.ones((8, 256), dtype=bool))
    refused(NotImplementedError, "inject_dropout_masks", g=gd, ms=dr, online=False)
    # the library's own checks, as a direct caller of the C ABI meets them
    lib = hb.lib()
    for t in members:
        t._prepare(B)
    scs, _ = group._next_scalars([1.0 / B] * K)
    out = (C.c_float * (3 * K))()
    rows = np.zeros((K, rings[0]._ld), dtype=np.float32)
    ring_ptrs = (C.c_void_p * K)(*[r._rows.data_ptr() for r in rings])
    off_ptrs = (C.c_void_p * K)(off._rows.data_ptr(), off._rows.data_ptr())
    caps, ptrs = (C.c_int64 * K)(16, 16), (C.c_int64 * K)(*[r._pointer for r in rings])

    def online(idx, n_off=(4, 4), offs=off_ptrs, size_off=(N_OFF_ROWS, N_OFF_ROWS), n=(B, B)):
        idx = np.array(idx, dtype=np.int64)
        before = state()
        rc = lib.iqlhip_group_online_step_replay2(group._group(), ring_ptrs, rings[0]._ld, caps, ptrs, rows.ctypes.data,
                                                  idx.ctypes.data, (C.c_int32 * K)(*n), scs, out, None, None, None, None,
                                                  None, members[0]._stream(), offs, (C.c_int64 * K)(*size_off),
                                                  (C.c_int32 * K)(*n_off))
        torch.cuda.synchronize()
        assert same(before, state())
        return rc

    good = [0, 1, 2, 3, 0, 1, 2, 3]
    assert online(good + [0, 1, 2, N_OFF_ROWS] + good[4:]) == hb.E_INDEX          # member 1: offline index past its size
    assert online(good + [0, 1, 2, -1] + good[4:]) == hb.E_INDEX
    assert online(good[:4] + [0, 1, 2, 16] + good) == hb.E_INDEX                  # member 0: online index past the ring
    assert online([0, 1, 2, 16] + good[4:] + good, size_off=(16, N_OFF_ROWS)) == hb.E_INDEX
    assert online(good + good, n_off=(4, 0)) == hb.E_INVAL
    assert online(good + good, n_off=(B, 4)) == hb.E_INVAL
    assert online(good + good, size_off=(N_OFF_ROWS, 0)) == hb.E_INVAL
    assert online(good + good, offs=(C.c_void_p * K)(off._rows.data_ptr(), None)) == hb.E_INVAL
    assert online(good + good, offs=(C.c_void_p * K)(off._rows.data_ptr(), rings[0]._rows.data_ptr())) == hb.E_INVAL
    with pytest.raises(ValueError, match="overlaps"):
        hb.check(hb.E_INVAL)
    tabs = [np.ascontiguousarray(np.zeros((3, 12), dtype=np.float32)) for _ in range(K)]
    on_ptrs = ring_ptrs

    def burst(n_off=(4, 4), ons=on_ptrs, size_on=(4, 4), Bs=(B, B)):
        before = state()
        rc = lib.iqlhip_group_train_steps_replay2(group._group(), off_ptrs, (C.c_int64 * K)(N_OFF_ROWS, N_OFF_ROWS), ons,
                                                  (C.c_int64 * K)(*size_on), rings[0]._ld, (C.c_int32 * K)(*Bs),
                                                  (C.c_int32 * K)(*n_off), (C.c_void_p * K)(*[t.ctypes.data for t in tabs]), 3,
                                                  (C.c_uint64 * K)(1, 2), (C.c_uint64 * K)(0, 0), members[0]._stream())
        torch.cuda.synchronize()
        assert same(before, state())
        return rc

    assert burst(n_off=(0, 4)) == hb.E_INVAL
    assert burst(n_off=(4, B)) == hb.E_INVAL
    assert burst(size_on=(4, 0)) == hb.E_INVAL
    assert burst(ons=(C.c_void_p * K)(rings[0]._rows.data_ptr(), off._rows.data_ptr())) == hb.E_INVAL
    assert burst(Bs=(B, 0)) == hb.E_INVAL
    gb = iql.ImplicitQLearningGroup(bf)
    for t in bf:
        t._prepare(1024)
    rc = lib.iqlhip_group_train_steps_replay2(gb._group(), off_ptrs, (C.c_int64 * K)(N_OFF_ROWS, N_OFF_ROWS), on_ptrs,
                                              (C.c_int64 * K)(4, 4), rings[0]._ld, (C.c_int32 * K)(64, 600),
                                              (C.c_int32 * K)(4, 4), (C.c_void_p * K)(*[t.ctypes.data for t in tabs]), 3,
                                              (C.c_uint64 * K)(1, 2), (C.c_uint64 * K)(0, 0), bf[0]._stream())
    assert rc == hb.E_UNSUPPORTED
    # the group still steps afterwards
    logs = group.online_step_replay_mix(off, rings, *tr, B, 0.5)
    assert all(np.isfinite(log["value_loss"]) for log in logs) and [r._size for r in rings] == [5, 5]
    assert np.all(np.isfinite(group.train_steps_replay_mix(off, rings, 3, B, [1, 2], 0.5)))
