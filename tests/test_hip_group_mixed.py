"""GPU tests of trainer groups whose members train at different batch sizes (ImplicitQLearningGroup(...,
mixed_batch=True) / iqlhip_group_*_mixed): every member ends exactly — bit for bit — where a twin (a trainer built
identically that runs the same steps alone at the member's own batch size) ends: losses, parameters and targets, both
Adam moments, total_it, learning rates, optimiser step counts and, with actor dropout, the keep-bit stream positions.
Equal sizes through the mixed path give the bits of the uniform path; bad calls are refused before anything moves."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import step_batch
from test_hip_group import _assert_same_state, _buffer, _pair

pytestmark = pytest.mark.gpu

S, A = 17, 6
DOOR = (39, 28)      # door-*-v1's dims: the reference's actor-dropout configurations


def _hip():
    import iql
    import iqlhip_binding as hb
    from hip_helpers import read_moments, read_params, to_torch_batch
    return iql, hb, read_moments, read_params, to_torch_batch


def _twins(K, gaussian=True, precision="f32", max_steps=1000):
    ms = max_steps if isinstance(max_steps, (list, tuple)) else [max_steps] * K
    pairs = [_pair(i, gaussian, max_steps=ms[i], precision=precision) for i in range(K)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _eager(sizes, gaussian, precision, steps=3):
    iql, _, _, _, to_tb = _hip()
    K = len(sizes)
    members, twins = _twins(K, gaussian, precision)
    group = iql.ImplicitQLearningGroup(members, mixed_batch=True)
    for step in range(steps):
        batches = [to_tb(step_batch(S, A, B, seed=1000 * i + step)) for i, B in enumerate(sizes)]
        logs = group.train(batches)
        for i in range(K):
            want = twins[i].train(batches[i])
            assert logs[i] == want, (step, i, sizes[i], logs[i], want)
    for i in range(K):
        _assert_same_state(members[i], twins[i], f"member {i} ({sizes[i]} rows)")


# ------------------------------------------------------------------------------------------------------ eager train
# (33: a partial second row tile; 256: a FULL member inside a non-FULL backward launch; 100: a ragged single chunk;
#  600: three chunks)
@pytest.mark.parametrize("gaussian", [True, False])
def test_eager_mixed_sizes_equal_solo_steps_bitwise(gaussian):
    _eager((33, 256, 100, 600), gaussian, "f32")


# (the forward's slices per block follow the sum of the members' row tiles: at most 8 tiles run the one-slice block
#  map, up to 16 the two-slice map, more the four-slice map — sizes for each, so that each map's "row tile outside the
#  batch" exit is reached by a member smaller than the largest)
@pytest.mark.parametrize("sizes", [(1, 32, 256),      # one row; exactly one row tile; one full chunk (two-slice map)
                                   (256, 512),        # every member FULL, two chunk counts
                                   (33, 100),         # 2 + 4 row tiles: the one-slice map
                                   (1, 40, 64)])      # 1 + 2 + 2 row tiles: the one-slice map, a one-row member
def test_eager_mixed_sizes_at_tile_and_chunk_edges(sizes):
    _eager(sizes, True, "f32")


def test_eager_mixed_sizes_bf16():
    _eager((32, 100, 256, 512), True, "bf16")


# ------------------------------------------------------------------------------------------- device-drawn train_steps
@pytest.mark.parametrize("shared", [True, False])
def test_device_drawn_mixed_sizes_equal_solo_train_steps_bitwise(shared):
    iql = _hip()[0]
    K, n, sizes = 3, 7, (64, 256, 100)
    # member 2 follows a cosine schedule over 40 steps: its per-step learning-rate table changes every step
    members, twins = _twins(K, max_steps=[None, None, 40])
    bufs = _buffer(5000, 22) if shared else [_buffer(3000, 23), _buffer(4100, 24), _buffer(5000, 25)]
    seeds = [77, 78, 79]
    group = iql.ImplicitQLearningGroup(members, mixed_batch=True)
    for rnd in range(2):
        got = group.train_steps(bufs, n, list(sizes), seeds)
        assert got.shape == (K, n, 3) and np.all(np.isfinite(got))
        for i in range(K):
            want = twins[i].train_steps(bufs if shared else bufs[i], n, sizes[i], seed=seeds[i])
            assert np.array_equal(got[i], want), (rnd, i)
    for i in range(K):
        _assert_same_state(members[i], twins[i], f"member {i}")
    # a member handed back to solo training continues exactly (the group overwrote its staging rows)
    for i in range(K):
        buf = bufs if shared else bufs[i]
        a = members[i].train_steps(buf, 4, sizes[i], seed=seeds[i])
        b = twins[i].train_steps(buf, 4, sizes[i], seed=seeds[i])
        assert np.array_equal(a, b), i
        _assert_same_state(members[i], twins[i], f"member {i} back to solo")


def test_device_drawn_mixed_sizes_in_a_one_slice_forward_grid():
    """Sizes whose row tiles sum to 5: the forward runs its one-slice block map, in which the small members' surplus
    blocks must leave before they touch a row tile outside their batch."""
    iql = _hip()[0]
    K, n, sizes = 3, 5, (1, 40, 64)
    members, twins = _twins(K, max_steps=None)
    buf = _buffer(3000, 41)
    seeds = [11, 12, 13]
    got = iql.ImplicitQLearningGroup(members, mixed_batch=True).train_steps(buf, n, list(sizes), seeds)
    for i in range(K):
        assert np.array_equal(got[i], twins[i].train_steps(buf, n, sizes[i], seed=seeds[i])), i
        _assert_same_state(members[i], twins[i], f"member {i}")


# ------------------------------------------------------------------------------------------------------ actor dropout
def test_mixed_sizes_with_actor_dropout_equal_solo_twins():
    from test_hip_group_dropout import _assert_same_state as same_with_counters
    from test_hip_group_dropout import _counters, _keep_bits
    from test_hip_group_dropout import _pair as drop_pair
    iql, _, _, _, to_tb = _hip()
    Sd, Ad = DOOR
    rates, sizes = (0.1, 0.0, 0.1), (100, 256, 40)
    pairs = [drop_pair(i, True, rates[i], S_=Sd, A_=Ad, max_steps=None, seed=100 + i) for i in range(3)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    group = iql.ImplicitQLearningGroup(members, actor_dropout=True, mixed_batch=True)
    for step in range(3):
        batches = [to_tb(step_batch(Sd, Ad, B, seed=1000 * i + step)) for i, B in enumerate(sizes)]
        logs = group.train(batches)
        for i in range(3):
            assert logs[i] == twins[i].train(batches[i]), (step, i)
            if rates[i] > 0:
                assert np.array_equal(_keep_bits(members[i], sizes[i]), _keep_bits(twins[i], sizes[i])), (step, i)
    for i in range(3):
        same_with_counters(members[i], twins[i], f"member {i} after train")
    assert [_counters(t)[0] for t in members] == [3, 0, 3]
    bufs = [_buffer(3000 + 500 * i, 60 + i, Sd, Ad) for i in range(3)]
    seeds = [5, 6, 7]
    got = group.train_steps(bufs, 5, list(sizes), seeds)
    for i in range(3):
        assert np.array_equal(got[i], twins[i].train_steps(bufs[i], 5, sizes[i], seed=seeds[i])), i
        same_with_counters(members[i], twins[i], f"member {i} after train_steps")
        if rates[i] > 0:
            assert np.array_equal(_keep_bits(members[i], sizes[i]), _keep_bits(twins[i], sizes[i])), i


# -------------------------------------------------------------------------------------------------------- online_step
def test_online_step_mixed_sizes_equal_solo_online_steps():
    from test_hip_group_online import _assert_same, _setup, _streams, _tr
    iql = _hip()[0]
    K, sizes, cap, iters = 3, (64, 256, 100), 50, 3
    members, twins, bufs, tbufs = _setup(K, S, A, True, cap)
    for t in members + twins:
        t.actor.train()                               # (device noise in the actions)
    group = iql.ImplicitQLearningGroup(members, mixed_batch=True)
    streams = _streams(K, iters, S, A)
    asks = (True, False, True)
    np.random.seed(5)
    got = []
    for it in range(iters):
        trs = [_tr(streams[k], it) for k in range(K)]
        args = [list(x) for x in zip(*trs)]
        an = [trs[k][3] if asks[k] else None for k in range(K)]
        got.append(group.online_step(bufs, *args, list(sizes), act_next=an))
    np.random.seed(5)
    for it in range(iters):
        logs, acts = got[it]
        for k in range(K):
            s, a, r, ns, d = _tr(streams[k], it)
            res = twins[k].online_step(tbufs[k], s, a, r, ns, d, sizes[k], act_next=ns if asks[k] else None)
            if asks[k]:
                assert logs[k] == res[0], (it, k)
                assert acts[k].shape == res[1].shape and np.array_equal(acts[k], res[1]), (it, k)
            else:
                assert logs[k] == res and acts[k] is None, (it, k)
    for k in range(K):
        _assert_same(members[k], twins[k], bufs[k], tbufs[k], f"member {k}")
        assert (bufs[k]._pointer, bufs[k]._size) == (iters, iters)


# -------------------------------------------------------------------------------- equal sizes through the mixed path
def test_equal_sizes_through_the_mixed_path_give_the_uniform_path_bits():
    from test_hip_group_online import _streams, _tr
    iql, hb, _, _, to_tb = _hip()
    K, B, n = 3, 256, 4
    uni = [_pair(i, True, max_steps=None)[0] for i in range(K)]
    mix = [_pair(i, True, max_steps=None)[0] for i in range(K)]
    raw = [_pair(i, True, max_steps=None)[0] for i in range(K)]
    g_uni = iql.ImplicitQLearningGroup(uni)
    g_mix = iql.ImplicitQLearningGroup(mix, mixed_batch=True)
    buf = _buffer(5000, 33)
    seeds = [3, 4, 5]
    for step in range(2):
        batches = [to_tb(step_batch(S, A, B, seed=70 * i + step)) for i in range(K)]
        assert g_uni.train(batches) == g_mix.train(batches), step
    assert np.array_equal(g_uni.train_steps(buf, n, B, seeds), g_mix.train_steps(buf, n, [B] * K, seeds))
    # the online step (separate rings with the same contents)
    rings = [[iql.ReplayBuffer(S, A, 40, "cuda") for _ in range(K)] for _ in range(2)]
    streams = _streams(K, 2, S, A)
    for it in range(2):
        args = [list(x) for x in zip(*[_tr(streams[k], it) for k in range(K)])]
        res = []
        for g, rg in ((g_uni, rings[0]), (g_mix, rings[1])):
            res.append(g.online_step(rg, *args, B, rngs=[np.random.RandomState(90 + k) for k in range(K)]))
        assert res[0] == res[1], it
    for i in range(K):
        _assert_same_state(uni[i], mix[i], f"member {i}")
        assert torch.equal(rings[0][i]._rows, rings[1][i]._rows)
    # the raw eager entry points at equal rows: iqlhip_group_step_mixed against iqlhip_group_step
    pair = [[_pair(i, True, max_steps=None)[0] for i in range(K)] for _ in range(2)]
    batches = [to_tb(step_batch(S, A, B, seed=500 + i)) for i in range(K)]
    outs = []
    for trs, name in zip(pair, ("iqlhip_group_step", "iqlhip_group_step_mixed")):
        grp = iql.ImplicitQLearningGroup(trs)
        for t in trs:
            t._prepare(B)
        structs, keep = (hb.Batch * K)(), []
        for i, t in enumerate(trs):
            structs[i], kp, _ = t._batch_struct(batches[i])
            keep.append(kp)
        scs, adam_next = grp._next_scalars([1.0 / B] * K)
        out = (C.c_float * (3 * K))()
        hb.check(getattr(hb.lib(), name)(grp._group(), structs, scs, out, trs[0]._stream()))
        grp._commit_step(adam_next, out)
        outs.append(list(out))
    assert outs[0] == outs[1]
    for i in range(K):
        _assert_same_state(pair[0][i], pair[1][i], f"raw step, member {i}")
    # the raw entry point, driven as ImplicitQLearningGroup drives it, against g_uni's first train_steps call
    fresh = [_pair(i, True, max_steps=None)[0] for i in range(K)]
    want = iql.ImplicitQLearningGroup(fresh).train_steps(buf, n, B, seeds)
    g = C.c_void_p()
    hb.check(hb.lib().iqlhip_group_create((C.c_void_p * K)(*[t._ctx.value for t in raw]), K, C.byref(g)))
    try:
        for t in raw:
            t._prepare(B)
        tabs = [np.ascontiguousarray(t._scalar_table(n, 1.0 / B)) for t in raw]
        stream = torch.cuda.current_stream().cuda_stream
        hb.check(hb.lib().iqlhip_group_train_steps_mixed(
            g, (C.c_void_p * K)(*[buf._rows.data_ptr()] * K), buf._ld, (C.c_int64 * K)(*[buf._index_bound()] * K),
            (C.c_int32 * K)(*[B] * K), (C.c_void_p * K)(*[tb.ctypes.data for tb in tabs]), n,
            (C.c_uint64 * K)(*seeds), (C.c_uint64 * K)(*[0] * K), 0, stream))
        out = (C.c_float * (K * n * 3))()
        hb.check(hb.lib().iqlhip_group_read_losses(g, out, n, stream))
    finally:
        hb.check(hb.lib().iqlhip_group_destroy(g))
    assert np.array_equal(np.frombuffer(out, dtype=np.float32).reshape(K, n, 3), want)


# ---------------------------------------------------------------------------------------------------------- refusals
def _snapshot(trainers, bufs=()):
    from test_hip_group_online import _counters
    _, _, read_moments, read_params, _ = _hip()
    torch.cuda.synchronize()
    snap = []
    for t in trainers:
        p, m = read_params(t), read_moments(t)
        arrays = [p[n][k].copy() for n in sorted(p) for k in sorted(p[n])]
        arrays += [m[w][n][k].copy() for w in ("m", "v") for n in sorted(m[w]) for k in sorted(m[w][n])]
        snap.append((arrays, t.total_it, dict(t._adam_t), _counters(t)))
    return snap, [(b._pointer, b._size, b._writes, b._rows.clone()) for b in bufs]


def _assert_unchanged(before, trainers, bufs=()):
    after = _snapshot(trainers, bufs)
    for i, ((a0, it0, ad0, c0), (a1, it1, ad1, c1)) in enumerate(zip(before[0], after[0])):
        assert (it0, ad0, c0) == (it1, ad1, c1), i
        assert len(a0) == len(a1) and all(np.array_equal(x, y) for x, y in zip(a0, a1)), i
    for (p0, s0, w0, r0), (p1, s1, w1, r1) in zip(before[1], after[1]):
        assert (p0, s0, w0) == (p1, s1, w1) and torch.equal(r0, r1)


def test_bad_mixed_calls_are_refused_before_anything_moves():
    from test_hip_group_online import _streams, _tr
    iql, hb, _, _, to_tb = _hip()
    lib = hb.lib()
    a, b = _pair(0, True)[0], _pair(1, True)[0]
    plain = iql.ImplicitQLearningGroup([a, b])
    mixed = iql.ImplicitQLearningGroup([a, b], mixed_batch=True)
    buf = _buffer(3000, 51)
    rings = [iql.ReplayBuffer(S, A, 40, "cuda") for _ in range(2)]
    tr = [list(x) for x in zip(*[_tr(st, 0) for st in _streams(2, 1, S, A)])]
    mixed.online_step(rings, *tr, [8, 16])            # (a first transition in each ring)
    for t in (a, b):
        t._prepare(64)
    # (tables for the raw calls below, built first: _scalar_table advances the host's Adam step counts)
    tabs = [np.ascontiguousarray(t._scalar_table(2, 1.0 / 64)) for t in (a, b)]
    before = _snapshot([a, b], rings)
    # unequal sizes on a group without mixed_batch
    with pytest.raises(ValueError):
        plain.train_steps(buf, 2, [64, 128], [1, 2])
    with pytest.raises(ValueError):
        plain.online_step(rings, *tr, [64, 128])
    # a size list of the wrong length
    with pytest.raises(ValueError):
        mixed.train_steps(buf, 2, [64, 128, 256], [1, 2])
    with pytest.raises(ValueError):
        mixed.online_step(rings, *tr, [64])
    # C level: a NULL size array, reported with the other NULL checks
    g = mixed._group()
    K = 2
    stream = torch.cuda.current_stream().cuda_stream
    ts_args = lambda B: (g, (C.c_void_p * K)(*[buf._rows.data_ptr()] * K), buf._ld,      # noqa: E731
                         (C.c_int64 * K)(*[buf._index_bound()] * K), B,
                         (C.c_void_p * K)(*[tb.ctypes.data for tb in tabs]), 2, (C.c_uint64 * K)(1, 2),
                         (C.c_uint64 * K)(0, 0), 0, stream)
    assert lib.iqlhip_group_train_steps_mixed(*ts_args(None)) == hb.E_INVAL
    assert "NULL" in hb.last_error()
    scs = (hb.StepScalars * K)()
    out = (C.c_float * (3 * K))()
    row = np.zeros((K, rings[0]._ld), dtype=np.float32)
    idx = np.zeros(2 * 64, dtype=np.int64)
    on_args = lambda n: (g, (C.c_void_p * K)(*[r._rows.data_ptr() for r in rings]), rings[0]._ld,      # noqa: E731
                         (C.c_int64 * K)(40, 40), (C.c_int64 * K)(1, 1), row.ctypes.data, idx.ctypes.data, n, scs, out,
                         None, None, None, None, None, stream)
    assert lib.iqlhip_group_online_step_mixed(*on_args(None)) == hb.E_INVAL
    assert "NULL" in hb.last_error()
    # C level: rows_k above that member's max_batch (member 1), and 0 rows
    mb = b._max_batch
    for sizes in ((64, mb + 1), (0, 64)):
        assert lib.iqlhip_group_train_steps_mixed(*ts_args((C.c_int32 * K)(*sizes))) == hb.E_INVAL, sizes
        assert lib.iqlhip_group_online_step_mixed(*on_args((C.c_int32 * K)(*sizes))) == hb.E_INVAL, sizes
    structs, keep = (hb.Batch * K)(), []
    for i, (t, rows) in enumerate(((a, 64), (b, mb + 1))):
        st, kp, _ = t._batch_struct(to_tb(step_batch(S, A, rows, seed=i)))
        structs[i] = st
        keep.append(kp)
    assert lib.iqlhip_group_step_mixed(g, structs, scs, out, stream) == hb.E_INVAL
    assert "member 1" in hb.last_error()
    # an index outside member 1's ring
    idx[64] = 40
    assert lib.iqlhip_group_online_step_mixed(*on_args((C.c_int32 * K)(64, 64))) == hb.E_INDEX
    _assert_unchanged(before, [a, b], rings)
    # a bf16 member above 512 rows next to a small one
    for t in (a, b):
        t.set_precision("bf16")
        t._prepare(1024)                              # (contexts for 1 024 rows: only the bf16 limit refuses below)
    g = mixed._group()
    before = _snapshot([a, b], rings)
    with pytest.raises(NotImplementedError):
        mixed.train([to_tb(step_batch(S, A, 64, seed=1)), to_tb(step_batch(S, A, 600, seed=2))])
    with pytest.raises(NotImplementedError):
        mixed.train_steps(buf, 2, [1024, 64], [1, 2])
    with pytest.raises(NotImplementedError):
        mixed.online_step(rings, *tr, [64, 1024])
    assert lib.iqlhip_group_train_steps_mixed(*ts_args((C.c_int32 * K)(64, 600))) == hb.E_UNSUPPORTED
    _assert_unchanged(before, [a, b], rings)
    # ... and the group still steps
    logs = mixed.train([to_tb(step_batch(S, A, 64, seed=1)), to_tb(step_batch(S, A, 512, seed=2))])
    assert len(logs) == 2 and all(np.isfinite(list(l.values())).all() for l in logs)
