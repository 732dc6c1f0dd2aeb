"""GPU tests of weighted replay sampling in trainer groups (ImplicitQLearningGroup.train_steps_weighted /
iqlhip_group_train_steps_weighted; DESIGN.md 6i "trainer groups"): every member ends exactly — bit for bit — where its
solo train_steps_weighted (a member without a table: its solo train_steps) leaves a twin built identically:
parameters, targets, Adam moments, losses, step counts, dropout positions and step statistics.  Buffer sizes 65, 4097
and 262145 cover tables of two, three and four levels with a ragged last node at each."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import synth
import weighted_ref as W
from test_group_weighted_cpu import POISON_B, POISON_N, POISON_SEEDS, POISON_STEPS, poison_weights

pytestmark = pytest.mark.gpu

S, A = 17, 6


def _hip():
    import hip_helpers as H
    import iql
    import iqlhip_binding as hb
    import iqlhip_weighted as wtd
    return iql, hb, H, wtd


def _pair(i, dropout=0.0, bf16=False, drop_seed=None, stats=False, clip=None, count=2, dims=(S, A)):
    """Member i and its twin(s): the same parameters, hyper-parameters, learning rates and opt-in settings."""
    H = _hip()[2]
    S, A = dims
    params = synth.synth_params(S, A, seed=300 + i)
    hyper = {"iql_tau": 0.6 + 0.1 * (i % 4), "beta": 2.0 + i, "discount": 0.99, "tau": 0.005 * (1 + i)}
    lrs = {"v": 3e-4 * (1 + i), "q": 2e-4 * (1 + i), "pi": 1e-4 * (1 + i)}
    out = []
    for _ in range(count):
        t = H.build_hip_trainer(params, S, A, True, hyper, lrs, 40 if i == 2 else 1000, dropout=dropout)
        if drop_seed is not None:
            t.set_dropout_seed(drop_seed)
        if bf16:
            t.set_precision("bf16")
        t.set_step_stats(stats)
        t.set_grad_clip(clip)
        out.append(t)
    return out


def _pairs(K, **kw):
    pairs = [_pair(i, **kw) for i in range(K)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


@functools.lru_cache(maxsize=None)
def _data(n, dims=(S, A)):
    return synth.synth_transitions(n, dims[0], dims[1], seed=22)


def _buffer(n, poison=False, dims=(S, A)):
    iql = _hip()[0]
    S, A = dims
    data = {k: v.copy() for k, v in _data(n, dims).items()}
    if poison:      # (states AND rewards: a NaN pre-activation alone dies in the ReLU's max(x, 0); a NaN reward reaches the losses)
        for key in ("observations", "next_observations", "rewards"):
            data[key][1::2] = np.nan
    buf = iql.ReplayBuffer(S, A, n, "cuda")
    buf.load_d4rl_dataset(data)
    return buf


@functools.lru_cache(maxsize=None)
def _skewed(n, seed=8, sigma=2.0):
    """Log-normal weights over n rows, a tenth of them zero, zeros at both ends."""
    rng = np.random.RandomState(seed)
    w = np.exp(sigma * rng.randn(n)).astype(np.float32)
    w[rng.rand(n) < 0.1] = 0.0
    w[:3] = 0.0
    w[-2:] = 0.0
    w[n // 2] = 1.0
    w.setflags(write=False)
    return w


def _far_end(n):
    w = np.zeros(n, dtype=np.float32)
    w[n - 1] = 3.0
    return w


def _counters(t):
    hb = _hip()[1]
    c = (C.c_uint64 * 2)()
    hb.check(hb.lib().iqlhip_get_counters(t._ctx, c))
    return int(c[0]), int(c[1])


def _assert_same(a, b, what=""):
    H = _hip()[2]
    H.assert_same_trainer_state(a, b, what)
    assert np.array_equal(H.arenas(a), H.arenas(b)), what
    assert a.total_it == b.total_it, what
    assert _counters(a) == _counters(b), (what, _counters(a), _counters(b))


def _assert_losses(got, want, what=""):
    assert got.shape == want.shape and np.all(np.isfinite(got)), what
    assert np.array_equal(got, want), (what, got[:2], want[:2])


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("B", [256, 7])
def test_shared_buffer_and_shared_table_equal_solo_calls_bitwise(B):
    iql = _hip()[0]
    K, n, steps, seeds = 3, 4097, 5, [77, 78, 79]
    buf = _buffer(n)
    buf.set_sample_weights(_skewed(n))
    members, twins = _pairs(K)
    got = iql.ImplicitQLearningGroup(members).train_steps_weighted(buf, steps, B, seeds)
    assert got.shape == (K, steps, 3)
    for i in range(K):
        _assert_losses(got[i], twins[i].train_steps_weighted(buf, steps, B, seed=seeds[i]), f"member {i}")
        _assert_same(members[i], twins[i], f"member {i}")
        assert members[i].total_it == steps
    assert not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("dims", [(127, 1), (72, 28)])
def test_wide_rows_and_split_staging_equal_solo_calls_bitwise(dims):
    """iql_gather_weighted_group_kernel copies a row with the solo gathers' loop, 64 float4 per pass of a wave: at
    (127, 1) a packed row has 65 (tests/chunk_kind_shapes.py), the only shape that takes a second pass; at (72, 28) the
    group's forward stages V and pi by LDS-DMA while the critics read W0 from global.  300 rows: ten row tiles per member,
    two backward chunks."""
    from helpers import row_f4, w0_lds_k
    iql = _hip()[0]
    assert (row_f4(*dims), w0_lds_k(*dims)) == {(127, 1): (65, 0), (72, 28): (44, 72)}[dims]
    K, n, steps, B, seeds = 3, 2000, 3, 300, [77, 78, 79]
    buf = _buffer(n, dims=dims)
    buf.set_sample_weights(_skewed(n))
    pairs = [_pair(i, dims=dims) for i in range(K)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    got = iql.ImplicitQLearningGroup(members).train_steps_weighted(buf, steps, B, seeds)
    assert got.shape == (K, steps, 3)
    for i in range(K):
        _assert_losses(got[i], twins[i].train_steps_weighted(buf, steps, B, seed=seeds[i]), f"member {i}")
        _assert_same(members[i], twins[i], f"member {i}")
        assert members[i].total_it == steps
    assert not np.array_equal(got[0], got[1])
    # the solo call gathers through the same device function as the group: member 0 is also rebuilt from eager steps on
    # the integer reference's rows (gathered by ReplayBuffer.gather), which share nothing with either
    from burst_twins import eager_weighted_segment
    eager = _pair(0, count=1, dims=dims)[0]
    _assert_losses(got[0], eager_weighted_segment(eager, buf, _skewed(n), steps, B, seeds[0]), "member 0, eager rebuild")
    _hip()[2].assert_same_trainer_state(members[0], eager, "member 0, eager rebuild")


# ---------------------------------------------------------------------------------------------------------------- 2
def test_a_table_per_member_on_one_shared_buffer():
    """Four table levels; member 2's table has all its mass on the last row.  Member 0 is also rebuilt eagerly from the
    integer reference's indices, which pins the solo weights= keyword itself."""
    iql, _, _, wtd = _hip()
    K, n, steps, B, seeds = 3, 262145, 3, 64, [5, 6, 7]
    buf = _buffer(n)                                           # (no table of its own)
    ws = [_skewed(n, 8, 2.0), _skewed(n, 9, 4.0), _far_end(n)]
    tables = [wtd.SampleWeights(ws[0]), wtd.SampleWeights(torch.from_numpy(ws[1].copy()).cuda()), wtd.SampleWeights(ws[2])]
    assert [t.n for t in tables] == [n] * 3 and len({t.generation for t in tables}) == 3
    assert torch.all(tables[2].draw_indices(300, 3, 9) == n - 1)
    members, twins = _pairs(K)
    eager = _pair(0, count=1)[0]
    got = iql.ImplicitQLearningGroup(members).train_steps_weighted(buf, steps, B, seeds, weights=tables)
    for i in range(K):
        want = twins[i].train_steps_weighted(buf, steps, B, seed=seeds[i], weights=tables[i])
        _assert_losses(got[i], want, f"member {i}")
        _assert_same(members[i], twins[i], f"member {i}")
    idx = W.draw_indices(steps * B, ws[0], seeds[0], 0)
    assert np.array_equal(tables[0].draw_indices(steps * B, seeds[0], 0).cpu().numpy(), idx)
    for k in range(steps):
        log = eager.train(buf.gather(torch.from_numpy(idx[k * B:(k + 1) * B])))
        assert [log["value_loss"], log["q_loss"], log["actor_loss"]] == [float(x) for x in got[0, k]], k
    _hip()[2].assert_same_trainer_state(members[0], eager, "eager rebuild")
    assert buf.sample_weights_n is None
    with pytest.raises(ValueError, match="no sample weights"):
        twins[0].train_steps_weighted(buf, 2, B, seed=5)
    for t in tables:
        t.free()
    with pytest.raises(ValueError, match="freed"):
        twins[0].train_steps_weighted(buf, 2, B, seed=5, weights=tables[0])


# ---------------------------------------------------------------------------------------------------------------- 3
def test_uniform_and_weighted_members_side_by_side():
    iql, _, _, wtd = _hip()
    n, steps, B, seeds = 4097, 5, 256, [11, 12, 13]
    buf = _buffer(n)
    buf.set_sample_weights(_skewed(n, 3, 1.0))                 # (ignored: every member names its table, or None)
    w1, w2 = wtd.SampleWeights(_skewed(n)), wtd.SampleWeights(_skewed(n, 9, 4.0))
    members, twins = _pairs(3)
    got = iql.ImplicitQLearningGroup(members).train_steps_weighted(buf, steps, B, seeds, weights=[w1, None, w2])
    want = [twins[0].train_steps_weighted(buf, steps, B, seed=seeds[0], weights=w1),
            twins[1].train_steps(buf, steps, B, seed=seeds[1]),
            twins[2].train_steps_weighted(buf, steps, B, seed=seeds[2], weights=w2)]
    for i in range(3):
        _assert_losses(got[i], want[i], f"member {i}")
        _assert_same(members[i], twins[i], f"member {i}")
    # no member with a table: group.train_steps
    members, twins = _pairs(2)
    got = iql.ImplicitQLearningGroup(members).train_steps_weighted(buf, steps, B, seeds[:2], weights=[None, None])
    want = iql.ImplicitQLearningGroup(twins).train_steps(buf, steps, B, seeds[:2])
    _assert_losses(got, want, "[None, None]")
    for i in range(2):
        _assert_same(members[i], twins[i], f"uniform member {i}")


# ---------------------------------------------------------------------------------------------------------------- 4
def test_a_batch_size_per_member():
    iql, _, _, wtd = _hip()
    K, n, steps, Bs, seeds = 4, 65, 5, [64, 7, 256, 33], [1, 2, 3, 4]
    buf = _buffer(n)
    wa, wb = wtd.SampleWeights(_skewed(n)), wtd.SampleWeights(_far_end(n))
    tables = [wa, wb, wa, None]
    members, twins = _pairs(K)
    got = iql.ImplicitQLearningGroup(members, mixed_batch=True).train_steps_weighted(buf, steps, Bs, seeds, weights=tables)
    for i in range(K):
        if tables[i] is None:
            want = twins[i].train_steps(buf, steps, Bs[i], seed=seeds[i])
        else:
            want = twins[i].train_steps_weighted(buf, steps, Bs[i], seed=seeds[i], weights=tables[i])
        _assert_losses(got[i], want, f"member {i}")
        _assert_same(members[i], twins[i], f"member {i}")


# ---------------------------------------------------------------------------------------------------------------- 5
def test_poisoned_rows_are_never_drawn():
    """Odd rows hold NaN states and rewards and weigh 0 (tests/test_group_weighted_cpu.py checks the premise in the reference): a
    member that fell back to the uniform draw would train on one in its first step."""
    iql, _, H, wtd = _hip()
    K = len(POISON_SEEDS)
    buf = _buffer(POISON_N, poison=True)
    table = wtd.SampleWeights(poison_weights())
    members, twins = _pairs(K)
    got = iql.ImplicitQLearningGroup(members).train_steps_weighted(buf, POISON_STEPS, POISON_B, list(POISON_SEEDS), weights=table)
    assert np.all(np.isfinite(got))
    for t in members:
        assert np.all(np.isfinite(H.arenas(t)))
    # per-member tables, one of them the buffer's own: the same
    buf.set_sample_weights(poison_weights())
    more, _ = _pairs(K)
    again = iql.ImplicitQLearningGroup(more).train_steps_weighted(buf, POISON_STEPS, POISON_B, list(POISON_SEEDS))
    assert np.array_equal(again, got)
    uniform = iql.ImplicitQLearningGroup(twins).train_steps(buf, POISON_STEPS, POISON_B, list(POISON_SEEDS))
    assert np.all(np.any(np.isnan(uniform), axis=(1, 2)))      # every uniform member met a poisoned row


# ---------------------------------------------------------------------------------------------------------------- 6
def test_dropout_group_with_statistics_and_clipping():
    """Rates 0.1 / 0 / 0.1, own dropout seeds, statistics on member 0, clipping on member 2: the launch that gathers by
    weight also draws the step's keep-bits."""
    iql, _, _, wtd = _hip()
    n, steps, B, seeds = 4097, 4, 64, [21, 22, 23]
    buf = _buffer(n)
    tables = [wtd.SampleWeights(_skewed(n)), wtd.SampleWeights(_skewed(n, 9, 4.0)), None]
    pairs = [_pair(0, dropout=0.1, drop_seed=31, stats=True), _pair(1), _pair(2, dropout=0.1, drop_seed=33, clip=1.0)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    group = iql.ImplicitQLearningGroup(members, actor_dropout=True)

    def solo(i, **kw):
        if tables[i] is None:
            return twins[i].train_steps(buf, steps, B, seed=seeds[i], **kw)
        return twins[i].train_steps_weighted(buf, steps, B, seed=seeds[i], weights=tables[i], **kw)

    got = group.train_steps_weighted(buf, steps, B, seeds, weights=tables)
    for i in range(3):
        _assert_losses(got[i], solo(i), f"member {i}")
        _assert_same(members[i], twins[i], f"member {i}")
    assert [_counters(t)[0] for t in members] == [steps, 0, steps]
    stats = group.train_steps_weighted(buf, steps, B, seeds, weights=tables, return_stats=True)
    assert stats.shape == (steps, 3, 16) and np.all(np.isnan(stats[:, 1:]))
    _, want_stats = solo(0, return_stats=True)
    assert np.array_equal(stats[:, 0], want_stats)
    solo(1), solo(2)
    for i in range(3):
        _assert_same(members[i], twins[i], f"member {i}, second call")
    assert [_counters(t)[0] for t in members] == [2 * steps, 0, 2 * steps]


# ---------------------------------------------------------------------------------------------------------------- 7
def test_bf16_equal_weights_are_the_uniform_group_call():
    iql, _, _, wtd = _hip()
    n, steps, B, seeds = 4097, 5, 256, [3, 4, 5]
    buf = _buffer(n)
    table = wtd.SampleWeights(np.full(n, 0.7, dtype=np.float32))
    members, twins = _pairs(3, bf16=True)
    got = iql.ImplicitQLearningGroup(members).train_steps_weighted(buf, steps, B, seeds, weights=table)
    want = iql.ImplicitQLearningGroup(twins).train_steps(buf, steps, B, seeds)
    _assert_losses(got, want, "bf16")
    for i in range(3):
        _assert_same(members[i], twins[i], f"bf16 member {i}")


# ---------------------------------------------------------------------------------------------------------------- 8
def test_calls_cut_differently_give_the_same_result():
    iql, _, _, wtd = _hip()
    n, B, seeds = 4097, 64, [8, 9]
    buf = _buffer(n)
    tables = [wtd.SampleWeights(_skewed(n)), wtd.SampleWeights(_skewed(n, 9, 4.0))]
    trios = [_pair(i, count=3) for i in range(2)]
    groups = [iql.ImplicitQLearningGroup([trios[0][j], trios[1][j]]) for j in range(3)]
    one = groups[0].train_steps_weighted(buf, 6, B, seeds, weights=tables)
    two = np.concatenate([groups[1].train_steps_weighted(buf, 2, B, seeds, weights=tables),
                          groups[1].train_steps_weighted(buf, 4, B, seeds, weights=tables)], axis=1)
    cut = groups[2].train_steps_weighted(buf, 6, B, seeds, weights=tables, chunk=2)
    _assert_losses(two, one, "2 + 4")
    _assert_losses(cut, one, "chunk=2")
    for i in range(2):
        _assert_same(trios[i][1], trios[i][0], f"2 + 4, member {i}")
        _assert_same(trios[i][2], trios[i][0], f"chunk=2, member {i}")


# ---------------------------------------------------------------------------------------------------------------- 9
def _snapshot(trainers, buf):
    H = _hip()[2]
    return ([(H.arenas(t).copy(), t.total_it, dict(t._adam_t), t.actor_optimizer.param_groups[0]["lr"], t._ts_token,
              _counters(t)) for t in trainers], buf.sample_weights_n, buf._weights_gen, buf._writes)


def _assert_unchanged(trainers, buf, snap):
    now = _snapshot(trainers, buf)
    assert now[1:] == snap[1:]
    for a, b in zip(now[0], snap[0]):
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def test_refusals_leave_everything_as_it_was():
    iql, hb, _, wtd = _hip()
    n, B, seeds = 4097, 64, [5, 6]
    buf, bare = _buffer(n), _buffer(n)
    buf.set_sample_weights(_skewed(n))
    table, short = wtd.SampleWeights(_skewed(n, 9, 4.0)), wtd.SampleWeights(np.ones(n - 1, dtype=np.float32))
    pairs = [_pair(0, dropout=0.1, drop_seed=41), _pair(1)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    group = iql.ImplicitQLearningGroup(members, actor_dropout=True)
    group.train_steps_weighted(buf, 3, B, seeds)               # (counters, schedules and dropout positions off zero)
    for i in range(2):
        twins[i].train_steps_weighted(buf, 3, B, seed=seeds[i])
    snap = _snapshot(members, buf)
    with pytest.raises(ValueError, match="cover 4096 rows"):
        group.train_steps_weighted(buf, 2, B, seeds, weights=[table, short])
    with pytest.raises(ValueError, match="cover 4096 rows"):
        group.train_steps_weighted(buf, 2, B, seeds, weights=short)
    with pytest.raises(ValueError, match="no sample weights"):
        group.train_steps_weighted([buf, bare], 2, B, seeds)
    with pytest.raises(ValueError, match="weight tables for a group of 2"):
        group.train_steps_weighted(buf, 2, B, seeds, weights=[table])
    with pytest.raises(ValueError, match="differ"):
        group.train_steps_weighted(buf, 2, [64, 32], seeds, weights=table)      # not a mixed_batch group
    with pytest.raises(ValueError):
        group.train_steps_weighted(buf, 2, B, seeds, weights=table, return_stats=True)   # no member has statistics on
    members[1]._dp_exchange = "p2p"                            # (what enable_data_parallel records)
    try:
        with pytest.raises(NotImplementedError, match="data parallelism"):
            group.train_steps_weighted(buf, 2, B, seeds, weights=table)
    finally:
        members[1]._dp_exchange = None
    _assert_unchanged(members, buf, snap)
    # the library's own refusals: no table array, a table that does not weigh size[k] rows
    g = group._group()
    rows = (C.c_void_p * 2)(buf._rows.data_ptr(), buf._rows.data_ptr())
    tab = np.zeros((2, 12), dtype=np.float32)
    tabs = (C.c_void_p * 2)(tab.ctypes.data, tab.ctypes.data)
    args = [g, rows, buf._ld, (C.c_int64 * 2)(n, n), (C.c_int32 * 2)(B, B), tabs, 2, (C.c_uint64 * 2)(*seeds),
            (C.c_uint64 * 2)(0, 0), 0, members[0]._stream()]
    assert hb.lib().iqlhip_group_train_steps_weighted(*args, None) == hb.E_INVAL
    assert hb.lib().iqlhip_group_train_steps_weighted(*args, (C.c_void_p * 2)(table._table, short._table)) == hb.E_INVAL
    assert "member 1" in hb.last_error()
    args[3] = (C.c_int64 * 2)(n, n - 1)                         # the table fits, but member 1's rows do not reach row n - 1
    assert hb.lib().iqlhip_group_train_steps_weighted(*args, (C.c_void_p * 2)(table._table, table._table)) == hb.E_INVAL
    _assert_unchanged(members, buf, snap)
    # bf16 beyond the small-batch kernels
    bm, _ = _pairs(2, bf16=True)
    for t in bm:
        t.reserve_batch(1024)
    snap_b = _snapshot(bm, buf)
    with pytest.raises(NotImplementedError, match="512"):
        iql.ImplicitQLearningGroup(bm).train_steps_weighted(buf, 2, 1024, seeds, weights=table)
    _assert_unchanged(bm, buf, snap_b)
    # ... and the group goes on exactly where its twins do
    got = group.train_steps_weighted(buf, 3, B, seeds, weights=[None, table])
    _assert_losses(got[0], twins[0].train_steps(buf, 3, B, seed=seeds[0]), "after, member 0")
    _assert_losses(got[1], twins[1].train_steps_weighted(buf, 3, B, seed=seeds[1], weights=table), "after, member 1")
    for i in range(2):
        _assert_same(members[i], twins[i], f"after the refusals, member {i}")


# ---------------------------------------------------------------------------------------------------------------- 10
def test_a_group_of_one_is_the_solo_call():
    iql, _, _, wtd = _hip()
    n, B = 4097, 64
    buf = _buffer(n)
    buf.set_sample_weights(_skewed(n))
    table = wtd.SampleWeights(_skewed(n, 9, 4.0))
    m, twin = _pair(0)
    group = iql.ImplicitQLearningGroup([m])
    got = [group.train_steps_weighted(buf, 4, B, [5]), group.train_steps_weighted(buf, 4, B, [5], weights=table),
           group.train_steps_weighted(buf, 4, B, [5], weights=[table]), group.train_steps_weighted(buf, 4, B, [5], weights=[None])]
    want = [twin.train_steps_weighted(buf, 4, B, seed=5), twin.train_steps_weighted(buf, 4, B, seed=5, weights=table),
            twin.train_steps_weighted(buf, 4, B, seed=5, weights=table), twin.train_steps(buf, 4, B, seed=5)]
    for a, b in zip(got, want):
        assert a.shape == (1, 4, 3)
        _assert_losses(a[0], b, "group of one")
    _assert_same(m, twin, "group of one")
