"""GPU tests of weighted replay sampling: the device table and the device draw against the integer
reference (tests/weighted_ref.py) bit for bit, and train_steps_weighted against plain train_steps (equal weights) and
against eager train() calls on the reference's rows (skewed weights) — parameters, optimiser state, targets, losses and
counters compared bitwise."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import synth
import weighted_ref as W
from burst_twins import eager_weighted_segment, skewed_weights      # (the twin, shared with the shape table's tests)

pytestmark = pytest.mark.gpu

S, A = 17, 6
HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
N_ROWS = 5000
SIZES = [1, 63, 64, 65, 4095, 4096, 4097, 262145]        # the boundaries of one, two, three and four levels
M64 = (1 << 64) - 1


def _hip():
    import hip_helpers as H
    import iql
    import iqlhip_binding as hb
    return iql, hb, H


@functools.lru_cache(maxsize=None)
def _params():
    return synth.synth_params(S, A, seed=21)


@functools.lru_cache(maxsize=None)
def _data():
    return synth.synth_transitions(N_ROWS, S, A, seed=22)


def _new_buffer(n=N_ROWS, capacity=None):
    iql = _hip()[0]
    buf = iql.ReplayBuffer(S, A, capacity or n, "cuda")
    buf.load_d4rl_dataset({k: v[:n].copy() for k, v in _data().items()})
    return buf


def _Rows(n):
    """A buffer that draws over n rows for the table and draw tests, which never read a row: the bookkeeping only."""
    iql = _hip()[0]
    buf = iql.ReplayBuffer(1, 1, 1, "cuda")
    buf._size = buf._pointer = n
    return buf


@functools.lru_cache(maxsize=None)
def _weights(n):
    """Isolated zeros, runs of zeros at both ends (where n allows), a dynamic range beyond 2^39."""
    rng = np.random.RandomState(n)
    w = (rng.rand(n) * np.exp2(rng.randint(-45, 3, size=n))).astype(np.float32)
    w[rng.rand(n) < 0.1] = 0.0
    if n >= 63:
        w[:7] = 0.0
        w[-9:] = 0.0
        w[n // 2] = 1.5                    # (the largest: everything below 1.5 * 2^-39 quantises to 0)
    if not np.any(w > 0):
        w[0] = 0.25
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _skewed():
    """Weights over the N_ROWS rows of the training tests: log-normal, a tenth of them zero."""
    return skewed_weights(N_ROWS, of=N_ROWS)


def _build(dropout=0.0, bf16=False, stats=False, clip=None):
    tr = _hip()[2].build_hip_trainer(_params(), S, A, True, dict(HYPER), dict(LRS), 1000, dropout=dropout)
    if dropout:
        tr.set_dropout_seed(11)
    if bf16:
        tr.set_precision("bf16")
    tr.set_step_stats(stats)
    tr.set_grad_clip(clip)
    return tr


def _device_table(buf):
    hb = _hip()[1]
    n, total, levels, gen = C.c_int64(), C.c_uint64(), C.c_int32(), C.c_uint64()
    cum = np.empty(buf.sample_weights_n, dtype=np.uint64)
    hb.check(hb.lib().iqlhip_weights_info(buf._weights, C.byref(n), C.byref(total), C.byref(levels), C.byref(gen),
                                          cum.ctypes.data))
    assert n.value == buf.sample_weights_n
    return cum, int(total.value), int(levels.value), int(gen.value)


def _levels(n):
    k = 1
    while n > 64:
        n = (n + 63) // 64
        k += 1
    return k


def _assert_steps_equal(lg, le, what=""):
    assert np.all(np.isfinite(lg))
    bad = np.nonzero(np.any(lg != le, axis=1))[0]
    assert bad.size == 0, f"{what}: steps {bad.tolist()} differ: {lg[bad[0]]} vs {le[bad[0]]}"


# ---------------------------------------------------------------- the table
@pytest.mark.parametrize("n", SIZES)
def test_table_equals_the_reference(n):
    w = _weights(n)
    cum_ref, total_ref = W.table(w)
    buf = _Rows(n)
    buf.set_sample_weights(w)                                   # a host array
    assert buf.sample_weights_n == n
    cum, total, levels, gen_host = _device_table(buf)
    assert levels == _levels(n)
    assert total == total_ref and np.array_equal(cum, cum_ref)
    buf.set_sample_weights(torch.from_numpy(w.copy()).cuda())   # a device tensor: the same table, a new generation
    cum, total, _, gen_dev = _device_table(buf)
    assert total == total_ref and np.array_equal(cum, cum_ref) and gen_dev != gen_host
    buf.set_sample_weights(torch.from_numpy(w.copy()))          # a host tensor
    assert np.array_equal(_device_table(buf)[0], cum_ref)
    buf.set_sample_weights(None)
    assert buf.sample_weights_n is None


# ---------------------------------------------------------------- the draw
@pytest.mark.parametrize("n", SIZES)
def test_draw_equals_the_reference(n):
    w = _weights(n)
    buf = _Rows(n)
    buf.set_sample_weights(w)
    for seed, offset in ((5, 0), (2 ** 63 + 11, 12345677), (7, M64), (9, M64 - 1024)):      # even / odd offsets, the wrap
        got = buf.draw_weighted_indices(4099, seed, offset).cpu().numpy()
        want = W.draw_indices(4099, w, seed, offset)
        assert np.array_equal(got, want), (n, seed, offset, np.nonzero(got != want)[0][:5])
        assert np.all(w[got] > 0)                               # zero-weight rows are absent
    # an odd first index: indices j0 .. of a stream are the tail of the draw from 0
    got = buf.draw_weighted_indices(200, 5, 40).cpu().numpy()
    assert np.array_equal(got[3:], W.draw_indices(197, w, 5, 40, j0=3))


@pytest.mark.parametrize("n", [1, 65, 4097, 262145])
@pytest.mark.parametrize("last", [False, True])
def test_a_single_non_zero_row(n, last):
    w = np.zeros(n, dtype=np.float32)
    row = n - 1 if last else 0
    w[row] = 3.0
    buf = _Rows(n)
    buf.set_sample_weights(w)
    assert torch.all(buf.draw_weighted_indices(4099, 3, M64 - 5) == row)


# ---------------------------------------------------------------- equal weights: the plain call
@pytest.mark.parametrize("B", [256, 7])
def test_equal_weights_are_train_steps(B):
    """70 steps: the directly launched head and captured chunks.  Everything a call moves is compared."""
    H = _hip()[2]
    bw, bp = _new_buffer(), _new_buffer()
    bw.set_sample_weights(np.full(N_ROWS, 0.7, dtype=np.float32))
    g, e = _build(), _build()
    lg = g.train_steps_weighted(bw, 70, B, seed=5)
    le = e.train_steps(bp, 70, B, seed=5)
    _assert_steps_equal(lg, le, f"B={B}")
    H.assert_same_trainer_state(g, e, "equal weights")
    assert np.array_equal(H.arenas(g), H.arenas(e))
    assert g.total_it == e.total_it == 70
    # the stream goes on where a plain call's would: the next plain calls draw the same rows
    _assert_steps_equal(g.train_steps(bp, 6, B, seed=5), e.train_steps(bp, 6, B, seed=5), "the call after")


def test_bf16_equal_weights_are_train_steps():
    H = _hip()[2]
    bw, bp = _new_buffer(), _new_buffer()
    bw.set_sample_weights(torch.ones(N_ROWS, device="cuda"))
    g, e = _build(bf16=True), _build(bf16=True)
    _assert_steps_equal(g.train_steps_weighted(bw, 70, 256, seed=3), e.train_steps(bp, 70, 256, seed=3), "bf16")
    H.assert_same_trainer_state(g, e, "bf16 equal weights")


# ---------------------------------------------------------------- skewed weights: eager steps on the reference's rows
@pytest.mark.parametrize("B", [256, 7])
def test_skewed_weights_equal_eager_steps(B):
    H = _hip()[2]
    buf, w = _new_buffer(), _skewed()
    buf.set_sample_weights(w)
    g, e = _build(), _build()
    lg = g.train_steps_weighted(buf, 70, B, seed=5)
    le = eager_weighted_segment(e, buf, w, 70, B, 5)
    _assert_steps_equal(lg, le, f"B={B}")
    H.assert_same_trainer_state(g, e, "skewed vs eager")
    assert len({tuple(r) for r in lg}) == 70


def test_split_calls_continue_on_the_staged_rows():
    """3 + 67 steps at an even batch size: the second call follows the first one's stream; 4 + 66: it also starts on the
    rows the first one's last forward staged (an even step count ends on the staging buffer a call's step 0 reads)."""
    H = _hip()[2]
    buf, w = _new_buffer(), _skewed()
    buf.set_sample_weights(w)
    for first in (3, 4):
        g, e = _build(), _build()
        lg = np.concatenate([g.train_steps_weighted(buf, first, 64, seed=5), g.train_steps_weighted(buf, 70 - first, 64, seed=5)])
        le = eager_weighted_segment(e, buf, w, 70, 64, 5)
        _assert_steps_equal(lg, le, f"{first} + {70 - first}")
        H.assert_same_trainer_state(g, e, "split")


def test_new_weights_between_two_calls():
    """The second call draws from the new table: nothing staged by the first call's last forward is used."""
    H = _hip()[2]
    buf, w1 = _new_buffer(), _skewed()
    w2 = np.ascontiguousarray(w1[::-1])
    g, e = _build(), _build()
    buf.set_sample_weights(w1)
    la = g.train_steps_weighted(buf, 4, 64, seed=5)
    ea = eager_weighted_segment(e, buf, w1, 4, 64, 5)
    buf.set_sample_weights(w2)
    lb = g.train_steps_weighted(buf, 66, 64, seed=5)
    eb = eager_weighted_segment(e, buf, w2, 66, 64, 5)
    _assert_steps_equal(np.concatenate([la, lb]), np.concatenate([ea, eb]), "new weights")
    H.assert_same_trainer_state(g, e, "new weights")


def test_plain_and_weighted_calls_never_continue_each_other():
    H = _hip()[2]
    buf, w = _new_buffer(), _skewed()
    buf.set_sample_weights(w)
    g, e = _build(), _build()
    for seg in ("plain", "weighted", "plain", "weighted"):
        if seg == "plain":
            lg, le = g.train_steps(buf, 4, 64, seed=5), H.eager_segment(e, buf, 4, 64, 5)
        else:
            lg, le = g.train_steps_weighted(buf, 4, 64, seed=5), eager_weighted_segment(e, buf, w, 4, 64, 5)
        _assert_steps_equal(lg, le, seg)
    H.assert_same_trainer_state(g, e, "plain / weighted")


def test_the_library_checks_the_table_generation():
    """IQLHIP_TS_CONTINUE passed to every call through the C ABI: honoured behind a weighted call on the same table
    only — not behind a plain call, not behind a call on another table, and a plain call honours it behind no weighted
    one.  Every call is contiguous with the one before in all else the library compares, so a continuation wrongly
    honoured would train step 0 on rows drawn the other way."""
    _, hb, H = _hip()
    buf, w = _new_buffer(), _skewed()
    lib, B, seed = hb.lib(), 64, 5

    def call(tr, k, weighted):
        tr._prepare(B)
        tab = tr._scalar_table(k, 1.0 / B)
        off = tr.total_it * (B // 2)
        if weighted:
            hb.check(lib.iqlhip_train_steps_weighted(tr._ctx, buf._rows.data_ptr(), buf._ld, N_ROWS, B, tab.ctypes.data, k,
                                                     seed, off, hb.TS_CONTINUE, tr._stream(), buf._weights))
        else:
            hb.check(lib.iqlhip_train_steps(tr._ctx, buf._rows.data_ptr(), buf._ld, N_ROWS, B, tab.ctypes.data, k, seed,
                                            off, hb.TS_CONTINUE, tr._stream()))
        out = (C.c_float * (3 * k))()
        hb.check(lib.iqlhip_read_loss_ring(tr._ctx, out, k, tr._stream()))
        tr.total_it += k
        return np.frombuffer(out, dtype=np.float32).reshape(k, 3).copy()

    g, e = _build(), _build()
    buf.set_sample_weights(w)
    got = [call(g, 4, False), call(g, 4, True), call(g, 4, True)]
    want = [H.eager_segment(e, buf, 4, B, seed), eager_weighted_segment(e, buf, w, 4, B, seed),
            eager_weighted_segment(e, buf, w, 4, B, seed)]
    w2 = np.ascontiguousarray(w[::-1])
    buf.set_sample_weights(w2)
    got += [call(g, 4, True), call(g, 4, False)]
    want += [eager_weighted_segment(e, buf, w2, 4, B, seed), H.eager_segment(e, buf, 4, B, seed)]
    _assert_steps_equal(np.concatenate(got), np.concatenate(want), "generation")
    H.assert_same_trainer_state(g, e, "generation")


def test_sample_weighted_returns_the_reference_rows():
    buf, w = _new_buffer(), _skewed()
    buf.set_sample_weights(w)
    idx = W.draw_indices(33, w, 17, 1000)
    got = buf.sample_weighted(33, 17, 1000)
    want = buf.gather(torch.from_numpy(idx))
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_dropout_statistics_and_clipping_together():
    H = _hip()[2]
    buf, w = _new_buffer(), _skewed()
    buf.set_sample_weights(w)
    kw = dict(dropout=0.1, stats=True, clip=1.0)
    g, e = _build(**kw), _build(**kw)
    lg, sg = g.train_steps_weighted(buf, 70, 64, seed=5, return_stats=True)
    le, se = eager_weighted_segment(e, buf, w, 70, 64, 5, with_stats=True)
    _assert_steps_equal(lg, le, "combined")
    assert np.array_equal(sg, se)
    H.assert_same_trainer_state(g, e, "combined")


# ---------------------------------------------------------------- every other call ignores weights
def test_other_calls_ignore_weights():
    H = _hip()[2]
    bw, bp = _new_buffer(capacity=N_ROWS + 8), _new_buffer(capacity=N_ROWS + 8)
    bw.set_sample_weights(_skewed())
    g, e = _build(), _build()
    _assert_steps_equal(g.train_steps(bw, 6, 64, seed=5), e.train_steps(bp, 6, 64, seed=5), "train_steps")
    np.random.seed(4)
    sa = bw.sample(32)
    np.random.seed(4)
    sb = bp.sample(32)
    for a, b in zip(sa, sb):
        assert torch.equal(a, b)
    d = _data()
    np.random.seed(6)
    la = g.online_step(bw, d["observations"][0], d["actions"][0], 1.0, d["next_observations"][0], False, 32)
    np.random.seed(6)
    lb = e.online_step(bp, d["observations"][0], d["actions"][0], 1.0, d["next_observations"][0], False, 32)
    assert la == lb
    H.assert_same_trainer_state(g, e, "weights ignored")
    # the online step grew the buffer: the weights no longer cover its index bound
    with pytest.raises(ValueError, match="set_sample_weights again"):
        g.train_steps_weighted(bw, 2, 32, seed=5)


# ---------------------------------------------------------------- refusals
def _snapshot(tr, buf):
    H = _hip()[2]
    return (H.arenas(tr).copy(), tr.total_it, dict(tr._adam_t), tr.actor_optimizer.param_groups[0]["lr"], tr._ts_token,
            buf.sample_weights_n, buf._weights_gen)


def _assert_unchanged(tr, buf, snap):
    now = _snapshot(tr, buf)
    assert np.array_equal(now[0], snap[0]) and now[1:] == snap[1:]


def test_refusals_leave_everything_as_it_was():
    iql, hb, H = _hip()
    buf, twin_buf, w = _new_buffer(), _new_buffer(), _skewed()
    g, twin = _build(), _build()
    buf.set_sample_weights(w)
    g.train_steps_weighted(buf, 4, 64, seed=5)
    eager_weighted_segment(twin, twin_buf, w, 4, 64, 5)
    snap = _snapshot(g, buf)
    cum0 = _device_table(buf)[0].copy()
    # weights the library or the checks refuse: the previous table stays in force
    for bad in (np.full(N_ROWS, np.nan, dtype=np.float32), np.full(N_ROWS, np.inf, dtype=np.float32),
                -np.ones(N_ROWS, dtype=np.float32), np.zeros(N_ROWS, dtype=np.float32),
                np.ones(N_ROWS - 1, dtype=np.float32), np.ones(N_ROWS, dtype=np.float64), np.ones((N_ROWS, 1), dtype=np.float32)):
        for form in (bad, torch.from_numpy(bad).cuda()):
            with pytest.raises(ValueError):
                buf.set_sample_weights(form)
            _assert_unchanged(g, buf, snap)
    one_bad = w.copy()
    one_bad[N_ROWS - 1] = -1e-30
    with pytest.raises(ValueError):
        buf.set_sample_weights(torch.from_numpy(one_bad).cuda())
    assert np.array_equal(_device_table(buf)[0], cum0)
    # calls
    with pytest.raises(ValueError, match="no sample weights"):
        g.train_steps_weighted(twin_buf, 2, 64, seed=5)
    with pytest.raises(ValueError):
        g.train_steps_weighted(buf, 2, 64, seed=5, return_stats=True)            # statistics are off
    keep = np.ones((64, 256), dtype=bool)
    gd = _build(dropout=0.1)
    gd.inject_dropout_masks(keep, keep)
    snap_d = _snapshot(gd, buf)
    with pytest.raises(NotImplementedError):
        gd.train_steps_weighted(buf, 2, 64, seed=5)
    with pytest.raises(NotImplementedError):
        gd.prepare_train_steps_weighted(buf, 64)
    _assert_unchanged(gd, buf, snap_d)
    gb = _build(bf16=True)
    gb.reserve_batch(1024)
    snap_b = _snapshot(gb, buf)
    with pytest.raises(NotImplementedError):
        gb.train_steps_weighted(buf, 2, 1024, seed=5)
    _assert_unchanged(gb, buf, snap_b)
    g._dp_exchange = "p2p"                                       # (what enable_data_parallel records)
    try:
        with pytest.raises(NotImplementedError):
            g.train_steps_weighted(buf, 2, 64, seed=5)
    finally:
        g._dp_exchange = None
    _assert_unchanged(g, buf, snap)
    # the library's own refusal of a table that does not cover `size` rows
    tab = np.zeros((2, 12), dtype=np.float32)
    rc = hb.lib().iqlhip_train_steps_weighted(g._ctx, buf._rows.data_ptr(), buf._ld, N_ROWS - 1, 64, tab.ctypes.data, 2, 5, 0, 0,
                                              g._stream(), buf._weights)
    assert rc == hb.E_INVAL
    _assert_unchanged(g, buf, snap)
    # ... and the staged batch is still the one the first call left: the next calls match the untouched twin
    _assert_steps_equal(g.train_steps_weighted(buf, 4, 64, seed=5), eager_weighted_segment(twin, twin_buf, w, 4, 64, 5), "after")
    _assert_steps_equal(g.train_steps(buf, 4, 64, seed=5), H.eager_segment(twin, twin_buf, 4, 64, 5), "plain after")
    H.assert_same_trainer_state(g, twin, "after the refusals")
