"""GPU tests of updatable weight tables (iqlhip_weights_build_updatable / iqlhip_weights_update; DESIGN.md 6i "updatable
tables"): the node-local layout draws what the static table draws, an update leaves what a fresh build of the changed
weights holds — bit for bit, against the CPU statement in tests/weighted_update_ref.py — and the weighted training calls
take such a table."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import synth
import weighted_ref as W
import weighted_update_ref as U

pytestmark = pytest.mark.gpu

S, A = 17, 6
HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
SIZES = [1, 63, 64, 65, 4097, 262145]          # one, two, three and four levels, ragged last nodes
STREAMS = ((5, 0), (2 ** 63 + 11, 12345677))   # (seed, offset): an even and an odd offset
N_DRAW = 2048


def _hip():
    import hip_helpers as H
    import iql
    import iqlhip_binding as hb
    import iqlhip_weighted as wtd
    return iql, hb, H, wtd


def _dev(x):
    return torch.from_numpy(np.array(x)).cuda()                           # (a copy: the cached vectors are read-only)


@functools.lru_cache(maxsize=None)
def _lognormal(n, seed=0):
    """Log-normal weights, a tenth of them zero; the largest is 8.0 (row n // 2), so the scale is known: e = 3."""
    rng = np.random.RandomState(1000 * seed + n)
    w = np.minimum(np.exp(1.5 * rng.randn(n)), 7.5).astype(np.float32)
    w[rng.rand(n) < 0.1] = 0.0
    w[n // 2] = 8.0
    w.setflags(write=False)
    return w


def _static_cum(table):
    hb = _hip()[1]
    cum = np.empty(table.n, dtype=np.uint64)
    hb.check(hb.lib().iqlhip_weights_info(table._table, None, None, None, None, cum.ctypes.data))
    return cum


def _draws(table):
    return [table.draw_indices(N_DRAW, s, o).cpu().numpy() for s, o in STREAMS]


def _assert_state(table, ref, what=""):
    """Leaves, total and draws of a device table against the CPU reference table."""
    q = table.leaves()
    assert np.array_equal(q, ref.q), (what, np.nonzero(q != ref.q)[0][:5])
    assert table.total() == ref.total, what
    for (s, o), got in zip(STREAMS, _draws(table)):
        assert np.array_equal(got, ref.draw_indices(N_DRAW, s, o)), (what, s, o)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("n", SIZES)
def test_layout_identity(n):
    wtd = _hip()[3]
    w = _lognormal(n)
    static = wtd.SampleWeights(w)
    upd = wtd.SampleWeights(w, updatable=True)
    roomy = wtd.SampleWeights(_dev(w), updatable=True, capacity=n + 100)
    assert upd.updatable and not static.updatable and upd.n == n and roomy.n == n + 100
    assert upd.version == 0 and upd.flags() == 0
    cum = _static_cum(static)
    q_static = np.diff(cum, prepend=np.uint64(0))
    assert np.array_equal(q_static, W.quantise(w))
    assert np.array_equal(static.leaves(), q_static)                      # (the read-back serves a static table too)
    assert np.array_equal(upd.leaves(), q_static) and upd.total() == int(cum[-1]) == static.total()
    lr = roomy.leaves()
    assert np.array_equal(lr[:n], q_static) and not lr[n:].any() and roomy.total() == int(cum[-1])
    for (s, o), a, b, c in zip(STREAMS, _draws(static), _draws(upd), _draws(roomy)):
        want = W.draw_indices(N_DRAW, w, s, o)
        assert np.array_equal(a, want) and np.array_equal(b, want) and np.array_equal(c, want), (n, s, o)
        assert c.max() < n


# ---------------------------------------------------------------------------------------------------------------- 2
def _entries(n, m, rng):
    """m update entries: rows 0, 63, 64 and n - 1, two rows of one level-0 node, one row three times with different
    weights (as far as n and m allow); the rest random with replacement.  Weights in [0, 16): inside the scale."""
    rep = min(5, n - 1)
    rows = [0, 63, 64, n - 1, min(66, n - 1), min(67, n - 1), rep, rep, rep]
    rows = [r for r in rows if r < n][:m]
    idx = np.array(rows + list(rng.randint(0, n, size=m - len(rows))), dtype=np.int64)
    w = (rng.rand(m) * 15.9).astype(np.float32)
    w[rng.rand(m) < 0.15] = 0.0
    return idx, w


@pytest.mark.parametrize("n", SIZES)
def test_update_equals_rebuild(n):
    wtd = _hip()[3]
    rng = np.random.RandomState(n)
    w = _lognormal(n)
    MW = 10.0                                                             # e = 3: weights below 16 are inside the scale
    tab = wtd.SampleWeights(w, updatable=True, max_weight=MW)
    ref = U.Table(w, max_weight=MW)
    mod = w.copy()
    for k, m in enumerate((1, 64, 257)):
        idx, uw = _entries(n, m, rng)
        tab.update(_dev(idx), _dev(uw))
        ref.update(idx, uw)
        for i, x in zip(idx, uw):
            mod[i] = x
        assert tab.version == ref.version == k + 1
        _assert_state(tab, ref, f"n={n} m={m}")
        # (`mod` took the entries in order: a row given several times holds its last weight)
        assert np.array_equal(tab.leaves(), U.quantise_at(mod, ref.e)), (n, m)
    assert tab.flags() == 0
    if mod.any():
        fresh = wtd.SampleWeights(mod, updatable=True, max_weight=MW)
        assert np.array_equal(fresh.leaves(), tab.leaves()) and fresh.total() == tab.total()
        for a, b in zip(_draws(fresh), _draws(tab)):
            assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- 3
def test_no_drift_over_many_updates():
    wtd = _hip()[3]
    n, MW = 4097, 10.0
    rng = np.random.RandomState(3)
    w = _lognormal(n)
    tab = wtd.SampleWeights(w, updatable=True, max_weight=MW)
    ref = U.Table(w, max_weight=MW)
    mod = w.copy()
    for _ in range(40):
        idx = rng.randint(0, n, size=256).astype(np.int64)
        uw = (rng.rand(256) * 15.9).astype(np.float32)
        uw[rng.rand(256) < 0.2] = 0.0
        tab.update(_dev(idx), _dev(uw))
        ref.update(idx, uw)
        for i, x in zip(idx, uw):
            mod[i] = x
    assert tab.version == 40
    _assert_state(tab, ref, "40 rounds")
    fresh = wtd.SampleWeights(mod, updatable=True, max_weight=MW)
    assert np.array_equal(fresh.leaves(), tab.leaves()) and fresh.total() == tab.total()
    assert np.array_equal(_draws(fresh)[0], _draws(tab)[0])


# ---------------------------------------------------------------------------------------------------------------- 4
def test_edge_values():
    wtd = _hip()[3]
    n = 4097
    w = _lognormal(n)
    tab = wtd.SampleWeights(w, updatable=True)                            # e = 3
    ref = U.Table(w)
    # a weight of 0: the row is absent from the draws
    heavy = int(np.argmax(w))
    tab.update(_dev(np.array([heavy], dtype=np.int64)), _dev(np.zeros(1, dtype=np.float32)))
    ref.update([heavy], np.zeros(1, dtype=np.float32))
    got = tab.draw_indices(4096, 9, 4).cpu().numpy()
    assert heavy not in got and np.array_equal(got, ref.draw_indices(4096, 9, 4))
    # a weight above the scale saturates
    tab.update(_dev(np.array([7], dtype=np.int64)), _dev(np.array([1e6], dtype=np.float32)))
    ref.update([7], np.array([1e6], dtype=np.float32))
    assert int(tab.leaves()[7]) == (1 << 39) - 1 == int(ref.q[7])
    assert tab.flags() == 0
    # bad entries are skipped and flagged, one kind at a time; the other entries of the call are applied
    bound = 4000
    for bad_i, bad_w, bit in ((10, np.nan, 1), (10, np.inf, 1), (10, -1.0, 2), (-1, 1.0, 4), (bound, 1.0, 4), (n - 1, 1.0, 4)):
        idx = np.array([20, bad_i, 21], dtype=np.int64)
        uw = np.array([0.5, bad_w, 2.5], dtype=np.float32)
        before = tab.leaves()
        tab.update(_dev(idx), _dev(uw), bound=bound)
        ref.update(idx, uw, bound=bound)
        assert tab.flags() == bit == ref.flags, (bad_i, bad_w)
        after = tab.leaves()
        assert np.array_equal(after, ref.q)
        if 0 <= bad_i < n:
            assert after[bad_i] == before[bad_i]
        assert int(after[20]) == int(U.quantise_at(uw[:1], ref.e)[0]) and int(after[21]) == int(U.quantise_at(uw[2:], ref.e)[0])
        tab.clear_flags()
        ref.flags = 0
        assert tab.flags() == 0
    tab.update(_dev(np.array([3], dtype=np.int64)), _dev(np.array([-0.0], dtype=np.float32)))      # -0.0 is zero
    assert tab.flags() == 0 and int(tab.leaves()[3]) == 0
    ref.update([3], np.array([-0.0], dtype=np.float32))
    _assert_state(tab, ref, "edge values")
    # every row zeroed: the total is 0 and draws stay inside [0, n)
    tab.update(torch.arange(n, device="cuda"), torch.zeros(n, device="cuda"))
    assert tab.total() == 0 and not tab.leaves().any()
    got = tab.draw_indices(4096, 1, 2)
    assert int(got.min()) >= 0 and int(got.max()) < n
    # ... and the table comes back
    tab.update(_dev(np.array([5, 4000], dtype=np.int64)), _dev(np.array([1.0, 3.0], dtype=np.float32)))
    assert set(tab.draw_indices(4096, 1, 2).cpu().numpy().tolist()) == {5, 4000}
    with pytest.raises(ValueError, match="not updatable"):
        wtd.SampleWeights(w).update(torch.zeros(1, dtype=torch.int64, device="cuda"), torch.ones(1, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- 5-7
N_ROWS = 1000


@functools.lru_cache(maxsize=None)
def _params():
    return synth.synth_params(S, A, seed=21)


@functools.lru_cache(maxsize=None)
def _data():
    return synth.synth_transitions(1536, S, A, seed=22)


def _new_buffer(n=N_ROWS, capacity=None):
    iql = _hip()[0]
    buf = iql.ReplayBuffer(S, A, capacity or n, "cuda")
    buf.load_d4rl_dataset({k: v[:n].copy() for k, v in _data().items()})
    return buf


def _build(bf16=False):
    tr = _hip()[2].build_hip_trainer(_params(), S, A, True, dict(HYPER), dict(LRS), 1000)
    if bf16:
        tr.set_precision("bf16")
    return tr


def _same(a, b, what):
    H = _hip()[2]
    H.assert_same_trainer_state(a, b, what)
    assert np.array_equal(H.arenas(a), H.arenas(b)), what
    assert a.total_it == b.total_it, what


def eager_weighted_segment(tr, buf, w, K, B, seed):
    """K eager train() steps on the rows train_steps_weighted(buf, K, B, seed) draws at the trainer's total_it."""
    idx = W.draw_indices(K * B, w, seed, tr.total_it * ((B + 1) // 2))
    losses = np.empty((K, 3), dtype=np.float32)
    for k in range(K):
        log = tr.train(buf.gather(torch.from_numpy(idx[k * B:(k + 1) * B])))
        losses[k] = [log["value_loss"], log["q_loss"], log["actor_loss"]]
    return losses


@pytest.mark.parametrize("bf16", [False, True])
def test_training_on_an_updatable_table_is_training_on_the_static_one(bf16):
    w = _lognormal(N_ROWS, seed=1)
    bu, bs = _new_buffer(N_ROWS, 1536), _new_buffer(N_ROWS, 1536)
    bu.set_sample_weights(w, updatable=True)
    bs.set_sample_weights(w)
    assert bu.sample_weights_n == 1536 and bs.sample_weights_n == N_ROWS
    g, e = _build(bf16), _build(bf16)
    lg = g.train_steps_weighted(bu, 8, 64, seed=5)
    le = e.train_steps_weighted(bs, 8, 64, seed=5)
    assert np.all(np.isfinite(lg)) and np.array_equal(lg, le)
    _same(g, e, "updatable vs static")


def test_an_update_ends_the_continuation():
    """Through the C ABI with IQLHIP_TS_CONTINUE on every call: honoured behind a call on the same table version, not
    behind an update — a continuation wrongly honoured would train step 0 on rows drawn by the old weights.  The twin
    runs eager steps on the reference's rows for the weights in force at each call."""
    _, hb, H, wtd = _hip()
    lib, B, seed = hb.lib(), 64, 5
    w1 = _lognormal(N_ROWS, seed=1)
    buf = _new_buffer()
    tab = wtd.SampleWeights(w1, updatable=True)

    def call(tr, k):
        tr._prepare(B)
        sc = tr._scalar_table(k, 1.0 / B)
        hb.check(lib.iqlhip_train_steps_weighted(tr._ctx, buf._rows.data_ptr(), buf._ld, N_ROWS, B, sc.ctypes.data, k, seed,
                                                 tr.total_it * (B // 2), hb.TS_CONTINUE, tr._stream(), tab._table))
        out = (C.c_float * (3 * k))()
        hb.check(lib.iqlhip_read_loss_ring(tr._ctx, out, k, tr._stream()))
        tr.total_it += k
        return np.frombuffer(out, dtype=np.float32).reshape(k, 3).copy()

    g, e = _build(), _build()
    got = [call(g, 4), call(g, 4)]                                        # the second continues: same generation, version
    want = [eager_weighted_segment(e, buf, w1, 4, B, seed), eager_weighted_segment(e, buf, w1, 4, B, seed)]
    # 64 rows change, among them every row the next step would draw by the old weights (the largest weight stays: one scale)
    nxt = np.unique(W.draw_indices(B, w1, seed, g.total_it * (B // 2)))
    nxt = nxt[nxt != N_ROWS // 2]
    rows = np.concatenate([nxt, np.setdiff1d(np.arange(100, 200), nxt)])[:64].astype(np.int64)
    w2 = w1.copy()
    w2[rows] = 0.0
    w2[rows[-3:]] = 6.0
    tab.update(_dev(rows), _dev(w2[rows]))
    got += [call(g, 4), call(g, 4)]
    want += [eager_weighted_segment(e, buf, w2, 4, B, seed), eager_weighted_segment(e, buf, w2, 4, B, seed)]
    got, want = np.concatenate(got), np.concatenate(want)
    assert np.all(np.isfinite(got))
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    assert bad.size == 0, f"steps {bad.tolist()} differ"
    H.assert_same_trainer_state(g, e, "update between continued calls")


def test_python_continuation_keys_on_the_version():
    """The same through train_steps_weighted: two calls with CONTINUE, an update, a third — against a trainer that ran
    the calls without a continuation, the last on a fresh build of the updated weights."""
    wtd = _hip()[3]
    w1 = _lognormal(N_ROWS, seed=1)
    buf = _new_buffer()
    tab = wtd.SampleWeights(w1, updatable=True)
    g, e = _build(), _build()
    lg = [g.train_steps_weighted(buf, 4, 64, seed=5, weights=tab)]
    tok = g._ts_token
    lg.append(g.train_steps_weighted(buf, 4, 64, seed=5, weights=tab))
    assert g._ts_token == tok                                             # no update in between: the token stands
    rows = np.arange(300, 364, dtype=np.int64)
    w2 = w1.copy()
    w2[rows] = np.linspace(0.0, 7.0, 64, dtype=np.float32)
    tab.update(_dev(rows), _dev(w2[rows]))
    lg.append(g.train_steps_weighted(buf, 4, 64, seed=5, weights=tab))
    assert g._ts_token != tok
    le = []
    for w in (w1, w1, w2):
        fresh = wtd.SampleWeights(w, updatable=True, max_weight=8.0)
        e._ts_token = None
        le.append(e.train_steps_weighted(buf, 4, 64, seed=5, weights=fresh))
    assert np.array_equal(np.concatenate(lg), np.concatenate(le))
    _same(g, e, "continuation")


def test_ring_growth():
    wtd = _hip()[3]
    n0, cap = 500, 1024
    w = _lognormal(n0, seed=2)
    buf = _new_buffer(n0, cap)
    buf.set_sample_weights(w, updatable=True)
    rng = np.random.RandomState(5)
    new_w = (rng.rand(10) * 7.9).astype(np.float32)                       # (below the largest weight: one scale)
    for k in range(10):
        row = buf._pointer
        assert row == n0 + k
        buf.add_transition(rng.randn(S).astype(np.float32), rng.randn(A).astype(np.float32), float(rng.randn()),
                           rng.randn(S).astype(np.float32), False)
        buf.update_sample_weights(torch.tensor([row], device="cuda"), torch.tensor([new_w[k]], device="cuda"))
    assert buf._index_bound() == n0 + 10 and buf.sample_weights_flags() == 0
    w510 = np.concatenate([w, new_w])
    static = wtd.SampleWeights(w510)
    for s, o in STREAMS:
        got = buf.draw_weighted_indices(N_DRAW, s, o).cpu().numpy()
        assert np.array_equal(got, static.draw_indices(N_DRAW, s, o).cpu().numpy())
        assert np.array_equal(got, W.draw_indices(N_DRAW, w510, s, o))
    # an index at the bound is out of range for the buffer's update
    buf.update_sample_weights(torch.tensor([n0 + 10], device="cuda"), torch.tensor([1.0], device="cuda"))
    assert buf.sample_weights_flags() == 4
    buf.clear_sample_weights_flags()
    assert buf.sample_weights_flags() == 0
    # the weighted training call is not refused, and trains what a static table over the 510 rows trains
    g, e = _build(), _build()
    lg = g.train_steps_weighted(buf, 4, 64, seed=5)
    le = e.train_steps_weighted(buf, 4, 64, seed=5, weights=static)
    assert np.all(np.isfinite(lg)) and np.array_equal(lg, le)
    _same(g, e, "ring growth")


# ---------------------------------------------------------------------------------------------------------------- 8
def test_group_takes_updatable_and_static_tables():
    iql, _, H, wtd = _hip()
    n, steps, B, seeds = 1536, 4, 64, [5, 6]
    buf = _new_buffer(n)
    w = _lognormal(n, seed=3)
    upd, static = wtd.SampleWeights(w, updatable=True), wtd.SampleWeights(w)
    rows = np.arange(64, 192, dtype=np.int64)
    w2 = w.copy()
    w2[rows] = 0.0
    w2[rows[::7]] = 5.0
    upd.update(_dev(rows), _dev(w2[rows]))
    members = [H.build_hip_trainer(synth.synth_params(S, A, seed=300 + i), S, A, True, dict(HYPER), dict(LRS), 1000)
               for i in range(2)]
    twins = [H.build_hip_trainer(synth.synth_params(S, A, seed=300 + i), S, A, True, dict(HYPER), dict(LRS), 1000)
             for i in range(2)]
    got = iql.ImplicitQLearningGroup(members).train_steps_weighted(buf, steps, B, seeds, weights=[upd, static])
    for i, tab in enumerate((upd, static)):
        want = twins[i].train_steps_weighted(buf, steps, B, seed=seeds[i], weights=tab)
        assert np.all(np.isfinite(got[i])) and np.array_equal(got[i], want), i
        _same(members[i], twins[i], f"member {i}")
    # the update took: member 0 on the updated table is member 0 on a static table of the updated weights
    third = H.build_hip_trainer(synth.synth_params(S, A, seed=300), S, A, True, dict(HYPER), dict(LRS), 1000)
    assert np.array_equal(got[0], third.train_steps_weighted(buf, steps, B, seed=seeds[0], weights=wtd.SampleWeights(w2)))
    assert not np.array_equal(got[0], got[1])
