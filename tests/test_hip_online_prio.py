"""GPU tests of online prioritised replay (DESIGN.md 6j "Online prioritised replay"): tables that track their largest
priority, new rows entering at it (iqlhip_weights_insert_max, ReplayBuffer.add_transition on a tracking table), and
trainer.online_step_prioritized.

Every comparison is integer or bit for bit: the tables against tests/online_prio_ref.py (integers), the tracking
instantiations of the update against the plain ones on a twin table, and the one-call online iteration against the eager
sequence add_transition -> draw_weighted_indices(is_beta) -> train(loss_weights, return_td) -> update_sample_weights_td ->
act written with the public calls on a twin buffer and a twin trainer.  No tolerance is involved."""
import numpy as np
import pytest
import torch

import online_prio_ref as OP
import synth
import weighted_update_ref as U

pytestmark = pytest.mark.gpu

HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
S, A = 17, 6
MAX_WEIGHT = 64.0


def _trainer(dropout=0.0):
    from hip_helpers import build_hip_trainer
    return build_hip_trainer(synth.synth_params(S, A, seed=3, gaussian=True), S, A, True, HYPER, LRS, 1000, dropout=dropout)


def _tr(st, i):
    return (st["observations"][i], st["actions"][i], float(st["rewards"][i]), st["next_observations"][i],
            bool(st["terminals"][i]))


def _state(tab):
    """(leaves, total, flags, version) as the library holds them."""
    import iqlhip_weighted as wtd
    total, flags, version, q = wtd.table_state(tab._table, tab.n, leaves=True)
    return q, total, flags, version


def _buf_state(buf):
    import iqlhip_weighted as wtd
    total, flags, version, q = wtd.table_state(buf._weights, buf.sample_weights_n, leaves=True)
    return q, total, flags, version


def _assert_table_is(tab, ref, what):
    q, total, flags, version = _state(tab)
    assert np.array_equal(q, ref.q), (what, np.nonzero(q != ref.q)[0][:8])
    assert total == ref.total and flags == ref.flags and version == ref.version, (what, total, flags, version)
    assert tab.max_priority() == (ref.q_max, ref.w_max), what
    got = tab.draw_indices(512, 11, 3).cpu().numpy()
    assert np.array_equal(got, ref.draw_indices(512, 11, 3)), what


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("cap", [64, 65, 4097])
def test_insert_max_equals_the_reference(cap):
    """One, two and three levels, the last node of every upper level partial (65 = 64 + 1; 4097 = 64 * 64 + 1)."""
    import iqlhip_weighted as wtd
    rng = np.random.default_rng(cap)
    n = cap - 3                                      # the last three rows weigh 0: inserts into a zero row
    w = rng.uniform(0.01, 1.0, n).astype(np.float32)
    w[0] = 0.0
    tab = wtd.SampleWeights(w, updatable=True, capacity=cap, max_weight=4.0, track_max=True, new_row_weight=2.0)
    ref = OP.TrackingTable(w, capacity=cap, max_weight=4.0, new_row_weight=2.0)
    assert tab.tracks_max and tab.n == cap
    _assert_table_is(tab, ref, "after the build")
    rows = [r for r in (0, 63, 64, cap // 2, cap - 2, cap - 1) if r < cap]
    for r in rows:
        tab.insert_max(r)
        ref.insert_max(r)
        _assert_table_is(tab, ref, f"insert at row {r}")
        assert int(tab.leaves()[r]) == ref.q_max
    tab.insert_max(rows[1])                          # the row already holds q_max: d = 0
    ref.insert_max(rows[1])
    _assert_table_is(tab, ref, "insert over the maximum")
    assert tab.version == ref.version == len(rows) + 1
    # a raised maximum is what the next insert writes
    tab.update(torch.tensor([5], device="cuda"), torch.tensor([3.0], device="cuda"))
    ref.update([5], np.array([3.0], dtype=np.float32))
    tab.insert_max(cap - 1, bound=cap)
    ref.insert_max(cap - 1)
    _assert_table_is(tab, ref, "insert after a raise")
    with pytest.raises(ValueError):
        tab.insert_max(cap)
    with pytest.raises(ValueError):
        tab.insert_max(4, bound=4)
    plain = wtd.SampleWeights(w, updatable=True, capacity=cap, max_weight=4.0)
    assert not plain.tracks_max
    with pytest.raises(ValueError):
        plain.insert_max(0)
    with pytest.raises(ValueError):
        plain.max_priority()


# ------------------------------------------------------------------------------------------------------------------ 2
def test_updates_raise_the_maximum_by_applied_entries_only():
    import iqlhip_weighted as wtd
    cap = 4097
    rng = np.random.default_rng(7)
    w = rng.uniform(0.0, 0.25, cap - 1).astype(np.float32)
    kw = dict(updatable=True, capacity=cap, max_weight=8.0)
    tab = wtd.SampleWeights(w, track_max=True, new_row_weight=0.25, **kw)
    plain = wtd.SampleWeights(w, **kw)
    ref = OP.TrackingTable(w, capacity=cap, max_weight=8.0, new_row_weight=0.25)
    q0 = ref.q_max
    calls = [
        # a duplicate whose losing entry is the larger one; skipped entries that would have raised
        ([3, 3, 70, 4096, 9, 10, 11], [7.0, 0.125, 0.2, 6.0, np.nan, -5.0, np.inf], 4096),
        ([3, 3], [0.125, 0.5], cap),                                         # the other order: raises to q(0.5)
        (rng.integers(0, cap, 700), rng.uniform(0.0, 4.0, 700), cap),        # three blocks of the launch, many duplicates
        ([100], [16.0], cap),                                                # 16 = 2^(e + 1): saturates
        ([100], [0.0], cap),                                                 # ... and the maximum stays
    ]
    seen = [q0]
    for k, (idx, ww, bound) in enumerate(calls):
        idx_t = torch.tensor(np.asarray(idx, dtype=np.int64), device="cuda")
        w_t = torch.tensor(np.asarray(ww, dtype=np.float32), device="cuda")
        tab.update(idx_t, w_t, bound=bound)
        plain.update(idx_t, w_t, bound=bound)
        ref.update(np.asarray(idx, dtype=np.int64), np.asarray(ww, dtype=np.float32), bound)
        _assert_table_is(tab, ref, f"update {k}")
        assert np.array_equal(plain.leaves(), tab.leaves()) and plain.total() == tab.total()
        seen.append(ref.q_max)
    assert seen[1] == q0 and seen[2] > seen[1] and seen[4] == seen[5] == U.Q_SATURATED
    assert tab.flags() == plain.flags() == U.FLAG_NONFINITE | U.FLAG_NEGATIVE | U.FLAG_INDEX


def test_update_td_raises_the_maximum_to_the_largest_applied_priority():
    import iqlhip_weighted as wtd
    cap, m = 4097, 600
    rng = np.random.default_rng(8)
    w = rng.uniform(0.0, 0.01, cap).astype(np.float32)
    kw = dict(updatable=True, max_weight=MAX_WEIGHT)
    tab = wtd.SampleWeights(w, track_max=True, new_row_weight=0.01, **kw)
    plain = wtd.SampleWeights(w, **kw)
    q_max0 = tab.max_priority()[0]
    idx = rng.integers(0, 300, m).astype(np.int64)                           # duplicates throughout
    td = rng.standard_normal((m, 2)).astype(np.float32)
    td[5] = (np.nan, 1e6)                                                    # skipped: raises nothing
    td[6] = (1e30, 0.0)                                                      # the last entry of row 299: saturates
    idx[5], idx[6], idx[7:] = 298, 299, np.minimum(idx[7:], 297)
    idx_t, td_t = torch.tensor(idx, device="cuda"), torch.tensor(td, device="cuda")
    for t in (tab, plain):
        t.update_td(idx_t, td_t, 0.6, 1e-3)
    q, total, flags, version = _state(tab)
    assert np.array_equal(q, plain.leaves()) and total == plain.total() and flags == plain.flags() == U.FLAG_NONFINITE
    applied = np.unique(np.delete(idx, 5))
    assert int(q[299]) == U.Q_SATURATED
    assert tab.max_priority()[0] == max(q_max0, int(q[applied].max())) == U.Q_SATURATED
    # without the saturating entry: the maximum is the largest leaf among the applied rows, nothing more
    tab2 = wtd.SampleWeights(w, track_max=True, new_row_weight=0.01, **kw)
    keep = np.arange(m) != 6
    mask = torch.tensor(keep, device="cuda")
    tab2.update_td(idx_t[mask], td_t[mask], 0.6, 1e-3)
    q2 = tab2.leaves()
    applied2 = np.unique(idx[keep & (np.arange(m) != 5)])
    assert q_max0 < tab2.max_priority()[0] == int(q2[applied2].max()) < U.Q_SATURATED


def _prio_buffer(n, track, w):
    import iql
    buf = iql.ReplayBuffer(S, A, n, "cuda")
    buf.load_d4rl_dataset(synth.synth_transitions(n, S, A, seed=5))
    if track:
        buf.set_sample_weights(w, updatable=True, max_weight=MAX_WEIGHT, track_max=True, new_row_weight=0.01)
    else:
        buf.set_sample_weights(w, updatable=True, max_weight=MAX_WEIGHT)
    return buf


@pytest.mark.parametrize("chunk", [2, 6])
def test_prioritized_burst_on_a_tracking_table(chunk):
    from burst_twins import eager_prioritized_segment
    from hip_helpers import assert_same_trainer_state
    n, B, steps = 2000, 64, 6
    w = np.random.default_rng(4).uniform(0.001, 0.01, n).astype(np.float32)
    burst_buf, eager_buf, plain_buf = _prio_buffer(n, True, w), _prio_buffer(n, True, w), _prio_buffer(n, False, w)
    burst, eager, plain = _trainer(), _trainer(), _trainer()
    q0, total0, _, version0 = _buf_state(burst_buf)
    qm0 = burst_buf.sample_weights_max()
    burst.prepare_train_steps_prioritized(burst_buf, B)                      # the rehearsal: tree and maximum untouched
    q1, total1, flags1, version1 = _buf_state(burst_buf)
    assert np.array_equal(q1, q0) and (total1, flags1, version1) == (total0, 0, version0)
    assert burst_buf.sample_weights_max() == qm0
    lb = burst.train_steps_prioritized(burst_buf, steps, B, seed=9, alpha=0.6, eps=1e-3, is_beta=0.5, chunk=chunk)
    le = eager_prioritized_segment(eager, eager_buf, steps, B, 9, 0.6, 1e-3, 0.5)
    lp = plain.train_steps_prioritized(plain_buf, steps, B, seed=9, alpha=0.6, eps=1e-3, is_beta=0.5, chunk=chunk)
    assert np.array_equal(lb, le) and np.array_equal(lb, lp)
    assert_same_trainer_state(burst, eager, "tracking burst vs eager")
    assert_same_trainer_state(burst, plain, "tracking burst vs the plain table's")
    qb, tb, fb, _ = _buf_state(burst_buf)
    for other in (eager_buf, plain_buf):
        qo, to, fo, _ = _buf_state(other)
        assert np.array_equal(qb, qo) and tb == to and fb == fo == 0
    qm = burst_buf.sample_weights_max()
    assert qm == eager_buf.sample_weights_max()
    # every priority (>= 1e-3 ** 0.6 = 0.0158) is above the weights and new_row_weight (0.01): the maximum has moved, and
    # it is at least the largest leaf (a leaf may have been overwritten by a smaller priority since: >=, not ==)
    assert qm[0] > qm0[0] and qm[0] >= int(qb.max())


# ------------------------------------------------------------------------------------------------------------------ 3
CAP, START, ITERS = 40, 37, 12
ALPHA, EPS, BETA, SEED, OFF0 = 0.6, 1e-3, 0.4, 21, (1 << 32) - 5


def _online_pair(dropout, stats_clip, eval_mode):
    import iql
    out = []
    w = np.random.default_rng(12).uniform(0.004, 0.01, START).astype(np.float32)
    for _ in range(2):
        tr = _trainer(dropout=dropout)
        if dropout:
            tr.set_dropout_seed(77)
        if stats_clip:
            tr.set_step_stats(True)
            tr.set_grad_clip(1.0)
        if eval_mode:
            tr.actor.eval()
        buf = iql.ReplayBuffer(S, A, CAP, "cuda")
        buf.load_d4rl_dataset(synth.synth_transitions(START, S, A, seed=5))
        buf.set_sample_weights(w, updatable=True, max_weight=MAX_WEIGHT, track_max=True, new_row_weight=0.01)
        out.append((tr, buf))
    return out


def _assert_online_state_equal(a, buf_a, b, buf_b, what):
    from hip_helpers import assert_same_trainer_state
    assert_same_trainer_state(a, b, what)
    sa, sb = _buf_state(buf_a), _buf_state(buf_b)
    assert np.array_equal(sa[0], sb[0]), (what, np.nonzero(sa[0] != sb[0])[0])
    assert sa[1:] == sb[1:], (what, sa[1:], sb[1:])                           # total, flags, version
    assert buf_a.sample_weights_max() == buf_b.sample_weights_max(), what
    assert buf_a._weights_version == buf_b._weights_version == sa[3], what
    assert (buf_a._pointer, buf_a._size) == (buf_b._pointer, buf_b._size), what
    assert torch.equal(buf_a._rows, buf_b._rows), what


@pytest.mark.parametrize("B,act,dropout,stats_clip,eval_mode", [
    (32, True, 0.0, False, True),           # act_next in eval mode
    (33, True, 0.0, False, False),          # an odd batch (half a counter per call), act_next sampling
    (32, False, 0.0, True, False),          # statistics and clipping on
    (32, False, 0.1, False, False),         # a dropout actor
])
def test_online_step_prioritized_equals_the_eager_sequence(B, act, dropout, stats_clip, eval_mode):
    (one, buf_one), (eag, buf_eag) = _online_pair(dropout, stats_clip, eval_mode)
    st = synth.synth_transitions(ITERS, S, A, seed=703, antmaze_rewards=True)
    per = (B + 1) // 2
    drew_new_row = 0
    for it in range(ITERS):
        tr = _tr(st, it)
        nxt = tr[3] if act else None
        off = OFF0 + it * per
        # the one call (an explicit offset first, then the buffer's own counter)
        res = one.online_step_prioritized(buf_one, *tr, B, SEED, offset=(off if it == 0 else None), alpha=ALPHA, eps=EPS,
                                          is_beta=BETA, act_next=nxt)
        log_one, a_one = res if act else (res, None)
        assert buf_one._prio_online_offset == off + per
        # the eager sequence
        pointer = buf_eag._pointer
        buf_eag.add_transition(*tr)
        assert int(_buf_state(buf_eag)[0][pointer]) == buf_eag.sample_weights_max()[0]      # the new row sits at the maximum
        idx, c = buf_eag.draw_weighted_indices(B, SEED, off, is_beta=BETA, batch_size=B)
        log_eag = eag.train(buf_eag.gather(idx), loss_weights=c, return_td=True)
        td = eag.last_td_errors()
        buf_eag.update_sample_weights_td(idx, td, ALPHA, EPS)
        a_eag = eag.actor.act(nxt, "cuda") if act else None
        assert log_one == log_eag, (it, log_one, log_eag)
        if stats_clip:
            assert any(k.startswith("stats/") for k in log_one) and one.last_grad_clip() == eag.last_grad_clip()
        if act:
            assert a_one.dtype == a_eag.dtype and np.array_equal(a_one, a_eag), it
        assert torch.equal(one.last_prioritized_indices(), idx), it
        assert torch.equal(one.last_td_errors(), td), it
        drew_new_row += int((idx == pointer).any())
        if it % 4 == 3 or it == ITERS - 1:
            _assert_online_state_equal(one, buf_one, eag, buf_eag, f"iteration {it}")
    assert buf_one._size == CAP and buf_one._pointer == (START + ITERS) % CAP                # filled, wrapped, overwrote
    assert drew_new_row > 0                                                                  # the draw runs behind the insert


# ------------------------------------------------------------------------------------------------------------------ 4
def _moved(tr, buf):
    """What a refused call must leave alone."""
    state = (tr.total_it, dict(tr._adam_t), buf._pointer, buf._size, buf._writes)
    if buf._weights is not None:
        state += (_buf_state(buf)[3], buf._weights_version)
    if buf.sample_weights_track_max:
        state += (buf.sample_weights_max(),)
    return state


def test_refusals_move_nothing():
    import iql
    import iqlhip_weighted as wtd
    st = synth.synth_transitions(1, S, A, seed=704)
    tr_args = _tr(st, 0)
    w = np.random.default_rng(12).uniform(0.004, 0.01, START).astype(np.float32)

    def buffer(**kw):
        buf = iql.ReplayBuffer(S, A, CAP, "cuda")
        buf.load_d4rl_dataset(synth.synth_transitions(START, S, A, seed=5))
        buf.set_sample_weights(w, **kw)
        return buf
    track = dict(updatable=True, max_weight=MAX_WEIGHT, track_max=True, new_row_weight=0.01)
    cases = [
        ("a static table", buffer(), {}, None, ValueError),
        ("an updatable table that does not track", buffer(updatable=True, max_weight=MAX_WEIGHT), {}, None, ValueError),
        ("bf16", buffer(**track), {}, "bf16", NotImplementedError),
        ("alpha = eps = 0", buffer(**track), {"alpha": 0.0, "eps": 0.0}, None, ValueError),
        ("is_beta negative", buffer(**track), {"is_beta": -0.1}, None, ValueError),
    ]
    for what, buf, kw, precision, err in cases:
        tr = _trainer()
        if precision:
            tr.set_precision(precision)
        before = _moved(tr, buf)
        with pytest.raises(err):
            tr.online_step_prioritized(buf, *tr_args, 32, SEED, **kw)
        assert _moved(tr, buf) == before, what
        assert not hasattr(buf, "_prio_online_offset"), what
    # the library's own refusals, reached past the Python layer's
    import ctypes as C
    import iqlhip_binding as hb
    tr, buf = _trainer(), buffer(updatable=True, max_weight=MAX_WEIGHT)
    tr._prepare(32)
    sc, out = hb.StepScalars(), (C.c_float * 3)()
    tr._fill_scalars(sc, {g: t + 1 for g, t in tr._adam_t.items()}, tr._current_lrs(), 1.0 / 32)
    row = np.zeros(buf._ld, dtype=np.float32)

    def raw(table, alpha=0.6, eps=1e-3, beta=0.4):
        return hb.lib().iqlhip_online_step_prioritized(tr._ctx, buf._rows.data_ptr(), buf._ld, buf._buffer_size, buf._pointer,
                                                       row.ctypes.data, 32, C.byref(sc), out, None, 1.0, 0, None, tr._stream(),
                                                       table, SEED, 0, beta, alpha, eps)
    rows_before = buf._rows.clone()
    assert raw(buf._weights) == hb.E_INVAL                                   # not a tracking table
    small = wtd.SampleWeights(w, updatable=True, max_weight=MAX_WEIGHT, track_max=True)      # n = 37, not the capacity
    assert raw(small._table) == hb.E_INVAL
    full = wtd.SampleWeights(w, capacity=CAP, **track)
    state = _state(full), full.max_priority()
    assert raw(full._table, alpha=0.0, eps=0.0) == hb.E_INVAL
    assert raw(full._table, beta=float("nan")) == hb.E_INVAL
    tr.set_precision("bf16")
    assert raw(full._table) == hb.E_UNSUPPORTED
    tr.set_precision("f32")
    after = _state(full), full.max_priority()
    assert np.array_equal(after[0][0], state[0][0]) and after[0][1:] == state[0][1:] and after[1] == state[1]
    assert torch.equal(buf._rows, rows_before) and tr.total_it == 0
    # a tracking table in a group's prioritised call: refused, naming the member, before anything moves
    members = [_trainer(), _trainer()]
    gbuf = iql.ReplayBuffer(S, A, 2000, "cuda")
    gbuf.load_d4rl_dataset(synth.synth_transitions(2000, S, A, seed=5))
    gw = np.random.default_rng(4).uniform(0.001, 0.01, 2000).astype(np.float32)
    tabs = [wtd.SampleWeights(gw, updatable=True, max_weight=MAX_WEIGHT),
            wtd.SampleWeights(gw, updatable=True, max_weight=MAX_WEIGHT, track_max=True, new_row_weight=0.01)]
    before = [(_state(t)[1:], m.total_it, dict(m._adam_t)) for t, m in zip(tabs, members)], tabs[1].max_priority()
    group = iql.ImplicitQLearningGroup(members)
    with pytest.raises(NotImplementedError, match="member 1"):
        group.train_steps_prioritized(gbuf, 2, 64, [1, 2], weights=tabs)
    after = [(_state(t)[1:], m.total_it, dict(m._adam_t)) for t, m in zip(tabs, members)], tabs[1].max_priority()
    assert after == before
