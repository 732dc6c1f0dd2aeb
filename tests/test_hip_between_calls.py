"""GPU tests of what changes BETWEEN two train_steps calls on a live trainer ("What a call keeps for the
next one").  A call replays cached chunk graphs whose kernel arguments were frozen at capture, every step's forward
stages the rows, scalars and keep-bits of the step after it, and an even-length call leaves "step 0 of the next call"
staged.  A missed invalidation does not crash: it trains on the previous rows or the previous beta.

The harness (_run_case).  Three trainers from the same parameters read one GPU ReplayBuffer:
  G  runs train_steps(buf, K, B, seed);
  E  the eager twin, draws the same indices with iqlhip_draw_indices and runs train(buf.gather(...)) step by step
     (iqlhip_step: no graph, nothing staged ahead, no continuation — independent of everything under test);
  U  G's schedule without the in-between event.
A case is three calls with an event applied to G and E between the first and the second and taken back between the
second and the third (graphs cached before the event get reused after it).  Asserted, all bitwise: (a) every step's
three losses G == E; (b) parameters, targets and Adam moments at the end; (c) the actor learning rate; (d) the event
mattered — the call after it differs from U's in at least one loss, so that no case passes because the change never
reached the library.  The call in front of an event has an even number of steps, at least 6: it ends with a valid
continuation and has replayed (and cached) a 4- or 16-step chunk graph, so a missed invalidation has something stale
to use.  No tolerance anywhere."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import synth
from helpers import (GRAPH_CACHE_ENTRIES, SMALL_BUFFER, graph_cache_requests, step_batch, train_steps_graph_keys,
                     uses_large_batch_kernels)

pytestmark = pytest.mark.gpu

S, A, N = 17, 6, 5000
HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
SEGS = [(8, 256, 5), (6, 256, 5), (8, 256, 5)]      # one seed: the second and third call are offered as continuations


def _hip():
    import hip_helpers as H
    import iql
    import iqlhip_binding as hb
    return iql, hb, H


@functools.lru_cache(maxsize=None)
def _params(seed=21):
    return synth.synth_params(S, A, seed=seed)


def _new_buffer(n, seed, capacity=None):
    iql = _hip()[0]
    buf = iql.ReplayBuffer(S, A, capacity or n, "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in synth.synth_transitions(n, S, A, seed=seed).items()})
    return buf


@functools.lru_cache(maxsize=None)
def _buffer(seed=22):
    """A 5 000-row buffer shared by the cases that never write it."""
    return _new_buffer(N, seed)


def _build(max_steps=1000, dropout=0.0, hyper=HYPER, lrs=LRS, params=None):
    tr = _hip()[2].build_hip_trainer(params or _params(), S, A, True, dict(hyper), dict(lrs), max_steps, dropout=dropout)
    if dropout:
        tr.set_dropout_seed(11)
    return tr


def _each(fn):
    """An event that does the same to G and to E."""
    return lambda trainers: [fn(t) for t in trainers]


def _set(name, value):
    return _each(lambda t: setattr(t, name, value))


def _run_case(segments, event, revert, *, make=_build, setup=None, bufs=None, u_segments=None, u_bufs=None,
              mattered=(1,)):
    """The harness of the module docstring; returns (G, E, U, G's losses per call)."""
    H = _hip()[2]
    g, e, u = make(), make(), make()
    for t in (g, e, u):
        if setup:
            setup(t)
    bufs = bufs or [_buffer()] * len(segments)
    u_bufs = u_bufs or [bufs[0]] * len(segments)
    u_segments = u_segments or segments
    out = []
    for i, (K, B, seed) in enumerate(segments):
        if i == 1:
            assert K >= 1 and segments[0][0] % 2 == 0 and segments[0][0] >= 6
            event((g, e))
        if i == 2 and revert is not None:
            revert((g, e))
        lg = g.train_steps(bufs[i], K, B, seed=seed)
        le = H.eager_segment(e, bufs[i], K, B, seed)
        assert np.all(np.isfinite(lg))
        bad = np.nonzero(np.any(lg != le, axis=1))[0]
        assert bad.size == 0, f"call {i}: steps {bad.tolist()} differ from the eager twin: {lg[bad[0]]} vs {le[bad[0]]}"   # (a)
        lu = u.train_steps(u_bufs[i], *u_segments[i])
        if i in mattered:
            assert not np.array_equal(lg, lu), f"call {i}: the event changed no loss"                                   # (d)
        out.append(lg)
    H.assert_same_trainer_state(g, e, "G vs E")                                                                          # (b), (c)
    return g, e, u, out


# ------------------------------------------------------------------------------------------------ 1. hyper-parameters
@pytest.mark.parametrize("name,value", [("beta", 5.0), ("iql_tau", 0.9), ("discount", 0.9), ("tau", 0.05)])
def test_hyper_parameter_changed_between_calls(name, value):
    """_hyper_sent -> iqlhip_set_hyper -> drop_graph: the chunks captured with the old value (beta, iql_tau and discount
    are kernel arguments of the forward / backward, tau of the update kernel) must not be replayed, and are captured
    again when the value returns."""
    _run_case(SEGS, _set(name, value), _set(name, HYPER[name]))


# ------------------------------------------------------------------------------------------------ 2. learning rates
def _lr(which, value):
    def f(t):
        getattr(t, which).param_groups[0]["lr"] = value
    return _each(f)


@pytest.mark.parametrize("which", ["v_optimizer", "q_optimizer", "actor_optimizer"])
def test_learning_rate_changed_between_calls(which):
    """The look-ahead scalar table (_table_cache) was computed for the old rate while the GPU ran the previous call."""
    _run_case(SEGS, _lr(which, 1e-3), _lr(which, 3e-4))


def test_cosine_schedule_crosses_its_end_inside_a_call():
    """max_steps = 40: the second call (steps 37 .. 44) walks over the schedule's end, in the look-ahead table as in
    the eager scheduler; a critic's rate changes in front of it."""
    g, e, _, _ = _run_case([(36, 256, 5), (8, 256, 5), (8, 256, 5)], _lr("q_optimizer", 1e-3), _lr("q_optimizer", 3e-4),
                           make=lambda: _build(max_steps=40))
    assert g.actor_lr_schedule.last_epoch == 52 and g.actor_optimizer.param_groups[0]["lr"] > 0.0


def test_learning_rate_changed_without_a_schedule():
    g, _, _, _ = _run_case(SEGS, _lr("actor_optimizer", 1e-3), _lr("actor_optimizer", 3e-4),
                           make=lambda: _build(max_steps=None))
    assert g.actor_lr_schedule is None and g.actor_optimizer.param_groups[0]["lr"] == 3e-4


# ------------------------------------------------------------------------------------------------ 3. actor dropout
DROP_SEGS = [(8, 100, 5), (6, 100, 5), (8, 100, 5)]          # 100 rows: ragged, no multiple of 32


def test_actor_eval_then_train_between_calls():
    """actor.eval() sends rate 0 (GraphKey.drop_p changes, and back); the keep-bit position carries on behind the
    evaluation-mode steps where eager steps leave it — they draw nothing and do not move it."""
    g, e, _, _ = _run_case(DROP_SEGS, _each(lambda t: t.actor.eval()), _each(lambda t: t.actor.train()),
                           make=lambda: _build(dropout=0.1))
    ctr = (C.c_uint64 * 2)()
    _, hb, _ = _hip()
    hb.check(hb.lib().iqlhip_get_counters(g._ctx, ctr))
    assert ctr[0] == 16          # the 8 + 8 steps that drew


def test_dropout_seed_changed_between_calls():
    """The key travels in the call's header, not in GraphKey: the cached chunks are replayed with the new key, and the
    continuation record (which compares it) must not hand over keep-bits drawn under the old one."""
    def reseed(seed):
        return _each(lambda t: t.set_dropout_seed(seed))
    _run_case(DROP_SEGS, reseed(12), reseed(11), make=lambda: _build(dropout=0.1))


# ------------------------------------------------------------------------------------------------ 4. precision
def _precision(mode):
    return _each(lambda t: t.set_precision(mode))


def test_precision_changed_between_calls():
    _run_case(SEGS, _precision("bf16"), _precision("f32"))


def test_bf16_across_the_large_batch_threshold_and_back():
    """256 -> 600 -> 256 rows in bf16 on one context (scratch reserved up front): the small-batch chunks cached by the
    first call are replayed by the third, behind steps of the large-batch kernels that used the same scratch."""
    assert uses_large_batch_kernels(S, A, 600) and not uses_large_batch_kernels(S, A, 256)

    def setup(t):
        t.reserve_batch(768)
        t.set_precision("bf16")
    _run_case([(8, 256, 5), (6, 600, 5), (8, 256, 5)], lambda trainers: None, None, setup=setup, u_segments=SEGS)


# ------------------------------------------------------------------------------------------------ 5. batch size, buffer
def test_batch_size_changed_between_calls():
    _run_case([(8, 256, 5), (6, 33, 5), (8, 256, 5)], lambda trainers: None, None, u_segments=SEGS)


def test_batch_grows_past_max_batch_between_calls():
    """700 rows: _attach re-creates the context (new scratch, empty graph cache, counters carried over)."""
    g, _, u, _ = _run_case([(8, 256, 5), (6, 700, 5), (8, 256, 5)], lambda trainers: None, None, u_segments=SEGS)
    assert g._max_batch == 768 and u._max_batch == 256


def test_second_buffer_between_calls():
    """GraphKey.rows: the idle-work records of a cached chunk point at the buffer it was captured for."""
    a, b = _buffer(22), _buffer(23)
    assert a._rows.data_ptr() != b._rows.data_ptr() and a._rows.shape == b._rows.shape
    _run_case(SEGS, lambda trainers: None, None, bufs=[a, b, a])


# ------------------------------------------------------------------------------------------------ 6. rows written
def _small_buffer():
    """40 rows in a ring of 40, its pointer back at row 0 (39 loaded, one added)."""
    n = SMALL_BUFFER["N"]
    buf = _new_buffer(n - 1, 31, capacity=n)
    d = synth.synth_transitions(1, S, A, seed=32)
    buf.add_transition(d["observations"][0], d["actions"][0], float(d["rewards"][0]), d["next_observations"][0], False)
    assert buf._size == n and buf._pointer == SMALL_BUFFER["pointer_row"]
    return buf


def _write_add(buf):
    d = synth.synth_transitions(1, S, A, seed=33)
    buf.add_transition(d["observations"][0], d["actions"][0], 2.5, d["next_observations"][0], True)
    return [SMALL_BUFFER["pointer_row"]]


def _write_reward_view(buf):
    buf._rewards[SMALL_BUFFER["reward_row"]] = 7.5
    return [SMALL_BUFFER["reward_row"]]


def _write_copy(buf):
    buf._rows.copy_(_new_buffer(SMALL_BUFFER["N"], 34)._rows)           # the same address, new content


def _write_normalize(buf):
    buf.normalize_states_(np.full(S, 0.25, dtype=np.float32), np.full(S, 1.5, dtype=np.float32))


def _write_modify_reward(buf):
    assert buf.modify_reward_("hopper-medium-v2", max_episode_steps=10)["max_episode_steps"] == 10


def _write_fill_synthetic(buf):
    buf._size = buf._pointer = 0           # (fill_synthetic loads an empty buffer, like load_d4rl_dataset)
    buf.fill_synthetic(SMALL_BUFFER["N"], seed=9)


@pytest.mark.parametrize("writer", [_write_add, _write_reward_view, _write_copy, _write_normalize, _write_modify_reward,
                                    _write_fill_synthetic], ids=lambda f: f.__name__[7:])
def test_rows_written_between_calls(writer):
    """Every writer of the replay rows, between two even-length calls on a 40-row buffer (each 256-row batch holds
    almost every row): the rows the previous call staged for "the next step" are stale, the shim's token (the buffer's
    write count and the row tensor's version) must withhold IQLHIP_TS_CONTINUE."""
    H = _hip()[2]
    c = SMALL_BUFFER
    buf, buf_u = _small_buffer(), _small_buffer()
    assert torch.equal(buf._rows, buf_u._rows)
    saved = buf._rows.clone()
    segs = [(k, c["B"], c["seed"]) for k in c["segments"]]

    def event(trainers):
        g = trainers[0]
        rows = writer(buf)
        # a condition of the test: what was written is in the first batch of the next call (the CPU companion checks the
        # same from the CPU index draw)
        first = set(H.draw_indices(c["B"], buf._index_bound(), c["seed"], g.total_it * ((c["B"] + 1) // 2)).tolist())
        if rows is None:            # a writer of every row
            assert len(first) >= c["N"] - 2
        else:
            assert all(r in first for r in rows), (rows, sorted(first))
        assert not torch.equal(buf._rows, saved)

    _run_case(segs, event, lambda trainers: buf._rows.copy_(saved), bufs=[buf] * 3, u_bufs=[buf_u] * 3)
    assert torch.equal(buf_u._rows, saved)


# ------------------------------------------------------------------------------------------------ 6b. the library's checks
class _Twin:
    """A context driven through the C ABI, with IQLHIP_TS_CONTINUE always (flag = 1) or never (0) passed."""

    def __init__(self, flag, dropout):
        iql, hb, H = _hip()
        self.flag, self.hb, self.H = flag, hb, H
        self.tr = _build(dropout=dropout)
        self.buf = _new_buffer(N, 41, capacity=N + 8)          # (room for the online step's transition)
        self.partner = _build(dropout=dropout, params=_params(51))
        self.group = iql.ImplicitQLearningGroup([self.tr, self.partner], actor_dropout=dropout > 0)

    def ts(self, K, B, seed, offset):
        tr, hb, buf = self.tr, self.hb, self.buf
        tr._prepare(B)
        tab = tr._scalar_table(K, 1.0 / B)
        hb.check(hb.lib().iqlhip_train_steps(tr._ctx, buf._rows.data_ptr(), buf._ld, buf._index_bound(), B, tab.ctypes.data,
                                             K, seed, offset, self.flag, tr._stream()))
        tr.total_it += K
        out = (C.c_float * (3 * K))()
        hb.check(hb.lib().iqlhip_read_loss_ring(tr._ctx, out, K, tr._stream()))
        return np.frombuffer(out, dtype=np.float32).reshape(K, 3).copy()

    def split_step(self, batch):
        """iqlhip_forward_backward + iqlhip_apply_update."""
        tr, hb = self.tr, self.hb
        b, keep, B = tr._batch_struct(batch)
        tr._prepare(B)
        for g in tr._adam_t:
            tr._adam_t[g] += 1
        sc = hb.StepScalars()
        tr._fill_scalars(sc, tr._adam_t, tr._current_lrs(), 1.0 / B)
        flat = tr._dp_flat()
        hb.check(hb.lib().iqlhip_forward_backward(tr._ctx, C.byref(b), C.byref(sc), flat.data_ptr(), tr._stream()))
        hb.check(hb.lib().iqlhip_apply_update(tr._ctx, flat.data_ptr(), C.byref(sc), tr._stream()))
        tr.total_it += 1
        tr._advance_schedule(1)


@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_results_are_identical_with_and_without_the_continue_flag(dropout):
    """include/iqlhip.h: "Results are identical with and without the flag" — the library itself checks that a call
    continues the previous one.  Twin contexts, one always passing IQLHIP_TS_CONTINUE, one never, through boundaries
    at which the flag must be ignored (and one genuinely contiguous boundary at which it is honoured).  Without dropout
    too: with it, every entry point that draws also moves the keep-bit position the record compares, which would hide
    a missing `cont.valid = false`."""
    _, hb, H = _hip()
    B = 64
    a, n = _Twin(hb.TS_CONTINUE, dropout), _Twin(0, dropout)
    batch = H.to_torch_batch(step_batch(S, A, B, seed=61))
    other = H.to_torch_batch(step_batch(S, A, B, seed=62))
    tr_row = synth.synth_transitions(1, S, A, seed=63)

    def online(t):
        np.random.seed(64)
        t.tr.online_step(t.buf, tr_row["observations"][0], tr_row["actions"][0], 1.5, tr_row["next_observations"][0],
                         False, B)

    def rate(p):
        def f(t):
            for m in t.tr.actor.modules():
                if isinstance(m, torch.nn.Dropout):
                    m.p = p
        return f

    # (what happens in front of the call, K, B, seed, offset or None = where the previous call ended)
    plan = [("first call", None, 8, B, 5, 0),
            ("contiguous: the flag is honoured", None, 6, B, 5, None),
            ("changed seed", None, 6, B, 6, None),
            ("offset not where the previous call ended", None, 6, B, 6, 5000),
            ("contiguous again, odd number of steps", None, 5, B, 6, None),
            ("after an odd number of steps", None, 6, B, 6, None),
            ("odd K * B", None, 3, 33, 6, 9000),
            ("after an odd K * B", None, 6, 33, 6, 9000 + 50),
            ("even again", None, 8, B, 7, 20000),
            ("iqlhip_step in between", lambda t: t.tr.train(batch), 6, B, 7, None),
            ("iqlhip_online_step in between", online, 6, B, 7, None),
            ("forward_backward + apply_update in between", lambda t: t.split_step(batch), 6, B, 7, None),
            ("iqlhip_debug_time_kernel in between", lambda t: t.tr.time_kernel(batch, 0, repeat=2), 6, B, 7, None),
            ("iqlhip_train_steps_prepare in between", lambda t: t.tr.prepare_train_steps(t.buf, B), 6, B, 7, None),
            ("another dropout rate", rate(0.2), 6, B, 7, None),
            ("another dropout seed", lambda t: t.tr.set_dropout_seed(13), 6, B, 7, None),
            ("a group call that contains the context", lambda t: t.group.train([batch, other]), 6, B, 7, None),
            ("contiguous at the end", None, 8, B, 7, None)]
    if not dropout:
        plan = [p for p in plan if "dropout" not in p[0]]
    nxt = 0
    for what, between, K, rows, seed, offset in plan:
        offset = nxt if offset is None else offset
        got = []
        for t in (a, n):
            if between is not None:
                between(t)
            got.append(t.ts(K, rows, seed, offset))
        assert np.all(np.isfinite(got[0])), what
        assert np.array_equal(got[0], got[1]), (what, got[0], got[1])
        assert np.array_equal(H.arenas(a.tr), H.arenas(n.tr)), what
        nxt = offset + (K * rows + 1) // 2
    assert torch.equal(a.buf._rows, n.buf._rows)
    H.assert_same_trainer_state(a.tr, n.tr, "flag always vs never")


KINDS = ("plain", "mixed", "weighted", "weighted_is", "prioritized")


class _KindTwin:
    """One trainer driven through the C ABI by all five kinds of multi-step call: one offline buffer whose updatable
    table the three weighted kinds share (it spans the buffer: plain and weighted calls name the same size), one online
    buffer for the mixed calls."""
    N, B, K, IS_BETA, ALPHA, EPS = 300, 8, 2, 0.5, 0.6, 1e-3

    def __init__(self):
        self.tr = _build()
        self.buf, self.online = _new_buffer(self.N, 41), _new_buffer(self.N, 42)
        w = np.random.RandomState(2).rand(self.N).astype(np.float32) ** 4 + np.float32(1e-3)       # skewed
        self.buf.set_sample_weights(w, updatable=True, max_weight=64.0)

    def call(self, kind, seed, flag):
        """K steps of `kind` at the trainer's position in the index stream; returns their losses."""
        _, hb, _ = _hip()
        tr, buf, lib, B, K = self.tr, self.buf, hb.lib(), self.B, self.K
        tr._prepare(B)
        tab = tr._scalar_table(K, 1.0 / B)
        off = tr.total_it * (B // 2)
        head = (tr._ctx, buf._rows.data_ptr(), buf._ld, self.N, B, tab.ctypes.data, K, seed, off, flag, tr._stream())
        if kind == "plain":
            hb.check(lib.iqlhip_train_steps(*head))
        elif kind == "mixed":              # (no flags argument: a mixed call never continues)
            hb.check(lib.iqlhip_train_steps_mixed(tr._ctx, buf._rows.data_ptr(), self.N, self.online._rows.data_ptr(), self.N,
                                                  buf._ld, B, B // 2, tab.ctypes.data, K, seed, off, tr._stream()))
        elif kind == "weighted":
            hb.check(lib.iqlhip_train_steps_weighted(*head, buf._weights))
        elif kind == "weighted_is":
            hb.check(lib.iqlhip_train_steps_weighted_is(*head, buf._weights, self.IS_BETA))
        else:
            hb.check(lib.iqlhip_train_steps_prioritized(*head, buf._weights, self.IS_BETA, self.ALPHA, self.EPS))
        out = (C.c_float * (3 * K))()
        hb.check(lib.iqlhip_read_loss_ring(tr._ctx, out, K, tr._stream()))
        tr.total_it += K
        return np.frombuffer(out, dtype=np.float32).reshape(K, 3).copy()


def test_every_pair_of_kinds_continues_only_its_own():
    """Every ordered pair (first, second) of the five kinds of multi-step call, two steps each at 8 rows, through the C
    ABI with IQLHIP_TS_CONTINUE on every call.  The second call is contiguous with the first in everything the token
    compares (rows, stride, size, batch, seed, counter position, no dropout), so only the library's knowledge of the
    KIND decides whether it starts on the rows the first one staged.  The twin makes the same calls with the flag only
    where include/iqlhip.h documents a continuation: first == second, and not the mixed kind (prioritised ->
    prioritised is one: the first call's own version bump is in its token).  Second call's losses and the trainer
    state, bit for bit.  Each pair has a seed of its own, so no first call continues the pair before it."""
    _, hb, H = _hip()
    a, t = _KindTwin(), _KindTwin()
    assert a.buf._index_bound() == a.N == a.buf.sample_weights_n
    pair = 0
    for first in KINDS:
        for second in KINDS:
            seed = 100 + pair
            pair += 1
            documented = hb.TS_CONTINUE if (first == second and first != "mixed") else 0
            fa, ft = a.call(first, seed, hb.TS_CONTINUE), t.call(first, seed, 0)
            sa, st = a.call(second, seed, hb.TS_CONTINUE), t.call(second, seed, documented)
            assert np.all(np.isfinite(sa)), (first, second)
            assert np.array_equal(fa, ft), (first, second, fa, ft)
            assert np.array_equal(sa, st), (first, second, sa, st)
            assert np.array_equal(H.arenas(a.tr), H.arenas(t.tr)), (first, second)
    H.assert_same_trainer_state(a.tr, t.tr, "flag always vs where documented")


# ------------------------------------------------------------------------------------------------ 7. injected masks
def test_train_steps_refuses_pending_injected_masks():
    """iqlhip_train_steps draws its own keep-bits (two halves, the next step's drawn by the step before) and cannot use
    masks written by iqlhip_debug_write_masks: it refuses, IQLHIP_EUNSUPPORTED, before anything is launched or any
    counter moves; iqlhip_set_dropout clears the masks and the refusal."""
    _, hb, H = _hip()
    B, buf = 256, _buffer()
    tr, twin = _build(dropout=0.1), _build(dropout=0.1)
    first = H.to_torch_batch(step_batch(S, A, B, seed=71))
    assert tr.train(first) == twin.train(first)
    k0, k1 = synth.synth_dropout_keep(B, 0.1, seed=72)
    tr.inject_dropout_masks(k0, k1)

    def snapshot():
        ctr = (C.c_uint64 * 2)()
        hb.check(hb.lib().iqlhip_get_counters(tr._ctx, ctr))
        return (H.arenas(tr), (int(ctr[0]), int(ctr[1])), tr.total_it, dict(tr._adam_t), tr._schedule_state())
    before = snapshot()
    with pytest.raises(NotImplementedError):
        tr.train_steps(buf, 6, B, seed=5)
    with pytest.raises(NotImplementedError):
        tr.prepare_train_steps(buf, B)
    # ... and the library itself, called past the shim's check
    tab = tr._build_table(6, 1.0 / B, tr._adam_t, np.full(6, 3e-4))
    rc = hb.lib().iqlhip_train_steps(tr._ctx, buf._rows.data_ptr(), buf._ld, N, B, tab.ctypes.data, 6, 5, tr.total_it * 128,
                                     0, tr._stream())
    assert rc == hb.E_UNSUPPORTED and "iqlhip_debug_write_masks" in hb.last_error()
    assert hb.lib().iqlhip_train_steps_prepare(tr._ctx, buf._rows.data_ptr(), buf._ld, B, 1.0 / B,
                                               tr._stream()) == hb.E_UNSUPPORTED
    after = snapshot()
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:] and after[1][0] == 1
    # cleared by iqlhip_set_dropout (sent again by the shim when the key is set): the call runs, and draws what a trainer
    # that never held injected masks draws
    tr.set_dropout_seed(11)
    got = tr.train_steps(buf, 6, B, seed=5)
    assert np.array_equal(got, twin.train_steps(buf, 6, B, seed=5))
    H.assert_same_trainer_state(tr, twin)


# ------------------------------------------------------------------------------------------------ 8. inference, edits
def test_inference_between_calls_keeps_the_staged_rows():
    """actor.act, a 4 096-row actor_forward (more rows than max_batch) and iqlhip_actor_sample between two even-length
    calls: the second call continues on the rows the first one staged (nothing wrote the buffer: the flag is passed and
    honoured) and the two equal one call of the summed length."""
    H = _hip()[2]
    buf = _buffer()
    g, u = _build(), _build()
    l1 = g.train_steps(buf, 8, 256, seed=5)
    states = torch.from_numpy(synth.synth_transitions(4096, S, A, seed=81)["observations"]).cuda()
    assert states.shape[0] > g._max_batch
    assert g.actor.act(states[0].cpu().numpy(), "cuda").shape == (A,)
    assert g.actor_forward(states).shape == (4096, A)
    assert g.actor_forward(states[:100], sample=True).shape == (100, A)
    l2 = g.train_steps(buf, 6, 256, seed=5)
    lu = u.train_steps(buf, 14, 256, seed=5)
    assert np.array_equal(np.concatenate([l1, l2]), lu)
    H.assert_same_trainer_state(g, u)


def _linear1(mod):
    return [m for m in mod.modules() if isinstance(m, torch.nn.Linear)][1]


def _edit_qf(g, ckpt):
    with torch.no_grad():
        _linear1(g.qf.q1).weight[5, 7] += 0.25


def _edit_target(g, ckpt):
    with torch.no_grad():
        _linear1(g.q_target.q2).weight[9, 3] += 0.25


def _load_checkpoint(g, ckpt):
    g.load_state_dict(ckpt)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("event", [_load_checkpoint, _edit_qf, _edit_target], ids=lambda f: f.__name__.strip("_"))
def test_parameters_written_from_outside_between_calls(event, precision):
    """load_state_dict of an earlier checkpoint, an in-place edit of a critic weight, and one of a TARGET weight: the
    next call equals a fresh trainer built from that state with the same counters and schedule.  In bf16 the library
    keeps shadows of both arenas; every call rebuilds them from the fp32 masters (the target edit catches a refresh
    that forgets the target's)."""
    H = _hip()[2]
    buf = _buffer()
    g, u = _build(), _build()
    for t in (g, u):
        t.set_precision(precision)
    g.train_steps(buf, 8, 256, seed=5)
    ckpt = copy.deepcopy(g.state_dict())
    g.train_steps(buf, 6, 256, seed=5)
    event(g, ckpt)
    state = H.read_params(g)
    f = _build(params=state)
    f.set_precision(precision)
    f.load_state_dict(copy.deepcopy(g.state_dict()))           # moments, step counts, schedule (resets the target ...)
    H._load_mlp(f.q_target.q1, state["qt1"])                   # (... which is g's, not a copy of its critics)
    H._load_mlp(f.q_target.q2, state["qt2"])
    H.assert_same_trainer_state(g, f, "fresh trainer")
    lg = g.train_steps(buf, 8, 256, seed=5)
    lf = f.train_steps(buf, 8, 256, seed=5)
    assert np.all(np.isfinite(lg)) and np.array_equal(lg, lf), (lg, lf)
    H.assert_same_trainer_state(g, f, "after the call")
    u.train_steps(buf, 14, 256, seed=5)
    assert not np.array_equal(lg, u.train_steps(buf, 8, 256, seed=5))            # the event mattered


# ------------------------------------------------------------------------------------------------ 9. cache eviction
def test_graph_cache_eviction_under_calls_in_flight():
    """Five batch sizes at 23 steps (a head of 2, then chunks of 4, 16 and 1: four cache entries each) cycled three
    times: 20 distinct keys against 12 entries, so from the fourth call on every chunk request evicts the least recently
    used entry — with return_losses=False no host synchronisation separates the calls, and the evicted graph may still
    be executing.  Equal to eager steps at the end, and per step in the last round."""
    H = _hip()[2]
    buf = _buffer()
    sizes, K, rounds = (32, 64, 96, 128, 160), 23, 3
    calls = [train_steps_graph_keys(K, B, rows=buf._rows.data_ptr()) for _ in range(rounds) for B in sizes]
    distinct, evictions = graph_cache_requests(calls)
    assert distinct > GRAPH_CACHE_ENTRIES and evictions >= 2 * distinct
    g, e = _build(), _build()
    last = []
    for r in range(rounds):
        for B in sizes:
            out = g.train_steps(buf, K, B, seed=5, return_losses=(r == rounds - 1))
            if out is not None:
                last.append(out)
    want = [H.eager_segment(e, buf, K, B, 5) for _ in range(rounds) for B in sizes]
    for got, ref, B in zip(last, want[-len(sizes):], sizes):
        assert np.array_equal(got, ref), B
    H.assert_same_trainer_state(g, e)
