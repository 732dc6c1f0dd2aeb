"""GPU tests of ReplayBuffer.add_transitions and ImplicitQLearning.online_step_vec: E transitions, U
gradient steps and the next actions of E2 states in one library call, against a twin trainer from the same seed that makes
the eager sequence the call stands for — E times `add_transition`, U times `train(sample(B))`, one `actor_forward` —
under the same numpy seed.  Everything compared is compared bitwise.  (S, A) = (3, 2) and (17, 6): row strides of 12 and
44 floats, 3 and 11 float4 per row, so rows straddle the gather's 256-thread blocks."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu

HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
DIMS = [(3, 2), (17, 6)]
SEED = 7          # np.random.seed of every comparison: every iteration of every test draws one of its new rows (asserted in
                  # _run; seed 5 misses one in iteration 7 of the twelve one-row iterations)


def _hip():
    import hip_helpers as H
    import iql
    import iqlhip_binding as hb
    return iql, hb, H


@functools.lru_cache(maxsize=None)
def _params(S, A):
    return synth.synth_params(S, A, seed=31)


@functools.lru_cache(maxsize=None)
def _data(S, A, n=1200):
    d = synth.synth_transitions(n, S, A, seed=32)
    return (d["observations"], d["actions"], d["rewards"].astype(np.float32), d["next_observations"],
            d["terminals"].astype(np.float32))


def _block(S, A, lo, n):
    """Transitions lo .. lo + n - 1 of the stream, as add_transitions / online_step_vec take them."""
    return tuple(x[lo: lo + n] for x in _data(S, A))


def _build(S, A, gaussian=True, bf16=False, stats=False, clip=None, train_mode=True, dropout=0.0, act_dropout=False):
    tr = _hip()[2].build_hip_trainer(_params(S, A), S, A, gaussian, dict(HYPER, deterministic=not gaussian), dict(LRS), 1000,
                                     dropout=dropout)
    if bf16:
        tr.set_precision("bf16")
    tr.set_step_stats(stats)
    tr.set_grad_clip(clip)
    tr.set_act_dropout(act_dropout)
    tr.actor.train(train_mode)
    return tr


def _ring(S, A, cap, prefill=0, lo=1000):
    ring = _hip()[0].ReplayBuffer(S, A, cap, "cuda")
    for e in range(prefill):
        ring.add_transition(*(x[0] for x in _block(S, A, lo + e, 1)))
    return ring


def _add_each(ring, block):
    for e in range(len(block[0])):
        ring.add_transition(block[0][e], block[1][e], float(block[2][e]), block[3][e], bool(block[4][e]))


def _counters(tr):
    hb = _hip()[1]
    out = (C.c_uint64 * 2)()
    hb.check(hb.lib().iqlhip_get_counters(tr._ctx, out))
    return int(out[0]), int(out[1]), tr.act_dropout_calls()


def _same_ring(a, b):
    assert (a._pointer, a._size, a._writes) == (b._pointer, b._size, b._writes)
    assert torch.equal(a._rows, b._rows)


def _new_rows_drawn(cap, size, pointer, E, B, U, iters, seed):
    """Per iteration: whether one of the U * B indices the seeded global stream gives falls into the E new slots."""
    np.random.seed(seed)
    hit = []
    for _ in range(iters):
        size = min(size + E, cap)
        idx = np.concatenate([np.random.randint(0, size, size=B) for _ in range(U)])
        hit.append(bool((((idx - pointer) % cap) < E).any()))
        pointer = (pointer + E) % cap
    return hit


def _run(S, A, E, B, U, iters, cap, prefill=0, E2=None, eager=None, **kw):
    """`iters` fused calls on one trainer against the eager sequence on its twin; returns the fused trainer and results."""
    iql, hb, H = _hip()
    g, t = _build(S, A, **kw), _build(S, A, **kw)
    ring_g, ring_t = _ring(S, A, cap, prefill), _ring(S, A, cap, prefill)
    if U:
        assert all(_new_rows_drawn(cap, ring_g._size, ring_g._pointer, E, B, U, iters, SEED)), "no new row drawn: pick another seed"
    acts = [None if E2 is None else _block(S, A, 500 + 7 * it, E2)[0] for it in range(iters)]
    np.random.seed(SEED)
    got = [g.online_step_vec(ring_g, *_block(S, A, E * it, E), B, updates=U, act_next=acts[it]) for it in range(iters)]
    np.random.seed(SEED)
    for it in range(iters):
        if eager is not None:
            want = eager(t, ring_t, it, acts[it])
            logs, a = ([want[0]], want[1][None, :]) if E2 is not None else ([want], None)
        else:
            _add_each(ring_t, _block(S, A, E * it, E))
            logs = [t.train(ring_t.sample(B)) for _ in range(U)]
            a = None
            if E2 is not None:
                a = t.actor_forward(torch.from_numpy(acts[it]).to("cuda"), sample=t.actor.training).cpu().numpy()
        res_logs, res_a = got[it] if E2 is not None else (got[it], None)
        assert isinstance(res_logs, list) and len(res_logs) == U
        assert res_logs == logs, (it, res_logs, logs)
        assert all(np.isfinite(v) for log in logs for v in log.values())
        if E2 is not None:
            assert res_a.shape == (E2, A) and res_a.dtype == np.float32
            assert np.array_equal(res_a, a), it
    if g.total_it:
        H.assert_same_trainer_state(g, t, "one call vs the eager sequence")
    else:          # (no step has run: the optimizers hold no state to read yet; the arenas are what was loaded)
        assert (g.total_it, g._adam_t) == (t.total_it, t._adam_t) and np.array_equal(H.arenas(g), H.arenas(t))
        assert g.actor_optimizer.param_groups[0]["lr"] == t.actor_optimizer.param_groups[0]["lr"] == LRS["pi"]
    _same_ring(ring_g, ring_t)
    assert _counters(g) == _counters(t)
    return g, t, ring_g, got


# ---- 1. add_transitions alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,A", DIMS)
def test_add_transitions_equals_single_writes_across_the_wrap(S, A):
    iql = _hip()[0]
    a, b = iql.ReplayBuffer(S, A, 8, "cuda"), iql.ReplayBuffer(S, A, 8, "cuda")
    for it in range(5):                      # E = 3: the second call fills to 6, the third wraps mid-call (rows 6, 7, 0)
        blk = _block(S, A, 3 * it, 3)
        a.add_transitions(*blk)
        _add_each(b, blk)
        _same_ring(a, b)
    assert (a._pointer, a._size, a._writes) == (7, 8, 15)
    blk = _block(S, A, 40, 8)                # E = 8: the whole ring, from pointer 7
    a.add_transitions(*blk)
    _add_each(b, blk)
    _same_ring(a, b)
    assert torch.equal(a._rows[7, :S].cpu(), torch.from_numpy(blk[0][0]))


@pytest.mark.parametrize("S,A", DIMS)
def test_add_transitions_with_a_tracking_table(S, A):
    iql = _hip()[0]
    bufs = []
    for vec in (True, False):
        buf = _ring(S, A, 8, prefill=4)
        buf.set_sample_weights(torch.tensor([0.5, 2.5, 1.0, 0.25], device="cuda"), updatable=True, track_max=True)
        for it in range(3):                  # 9 rows: wraps
            blk = _block(S, A, 3 * it, 3)
            buf.add_transitions(*blk) if vec else _add_each(buf, blk)
        bufs.append(buf)
    a, b = bufs
    _same_ring(a, b)
    assert a._weights_version == b._weights_version
    assert a.sample_weights_max() == b.sample_weights_max() and a.sample_weights_max()[1] == 2.5
    import iqlhip_weighted as wtd
    ta, tb = wtd.table_state(a._weights, 8, leaves=True), wtd.table_state(b._weights, 8, leaves=True)
    assert ta[:3] == tb[:3] and np.array_equal(ta[3], tb[3])      # total, flags, version; the leaves
    assert ta[3].min() == ta[3].max() > 0          # nine inserts into eight slots: every row holds the running maximum
    draws = [x.draw_weighted_indices(64, 3, 0) for x in (a, b)]
    assert torch.equal(*draws)


# ---- 2. the fused call against the eager sequence ----------------------------------------------------------------------
@pytest.mark.parametrize("S,A", DIMS)
@pytest.mark.parametrize("U", [0, 1, 3])
@pytest.mark.parametrize("train_mode", [True, False], ids=["sampling", "eval"])
def test_six_iterations_equal_the_eager_sequence(S, A, U, train_mode):
    g, _, ring, got = _run(S, A, E=3, B=16, U=U, iters=6, cap=8, E2=3, train_mode=train_mode)
    assert g.total_it == 6 * U and ring._writes == 18
    assert _counters(g)[1] == (6 if train_mode else 0)          # the act() noise counter: once per call that samples
    if U == 0:
        assert all(logs == [] for logs, _ in got)


# ---- 3. E = 1, U = 1 is online_step(act_next=...) ----------------------------------------------------------------------
@pytest.mark.parametrize("S,A", DIMS)
def test_one_env_one_update_is_online_step(S, A):
    def eager(t, ring, it, act):
        blk = _block(S, A, it, 1)
        return t.online_step(ring, blk[0][0], blk[1][0], float(blk[2][0]), blk[3][0], bool(blk[4][0]), 16, act_next=act[0])
    _run(S, A, E=1, B=16, U=1, iters=12, cap=8, E2=1, eager=eager)


# ---- 4. the step's real tile shape, staging slices beyond the first ----------------------------------------------------
@pytest.mark.parametrize("S,A", DIMS)
def test_full_tile_batches_on_a_larger_ring(S, A):
    _run(S, A, E=8, B=256, U=2, iters=2, cap=1024, prefill=40, E2=5)


# ---- 5. options --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,A", DIMS)
def test_statistics_of_every_step(S, A):
    _, _, _, got = _run(S, A, E=3, B=16, U=3, iters=3, cap=8, stats=True)
    for logs in got:
        assert all(len(log) == 19 for log in logs)
        assert logs[0] != logs[1] and logs[1] != logs[2]          # every dict carries its own step's numbers


@pytest.mark.parametrize("S,A", DIMS)
def test_gradient_clipping(S, A):
    g, t, _, _ = _run(S, A, E=3, B=16, U=3, iters=3, cap=8, clip=1.0, E2=2)
    assert g.last_grad_clip() == t.last_grad_clip()


@pytest.mark.parametrize("S,A", DIMS)
def test_actor_dropout_in_the_steps_and_in_the_act(S, A):
    g, _, _, _ = _run(S, A, E=3, B=16, U=3, iters=3, cap=8, dropout=0.1, act_dropout=True, E2=3)
    assert _counters(g) == (9, 3, 3)          # keep-bit draws: one per step; noise and act keep-bits: one per call


@pytest.mark.parametrize("S,A", DIMS)
def test_bf16(S, A):
    _run(S, A, E=3, B=16, U=3, iters=3, cap=8, bf16=True, E2=3)


# ---- 6. train_steps behind the call ------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,A", DIMS)
def test_train_steps_after_the_call_sees_the_new_rows(S, A):
    iql, hb, H = _hip()
    g, t = _build(S, A), _build(S, A)
    ring_g, ring_t = _ring(S, A, 8, 5), _ring(S, A, 8, 5)
    for tr, ring in ((g, ring_g), (t, ring_t)):
        tr.train_steps(ring, 4, 16, seed=3)          # leaves rows staged for a continuation
    blk = _block(S, A, 0, 3)
    np.random.seed(SEED)
    g.online_step_vec(ring_g, *blk, 16, updates=0)          # no step: only the ring's write count tells
    np.random.seed(SEED)
    _add_each(ring_t, blk)
    la, lb = g.train_steps(ring_g, 4, 16, seed=3), t.train_steps(ring_t, 4, 16, seed=3)
    assert np.array_equal(la, lb)
    fresh = _build(S, A)                              # ... and equal to a trainer that never staged anything ahead
    fresh.train_steps(_ring(S, A, 8, 5), 4, 16, seed=3)
    assert np.array_equal(fresh.train_steps(ring_g, 4, 16, seed=3), la)
    H.assert_same_trainer_state(g, t, "train_steps behind online_step_vec")
    H.assert_same_trainer_state(g, fresh, "a continuation was not taken")


# ---- 7. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    iql, hb, H = _hip()
    S, A, B = 17, 6, 16
    g = _build(S, A, dropout=0.1)
    ring = _ring(S, A, 8, 4)
    blk = _block(S, A, 0, 3)
    act = _block(S, A, 100, 2)[0]

    def state():
        return (g.total_it, dict(g._adam_t), ring._pointer, ring._size, ring._writes, ring._rows.clone(), H.arenas(g),
                _counters(g), np.random.get_state()[1].copy(), np.random.get_state()[2])

    def same(a, b):
        return all(torch.equal(x, y) if isinstance(x, torch.Tensor) else np.array_equal(x, y) for x, y in zip(a, b))

    def refused(exc, *args, **kw):
        s0 = state()
        with pytest.raises(exc):
            g.online_step_vec(*args, **kw)
        assert same(state(), s0)

    np.random.seed(SEED)
    refused(ValueError, ring, *_block(S, A, 0, 9), B)                               # E > capacity
    refused(ValueError, ring, *blk, B, updates=33)
    refused(ValueError, ring, *blk, B, updates=-1)
    refused(ValueError, ring, *blk, 513)
    refused(ValueError, ring, *blk, 0)
    refused(ValueError, ring, blk[0], blk[1][:2], blk[2], blk[3], blk[4], B)         # shapes that disagree
    refused(ValueError, ring, *blk, B, act_next=np.zeros((65, S), dtype=np.float32))
    refused(ValueError, ring, *blk, B, act_next=np.zeros((2, S + 1), dtype=np.float32))
    refused(ValueError, iql.ReplayBuffer(S, A, 8, "cpu"), *blk, B)
    refused(NotImplementedError, ring, *blk, B, act_next=act)                        # a dropout actor without the opt-in
    tracked = _ring(S, A, 8, 4)
    tracked.set_sample_weights(torch.ones(4, device="cuda"), updatable=True, track_max=True)
    refused(NotImplementedError, tracked, *blk, B)
    assert (tracked._pointer, tracked._size, tracked._writes) == (4, 4, 4)
    g.set_precision("bf16")
    refused(NotImplementedError, ring, *blk, 513)
    g.set_precision("f32")
    # the library's own refusals: an index outside the ring, the sizes
    lib, sc, out = hb.lib(), (hb.StepScalars * 2)(), (C.c_float * 6)()
    rows = np.zeros((3, ring._ld), dtype=np.float32)
    idx = np.zeros(2 * B, dtype=np.int64)

    def call(n_rows=3, n_upd=2, rows_b=B, a_rows=0, a_in=None, a_out=None):
        return lib.iqlhip_online_step_vec(g._ctx, ring._rows.data_ptr(), ring._ld, 8, ring._pointer, rows.ctypes.data, n_rows,
                                          idx.ctypes.data, rows_b, n_upd, C.addressof(sc), C.addressof(out), a_in, a_rows, 1.0, 0,
                                          a_out, torch.cuda.current_stream().cuda_stream)
    s0 = state()
    idx[B + 3] = 8
    assert call() == hb.E_INDEX
    idx[B + 3] = 0
    for bad in (dict(n_rows=0), dict(n_rows=9), dict(n_upd=33), dict(n_upd=-1), dict(rows_b=0), dict(rows_b=513),
                dict(a_rows=0, a_in=rows.ctypes.data, a_out=rows.ctypes.data), dict(a_rows=65, a_in=rows.ctypes.data, a_out=rows.ctypes.data),
                dict(a_rows=1, a_in=rows.ctypes.data)):
        assert call(**bad) == hb.E_INVAL, bad
    g.inject_dropout_masks(*(np.ones((B, 256), dtype=np.uint8),) * 2)
    refused(NotImplementedError, ring, *blk, B)
    assert call() == hb.E_UNSUPPORTED
    assert same(state(), s0)
