"""GPU tests of ImplicitQLearning.online_step_mixed: one library call per online iteration with the batch
mixed from an offline buffer and the online ring, against a twin trainer that makes the four calls it stands for —
`online.add_transition(...)`, `offline.sample(n_off)`, `online.sample(n_on)`, `train(vstack)` — under the same numpy
seed.  Everything compared is compared bitwise."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu

HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
DIMS = [(17, 6), (39, 28)]          # packed strides 44 and 108: 11 and 27 float4 per row
N_OFF_ROWS = 300


def _hip():
    import hip_helpers as H
    import iql
    import iqlhip_binding as hb
    return iql, hb, H


@functools.lru_cache(maxsize=None)
def _params(S, A):
    return synth.synth_params(S, A, seed=21)


@functools.lru_cache(maxsize=None)
def _offline(S, A):
    """The offline buffer: never written by a test, shared by every trainer."""
    iql = _hip()[0]
    buf = iql.ReplayBuffer(S, A, N_OFF_ROWS, "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in synth.synth_transitions(N_OFF_ROWS, S, A, seed=22).items()})
    return buf


@functools.lru_cache(maxsize=None)
def _stream(S, A, n=16):
    d = synth.synth_transitions(n, S, A, seed=23)
    return [(d["observations"][i], d["actions"][i], float(d["rewards"][i]), d["next_observations"][i],
             bool(d["terminals"][i])) for i in range(n)]


def _build(S, A, bf16=False, stats=False, clip=None, train_mode=True):
    tr = _hip()[2].build_hip_trainer(_params(S, A), S, A, True, dict(HYPER), dict(LRS), 1000)
    if bf16:
        tr.set_precision("bf16")
    tr.set_step_stats(stats)
    tr.set_grad_clip(clip)
    tr.actor.train(train_mode)
    return tr


def _ring(S, A, cap, prefill):
    iql = _hip()[0]
    ring = iql.ReplayBuffer(S, A, cap, "cuda")
    for t in _stream(S, A)[8:8 + prefill]:
        ring.add_transition(*t)
    return ring


def _run(S, A, B, ratio=0.5, iters=6, cap=64, prefill=0, act=False, **kw):
    iql, hb, H = _hip()
    import iqlhip_mixed as mixed
    n_off, n_on = mixed.split(B, ratio)
    off = _offline(S, A)
    g, t = _build(S, A, **kw), _build(S, A, **kw)
    ring_g, ring_t = _ring(S, A, cap, prefill), _ring(S, A, cap, prefill)
    stream = _stream(S, A)
    np.random.seed(5)
    got = [g.online_step_mixed(off, ring_g, *stream[it], B, ratio, act_next=stream[it][3] if act else None)
           for it in range(iters)]
    np.random.seed(5)
    for it in range(iters):
        ring_t.add_transition(*stream[it])
        b_off, b_on = off.sample(n_off), ring_t.sample(n_on)
        log = t.train([torch.vstack(pair) for pair in zip(b_off, b_on)])
        if act:
            a = t.act_one(stream[it][3], t.actor.max_action, sample=t.actor.training)
            assert got[it][0] == log, (it, got[it][0], log)
            assert np.array_equal(got[it][1], a), it
        else:
            assert got[it] == log, (it, got[it], log)
        assert all(np.isfinite(v) for v in log.values())
    H.assert_same_trainer_state(g, t, "one call vs four")
    assert (ring_g._pointer, ring_g._size, ring_g._writes) == (ring_t._pointer, ring_t._size, ring_t._writes)
    assert torch.equal(ring_g._rows, ring_t._rows)
    return g, got


@pytest.mark.parametrize("S,A", DIMS)
@pytest.mark.parametrize("B", [8, 256])
def test_six_iterations_equal_the_four_call_sequence(S, A, B):
    """B = 8: one block holds rows of both kinds; B = 256: 11 / 27 blocks, one of which straddles n_off.  The ring is
    empty before the first call: its new size is 1 and every online index equals `pointer` (the pinned row)."""
    g, _ = _run(S, A, B)
    assert g.total_it == 6


@pytest.mark.parametrize("S,A", DIMS)
def test_ring_that_wraps(S, A):
    _run(S, A, 8, ratio=0.4, cap=4, prefill=2)


@pytest.mark.parametrize("S,A", DIMS)
@pytest.mark.parametrize("train_mode", [False, True], ids=["eval", "sampling"])
def test_act_next(S, A, train_mode):
    _, got = _run(S, A, 8, ratio=0.4, act=True, train_mode=train_mode, prefill=3)
    assert got[0][1].shape == (A,)


@pytest.mark.parametrize("S,A", DIMS)
def test_statistics_and_clipping(S, A):
    _, got = _run(S, A, 256, stats=True, prefill=5)
    assert len(got[0]) == 19
    g, _ = _run(S, A, 8, ratio=0.4, clip=0.05, prefill=5)
    assert min(g.last_grad_clip()[k] for k in ("coef_vf", "coef_qf", "coef_actor")) < 1.0      # the limit did clip


def test_bf16():
    _run(39, 28, 256, bf16=True, prefill=5)


def test_refusals_move_nothing():
    iql, hb, H = _hip()
    import iqlhip_mixed as mixed
    S, A, B = 17, 6, 8
    off, g = _offline(S, A), _build(S, A)
    ring = _ring(S, A, 16, 4)
    tr = _stream(S, A)[0]

    def state():
        return (g.total_it, dict(g._adam_t), ring._pointer, ring._size, ring._writes, ring._rows.clone(),
                np.random.get_state()[1].copy(), np.random.get_state()[2])

    def same(a, b):
        return all(torch.equal(x, y) if torch.is_tensor(x) else np.array_equal(x, y) for x, y in zip(a, b))

    def refused(exc, off_=off, ring_=ring, B_=B, ratio=0.5, match=None):
        before = state()
        with pytest.raises(exc, match=match):
            g.online_step_mixed(off_, ring_, *tr, B_, ratio)
        assert same(before, state())

    refused(ValueError, off_=ring, match="distinct")                                   # the same buffer twice
    refused(ValueError, off_=iql.OfflineReplayBuffer(S, A, 16, "cuda"), match="finetune")
    refused(ValueError, ring_=iql.OfflineReplayBuffer(S, A, 16, "cuda"), match="finetune")
    refused(ValueError, ring_=iql.ReplayBuffer(S, A, 16, "cpu"), match="GPU")
    refused(ValueError, off_=iql.ReplayBuffer(S, A, 16, "cpu"), match="GPU")
    refused(ValueError, ring_=iql.ReplayBuffer(S + 1, A, 16, "cuda"), match="state_dim")
    refused(ValueError, off_=iql.ReplayBuffer(S, A, 16, "cuda"), match="empty")        # empty offline buffer
    refused(ValueError, ratio=0.0, match="online_step")
    refused(ValueError, ratio=1.0, match="online_step")
    # a C-level out-of-range index in either array: IndexError before anything is launched (the ring row at `pointer`
    # is not written), through the trainer ...
    good = mixed.draw_host_indices
    for bad_off in (True, False):
        def draw(size_off, n_off, size_on, n_on, bad_off=bad_off):
            io, ion = good(size_off, n_off, size_on, n_on)
            (io if bad_off else ion)[-1] = size_off if bad_off else ring._buffer_size
            return io, ion
        mixed.draw_host_indices = draw
        try:
            before = state()
            with pytest.raises(IndexError):
                g.online_step_mixed(off, ring, *tr, B, 0.5)
            after = state()
            assert same(before[:6], after[:6])
        finally:
            mixed.draw_host_indices = good
    # ... and as a direct caller of the C ABI
    g._prepare(B)
    sc = hb.StepScalars()
    g._fill_scalars(sc, {k: v + 1 for k, v in g._adam_t.items()}, g._current_lrs(), 1.0 / B)
    row = np.zeros(ring._ld, dtype=np.float32)
    out = (C.c_float * 3)()
    for io, ion in (([0, 1, 2, N_OFF_ROWS], [0, 1, 2, 3]), ([0, 1, 2, -1], [0, 1, 2, 3]), ([0, 1, 2, 3], [0, 1, 2, 16]),
                    ([0, 1, 2, 3], [-1, 1, 2, 3])):
        io, ion = np.array(io, dtype=np.int64), np.array(ion, dtype=np.int64)
        before = state()
        rc = hb.lib().iqlhip_online_step_mixed(g._ctx, ring._rows.data_ptr(), ring._ld, ring._buffer_size, ring._pointer,
                                               row.ctypes.data, ion.ctypes.data, 4, C.byref(sc), out, None, 1.0, 0, None,
                                               g._stream(), off._rows.data_ptr(), off._size, io.ctypes.data, 4)
        assert rc == hb.E_INDEX, (io, ion)
        with pytest.raises(IndexError):
            hb.check(rc)
        torch.cuda.synchronize()
        assert same(before, state())
    # the trainer still steps afterwards
    np.random.seed(3)
    log = g.online_step_mixed(off, ring, *tr, B, 0.5)
    assert np.isfinite(log["value_loss"]) and g.total_it == 1 and ring._size == 5
