"""GPU tests of ImplicitQLearning.train_steps_mixed: many steps on batches mixed from two buffers with no
host round trip, against a twin trainer that calls train() on batches gathered from the indices of tests/mixed_ref.py
(the CPU Philox reference) through iqlhip_rows_gather_packed_h into one packed block.  Per-step losses and the final
state are compared bitwise."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import mixed_ref
import synth
from burst_twins import eager_mixed_segment, mixing_ratio as _ratio      # (the twin, shared with the shape table's tests)

pytestmark = pytest.mark.gpu

S, A = 17, 6
HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
N_OFF_ROWS, N_ON_ROWS, ON_CAP = 5000, 37, 64
SPLITS = [(8, 3), (7, 2), (256, 128)]           # (B, n_off); ratio = n_off / B + a little


def _hip():
    import hip_helpers as H
    import iql
    import iqlhip_binding as hb
    return iql, hb, H


@functools.lru_cache(maxsize=None)
def _params():
    return synth.synth_params(S, A, seed=21)


def _new_buffer(n, seed, capacity):
    iql = _hip()[0]
    buf = iql.ReplayBuffer(S, A, capacity, "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in synth.synth_transitions(n, S, A, seed=seed).items()})
    return buf


@functools.lru_cache(maxsize=None)
def _offline():
    return _new_buffer(N_OFF_ROWS, 22, N_OFF_ROWS)


@functools.lru_cache(maxsize=None)
def _online():
    """An online buffer the tests that do not write it share."""
    return _new_buffer(N_ON_ROWS, 24, ON_CAP)


def _build(dropout=0.0, bf16=False, stats=False, clip=None):
    tr = _hip()[2].build_hip_trainer(_params(), S, A, True, dict(HYPER), dict(LRS), 1000, dropout=dropout)
    if dropout:
        tr.set_dropout_seed(11)
    if bf16:
        tr.set_precision("bf16")
    tr.set_step_stats(stats)
    tr.set_grad_clip(clip)
    return tr


def _assert_steps_equal(lg, le, what=""):
    assert np.all(np.isfinite(lg))
    bad = np.nonzero(np.any(lg != le, axis=1))[0]
    assert bad.size == 0, f"{what}: steps {bad.tolist()} differ from the eager twin: {lg[bad[0]]} vs {le[bad[0]]}"


def _case(K, B, n_off, seed=5, **kw):
    H = _hip()[2]
    off, on = _offline(), _online()
    g, e = _build(**kw), _build(**kw)
    lg = g.train_steps_mixed(off, on, K, B, _ratio(B, n_off), seed=seed)
    le = eager_mixed_segment(e, off, on, K, B, n_off, seed)
    _assert_steps_equal(lg, le, f"K={K} B={B} n_off={n_off}")
    H.assert_same_trainer_state(g, e, "mixed vs eager")
    return g, lg


@pytest.mark.parametrize("B,n_off", SPLITS)
@pytest.mark.parametrize("K", [7, 70])
def test_steps_equal_the_eager_twin(K, B, n_off):
    """7 steps: the direct head (4) + the 2- and 1-step chunks; 70: the head (2) + 4 + 64.  B = 7: a step's first index
    alternates between a counter's two word pairs."""
    _, lg = _case(K, B, n_off)
    assert len({tuple(r) for r in lg}) == K                     # every step trained on another batch


@pytest.mark.parametrize("B,n_off", SPLITS)
@pytest.mark.parametrize("K", [7, 70])
def test_with_actor_dropout(K, B, n_off):
    """The same cases with dropout 0.1: the idle blocks stage the next step's two-source rows and its keep-bits."""
    _case(K, B, n_off, dropout=0.1)


def test_bf16_256_rows():
    _case(7, 256, 128, bf16=True)


def test_online_buffer_grows_between_calls():
    """Both sizes are header words of the call: the second call draws over the new size (no recapture: the chunk graphs
    of the first call are replayed) and sees the new rows."""
    H = _hip()[2]
    off = _offline()
    on = _new_buffer(5, 25, ON_CAP)
    g, e = _build(), _build()
    B, n_off, K = 8, 3, 6
    new = synth.synth_transitions(30, S, A, seed=26)
    for call in range(2):
        lg = g.train_steps_mixed(off, on, K, B, _ratio(B, n_off), seed=5)
        if call == 1:
            _, idx_on = mixed_ref.mixed_indices(K, B, n_off, off._size, on._size, 5, mixed_ref.call_offset(e.total_it, B))
            assert idx_on.max() >= 5                            # the call reached rows the first one could not
        le = eager_mixed_segment(e, off, on, K, B, n_off, 5)
        _assert_steps_equal(lg, le, f"call {call}")
        if call == 0:
            for i in range(30):
                on.add_transition(new["observations"][i], new["actions"][i], float(new["rewards"][i]),
                                  new["next_observations"][i], bool(new["terminals"][i]))
            assert on._size == 35
    H.assert_same_trainer_state(g, e, "grown ring")


def test_plain_mixed_plain_on_the_same_buffers():
    """The chunk-graph cache keeps the plain and the mixed kind apart: the segments share the offline rows, B and the
    chunk sizes, so a key without the second rows pointer would replay a plain chunk for a mixed call or the reverse.
    (The trainer offers no continuation across a mixed call; the library's own refusal is the next test's.)"""
    H = _hip()[2]
    off, on = _offline(), _online()
    g, e = _build(), _build()
    B, n_off, K = 8, 3, 8
    for seg in ("plain", "mixed", "plain", "mixed"):
        if seg == "plain":
            lg = g.train_steps(off, K, B, seed=5)
            le = H.eager_segment(e, off, K, B, 5)
        else:
            lg = g.train_steps_mixed(off, on, K, B, _ratio(B, n_off), seed=5)
            le = eager_mixed_segment(e, off, on, K, B, n_off, 5)
        _assert_steps_equal(lg, le, seg)
    H.assert_same_trainer_state(g, e, "plain / mixed / plain / mixed")


def test_the_library_continues_nothing_across_a_mixed_call():
    """Two contexts driven through the C ABI, one passing IQLHIP_TS_CONTINUE to every plain call, one never.  The third
    call is contiguous with the first in everything the library compares (rows, size, B, seed, offset = where the first
    ended, no dropout), so only the mixed call — or the mixed prepare — between them withholds the continuation: were it
    honoured, step 0 would train on the mixed batch the mixed call's last forward staged.  Losses and state are equal."""
    _, hb, H = _hip()
    off, on = _offline(), _online()
    B, n_off, K, seed = 64, 24, 8, 5
    lib = hb.lib()

    def ring(tr, k):
        out = (C.c_float * (3 * k))()
        hb.check(lib.iqlhip_read_loss_ring(tr._ctx, out, k, tr._stream()))
        tr.total_it += k
        return np.frombuffer(out, dtype=np.float32).reshape(k, 3).copy()

    def plain(tr, k, offset, flag):
        tr._prepare(B)
        tab = tr._scalar_table(k, 1.0 / B)
        hb.check(lib.iqlhip_train_steps(tr._ctx, off._rows.data_ptr(), off._ld, off._size, B, tab.ctypes.data, k, seed,
                                        offset, flag, tr._stream()))
        return ring(tr, k)

    def mixed(tr, k, offset):
        tr._prepare(B)
        tab = tr._scalar_table(k, 1.0 / B)
        hb.check(lib.iqlhip_train_steps_mixed(tr._ctx, off._rows.data_ptr(), off._size, on._rows.data_ptr(), on._size,
                                              off._ld, B, n_off, tab.ctypes.data, k, seed, offset, tr._stream()))
        return ring(tr, k)

    for between in ("call", "prepare"):
        runs = []
        for flag in (hb.TS_CONTINUE, 0):
            tr = _build()
            out = [plain(tr, K, 0, flag)]
            if between == "call":
                out.append(mixed(tr, 6, 100000))
            else:
                hb.check(lib.iqlhip_train_steps_mixed_prepare(tr._ctx, off._rows.data_ptr(), on._rows.data_ptr(), off._ld,
                                                              B, n_off, 1.0 / B, tr._stream()))
            out.append(plain(tr, 6, K * B // 2, flag))
            out.append(plain(tr, 6, K * B // 2 + 6 * B // 2, flag))       # (a genuine continuation, honoured with the flag)
            runs.append((tr, np.concatenate(out)))
        (a, la), (n, ln) = runs
        assert np.all(np.isfinite(la)) and np.array_equal(la, ln), between
        H.assert_same_trainer_state(a, n, between)


def test_prepare_trains_nothing_and_the_call_after_it_equals_the_twin():
    """prepare_train_steps_mixed captures and rehearses every two-source chunk graph (arenas saved and restored): the
    parameters, targets and moments are what they were, no counter has moved, and the mixed call that follows — on
    graphs that are all cached by then — equals the eager twin's steps."""
    H = _hip()[2]
    off, on = _offline(), _online()
    B, n_off, K = 8, 3, 70
    for kw in ({}, {"dropout": 0.1}):
        g, e = _build(**kw), _build(**kw)
        before = (g.total_it, dict(g._adam_t), H.arenas(g), g.actor_optimizer.param_groups[0]["lr"])
        g.prepare_train_steps_mixed(off, on, B, _ratio(B, n_off))
        torch.cuda.synchronize()
        assert before[:2] == (g.total_it, dict(g._adam_t)) and before[3] == g.actor_optimizer.param_groups[0]["lr"]
        assert np.array_equal(before[2], H.arenas(g))
        lg = g.train_steps_mixed(off, on, K, B, _ratio(B, n_off), seed=5)
        le = eager_mixed_segment(e, off, on, K, B, n_off, 5)
        _assert_steps_equal(lg, le, f"after prepare {kw}")
        H.assert_same_trainer_state(g, e, "after prepare")


def test_statistics_and_clipping():
    H = _hip()[2]
    off, on = _offline(), _online()
    g, e = _build(stats=True, clip=0.05), _build(stats=True, clip=0.05)
    B, n_off, K = 256, 128, 7
    lg, sg = g.train_steps_mixed(off, on, K, B, _ratio(B, n_off), seed=5, return_stats=True)
    le, se = eager_mixed_segment(e, off, on, K, B, n_off, 5, with_stats=True)
    _assert_steps_equal(lg, le)
    assert sg.shape == (K, 16) and np.array_equal(sg, se)
    H.assert_same_trainer_state(g, e, "stats + clip")
    assert g.last_grad_clip() == e.last_grad_clip()
    with pytest.raises(ValueError):
        _build().train_steps_mixed(off, on, 2, 8, 0.4, return_stats=True)


def test_refusals_move_nothing():
    iql, hb, H = _hip()
    off, on = _offline(), _online()
    g = _build(dropout=0.1)

    def refused(exc, tr=g, B=8, ratio=0.4, off_=off, on_=on):
        before = (tr.total_it, dict(tr._adam_t), H.arenas(tr))
        with pytest.raises(exc):
            tr.train_steps_mixed(off_, on_, 4, B, ratio)
        assert before[:2] == (tr.total_it, dict(tr._adam_t)) and np.array_equal(before[2], H.arenas(tr))

    refused(ValueError, ratio=0.0)
    refused(ValueError, ratio=1.0)
    refused(ValueError, on_=off)
    refused(ValueError, on_=iql.ReplayBuffer(S, A, 8, "cuda"))              # empty online buffer
    refused(ValueError, on_=iql.OfflineReplayBuffer(S, A, 8, "cuda"))
    g.inject_dropout_masks(np.ones((8, 256), dtype=bool), np.ones((8, 256), dtype=bool))
    refused(NotImplementedError)                                             # pending injected masks
    g.set_dropout_seed(11)
    bf = _build(bf16=True)
    refused(NotImplementedError, tr=bf, B=600, ratio=0.5)                    # the large-batch kernels
    assert np.all(np.isfinite(g.train_steps_mixed(off, on, 4, 8, 0.4)))      # ... and it still trains


@pytest.fixture
def gloo_world1():
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(29600 + os.getpid() % 1000)
    dist.init_process_group("gloo", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


def test_data_parallelism_is_refused_before_any_launch(gloo_world1):
    iql, hb, H = _hip()
    off, on = _offline(), _online()
    tr = _build()
    tr.enable_data_parallel(exchange="p2p")
    before = (tr.total_it, dict(tr._adam_t), H.arenas(tr))
    with pytest.raises(NotImplementedError, match="data parallelism"):
        tr.train_steps_mixed(off, on, 4, 8, 0.4)
    ring = iql.ReplayBuffer(S, A, 8, "cuda")
    t = synth.synth_transitions(1, S, A, seed=3)
    with pytest.raises(NotImplementedError, match="data parallelism"):
        tr.online_step_mixed(off, ring, t["observations"][0], t["actions"][0], 0.0, t["next_observations"][0], False, 8, 0.4)
    assert ring._size == 0 and ring._writes == 0
    # the library's own check (what a direct C caller meets)
    tab = np.zeros((4, 12), dtype=np.float32)
    rc = hb.lib().iqlhip_train_steps_mixed(tr._ctx, off._rows.data_ptr(), off._size, on._rows.data_ptr(), on._size, off._ld,
                                           8, 3, tab.ctypes.data, 4, 5, 0, tr._stream())
    assert rc == hb.E_UNSUPPORTED and "data-parallel exchange" in hb.last_error()
    sc, out3 = hb.StepScalars(), (C.c_float * 3)()
    row, idx = np.zeros(ring._ld, dtype=np.float32), np.zeros(4, dtype=np.int64)
    rc = hb.lib().iqlhip_online_step_mixed(tr._ctx, ring._rows.data_ptr(), ring._ld, ring._buffer_size, 0, row.ctypes.data,
                                           idx.ctypes.data, 4, C.byref(sc), out3, None, 1.0, 0, None, tr._stream(),
                                           off._rows.data_ptr(), off._size, idx.ctypes.data, 4)
    assert rc == hb.E_UNSUPPORTED and "data-parallel exchange" in hb.last_error()
    torch.cuda.synchronize()
    assert before[:2] == (tr.total_it, dict(tr._adam_t)) and np.array_equal(before[2], H.arenas(tr))
