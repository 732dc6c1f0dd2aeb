"""CPU tests of the variance learner's replay-buffer windows (DESIGN.md 6l "From a replay buffer"): the numpy restatement
of the window packing (tests/variance_window_ref.py) against pack_block on the same rows, the burst's start rows against
oracle/philox_ref.py and against big-integer arithmetic on the scalar generator, and the new C ABI's declarations."""
import os
import re

import numpy as np
import pytest

import iqlhip_binding as hb
import variance_window_ref as W
from oracle import philox_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = {"iqlhip_var_pack_window": 10, "iqlhip_var_values_window": 11, "iqlhip_var_train_steps": 14,
                 "iqlhip_var_read_train_ring": 5}


@pytest.mark.parametrize("S,A,B,pad", [(17, 6, 256, 0), (3, 1, 1, 0), (17, 6, 257, 0), (127, 2, 33, 0), (5, 28, 64, 0),
                                         (17, 6, 33, 8)])
def test_window_packing_is_pack_block_of_the_rows(S, A, B, pad):
    from iqlhip_variance import pack_block
    n = B + 40
    rows = W.synthetic_rows(n, S, A, seed=S + B, ld=W.row_stride(S, A) + pad)
    for start in (0, 7, n - B):
        obs, _a, rew, _d, nxt, nd = W.window_tensors(rows, start, B, S, A)
        want, b = pack_block(S, obs, rew, nxt, nd)
        got = W.pack_window(rows, start, B, S, A)
        assert b == B and got.shape == (B * S + S + 2 * B,) and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the last next-state is the LAST row's, and a window must stay inside the rows
    assert np.array_equal(W.pack_window(rows, 3, B, S, A)[B * S:(B + 1) * S], rows[3 + B - 1, S + A:2 * S + A])
    for bad in (-1, n - B + 1):
        with pytest.raises(ValueError):
            W.pack_window(rows, bad, B, S, A)


def _start_by_hand(seed, j, span):
    """Index j of the index stream at counter offset 0, from the scalar generator and Python integers."""
    ctr = j >> 1
    o = P.philox4x32_10_scalar(ctr & 0xFFFFFFFF, ctr >> 32, P.TAG_INDEX, 0, seed & 0xFFFFFFFF, seed >> 32)
    bits = (o[3] << 32 | o[2]) if j & 1 else (o[1] << 32 | o[0])
    return (bits * span) >> 64


@pytest.mark.parametrize("span", [1, 2, 1000])
@pytest.mark.parametrize("listed", [False, True])
def test_burst_starts(span, listed):
    B, seed, n = 16, 0x1234567_89ABCDEF, 64
    size = span + B - 1
    starts = None
    if listed:      # a list of `span` entries: the draw picks the ENTRY, the entries need not be sorted or distinct
        starts = np.random.RandomState(span).randint(0, size - B + 1, size=span).astype(np.int64)
    got = W.burst_starts(n, size, B, seed, 0, starts)
    assert got.dtype == np.int64 and got.shape == (n,)
    picks = np.array([_start_by_hand(seed, j, span) for j in range(n)], dtype=np.int64)
    assert np.array_equal(got, picks if starts is None else starts[picks])
    assert got.min() >= 0 and got.max() <= size - B
    if span == 1:
        assert (got == (0 if starts is None else starts[0])).all()
    if span == 1000 and not listed:
        assert len(set(got.tolist())) > n // 2            # (a stream, not a constant)
    # what iqlhip_draw_indices writes for (n, span, seed, offset 0)
    assert np.array_equal(picks, P.draw_indices(n, span, seed, 0))
    # update k depends on offset + k alone: any split, odd ones included, gives the same starts
    for cut in (1, 3, 32):
        two = np.concatenate([W.burst_starts(cut, size, B, seed, 0, starts), W.burst_starts(n - cut, size, B, seed, cut, starts)])
        assert np.array_equal(two, got)


def test_new_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    bound = {name: (res, args) for name, res, args in hb.SYMBOLS}
    for name, n_args in NEW_FUNCTIONS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name
        assert name in bound and len(bound[name][1]) == n_args, name
        assert hasattr(hb.lib(), name), name
    m = re.search(r"#define\s+IQLHIP_VAR_TRAIN_MAX_STEPS\s+(\d+)", header)
    assert m and int(m.group(1)) == hb.IQLHIP_VAR_TRAIN_MAX_STEPS == 1024
    import variance_learner as VL
    assert VL.TRAIN_MAX_STEPS == 1024
    for method in ("pack_window", "update_from_buffer", "get_values_window", "train_on_buffer", "run_training_on_buffer"):
        assert callable(getattr(VL.VarianceLearner, method)), method


def test_cpu_learner_and_cpu_buffer_are_refused():
    import iql
    import variance_learner as VL
    L = VL.VarianceLearner(5, 2, None, None, batch_size=4, device="cpu")
    buf = iql.ReplayBuffer(5, 2, 16, "cpu")
    for call in (lambda: L.pack_window(buf, 0), lambda: L.update_from_buffer(buf, 0, False), lambda: L.get_values_window(buf, 0),
                 lambda: L.train_on_buffer(buf, 2, seed=1), lambda: L.run_training_on_buffer(buf, 2, save_dir=None)):
        with pytest.raises(NotImplementedError):
            call()
    assert L._adam_t == [0, 0] and hasattr(L, "mf")
