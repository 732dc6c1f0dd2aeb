"""CPU tests of updatable weight tables (DESIGN.md 6i "updatable tables"): the integer statement of the update and of the
node-local tree (tests/weighted_update_ref.py), and the checks that need no GPU."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import iqlhip_binding as hb
import iqlhip_weighted as wtd
import weighted_ref as W
import weighted_update_ref as U
from oracle import philox_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 63, 64, 65, 4097, 262145]          # 262 145: the first size with four levels
NEW_SYMBOLS = ("iqlhip_weights_build_updatable", "iqlhip_weights_update", "iqlhip_weights_clear_flags",
               "iqlhip_weights_state")
M64 = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def _weights(n):
    rng = np.random.RandomState(100 + n)
    w = np.exp(1.5 * rng.randn(n)).astype(np.float32)
    w[rng.rand(n) < 0.1] = 0.0
    if not np.any(w > 0):
        w[0] = 0.5
    w.setflags(write=False)
    return w


def _update(n, m, rng, wmax):
    """m entries over n rows: duplicates, zeros, saturating weights, and one skipped entry of every kind."""
    idx = rng.randint(0, n, size=m).astype(np.int64)
    w = np.exp(1.5 * rng.randn(m)).astype(np.float32)
    w[rng.rand(m) < 0.2] = 0.0
    w[rng.rand(m) < 0.1] = np.float32(wmax * 64.0)                  # beyond the scale: saturates
    if m >= 8:
        idx[1] = idx[5] = idx[7] = idx[0]                           # one row four times: position 7 wins
        w[2], w[3], w[4] = np.nan, -1.0, np.inf
        idx[6] = -1
        idx[m - 1] = n                                              # == bound
    return idx, w


# ---------------------------------------------------------------- quantisation at a fixed scale
def test_quantisation_at_a_fixed_scale_is_floor_and_saturates():
    rng = np.random.RandomState(4)
    for e in (-140, -20, 0, 3, 100):
        w = (rng.rand(2000) * np.float32(2.0) ** np.float32(e + 1)).astype(np.float32)
        w = w[w < np.float32(2.0) ** (e + 1)] if e + 1 <= 127 else w
        # (float64 holds w * 2^(38 - e) exactly where it is not below 1; int() floors)
        want = [int(float(x) * 2.0 ** (38 - e)) if float(x) * 2.0 ** (38 - e) >= 1.0 else 0 for x in w]
        assert [int(a) for a in U.quantise_at(w, e)] == want
        top = np.float32(2.0) ** (e + 1)
        edge = np.array([np.nextafter(top, np.float32(0)), top, top * np.float32(3)], dtype=np.float32)
        q = U.quantise_at(edge, e)
        assert int(q[1]) == int(q[2]) == U.Q_SATURATED and int(q[0]) < U.Q_SATURATED
        if e > -100:                                                # (a normal top: 24 significant bits below it)
            assert int(q[0]) == (1 << 39) - (1 << 15)
    # max_weight = 0: the static table's q[]
    w = _weights(4097)
    assert np.array_equal(U.Table(w).q, W.quantise(w))
    assert U.Table(w, max_weight=1000.0).e == 9 and U.Table(w, max_weight=1e-3).e == W.exponent(w)


# ---------------------------------------------------------------- update == rebuild
@pytest.mark.parametrize("n", SIZES)
def test_update_equals_a_build_of_the_modified_weights(n):
    rng = np.random.RandomState(n)
    w = _weights(n)
    cap = n + (37 if n > 1 else 0)
    tab = U.Table(w, capacity=cap, max_weight=float(w.max()) * 1.5)
    assert tab.n == cap and np.all(tab.q[n:] == 0)
    mod = np.zeros(cap, dtype=np.float32)
    mod[:n] = w
    for m in (1, 64, 257):
        idx, uw = _update(n, m, rng, float(w.max()))
        tab.update(idx, uw, bound=n)
        for i, x in zip(idx, uw):                                   # the same semantics, entry by entry, on the weights
            if np.isfinite(x) and not x < 0 and 0 <= i < n:
                mod[i] = x
    assert tab.version == 3
    assert tab.flags == U.FLAG_NONFINITE | U.FLAG_NEGATIVE | U.FLAG_INDEX
    fresh_q = U.quantise_at(mod, tab.e)
    assert np.array_equal(tab.q, fresh_q)
    assert n < 63 or np.any(tab.q == U.Q_SATURATED)
    got, want = tab.tree(), U.build_tree_np(fresh_q)
    assert len(got) == len(want) == len(U.level_sizes(cap))
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert tab.total == int(want[-1][-1]) == sum(int(x) for x in fresh_q)
    if cap <= 4200:                                                 # the numpy tree is the plain-integer tree
        for a, b in zip(got, U.build_tree(fresh_q)):
            assert [int(x) for x in a] == b


def test_the_last_position_wins_and_bad_entries_are_skipped():
    tab = U.Table(np.ones(10, dtype=np.float32), max_weight=4.0)
    one = int(tab.q[0])
    tab.update([3, 3, 3, 4, 5, 6, -1, 10], np.array([2.0, 0.5, 4.0, np.nan, -1.0, -0.0, 1.0, 1.0], dtype=np.float32))
    assert int(tab.q[3]) == 4 * one                                 # the last of the three
    assert int(tab.q[4]) == one and int(tab.q[5]) == one            # skipped: as they were
    assert int(tab.q[6]) == 0                                       # -0.0 is zero
    assert tab.flags == 7
    tab.update([3, 3], np.array([2.0, np.inf], dtype=np.float32))   # a bad last entry does not undo the valid one before
    assert int(tab.q[3]) == 2 * one
    tab.update(np.arange(10), np.zeros(10, dtype=np.float32))       # total 0 is allowed; draws stay in range
    assert tab.total == 0
    assert np.all(tab.draw_indices(100, 1, 2) == 9)
    assert all(U.descend_r(tab.tree(), r) == 9 for r in (0, M64))


# ---------------------------------------------------------------- the descent
@pytest.mark.parametrize("n", SIZES)
def test_local_descent_equals_the_global_search(n):
    w = _weights(n)
    q = W.quantise(w)
    cum, total = W.table(w)
    levels = U.build_tree_np(q)
    assert int(levels[-1][-1]) == total
    r = [0, M64, 1, M64 - 1] + [int(x) for x in W.random_bits(300, 11, 2 ** 64 - 7)]
    want = np.searchsorted(cum, P.mulhi64(np.array(r, dtype=np.uint64), total), side="right")
    assert [U.descend_r(levels, x) for x in r] == [int(x) for x in want]
    # t exactly on, one below and one above a node's boundary, at every level; the ends
    ts = {0, total - 1}
    for k in (63, 64, 127, 4095, 4096, 262143, 262144):
        if k < n:
            ts |= {int(cum[k]) - 1, int(cum[k]), int(cum[k]) + 1}
    for t in sorted(x for x in ts if 0 <= x < total):
        assert U.descend(levels, t) == int(np.searchsorted(cum, np.uint64(t), side="right")), (n, t)
    # ... and the reference's own draw is that search
    assert np.array_equal(U.Table(w).draw_indices(300, 11, 5), W.draw_indices(300, w, 11, 5))


# ---------------------------------------------------------------- C ABI and argument checks
def test_header_binding_and_library_agree_on_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    declared = set(re.findall(r"\b(iqlhip_[a-z_0-9]+)\s*\(", header))
    bound = {name for name, _, _ in hb.SYMBOLS}
    lib = hb.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in bound and hasattr(lib, name), name


def test_updatable_argument_checks():
    assert wtd.check_updatable_args(5, None, None) == (5, 0.0)
    assert wtd.check_updatable_args(5, 9, 2.5) == (9, 2.5)
    with pytest.raises(ValueError, match="smaller"):
        wtd.check_updatable_args(5, 4, None)                        # capacity < n
    with pytest.raises(ValueError, match="2\\^24"):
        wtd.check_updatable_args(5, (1 << 24) + 1, None)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="max_weight"):
            wtd.check_updatable_args(5, None, bad)
    # capacity / max_weight without updatable=True: refused before any look at a device
    with pytest.raises(ValueError, match="updatable"):
        wtd.SampleWeights(np.ones(5, dtype=np.float32), capacity=9)
    with pytest.raises(ValueError, match="smaller"):
        wtd.SampleWeights(np.ones(5, dtype=np.float32), updatable=True, capacity=4)
    with pytest.raises(ValueError, match="2\\^24"):
        wtd.SampleWeights(np.ones(5, dtype=np.float32), updatable=True, capacity=(1 << 24) + 1)


def test_update_argument_checks():
    idx, w = torch.zeros(4, dtype=torch.int64), torch.ones(4)
    assert wtd.check_update_args(idx, w) == 4
    for bad_idx, bad_w in ((idx[:3], w), (idx.to(torch.int32), w), (idx, w.double()), (idx[:, None], w[:, None]),
                           (idx.numpy(), w)):
        with pytest.raises(ValueError):
            wtd.check_update_args(bad_idx, bad_w)
    with pytest.raises(ValueError, match="device"):
        wtd.check_update_args(idx, w, torch.device("cuda", 0))
    static = object.__new__(wtd.SampleWeights)                      # a live static table, as far as update() looks
    static._table, static._n, static._updatable = 1, 4, False
    with pytest.raises(ValueError, match="not updatable"):
        static.update(idx, w)
    static._table = None                                            # (nothing for the destructor to free)


def test_check_call_lets_an_updatable_table_outlive_the_index_bound():
    class Fake:
        _gpu = True
        sample_weights_n = 16
        _weights_updatable = True
        size = 7

        def _index_bound(self):
            return self.size
    f = Fake()
    assert wtd.check_call(f) == 16
    f.size = 8
    assert wtd.check_call(f) == 16
    f._weights_updatable = False
    with pytest.raises(ValueError, match="set_sample_weights again"):
        wtd.check_call(f)
