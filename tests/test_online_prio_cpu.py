"""CPU tests of online prioritised replay (DESIGN.md 6j "Online prioritised replay"): the reference table with a maximum
word (tests/online_prio_ref.py) against a fresh build of its leaves, the rules q_max follows, the Python layer's argument
checks, and the new symbols in the header, the binding and the built library."""
import os
import re

import numpy as np
import pytest

import iqlhip_binding as hb
import iqlhip_weighted as wtd
import online_prio_ref as OP
import weighted_update_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("iqlhip_weights_build_tracking", "iqlhip_weights_max", "iqlhip_weights_insert_max",
               "iqlhip_online_step_prioritized", "iqlhip_online_prioritized_batch")


def _tree_equals_fresh_build(t):
    fresh = U.build_tree_np(t.q)
    held = t.tree()
    assert len(fresh) == len(held)
    for a, b in zip(fresh, held):
        assert np.array_equal(a, b)
    assert int(fresh[-1][-1]) == t.total


# ---------------------------------------------------------------- the reference table
@pytest.mark.parametrize("cap", [64, 65, 4097])
def test_mixed_updates_and_inserts_equal_a_fresh_build(cap):
    rng = np.random.default_rng(cap)
    n = cap - 3
    w = rng.uniform(0.0, 1.0, n).astype(np.float32)
    t = OP.TrackingTable(w, capacity=cap, max_weight=4.0, new_row_weight=1.0)
    shadow = np.zeros(cap, dtype=np.uint64)
    shadow[:n] = U.quantise_at(w, t.e)
    assert np.array_equal(t.q, shadow)
    q_max_seen = t.q_max
    for step in range(12):
        if step % 3 == 2:
            row = int(rng.integers(0, cap))
            t.insert_max(row)
            shadow[row] = np.uint64(t.q_max)
        else:
            idx = rng.integers(0, cap, 40).astype(np.int64)
            ww = rng.uniform(0.0, 3.0, 40).astype(np.float32)
            t.update(idx, ww)
            qn = U.quantise_at(ww, t.e)
            for i, qv in zip(idx, qn):
                shadow[i] = qv
        assert np.array_equal(t.q, shadow)
        assert t.q_max >= q_max_seen          # never falls
        q_max_seen = t.q_max
        _tree_equals_fresh_build(t)
    assert t.version == 12


def test_q_max_after_the_build():
    w = np.array([0.25, 0.5, 0.125], dtype=np.float32)
    # e = floor(log2(0.5)) = -1: q = w * 2^39
    t = OP.TrackingTable(w, capacity=8, new_row_weight=0.375)
    assert t.e == -1 and t.q_max == int(0.5 * 2 ** 39)                       # the largest weight present
    t = OP.TrackingTable(w, capacity=8, max_weight=1.0, new_row_weight=1.0)
    assert t.e == 0 and t.q_max == 1 << 38 and t.w_max == 1.0                # new_row_weight above every weight
    t = OP.TrackingTable(w, capacity=8, new_row_weight=1.0)
    assert t.q_max == U.Q_SATURATED                                          # 1.0 >= 2^(e + 1): saturates like any weight


def test_losing_duplicate_does_not_raise_the_maximum():
    w = np.full(16, 0.25, dtype=np.float32)
    t = OP.TrackingTable(w, max_weight=8.0, new_row_weight=0.25)
    q0 = t.q_max
    # row 3: first 4.0 (the larger, loses), then 0.125 (wins)
    t.update(np.array([3, 3], dtype=np.int64), np.array([4.0, 0.125], dtype=np.float32))
    assert t.q_max == q0 and int(t.q[3]) == int(U.quantise_at(np.array([0.125], dtype=np.float32), t.e)[0])
    # the other order: the larger one wins and raises
    t.update(np.array([3, 3], dtype=np.int64), np.array([0.125, 4.0], dtype=np.float32))
    assert t.q_max == int(U.quantise_at(np.array([4.0], dtype=np.float32), t.e)[0]) > q0
    _tree_equals_fresh_build(t)


def test_skipped_entries_do_not_raise_the_maximum():
    w = np.full(16, 0.25, dtype=np.float32)
    t = OP.TrackingTable(w, max_weight=8.0, new_row_weight=0.25)
    q0 = t.q_max
    idx = np.array([1, 2, 3, 99, -1, 12], dtype=np.int64)
    ww = np.array([np.nan, np.inf, -4.0, 4.0, 4.0, 4.0], dtype=np.float32)
    t.update(idx, ww, bound=10)              # row 12 is outside the bound
    assert t.q_max == q0
    assert t.flags == U.FLAG_NONFINITE | U.FLAG_NEGATIVE | U.FLAG_INDEX
    assert np.all(t.q == t.q[0])


def test_saturating_weight_raises_the_maximum_to_saturation_and_it_stays():
    w = np.full(16, 0.25, dtype=np.float32)
    t = OP.TrackingTable(w, max_weight=1.0, new_row_weight=0.25)
    t.update(np.array([5], dtype=np.int64), np.array([2.0], dtype=np.float32))      # 2.0 = 2^(e + 1)
    assert t.q_max == U.Q_SATURATED
    t.update(np.array([5], dtype=np.int64), np.array([0.0], dtype=np.float32))
    assert t.q_max == U.Q_SATURATED and int(t.q[5]) == 0
    t.insert_max(7)
    assert int(t.q[7]) == U.Q_SATURATED
    _tree_equals_fresh_build(t)


def test_insert_into_a_zero_row_and_over_the_maximum():
    w = np.array([0.5, 0.0, 1.0, 0.25], dtype=np.float32)
    t = OP.TrackingTable(w, capacity=6, new_row_weight=0.5)
    t.insert_max(1)
    t.insert_max(2)                          # already holds q_max: nothing changes but the version
    t.insert_max(5)                          # a row beyond the given weights
    assert [int(x) for x in t.q] == [1 << 37, 1 << 38, 1 << 38, 1 << 36, 0, 1 << 38]
    assert t.version == 3
    with pytest.raises(AssertionError):
        t.insert_max(4, bound=4)


# ---------------------------------------------------------------- the Python layer's checks
def test_tracking_arguments():
    assert wtd.check_tracking_args(True, True, None) == 1.0
    assert wtd.check_tracking_args(True, True, 0.5) == 0.5
    assert wtd.check_tracking_args(True, False, None) is None
    assert wtd.check_tracking_args(False, False, None) is None
    with pytest.raises(ValueError):
        wtd.check_tracking_args(False, True, None)           # track_max without updatable
    with pytest.raises(ValueError):
        wtd.check_tracking_args(True, False, 1.0)            # new_row_weight without track_max
    for bad in (0.0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError):
            wtd.check_tracking_args(True, True, bad)


def test_insert_arguments():
    assert wtd.check_insert_args(3, None, 8) == (3, 8)
    assert wtd.check_insert_args(3, 4, 8) == (3, 4)
    for row, bound in ((8, None), (-1, None), (4, 4), (0, 9), (0, -1), (0, 0)):
        with pytest.raises(ValueError):
            wtd.check_insert_args(row, bound, 8)


def test_offset_step_is_the_counters_a_draw_consumes():
    assert [wtd.online_offset_step(b) for b in (1, 2, 32, 33, 256)] == [1, 1, 16, 17, 128]


def test_sample_weights_refuses_tracking_without_updatable():
    w = np.ones(4, dtype=np.float32)
    with pytest.raises(ValueError):
        wtd.SampleWeights(w, track_max=True)
    with pytest.raises(ValueError):
        wtd.SampleWeights(w, updatable=True, new_row_weight=1.0)
    with pytest.raises(ValueError):
        wtd.SampleWeights(w, updatable=True, track_max=True, new_row_weight=0.0)


def test_buffer_refuses_tracking_on_the_host_and_without_updatable():
    import iql
    buf = iql.ReplayBuffer(3, 2, 8, "cpu")
    buf.add_transition(np.zeros(3), np.zeros(2), 0.0, np.zeros(3), False)
    with pytest.raises(ValueError):
        buf.set_sample_weights(np.ones(1, dtype=np.float32), track_max=True)
    assert buf.sample_weights_track_max is False
    with pytest.raises(ValueError):
        buf.sample_weights_max()
    with pytest.raises(ValueError):
        buf.insert_max_sample_weight(0)


# ---------------------------------------------------------------- the C ABI
def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    bound = {name for name, _, _ in hb.SYMBOLS}
    lib = hb.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in bound, name
        assert hasattr(lib, name), name
