"""CPU tests of weighted replay sampling in trainer groups (DESIGN.md 6i "trainer groups"): the C ABI's new symbol, the
host-side resolution of which table each member draws by (iqlhip_weighted.check_group_call), and the premise of the GPU
poison test (tests/test_hip_group_weighted.py), checked in the reference alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import iql
import iqlhip_binding as hb
import iqlhip_weighted as wtd
import weighted_ref as W
from oracle import philox_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, N_ARGS = "iqlhip_group_train_steps_weighted", 12

# The poison fixture of the GPU test: odd rows hold NaN states and rewards and weigh 0, even rows weigh 1; K fresh members
# (total_it = 0: stream offset 0) draw POISON_STEPS batches of POISON_B rows under POISON_SEEDS.
POISON_N, POISON_B, POISON_STEPS, POISON_SEEDS = 4097, 64, 4, (5, 6, 7)


def poison_weights():
    w = np.ones(POISON_N, dtype=np.float32)
    w[1::2] = 0.0
    return w


def poison_triples():
    """(seed, offset, count) of every member's draws in the GPU poison test."""
    return [(seed, 0, POISON_STEPS * POISON_B) for seed in POISON_SEEDS]


# ---------------------------------------------------------------- C ABI
def test_header_binding_and_library_agree_on_the_new_symbol():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    m = re.search(r"int\s+" + ENTRY + r"\s*\(([^;]*)\)\s*;", header)
    assert m and len(m.group(1).split(",")) == N_ARGS
    bound = {name: args for name, _, args in hb.SYMBOLS}
    assert len(bound[ENTRY]) == N_ARGS
    fn = getattr(hb.lib(), ENTRY)                    # (AttributeError if the built library does not export it)
    assert fn.restype is C.c_int and len(fn.argtypes) == N_ARGS
    m = re.search(r"#define\s+IQLHIP_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == hb.lib().iqlhip_version() >= 380
    assert callable(getattr(iql.ImplicitQLearningGroup, "train_steps_weighted", None))
    assert callable(getattr(wtd, "SampleWeights", None)) and callable(getattr(wtd, "check_group_call", None))


def test_entry_point_rejects_null_arguments_before_looking_at_a_member():
    lib = hb.lib()
    fake = 4096       # never dereferenced: every rejection below comes before the group or a member is looked at
    two_p = (C.c_void_p * 2)(fake, fake + 64)
    two_i64 = (C.c_int64 * 2)(8, 8)
    two_u64 = (C.c_uint64 * 2)(1, 2)
    two_i32 = (C.c_int32 * 2)(8, 8)
    full = [fake, two_p, 48, two_i64, two_i32, two_p, 2, two_u64, two_u64, 0, None, two_p]
    for hole in (0, 1, 3, 4, 5, 7, 8, 11):
        args = list(full)
        args[hole] = None
        assert getattr(lib, ENTRY)(*args) == hb.E_INVAL, hole
        with pytest.raises(ValueError, match="NULL"):
            hb.check(getattr(lib, ENTRY)(*args))


# ---------------------------------------------------------------- which table a member draws by
class _Buf:
    """What check_group_call looks at of a GPU replay buffer."""
    _gpu = True

    def __init__(self, size, weights_n=None):
        self.size, self.sample_weights_n = size, weights_n

    def _index_bound(self):
        return self.size


class _Table(wtd.SampleWeights):
    """A SampleWeights without a device table: n rows, alive."""

    def __init__(self, n):
        self._table, self._n, self._gen, self._device = object(), n, 1, None

    def free(self):
        self._table = None


def test_check_group_call_with_the_buffers_own_tables():
    a, b = _Buf(100, 100), _Buf(70, 70)
    assert wtd.check_group_call(a, None, 3) == [a, a, a]
    assert wtd.check_group_call([a, b], None, 2) == [a, b]
    with pytest.raises(ValueError, match=r"no sample weights.*member 1"):
        wtd.check_group_call([a, _Buf(70)], None, 2)
    b.size = 71                                              # the index bound moved since the weights were set
    with pytest.raises(ValueError, match=r"set_sample_weights again.*member 1"):
        wtd.check_group_call([a, b], None, 2)
    with pytest.raises(ValueError, match="3 buffers"):
        wtd.check_group_call([a, a], None, 3)
    cpu = iql.ReplayBuffer(3, 2, 10, "cpu")
    with pytest.raises(ValueError, match="GPU"):
        wtd.check_group_call(cpu, None, 2)


def test_check_group_call_with_free_standing_tables():
    shared, w100, w70 = _Buf(100), _Table(100), _Table(70)    # (the buffer itself has no weights: none are needed)
    assert wtd.check_group_call(shared, w100, 3) == [w100, w100, w100]
    assert wtd.check_group_call(shared, [w100, None, w100], 3) == [w100, None, w100]
    assert wtd.check_group_call(shared, [None, None], 2) == [None, None]
    assert wtd.check_group_call([shared, _Buf(70)], (w100, w70), 2) == [w100, w70]
    with pytest.raises(ValueError, match="2 weight tables for a group of 3"):
        wtd.check_group_call(shared, [w100, w100], 3)
    with pytest.raises(ValueError, match=r"cover 70 rows.*draws over 100.*member 1"):
        wtd.check_group_call(shared, [w100, w70, None], 3)
    with pytest.raises(ValueError, match="cover 70 rows"):
        wtd.check_group_call(shared, w70, 2)
    with pytest.raises(ValueError, match="SampleWeights"):
        wtd.check_group_call(shared, [w100, np.ones(100, dtype=np.float32)], 2)
    with pytest.raises(ValueError, match="SampleWeights"):
        wtd.check_group_call(shared, np.ones(100, dtype=np.float32), 2)
    cpu = iql.ReplayBuffer(3, 2, 10, "cpu")
    for weights in (_Table(10), [None, None]):
        with pytest.raises(ValueError, match="GPU"):
            wtd.check_group_call(cpu, weights, 2)
    gone = _Table(100)
    gone.free()
    with pytest.raises(ValueError, match="freed"):
        wtd.check_group_call(shared, gone, 2)
    assert wtd.check_table(shared, w100) == 100


def test_sample_weights_checks_the_vector_before_any_device_work():
    for bad in (np.ones(5, dtype=np.float64), np.ones((5, 1), dtype=np.float32), [1.0] * 5, np.ones(0, dtype=np.float32),
                np.array([1.0, np.nan], dtype=np.float32), np.array([1.0, -1.0], dtype=np.float32),
                np.zeros(4, dtype=np.float32)):
        with pytest.raises(ValueError):
            wtd.SampleWeights(bad, device="cuda:0")
    with pytest.raises(ValueError, match="GPU"):
        wtd.SampleWeights(np.ones(4, dtype=np.float32), device="cpu")


# ---------------------------------------------------------------- the poison fixture's premise, in the reference alone
def test_poison_fixture_weighted_draws_avoid_every_poisoned_row_and_uniform_draws_do_not():
    w = poison_weights()
    for seed, offset, count in poison_triples():
        idx = W.draw_indices(count, w, seed, offset)
        assert idx.shape == (count,) and np.all(w[idx] > 0) and np.all(idx % 2 == 0), seed
        uniform = P.draw_indices(count, POISON_N, seed, offset)
        assert np.any(w[uniform] == 0), seed
        # ... in the very first step already: a member that falls back to the uniform draw trains on a NaN row at once
        assert np.any(w[uniform[:POISON_B]] == 0), seed
