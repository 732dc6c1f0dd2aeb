"""CPU tests of per-row loss weights, importance-sampling weights and prioritised replay in trainer groups (DESIGN.md 6j
"trainer groups"): the C ABI's three new symbols, and the Python argument normalisation — alpha / eps / is_beta as one
number or K of them, and the one-table-per-member rule of the prioritised call — which raises before any library call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import iql
import iqlhip_binding as hb
import iqlhip_weighted as wtd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"iqlhip_group_step_rw": 7, "iqlhip_group_train_steps_weighted_is": 13,
           "iqlhip_group_train_steps_prioritized": 15}


# ---------------------------------------------------------------- C ABI
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_header_binding_and_library_agree_on_the_new_symbols(entry):
    n_args = ENTRIES[entry]
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    m = re.search(r"int\s+" + entry + r"\s*\(([^;]*)\)\s*;", header)
    assert m and len(m.group(1).split(",")) == n_args
    bound = {name: args for name, _, args in hb.SYMBOLS}
    assert len(bound[entry]) == n_args
    fn = getattr(hb.lib(), entry)                    # (AttributeError if the built library does not export it)
    assert fn.restype is C.c_int and len(fn.argtypes) == n_args
    m = re.search(r"#define\s+IQLHIP_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == hb.lib().iqlhip_version() >= 400
    m = re.search(r"#define\s+IQLHIP_GROUP_TS_CONTINUE\s+(\d+)", header)
    assert m and int(m.group(1)) == hb.IQLHIP_GROUP_TS_CONTINUE
    for name in ("train_steps_prioritized", "last_td_errors"):
        assert callable(getattr(iql.ImplicitQLearningGroup, name, None))


def test_entry_points_reject_null_arguments_before_looking_at_a_member():
    lib = hb.lib()
    fake = 4096       # never dereferenced: every rejection below comes before the group or a member is looked at
    two_p = (C.c_void_p * 2)(fake, fake + 64)
    two_i64 = (C.c_int64 * 2)(8, 8)
    two_u64 = (C.c_uint64 * 2)(1, 2)
    two_i32 = (C.c_int32 * 2)(8, 8)
    two_f = (C.c_float * 2)(0.5, 0.5)
    full = [fake, two_p, 48, two_i64, two_i32, two_p, 2, two_u64, two_u64, 0, None, two_p, two_f, two_f, two_f]
    for entry, holes in (("iqlhip_group_train_steps_weighted_is", (0, 1, 3, 4, 5, 7, 8, 11, 12)),
                         ("iqlhip_group_train_steps_prioritized", (0, 1, 3, 4, 5, 7, 8, 11, 12, 13, 14))):
        for hole in holes:
            args = list(full[:ENTRIES[entry]])
            args[hole] = None
            assert getattr(lib, entry)(*args) == hb.E_INVAL, (entry, hole)
            with pytest.raises(ValueError, match="NULL"):
                hb.check(getattr(lib, entry)(*args))
    for hole in (0, 1, 2, 3, 4):
        args = [fake, (hb.Batch * 2)(), (hb.StepScalars * 2)(), two_p, two_p, None, None]
        args[hole] = None
        assert lib.iqlhip_group_step_rw(*args) == hb.E_INVAL, hole


# ---------------------------------------------------------------- one number, or one per member
def test_scalar_and_per_member_exponents():
    assert wtd.per_member(0.5, 3, "alpha") == [0.5, 0.5, 0.5]
    assert wtd.per_member([0.1, 0.2], 2, "alpha") == [0.1, 0.2]
    assert wtd.per_member(np.array([0.1, 0.2]), 2, "eps") == [0.1, 0.2]
    for bad in ([0.1], (0.1, 0.2, 0.3), np.zeros(4)):
        with pytest.raises(ValueError, match="for a group of 2"):
            wtd.per_member(bad, 2, "alpha")
    assert wtd.check_group_priority_args(2, 0.6, 1e-3) == ([0.6, 0.6], [1e-3, 1e-3])
    assert wtd.check_group_priority_args(2, [0.6, 0.0], [0.0, 0.5]) == ([0.6, 0.0], [0.0, 0.5])
    assert wtd.check_group_priority_args(3, 1, [0.0, 0.5, 1]) == ([1.0, 1.0, 1.0], [0.0, 0.5, 1.0])
    with pytest.raises(ValueError, match=r"alpha = 0 needs eps > 0.*member 1"):
        wtd.check_group_priority_args(2, [0.6, 0.0], [1e-3, 0.0])
    with pytest.raises(ValueError, match=r"alpha = 0 needs eps > 0.*member 0"):
        wtd.check_group_priority_args(2, 0.0, 0.0)
    for alpha, eps in (([0.6, -0.1], 1e-3), (0.6, [1e-3, float("inf")]), ([0.6, float("nan")], 1e-3), (["x", 0.6], 1e-3)):
        with pytest.raises(ValueError, match="member"):
            wtd.check_group_priority_args(2, alpha, eps)
    with pytest.raises(ValueError, match="3 values of alpha for a group of 2"):
        wtd.check_group_priority_args(2, [0.6, 0.6, 0.6], 1e-3)
    with pytest.raises(ValueError, match="1 values of eps for a group of 2"):
        wtd.check_group_priority_args(2, 0.6, [1e-3])
    assert wtd.check_group_is_beta(3, 0.4) == [0.4, 0.4, 0.4]
    assert wtd.check_group_is_beta(2, [0, 1]) == [0.0, 1.0]
    for bad in ([0.4, -0.1], [0.4, float("nan")], [0.4, float("inf")], [0.4, None]):
        with pytest.raises(ValueError, match=r"is_beta.*member 1"):
            wtd.check_group_is_beta(2, bad)
    with pytest.raises(ValueError, match="3 values of is_beta for a group of 2"):
        wtd.check_group_is_beta(2, [0.4, 0.4, 0.4])


# ---------------------------------------------------------------- a table per member
class _Buf:
    """What the group checks look at of a GPU replay buffer."""
    _gpu = True

    def __init__(self, size, weights_n=None, updatable=False, capacity=None):
        self.size, self.sample_weights_n, self._weights_updatable = size, weights_n, updatable
        self._buffer_size = size if capacity is None else capacity

    def _index_bound(self):
        return self.size


class _Table(wtd.SampleWeights):
    """A SampleWeights without a device table: n rows, alive."""

    def __init__(self, n, updatable=True):
        self._table, self._n, self._gen, self._device, self._updatable = object(), n, 1, None, updatable

    def free(self):
        self._table = None


def test_a_prioritised_group_call_needs_an_updatable_table_of_its_own_per_member():
    shared = _Buf(100)
    a, b, c = _Table(100), _Table(100), _Table(100)
    assert wtd.check_group_prioritized(shared, [a, b, c], 3) == [a, b, c]
    with pytest.raises(ValueError, match=r"member 2 draws by the table of member 0"):
        wtd.check_group_prioritized(shared, [a, b, a], 3)
    with pytest.raises(ValueError, match=r"member 1 draws by the table of member 0"):
        wtd.check_group_prioritized(shared, a, 2)                     # one SampleWeights for all members
    with pytest.raises(ValueError, match=r"table for every member \(member 1 has none\)"):
        wtd.check_group_prioritized(shared, [a, None], 2)
    with pytest.raises(ValueError, match=r"updatable.*member 1"):
        wtd.check_group_prioritized(shared, [a, _Table(100, updatable=False)], 2)
    with pytest.raises(ValueError, match=r"span 70 rows.*member 1"):
        wtd.check_group_prioritized(shared, [a, _Table(70)], 2)
    with pytest.raises(ValueError, match="2 weight tables for a group of 3"):
        wtd.check_group_prioritized(shared, [a, b], 3)
    # the buffers' own tables: one buffer each is fine, one shared buffer is one table for two members
    own = [_Buf(100, 100, updatable=True), _Buf(80, 80, updatable=True)]
    assert wtd.check_group_prioritized(own, None, 2) == own
    with pytest.raises(ValueError, match=r"member 1 draws by the table of member 0"):
        wtd.check_group_prioritized(own[0], None, 2)
    with pytest.raises(ValueError, match=r"updatable.*member 1"):
        wtd.check_group_prioritized([own[0], _Buf(80, 80)], None, 2)
    with pytest.raises(ValueError, match=r"no sample weights.*member 1"):
        wtd.check_group_prioritized([own[0], _Buf(80)], None, 2)
    # the weighted call with is_beta keeps check_group_call's rules: tables may be shared, members may be uniform
    assert wtd.check_group_call(shared, [a, a, None], 3) == [a, a, None]
