"""CPU tests of variance-learner groups (DESIGN.md 6l "Groups of learners"; no GPU in the process): the new C ABI is
declared, exported and bound with matching argument counts; VarianceLearnerGroup refuses what it must before any library
call; seeds / offsets / starts are normalised to one entry per member; the scalar table of a split burst is the solo
calls' per-update scalars, update-major."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import iqlhip_binding as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = {"iqlhip_var_group_create": 3, "iqlhip_var_group_destroy": 1, "iqlhip_var_group_step": 6,
                 "iqlhip_var_group_values": 6, "iqlhip_var_group_read_loss": 5, "iqlhip_var_group_pack_windows": 9,
                 "iqlhip_var_group_step_windows": 10, "iqlhip_var_group_values_windows": 10,
                 "iqlhip_var_group_train_steps": 14, "iqlhip_var_group_read_train_ring": 5}
SCALAR_FIELDS = ("step_size", "bc2_sqrt", "beta2", "one_minus_beta1", "one_minus_beta2", "eps", "aligned_rewards")


def test_new_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    bound = {name: (res, args) for name, res, args in hb.SYMBOLS}
    for name, n_args in NEW_FUNCTIONS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == n_args, name
        fn = getattr(hb.lib(), name)                  # (AttributeError if the built library does not export it)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args, name
    assert re.search(r"typedef\s+struct\s+iqlhip_var_group\s+iqlhip_var_group\s*;", header)
    import variance_learner as VL
    assert VL.MAX_GROUP == hb.IQLHIP_MAX_GROUP == 16 and "VarianceLearnerGroup" in VL.__all__
    for method in ("update", "get_values", "update_from_buffer", "get_values_window", "train_on_buffer",
                   "run_training_on_buffer", "gates"):
        assert callable(getattr(VL.VarianceLearnerGroup, method)), method


def _cpu(S=5, B=4):
    import variance_learner as VL
    return VL.VarianceLearner(S, 2, None, None, batch_size=B, device="cpu")


def _as_if_attached(L, index=0):
    """A CPU learner that looks attached (a handle that is never passed on, a GPU device): what the group's own checks
    read.  No library call may follow."""
    L._h, L._dev = C.c_void_p(0x1000 + id(L) % 4096), torch.device("cuda", index)
    return L


def _detach(*learners):
    for L in learners:
        L._h = None      # (the learner's destructor would hand the handle to the library)


def test_cpu_learners_are_refused():
    import variance_learner as VL
    a, b = _cpu(), _cpu()
    with pytest.raises(NotImplementedError, match="member 0"):
        VL.VarianceLearnerGroup([a, b])
    c = _as_if_attached(_cpu())
    try:
        with pytest.raises(NotImplementedError, match="member 1"):
            VL.VarianceLearnerGroup([c, b])
    finally:
        _detach(c)
    assert a._adam_t == [0, 0] and b._adam_t == [0, 0]


def test_refusals_that_need_no_library_call():
    import iql
    import variance_learner as VL
    a, b, other_dim, other_dev, other_b = (_as_if_attached(_cpu()), _as_if_attached(_cpu()), _as_if_attached(_cpu(S=6)),
                                           _as_if_attached(_cpu(), index=1), _as_if_attached(_cpu(B=3)))
    try:
        with pytest.raises(ValueError, match="member 1: the learner is member 0 too"):
            VL.VarianceLearnerGroup([a, a])
        with pytest.raises(ValueError, match="member 2: the learner is member 0 too"):
            VL.VarianceLearnerGroup([a, b, a])
        with pytest.raises(ValueError, match="member 1: state_dim = 6"):
            VL.VarianceLearnerGroup([a, other_dim])
        with pytest.raises(ValueError, match="member 1: device"):
            VL.VarianceLearnerGroup([a, other_dev])
        with pytest.raises(ValueError, match="1..16 members, got 0"):
            VL.VarianceLearnerGroup([])
        with pytest.raises(ValueError, match="1..16 members, got 17"):
            VL.VarianceLearnerGroup([a] * 17)
        g = VL.VarianceLearnerGroup([a, b])
        assert g.K == 2 and g._g is None
        buf = iql.ReplayBuffer(5, 2, 16, "cpu")
        buf._size = 16
        batch = ([np.zeros(5, np.float32)] * 4, None, [0.0] * 4, None, [np.zeros(5, np.float32)] * 4, [False] * 4)
        calls = [
            lambda: g.update([batch], False), lambda: g.update([batch] * 3, True), lambda: g.get_values([batch]),
            lambda: g.update_from_buffer([buf], 0, False), lambda: g.update_from_buffer(buf, [0, 0, 0], False),
            lambda: g.get_values_window([buf] * 3, 0), lambda: g.get_values_window(buf, [0]),
            lambda: g.train_on_buffer([buf] * 3, 2, seeds=1), lambda: g.train_on_buffer(buf, 2, seeds=[1, 2, 3]),
            lambda: g.train_on_buffer(buf, 2, seeds=1, offsets=[0]),
            # buffers on another device than the learners
            lambda: g.update_from_buffer(buf, 0, False), lambda: g.get_values_window(buf, 0),
            lambda: g.train_on_buffer(buf, 2, seeds=1), lambda: g.run_training_on_buffer(buf, 4, seeds=1, save_dir=None),
            lambda: g.run_training_on_buffer(buf, 4, seeds=1, env_names=["a"], save_dir=None),
        ]
        for i, call in enumerate(calls):
            with pytest.raises(ValueError):
                call()
            assert g._g is None and a._adam_t == [0, 0] and b._adam_t == [0, 0] and hasattr(a, "mf"), i
        # members of different batch_size cannot share a window call
        h = VL.VarianceLearnerGroup([a, other_b])
        with pytest.raises(ValueError, match="member 1: batch_size = 3"):
            h._batch_size()
    finally:
        _detach(a, b, other_dim, other_dev, other_b)


def test_per_member_normalisation():
    from iqlhip_variance import per_member, per_member_starts
    assert per_member(7, 3, "seeds") == [7, 7, 7] and per_member([1, 2, 3], 3, "seeds") == [1, 2, 3]
    assert per_member((4, 5), 2, "offsets") == [4, 5] and per_member(0, 1, "offsets") == [0]
    for bad in ([1, 2], [], (1, 2, 3, 4)):
        with pytest.raises(ValueError, match="one entry per member"):
            per_member(bad, 3, "seeds")
    assert per_member_starts(None, 3) == [None, None, None]
    one = np.array([3, 1, 2], dtype=np.int64)
    got = per_member_starts(one, 2)
    assert len(got) == 2 and got[0] is one and got[1] is one
    t = torch.tensor([5, 6], dtype=torch.int64)
    assert all(x is t for x in per_member_starts(t, 4))
    # a list of integers is ONE list for all, whatever its length
    got = per_member_starts([3, 1, 2], 2)
    assert len(got) == 2 and all(x.dtype == np.int64 and x.tolist() == [3, 1, 2] for x in got)
    got = per_member_starts([], 2)
    assert len(got) == 2 and all(x.dtype == np.int64 and x.size == 0 for x in got)
    # entries that are lists, arrays, tensors or None: one per member
    got = per_member_starts([one, None, [4, 5]], 3)
    assert got[0] is one and got[1] is None and got[2].dtype == np.int64 and got[2].tolist() == [4, 5]
    assert per_member_starts((None, None), 2) == [None, None]
    for bad in ([one, None], [None], [None, t, None, None]):
        with pytest.raises(ValueError, match="one entry per member"):
            per_member_starts(bad, 3)


def _fields(s):
    return tuple(getattr(s, f) for f in SCALAR_FIELDS)


def test_scalar_table_of_a_split_burst_is_the_solo_scalars():
    from iqlhip_variance import TRAIN_MAX_STEPS, adam_scalars, burst_chunks, group_scalar_table
    assert burst_chunks(1) == [1] and burst_chunks(1024) == [1024] and burst_chunks(1030) == [1024, 6]
    assert burst_chunks(2 * TRAIN_MAX_STEPS + 1) == [TRAIN_MAX_STEPS, TRAIN_MAX_STEPS, 1]
    hypers = [(1e-4, (0.9, 0.999), 1e-8), (3e-4, (0.8, 0.99), 1e-6), (1e-3, (0.9, 0.999), 1e-8)]
    aligned = [False, True, False]
    t0 = [0, 7, 2000]                                  # members at different step counts
    K, n = 3, 1030
    # what the solo bursts pass, per member: update i of the burst is Adam step t0 + i + 1 (iqlhip_var_train_steps)
    solo = [[_fields(adam_scalars(*hypers[k], t0[k] + i + 1, aligned[k])) for i in range(n)] for k in range(K)]
    done, t = 0, list(t0)
    for m in burst_chunks(n):
        tab = group_scalar_table(hypers, t, m, aligned)
        assert len(tab) == m * K and C.sizeof(tab) == m * K * C.sizeof(hb.VarScalars)
        for i in (0, 1, m // 2, m - 1):
            for k in range(K):
                assert _fields(tab[i * K + k]) == solo[k][done + i], (done, i, k)
        t = [x + m for x in t]
        done += m
    assert done == n
    whole = [_fields(s) for s in group_scalar_table(hypers, t0, 8, aligned)]
    parts = [_fields(s) for s in group_scalar_table(hypers, t0, 3, aligned)] + \
            [_fields(s) for s in group_scalar_table(hypers, [x + 3 for x in t0], 5, aligned)]
    assert whole == parts
    assert C.sizeof(hb.VarScalars) == 32
