"""CPU-only tests of mixed batch sizes in trainer groups (no GPU in the process): the three _mixed entry points are
declared, exported and bound with the declared argument counts; they reject NULL arguments before any member is
looked at; the Python option validates its size arguments; and the group create flags stay as they were."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import iql
import iqlhip_binding as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED = {"iqlhip_group_step_mixed": 5, "iqlhip_group_train_steps_mixed": 11, "iqlhip_group_online_step_mixed": 16}


def _declared_args(header: str, name: str) -> int:
    m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, name
    return len(m.group(1).split(","))


def test_mixed_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    bound = {name: args for name, _, args in hb.SYMBOLS}
    for name, n_args in MIXED.items():
        assert _declared_args(header, name) == n_args, name
        # one argument list with the uniform entry point's, but for the size argument
        assert _declared_args(header, name[:-len("_mixed")]) == n_args, name
        assert len(bound[name]) == n_args, name
        fn = getattr(hb.lib(), name)                 # (AttributeError if the built library does not export it)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args
    assert bound["iqlhip_group_train_steps_mixed"][4] is not C.c_int32      # B: an array
    assert bound["iqlhip_group_online_step_mixed"][7] is not C.c_int32      # n: an array


def test_mixed_entry_points_reject_null_arguments_before_looking_at_a_member():
    lib = hb.lib()
    fake = 4096       # never dereferenced: every rejection below comes before the group or a member is looked at
    two_p = (C.c_void_p * 2)(fake, fake + 64)
    two_i64 = (C.c_int64 * 2)(8, 8)
    two_u64 = (C.c_uint64 * 2)(1, 2)
    two_i32 = (C.c_int32 * 2)(64, 128)
    scs = (hb.StepScalars * 2)()
    batches = (hb.Batch * 2)()
    out = (C.c_float * 6)()
    calls = [
        lambda: lib.iqlhip_group_step_mixed(None, batches, scs, out, None),
        lambda: lib.iqlhip_group_step_mixed(fake, None, scs, out, None),
        lambda: lib.iqlhip_group_step_mixed(fake, batches, None, out, None),
    ]
    ts = [fake, two_p, 44, two_i64, two_i32, two_p, 2, two_u64, two_u64, 0, None]
    for hole in (0, 1, 3, 4, 5, 7, 8):               # group, rows, size, B, tables, seeds, offsets
        args = list(ts)
        args[hole] = None
        calls.append(lambda args=args: lib.iqlhip_group_train_steps_mixed(*args))
    on = [fake, two_p, 44, two_i64, two_i64, fake, fake, two_i32, scs, out, None, None, None, None, None, None]
    for hole in (0, 1, 3, 4, 5, 6, 7, 8, 9):         # group, rings, capacity, pointer, row, idx, n, sc, out
        args = list(on)
        args[hole] = None
        calls.append(lambda args=args: lib.iqlhip_group_online_step_mixed(*args))
    for call in calls:
        assert call() == hb.E_INVAL
        with pytest.raises(ValueError, match="NULL"):
            hb.check(call())
    # (the uniform entry points' NULL checks are as they were)
    assert lib.iqlhip_group_train_steps(None, two_p, 44, two_i64, 64, two_p, 2, two_u64, two_u64, 0, None) == hb.E_INVAL
    assert lib.iqlhip_group_step(None, batches, scs, out, None) == hb.E_INVAL


def test_group_create_flags_still_has_one_flag():
    fake = 4096
    two = (C.c_void_p * 2)(fake, fake + 64)
    out = C.c_void_p()
    for flags in (2, hb.IQLHIP_GROUP_DROPOUT | 4, -1):
        assert hb.lib().iqlhip_group_create_flags(two, 2, flags, C.byref(out)) == hb.E_INVAL
    assert out.value is None


def _cpu_trainer(S=17, A=6):
    actor = iql.GaussianPolicy(S, A, 1.0)
    qf, vf = iql.TwinQ(S, A), iql.ValueFunction(S)
    return iql.ImplicitQLearning(max_action=1.0, actor=actor,
                                 actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                 q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                                 v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 max_steps=1000, device="cpu")


def test_mixed_batch_option_and_size_arguments_on_cpu():
    a, b = _cpu_trainer(), _cpu_trainer()
    # the keyword exists (a TypeError otherwise); CPU trainers are refused as they always were
    for mixed in (True, False):
        with pytest.raises(RuntimeError, match="GPU"):
            iql.ImplicitQLearningGroup([a, b], mixed_batch=mixed)
    with pytest.raises(ValueError, match="same trainer"):
        iql.ImplicitQLearningGroup([a, b, a], actor_dropout=True, mixed_batch=True)
    sizes = iql.ImplicitQLearningGroup._batch_sizes
    assert sizes(3, 256, False) == [256, 256, 256]
    assert sizes(3, 256, True) == [256, 256, 256]
    assert sizes(2, [64, 64], False) == [64, 64]      # a sequence of equal sizes needs no opt-in
    assert sizes(4, (64, 128, 256, 512), True) == [64, 128, 256, 512]
    assert sizes(2, torch.tensor([64, 128]).numpy(), True) == [64, 128]
    with pytest.raises(ValueError, match="mixed_batch"):
        sizes(2, [64, 128], False)
    with pytest.raises(ValueError, match="3 batch sizes for a group of 2"):
        sizes(2, [64, 128, 256], True)
    with pytest.raises(ValueError, match="1 batch sizes"):
        sizes(2, [64], False)
    with pytest.raises(ValueError, match=">= 1"):
        sizes(2, [64, 0], True)
    # a group object that holds CPU trainers anyway: the size arguments are validated before a member is looked at
    for mixed in (False, True):
        g = object.__new__(iql.ImplicitQLearningGroup)
        g.trainers, g._g, g._ctxs, g._actor_dropout, g._mixed_batch = [a, b], None, None, False, mixed
        bufs = [iql.ReplayBuffer(17, 6, 8, "cpu"), iql.ReplayBuffer(17, 6, 8, "cpu")]
        s, act = np.zeros(17, np.float32), np.zeros(6, np.float32)
        on = (bufs, [s, s], [act, act], [0.0, 0.0], [s, s], [False, False])
        with pytest.raises(ValueError, match="batch sizes for a group of 2"):
            g.train_steps(bufs, 2, [64, 128, 256], [1, 2])
        with pytest.raises(ValueError, match="batch sizes for a group of 2"):
            g.online_step(*on, [4])
        if not mixed:
            with pytest.raises(ValueError, match="mixed_batch"):
                g.train_steps(bufs, 2, [64, 128], [1, 2])
            with pytest.raises(ValueError, match="mixed_batch"):
                g.online_step(*on, [4, 8])
        with pytest.raises(RuntimeError, match="GPU"):      # (valid sizes: the members are looked at next)
            g.train_steps(bufs, 2, [64, 64] if not mixed else [64, 128], [1, 2])
        assert [(x._pointer, x._size) for x in bufs] == [(0, 0), (0, 0)]
        assert a.total_it == 0 and b.total_it == 0
