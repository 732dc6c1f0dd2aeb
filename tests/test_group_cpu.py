"""CPU-only tests of the trainer-group surface (no GPU in the process): the group entry points reject bad groups
before any device work, the Python class raises its validation errors for CPU-constructed trainers, and the built
library's resource report lists the group kernels without scratch or spills."""
import ctypes as C
import os
import re

import pytest
import torch

import iql
import iql_offline
import iqlhip_binding as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_entry_points_reject_bad_groups_before_device_work():
    lib = hb.lib()
    out = C.c_void_p()
    fake = 4096       # never dereferenced: every rejection below comes before a member is looked at
    two_same = (C.c_void_p * 2)(fake, fake)
    with_null = (C.c_void_p * 2)(fake, None)
    many = (C.c_void_p * (hb.IQLHIP_MAX_GROUP + 1))(*[fake + 64 * i for i in range(hb.IQLHIP_MAX_GROUP + 1)])
    for call in (
        lambda: lib.iqlhip_group_create(None, 2, C.byref(out)),               # NULL member array
        lambda: lib.iqlhip_group_create(two_same, 0, C.byref(out)),           # k = 0
        lambda: lib.iqlhip_group_create(many, hb.IQLHIP_MAX_GROUP + 1, C.byref(out)),
        lambda: lib.iqlhip_group_create(with_null, 2, C.byref(out)),          # a NULL member
        lambda: lib.iqlhip_group_create(two_same, 2, C.byref(out)),           # the same member twice
        lambda: lib.iqlhip_group_create(two_same, 1, None),                   # NULL out
        lambda: lib.iqlhip_group_destroy(None),
        lambda: lib.iqlhip_group_step(None, None, None, None, None),
        lambda: lib.iqlhip_group_train_steps(None, None, 0, None, 256, None, 1, None, None, 0, None),
        lambda: lib.iqlhip_group_read_losses(None, None, 1, None),
    ):
        with pytest.raises(ValueError):
            hb.check(call())
    assert out.value is None
    with pytest.raises(ValueError, match="same|again"):
        hb.check(lib.iqlhip_group_create(two_same, 2, C.byref(out)))
    with pytest.raises(ValueError, match=r"\[1,16\]"):
        hb.check(lib.iqlhip_group_create(many, hb.IQLHIP_MAX_GROUP + 1, C.byref(out)))


def _cpu_trainer(S=17, A=6):
    actor = iql.GaussianPolicy(S, A, 1.0)
    qf, vf = iql.TwinQ(S, A), iql.ValueFunction(S)
    return iql.ImplicitQLearning(max_action=1.0, actor=actor,
                                 actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                 q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                                 v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 max_steps=1000, device="cpu")


def test_group_class_validation_on_cpu_trainers():
    assert iql.ImplicitQLearningGroup is iql_offline.ImplicitQLearningGroup
    a, b = _cpu_trainer(), _cpu_trainer()
    with pytest.raises(ValueError):
        iql.ImplicitQLearningGroup([])
    with pytest.raises(ValueError):
        iql.ImplicitQLearningGroup([a] * (hb.IQLHIP_MAX_GROUP + 1))
    with pytest.raises(ValueError, match="same trainer"):
        iql.ImplicitQLearningGroup([a, b, a])
    with pytest.raises(ValueError, match="not an ImplicitQLearning"):
        iql.ImplicitQLearningGroup([a, object()])
    with pytest.raises(RuntimeError, match="GPU"):
        iql.ImplicitQLearningGroup([a, b])


def test_group_kernels_have_no_scratch_and_no_spills():
    path = os.path.join(ROOT, "jsrl-corl_amd", "libiqlhip.resources.txt")
    rows = {}
    for line in open(path):
        m = re.match(r"(\S+): (.*)$", line.strip())
        if m and "_group_kernel" in m.group(1):
            rows[m.group(1)] = dict(kv.split("=") for kv in m.group(2).split())
    names = sorted(rows)
    assert len([n for n in names if "iql_fwd_group_kernel" in n]) == 8, names
    assert len([n for n in names if "iql_bwd_group_kernel" in n]) == 4, names
    assert any("iql_update_group_kernel" in n for n in names), names
    assert any("iql_gather_group_kernel" in n for n in names), names
    for n, r in rows.items():
        assert int(r.get("ScratchSize", 0)) == 0, (n, r)
        assert int(r.get("VGPRsSpill", 0)) == 0 and int(r.get("SGPRsSpill", 0)) == 0, (n, r)
