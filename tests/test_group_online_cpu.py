"""CPU-only tests of the group online step (no GPU in the process): the library exports iqlhip_group_online_step and
rejects NULL arguments before any device work; ImplicitQLearningGroup.online_step checks its arguments and refuses
trainers that live on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import iql
import iqlhip_binding as hb


def test_group_online_symbol_is_exported():
    lib = hb.lib()
    fn = lib.iqlhip_group_online_step
    assert fn.restype is C.c_int and len(fn.argtypes) == 16


def test_group_online_entry_point_rejects_null_arguments():
    lib = hb.lib()
    K, S, A, B = 2, 17, 6, 4
    ld = hb.row_stride(S, A)
    rings = (C.c_void_p * K)(4096, 8192)      # never dereferenced: every call below is refused first
    caps = (C.c_int64 * K)(10, 10)
    ptrs = (C.c_int64 * K)(0, 0)
    rows = np.zeros((K, ld), dtype=np.float32)
    idx = np.zeros((K, B), dtype=np.int64)
    scs = (hb.StepScalars * K)()
    out = (C.c_float * (3 * K))()
    a_in = np.zeros((K, S), dtype=np.float32)
    a_out = np.zeros((K, A), dtype=np.float32)
    max_a = np.ones(K, dtype=np.float32)
    seeds = np.zeros(K, dtype=np.uint64)
    full = dict(g=None, rings=rings, ld=ld, caps=caps, ptrs=ptrs, rows=rows.ctypes.data, idx=idx.ctypes.data, n=B,
                sc=scs, out=out, a_in=None, mask=None, max_a=None, seeds=None, a_out=None, st=None)

    def call(**kw):
        a = dict(full, **kw)
        return lib.iqlhip_group_online_step(*a.values())

    for kw in ({}, dict(g=1, rings=None), dict(g=1, caps=None), dict(g=1, ptrs=None), dict(g=1, rows=None),
               dict(g=1, idx=None), dict(g=1, sc=None), dict(g=1, out=None),
               # act states without somewhere to put the actions, or without their max_action / seeds
               dict(g=1, a_in=a_in.ctypes.data, max_a=max_a.ctypes.data, seeds=seeds.ctypes.data),
               dict(g=1, a_in=a_in.ctypes.data, a_out=a_out.ctypes.data, seeds=seeds.ctypes.data),
               dict(g=1, a_in=a_in.ctypes.data, a_out=a_out.ctypes.data, max_a=max_a.ctypes.data)):
        with pytest.raises(ValueError):
            hb.check(call(**kw))
    assert "NULL" in hb.last_error() or "act_state_host" in hb.last_error()


def _cpu_trainer(S=17, A=6):
    actor = iql.GaussianPolicy(S, A, 1.0)
    qf, vf = iql.TwinQ(S, A), iql.ValueFunction(S)
    return iql.ImplicitQLearning(max_action=1.0, actor=actor,
                                 actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                 q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                                 v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 max_steps=1000, device="cpu")


def test_group_online_step_on_cpu_trainers_raises():
    a, b = _cpu_trainer(), _cpu_trainer()
    assert callable(getattr(iql.ImplicitQLearningGroup, "online_step", None))
    with pytest.raises(RuntimeError, match="GPU"):        # a group of CPU trainers cannot be formed at all
        iql.ImplicitQLearningGroup([a, b])
    # ... and a group object that holds them anyway refuses the online step before it touches anything
    g = object.__new__(iql.ImplicitQLearningGroup)
    g.trainers, g._g, g._ctxs = [a, b], None, None
    bufs = [iql.ReplayBuffer(17, 6, 8, "cpu"), iql.ReplayBuffer(17, 6, 8, "cpu")]
    s, act = np.zeros(17, np.float32), np.zeros(6, np.float32)
    args = (bufs, [s, s], [act, act], [0.0, 0.0], [s, s], [False, False], 4)
    with pytest.raises(ValueError, match="list of 2"):
        g.online_step(bufs[:1], *args[1:])
    with pytest.raises(ValueError, match="act_next"):
        g.online_step(*args, act_next=[s])
    with pytest.raises(ValueError, match="rngs"):
        g.online_step(*args, rngs=[np.random.RandomState(0)])
    with pytest.raises(RuntimeError, match="GPU"):
        g.online_step(*args)
    assert [(b._pointer, b._size) for b in bufs] == [(0, 0), (0, 0)]
    assert a.total_it == 0 and b.total_it == 0
