"""CPU-only tests of the trainer groups' replay-mix calls (no GPU in the process): the two entry points are declared,
exported and bound, and reject NULL arguments before a member is looked at; ImplicitQLearningGroup validates its
arguments and buffers before any device work; the per-member n_off is Cal-QL's; and the host index draw — per member
the offline draw, then the online one, in member order — is exercised with a stub in place of the library call."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import iql
import iqlhip_binding as hb
import iqlhip_mixed as mixed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"iqlhip_group_online_step_replay2": 19, "iqlhip_group_train_steps_replay2": 13}
S, A = 17, 6


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    bound = {name: args for name, _, args in hb.SYMBOLS}
    for name, n_args in ENTRY.items():
        m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert len(bound[name]) == n_args, name
        fn = getattr(hb.lib(), name)                 # (AttributeError if the built library does not export it)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args
    assert callable(getattr(iql.ImplicitQLearningGroup, "online_step_replay_mix", None))
    assert callable(getattr(iql.ImplicitQLearningGroup, "train_steps_replay_mix", None))


def test_entry_points_reject_null_arguments_before_looking_at_a_member():
    lib = hb.lib()
    fake = 4096       # never dereferenced: every rejection below comes before the group or a member is looked at
    two_p = (C.c_void_p * 2)(fake, fake + 64)
    two_i64 = (C.c_int64 * 2)(8, 8)
    two_u64 = (C.c_uint64 * 2)(1, 2)
    two_i32 = (C.c_int32 * 2)(8, 8)
    n_off = (C.c_int32 * 2)(4, 4)
    scs = (hb.StepScalars * 2)()
    out = (C.c_float * 6)()
    calls = []
    ts = [fake, two_p, two_i64, two_p, two_i64, 44, two_i32, n_off, two_p, 2, two_u64, two_u64, None]
    for hole in (0, 1, 2, 3, 4, 6, 7, 8, 10, 11):      # group, both rows / sizes, B, n_off, tables, seeds, offsets
        args = list(ts)
        args[hole] = None
        calls.append(lambda args=args: lib.iqlhip_group_train_steps_replay2(*args))
    on = [fake, two_p, 44, two_i64, two_i64, fake, fake, two_i32, scs, out, None, None, None, None, None, None,
          two_p, two_i64, n_off]
    for hole in (0, 1, 3, 4, 5, 6, 7, 8, 9, 16, 17, 18):
        args = list(on)
        args[hole] = None
        calls.append(lambda args=args: lib.iqlhip_group_online_step_replay2(*args))
    for call in calls:
        assert call() == hb.E_INVAL
        with pytest.raises(ValueError, match="NULL"):
            hb.check(call())


def test_n_off_is_cal_ql_s_split_per_member():
    assert [mixed.split(B, r)[0] for B, r in zip((8, 64, 256), (0.25, 0.5, 0.75))] == [2, 32, 192]
    assert mixed.split(7, 0.3) == (2, 5) and mixed.split(256, 0.999) == (255, 1) and mixed.split(8, 0.125) == (1, 7)
    for B, r in ((8, 0.0), (8, 1.0), (8, 0.1), (1, 0.5)):
        with pytest.raises(ValueError, match="n_off"):
            mixed.split(B, r)


def test_draw_host_indices_from_a_generator_equals_the_global_draw():
    np.random.seed(7)
    a = mixed.draw_host_indices(300, 5, 9, 3)
    b = mixed.draw_host_indices(300, 5, 9, 3, rng=np.random.RandomState(7))
    assert all(np.array_equal(x, y) and x.dtype == np.int64 for x, y in zip(a, b))


class _Trainer:
    """What the group methods touch of a member before the library call."""
    def __init__(self):
        self._dev, self._S, self._A, self._gaussian = torch.device("cpu"), S, A, True
        self._step_stats, self._act_dropout, self._precision = False, False, "f32"
        self.actor = types.SimpleNamespace(max_action=1.0, training=False)
        self.total_it, self.prepared = 0, []

    def _prepare(self, rows):
        self.prepared.append(rows)

    def _stream(self):
        return None

    def _refuse_injected_masks(self):
        pass


class _Refused(Exception):
    pass


def _buffer(cap, fill, cls=None):
    buf = (cls or iql.ReplayBuffer)(S, A, cap, "cpu")
    buf._gpu = True          # (the checks look at the flag and at the rows' device: the members' is the CPU here)
    buf._size = fill
    return buf


def _group(K, mixed_batch=False):
    g = object.__new__(iql.ImplicitQLearningGroup)
    g.trainers, g._g, g._ctxs, g._actor_dropout, g._mixed_batch = [_Trainer() for _ in range(K)], None, None, False, mixed_batch
    g._check_members = lambda: None
    g._group = lambda: None
    g._next_scalars = lambda inv: ((hb.StepScalars * K)(), [None] * K)
    return g


def _transitions(K):
    s, a = np.zeros(S, np.float32), np.zeros(A, np.float32)
    return [s] * K, [a] * K, [0.0] * K, [s] * K, [False] * K


def _stub_lib(monkeypatch, seen):
    def online(g, rings, ld, caps, ptrs, rows, idx, n, scs, out, a_in, mask, max_a, seeds, a_out, st, offs, size_off, n_off):
        K = len(n)
        total = sum(n)
        seen["idx"] = np.ctypeslib.as_array((C.c_int64 * total).from_address(idx)).copy()
        seen["n"], seen["n_off"], seen["size_off"] = list(n), list(n_off), list(size_off)
        seen["caps"], seen["ptrs"] = list(caps), list(ptrs)
        assert K == len(n_off)
        raise _Refused()

    monkeypatch.setattr(hb, "lib", lambda: types.SimpleNamespace(iqlhip_group_online_step_replay2=online))


def test_draw_order_is_offline_then_online_in_member_order(monkeypatch):
    K, Bs, ratios = 3, [8, 4, 6], [0.25, 0.5, 0.75]
    off = _buffer(300, 300)
    rings = [_buffer(16, fill) for fill in (0, 5, 16)]
    rings[2]._pointer = 3
    new_sizes = [1, 6, 16]
    n_offs = [2, 2, 4]
    seen = {}
    _stub_lib(monkeypatch, seen)
    g = _group(K, mixed_batch=True)
    # rngs=None: the global stream, consumed exactly as K solo draws in member order consume it
    np.random.seed(11)
    with pytest.raises(_Refused):
        g.online_step_replay_mix(off, rings, *_transitions(K), Bs, ratios)
    after_group = np.random.get_state()[1].copy(), np.random.get_state()[2]
    np.random.seed(11)
    want = []
    for k in range(K):
        want.extend(mixed.draw_host_indices(300, n_offs[k], new_sizes[k], Bs[k] - n_offs[k]))
    after_solo = np.random.get_state()[1].copy(), np.random.get_state()[2]
    assert np.array_equal(seen["idx"], np.concatenate(want))
    assert np.array_equal(after_group[0], after_solo[0]) and after_group[1] == after_solo[1]
    assert seen["n"] == Bs and seen["n_off"] == n_offs and seen["size_off"] == [300] * K
    assert seen["caps"] == [16] * K and seen["ptrs"] == [0, 0, 3]
    assert [t.prepared for t in g.trainers] == [[8], [4], [6]]
    # member 0's ring was empty: every one of its online indices is the row being inserted
    assert np.all(seen["idx"][2:8] == 0)
    # the failed call moved no ring and no counter
    assert [(b._pointer, b._size, b._writes) for b in rings] == [(0, 0, 0), (0, 5, 0), (3, 16, 0)]
    assert all(t.total_it == 0 for t in g.trainers)
    # rngs: each member from its own generator, the global stream untouched
    np.random.seed(3)
    before = np.random.get_state()[1].copy(), np.random.get_state()[2]
    with pytest.raises(_Refused):
        g.online_step_replay_mix(off, rings, *_transitions(K), Bs, ratios, rngs=[np.random.RandomState(20 + k) for k in range(K)])
    assert np.array_equal(before[0], np.random.get_state()[1]) and before[1] == np.random.get_state()[2]
    want = []
    for k in range(K):
        want.extend(mixed.draw_host_indices(300, n_offs[k], new_sizes[k], Bs[k] - n_offs[k], rng=np.random.RandomState(20 + k)))
    assert np.array_equal(seen["idx"], np.concatenate(want))


def test_arguments_and_buffers_are_validated_before_any_draw_or_device_work(monkeypatch):
    K = 2
    seen = {}
    _stub_lib(monkeypatch, seen)
    off, rings = _buffer(300, 300), [_buffer(16, 4), _buffer(16, 4)]
    tr = _transitions(K)
    np.random.seed(1)
    stream0 = np.random.get_state()[1].copy(), np.random.get_state()[2]

    def refused(exc, match, g=None, off_=off, rings_=rings, B=8, ratio=0.5, burst=True, **kw):
        g = g or _group(K)
        with pytest.raises(exc, match=match):
            g.online_step_replay_mix(off_, rings_, *tr, B, ratio, **kw)
        if burst and not kw:
            with pytest.raises(exc, match=match):
                g.train_steps_replay_mix(off_, rings_, 3, B, [1, 2], ratio)
        assert not seen                                          # the library was never called
        assert all(not t.prepared and t.total_it == 0 for t in g.trainers)
        assert np.array_equal(stream0[0], np.random.get_state()[1]) and stream0[1] == np.random.get_state()[2]
        assert [(b._pointer, b._size, b._writes) for b in rings] == [(0, 4, 0), (0, 4, 0)]

    refused(ValueError, "list of 2", rings_=rings[:1])                           # wrong list lengths
    refused(ValueError, "list of 2", rings_=rings[0])                            # the online buffers are never shared
    refused(ValueError, "list of 2", off_=[off])
    refused(ValueError, "mixing ratios", ratio=[0.5])
    refused(ValueError, "batch sizes for a group of 2", B=[8, 8, 8])
    refused(ValueError, "mixed_batch", B=[8, 16])                                # unequal sizes need the option
    refused(ValueError, "n_off", ratio=0.0)                                      # n_off outside [1, B - 1] ...
    refused(ValueError, "n_off", ratio=[0.5, 1.0])                               # ... for any member
    refused(ValueError, "distinct", off_=[off, rings[1]])                        # one object in both roles (member 1)
    refused(ValueError, "finetune", off_=_buffer(16, 4, iql.OfflineReplayBuffer))
    refused(ValueError, "finetune", rings_=[rings[0], _buffer(16, 4, iql.OfflineReplayBuffer)])
    refused(ValueError, "GPU", rings_=[rings[0], iql.ReplayBuffer(S, A, 16, "cpu")])
    refused(ValueError, "GPU", off_=iql.ReplayBuffer(S, A, 16, "cpu"))
    other = iql.ReplayBuffer(S + 1, A, 16, "cpu")
    other._gpu, other._size = True, 4
    refused(ValueError, "state_dim", rings_=[rings[0], other])
    refused(ValueError, "empty", off_=_buffer(16, 0))                            # empty offline buffer
    refused(ValueError, "shares an online", rings_=[rings[0], rings[0]])         # two members, one ring
    view = _buffer(16, 4)
    view._rows = rings[0]._rows                                                  # ... or one ring's rows behind two objects
    refused(ValueError, "shares an online", rings_=[rings[0], view])
    refused(ValueError, "offline buffer", off_=[rings[1], off])                  # member 1's ring is member 0's offline buffer
    wide = _buffer(16, 4)
    wide._ld += 4
    refused(ValueError, "row strides", off_=[off, wide], rings_=[rings[0], _buffer(16, 4)])
    for name in ("act_next", "rngs"):
        refused(ValueError, name, burst=False, **{name: [None]})
    with pytest.raises(ValueError, match="2 seeds"):
        _group(K).train_steps_replay_mix(off, rings, 3, 8, [1])
    with pytest.raises(ValueError, match="n_steps"):
        _group(K).train_steps_replay_mix(off, rings, 0, 8, [1, 2])
    with pytest.raises(ValueError, match="empty"):                               # empty online buffer: the burst only
        _group(K).train_steps_replay_mix(off, [rings[0], _buffer(16, 0)], 3, 8, [1, 2])
    with pytest.raises(ValueError, match="set_step_stats"):
        _group(K).train_steps_replay_mix(off, rings, 3, 8, [1, 2], return_stats=True)
    # an empty ring is fine for the online call (the insert comes first), and per-member ratios need no option
    with pytest.raises(_Refused):
        _group(K).online_step_replay_mix(off, [rings[0], _buffer(16, 0)], *tr, 8, [0.25, 0.75])
    assert seen["n_off"] == [2, 6]


def _cpu_trainer():
    actor = iql.GaussianPolicy(S, A, 1.0)
    qf, vf = iql.TwinQ(S, A), iql.ValueFunction(S)
    return iql.ImplicitQLearning(max_action=1.0, actor=actor,
                                 actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                 q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                                 v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 max_steps=1000, device="cpu")


def test_replay_mix_on_cpu_trainers_raises():
    a, b = _cpu_trainer(), _cpu_trainer()
    g = object.__new__(iql.ImplicitQLearningGroup)
    g.trainers, g._g, g._ctxs, g._actor_dropout, g._mixed_batch = [a, b], None, None, False, False
    off, rings = _buffer(300, 300), [_buffer(16, 4), _buffer(16, 4)]
    with pytest.raises(RuntimeError, match="GPU"):
        g.online_step_replay_mix(off, rings, *_transitions(2), 8)
    with pytest.raises(RuntimeError, match="GPU"):
        g.train_steps_replay_mix(off, rings, 3, 8, [1, 2])
    assert [(x._pointer, x._size, x._writes) for x in rings] == [(0, 4, 0), (0, 4, 0)]
    assert a.total_it == 0 and b.total_it == 0
