"""CPU-only tests of ImplicitQLearningGroup.online_step_vec's host side (DESIGN.md 6b "Group vector-environment online
step"), with a stub in place of the library that records the new entry point's arguments: the member-concatenated rows,
indices and act states, the [K][U] step scalars, and what moves when the call succeeds and when it fails.  The members are
real trainers built on the CPU (real optimizers, real cosine schedules), so the scalars and the commit are the ones a GPU
run computes; only what needs a context is stubbed out.  The built library's entry point is asked for its refusals that
need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import iql
import iqlhip_binding as hb
import iqlhip_replay as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, A, CAP = 3, 2, 6
LD = 12                     # a CPU buffer's row stride at these dimensions: 2 S + A + 2 = 10 columns and 2 of padding
N_SC = C.sizeof(hb.StepScalars)


def _array(ctype, addr, n):
    return np.ctypeslib.as_array((ctype * n).from_address(addr)).copy()


class _Lib:
    """The group vector entry point, the solo one and the solo one-transition one: record the arguments, write losses
    (and actions), return rc."""
    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def iqlhip_group_online_step_vec(self, g, rings, ld, caps, ptrs, rows, n_rows, idx, Bs, U, scs, out, a_in, a_rows, max_a,
                                     seeds, a_out, stream):
        K = len(rings)
        Es, Bl = list(n_rows), list(Bs)
        E2 = [0] * K if a_rows is None else [int(x) for x in _array(C.c_int32, a_rows, K)]
        self.calls.append(dict(
            g=g, rings=list(rings), ld=ld, caps=list(caps), ptrs=list(ptrs), Es=Es, Bs=Bl, U=U,
            host=_array(C.c_float, rows, sum(Es) * ld).reshape(sum(Es), ld),
            idx=None if idx is None else _array(C.c_int64, idx, U * sum(Bl)),
            sc=[[bytes((C.c_char * N_SC).from_address(scs + (k * U + u) * N_SC)) for u in range(U)] for k in range(K)],
            E2=E2, a_in=None if a_in is None else _array(C.c_float, a_in, sum(E2) * S).reshape(sum(E2), S),
            max_a=None if max_a is None else _array(C.c_float, max_a, K),
            seeds=None if seeds is None else _array(C.c_uint64, seeds, K), a_out=a_out))
        if self.rc == 0:
            (C.c_float * max(3 * K * U, 1)).from_address(out)[:3 * K * U] = [float(v) for v in range(3 * K * U)]
            if a_out is not None:
                (C.c_float * (sum(E2) * A)).from_address(a_out)[:] = [v / 8 for v in range(sum(E2) * A)]
        return self.rc

    def iqlhip_online_step_vec(self, ctx, rows, ld, cap, pointer, rows_host, n_rows, idx, n, U, scs, out, a_in, a_rows, max_a, seed,
                               a_out, stream):
        self.calls.append(dict(solo=True, n_rows=n_rows, n=n, U=U, a_rows=a_rows,
                               idx=None if idx is None else _array(C.c_int64, idx, U * n),
                               sc=[bytes((C.c_char * N_SC).from_address(scs + u * N_SC)) for u in range(U)]))
        if a_out is not None:
            (C.c_float * (a_rows * A)).from_address(a_out)[:] = [0.5] * (a_rows * A)
        return self.rc

    def iqlhip_last_error(self):
        return b"stub"


def _lib(monkeypatch, rc=0):
    lib = _Lib(rc)
    monkeypatch.setattr(hb, "lib", lambda: lib)
    return lib


def _trainer(seed, adam0, max_steps=50):
    """A real trainer on the CPU that passes for one with a context: adam0 steps into its Adam counts and schedule."""
    torch.manual_seed(seed)
    qf, vf, actor = iql.TwinQ(S, A), iql.ValueFunction(S), iql.GaussianPolicy(S, A, 1.5)
    tr = iql.ImplicitQLearning(max_action=1.5, actor=actor, actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                               q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=2e-4), v_network=vf,
                               v_optimizer=torch.optim.Adam(vf.parameters(), lr=1e-4), max_steps=max_steps, device="cpu")
    tr._dev, tr._S, tr._A, tr._gaussian = torch.device("cpu"), S, A, True
    tr._ctx = C.c_void_p(4096 + seed)          # (never handed to the built library: _release is stubbed out too)
    tr._release = lambda: None
    tr.prepared = []
    tr._require_gpu = lambda: None
    tr._prepare = tr.prepared.append
    tr._prepare_act = lambda: None
    tr._stream = lambda: None
    tr._advance_schedule(adam0)
    tr.total_it, tr._adam_t = adam0, {g: adam0 for g in ("v", "q", "pi")}
    return tr


def _group(K=2, mixed_batch=False):
    g = iql.ImplicitQLearningGroup([_trainer(k, 3 + 10 * k) for k in range(K)], mixed_batch=mixed_batch)
    g._group = lambda: 77
    return g


def _ring(size, pointer, cls=R.ReplayBuffer):
    buf = cls(S, A, CAP, "cpu")
    buf._gpu, buf._size, buf._pointer = True, size, pointer
    return buf


def _block(E, lo=0):
    rng = np.random.default_rng(100 + lo)
    return (rng.standard_normal((E, S)), rng.standard_normal((E, A)), rng.standard_normal(E), rng.standard_normal((E, S)),
            rng.random(E) < 0.5)


def _packed(block):
    s, a, r, ns, d = block
    rows = np.zeros((len(s), LD), dtype=np.float32)
    rows[:, :S], rows[:, S:S + A], rows[:, S + A:2 * S + A] = s, a, ns
    rows[:, 2 * S + A], rows[:, 2 * S + A + 1] = r, d
    return rows


def _args(blocks):
    """The K blocks as the five per-member lists the group call takes."""
    return tuple([b[j] for b in blocks] for j in range(5))


def _rng_state(rng=None):
    st = np.random.get_state() if rng is None else rng.get_state()
    return st[1].copy(), st[2]


def _same_rng(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1]


def _state(tr, ring):
    sch = tr.actor_lr_schedule
    return (tr.total_it, dict(tr._adam_t), tr.actor_optimizer.param_groups[0]["lr"], sch.last_epoch, sch._step_count,
            ring._writes, ring._pointer, ring._size)


ACT = [np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]]), None, np.array([[0.7, 0.8, 0.9]])]


def test_member_concatenated_arguments_and_the_commit(monkeypatch):
    lib, g = _lib(monkeypatch), _group(3, mixed_batch=True)
    rings = [_ring(2, 2), _ring(CAP, 5), _ring(0, 0)]
    blocks, Bs, U = [_block(1), _block(3, 1), _block(2, 2)], [4, 5, 7], 2
    sizes = [3, CAP, 2]                                          # every member's size after all of its inserts
    np.random.seed(3)
    want = [np.random.randint(0, sizes[k], size=Bs[k]) for k in range(3) for _ in range(U)]
    rng_after = _rng_state()
    np.random.seed(3)
    logs, acts = g.online_step_vec(rings, *_args(blocks), Bs, updates=U, act_next=ACT)
    (c,) = lib.calls
    assert c["g"] == 77 and c["ld"] == LD and c["U"] == U
    assert c["rings"] == [r._rows.data_ptr() for r in rings] and c["caps"] == [CAP] * 3 and c["ptrs"] == [2, 5, 0]
    assert c["Es"] == [1, 3, 2] and c["Bs"] == Bs
    assert c["host"].dtype == np.float32 and np.array_equal(c["host"], np.concatenate([_packed(b) for b in blocks]))
    assert c["idx"].dtype == np.int64 and np.array_equal(c["idx"], np.concatenate(want))          # k outer, u inner
    assert _same_rng(_rng_state(), rng_after)
    assert c["E2"] == [2, 0, 1] and np.array_equal(c["a_in"], np.concatenate([ACT[0], ACT[2]]).astype(np.float32))
    assert np.array_equal(c["max_a"], np.float32([1.5] * 3))
    assert [int(s) for s in c["seeds"]] == [g.trainers[0]._act_seed(), 0, g.trainers[2]._act_seed()] and c["seeds"][0] != 0
    # the return value: [K][U] dicts from out[k][u][3]; the actions split by E2_k, None for the member that asked for none
    assert logs == [[{"value_loss": 3.0 * (k * U + u), "q_loss": 3.0 * (k * U + u) + 1, "actor_loss": 3.0 * (k * U + u) + 2}
                     for u in range(U)] for k in range(3)]
    flat = (np.arange(3 * A, dtype=np.float32) / 8).reshape(3, A)
    assert acts[1] is None and np.array_equal(acts[0], flat[:2]) and np.array_equal(acts[2], flat[2:])
    assert acts[0].dtype == np.float32
    # the commit: every ring by its E_k (wrapping), every member by U steps
    assert [(r._writes, r._pointer, r._size) for r in rings] == [(1, 3, 3), (3, 2, CAP), (2, 2, 2)]
    for k, t in enumerate(g.trainers):
        assert t.total_it == 3 + 10 * k + U and t._adam_t == {x: 3 + 10 * k + U for x in ("v", "q", "pi")}
        assert (t.actor_lr_schedule.last_epoch, t.actor_lr_schedule._step_count) == (3 + 10 * k + U, 4 + 10 * k + U)
        assert t.prepared == [Bs[k]]


@pytest.mark.parametrize("U", [1, 4])
def test_scalars_and_draws_equal_those_of_the_solo_calls_in_member_order(U, monkeypatch):
    lib = _lib(monkeypatch)
    g, twins = _group(2), [_trainer(k, 3 + 10 * k) for k in range(2)]
    rings_g, rings_t = [_ring(CAP, 1), _ring(3, 3)], [_ring(CAP, 1), _ring(3, 3)]
    blocks, B = [_block(2), _block(1, 1)], 5
    np.random.seed(8)
    g.online_step_vec(rings_g, *_args(blocks), B, updates=U)
    np.random.seed(8)
    for t, ring, blk in zip(twins, rings_t, blocks):
        t.online_step_vec(ring, *blk, B, updates=U)
    got, solos = lib.calls[0], lib.calls[1:]
    assert [c.get("solo") for c in solos] == [True, True]
    assert got["sc"] == [c["sc"] for c in solos]                          # [K][U], bit for bit
    assert len({s for member in got["sc"] for s in member}) == 2 * U      # (and they differ from step to step, member to member)
    assert np.array_equal(got["idx"], np.concatenate([c["idx"] for c in solos]))
    for k in range(2):
        assert _state(g.trainers[k], rings_g[k]) == _state(twins[k], rings_t[k])


def test_draws_come_from_the_members_generators(monkeypatch):
    lib, g = _lib(monkeypatch), _group(2)
    rings, blocks, B, U = [_ring(CAP, 1), _ring(2, 2)], [_block(2), _block(2, 1)], 4, 3
    rngs = [np.random.RandomState(11), np.random.RandomState(12)]
    twins = [np.random.RandomState(11), np.random.RandomState(12)]
    want = [twins[k].randint(0, (CAP, 4)[k], size=B) for k in range(2) for _ in range(U)]
    np.random.seed(1)
    glob = _rng_state()
    g.online_step_vec(rings, *_args(blocks), B, updates=U, rngs=rngs)
    assert np.array_equal(lib.calls[0]["idx"], np.concatenate(want))
    assert _same_rng(_rng_state(), glob)                                   # the global stream is not touched
    after = np.random.RandomState(11)
    for _ in range(U):
        after.randint(0, CAP, size=B)
    assert _same_rng(_rng_state(rngs[0]), _rng_state(after))


def test_failed_call_moves_nothing(monkeypatch):
    lib, g = _lib(monkeypatch, rc=hb.E_INVAL), _group(2)
    rings = [_ring(CAP, 3), _ring(1, 1)]
    s0 = [_state(t, r) for t, r in zip(g.trainers, rings)]
    with pytest.raises(ValueError, match="stub"):
        g.online_step_vec(rings, *_args([_block(3), _block(2)]), 5, updates=3, act_next=ACT[:2])
    assert len(lib.calls) == 1 and [_state(t, r) for t, r in zip(g.trainers, rings)] == s0


def test_no_updates_draws_nothing_and_moves_no_step_counter(monkeypatch):
    lib, g = _lib(monkeypatch), _group(2)
    rings = [_ring(0, 0), _ring(CAP, 4)]
    s0 = [_state(t, r) for t, r in zip(g.trainers, rings)]
    np.random.seed(2)
    rng0 = _rng_state()
    assert g.online_step_vec(rings, *_args([_block(2), _block(3)]), 256, updates=0) == [[], []]
    logs, acts = g.online_step_vec(rings, *_args([_block(1), _block(1)]), 256, updates=0, act_next=[None, ACT[2]])
    assert logs == [[], []] and acts[0] is None and acts[1].shape == (1, A)
    assert _same_rng(_rng_state(), rng0)
    assert all(c["idx"] is None and c["U"] == 0 and c["sc"] == [[], []] for c in lib.calls)
    assert [c["ptrs"] for c in lib.calls] == [[0, 4], [2, 1]]
    assert [_state(t, r) for t, r in zip(g.trainers, rings)] == [s0[0][:5] + (3, 3, 3), s0[1][:5] + (4, 2, CAP)]


def test_a_group_of_one_delegates_to_the_solo_call(monkeypatch):
    lib, g = _lib(monkeypatch), _group(1)
    ring = _ring(2, 2)
    np.random.seed(4)
    logs, acts = g.online_step_vec([ring], *_args([_block(2)]), 5, updates=2, act_next=[ACT[0]])
    (c,) = lib.calls
    assert c.get("solo") and (c["n_rows"], c["n"], c["U"], c["a_rows"]) == (2, 5, 2, 2)
    assert len(logs) == 1 and len(logs[0]) == 2 and acts[0].shape == (2, A)
    assert g.online_step_vec([ring], *_args([_block(1)]), 5, updates=0) == [[]]
    logs, acts = g.online_step_vec([ring], *_args([_block(1)]), 5, updates=1, act_next=[None])
    assert len(logs[0]) == 1 and acts == [None]
    # ... but with generators of its own the group call is made
    g.online_step_vec([ring], *_args([_block(1)]), 5, updates=1, rngs=[np.random.RandomState(0)])
    assert "solo" not in lib.calls[-1] and lib.calls[-1]["Es"] == [1]


def test_every_refusal_comes_before_the_library_the_draw_and_the_commit(monkeypatch):
    lib, g = _lib(monkeypatch), _group(2)
    rings = [_ring(2, 2), _ring(3, 3)]
    blocks = [_block(3), _block(2, 1)]
    ok = _args(blocks)
    np.random.seed(1)
    rng0 = _rng_state()
    s0 = [_state(t, r) for t, r in zip(g.trainers, rings)]

    def refused(exc, bufs, args, B=5, match=None, **kw):
        with pytest.raises(exc, match=match):
            g.online_step_vec(bufs, *args, B, **kw)
        assert not lib.calls and _same_rng(_rng_state(), rng0)
        assert [_state(t, r) for t, r in zip(g.trainers, rings)] == s0
        assert all(t.prepared == [] for t in g.trainers)          # no member's settings were sent either

    def with_block(k, blk):
        return _args([blk if i == k else b for i, b in enumerate(blocks)])

    refused(ValueError, rings[:1], ok, match="list of 2")
    refused(ValueError, rings, ok, act_next=[ACT[0]], match="act_next")
    refused(ValueError, rings, ok, rngs=[np.random.RandomState(0)], match="rngs")
    refused(ValueError, rings, with_block(1, _block(CAP + 1)), match="member 1")               # E > capacity
    refused(ValueError, rings, with_block(0, tuple(x[:0] for x in blocks[0])), match="member 0")   # E = 0
    refused(ValueError, rings, ok, updates=hb.IQLHIP_VEC_MAX_UPDATES + 1)
    refused(ValueError, rings, ok, updates=-1)
    refused(ValueError, rings, ok, B=0)
    refused(ValueError, rings, ok, B=513)
    refused(ValueError, rings, ok, B=[4, 5])                                                   # unequal, not a mixed_batch group
    refused(ValueError, rings, ok, B=[5, 5, 5])
    b1 = blocks[1]
    refused(ValueError, rings, with_block(1, (b1[0], b1[1], b1[2][:1], b1[3], b1[4])), match="member 1")   # shapes that disagree
    refused(ValueError, rings, with_block(1, (b1[0][:, :2],) + b1[1:]), match="member 1")
    refused(ValueError, rings, ok, act_next=[None, np.zeros((hb.IQLHIP_VEC_MAX_ENVS + 1, S))], match="member 1")
    refused(ValueError, rings, ok, act_next=[np.zeros(S), None], match="member 0")
    refused(ValueError, [rings[0], R.ReplayBuffer(S, A, CAP, "cpu")], ok, match="member 1")    # a CPU ring
    refused(NotImplementedError, [rings[0], _ring(3, 3, cls=R.OfflineReplayBuffer)], ok, match="member 1")
    refused(ValueError, [rings[0], rings[0]], ok, match="member 1 shares")
    tracked = _ring(3, 3)
    tracked._weights_tracks = True
    refused(NotImplementedError, [rings[0], tracked], ok, match="member 1")
    t1 = g.trainers[1]
    for world, exchange in ((2, "rccl"), (1, "p2p")):
        t1._dp_world, t1._dp_exchange = world, exchange
        refused(NotImplementedError, rings, ok, match="member 1")
    t1._dp_world, t1._dp_exchange = 1, None
    t1._masks_injected = True
    refused(NotImplementedError, rings, ok, match="member 1")
    t1._masks_injected = False
    for t in g.trainers:
        t._precision = "bf16"
    refused(NotImplementedError, rings, ok, B=513)
    for t in g.trainers:
        t._precision = "f32"
    t1.actor_lr_schedule.eta_min = 1e-5               # a schedule only torch should advance: no rates to look up ahead
    refused(NotImplementedError, rings, ok, updates=2, match="member 1")
    t1.actor_lr_schedule.eta_min = 0
    actor = t1.actor
    t1.actor = iql.GaussianPolicy(S, A, 1.5, dropout=0.1)                                    # training mode, dropout
    refused(NotImplementedError, rings, ok, match="member 1")                                 # ... in a group without actor_dropout
    g._actor_dropout = True
    refused(NotImplementedError, rings, ok, act_next=[None, ACT[2]], match="member 1")        # ... acting without set_act_dropout(True)
    g.online_step_vec(rings, *ok, 5, act_next=[ACT[0], None])                                 # the other member may act
    assert len(lib.calls) == 1
    t1.actor = actor


def test_header_binding_and_library_agree_on_the_new_symbol():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    bound = {name: (res, args) for name, res, args in hb.SYMBOLS}
    name, n_args = "iqlhip_group_online_step_vec", 18
    m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m and len(m.group(1).split(",")) == n_args
    assert bound[name][0] is C.c_int and len(bound[name][1]) == n_args
    fn = getattr(hb.lib(), name)                     # (AttributeError if the built library does not export it)
    assert fn.restype is C.c_int and len(fn.argtypes) == n_args
    assert callable(getattr(iql.ImplicitQLearningGroup, "online_step_vec", None))


def test_entry_point_rejects_null_and_out_of_range_arguments_before_any_device_work():
    """The refusals that need no group are answered on a machine without a GPU (nothing is launched), with a message."""
    lib, K, ptr = hb.lib(), 2, 4096           # never dereferenced: a non-NULL, 16-byte aligned address
    rings, caps, ptrs = (C.c_void_p * K)(ptr, 2 * ptr), (C.c_int64 * K)(8, 8), (C.c_int64 * K)(0, 0)
    n_rows, Bs = (C.c_int32 * K)(3, 2), (C.c_int32 * K)(5, 5)
    rows, idx = np.zeros((5, LD), dtype=np.float32), np.zeros(2 * 10, dtype=np.int64)
    scs, out = (hb.StepScalars * (2 * K))(), (C.c_float * (6 * K))()
    a_in, a_out = np.zeros((2, S), dtype=np.float32), np.zeros((2, A), dtype=np.float32)
    a_rows, max_a, seeds = np.ones(K, dtype=np.int32), np.ones(K, dtype=np.float32), np.zeros(K, dtype=np.uint64)
    full = dict(g=1, rings=rings, ld=LD, caps=caps, ptrs=ptrs, rows=rows.ctypes.data, n_rows=n_rows, idx=idx.ctypes.data,
                Bs=Bs, U=2, sc=C.addressof(scs), out=C.addressof(out), a_in=None, a_rows=None, max_a=None, seeds=None,
                a_out=None, st=None)
    act = dict(a_in=a_in.ctypes.data, a_rows=a_rows.ctypes.data, max_a=max_a.ctypes.data, seeds=seeds.ctypes.data,
               a_out=a_out.ctypes.data)
    for bad in (dict(g=None), dict(rings=None), dict(caps=None), dict(ptrs=None), dict(rows=None), dict(n_rows=None),
                dict(Bs=None), dict(idx=None), dict(sc=None), dict(out=None), dict(U=-1), dict(U=hb.IQLHIP_VEC_MAX_UPDATES + 1),
                dict(act, a_rows=None), dict(act, max_a=None), dict(act, seeds=None), dict(act, a_out=None)):
        a = dict(full, **bad)
        assert lib.iqlhip_group_online_step_vec(*a.values()) == hb.E_INVAL, bad
        assert hb.last_error(), bad
