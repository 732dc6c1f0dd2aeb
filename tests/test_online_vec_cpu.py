"""CPU-only tests of ReplayBuffer.add_transitions and of ImplicitQLearning.online_step_vec's host side,
with a stub in place of the library that records the new entry point's arguments: the E packed rows, the U * B host
indices and the generator they come from, the U sets of step scalars, the act arguments, and what moves when the call
succeeds and when it fails.  The trainer is a real one built on the CPU (real optimizers, real cosine schedule), so the
scalars and the commit are the ones a GPU run computes; only what needs a context is stubbed out."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import iql
import iqlhip_binding as hb
import iqlhip_replay as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, A, CAP, B = 3, 2, 4, 5
LD = 12                     # a CPU buffer's row stride at these dimensions: 2 S + A + 2 = 10 columns and 2 of padding
ACTIONS = np.arange(2 * A, dtype=np.float32).reshape(2, A) / 8      # what the stub's act forward answers for two states


def _scalars(addr, n):
    return [bytes((C.c_char * C.sizeof(hb.StepScalars)).from_address(addr + u * C.sizeof(hb.StepScalars))) for u in range(n)]


class _Lib:
    """The vector entry point and the one-transition one: record the arguments, write losses (and actions), return rc."""
    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def iqlhip_online_step_vec(self, ctx, rows, ld, cap, pointer, rows_host, n_rows, idx, n, U, scs, out, a_in, a_rows, max_a, seed,
                               a_out, stream):
        host = np.ctypeslib.as_array((C.c_float * (n_rows * ld)).from_address(rows_host)).reshape(n_rows, ld).copy()
        self.calls.append(dict(rows=rows, ld=ld, cap=cap, pointer=pointer, host=host, n=n, U=U,
                               idx=None if idx is None else np.ctypeslib.as_array((C.c_int64 * (U * n)).from_address(idx)).copy(),
                               sc=_scalars(scs, U), max_a=max_a, seed=seed, a_rows=a_rows, a_out=a_out,
                               a_in=None if a_in is None else
                               np.ctypeslib.as_array((C.c_float * (a_rows * S)).from_address(a_in)).reshape(a_rows, S).copy()))
        if self.rc == 0:
            (C.c_float * (3 * max(U, 1))).from_address(out)[:3 * U] = [10.0 * (u // 3) + u % 3 for u in range(3 * U)]
            if a_out is not None:
                (C.c_float * (a_rows * A)).from_address(a_out)[:] = list(ACTIONS[:a_rows].reshape(-1))
        return self.rc

    def iqlhip_online_step(self, ctx, rows, ld, cap, pointer, row, idx, n, sc, out, a_in, max_a, seed, a_out, stream):
        self.calls.append(dict(sc=bytes(sc._obj), idx=np.ctypeslib.as_array((C.c_int64 * n).from_address(idx)).copy()))
        out[0], out[1], out[2] = 1.0, 2.0, 3.0
        return self.rc

    def iqlhip_last_error(self):
        return b"stub"


def _lib(monkeypatch, rc=0):
    lib = _Lib(rc)
    monkeypatch.setattr(hb, "lib", lambda: lib)
    return lib


def _trainer(max_steps=50, adam0=3):
    """A real trainer on the CPU that passes for one with a context: three steps into its Adam counts and schedule."""
    torch.manual_seed(0)
    qf, vf, actor = iql.TwinQ(S, A), iql.ValueFunction(S), iql.GaussianPolicy(S, A, 1.5)
    tr = iql.ImplicitQLearning(max_action=1.5, actor=actor, actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                               q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=2e-4), v_network=vf,
                               v_optimizer=torch.optim.Adam(vf.parameters(), lr=1e-4), max_steps=max_steps, device="cpu")
    tr._dev, tr._S, tr._A, tr._gaussian = torch.device("cpu"), S, A, True
    tr._on_row = np.zeros(LD, dtype=np.float32)
    tr.prepared = []
    tr._require_gpu = lambda: None
    tr._prepare = tr.prepared.append
    tr._prepare_act = lambda: None
    tr._stream = lambda: None
    tr._advance_schedule(adam0)
    tr.total_it, tr._adam_t = adam0, {g: adam0 for g in ("v", "q", "pi")}
    return tr


def _ring(size=2, pointer=2, cls=R.ReplayBuffer):
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


def _rng_state():
    st = np.random.get_state()
    return st[1].copy(), st[2]


def _same_rng(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1]


def _state(tr, ring):
    sch = tr.actor_lr_schedule
    return (tr.total_it, dict(tr._adam_t), tr.actor_optimizer.param_groups[0]["lr"], sch.last_epoch, sch._step_count,
            ring._writes, ring._pointer, ring._size)


ACT_NEXT = np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]])


def test_rows_indices_act_arguments_and_commit(monkeypatch):
    lib, tr, ring = _lib(monkeypatch), _trainer(), _ring(size=2, pointer=2)
    blk, U = _block(3), 2
    np.random.seed(3)
    want = [np.random.randint(0, CAP, size=B) for _ in range(U)]          # U sample() draws over the size after 3 inserts
    rng_after = _rng_state()
    np.random.seed(3)
    lr0 = tr.actor_optimizer.param_groups[0]["lr"]
    logs, acts = tr.online_step_vec(ring, *blk, B, updates=U, act_next=ACT_NEXT)
    (c,) = lib.calls
    assert (c["rows"], c["ld"], c["cap"], c["pointer"]) == (ring._rows.data_ptr(), LD, CAP, 2) and (c["n"], c["U"]) == (B, U)
    assert c["host"].dtype == np.float32 and np.array_equal(c["host"], _packed(blk))          # row order, pads zero
    assert c["idx"].dtype == np.int64 and np.array_equal(c["idx"], np.concatenate(want))
    assert _same_rng(_rng_state(), rng_after)
    assert c["a_rows"] == 2 and np.array_equal(c["a_in"], ACT_NEXT.astype(np.float32)) and c["max_a"] == 1.5
    assert c["seed"] == tr._act_seed() != 0
    assert logs == [{"value_loss": 0.0, "q_loss": 1.0, "actor_loss": 2.0}, {"value_loss": 10.0, "q_loss": 11.0, "actor_loss": 12.0}]
    assert acts.shape == (2, A) and acts.dtype == np.float32 and np.array_equal(acts, ACTIONS) and c["a_out"] == acts.ctypes.data
    # the commit: the ring by E = 3 (wrapping), the step counters and the schedule by U = 2
    assert (ring._writes, ring._pointer, ring._size) == (3, 1, CAP)
    assert tr.total_it == 5 and tr._adam_t == {"v": 5, "q": 5, "pi": 5}
    assert (tr.actor_lr_schedule.last_epoch, tr.actor_lr_schedule._step_count) == (5, 6)
    assert tr.actor_optimizer.param_groups[0]["lr"] < lr0 and tr.prepared == [B]


@pytest.mark.parametrize("U", [1, 4])
def test_scalars_equal_those_of_single_steps(U, monkeypatch):
    lib = _lib(monkeypatch)
    vec, one = _trainer(), _trainer()
    ring_v, ring_o = _ring(size=CAP, pointer=1), _ring(size=CAP, pointer=1)
    np.random.seed(8)
    vec.online_step_vec(ring_v, *_block(1), B, updates=U)
    np.random.seed(8)
    s, a, r, ns, d = _block(1)
    for u in range(U):
        one.online_step(ring_o, s[0], a[0], r[0], ns[0], d[0], B)
    got, singles = lib.calls[0], lib.calls[1:]
    assert len(got["sc"]) == U == len(singles)
    assert got["sc"] == [c["sc"] for c in singles]                      # bit for bit, step by step
    assert len(set(got["sc"])) == U                                      # (and they do differ from step to step)
    assert np.array_equal(got["idx"], np.concatenate([c["idx"] for c in singles]))
    assert _state(vec, ring_v)[:5] == _state(one, ring_o)[:5]          # the counters and the schedule end up alike


def test_failed_call_moves_nothing(monkeypatch):
    lib, tr, ring = _lib(monkeypatch, rc=hb.E_INVAL), _trainer(), _ring(size=CAP, pointer=3)
    s0 = _state(tr, ring)
    with pytest.raises(ValueError, match="stub"):
        tr.online_step_vec(ring, *_block(3), B, updates=3, act_next=ACT_NEXT)
    assert len(lib.calls) == 1 and _state(tr, ring) == s0


def test_no_updates_draws_nothing_and_moves_no_step_counter(monkeypatch):
    lib, tr, ring = _lib(monkeypatch), _trainer(), _ring(size=0, pointer=0)
    s0 = _state(tr, ring)
    np.random.seed(2)
    rng0 = _rng_state()
    assert tr.online_step_vec(ring, *_block(2), B, updates=0) == []
    logs, acts = tr.online_step_vec(ring, *_block(2, lo=2), 256, updates=0, act_next=ACT_NEXT[:1])
    assert logs == [] and np.array_equal(acts, ACTIONS[:1])
    assert _same_rng(_rng_state(), rng0)
    assert all(c["idx"] is None and c["U"] == 0 and c["sc"] == [] for c in lib.calls)
    assert [c["pointer"] for c in lib.calls] == [0, 2]
    assert _state(tr, ring) == s0[:5] + (4, 0, 4)


def test_every_refusal_comes_before_the_library_the_draw_and_the_commit(monkeypatch):
    lib, tr, ring = _lib(monkeypatch), _trainer(), _ring(size=2, pointer=2)
    blk = _block(3)
    np.random.seed(1)
    rng0, s0 = _rng_state(), _state(tr, ring)

    def refused(exc, buf, *args, **kw):
        with pytest.raises(exc):
            tr.online_step_vec(buf, *args, **kw)
        assert not lib.calls and _same_rng(_rng_state(), rng0) and _state(tr, ring) == s0

    refused(ValueError, ring, *_block(5), B)                                         # E > capacity
    refused(ValueError, _ring(), *(x[:0] for x in blk), B)                            # E = 0
    refused(ValueError, ring, *blk, B, updates=hb.IQLHIP_VEC_MAX_UPDATES + 1)
    refused(ValueError, ring, *blk, B, updates=-1)
    refused(ValueError, ring, *blk, 0)
    refused(ValueError, ring, *blk, 513)
    refused(ValueError, ring, blk[0], blk[1], blk[2][:2], blk[3], blk[4], B)          # shapes that disagree
    refused(ValueError, ring, blk[0][:, :2], *blk[1:], B)
    refused(ValueError, ring, *blk, B, act_next=np.zeros((hb.IQLHIP_VEC_MAX_ENVS + 1, S)))
    refused(ValueError, ring, *blk, B, act_next=np.zeros(S))
    refused(ValueError, R.ReplayBuffer(S, A, CAP, "cpu"), *blk, B)                    # a CPU ring
    tr._dev = torch.device("meta")
    refused(ValueError, ring, *blk, B)                                               # a ring on another device
    tr._dev = torch.device("cpu")
    refused(NotImplementedError, _ring(cls=R.OfflineReplayBuffer), *blk, B)
    for world, exchange in ((2, "rccl"), (2, "torch"), (1, "p2p")):
        tr._dp_world, tr._dp_exchange = world, exchange
        refused(NotImplementedError, ring, *blk, B)
    tr._dp_world, tr._dp_exchange = 1, None
    tr._masks_injected = True
    refused(NotImplementedError, ring, *blk, B)
    tr._masks_injected = False
    tr._precision = "bf16"
    refused(NotImplementedError, ring, *blk, 513)
    tr._precision = "f32"
    tracked = _ring()
    tracked._weights_tracks = True
    refused(NotImplementedError, tracked, *blk, B)
    tr.actor = iql.GaussianPolicy(S, A, 1.5, dropout=0.1)                            # training mode, no set_act_dropout(True)
    refused(NotImplementedError, ring, *blk, B, act_next=ACT_NEXT)
    tr.online_step_vec(ring, *blk, B)                                                # without act_next it runs
    assert len(lib.calls) == 1


@pytest.mark.parametrize("S_, A_", [(3, 2), (17, 6)])
def test_add_transitions_on_a_cpu_buffer_equals_single_inserts(S_, A_):
    a, b = R.ReplayBuffer(S_, A_, 8, "cpu"), R.ReplayBuffer(S_, A_, 8, "cpu")
    rng = np.random.default_rng(4)
    for it, E in enumerate([3, 3, 3, 3, 8, 1]):          # wraps inside the third call; then the whole ring at once
        blk = (rng.standard_normal((E, S_)), rng.standard_normal((E, A_)).tolist(), rng.standard_normal(E),
               rng.standard_normal((E, S_)).astype(np.float32), rng.random((E, 1)) < 0.5)
        a.add_transitions(*blk)
        for e in range(E):
            b.add_transition(blk[0][e], blk[1][e], blk[2][e], blk[3][e], bool(blk[4][e]))
        assert torch.equal(a._rows, b._rows), it
        assert (a._pointer, a._size, a._writes) == (b._pointer, b._size, b._writes), it
    assert (a._pointer, a._size, a._writes) == (5, 8, 21)


def test_add_transitions_refuses_bad_sizes_and_the_offline_flavour():
    buf = R.ReplayBuffer(S, A, CAP, "cpu")
    s, a, r, ns, d = _block(5)
    for bad in ((s, a, r, ns, d), (s[:0], a[:0], r[:0], ns[:0], d[:0]), (s[:2], a[:3], r[:2], ns[:2], d[:2]),
                (s[:2], a[:2], r[:3], ns[:2], d[:2]), (s[0], a[0], r[0], ns[0], d[0])):
        with pytest.raises(ValueError):
            buf.add_transitions(*bad)
    big = R.ReplayBuffer(S, A, 100, "cpu")
    with pytest.raises(ValueError):
        big.add_transitions(*_block(hb.IQLHIP_VEC_MAX_ENVS + 1))
    big.add_transitions(*_block(hb.IQLHIP_VEC_MAX_ENVS))
    assert (buf._pointer, buf._size, buf._writes) == (0, 0, 0) and (big._pointer, big._size, big._writes) == (64, 64, 64)
    with pytest.raises(NotImplementedError):
        R.OfflineReplayBuffer(S, A, CAP, "cpu").add_transitions(*_block(2))


def test_header_binding_and_library_agree_on_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    bound = {name: (res, args) for name, res, args in hb.SYMBOLS}
    for name, n_args in (("iqlhip_rows_write_ring", 7), ("iqlhip_online_step_vec", 18)):
        m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m and len(m.group(1).split(",")) == n_args
        assert bound[name][0] is C.c_int and len(bound[name][1]) == n_args
        fn = getattr(hb.lib(), name)                     # (AttributeError if the built library does not export it)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args
    for const, value in (("IQLHIP_VEC_MAX_ENVS", 64), ("IQLHIP_VEC_MAX_UPDATES", 32)):
        m = re.search(r"#define\s+" + const + r"\s+(\d+)", header)
        assert m and int(m.group(1)) == getattr(hb, const) == value
    assert callable(getattr(iql.ImplicitQLearning, "online_step_vec", None))
    assert callable(getattr(iql.ReplayBuffer, "add_transitions", None))


def test_entry_points_check_their_arguments_before_any_device_work():
    """The refusals that need no context are answered on a machine without a GPU (nothing is launched), with a message."""
    lib, ptr = hb.lib(), 4096           # never dereferenced: a non-NULL, 16-byte aligned address
    good = dict(rows=ptr, ld=12, cap=8, pointer=0, pin=ptr, n=3)
    for bad in ({"rows": None}, {"pin": None}, {"ld": 10}, {"ld": 4}, {"rows": ptr + 4}, {"pin": ptr + 8}, {"cap": 0},
                {"pointer": -1}, {"pointer": 8}, {"n": 0}, {"n": 9}, {"n": 65, "cap": 100}):
        a = dict(good, **bad)
        assert lib.iqlhip_rows_write_ring(a["rows"], a["ld"], a["cap"], a["pointer"], a["pin"], a["n"], None) == hb.E_INVAL, bad
        assert hb.last_error(), bad
    assert lib.iqlhip_online_step_vec(None, ptr, 12, 8, 0, ptr, 3, ptr, 5, 1, ptr, ptr, None, 0, 1.0, 0, None, None) == hb.E_INVAL
