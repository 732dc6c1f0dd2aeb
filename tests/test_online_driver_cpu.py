"""CPU-only tests of the two online drivers — ImplicitQLearning._run_online and ImplicitQLearningGroup._run_online, the one
"insert a transition, draw a batch, take a step, optionally act" behind every online_step* method — with a stub in place
of the library that records every online entry point's arguments: the packed row, the host indices and the generator
they come from, the act arguments, and what moves when the call succeeds and when it fails.  The `public` tests reach
the drivers through the seven public methods and hold for the seven separate copies the drivers replaced as well; the
others drive the drivers directly on stand-in objects."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import iqlhip_binding as hb
import iqlhip_group as G
import iqlhip_jsrl as J
import iqlhip_nstep as N
import iqlhip_replay as R
import iqlhip_trainer as T

S, A, CAP, B = 3, 2, 4, 5
LD = 12                     # a CPU buffer's row stride at these dimensions: 2 S + A + 2 = 10 columns and 2 of padding
IT0, ADAM0 = 10, 5          # total_it and the Adam step counts before the call under test
ACT_SEED = 77
ACTION = [0.5, -0.25]       # what the stub's act forward answers


def _floats(ptr, n):
    return None if ptr is None else np.ctypeslib.as_array((C.c_float * n).from_address(ptr)).copy()


def _ints(ptr, n):
    return None if ptr is None else np.ctypeslib.as_array((C.c_int64 * n).from_address(ptr)).copy()


class _Lib:
    """Every online entry point: records its arguments as a dict, writes losses (and the action), returns `rc`."""
    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def _solo(self, name, ld, cap, pointer, row, idx, n_idx, out, a_in, max_a, seed, a_out, **more):
        assert idx is None or isinstance(idx, int)
        self.calls.append(dict(name=name, ld=ld, cap=cap, pointer=pointer, row=_floats(row, ld), idx=_ints(idx, n_idx),
                               a_in=_floats(a_in, S), max_a=max_a, seed=seed, a_out=a_out, **more))
        if self.rc == 0:
            out[0], out[1], out[2] = 1.0, 2.0, 3.0
            if a_out is not None:
                (C.c_float * A).from_address(a_out)[:] = ACTION
        return self.rc

    def iqlhip_online_step(self, ctx, rows, ld, cap, pointer, row, idx, n, sc, out, a_in, max_a, seed, a_out, stream):
        return self._solo("plain", ld, cap, pointer, row, idx, n, out, a_in, max_a, seed, a_out, rows=rows)

    def iqlhip_online_step_mixed(self, ctx, rows, ld, cap, pointer, row, idx_on, n_on, sc, out, a_in, max_a, seed, a_out,
                                 stream, off_rows, off_size, idx_off, n_off):
        return self._solo("mixed", ld, cap, pointer, row, idx_on, n_on, out, a_in, max_a, seed, a_out, rows=rows,
                          off_rows=off_rows, off_size=off_size, idx_off=_ints(idx_off, n_off))

    def iqlhip_online_step_prioritized(self, ctx, rows, ld, cap, pointer, row, n, sc, out, a_in, max_a, seed, a_out, stream,
                                       table, draw_seed, offset, beta, alpha, eps):
        return self._solo("prio", ld, cap, pointer, row, None, n, out, a_in, max_a, seed, a_out, rows=rows, n=n,
                          draw=(draw_seed, offset, beta, alpha, eps))

    def iqlhip_online_step_nstep(self, ctx, raw_rows, rows, ld, cap, pointer, row, idx, n, sc, out, a_in, max_a, seed, a_out,
                                 stream, ends, end, new_size, horizon, discount, steps):
        return self._solo("nstep", ld, cap, pointer, row, idx, n, out, a_in, max_a, seed, a_out, rows=rows,
                          raw_rows=raw_rows, tail=(end, new_size, horizon, discount))

    def iqlhip_jsrl_online_step(self, handle, rows, ld, cap, pointer, row, idx, n, sc, out, a_in, who, gate_max, seed, max_a,
                                guide_max_a, a_out, flag, h, stream):
        flag._obj.value = 1
        return self._solo("jsrl", ld, cap, pointer, row, idx, n, out, a_in, max_a, seed, a_out, rows=rows,
                          tail=(who, gate_max, guide_max_a, h))

    def _group(self, name, rings, ld, caps, ptrs, rows, idx, n, out, a_in, mask, max_a, seeds, a_out, **more):
        K = len(caps)
        ns = [n] * K if isinstance(n, int) else list(n)
        self.calls.append(dict(name=name, ld=ld, caps=list(caps), ptrs=list(ptrs), rings=list(rings), n=ns,
                               rows=_floats(rows, K * ld).reshape(K, ld), idx=_ints(idx, sum(ns)),
                               a_in=None if a_in is None else _floats(a_in, K * S).reshape(K, S),
                               mask=None if mask is None else list((C.c_int32 * K).from_address(mask)),
                               seeds=None if seeds is None else list((C.c_uint64 * K).from_address(seeds)),
                               act_none=[a_in is None, mask is None, max_a is None, seeds is None, a_out is None], **more))
        if self.rc == 0:
            out[:] = [float(i) for i in range(3 * K)]
            if a_out is not None:
                (C.c_float * (K * A)).from_address(a_out)[:] = ACTION * K
        return self.rc

    def iqlhip_group_online_step(self, g, rings, ld, caps, ptrs, rows, idx, n, scs, out, a_in, mask, max_a, seeds, a_out,
                                 stream):
        return self._group("group", rings, ld, caps, ptrs, rows, idx, n, out, a_in, mask, max_a, seeds, a_out)

    def iqlhip_group_online_step_mixed(self, g, rings, ld, caps, ptrs, rows, idx, n, scs, out, a_in, mask, max_a, seeds,
                                       a_out, stream):
        return self._group("group_mixed", rings, ld, caps, ptrs, rows, idx, n, out, a_in, mask, max_a, seeds, a_out)

    def iqlhip_group_online_step_replay2(self, g, rings, ld, caps, ptrs, rows, idx, n, scs, out, a_in, mask, max_a, seeds,
                                         a_out, stream, offs, size_off, n_off):
        return self._group("replay_mix", rings, ld, caps, ptrs, rows, idx, n, out, a_in, mask, max_a, seeds, a_out,
                           offs=list(offs), size_off=list(size_off), n_off=list(n_off))

    def iqlhip_last_error(self):
        return b"stub"


def _lib(monkeypatch, rc=0):
    lib = _Lib(rc)
    monkeypatch.setattr(hb, "lib", lambda: lib)
    return lib


def _ring(size=2, pointer=2, cls=R.ReplayBuffer):
    """A ring of CAP rows on the CPU that passes for one on the trainer's device (the checks look at the flag and at
    the rows' device: the stand-in trainers' is the CPU)."""
    buf = cls(S, A, CAP, "cpu")
    buf._gpu, buf._size, buf._pointer = True, size, pointer
    return buf


def _ring_state(*bufs):
    return [(b._writes, b._pointer, b._size, b._weights_version, getattr(b, "_prio_online_offset", None)) for b in bufs]


def _rng_state():
    st = np.random.get_state()
    return st[1].copy(), st[2]


def _same_rng(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1]


class _Host:
    """What the online methods touch of a trainer beside the library call, as instance attributes of a stand-in."""
    def __init__(self):
        self._ctx, self._dev, self._S, self._A, self._gaussian = None, torch.device("cpu"), S, A, True
        self._dp_world, self._dp_rank, self._dp_exchange, self._precision = 1, 0, None, "f32"
        self.total_it, self._adam_t, self._step_stats, self._act_dropout = IT0, {g: ADAM0 for g in ("v", "q", "pi")}, False, False
        self._ts_token, self._eager_next, self._masks_injected = None, None, False
        self._last_td, self._last_td_it, self._last_prio_idx = ("online", B), IT0 - 1, (IT0 - 1, B)    # an earlier step's
        self._on_row, self._on_scalars, self._loss_out = np.zeros(LD, dtype=np.float32), hb.StepScalars(), (C.c_float * 3)()
        self.actor = types.SimpleNamespace(max_action=1.5, training=True)
        self.filled, self.scheduled, self.seed_rng, self.prepared = [], [], [], []

    def _prepare(self, rows):
        self.prepared.append(rows)

    def _require_gpu(self):
        pass

    def _prepare_act(self):
        pass

    def _stream(self):
        return None

    def acts_with_dropout(self):
        return False

    def _current_lrs(self):
        return {}

    def _fill_scalars(self, sc, t, lrs, inv_batch):
        self.filled.append((dict(t), inv_batch))

    def _advance_schedule(self, n):
        self.scheduled.append(n)

    def _act_seed(self):
        self.seed_rng.append(_rng_state())          # (where the global stream stood when the seed was taken)
        return ACT_SEED


def _trainer():
    """An ImplicitQLearning with everything around the online call stubbed out."""
    tr = object.__new__(T.ImplicitQLearning)
    host = _Host()
    tr.__dict__.update(host.__dict__)
    for name in ("_prepare", "_require_gpu", "_prepare_act", "_stream", "acts_with_dropout", "_current_lrs",
                 "_fill_scalars", "_advance_schedule", "_act_seed"):
        setattr(tr, name, types.MethodType(getattr(_Host, name), tr))
    return tr


def _trainer_state(tr):
    return tr.total_it, dict(tr._adam_t), list(tr.scheduled)


TRANSITION = (np.array([1.0, 2.0, 3.0]), np.array([4.0, 5.0]), 6.0, np.array([7.0, 8.0, 9.0]), True)
ROW = np.array([1, 2, 3, 4, 5, 7, 8, 9, 6, 1, 0, 0], dtype=np.float32)
ACT_NEXT = np.array([0.1, 0.2, 0.3])


def _nstep(raw):
    ns = object.__new__(N.NStepReplay)
    ns.raw, ns.buffer, ns.n, ns.discount = raw, _ring(raw._size, raw._pointer), 3, 0.99
    ns.ends, ns.steps = torch.zeros(CAP, dtype=torch.uint8), torch.zeros(CAP, dtype=torch.uint8)
    return ns


def _jsrl(tr):
    js = object.__new__(J.JsrlActors)
    js.learners, js.guides, js.gates, js.critics, js._h = [tr], [None], [None], [None], None
    js._check_members = lambda: None
    js._handle = lambda: None
    return js


def _prio_ring(**kw):
    buf = _ring(**kw)       # (a tracking table by its flags; the stub never dereferences the table)
    buf._weights_n, buf._weights_updatable, buf._weights_tracks, buf._weights_version = CAP, True, True, 6
    return buf


class _Case:
    """One solo method: how to call it on a ring, which rings move, and its draw."""
    def __init__(self, name, entry, what=None):
        self.name, self.entry, self.what = name, entry, what

    def rings(self, **kw):
        """(the object the method takes, the rings that move with a successful call)."""
        if self.name == "prio":
            buf = _prio_ring(**kw)
            return buf, [buf]
        if self.name == "nstep":
            ns = _nstep(_ring(**kw))
            return ns, [ns.raw, ns.buffer]
        buf = _ring(**kw)
        return buf, [buf]

    def call(self, tr, target, act_next=None, offline=None):
        if self.name == "plain":
            return tr.online_step(target, *TRANSITION, B, act_next=act_next)
        if self.name == "mixed":
            return tr.online_step_mixed(offline, target, *TRANSITION, B, 0.4, act_next=act_next)
        if self.name == "prio":
            return tr.online_step_prioritized(target, *TRANSITION, B, seed=9, act_next=act_next)
        if self.name == "nstep":
            return tr.online_step_nstep(target, *TRANSITION, B, act_next=act_next)
        return tr.online_step_jsrl(_jsrl(tr), target, *TRANSITION, B, ACT_NEXT if act_next is None else act_next, 1)


CASES = [_Case("plain", "plain", "online_step"), _Case("mixed", "mixed"), _Case("prio", "prio", "online_step_prioritized"),
         _Case("nstep", "nstep", "online_step_nstep"), _Case("jsrl", "jsrl", "online_step")]
SOLO = pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
OFF_SIZE = 300


def _offline():
    off = _ring(size=CAP, pointer=0)
    off._size = OFF_SIZE          # (only its size is read: the stub never dereferences its rows)
    return off


def _want_indices(case, seed, new_size):
    """The indices the call must pass after np.random.seed(seed), and where the global stream stands behind the draw."""
    np.random.seed(seed)
    off = None
    if case.name == "mixed":
        off = np.random.randint(0, OFF_SIZE, size=2)              # n_off = int(5 * 0.4): the offline draw comes first
        idx = np.random.randint(0, new_size, size=B - 2)
    elif case.name == "prio":
        idx = None                                                # (drawn on the device)
    else:
        idx = np.random.randint(0, new_size, size=B)
    return off, idx, _rng_state()


# ---- through the public methods: the five solo calls -----------------------------------------------------------------
# (online_step_jsrl selects the next action: it has no form without act_next)
@pytest.mark.parametrize("case, with_act", [(c, w) for c in CASES for w in (False, True) if w or c.name != "jsrl"],
                         ids=[c.name + ("-act" if w else "") for c in CASES for w in (False, True) if w or c.name != "jsrl"])
def test_public_solo_row_indices_act_arguments_and_commit(case, with_act, monkeypatch):
    lib, tr = _lib(monkeypatch), _trainer()
    target, moved = case.rings(size=2, pointer=2)
    off_want, idx_want, rng_after = _want_indices(case, 3, new_size=3)
    np.random.seed(3)
    res = case.call(tr, target, act_next=ACT_NEXT if with_act else None, offline=_offline())
    (c,) = lib.calls
    assert c["name"] == case.entry and (c["ld"], c["cap"], c["pointer"]) == (LD, CAP, 2)
    assert c["rows"] == moved[-1]._rows.data_ptr()
    # the row: the transition, the pad columns zero
    assert c["row"].dtype == np.float32 and np.array_equal(c["row"], ROW)
    # the indices: int64 (the stub reads 8-byte words), B of them, the global draw over the size after the insert
    if idx_want is None:
        assert c["idx"] is None and c["n"] == B
    else:
        assert c["idx"].shape == idx_want.shape and np.array_equal(c["idx"], idx_want)
    if off_want is not None:
        assert np.array_equal(c["idx_off"], off_want) and c["off_size"] == OFF_SIZE
    assert _same_rng(_rng_state(), rng_after)
    # the act arguments
    assert c["max_a"] == 1.5
    if with_act:
        assert np.array_equal(c["a_in"], ACT_NEXT.astype(np.float32)) and c["seed"] == ACT_SEED and c["a_out"] is not None
        assert len(tr.seed_rng) == 1 and _same_rng(tr.seed_rng[0], rng_after)       # the seed: behind the index draw
    else:
        assert c["a_in"] is None and c["a_out"] is None and c["seed"] == 0 and not tr.seed_rng
    # the commit: once
    log = {"value_loss": 1.0, "q_loss": 2.0, "actor_loss": 3.0}
    if case.name == "jsrl":
        assert res[0] == log and np.array_equal(res[1], np.float32(ACTION)) and res[2:] == (1, None)
    elif with_act:
        assert res[0] == log and np.array_equal(res[1], np.float32(ACTION)) and len(res) == 2
    else:
        assert res == log
    assert all((b._writes, b._pointer, b._size) == (1, 3, 3) for b in moved)
    assert _trainer_state(tr) == (IT0 + 1, {g: ADAM0 + 1 for g in ("v", "q", "pi")}, [1])
    assert tr.filled == [({g: ADAM0 + 1 for g in ("v", "q", "pi")}, 1.0 / B)]
    if case.name == "prio":
        assert (target._weights_version, target._prio_online_offset) == (8, 3)      # + 2; ceil(5 / 2) counters
        assert c["draw"] == (9, 0, 0.4, 0.6, 1e-6)
        assert tr._last_td == ("online", B) and tr._last_td_it == IT0 + 1 and tr._last_prio_idx == (IT0 + 1, B)
    if case.name == "nstep":
        assert c["raw_rows"] == target.raw._rows.data_ptr() and c["tail"] == (1, 3, 3, 0.99)


@SOLO
def test_public_solo_ring_wraps_at_capacity(case, monkeypatch):
    lib, tr = _lib(monkeypatch), _trainer()
    target, moved = case.rings(size=CAP, pointer=3)
    _, idx_want, _ = _want_indices(case, 5, new_size=CAP)
    np.random.seed(5)
    case.call(tr, target, offline=_offline())
    assert lib.calls[0]["pointer"] == 3
    if idx_want is not None:
        assert np.array_equal(lib.calls[0]["idx"], idx_want)
    assert all((b._writes, b._pointer, b._size) == (1, 0, CAP) for b in moved)


@SOLO
def test_public_solo_failed_call_moves_nothing(case, monkeypatch):
    lib, tr = _lib(monkeypatch, rc=hb.E_INVAL), _trainer()
    target, moved = case.rings(size=CAP, pointer=3)
    rings0, tr0 = _ring_state(*moved), _trainer_state(tr)
    with pytest.raises(ValueError, match="stub"):
        case.call(tr, target, act_next=ACT_NEXT, offline=_offline())
    assert len(lib.calls) == 1
    assert _ring_state(*moved) == rings0 and _trainer_state(tr) == tr0
    # what last_td_errors() / last_prioritized_indices() go by still names the earlier step (the prioritised call gives
    # up the earlier TD errors themselves in front of the library call, which may overwrite them before it fails)
    assert (tr._last_td_it, tr._last_prio_idx) == (IT0 - 1, (IT0 - 1, B))
    assert tr._last_td == (None if case.name == "prio" else ("online", B))


@pytest.mark.parametrize("case", [c for c in CASES if c.what], ids=[c.name for c in CASES if c.what])
def test_public_solo_wrong_ring_is_refused_before_any_draw(case, monkeypatch):
    lib, tr = _lib(monkeypatch), _trainer()
    np.random.seed(1)
    rng0 = _rng_state()

    def refused(exc, message, ring):
        target = _nstep(ring) if case.name == "nstep" else ring
        if case.name == "nstep":
            target.buffer = type(ring)(S, A, CAP, "cpu")          # (the derived buffer lives where the raw one does)
            target.buffer._gpu = ring._gpu
        with pytest.raises(exc) as e:
            case.call(tr, target)
        assert str(e.value) == message
        assert not lib.calls and _same_rng(_rng_state(), rng0) and _trainer_state(tr) == (IT0, {g: ADAM0 for g in ("v", "q", "pi")}, [])
        assert (ring._writes, ring._pointer, ring._size) == (0, 0, 0)

    holder = "an NStepReplay" if case.name == "nstep" else "a ReplayBuffer"
    if case.name != "nstep":        # (an NStepReplay cannot be formed on a CPU buffer; its device is checked all the same)
        refused(ValueError, f"{case.what} needs {holder} on the trainer's GPU", R.ReplayBuffer(S, A, CAP, "cpu"))
    tr._dev = torch.device("meta")
    refused(ValueError, f"{case.what} needs {holder} on the trainer's GPU", _ring(0, 0))
    tr._dev = torch.device("cpu")
    refused(NotImplementedError, f"{case.what} needs the finetune ReplayBuffer (the offline flavour has no add_transition)",
            _ring(0, 0, cls=R.OfflineReplayBuffer))


# ---- through the public methods: the two group calls -----------------------------------------------------------------
def _group(K, mixed_batch=False):
    g = object.__new__(G.ImplicitQLearningGroup)
    g.trainers, g._g, g._ctxs, g._actor_dropout, g._mixed_batch = [_Host() for _ in range(K)], None, None, False, mixed_batch
    g._check_members = lambda: None
    g._group = lambda: None
    return g


def _transitions(K):
    """K transitions that differ by member (member k's numbers are the solo TRANSITION's plus 10 k), and their rows."""
    cols = list(zip(*[tuple(x + 10 * k if i < 4 else x for i, x in enumerate(TRANSITION)) for k in range(K)]))
    rows = np.stack([ROW + 10 * k for k in range(K)])
    rows[:, 9:] = ROW[9:]
    return [list(c) for c in cols], rows


GROUP = pytest.mark.parametrize("method", ["online_step", "online_step_mixed_batch", "online_step_replay_mix"])


def _group_call(g, method, rings, trans, Bs, **kw):
    if method == "online_step_replay_mix":
        return g.online_step_replay_mix(_offline(), rings, *trans, Bs, 0.4, **kw)
    return g.online_step(rings, *trans, Bs, **kw)


def _group_want(method, Bs, new_sizes, rngs):
    out = []
    for k, (b, n) in enumerate(zip(Bs, new_sizes)):
        rng = np.random if rngs is None else rngs[k]
        if method == "online_step_replay_mix":
            out.append(rng.randint(0, OFF_SIZE, size=int(b * 0.4)))
            out.append(rng.randint(0, n, size=b - int(b * 0.4)))
        else:
            out.append(rng.randint(0, n, size=b))
    return np.concatenate(out)


@GROUP
@pytest.mark.parametrize("own_rngs", [False, True])
def test_public_group_rows_indices_act_arguments_and_commit(method, own_rngs, monkeypatch):
    K = 3
    lib, g = _lib(monkeypatch), _group(K, mixed_batch=method != "online_step")
    Bs = [5, 5, 5] if method == "online_step" else [5, 3, 6]
    rings = [_ring(0, 0), _ring(2, 2), _ring(CAP, 3)]
    trans, rows_want = _transitions(K)
    np.random.seed(4)
    rng0 = _rng_state()
    want = _group_want(method, Bs, [1, 3, CAP], [np.random.RandomState(20 + k) for k in range(K)] if own_rngs else None)
    rng_after = _rng_state()
    np.random.seed(4)
    kw = {"rngs": [np.random.RandomState(20 + k) for k in range(K)]} if own_rngs else {}
    logs = _group_call(g, method, rings, trans, Bs if method != "online_step" else 5, **kw)
    (c,) = lib.calls
    assert c["name"] == {"online_step": "group", "online_step_mixed_batch": "group_mixed"}.get(method, "replay_mix")
    assert c["ld"] == LD and c["caps"] == [CAP] * K and c["ptrs"] == [0, 2, 3] and c["n"] == Bs
    assert c["rings"] == [b._rows.data_ptr() for b in rings]
    assert np.array_equal(c["rows"], rows_want)
    assert c["idx"].shape == want.shape and np.array_equal(c["idx"], want)            # in member order
    assert _same_rng(_rng_state(), rng0 if own_rngs else rng_after)                   # rngs: the global stream untouched
    assert c["act_none"] == [True] * 5 and not any(t.seed_rng for t in g.trainers)
    if method == "online_step_replay_mix":
        assert c["size_off"] == [OFF_SIZE] * K and c["n_off"] == [int(b * 0.4) for b in Bs]
    assert logs == [{"value_loss": 3.0 * k, "q_loss": 3.0 * k + 1, "actor_loss": 3.0 * k + 2} for k in range(K)]
    assert [(b._writes, b._pointer, b._size) for b in rings] == [(1, 1, 1), (1, 3, 3), (1, 0, CAP)]
    assert all(_trainer_state(t) == (IT0 + 1, {x: ADAM0 + 1 for x in ("v", "q", "pi")}, [1]) for t in g.trainers)
    assert [t.filled for t in g.trainers] == [[({x: ADAM0 + 1 for x in ("v", "q", "pi")}, 1.0 / b)] for b in Bs]
    assert [t.prepared for t in g.trainers] == [[b] for b in Bs]


@GROUP
def test_public_group_act_next_for_some_members(method, monkeypatch):
    K = 2
    lib, g = _lib(monkeypatch), _group(K, mixed_batch=method != "online_step")
    rings = [_ring(2, 2), _ring(2, 2)]
    trans, _ = _transitions(K)
    logs, actions = _group_call(g, method, rings, trans, 5, act_next=[None, ACT_NEXT])
    (c,) = lib.calls
    assert c["act_none"] == [False] * 5 and c["mask"] == [0, 1] and c["seeds"] == [ACT_SEED] * K
    assert np.array_equal(c["a_in"], np.stack([np.zeros(S), ACT_NEXT]).astype(np.float32))
    assert len(logs) == K and actions[0] is None and np.array_equal(actions[1], np.float32(ACTION))


@GROUP
def test_public_group_failed_call_moves_nothing(method, monkeypatch):
    K = 2
    lib, g = _lib(monkeypatch, rc=hb.E_INVAL), _group(K, mixed_batch=method != "online_step")
    rings = [_ring(2, 2), _ring(CAP, 3)]
    trans, _ = _transitions(K)
    rings0, tr0 = _ring_state(*rings), [_trainer_state(t) for t in g.trainers]
    with pytest.raises(ValueError, match="stub"):
        _group_call(g, method, rings, trans, 5, act_next=[ACT_NEXT, None])
    assert len(lib.calls) == 1
    assert _ring_state(*rings) == rings0 and [_trainer_state(t) for t in g.trainers] == tr0


def test_public_group_wrong_ring_names_the_member_before_any_draw(monkeypatch):
    K = 2
    lib, g = _lib(monkeypatch), _group(K)
    trans, _ = _transitions(K)
    np.random.seed(1)
    rng0 = _rng_state()
    for exc, message, bad in (
            (ValueError, "iqlhip: online_step needs a ReplayBuffer on the trainer's GPU (member 1)", R.ReplayBuffer(S, A, CAP, "cpu")),
            (NotImplementedError, "online_step needs the finetune ReplayBuffer (the offline flavour has no add_transition; "
                                  "member 1)", _ring(0, 0, cls=R.OfflineReplayBuffer))):
        good = _ring(0, 0)
        with pytest.raises(exc) as e:
            g.online_step([good, bad], *trans, 5)
        assert str(e.value) == message
        assert not lib.calls and _same_rng(_rng_state(), rng0)
        assert _ring_state(good, bad) == _ring_state(_ring(0, 0), _ring(0, 0))
        assert all(_trainer_state(t) == (IT0, {x: ADAM0 for x in ("v", "q", "pi")}, []) for t in g.trainers)


# ---- the solo driver, driven directly --------------------------------------------------------------------------------
def _drive_solo(tr, ring, seen, draw=None, act_next=None, rc=0, commit_extra=None):
    def call(ring_args, row, idx, sc, out, act_args, stream):
        seen.append((ring_args, _floats(row, LD), idx, act_args, (ring._writes, ring._pointer, ring._size), tr.total_it))
        out[0], out[1], out[2] = 1.0, 2.0, 3.0
        return rc
    return T.ImplicitQLearning._run_online(tr, ring, TRANSITION, act_next, draw, 0.125, call, commit_extra)


def test_solo_driver_without_a_draw_passes_no_index_pointer(monkeypatch):
    _lib(monkeypatch)
    tr, ring, seen = _trainer(), _ring(2, 2), []
    np.random.seed(2)
    rng0 = _rng_state()
    log = _drive_solo(tr, ring, seen)
    ((ring_args, row, idx, act_args, ring_then, it_then),) = seen
    assert idx is None and _same_rng(_rng_state(), rng0)
    assert ring_args == (ring._rows.data_ptr(), LD, CAP, 2) and np.array_equal(row, ROW)
    assert act_args == (None, 1.5, 0, None)
    assert ring_then == (0, 2, 2) and it_then == IT0                  # nothing had moved when the library was called
    assert log == {"value_loss": 1.0, "q_loss": 2.0, "actor_loss": 3.0}                # no act_next: the dict alone
    assert tr.filled == [({g: ADAM0 + 1 for g in ("v", "q", "pi")}, 0.125)]            # inv_batch as the caller gave it


def test_solo_driver_draws_over_the_new_size_and_returns_the_action_with_act_next(monkeypatch):
    _lib(monkeypatch)
    tr, ring, seen, sizes = _trainer(), _ring(CAP, 3), [], []
    idx = np.arange(B, dtype=np.int64)

    def draw(new_size):
        sizes.append(new_size)
        return idx
    log, action = _drive_solo(tr, ring, seen, draw=draw, act_next=ACT_NEXT)
    assert sizes == [CAP] and seen[0][2] == idx.ctypes.data
    a_in, max_a, seed, a_out = seen[0][3]
    assert np.array_equal(_floats(a_in, S), np.float32(ACT_NEXT)) and (max_a, seed) == (1.5, ACT_SEED)
    assert a_out == action.ctypes.data and action.shape == (A,) and action.dtype == np.float32
    assert log["q_loss"] == 2.0 and (ring._writes, ring._pointer, ring._size) == (1, 0, CAP)


def test_solo_driver_commit_extra_runs_after_success_behind_the_ring(monkeypatch):
    _lib(monkeypatch)
    tr, ring, seen, extra = _trainer(), _ring(2, 2), [], []

    def commit_extra():
        extra.append(((ring._writes, ring._pointer, ring._size), _trainer_state(tr)))
    with pytest.raises(ValueError, match="stub"):
        _drive_solo(tr, ring, seen, rc=hb.E_INVAL, commit_extra=commit_extra)
    assert not extra and (ring._writes, ring._pointer, ring._size) == (0, 2, 2) and tr.total_it == IT0
    _drive_solo(tr, ring, seen, commit_extra=commit_extra)
    assert extra == [((1, 3, 3), (IT0 + 1, {g: ADAM0 + 1 for g in ("v", "q", "pi")}, [1]))]


# ---- the group driver, driven directly -------------------------------------------------------------------------------
def _drive_group(g, rings, seen, draw, act_next=None, rngs=None, rc=0):
    K = len(rings)

    def call(handle, ring_args, rows, idx, scs, out, act_args, stream):
        seen.append((ring_args, _floats(rows, K * LD).reshape(K, LD), idx, act_args,
                     [(b._writes, b._pointer, b._size) for b in rings], [t.total_it for t in g.trainers]))
        out[:] = [float(i) for i in range(3 * K)]
        if act_args[4] is not None:
            (C.c_float * (K * A)).from_address(act_args[4])[:] = ACTION * K
        return rc
    trans, _ = _transitions(K)
    return G.ImplicitQLearningGroup._run_online(g, rings, trans, [B] * K, act_next, rngs, draw, call)


def test_group_driver_draws_in_member_order_and_commits_after_success(monkeypatch):
    _lib(monkeypatch)
    K = 2
    g, rings, seen, drawn = _group(K), [_ring(2, 2), _ring(CAP, 3)], [], []
    rngs = [np.random.RandomState(k) for k in range(K)]

    def draw(k, new_size, rng):
        drawn.append((k, new_size, rng))
        return np.full(2, k, dtype=np.int64), np.full(B - 2, 10 + k, dtype=np.int64)        # two parts per member
    with pytest.raises(ValueError, match="stub"):
        _drive_group(g, rings, seen, draw, rc=hb.E_INVAL)
    assert drawn == [(0, 3, None), (1, CAP, None)]                     # rngs=None: the draw is told to use the global one
    assert [(b._writes, b._pointer, b._size) for b in rings] == [(0, 2, 2), (0, 3, CAP)]
    assert all(_trainer_state(t) == (IT0, {x: ADAM0 for x in ("v", "q", "pi")}, []) for t in g.trainers)
    del drawn[:]
    logs = _drive_group(g, rings, seen, draw, rngs=rngs)
    assert drawn == [(0, 3, rngs[0]), (1, CAP, rngs[1])]
    (ring_args, rows, idx, act_args, rings_then, its_then) = seen[1]
    assert list(ring_args[0]) == [b._rows.data_ptr() for b in rings] and ring_args[1] == LD
    assert list(ring_args[2]) == [CAP] * K and list(ring_args[3]) == [2, 3]
    assert np.array_equal(rows, _transitions(K)[1])
    assert list(_ints(idx, 2 * B)) == [0, 0, 10, 10, 10, 1, 1, 11, 11, 11]
    assert act_args == (None,) * 5
    assert rings_then == [(0, 2, 2), (0, 3, CAP)] and its_then == [IT0] * K      # nothing had moved at the library call
    assert isinstance(logs, list) and [l["value_loss"] for l in logs] == [0.0, 3.0]    # no act_next: the logs alone
    assert [(b._writes, b._pointer, b._size) for b in rings] == [(1, 3, 3), (1, 0, CAP)]
    assert all(_trainer_state(t) == (IT0 + 1, {x: ADAM0 + 1 for x in ("v", "q", "pi")}, [1]) for t in g.trainers)


def test_group_driver_returns_the_actions_with_act_next(monkeypatch):
    _lib(monkeypatch)
    K = 2
    g, rings, seen = _group(K), [_ring(2, 2), _ring(2, 2)], []
    logs, actions = _drive_group(g, rings, seen, lambda k, n, rng: (np.zeros(B, dtype=np.int64),), act_next=[ACT_NEXT, None])
    assert len(logs) == K and np.array_equal(actions[0], np.float32(ACTION)) and actions[1] is None
    assert all(a is not None for a in seen[0][3])
