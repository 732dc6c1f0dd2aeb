"""CPU-only tests of group scoring (no GPU in the process): iqlhip_group_score_rows is declared, exported and bound and
refuses NULL / bad arguments; ImplicitQLearningGroup.score_buffer / score / evaluate raise every refusal before any
library call (a stub in place of the library, as tests/test_score_cpu.py); the pointer tables and row counts the
library would see for shared and per-member buffers and index lists."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import iql
import iqlhip_binding as hb
import iqlhip_score as score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, A = 17, 6
LD = (2 * S + A + 2 + 3) // 4 * 4


def test_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    m = re.search(r"#define\s+IQLHIP_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == hb.lib().iqlhip_version() >= 370
    bound = {name: (res, args) for name, res, args in hb.SYMBOLS}
    d = re.search(r"int\s+iqlhip_group_score_rows\s*\(([^;]*)\)\s*;", header)
    assert d and len(d.group(1).split(",")) == 12
    res, args = bound["iqlhip_group_score_rows"]
    assert res is C.c_int and len(args) == 12
    fn = hb.lib().iqlhip_group_score_rows            # (AttributeError if the built library does not export it)
    assert fn.restype is C.c_int and len(fn.argtypes) == 12
    assert hb.SPREAD_NAMES == tuple("mean_" + n for n in hb.SCORE_NAMES) + tuple("std_" + n for n in hb.SCORE_NAMES)
    assert len(hb.SPREAD_NAMES) == 2 * hb.IQLHIP_N_SCORE


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    lib = hb.lib()
    fake = 4096       # never dereferenced: every rejection below comes before the group is looked at
    rows = (C.c_void_p * 2)(fake, fake)
    sizes = (C.c_int64 * 2)(8, 8)
    outs = (C.c_void_p * 2)(fake, fake)
    words = (C.c_float * 22)()
    call = lib.iqlhip_group_score_rows
    assert call(None, rows, 44, sizes, 0, 8, None, outs, None, 0, words, None) == hb.E_INVAL       # NULL group
    assert call(fake, None, 44, sizes, 0, 8, None, outs, None, 0, words, None) == hb.E_INVAL       # NULL rows table
    assert call(fake, rows, 44, None, 0, 8, None, outs, None, 0, words, None) == hb.E_INVAL        # NULL n_rows
    assert call(fake, rows, 44, sizes, 0, 0, None, outs, None, 0, words, None) == hb.E_INVAL       # n < 1
    assert call(fake, rows, 44, sizes, 0, 8, None, outs, None, -32, words, None) == hb.E_INVAL     # chunk_rows
    assert call(fake, rows, 44, sizes, 0, 8, None, outs, None, 48, words, None) == hb.E_INVAL
    assert call(fake, rows, 44, sizes, 0, 8, None, outs, fake + 4, 0, words, None) == hb.E_INVAL   # misaligned spread


# ---- the Python refusals, through a stub in place of the library: none of them may reach it
class _Stub:
    def __init__(self):
        self.calls = []
        self.seen = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            if name == "iqlhip_group_score_rows":
                self.seen.append(args)
            return 0
        return call


def _cpu_trainer():
    actor = iql.GaussianPolicy(S, A, 1.0)
    qf, vf = iql.TwinQ(S, A), iql.ValueFunction(S)
    return iql.ImplicitQLearning(max_action=1.0, actor=actor, actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                 q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                                 v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 max_steps=1000, device="cpu")


def _attach(tr, k):
    """Make a CPU trainer believe it is attached: a context word, its device = where the fake buffers live."""
    tr._ctx, tr._dev, tr._S, tr._A, tr._gaussian = C.c_void_p(4096 + 64 * k), torch.device("cpu"), S, A, True


@pytest.fixture
def group(monkeypatch):
    stub = _Stub()
    monkeypatch.setattr(hb, "lib", lambda: stub)
    monkeypatch.setattr(hb, "row_stride", lambda s, a: (2 * s + a + 2 + 3) // 4 * 4)
    trs = [_cpu_trainer() for _ in range(3)]
    for k, t in enumerate(trs):
        _attach(t, k)
        monkeypatch.setattr(t, "_stream", lambda: None)
    g = iql.ImplicitQLearningGroup(trs)
    yield g, stub
    g._g = None                    # (nothing for __del__ to release)
    for t in trs:
        t._ctx = None


def _buffer(rows=64, size=40, gpu=True, ld=LD, s=S, a=A):
    return types.SimpleNamespace(_rows=torch.zeros((rows, ld)), _gpu=gpu, _state_dim=s, _action_dim=a, _ld=ld, _size=size,
                                 _buffer_size=rows)


def _batch(n=4, s=S):
    return [torch.zeros(n, s), torch.zeros(n, A), torch.zeros(n, 1), torch.zeros(n, s), torch.zeros(n, 1)]


def test_a_cpu_trainer_in_the_group_raises_runtime_error(group):
    g, stub = group
    g.trainers[1]._ctx = None
    for call in (lambda: g.score_buffer(_buffer()), lambda: g.score(_batch()), lambda: g.evaluate(_batch())):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    assert stub.calls == []


def test_python_refusals_never_reach_the_library(group):
    g, stub = group
    ok, small = _buffer(), _buffer(size=30)
    i64 = lambda *v: np.array(v, dtype=np.int64)
    cases = [
        (ValueError, "2 buffers", lambda: g.score_buffer([ok, ok])),                                   # wrong counts
        (ValueError, "2 index lists", lambda: g.score_buffer(ok, indices=[i64(1), i64(2)])),
        (ValueError, "2 batches", lambda: g.score([_batch(), _batch()])),
        (ValueError, "one length", lambda: g.score_buffer(ok, indices=[i64(1, 2), i64(1, 2), i64(1)])),  # unequal lengths
        (ValueError, "one length", lambda: g.score([_batch(4), _batch(4), _batch(5)])),
        (ValueError, "beyond", lambda: g.score_buffer([ok, small, ok], n=31)),                         # the smallest buffer
        (ValueError, "beyond", lambda: g.score_buffer([ok, small, ok], start=10, n=21)),
        (ValueError, "empty range", lambda: g.score_buffer([ok, small, ok], start=30)),
        (IndexError, "index 30 is out of bounds", lambda: g.score_buffer([ok, small, ok], indices=i64(0, 30))),
        (IndexError, "index 40 is out of bounds", lambda: g.score_buffer(ok, indices=[i64(1), i64(40), i64(2)])),
        (IndexError, "index -1 is out of bounds", lambda: g.score_buffer(ok, indices=torch.tensor([5, -1]))),
        (ValueError, "not both", lambda: g.score_buffer(ok, start=1, indices=i64(1))),
        (ValueError, "int64", lambda: g.score_buffer(ok, indices=np.arange(3, dtype=np.int32))),
        (ValueError, "lives on", lambda: g.score_buffer([ok, _buffer(gpu=False), ok])),
        (ValueError, "state_dim", lambda: g.score_buffer([ok, ok, _buffer(s=11, a=3, ld=28)])),
        (ValueError, "empty", lambda: g.score_buffer([ok, ok, _buffer(size=0)])),
        (ValueError, r"\[3, 10, 8\]", lambda: g.score_buffer(ok, n=10, out=torch.zeros(10, 8))),        # out: shape,
        (ValueError, r"\[3, 10, 8\]", lambda: g.score_buffer(ok, n=10, out=torch.zeros(2, 10, 8))),
        (ValueError, "float32", lambda: g.score_buffer(ok, n=10, out=torch.zeros(3, 10, 8, dtype=torch.float64))),   # dtype,
        (ValueError, "float32", lambda: g.score_buffer(ok, n=10, out=torch.zeros(3, 10, 8, device="meta"))),         # device
        (ValueError, "contiguous", lambda: g.score_buffer(ok, n=10, out=torch.zeros(3, 10, 16)[:, :, ::2])),
        (ValueError, r"\[10, 16\]", lambda: g.score_buffer(ok, n=10, spread=torch.zeros(10, 8))),       # spread: shape,
        (ValueError, r"\[10, 16\]", lambda: g.score_buffer(ok, n=10, spread=torch.zeros(3, 10, 16))),
        (ValueError, "float32", lambda: g.score_buffer(ok, n=10, spread=torch.zeros(10, 16, dtype=torch.float64))),
        (ValueError, "float32", lambda: g.score_buffer(ok, n=10, spread=torch.zeros(10, 16, device="meta"))),
        (ValueError, "same rows", lambda: g.score_buffer([ok, _buffer(), ok], spread=True)),            # per-member rows
        (ValueError, "same rows", lambda: g.score_buffer(ok, indices=[i64(1), i64(1), i64(1)], spread=True)),
        (ValueError, "same rows", lambda: g.score([_batch(), _batch(), _batch()], spread=True)),
        (ValueError, "nothing to compute", lambda: g.score_buffer(ok, out=False, summary=False)),
        (ValueError, "nothing to compute", lambda: g.score(_batch(), out=False, summary=False, spread=False)),
        (ValueError, "multiple of 32", lambda: g.score_buffer(ok, chunk_rows=48)),
        (ValueError, "multiple of 32", lambda: g.score(_batch(), chunk_rows=0)),
        (ValueError, "shapes", lambda: g.score([_batch()[0], torch.zeros(4, 5)] + _batch()[2:])),
        (ValueError, r"\[3, 4, 8\]", lambda: g.score(_batch(), out=torch.zeros(3, 5, 8))),
    ]
    for exc, match, call in cases:
        with pytest.raises(exc, match=match):
            call()
    assert stub.calls == []


def _table(p, K=3):
    return [p[k] for k in range(K)]


def test_argument_marshalling_for_shared_and_per_member_rows(group):
    g, stub = group
    a, b, c = _buffer(), _buffer(rows=128, size=100), _buffer(size=33)
    # one shared buffer, a range: one pointer three times, one size three times; spread allowed
    scores, summaries, spread = g.score_buffer(a, start=8, n=16, spread=True, chunk_rows=64)
    args = stub.seen[-1]
    assert _table(args[1]) == [a._rows.data_ptr()] * 3 and args[2] == LD and _table(args[3]) == [40] * 3
    assert args[4:6] == (8, 16) and args[6] is None and args[9] == 64
    assert _table(args[7]) == [scores[k].data_ptr() for k in range(3)] and tuple(scores.shape) == (3, 16, 8)
    assert args[8] == spread.data_ptr() and tuple(spread.shape) == (16, 16)
    assert len(summaries) == 3 and all(list(s) == list(score.SUMMARY_KEYS) for s in summaries)
    # per-member buffers: three pointers, three sizes; n=None runs to the end of the smallest
    scores, summaries, spread = g.score_buffer([a, b, c], out=False)
    args = stub.seen[-1]
    assert _table(args[1]) == [x._rows.data_ptr() for x in (a, b, c)] and _table(args[3]) == [40, 100, 33]
    assert args[4:6] == (0, 33) and args[7] is None and args[8] is None and scores is None and spread is None
    # one shared index list: one device copy, one pointer three times; spread into the caller's tensor
    mine = torch.zeros(3, 16)
    _, summaries, spread = g.score_buffer(a, indices=np.array([3, 3, 39]), summary=False, spread=mine)
    args = stub.seen[-1]
    assert args[5] == 3 and len(set(_table(args[6]))) == 1 and args[10] is None and summaries is None and spread is mine
    # K index lists into K buffers: three pointers
    lists = [np.array([1, 39]), torch.tensor([99, 0]), np.array([32, 32])]
    g.score_buffer([a, b, c], indices=lists)
    args = stub.seen[-1]
    assert args[5] == 2 and len(set(_table(args[6]))) == 3 and _table(args[3]) == [40, 100, 33]
    # batches: a shared one is packed once, K are packed K times
    n_pack = stub.calls.count("iqlhip_pack_rows")
    g.score(_batch(5), spread=True)
    assert stub.calls.count("iqlhip_pack_rows") == n_pack + 1 and len(set(_table(stub.seen[-1][1]))) == 1
    assert _table(stub.seen[-1][3]) == [5] * 3 and stub.seen[-1][4:6] == (0, 5)
    ev = g.evaluate([_batch(5), _batch(5), _batch(5)])
    assert stub.calls.count("iqlhip_pack_rows") == n_pack + 4 and len(set(_table(stub.seen[-1][1]))) == 3
    assert len(ev) == 3 and all(list(e) == ["value_loss", "q_loss", "actor_loss"] for e in ev)
    assert stub.seen[-1][7] is None and stub.seen[-1][10] is not None
