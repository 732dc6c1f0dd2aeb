"""CPU-only tests of the two burst drivers — ImplicitQLearning._run_burst and ImplicitQLearningGroup._run_burst, the one
multi-step loop behind every train_steps* method — with a stub in place of the library that records every call: the
chunk lengths and Philox offsets, when TS_CONTINUE is passed, what a failed chunk leaves behind, and the shapes that
come back.  The `public` tests reach the loop through the public methods and hold for the six separate loops the
drivers replaced as well; the others drive the drivers directly on stand-in objects."""
import types
import weakref

import numpy as np
import pytest
import torch

import iqlhip_binding as hb
import iqlhip_group as G
import iqlhip_trainer as T

IT0 = 10        # total_it before the call under test
N_STATS = hb.IQLHIP_N_STATS


class _Lib:
    """Records (entry point, k, offset(s), flags) of every burst call; the fail_at-th call returns E_INVAL."""
    def __init__(self, fail_at=None):
        self.calls, self.fail_at = [], fail_at

    def rec(self, name, k, offset, flags):
        self.calls.append((name, int(k), offset, int(flags)))
        return hb.E_INVAL if len(self.calls) == self.fail_at else 0

    def iqlhip_train_steps(self, ctx, rows, ld, size, B, tab, k, seed, offset, flags, stream):
        return self.rec("plain", k, int(offset), flags)

    def iqlhip_train_steps_mixed(self, ctx, off, size_off, on, size_on, ld, B, n_off, tab, k, seed, offset, stream):
        return self.rec("mixed", k, int(offset), 0)

    def iqlhip_train_steps_weighted(self, ctx, rows, ld, size, B, tab, k, seed, offset, flags, stream, table):
        return self.rec("weighted", k, int(offset), flags)

    def iqlhip_train_steps_weighted_is(self, ctx, rows, ld, size, B, tab, k, seed, offset, flags, stream, table, beta):
        return self.rec("weighted_is", k, int(offset), flags)

    def iqlhip_group_train_steps(self, g, rows, ld, sizes, B, tabs, k, seeds, offs, flags, stream):
        return self.rec("group", k, list(offs), flags)

    def iqlhip_read_loss_ring(self, ctx, buf, k, stream):
        return 0

    def iqlhip_read_stats_ring(self, ctx, buf, k, stream):
        return 0

    def iqlhip_group_read_losses(self, g, out, k, stream):
        self.calls.append(("read_losses", int(k), None, 0))
        return 0

    def iqlhip_last_error(self):
        return b"stub"


def _lib(monkeypatch, fail_at=None):
    lib = _Lib(fail_at)
    monkeypatch.setattr(hb, "lib", lambda: lib)
    return lib


def _bursts(lib):
    return [c for c in lib.calls if c[0] != "read_losses"]


class _Rows:
    _ld, _writes, _size = 44, 0, 9

    def __init__(self):
        self._rows = torch.zeros(4, 44)


# ---- through the public methods --------------------------------------------------------------------------------------
def _public_trainer():
    """An ImplicitQLearning with everything in front of the loop stubbed out."""
    tr = object.__new__(T.ImplicitQLearning)
    tr._ctx, tr._dp_world, tr._dp_rank, tr._ts_token, tr.total_it, tr._step_stats = None, 1, 0, None, IT0, True
    tr._train_steps_args = lambda buf, b: (5000, 1.0 / b)
    tr._mixed_args = lambda off, on, b, ratio: (1, b - 1)
    tr._weighted_args = lambda buf, b, weights=None: (5000, None, (7, 1))
    tr._prepare = lambda rows: None
    tr._scalar_table = lambda k, inv: np.zeros((k, 12), dtype=np.float32)
    tr._lookahead_table = lambda k, inv: None
    tr._stream = lambda: 0
    return tr


def _plain_token(buf):
    return (weakref.ref(buf), buf._writes, buf._rows._version)


@pytest.mark.parametrize("B", [3, 4])
def test_public_plain_chunks_offsets_and_continuation(B, monkeypatch):
    lib, tr, buf = _lib(monkeypatch), _public_trainer(), _Rows()
    assert tr.train_steps(buf, 5, B, seed=3, chunk=2, return_losses=False) is None
    # (a) k = 2, 2, 1 at offsets total_it * half; (b) the first chunk starts afresh, the later ones continue it
    assert lib.calls == [("plain", 2, IT0 * 2, 0), ("plain", 2, (IT0 + 2) * 2, hb.TS_CONTINUE),
                         ("plain", 1, (IT0 + 4) * 2, hb.TS_CONTINUE)]
    assert tr.total_it == IT0 + 5 and tr._ts_token == _plain_token(buf)
    tr.train_steps(buf, 1, B, return_losses=False)                 # the next call on the untouched buffer continues
    buf._writes += 1
    tr.train_steps(buf, 1, B, return_losses=False)                 # a write ends the continuation
    buf._rows.add_(1.0)
    tr.train_steps(buf, 1, B, return_losses=False)                 # ... and so does an in-place write of the rows
    tr.train_steps(_Rows(), 1, B, return_losses=False)             # ... and another buffer
    assert [c[3] for c in lib.calls[3:]] == [hb.TS_CONTINUE, 0, 0, 0]
    assert tr.train_steps(buf, 0, B).shape == (0, 3) and len(lib.calls) == 7        # no steps: no library call


def test_public_failed_second_chunk_clears_the_token(monkeypatch):
    lib, tr, buf = _lib(monkeypatch, fail_at=2), _public_trainer(), _Rows()
    with pytest.raises(ValueError, match="stub"):
        tr.train_steps(buf, 5, 4, chunk=2, return_losses=False)
    assert len(lib.calls) == 2 and tr._ts_token is None and tr.total_it == IT0 + 2          # (c)


def test_public_mixed_never_continues_and_leaves_no_token(monkeypatch):
    lib, tr, buf = _lib(monkeypatch), _public_trainer(), _Rows()
    tr.train_steps(buf, 1, 4, return_losses=False)
    assert tr._ts_token is not None
    losses = tr.train_steps_mixed(buf, _Rows(), 5, 3, chunk=2)
    assert losses.shape == (5, 3)
    assert lib.calls[1:] == [("mixed", 2, (IT0 + 1) * 2, 0), ("mixed", 2, (IT0 + 3) * 2, 0), ("mixed", 1, (IT0 + 5) * 2, 0)]
    assert tr._ts_token is None and tr.total_it == IT0 + 6                                   # (d)
    tr.train_steps(buf, 1, 4, return_losses=False)
    tr.train_steps_mixed(buf, _Rows(), 0, 3)                       # no steps: the token is dropped all the same
    assert tr._ts_token is None and len(lib.calls) == 5
    tr.train_steps(buf, 1, 4, return_losses=False)
    assert lib.calls[-1][3] == 0                                   # the plain call behind a mixed one starts afresh


def test_public_weighted_token_kind_and_generation(monkeypatch):
    lib, tr, buf = _lib(monkeypatch), _public_trainer(), _Rows()
    losses, stats = tr.train_steps_weighted(buf, 5, 4, chunk=2, return_stats=True)
    assert losses.shape == (5, 3) and stats.shape == (5, N_STATS)
    assert [c[:2] + c[3:] for c in lib.calls] == [("weighted", 2, 0), ("weighted", 2, hb.TS_CONTINUE),
                                                  ("weighted", 1, hb.TS_CONTINUE)]
    assert [c[2] for c in lib.calls] == [IT0 * 2, (IT0 + 2) * 2, (IT0 + 4) * 2]
    assert tr._ts_token == _plain_token(buf) + ("weighted", (7, 1))
    tr.train_steps_weighted(buf, 2, 4, is_beta=0.5, return_losses=False)      # a kind of its own: starts afresh ...
    tr.train_steps_weighted(buf, 1, 4, is_beta=0.25, return_losses=False)     # ... and continues under another beta
    assert lib.calls[3:] == [("weighted_is", 2, (IT0 + 5) * 2, 0), ("weighted_is", 1, (IT0 + 7) * 2, hb.TS_CONTINUE)]
    assert tr._ts_token == _plain_token(buf) + ("weighted_is", (7, 1))
    tr.train_steps(buf, 1, 4, return_losses=False)                 # a plain call never continues a weighted one
    tr._weighted_args = lambda buf, b, weights=None: (5000, None, (7, 2))
    tr.train_steps_weighted(buf, 1, 4, return_losses=False)        # nor a weighted one a plain one
    tr.train_steps_weighted(buf, 1, 4, return_losses=False)
    tr._weighted_args = lambda buf, b, weights=None: (5000, None, (7, 3))
    tr.train_steps_weighted(buf, 1, 4, return_losses=False)        # an updated table ends the continuation
    assert [c[3] for c in lib.calls[5:]] == [0, 0, hb.TS_CONTINUE, 0]
    lib.fail_at = len(lib.calls) + 1
    with pytest.raises(ValueError, match="stub"):
        tr.train_steps_weighted(buf, 1, 4, return_losses=False)
    assert tr._ts_token is None


class _Member:
    """What a group burst touches of a member behind the checks."""
    _dev, _precision, _step_stats = torch.device("cpu"), "f32", False

    def __init__(self):
        self.total_it, self._ts_token, self.tables = IT0, "stale", []

    def _train_steps_args(self, buf, B):
        return 5000, 1.0 / B

    def _scalar_table(self, k, inv):
        self.tables.append((k, inv))
        return np.zeros((k, 12), dtype=np.float32)

    def _stream(self):
        return 0


def _group(K, mixed_batch=False):
    g = object.__new__(G.ImplicitQLearningGroup)
    g.trainers, g._g, g._ctxs, g._actor_dropout, g._mixed_batch = [_Member() for _ in range(K)], None, None, False, mixed_batch
    g._check_members = lambda: None
    g._group = lambda: None
    g._group_stats = lambda n: np.full((n, K, N_STATS), 2.0, dtype=np.float32)
    return g


def test_public_group_chunks_offsets_and_tokens(monkeypatch):
    lib, g, buf = _lib(monkeypatch), _group(2), _Rows()
    losses = g.train_steps(buf, 5, 4, seeds=[1, 2], chunk=2)
    assert losses.shape == (2, 5, 3)
    assert _bursts(lib) == [("group", 2, [IT0 * 2] * 2, 0), ("group", 2, [(IT0 + 2) * 2] * 2, 0),
                            ("group", 1, [(IT0 + 4) * 2] * 2, 0)]
    assert [c[1] for c in lib.calls if c[0] == "read_losses"] == [2, 2, 1]
    assert all(t.total_it == IT0 + 5 and t._ts_token is None for t in g.trainers)
    assert all(t.tables == [(2, 0.25), (2, 0.25), (1, 0.25)] for t in g.trainers)
    with pytest.raises(ValueError, match="n_steps"):
        g.train_steps(buf, 0, 4, seeds=[1, 2])
    # (f) a failed call clears every member's token and moves no counter
    lib.fail_at = len(lib.calls) + 1
    for t in g.trainers:
        t._ts_token = "stale"
    with pytest.raises(ValueError, match="stub"):
        g.train_steps(buf, 3, 4, seeds=[1, 2], return_losses=False)
    assert all(t.total_it == IT0 + 5 and t._ts_token is None for t in g.trainers)


# ---- the solo driver, driven directly --------------------------------------------------------------------------------
class _Solo:
    """What ImplicitQLearning._run_burst reads of a trainer."""
    def __init__(self):
        self.total_it, self._ts_token, self._adam_t = IT0, None, {"v": 0, "q": 0, "pi": 0}
        self.tables, self.lookahead, self.rings = [], [], []

    def _scalar_table(self, k, inv):
        self.tables.append((k, inv))
        return np.full((k, 12), float(len(self.tables)), dtype=np.float32)

    def _lookahead_table(self, k, inv):
        self.lookahead.append((k, inv))

    def _read_rings(self, k, stream, losses, stats):
        self.rings.append((k, stream))
        for a in (losses, stats):
            if a is not None:
                assert a.shape[0] == k
                a[:] = len(self.rings)


def _solo_burst(tr, n_steps, B, calls, chunk=2, losses=False, stats=False, token=None, fail_at=None):
    def call(tab, k, offset, flags):
        assert tab.shape == (k, 12) and tab[0, 0] == len(tr.tables)       # this chunk's table
        calls.append((k, offset, flags))
        return hb.E_INVAL if len(calls) == fail_at else 0
    return T.ImplicitQLearning._run_burst(tr, n_steps, B, 1.0 / B, chunk, losses, stats, "stream", call, token)


@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("n_steps", [0, 1, 2, 5])
def test_solo_driver_chunks_offsets_and_lookahead(n_steps, B, monkeypatch):
    _lib(monkeypatch)
    tr, calls = _Solo(), []
    _solo_burst(tr, n_steps, B, calls, token=lambda: ("tok",))
    ks = {0: [], 1: [1], 2: [2], 5: [2, 2, 1]}[n_steps]
    starts = [IT0 + sum(ks[:i]) for i in range(len(ks))]
    assert [(k, off) for k, off, _ in calls] == [(k, t * 2) for k, t in zip(ks, starts)]               # (a)
    assert [f for _, _, f in calls] == [0, hb.TS_CONTINUE, hb.TS_CONTINUE][:len(ks)]                  # (b)
    assert tr.tables == [(k, 1.0 / B) for k in ks] and tr.rings == [(k, "stream") for k in ks]
    # the table computed ahead is the next chunk's length, the last chunk's own after the last one
    assert tr.lookahead == [(k, 1.0 / B) for k in (ks[1:] + ks[-1:])]
    assert tr.total_it == IT0 + n_steps and tr._ts_token == (("tok",) if n_steps else None)


def test_solo_driver_continues_exactly_on_an_equal_token(monkeypatch):
    _lib(monkeypatch)
    tr, calls = _Solo(), []
    versions = iter([1, 1, 2, 2, 2])
    tr._ts_token = ("buf", 1)
    _solo_burst(tr, 5, 4, calls, chunk=1, token=lambda: ("buf", next(versions)))        # evaluated per chunk
    assert [f for _, _, f in calls] == [hb.TS_CONTINUE, hb.TS_CONTINUE, 0, hb.TS_CONTINUE, hb.TS_CONTINUE]
    assert tr._ts_token == ("buf", 2)
    with pytest.raises(StopIteration):
        next(versions)


@pytest.mark.parametrize("n_steps", [0, 5])
def test_solo_driver_without_a_token_never_continues(n_steps, monkeypatch):
    _lib(monkeypatch)
    tr, calls = _Solo(), []
    tr._ts_token = ("tok",)            # (another kind's: dropped before the loop, also when there are no steps)
    _solo_burst(tr, n_steps, 3, calls)
    assert [f for _, _, f in calls] == [0] * len(calls) and len(calls) == (3 if n_steps else 0)
    assert tr._ts_token is None                                                                     # (d)


@pytest.mark.parametrize("token", [None, lambda: ("tok",)])
def test_solo_driver_failed_second_chunk(token, monkeypatch):
    _lib(monkeypatch)
    tr, calls = _Solo(), []
    with pytest.raises(ValueError, match="stub"):
        _solo_burst(tr, 5, 4, calls, token=token, fail_at=2)
    assert len(calls) == 2 and tr._ts_token is None and tr.total_it == IT0 + 2                      # (c)
    assert len(tr.rings) == 1 and len(tr.lookahead) == 1


@pytest.mark.parametrize("n_steps", [0, 5])
def test_solo_driver_return_shapes(n_steps, monkeypatch):
    _lib(monkeypatch)
    for want_losses in (False, True):
        for want_stats in (False, True):
            res = _solo_burst(_Solo(), n_steps, 4, [], losses=want_losses, stats=want_stats)
            losses, stats = res if want_stats else (res, None)
            assert isinstance(res, tuple) == want_stats                                             # (e)
            assert (losses is None) == (not want_losses) and (stats is None) == (not want_stats)
            chunk_of_step = np.repeat([1.0, 2.0, 3.0], [2, 2, 1])[:n_steps]       # rings land in [done - k: done]
            if want_losses:
                assert losses.shape == (n_steps, 3) and losses.dtype == np.float32
                assert np.array_equal(losses, np.repeat(chunk_of_step[:, None], 3, axis=1))
            if want_stats:
                assert stats.shape == (n_steps, N_STATS) and stats.dtype == np.float32
                assert np.array_equal(stats[:, 0], chunk_of_step)


def test_solo_driver_clamps_chunk(monkeypatch):
    _lib(monkeypatch)
    for chunk, ks in ((0, [1, 1, 1]), (-5, [1, 1, 1]), (10 ** 9, [3])):
        calls = []
        _solo_burst(_Solo(), 3, 4, calls, chunk=chunk)
        assert [k for k, _, _ in calls] == ks
    calls = []
    _solo_burst(_Solo(), T.K_MAX + 1, 4, calls, chunk=10 ** 9)
    assert [k for k, _, _ in calls] == [T.K_MAX, 1]


# ---- the group driver, driven directly -------------------------------------------------------------------------------
def _group_burst(g, n_steps, Bs, calls, chunk=2, losses=False, stats=False, fail_at=None):
    K = len(Bs)

    def call(grp, B_arr, tab_ptrs, k, seed_arr, offs, stream):
        assert grp is g._group() and list(B_arr) == Bs and len(tab_ptrs) == K and all(tab_ptrs)
        assert list(seed_arr) == [1, 2 ** 64 - 2][:K]                    # masked to 64 bits
        calls.append((k, list(offs)))
        return hb.E_INVAL if len(calls) == fail_at else 0
    return G.ImplicitQLearningGroup._run_burst(g, n_steps, Bs, [1.0 / B for B in Bs], [1, -2][:K], chunk, losses, stats,
                                               call)


@pytest.mark.parametrize("n_steps", [1, 2, 5])
def test_group_driver_chunks_and_offsets(n_steps, monkeypatch):
    lib, g, calls = _lib(monkeypatch), _group(2, mixed_batch=True), []
    g.trainers[1].total_it = IT0 + 7
    _group_burst(g, n_steps, [3, 4], calls)
    ks = {1: [1], 2: [2], 5: [2, 2, 1]}[n_steps]
    starts = [sum(ks[:i]) for i in range(len(ks))]
    assert calls == [(k, [(IT0 + s) * 2, (IT0 + 7 + s) * 2]) for k, s in zip(ks, starts)]            # (a), half = 2
    assert [t.tables for t in g.trainers] == [[(k, 1.0 / B) for k in ks] for B in (3, 4)]
    assert [t.total_it for t in g.trainers] == [IT0 + n_steps, IT0 + 7 + n_steps]
    assert all(t._ts_token is None for t in g.trainers) and not lib.calls      # no losses wanted: none read


def test_group_driver_clears_every_token_before_it_raises(monkeypatch):
    _lib(monkeypatch)
    g, calls = _group(2, mixed_batch=True), []
    with pytest.raises(ValueError, match="stub"):
        _group_burst(g, 5, [3, 4], calls, fail_at=2)
    assert [k for k, _ in calls] == [2, 2]
    assert all(t._ts_token is None and t.total_it == IT0 + 2 for t in g.trainers)                  # (c), (f)
    for t in g.trainers:
        t._ts_token = "stale"
    with pytest.raises(ValueError, match="stub"):                  # ... on a first chunk that fails too
        _group_burst(g, 1, [3, 4], [], fail_at=1)
    assert all(t._ts_token is None and t.total_it == IT0 + 2 for t in g.trainers)


def test_group_driver_return_shapes_and_chunk_clamp(monkeypatch):
    lib = _lib(monkeypatch)
    for want_losses in (False, True):
        for want_stats in (False, True):
            res = _group_burst(_group(2, mixed_batch=True), 5, [3, 4], [], losses=want_losses, stats=want_stats)
            if want_stats:                                         # (e) the statistics INSTEAD of the losses
                assert res.shape == (5, 2, N_STATS) and res.dtype == np.float32 and np.all(res == 2.0)
            elif want_losses:
                assert res.shape == (2, 5, 3) and res.dtype == np.float32
            else:
                assert res is None
    assert [c[1] for c in lib.calls] == [2, 2, 1] * 2              # the losses are read whenever they are wanted
    monkeypatch.setattr(hb, "IQLHIP_GROUP_MAX_STEPS", 3)
    calls = []
    _group_burst(_group(2, mixed_batch=True), 7, [3, 4], calls, chunk=10 ** 9)
    assert [k for k, _ in calls] == [3, 3, 1]
    calls = []
    _group_burst(_group(2, mixed_batch=True), 2, [3, 4], calls, chunk=0)
    assert [k for k, _ in calls] == [1, 1]


def test_group_of_one_results_take_the_group_shapes():
    reshape = G.ImplicitQLearningGroup._solo_burst_result
    for n in (1, 5):
        losses = np.arange(n * 3, dtype=np.float32).reshape(n, 3)
        stats = np.arange(n * N_STATS, dtype=np.float32).reshape(n, N_STATS)
        got = reshape(losses, False)
        assert got.shape == (1, n, 3) and np.array_equal(got[0], losses)                # [K, n, 3]
        for solo in ((losses, stats), (None, stats)):
            got = reshape(solo, True)
            assert got.shape == (n, 1, N_STATS) and np.array_equal(got[:, 0], stats)    # [n, K, 16]
    assert reshape(None, False) is None
