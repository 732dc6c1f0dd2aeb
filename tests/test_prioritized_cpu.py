"""CPU tests of prioritised replay inside the chunk graphs (DESIGN.md 6j "Prioritised replay inside the chunk graphs"): the
Python layer's argument checks, the burst's continuation token and version bump against a recording stand-in for the
library, and the order of the lag-1 loop (tests/prioritized_ref.py) on the inputs of tests/test_hip_prioritized.py's
duplicate test."""
import os
import re

import numpy as np
import pytest
import torch

import iqlhip_binding as hb
import iqlhip_trainer as T
import iqlhip_weighted as wtd
import prioritized_ref as PR
import weighted_update_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("iqlhip_weights_update_td", "iqlhip_train_steps_prioritized", "iqlhip_train_steps_prioritized_prepare")
IT0 = 10


# ---------------------------------------------------------------- the Python layer's checks
def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    bound = {name for name, _, _ in hb.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in bound, name


@pytest.mark.parametrize("alpha,eps", [(-0.1, 1e-3), (float("nan"), 1e-3), (float("inf"), 1e-3), (0.6, -1e-3),
                                       (0.6, float("nan")), (0.6, float("inf")), (0.0, 0.0), ("x", 1e-3), (0.6, None)])
def test_priority_arguments_refused(alpha, eps):
    with pytest.raises(ValueError):
        wtd.check_priority_args(alpha, eps)


def test_priority_arguments_accepted():
    assert wtd.check_priority_args(0.6, 1e-3) == (0.6, 1e-3)
    assert wtd.check_priority_args(0, 1e-3) == (0.0, 1e-3)          # alpha = 0: every priority 1
    assert wtd.check_priority_args(1, 0) == (1.0, 0.0)              # eps = 0 with alpha > 0: a zero TD error weighs 0


def test_td_update_argument_shapes():
    idx, td = torch.zeros(5, dtype=torch.int64), torch.zeros(5, 2)
    assert wtd.check_td_args(idx, td) == 5
    for bad_idx, bad_td in ((idx.int(), td), (idx, td.double()), (idx, torch.zeros(5)), (idx, torch.zeros(5, 3)),
                            (idx, torch.zeros(4, 2)), (idx.reshape(5, 1), td), (idx.numpy(), td), (idx, td.numpy())):
        with pytest.raises(ValueError):
            wtd.check_td_args(bad_idx, bad_td)
    with pytest.raises(ValueError):
        wtd.check_td_args(idx, td, torch.device("cuda", 0))          # host tensors for a table on a GPU


# ---------------------------------------------------------------- the burst against a recording library
class _Lib:
    def __init__(self, fail_at=None):
        self.calls, self.fail_at = [], fail_at

    def iqlhip_train_steps_prioritized(self, ctx, rows, ld, size, B, tab, k, seed, offset, flags, stream, table, beta, alpha, eps):
        self.calls.append(("prioritized", int(k), int(offset), int(flags), (beta, alpha, eps)))
        return hb.E_INVAL if len(self.calls) == self.fail_at else 0

    def iqlhip_train_steps_weighted_is(self, ctx, rows, ld, size, B, tab, k, seed, offset, flags, stream, table, beta):
        self.calls.append(("weighted_is", int(k), int(offset), int(flags), (beta,)))
        return 0

    def iqlhip_read_loss_ring(self, ctx, buf, k, stream):
        return 0

    def iqlhip_read_stats_ring(self, ctx, buf, k, stream):
        return 0

    def iqlhip_last_error(self):
        return b"stub"


class _Buf:
    _ld, _writes, _size, _gpu = 44, 0, 9, True
    _weights, _weights_gen, _weights_version, _weights_updatable = object(), 7, 3, True

    def __init__(self):
        self._rows = torch.zeros(4, 44)


class _Tab:
    updatable, generation, _table, _version = True, 9, object(), 5
    version = property(lambda self: self._version)


def _trainer(monkeypatch, fail_at=None):
    lib = _Lib(fail_at)
    monkeypatch.setattr(hb, "lib", lambda: lib)
    tr = object.__new__(T.ImplicitQLearning)
    tr._ctx, tr._dp_world, tr._dp_rank, tr._ts_token, tr.total_it, tr._step_stats = None, 1, 0, None, IT0, True
    tr._precision = "f32"

    def weighted_args(buf, b, weights=None):
        if weights is None:
            return 5000, buf._weights, (buf._weights_gen, buf._weights_version)
        return 5000, weights._table, (weights.generation, weights.version)
    tr._weighted_args = weighted_args
    tr._prepare = lambda rows: None
    tr._scalar_table = lambda k, inv: np.zeros((k, 12), dtype=np.float32)
    tr._lookahead_table = lambda k, inv: None
    tr._stream = lambda: 0
    return lib, tr


def test_pieces_of_one_call_continue_and_calls_never_do(monkeypatch):
    lib, tr = _trainer(monkeypatch)
    buf = _Buf()
    losses = tr.train_steps_prioritized(buf, 5, 4, seed=3, alpha=0.7, eps=0.01, is_beta=0.4, chunk=2)
    assert losses.shape == (5, 3)
    # the first piece draws afresh, the later pieces go on with the lag-1 chain; offsets are train_steps' own
    assert lib.calls == [("prioritized", 2, IT0 * 2, 0, (0.4, 0.7, 0.01)),
                         ("prioritized", 2, (IT0 + 2) * 2, hb.TS_CONTINUE, (0.4, 0.7, 0.01)),
                         ("prioritized", 1, (IT0 + 4) * 2, hb.TS_CONTINUE, (0.4, 0.7, 0.01))]
    assert tr.total_it == IT0 + 5
    # the same call again on the untouched buffer: its first piece never continues the previous call
    for _ in range(3):
        n = len(lib.calls)
        tr.train_steps_prioritized(buf, 4, 4, seed=3, chunk=2, return_losses=False)
        assert [c[3] for c in lib.calls[n:]] == [0, hb.TS_CONTINUE]
    # ... nor does a weighted call with is_beta behind it, nor a prioritised call behind that one
    tr.train_steps_weighted(buf, 2, 4, seed=3, is_beta=0.4, return_losses=False)
    tr.train_steps_prioritized(buf, 2, 4, seed=3, return_losses=False)
    assert [c[3] for c in lib.calls[-2:]] == [0, 0]


def test_chunk_is_rounded_down_to_an_even_number(monkeypatch):
    lib, tr = _trainer(monkeypatch)
    tr.train_steps_prioritized(_Buf(), 7, 4, chunk=3, return_losses=False)
    assert [c[1] for c in lib.calls] == [2, 2, 2, 1]
    lib.calls.clear()
    tr.train_steps_prioritized(_Buf(), 3, 4, chunk=1, return_losses=False)
    assert [c[1] for c in lib.calls] == [2, 1]


def test_version_moves_once_per_library_call(monkeypatch):
    lib, tr = _trainer(monkeypatch)
    buf, tab = _Buf(), _Tab()
    v0 = buf._weights_version
    tr.train_steps_prioritized(buf, 5, 4, chunk=2, return_losses=False)          # three library calls
    assert buf._weights_version == v0 + 3 and len(lib.calls) == 3
    tr.train_steps_prioritized(buf, 2, 4, return_losses=False, weights=tab)       # the table given instead: its version
    assert buf._weights_version == v0 + 3 and tab.version == 6
    tr.train_steps_prioritized(buf, 0, 4, return_losses=False)                    # no steps: no call, no bump
    assert buf._weights_version == v0 + 3 and len(lib.calls) == 4


def test_failed_piece_leaves_no_token_and_no_bump(monkeypatch):
    lib, tr = _trainer(monkeypatch, fail_at=2)
    buf = _Buf()
    v0 = buf._weights_version
    with pytest.raises(ValueError, match="stub"):
        tr.train_steps_prioritized(buf, 5, 4, chunk=2, return_losses=False)
    assert len(lib.calls) == 2 and tr._ts_token is None and tr.total_it == IT0 + 2 and buf._weights_version == v0 + 1


def test_refusals_before_any_library_call(monkeypatch):
    lib, tr = _trainer(monkeypatch)
    buf = _Buf()
    for kw in ({"alpha": -1.0}, {"eps": float("nan")}, {"alpha": 0.0, "eps": 0.0}, {"is_beta": -0.5},
               {"is_beta": float("inf")}):
        with pytest.raises(ValueError):
            tr.train_steps_prioritized(buf, 2, 4, **kw)
    static = _Buf()
    static._weights_updatable = False
    with pytest.raises(ValueError, match="updatable"):
        tr.train_steps_prioritized(static, 2, 4)
    tab = _Tab()
    tab.updatable = False
    with pytest.raises(ValueError, match="updatable"):
        tr.train_steps_prioritized(buf, 2, 4, weights=tab)
    tr._precision = "bf16"
    with pytest.raises(NotImplementedError, match="bf16"):
        tr.train_steps_prioritized(buf, 2, 4)
    tr._precision = "f32"
    tr._step_stats = False
    with pytest.raises(ValueError, match="set_step_stats"):
        tr.train_steps_prioritized(buf, 2, 4, return_stats=True)
    assert lib.calls == [] and tr.total_it == IT0 and buf._weights_version == 3


# ---------------------------------------------------------------- the order of the loop
def _dup_table():
    return U.Table(PR.dup_weights(), max_weight=PR.DUP_MAX_WEIGHT)


def test_lag_loop_is_the_eager_calls_in_the_stated_order():
    """run_loop(lag=True) written out by hand for three steps: draw t + 1 comes before the update of t."""
    td_fn = PR.model_td(np.linspace(0.01, 3.0, PR.DUP_N))
    a, b = _dup_table(), _dup_table()
    batches = PR.run_loop(a, 3, PR.DUP_B, PR.DUP_SEED, 40, td_fn, PR.DUP_ALPHA, PR.DUP_EPS)
    state = 0.0
    i0 = b.draw_indices(PR.DUP_B, PR.DUP_SEED, 40, 0)
    i1 = b.draw_indices(PR.DUP_B, PR.DUP_SEED, 40, PR.DUP_B)
    td, state = td_fn(0, i0, state)
    b.update(i0, PR.priority64(td, PR.DUP_ALPHA, PR.DUP_EPS).astype(np.float32))
    i2 = b.draw_indices(PR.DUP_B, PR.DUP_SEED, 40, 2 * PR.DUP_B)
    td, state = td_fn(1, i1, state)
    b.update(i1, PR.priority64(td, PR.DUP_ALPHA, PR.DUP_EPS).astype(np.float32))
    b.draw_indices(PR.DUP_B, PR.DUP_SEED, 40, 3 * PR.DUP_B)
    td, state = td_fn(2, i2, state)
    b.update(i2, PR.priority64(td, PR.DUP_ALPHA, PR.DUP_EPS).astype(np.float32))
    assert all(np.array_equal(x, y) for x, y in zip(batches, (i0, i1, i2)))
    assert np.array_equal(a.q, b.q) and a.version == b.version == 3 and a.flags == 0


def test_the_two_update_orders_give_different_tables_on_the_duplicate_inputs():
    """The inputs of test_hip_prioritized's duplicate test: 8 weighted rows, batches of 64.  Every batch holds duplicates,
    every step redraws rows the step before re-prioritised, and drawing step t + 1 before or after the update of step t
    ends in different tables — the GPU test's discriminating assertion has something to discriminate."""
    td_fn = PR.model_td(np.linspace(0.01, 3.0, PR.DUP_N))
    lag, first = _dup_table(), _dup_table()
    bl = PR.run_loop(lag, PR.DUP_STEPS, PR.DUP_B, PR.DUP_SEED, 0, td_fn, PR.DUP_ALPHA, PR.DUP_EPS, lag=True)
    bf = PR.run_loop(first, PR.DUP_STEPS, PR.DUP_B, PR.DUP_SEED, 0, td_fn, PR.DUP_ALPHA, PR.DUP_EPS, lag=False)
    for batch in bl + bf:
        assert set(batch.tolist()) <= set(PR.DUP_ROWS.tolist())             # only weighted rows are ever drawn
        assert len(set(batch.tolist())) < PR.DUP_B                          # duplicates, by pigeonhole
    assert np.array_equal(bl[0], bf[0])                                     # step 0 is the same fresh draw
    assert any(not np.array_equal(x, y) for x, y in zip(bl[1:], bf[1:]))    # the draws part ways after step 0
    assert not np.array_equal(lag.q, first.q)
    assert np.all(lag.q[np.setdiff1d(np.arange(PR.DUP_N), PR.DUP_ROWS)] == 0)
