"""Prioritised replay inside the chunk graphs (trainer.train_steps_prioritized; DESIGN.md 6j "Prioritised replay inside the
chunk graphs") and the eager update by TD errors (update_sample_weights_td).

The reference of every burst test is the eager lag-1 loop written with the public eager calls, the draw of step t + 1 in
front of the update of step t:
    idx, c = draw(0)
    for t: nxt = draw(t + 1); train(gather(idx), loss_weights=c, return_td=True);
           update_sample_weights_td(idx, last_td_errors(), alpha, eps); idx, c = nxt
A burst equals it bit for bit: the priority formula is ONE device function for both, everything else is integers.

The eager update against float64 (max(|e1|, |e2|) + eps) ** alpha: the bound is four times the largest relative error
measured on the device (profiles/prioritized_parity_margins.txt: 3.8e-7, so 1.52e-6) and never above 1e-5 — in the grid
|alpha log2 x| <= 24, one ulp of the log result is at most 2^-19 absolute, after exp2 about 1.3e-6 relative per ulp, and a
few ulps come from the two intrinsics and the product."""
import numpy as np
import pytest
import torch

import prioritized_ref as PR
import synth
from burst_twins import (eager_prioritized_segment as _eager, fourth_power_weights,      # (shared with the shape table's tests)
                         table_of as _table)

pytestmark = pytest.mark.gpu

HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
S, A, N = 17, 6, 2000
MAX_WEIGHT = 64.0
FORMULA_BOUND = min(4 * 3.8e-7, 1e-5)          # 4 x the measured margin (module docstring), capped


def _trainer(dropout=0.0):
    from hip_helpers import build_hip_trainer
    return build_hip_trainer(synth.synth_params(S, A, seed=3, gaussian=True), S, A, True, HYPER, LRS, 1000, dropout=dropout)


def _losses(log):
    return np.array([log["value_loss"], log["q_loss"], log["actor_loss"]], dtype=np.float32)


def _weights(n=N):
    return fourth_power_weights(n)


def _buffer(w=None, n=N, updatable=True):
    """The 2 000-row buffer of test_hip_loss_weights._burst_buffer with an updatable table at a fixed scale."""
    import iql
    buf = iql.ReplayBuffer(S, A, n, "cuda")
    buf.load_d4rl_dataset(synth.synth_transitions(n, S, A, seed=5))
    w = _weights(n) if w is None else w
    if updatable:
        buf.set_sample_weights(w, updatable=True, max_weight=MAX_WEIGHT)
    else:
        buf.set_sample_weights(w)
    return buf


def _assert_burst_equals_eager(burst_buf, eager_buf, burst, eager, lb, le, what):
    from hip_helpers import assert_same_trainer_state
    assert lb.dtype == np.float32 and lb.shape == le.shape
    assert np.array_equal(lb, le), (what, lb, le)
    assert_same_trainer_state(burst, eager, what)
    qb, tb = _table(burst_buf)
    qe, te = _table(eager_buf)
    assert np.array_equal(qb, qe), (what, int(np.sum(qb != qe)))
    assert tb == te == int(np.sum(qb.astype(object)))
    assert burst_buf.sample_weights_flags() == 0 and eager_buf.sample_weights_flags() == 0


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("B", [64, 300])
def test_burst_equals_the_eager_lag_loop(B):
    from hip_helpers import assert_same_trainer_state
    bufs = [_buffer() for _ in range(3)]
    q0, _ = _table(bufs[0])
    burst, small, eager = (_trainer() for _ in range(3))
    lb = burst.train_steps_prioritized(bufs[0], 5, B, seed=9, alpha=0.6, eps=1e-3, is_beta=0.5)
    le = _eager(eager, bufs[2], 5, B, 9, 0.6, 1e-3, 0.5)
    assert lb.shape == (5, 3)
    _assert_burst_equals_eager(bufs[0], bufs[2], burst, eager, lb, le, f"burst vs eager, B={B}")
    assert np.any(_table(bufs[0])[0] != q0)                                  # (priorities were written)
    ls = small.train_steps_prioritized(bufs[1], 5, B, seed=9, alpha=0.6, eps=1e-3, is_beta=0.5, chunk=2)
    assert np.array_equal(ls, lb)
    assert_same_trainer_state(small, burst, "chunk=2 vs chunk=64")
    assert np.array_equal(_table(bufs[1])[0], _table(bufs[0])[0]) and _table(bufs[1])[1] == _table(bufs[0])[1]


# ------------------------------------------------------------------------------------------------------------------ 2
def test_duplicates_and_the_lag_are_exercised():
    bufs = [_buffer(PR.dup_weights()) for _ in range(3)]
    burst, eager, other = (_trainer() for _ in range(3))
    args = (PR.DUP_ALPHA, PR.DUP_EPS, PR.DUP_BETA)
    idx0 = bufs[0].draw_weighted_indices(PR.DUP_B, PR.DUP_SEED, 0).cpu().numpy()
    assert set(idx0.tolist()) <= set(PR.DUP_ROWS.tolist()) and len(set(idx0.tolist())) <= 8      # duplicates in every batch
    lb = burst.train_steps_prioritized(bufs[0], PR.DUP_STEPS, PR.DUP_B, seed=PR.DUP_SEED, alpha=args[0], eps=args[1],
                                       is_beta=args[2])
    le = _eager(eager, bufs[1], PR.DUP_STEPS, PR.DUP_B, PR.DUP_SEED, *args)
    _assert_burst_equals_eager(bufs[0], bufs[1], burst, eager, lb, le, "8 weighted rows")
    # the other order — update t before the draw of t + 1 — ends in another table: the equality above can tell them apart
    _eager(other, bufs[2], PR.DUP_STEPS, PR.DUP_B, PR.DUP_SEED, *args, lag=False)
    q_lag, q_first = _table(bufs[0])[0], _table(bufs[2])[0]
    assert not np.array_equal(q_lag, q_first)
    rest = np.setdiff1d(np.arange(N), PR.DUP_ROWS)
    assert np.all(q_lag[rest] == 0) and np.all(q_lag[PR.DUP_ROWS] > 0)


# ------------------------------------------------------------------------------------------------------------------ 3
def test_three_table_levels_and_the_tree_equals_a_rebuild():
    import iqlhip_weighted as wtd
    n, B = 5000, 64                                  # 79 level-0 nodes, 2 level-1 nodes under a top
    bufs = [_buffer(n=n) for _ in range(2)]
    burst, eager = _trainer(), _trainer()
    lb = burst.train_steps_prioritized(bufs[0], 4, B, seed=5, alpha=0.6, eps=1e-3, is_beta=0.5)
    le = _eager(eager, bufs[1], 4, B, 5, 0.6, 1e-3, 0.5)
    _assert_burst_equals_eager(bufs[0], bufs[1], burst, eager, lb, le, "three levels")
    # the tree holds what a build over the dequantised leaves holds (sums in every node, not only the leaves' differences)
    q, total = _table(bufs[0])
    e = int(np.floor(np.log2(MAX_WEIGHT)))
    w = (q.astype(np.float64) * 2.0 ** (e - 38)).astype(np.float32)
    fresh = wtd.SampleWeights(w, updatable=True, max_weight=MAX_WEIGHT)
    assert np.array_equal(fresh.leaves(), q) and fresh.total() == total
    a = bufs[0].draw_weighted_indices(512, 3, 0).cpu().numpy()
    assert np.array_equal(a, fresh.draw_indices(512, 3, 0).cpu().numpy())    # ... and the descent through it agrees


# ------------------------------------------------------------------------------------------------------------------ 4
def test_alpha_zero_on_unit_weights_is_the_weighted_burst():
    from hip_helpers import assert_same_trainer_state
    B, beta = 64, 0.5
    ones = np.ones(N, dtype=np.float32)
    ba, bb = _buffer(ones), _buffer(ones)
    q0, t0 = _table(ba)
    a, b = _trainer(), _trainer()
    la = a.train_steps_prioritized(ba, 5, B, seed=9, alpha=0.0, eps=1e-3, is_beta=beta)
    lw = b.train_steps_weighted(bb, 5, B, seed=9, is_beta=beta)
    assert np.array_equal(la, lw)
    assert_same_trainer_state(a, b, "alpha = 0 on unit weights")
    q1, t1 = _table(ba)
    assert np.array_equal(q1, q0) and t1 == t0 and ba.sample_weights_flags() == 0      # every priority is exactly 1.0


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("first,second", [(3, 2), (4, 2)])
def test_two_calls_are_two_fresh_draws(first, second):
    from hip_helpers import assert_same_trainer_state
    B = 64
    bufs = [_buffer() for _ in range(3)]
    burst, eager, single = (_trainer() for _ in range(3))
    l1 = burst.train_steps_prioritized(bufs[0], first, B, seed=4, alpha=0.6, eps=1e-3, is_beta=0.3)
    l2 = burst.train_steps_prioritized(bufs[0], second, B, seed=4, alpha=0.9, eps=1e-2, is_beta=0.9)
    e1 = _eager(eager, bufs[1], first, B, 4, 0.6, 1e-3, 0.3)
    e2 = _eager(eager, bufs[1], second, B, 4, 0.9, 1e-2, 0.9)          # its step 0: a fresh draw from the updated table
    _assert_burst_equals_eager(bufs[0], bufs[1], burst, eager, np.concatenate([l1, l2]), np.concatenate([e1, e2]),
                               f"{first} + {second} steps")
    # one call of first + second steps is another computation (its step `first` was drawn one update earlier)
    ls = single.train_steps_prioritized(bufs[2], first + second, B, seed=4, alpha=0.6, eps=1e-3, is_beta=0.3)
    assert np.array_equal(ls[:first], l1)
    assert not np.array_equal(_table(bufs[2])[0], _table(bufs[0])[0])
    # a plain weighted call behind it stays right: it gathers afresh from the table as it now stands
    lw = burst.train_steps_weighted(bufs[0], 2, B, seed=4, is_beta=0.5)
    idx, c = bufs[1].draw_weighted_indices(2 * B, 4, eager.total_it * (B // 2), is_beta=0.5, batch_size=B)
    ew = np.stack([_losses(eager.train(bufs[1].gather(idx[k * B:(k + 1) * B]), loss_weights=c[k * B:(k + 1) * B]))
                   for k in range(2)])
    assert np.array_equal(lw, ew)
    assert_same_trainer_state(burst, eager, "weighted call behind a prioritised one")


# ------------------------------------------------------------------------------------------------------------------ 6
def test_statistics_clipping_and_dropout_together():
    B = 64
    bufs = [_buffer() for _ in range(2)]
    trs = [_trainer(dropout=0.1) for _ in range(2)]
    for tr in trs:
        tr.set_dropout_seed(77)
        tr.set_step_stats(True)
        tr.set_grad_clip(1.0)
    lb, sb = trs[0].train_steps_prioritized(bufs[0], 3, B, seed=9, alpha=0.6, eps=1e-3, is_beta=0.5, return_stats=True)
    le = _eager(trs[1], bufs[1], 3, B, 9, 0.6, 1e-3, 0.5)
    assert sb.shape == (3, 16) and np.all(np.isfinite(sb))
    _assert_burst_equals_eager(bufs[0], bufs[1], trs[0], trs[1], lb, le, "statistics, clipping and dropout")
    assert trs[0].last_grad_clip() == trs[1].last_grad_clip()


# ------------------------------------------------------------------------------------------------------------------ 7
def _td_grid(alpha_count=1):
    """TD magnitudes from 1e-6 to 1e2 (log-spaced, both signs, the larger one in either column), one row each."""
    mag = np.logspace(-6, 2, 1536).astype(np.float32)
    rng = np.random.RandomState(8)
    other = (mag * rng.rand(mag.size)).astype(np.float32)
    sign = np.where(rng.rand(mag.size) < 0.5, -1.0, 1.0).astype(np.float32)
    swap = rng.rand(mag.size) < 0.5
    td = np.stack([np.where(swap, other, mag * sign), np.where(swap, mag * sign, other)], axis=1).astype(np.float32)
    return td


@pytest.mark.parametrize("alpha", [0.3, 0.6, 1.0])
def test_update_td_against_float64(alpha):
    import iqlhip_weighted as wtd
    eps = 1e-3
    td = _td_grid()
    m = td.shape[0]
    tab = wtd.SampleWeights(np.ones(m, dtype=np.float32), updatable=True, max_weight=128.0)      # scale e = 7
    idx = torch.arange(m, dtype=torch.int64, device="cuda")
    tab.update_td(idx, torch.from_numpy(td).cuda(), alpha, eps)
    got = tab.leaves().astype(np.float64) * 2.0 ** (7 - 38)
    want = (np.max(np.abs(td.astype(np.float64)), axis=1) + np.float64(np.float32(eps))) ** np.float64(np.float32(alpha))
    keep = want >= 2.0 ** (7 - 10)                    # quantisation (2^-31 absolute) below 2^-28 relative: under the bound
    assert keep.sum() > 200
    err = np.max(np.abs(got[keep] - want[keep]) / want[keep])
    print(f"update_td alpha={alpha}: max rel err {err:.3g} over {int(keep.sum())} rows (bound {FORMULA_BOUND:.3g})")
    assert err <= FORMULA_BOUND, err
    assert tab.flags() == 0 and tab.version == 1


def test_update_td_skips_flags_and_duplicates():
    import iqlhip_weighted as wtd
    n = 200
    tab = wtd.SampleWeights(np.ones(n, dtype=np.float32), updatable=True, max_weight=64.0)
    q0 = tab.leaves()
    idx = torch.tensor([5, 6, 7, 150, 9, 9, 9], dtype=torch.int64, device="cuda")
    td = torch.tensor([[1.0, 0.5], [float("nan"), 0.5], [0.5, float("inf")], [1.0, 1.0], [4.0, 0.0], [0.0, -2.0], [0.25, 0.1]],
                      dtype=torch.float32, device="cuda")
    tab.update_td(idx, td, 1.0, 0.0, bound=100)                                   # row 150 lies beyond the bound
    q = tab.leaves()
    one = int(q0[0])
    assert tab.flags() == 1 | 4
    assert q[6] == one and q[7] == one and q[150] == one                          # skipped: as they were
    assert q[5] == one and q[9] == one // 4                                       # |1.0|; the LAST entry of row 9: 0.25
    assert np.array_equal(np.delete(q, [9]), np.delete(q0, [9]))
    # a NaN in the smaller error is not dropped by the maximum
    tab.clear_flags()
    tab.update_td(idx[:1], torch.tensor([[3.0, float("nan")]], device="cuda"), 1.0, 0.0)
    assert tab.flags() == 1 and tab.leaves()[5] == one
    for bad in ((-1.0, 1e-3), (0.5, -1e-3), (float("nan"), 1e-3), (0.0, 0.0)):
        with pytest.raises(ValueError):
            tab.update_td(idx, td, *bad)
    with pytest.raises(ValueError):
        wtd.SampleWeights(np.ones(n, dtype=np.float32)).update_td(idx, td, 0.6, 1e-3)          # a static table
    buf = _buffer(updatable=False)
    with pytest.raises(ValueError):
        buf.update_sample_weights_td(idx, td, 0.6, 1e-3)
    # the library itself refuses the same before any launch
    import iqlhip_binding as hb
    v = tab.version
    for alpha, eps in ((-1.0, 1e-3), (0.5, float("inf")), (0.0, 0.0)):
        rc = hb.lib().iqlhip_weights_update_td(tab._table, idx.data_ptr(), td.data_ptr(), 7, n, alpha, eps, None)
        assert rc == hb.E_INVAL, rc
    assert wtd.table_state(tab._table)[2] == v


# ------------------------------------------------------------------------------------------------------------------ 8
def test_refusals_leave_everything_untouched():
    from hip_helpers import arenas
    buf, static = _buffer(), _buffer(updatable=False)
    tr = _trainer()
    q0, t0 = _table(buf)
    before, it, ver = arenas(tr), tr.total_it, buf._weights_version
    with pytest.raises(ValueError, match="updatable"):
        tr.train_steps_prioritized(static, 2, 64, seed=1)
    with pytest.raises(ValueError, match="updatable"):
        tr.prepare_train_steps_prioritized(static, 64)
    for kw in ({"alpha": -0.5}, {"alpha": float("nan")}, {"eps": -1.0}, {"eps": float("inf")}, {"alpha": 0.0, "eps": 0.0},
               {"is_beta": -0.5}, {"is_beta": float("nan")}):
        with pytest.raises(ValueError):
            tr.train_steps_prioritized(buf, 2, 64, seed=1, **kw)
    tr.set_precision("bf16")
    with pytest.raises(NotImplementedError, match="bf16"):
        tr.train_steps_prioritized(buf, 2, 64, seed=1)
    with pytest.raises(NotImplementedError, match="bf16"):
        tr.prepare_train_steps_prioritized(buf, 64)
    # ... and the library itself, past the Python layer's checks: bf16 is IQLHIP_EUNSUPPORTED, a static table IQLHIP_EINVAL
    import iqlhip_binding as hb
    tab = np.zeros((2, 12), dtype=np.float32)         # (never read: every call below is refused in front of it)
    rows, ld = buf._rows.data_ptr(), buf._ld
    rc = hb.lib().iqlhip_train_steps_prioritized(tr._ctx, rows, ld, N, 64, tab.ctypes.data, 2, 1, 0, 0, tr._stream(),
                                                 buf._weights, 0.5, 0.6, 1e-3)
    assert rc == hb.E_UNSUPPORTED, rc
    tr.set_precision("f32")
    rc = hb.lib().iqlhip_train_steps_prioritized(tr._ctx, static._rows.data_ptr(), ld, N, 64, tab.ctypes.data, 2, 1, 0, 0,
                                                 tr._stream(), static._weights, 0.5, 0.6, 1e-3)
    assert rc == hb.E_INVAL, rc
    for beta, alpha, eps in ((0.5, -1.0, 1e-3), (0.5, 0.0, 0.0), (float("nan"), 0.6, 1e-3)):
        rc = hb.lib().iqlhip_train_steps_prioritized(tr._ctx, rows, ld, N, 64, tab.ctypes.data, 2, 1, 0, 0, tr._stream(),
                                                     buf._weights, beta, alpha, eps)
        assert rc == hb.E_INVAL, (rc, beta, alpha, eps)
    torch.cuda.synchronize()
    q1, t1 = _table(buf)
    import iqlhip_weighted as wtd
    assert np.array_equal(arenas(tr), before) and tr.total_it == it
    assert buf._weights_version == ver == wtd.table_state(buf._weights)[2]
    assert np.array_equal(q1, q0) and t1 == t0 and buf.sample_weights_flags() == 0
    # prepare rehearses the graphs: it trains nothing and changes no leaf
    tr.prepare_train_steps_prioritized(buf, 64)
    q2, t2 = _table(buf)
    assert np.array_equal(arenas(tr), before) and tr.total_it == it
    assert np.array_equal(q2, q0) and t2 == t0 and buf.sample_weights_flags() == 0 and buf._weights_version == ver
    # ... and the call behind it is the call without it
    twin_buf, twin = _buffer(), _trainer()
    la = tr.train_steps_prioritized(buf, 4, 64, seed=1)
    lb = twin.train_steps_prioritized(twin_buf, 4, 64, seed=1)
    assert np.array_equal(la, lb) and np.array_equal(_table(buf)[0], _table(twin_buf)[0])
