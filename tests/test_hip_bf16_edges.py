"""GPU tests of the bf16 step at edge shapes and row layouts, on both of its paths: the small-batch kernels (iql_fwd_kernel /
iql_bwd_kernel with bf16 operands: up to 512 rows, and any batch once S + A + 1 > 80) and the large-batch kernels
(iqlhip_lb_kernels.h: more than 512 rows with S + A + 1 <= 80, `use_lb` in csrc/iqlhip.hip).

Each edge shape is checked twice:
  * against the float64 oracle at the bf16 bounds of tests/test_hip_lb.py (losses rel 5e-3; gradients within 8.5e-2 in
    relative L2 per tensor, tensors of <= 32 elements within 2e-2 of the residual scale), plus one train step;
  * row layout: the gradient must equal the gradient of the same rows reversed and randomly permuted to fp32 summation
    accuracy (tests/helpers.py: permutation_bounds) — far tighter than the oracle bound, and at most a tenth of what
    dropping or doubling the smallest row group the kernels handle separately would move each tensor by.
Each case prints its worst errors against the oracle and its permutation margin (tolerance / that contribution)."""
import numpy as np
import pytest

from helpers import permutation_bounds, rows_of, step_batch, uses_large_batch_kernels, w0_lds_k
from test_hip_lb import GRAD_RL2, LOSS_RTOL, _check_grads

pytestmark = pytest.mark.gpu


def _hip():
    from hip_helpers import build_hip_trainer, read_params, to_torch_batch, unflatten_grads
    return build_hip_trainer, read_params, to_torch_batch, unflatten_grads


def _case(S, A, B, gaussian):
    import synth
    params = synth.synth_params(S, A, seed=700 + 3 * S + A, gaussian=gaussian)
    batch = step_batch(S, A, B, seed=800 + S + A + B)
    hyper = {"iql_tau": 0.8, "beta": 3.0, "discount": 0.99, "tau": 0.005, "deterministic": not gaussian}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    return params, batch, hyper, lrs


def _check_row_permutations(tr, params, batch, hyper, base, what):
    """base: the unflattened gradient of `batch` on trainer `tr`.  Returns (largest tolerance / contribution over the
    tensors held to the fp32 bound, largest observed difference / tolerance, the tensors bounded by their contribution)."""
    _, _, to_tb, unflat = _hip()
    B = batch["s"].shape[0]
    tols, margin, coarse = {}, 0.0, []
    for key, (tol, contrib) in permutation_bounds(params, batch, hyper).items():
        assert 0.0 < tol and 0.0 < contrib, (what, key, tol, contrib)
        if tol > 0.1 * contrib:
            # The fp32 bound is not 10x below this group's contribution where one row's share of a sum of B rows is
            # small next to the bound, which grows with every row's magnitude: at 8 192 rows the last row's advantage
            # is small and it moves the value net's tensors by 0.3 - 1.6x the bound; at 1 024 rows of 2-wide inputs
            # the policy's w0 by 2.5x it.  Such a tensor is bounded against the contribution's scale instead: half
            # of it, so a dropped or doubled group still moves it by twice the tolerance.
            tol = 0.5 * contrib
            coarse.append(key)
        else:
            margin = max(margin, tol / contrib)
        tols[key] = tol
    seen = 0.0
    for name, perm in (("reversed", np.arange(B)[::-1]), ("random", np.random.default_rng(B).permutation(B))):
        got, _ = unflat(tr, tr.flat_gradient(to_tb(rows_of(batch, perm))))
        for (net, t), tol in tols.items():
            d = float(np.max(np.abs(got[net][t].astype(np.float64) - base[net][t])))
            assert d <= tol, (what, name, net, t, d, tol)
            seen = max(seen, d / tol)
    return margin, seen, coarse


# (S, A, B, gaussian, large-batch kernels, w0_lds_k): the path of each case, checked against helpers' restatements of
# use_lb and iqlhip_create's layer-0 staging rule (w0_lds_k > 64: layer-0 weights staged by LDS-DMA; 0: read from global)
BF16_EDGE_CASES = [
    # small-batch bf16 kernels, B <= 512
    (100, 28, 64, True, False, 0),       # kq = 128, S = 100 > 96: every layer-0 weight read from global
    (96, 32, 40, False, False, 0),       # kq = 128; S = 96 does not fit LDS next to A = 32's head tile; two head tiles
    (2, 1, 256, True, False, 3),         # smallest dims
    (17, 6, 1, True, False, 23),         # one row
    (17, 6, 257, True, False, 23),       # one row past a 256-row chunk
    (40, 17, 256, True, False, 57),      # A = 17: 15 padded action dims; kq = 57 staged through registers
    (3, 9, 33, True, False, 12),         # 9 action dims; one row past a row tile
    (17, 6, 512, True, False, 23),       # the largest batch of the small-batch path
    (72, 28, 256, True, False, 72),      # kq = 100 > 96, S = 72: V and pi staged by LDS-DMA, the critics from global
    (127, 1, 300, True, False, 0),       # the widest packed row (65 float4: the forward's ninth row-tile register); A = 1
    # small-batch bf16 kernels above 512 rows: S + A + 1 > 80 rules the large-batch kernels out
    (100, 28, 1024, True, False, 0),     # S + A + 1 = 129; W0 from global
    (52, 28, 1024, True, False, 80),     # S + A + 1 = 81, one past the large-batch limit; kq = 80 staged by LDS-DMA
    (72, 28, 1024, True, False, 72),     # S + A + 1 = 101; split staging inside the LDS-DMA kernel
    (127, 1, 1024, True, False, 0),      # S + A + 1 = 129; the widest packed row over 32 row tiles
    # large-batch kernels (iqlhip_lb_kernels.h)
    (17, 6, 513, True, True, 23),        # one row past the switch: 17 row tiles, the last holds one row
    (26, 6, 1024, True, True, 32),       # kq = 32: the widest iql_fwd_lb_kernel<NKB = 1>
    (27, 6, 1024, True, True, 33),       # kq = 33: the narrowest iql_fwd_lb_kernel<NKB = 2>
    (51, 28, 1024, False, True, 79),     # kq = 79, S + A + 1 = 80 (the limit): iql_fwd_lb_kernel<NKB = 3>
    (47, 32, 2080, True, True, 79),      # A = 32; 65 row tiles (policy tiles spread), a half-filled last chunk group
    (40, 17, 600, True, True, 57),       # A = 17; 24-row ragged tail: a partial row tile, 64-row GEMM stage and chunk
    (2, 1, 1024, True, True, 3),         # smallest dims
    (17, 6, 16384, False, True, 23),     # the library's largest batch
]


@pytest.mark.parametrize("S,A,B,gaussian,lb,w0k", BF16_EDGE_CASES)
def test_bf16_edge_shape_against_oracle_and_row_permutations(S, A, B, gaussian, lb, w0k):
    from oracle import iql_oracle as O
    build, _, to_tb, unflat = _hip()
    assert (uses_large_batch_kernels(S, A, B), w0_lds_k(S, A)) == (lb, w0k)
    params, batch, hyper, lrs = _case(S, A, B, gaussian)
    ref = O.iql_losses_and_grads(params, batch, hyper, dtype=np.float64)
    want_l = [ref["value_loss"], ref["q_loss"], ref["actor_loss"]]
    tr = build(params, S, A, gaussian, hyper, lrs, 1000)
    tr.set_precision("bf16")
    tb = to_tb(batch)
    grads, lw = unflat(tr, tr.flat_gradient(tb))
    loss_rtol, grad_rl2 = [LOSS_RTOL] * 3, GRAD_RL2
    if B == 1:
        # One row, nothing averages bf16 rounding out.  The value loss is 0.2 * adv^2 with adv = tq - v = -1.8e-2, the
        # difference of two heads that are each cancelling sums over 256 bf16-rounded hidden units: an adv error of
        # ~1.3e-4 is 1.4 % of the loss (observed 1.38e-2).  5 of the value net's 133 active layer-1 units sit within
        # bf16 rounding of the ReLU threshold, and each flip removes a whole row of vf.w1's gradient (observed relative
        # L2 error 0.107).  The same step in fp32 holds test_edge_shapes_match_oracle's bounds: rounding, not a wrong row.
        loss_rtol[0], grad_rl2 = 2e-2, 0.15
        f32 = build(params, S, A, gaussian, hyper, lrs, 1000)
        g32, lw32 = unflat(f32, f32.flat_gradient(tb))
        for got, want in zip(lw32, want_l):
            assert abs(got - want) <= 1e-5 * abs(want), (lw32, want_l)
        for n, ts in ref["grads"].items():
            for k, want in ts.items():
                gmax = float(np.max(np.abs(want)))
                assert np.max(np.abs(g32[n][k].reshape(want.shape) - want)) <= 2e-5 * gmax, (n, k)
    for got, want, rt in zip(lw, want_l, loss_rtol):
        assert abs(got - want) <= rt * abs(want), (lw, want_l)
    worst = _check_grads(grads, ref["grads"], grad_rl2)
    assert worst > 1e-5          # the bf16 path really ran (fp32 would sit at ~1e-7)
    worst_l = max(abs(g - w) / abs(w) for g, w in zip(lw, want_l))
    what = f"bf16 S={S} A={A} B={B} ({'large' if lb else 'small'}-batch kernels)"
    margin, seen, coarse = _check_row_permutations(tr, params, batch, hyper, grads, what)
    print(f"{what}: worst relative-L2 gradient error vs oracle {worst:.3e}, worst loss error {worst_l:.3e}; "
          f"row permutations: margin {margin:.3e}, worst difference / tolerance {seen:.3f}, "
          f"bounded by half the contribution: {coarse}")
    log = tr.train(tb)
    for got, want, rt in zip([log["value_loss"], log["q_loss"], log["actor_loss"]], want_l, loss_rtol):
        assert abs(got - want) <= rt * abs(want)


@pytest.mark.parametrize("S,A,B,gaussian,precision", [
    # tests/test_hip_lb.py's large-batch shapes
    (39, 28, 1024, True, "bf16"),
    (39, 28, 8192, True, "bf16"),
    (39, 28, 600, True, "bf16"),
    (39, 28, 1000, True, "bf16"),
    (17, 6, 1024, False, "bf16"),
    (29, 8, 2080, True, "bf16"),
    # fp32 at the library's largest batch, where test_edge_shapes_match_oracle drops its relative bound
    (17, 6, 16384, False, "f32"),
])
def test_gradient_is_invariant_to_row_order(S, A, B, gaussian, precision):
    build, _, to_tb, unflat = _hip()
    params, batch, hyper, lrs = _case(S, A, B, gaussian)
    tr = build(params, S, A, gaussian, hyper, lrs, 1000)
    if precision == "bf16":
        tr.set_precision("bf16")
    grads, _ = unflat(tr, tr.flat_gradient(to_tb(batch)))
    what = f"{precision} S={S} A={A} B={B}"
    margin, seen, coarse = _check_row_permutations(tr, params, batch, hyper, grads, what)
    print(f"{what}: row permutations: margin {margin:.3e}, worst difference / tolerance {seen:.3f}, "
          f"bounded by half the contribution: {coarse}")


@pytest.mark.parametrize("S,A,big,small", [
    (17, 6, 512, 300),       # small-batch bf16 kernels -> small-batch
    (39, 28, 1024, 600),     # large-batch -> large-batch, ragged
    (39, 28, 1024, 300),     # large-batch -> small-batch
])
def test_bf16_step_ignores_rows_of_an_earlier_larger_batch(S, A, big, small):
    """The rows >= B of the staging buffer and of every scratch array hold an earlier, larger batch's values: the step
    over the first B rows is bit for bit the step of a trainer that never saw them (same context size)."""
    build, read_params, to_tb, _ = _hip()
    params, bb, hyper, lrs = _case(S, A, big, True)
    sb = rows_of(bb, np.arange(small))
    outs = []
    for warm in (False, True):
        tr = build(params, S, A, True, hyper, lrs, 1000)
        tr.set_precision("bf16")
        tr._prepare(big)
        if warm:
            tr.flat_gradient(to_tb(bb))
        flat = tr.flat_gradient(to_tb(sb))
        log = tr.train(to_tb(sb))
        outs.append((flat, log, read_params(tr)))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert outs[0][1] == outs[1][1]
    for n in outs[0][2]:
        for k in outs[0][2][n]:
            assert np.array_equal(outs[0][2][n][k], outs[1][2][n][k]), (n, k)
