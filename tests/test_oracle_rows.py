"""The premise of the GPU row-permutation checks (tests/helpers.py: permutation_bounds; tests/test_hip_bf16_edges.py):
the step's gradient is a sum of per-row terms.  Pinned here on the oracle, which tests/test_oracle_golden.py pins to the
reference: the gradients of any split of a batch into row groups, each taken with the whole batch's divisor, add up to
the whole batch's gradient; and the per-row magnitude sums the permutation tolerance is built from are exactly the sums
of the rows' own gradients' magnitudes."""
import numpy as np
import pytest

import synth
from helpers import row_abs_grad_sums, rows_of, smallest_row_groups, step_batch


def _case(S, A, B, gaussian):
    params = synth.synth_params(S, A, seed=11 * S + A, gaussian=gaussian)
    batch = step_batch(S, A, B, seed=B + S)
    hyper = {"iql_tau": 0.8, "beta": 3.0, "discount": 0.99, "tau": 0.005, "deterministic": not gaussian}
    return params, batch, hyper


@pytest.mark.parametrize("S,A,B,gaussian", [(17, 6, 100, True), (39, 28, 600, True), (3, 9, 33, False),
                                            (29, 8, 257, False)])
def test_oracle_gradient_is_the_sum_of_its_row_groups(S, A, B, gaussian):
    from oracle import iql_oracle as O
    params, batch, hyper = _case(S, A, B, gaussian)
    whole = O.iql_losses_and_grads(params, batch, hyper, dtype=np.float64)["grads"]
    scale = row_abs_grad_sums(params, batch, hyper)
    rng = np.random.default_rng(B)
    perm = rng.permutation(B)
    cuts = sorted({0, B, *[int(c) for c in rng.integers(1, B, 6)]})
    total = {n: {t: np.zeros_like(v) for t, v in ts.items()} for n, ts in whole.items()}
    for a, b in zip(cuts[:-1], cuts[1:]):
        g = O.iql_losses_and_grads(params, rows_of(batch, perm[a:b]), hyper, dtype=np.float64, grad_scale_rows=B)
        for n, ts in g["grads"].items():
            for t, v in ts.items():
                total[n][t] += v
    for n, ts in whole.items():
        for t, want in ts.items():
            s = float(np.max(scale[n][t]))
            err = float(np.max(np.abs(total[n][t] - want)))
            assert err <= 1e-12 * s, (n, t, err, s)
            # the magnitude sums bound the gradient itself (triangle inequality)
            assert np.all(np.abs(want) <= scale[n][t] * (1 + 1e-12)), (n, t)


@pytest.mark.parametrize("B,gaussian", [(33, True), (40, False)])
def test_row_abs_grad_sums_are_sums_of_row_gradient_magnitudes(B, gaussian):
    from oracle import iql_oracle as O
    params, batch, hyper = _case(5, 3, B, gaussian)
    got = row_abs_grad_sums(params, batch, hyper)
    want = None
    for r in range(B):
        g = O.iql_losses_and_grads(params, rows_of(batch, [r]), hyper, dtype=np.float64, grad_scale_rows=B)["grads"]
        if want is None:
            want = {n: {t: np.abs(v) for t, v in ts.items()} for n, ts in g.items()}
        else:
            for n, ts in g.items():
                for t, v in ts.items():
                    want[n][t] += np.abs(v)
    for n, ts in want.items():
        assert set(got[n]) == set(ts), n
        for t, w in ts.items():
            assert np.allclose(got[n][t], w, rtol=1e-12, atol=0.0), (n, t)


def test_smallest_row_groups():
    assert [g.tolist() for g in smallest_row_groups(1)] == [[0]]
    assert [g.tolist() for g in smallest_row_groups(3)] == [[0, 1, 2]]
    assert [g.tolist() for g in smallest_row_groups(64)] == [[63], [0]]
    assert [g.tolist() for g in smallest_row_groups(35)] == [[32, 33, 34], [0, 1, 2]]
