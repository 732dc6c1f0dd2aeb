"""CPU test of the value-edge inputs themselves (tests/value_edges.py), from the float64 oracle alone: for every case of
the GPU matrix (tests/test_hip_value_edges.py) the branches the inputs are for really fire (a), the result is finite
(b), every wrong reference of value_edges.mutants is told from the right one by an assertion the GPU test makes on that
case (c), and the fp32 bounds that test uses stand four times above fp32 arithmetic's own error (d).

(c) is a condition, not a measurement: a tolerance-based assertion counts for a mutant only when the mutant moves the
asserted quantity by at least SENSITIVITY times its tolerance; a mutant the tolerances of a path cannot see — at bf16
bounds a quarter of the rows' terminal flags move the critics' gradients by less than the bound — must break one of
the exact relations the GPU test holds on that path, which is checked here on the mutant itself."""
import functools

import numpy as np
import pytest

import value_edges as ve
from helpers import bwd_instantiation, uses_large_batch_kernels, w0_lds_k
from oracle import iql_oracle as O

SENSITIVITY = 10.0
NOISE_MARGIN = 4.0


@functools.lru_cache(maxsize=None)
def _case(name):
    params, batch, hyper = ve.case_inputs(name)
    return params, batch, hyper, O.iql_losses_and_grads(params, batch, hyper, dtype=np.float64)


def _flat(res, nets=("vf", "q1", "q2", "pi")):
    return np.concatenate([np.ravel(res["grads"][n][k]) for n in nets for k in sorted(res["grads"][n])]
                          + [np.array([res[k] for k in ve.LOSS_NAMES], dtype=np.float64)])


@pytest.mark.parametrize("name", ve.CASE_NAMES)
def test_case_paths_are_the_stated_ones(name):
    _, S, A, B, gaussian, precision, lb, w0k, bwd = ve.CASE[name]
    assert (precision == "bf16" and uses_large_batch_kernels(S, A, B), w0_lds_k(S, A)) == (lb, w0k)
    assert bwd_instantiation(S, A, B, precision) == bwd
    if name.endswith("_multi"):       # the smallest batch of the multi-round backward
        assert "MULTI=0" in bwd_instantiation(S, A, B - 1, precision) and "MULTI=1" in bwd


# ------------------------------------------------------------------------------------------------- (a) and (b)
@pytest.mark.parametrize("name", ve.CASE_NAMES)
def test_inputs_reach_every_branch_and_stay_finite(name):
    case = ve.CASE[name]
    S, A, B, gaussian = case.S, case.A, case.B, case.gaussian
    params, batch, hyper, ref = _case(name)
    clamped = hyper["beta"] * ref["adv"] >= np.log(O.EXP_ADV_MAX)
    assert 0.05 <= clamped.mean() <= 0.95, clamped.mean()
    assert np.array_equal(clamped, ref["exp_adv"] == O.EXP_ADV_MAX)
    assert (ref["adv"] < 0).any() and (ref["adv"] > 0).any()
    pre = ve.pre_activations(params, batch)
    hi, lo = ve.overflow_dims(A)
    assert hi != lo and np.all(pre[:, hi] == 60.0) and np.all(pre[:, lo] == -60.0)
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(np.float32(2.0) * pre[:, hi].astype(np.float32))).all()
    assert (np.exp(np.float32(2.0) * pre[:, lo].astype(np.float32)) == 0.0).all()
    others = np.delete(np.abs(pre), [hi, lo], axis=1)
    assert (others >= ve.PRE_SATURATED).mean() >= 0.05 and (others < 2.0).mean() >= 0.05, (others >= 12).mean()
    assert 0.24 <= batch["d"].mean() <= 0.26
    assert (batch["a"] == 1.0).any() and (batch["a"] == -1.0).any() and np.abs(batch["r"]).max() > 20.0
    assert np.array_equal(batch["s"][B // 2: B // 2 + 16], batch["s"][:16])
    if gaussian:
        ls = params["pi"]["log_std"]
        classes = ve.log_std_classes(ls)
        assert len(classes["below"]) == 1
        for cls, dims in classes.items():
            assert len(dims) > 0, cls
            assert A <= 16 or dims.max() >= 16, (cls, dims)
            assert A <= 8 or dims.max() >= 8, (cls, dims)
        assert set(classes["below"]).isdisjoint({hi, lo}) and set(classes["at_min"]).isdisjoint({hi, lo})
    assert np.all(np.isfinite(_flat(ref)))
    for k in ("next_v", "adv", "mu", "exp_adv"):
        assert np.all(np.isfinite(ref[k])), k
    print(f"{name}: clamped rows {clamped.mean():.3f}, adv < 0 {np.mean(ref['adv'] < 0):.3f}, "
          f"|pre| >= 12 {(others >= 12).mean():.3f}, losses {[float(ref[k]) for k in ve.LOSS_NAMES]}")


# ---------------------------------------------------------------------------------------------------------- (c)
def _relations(name, step, c=None):
    """{exact relation of the GPU test: True when `step` (a function (params, batch, hyper) -> float64 result) keeps it}."""
    gaussian = ve.CASE[name].gaussian
    params, batch, hyper, _ = _case(name)
    out = {}
    base = step(params, batch, hyper)
    if gaussian:
        inside = ve.inside_dims(params["pi"]["log_std"])
        g = base["grads"]["pi"]["log_std"]
        out["log_std gradient == 0 outside the clamp"] = bool(np.all(g[~inside] == 0.0))
        out["log_std gradient != 0 inside the clamp"] = bool(np.all(g[inside] != 0.0))
    out["terminal rows ignore their next state"] = bool(
        np.array_equal(_flat(base), _flat(step(params, ve.with_other_next_states(batch), hyper))))
    if c is None:
        a, b = (step(*ve.case_inputs(name, target_shift=s)) for s in ve.ALL_CLAMPED_SHIFTS)
        out["all rows clamped: policy independent of the target shift"] = bool(
            np.array_equal(_flat(a, ("pi",))[:-3], _flat(b, ("pi",))[:-3]) and a["actor_loss"] == b["actor_loss"])
        assert not np.array_equal(_flat(a, ("vf",)), _flat(b, ("vf",)))
    return out


def _cells(name, c=None):
    """{mutant: [the GPU test's assertions on this case that tell it from the oracle]}."""
    params, batch, hyper, ref = _case(name)
    precision = ve.CASE[name].precision
    if c is not None:
        ref, precision = ve.mutant_free(params, batch, hyper, c), "f32rw"
    truth = _relations(name, lambda p, b, h: ve.mutant_free(p, b, h, c), c)
    assert all(truth.values()), (name, truth)          # the right reference keeps every exact relation
    cells, margins = {}, {}
    for mname in ve.MUTANTS:
        if not ve.mutant_applies(mname, hyper):
            continue
        m = ve.mutant(mname, params, batch, hyper, c)
        moved = ve.oracle_check_errors([m[k] for k in ve.LOSS_NAMES], m["grads"], ref, precision)
        seen = sorted(((r, k) for k, r in moved.items() if r >= SENSITIVITY), reverse=True)
        margins[mname] = max(moved.values())
        cell = [f"oracle check: {k} moves by {r:.3g} x its tolerance" for r, k in seen[:2]]
        broken = _relations(name, lambda p, b, h: ve.mutant(mname, p, b, h, c), c)
        cell += [f"exact: {rel}" for rel, kept in broken.items() if not kept]
        cells[mname] = cell
    return cells, margins


PATHS = [(n, False) for n in ve.CASE_NAMES] + [(n, True) for n in ve.FP32_CASE_NAMES]


@pytest.mark.parametrize("name,weighted", PATHS)
def test_every_mutant_is_caught_on_every_path(name, weighted):
    B = ve.CASE[name].B
    cells, margins = _cells(name, ve.row_weights(B) if weighted else None)
    what = name + (" (row-weighted backward)" if weighted else "")
    for mname, cell in cells.items():
        print(f"{what} | {mname} | largest movement / tolerance {margins[mname]:.3g} | " + "; ".join(cell))
    empty = [m for m, cell in cells.items() if not cell]
    assert not empty, (what, empty)
    if ve.CASE[name].precision == "f32":     # fp32 bounds see every mutant by themselves
        assert all(any(x.startswith("oracle check") for x in cell) for cell in cells.values()), (what, cells)


# ---------------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("name", ve.FP32_CASE_NAMES)
def test_fp32_bounds_stand_above_the_fp32_noise_floor(name):
    """The fp32 oracle against the float64 oracle, in units of the GPU test's fp32 tolerances: fp32 arithmetic in
    numpy's order — one valid fp32 evaluation, like the kernels' — stays NOISE_MARGIN times inside them, also for the
    row-weighted step and its TD errors (2e-5 of the largest, tests/test_hip_loss_weights.py)."""
    from loss_weights_ref import weighted_losses_and_grads
    params, batch, hyper, ref = _case(name)
    f32 = O.iql_losses_and_grads(params, batch, hyper, dtype=np.float32)
    errs = ve.oracle_check_errors([f32[k] for k in ve.LOSS_NAMES], f32["grads"], ref, "f32")
    c = ve.row_weights(ve.CASE[name].B)
    w64 = weighted_losses_and_grads(params, batch, hyper, c, dtype=np.float64)
    w32 = weighted_losses_and_grads(params, batch, hyper, c, dtype=np.float32)
    werrs = ve.oracle_check_errors([w32[k] for k in ve.LOSS_NAMES], w32["grads"], w64, "f32rw")
    td = float(np.max(np.abs(w32["td"] - w64["td"])) / np.max(np.abs(w64["td"]))) / ve.TD_RTOL
    worst = max(errs.items(), key=lambda kv: kv[1])
    wworst = max(werrs.items(), key=lambda kv: kv[1])
    print(f"{name}: fp32 oracle vs float64 oracle, error / tolerance: plain {worst[1]:.3g} ({worst[0]}), "
          f"row-weighted {wworst[1]:.3g} ({wworst[0]}), TD errors {td:.3g}")
    assert NOISE_MARGIN * worst[1] <= 1.0, worst
    assert NOISE_MARGIN * wworst[1] <= 1.0, wworst
    assert NOISE_MARGIN * td <= 1.0, td
