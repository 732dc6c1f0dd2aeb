"""GPU tests of the IQL step at trained-like values (tests/value_edges.py) on every kernel path: clamped and unclamped
advantage weights in one batch, log_std above, below and exactly on its clamp, saturated and overflowing tanh, a quarter
of the rows terminal — fp32 (one-slice and multi-round backward, the row-weighted backward), the small-batch bf16
kernels and the large-batch bf16 kernels (NKB = 1 / 2 / 3, column split, SPREAD).

Two kinds of checks.  The oracle check holds losses and every gradient tensor to the float64 oracle at the project's
existing bounds (value_edges.oracle_check_errors: fp32 as test_edge_shapes_match_oracle, bf16 as tests/test_hip_lb.py).
The exact relations hold at any precision — which is what the bf16 paths need: tests/test_value_edges_cpu.py shows,
mutant by mutant, which of the two catches a step that got one branch wrong.  Margins: profiles/value_edges_margins.txt."""
import numpy as np
import pytest
import torch

import value_edges as ve
from helpers import bwd_instantiation, rel_err, uses_large_batch_kernels, w0_lds_k

pytestmark = pytest.mark.gpu


def _hip():
    from hip_helpers import build_hip_trainer, read_params, to_torch_batch, unflatten_grads
    return build_hip_trainer, read_params, to_torch_batch, unflatten_grads


def _trainer(name, params):
    build = _hip()[0]
    c = ve.CASE[name]
    S, A, B, gaussian, precision = c.S, c.A, c.B, c.gaussian, c.precision
    hyper = dict(ve.HYPER, deterministic=not gaussian)
    tr = build(params, S, A, gaussian, hyper, ve.LRS, 1000)
    if precision == "bf16":
        tr.set_precision("bf16")
    return tr


def _step_words(tr, flat):
    """The gradient and the three loss words of a flat gradient (the fourth tail word is a spare)."""
    return flat[: tr._layout.n_params + 3]


def _report(what, errs):
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:3]
    print(f"{what}: error / tolerance, worst three: " + ", ".join(f"{k} {v:.3g}" for k, v in worst))
    bad = {k: v for k, v in errs.items() if not v <= 1.0}
    assert not bad, (what, bad)


@pytest.mark.parametrize("name", ve.CASE_NAMES)
def test_step_at_trained_like_values(name):
    from oracle import iql_oracle as O
    _, read_params, to_tb, unflat = _hip()
    _, S, A, B, gaussian, precision, lb, w0k, bwd = ve.CASE[name]
    assert (precision == "bf16" and uses_large_batch_kernels(S, A, B), w0_lds_k(S, A)) == (lb, w0k)
    assert bwd_instantiation(S, A, B, precision) == bwd
    params, batch, hyper = ve.case_inputs(name)
    ref = O.iql_losses_and_grads(params, batch, hyper, dtype=np.float64)
    tr = _trainer(name, params)
    L = tr._layout
    tb = to_tb(batch)
    flat = tr.flat_gradient(tb).copy()
    assert np.all(np.isfinite(flat))
    grads, lw = unflat(tr, flat)

    # the oracle check, at the existing bounds
    _report(f"{name} [{bwd}] gradient", ve.oracle_check_errors(lw, grads, ref, precision))
    # ... and the precision asked for really ran: bf16 operands leave >= 1e-5 in relative L2 (tests/test_hip_lb.py),
    # the fp32 kernels sit at ~1e-7
    rl2 = max(float(np.linalg.norm(grads[n][t].reshape(w.shape) - w) / np.linalg.norm(w))
              for n, ts in ref["grads"].items() for t, w in ts.items() if w.size > 32)
    assert (rl2 > 1e-5) == (precision == "bf16"), (precision, rl2)

    # log_std: exactly no gradient outside the clamp, some at every dim inside it — 2.0 and -20.0 are inside
    if gaussian:
        inside = ve.inside_dims(params["pi"]["log_std"])
        g = grads["pi"]["log_std"]
        assert np.all(g[~inside] == 0.0), (g, inside)
        assert np.all(g[inside] != 0.0), (g, inside)
    else:
        # (a deterministic policy has no log_std in the arena: there is no content to vary)
        assert L.net[3].log_std == -1 and "log_std" not in grads["pi"]

    # terminal rows: (1 - d) = 0 multiplies V(s'), so their next states are never seen
    other = tr.flat_gradient(to_tb(ve.with_other_next_states(batch)))
    assert np.array_equal(_step_words(tr, other), _step_words(tr, flat))

    # every row on the clamp: the policy's gradient and loss no longer depend on how far above it the advantages lie
    segs = []
    for shift in ve.ALL_CLAMPED_SHIFTS:
        p2, b2, _ = ve.case_inputs(name, target_shift=shift)
        f2 = _trainer(name, p2).flat_gradient(to_tb(b2)).copy()
        assert np.all(np.isfinite(f2))
        segs.append(f2)
    pi0, pi1, v0, v1 = int(L.net[3].seg_begin), int(L.net[3].seg_end), int(L.net[0].seg_begin), int(L.net[0].seg_end)
    assert np.array_equal(segs[0][pi0:pi1], segs[1][pi0:pi1]) and np.any(segs[0][pi0:pi1] != 0.0)
    assert segs[0][L.n_params + 2] == segs[1][L.n_params + 2]
    assert not np.array_equal(segs[0][v0:v1], segs[1][v0:v1]) and segs[0][L.n_params] != segs[1][L.n_params]

    # one train() from these parameters: the same losses, and every tensor moves — except the log_std dims outside the
    # clamp, which stay put.  (That rests on the fresh trainer's zero moments: g = 0 with m = v = 0 gives an update of
    # 0 / (0 + eps) = 0.  With a nonzero first moment Adam keeps moving such a dim by its momentum, here as in torch;
    # tests/test_hip_adam_state.py covers the update from nonzero moments.)
    log = tr.train(tb)
    got_l = [log["value_loss"], log["q_loss"], log["actor_loss"]]
    errs = ve.oracle_check_errors(got_l, None, ref, precision)
    assert all(v <= 1.0 for v in errs.values()), errs
    after = read_params(tr)
    for net in ("vf", "q1", "q2", "pi"):
        for t, before in params[net].items():
            now = after[net][t].reshape(before.shape)
            assert np.all(np.isfinite(now)), (net, t)
            if t == "log_std":
                assert np.array_equal(now[~inside], before[~inside]) and np.all(now[inside] != before[inside]), now
            else:
                assert np.any(now != before), (net, t)
    for net, src in (("qt1", "q1"), ("qt2", "q2")):
        for t, before in params[net].items():
            assert np.any(after[net][t].reshape(before.shape) != before), (net, t)


@pytest.mark.parametrize("name", ve.FP32_CASE_NAMES)
def test_row_weighted_step_at_trained_like_values(name):
    """The row-weighted backward (fp32 only: bf16 and the large-batch path refuse it) with weights in {0, 0.25, 1, 1000}
    against tests/loss_weights_ref.py in float64 at tests/test_hip_loss_weights.py's bounds."""
    from loss_weights_ref import weighted_losses_and_grads
    _, _, to_tb, unflat = _hip()
    c = ve.CASE[name]
    S, A, B, gaussian, precision = c.S, c.A, c.B, c.gaussian, c.precision
    params, batch, hyper = ve.case_inputs(name)
    c = ve.row_weights(B)
    ref = weighted_losses_and_grads(params, batch, hyper, c, dtype=np.float64)
    tr = _trainer(name, params)
    tb, ct = to_tb(batch), torch.from_numpy(c).cuda()
    flat = tr.flat_gradient(tb, loss_weights=ct).copy()
    assert np.all(np.isfinite(flat))
    grads, lw = unflat(tr, flat)
    what = f"{name} [{bwd_instantiation(S, A, B, precision, row_weighted=True)}]"
    _report(what + " gradient", ve.oracle_check_errors(lw, grads, ref, "f32rw"))
    if gaussian:
        inside = ve.inside_dims(params["pi"]["log_std"])
        assert np.all(grads["pi"]["log_std"][~inside] == 0.0) and np.all(grads["pi"]["log_std"][inside] != 0.0)
    # a zero-weight row contributes exactly nothing, whatever it holds
    other = tr.flat_gradient(to_tb(ve.with_other_zero_weight_rows(batch, c)), loss_weights=ct)
    assert np.array_equal(_step_words(tr, other), _step_words(tr, flat))
    # ... and neither does a terminal row's next state
    other = tr.flat_gradient(to_tb(ve.with_other_next_states(batch)), loss_weights=ct)
    assert np.array_equal(_step_words(tr, other), _step_words(tr, flat))
    log = tr.train(tb, loss_weights=ct, return_td=True)
    errs = ve.oracle_check_errors([log["value_loss"], log["q_loss"], log["actor_loss"]], None, ref, "f32rw")
    assert all(v <= 1.0 for v in errs.values()), errs
    td = rel_err(tr.last_td_errors().cpu().numpy(), ref["td"])
    print(f"{what} TD errors: {td:.3g} of the largest (bound {ve.TD_RTOL:g})")
    assert td <= ve.TD_RTOL, td
