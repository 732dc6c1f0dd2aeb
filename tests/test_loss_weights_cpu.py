"""Per-row loss weights, CPU side: the numpy restatement (tests/loss_weights_ref.py) against the reference fixtures
g20_loss_weights_* at the bounds tests/test_oracle_golden.py uses for the unweighted ones, and the host argument checks."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import ROOT, check_step_against_golden, load_golden, rel_err, single_step_inputs
from loss_weights_ref import GOLDENS, weighted_losses_and_grads, weighted_step
from oracle import iql_oracle as O


@pytest.mark.parametrize("name", GOLDENS)
def test_numpy_restatement_matches_weighted_reference(name):
    z, meta = load_golden(name)
    params, batch, hyper = single_step_inputs(meta)
    c = z["weights"]
    assert c.dtype == np.float32 and c.shape == (meta["B"],) and c.min() >= 0.05 and c.max() <= 1.0
    newp, newo, info = weighted_step(params, O.new_opt_state(params), batch, hyper, meta["lrs"], c)
    check_step_against_golden(z, meta, info, newp, newo, grad_rtol=3e-5, param_atol=2e-6, loss_rtol=1e-5,
                              target_atol=1e-7, moment_rtol=5e-5)
    assert rel_err(info["td"], z["inter.td"]) <= 2e-5


def test_ones_weights_reduce_to_the_unweighted_oracle():
    z, meta = load_golden(GOLDENS[0])
    params, batch, hyper = single_step_inputs(meta)
    a = O.iql_losses_and_grads(params, batch, hyper)
    b = weighted_losses_and_grads(params, batch, hyper, np.ones(meta["B"], dtype=np.float32))
    for k in ("value_loss", "q_loss", "actor_loss"):
        assert a[k] == b[k], k
    for net in a["grads"]:
        for t in a["grads"][net]:
            assert np.array_equal(a["grads"][net][t], b["grads"][net][t]), (net, t)


def test_check_loss_weights_shape_dtype_device():
    from iqlhip_trainer import check_loss_weights
    B = 7
    ok = torch.rand(B)
    assert check_loss_weights(ok, B, "cpu").shape == (B,)
    assert check_loss_weights(ok.reshape(B, 1), B, "cpu").shape == (B,)
    assert check_loss_weights(torch.rand(2 * B)[::2], B, "cpu").is_contiguous()
    with pytest.raises(TypeError):
        check_loss_weights(np.ones(B, dtype=np.float32), B, "cpu")
    with pytest.raises(TypeError):
        check_loss_weights(ok.double(), B, "cpu")
    for bad in (torch.rand(B + 1), torch.rand(1, B), torch.rand(B, 2), torch.rand(())):
        with pytest.raises(ValueError):
            check_loss_weights(bad, B, "cpu")
    with pytest.raises(ValueError):
        check_loss_weights(torch.empty(B, device="meta"), B, "cpu")


def test_is_draw_arguments_are_checked_on_the_host():
    from iqlhip_weighted import check_is_args
    assert check_is_args(192, 0.4, 64) == (0.4, 64)
    assert check_is_args(10, 0, None) == (0.0, 10)
    for beta in (-0.1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError):
            check_is_args(10, beta, None)
    for bs in (0, -1, 11):
        with pytest.raises(ValueError):
            check_is_args(10, 0.5, bs)


def test_unsupported_combinations_raise_before_any_device_work():
    """bf16 and data parallelism refuse loss_weights / return_td in the Python layer (no context is needed for that)."""
    from iqlhip_trainer import ImplicitQLearning
    for attrs in ({"_precision": "bf16", "_dp_world": 1, "_dp_exchange": None},
                  {"_precision": "f32", "_dp_world": 2, "_dp_exchange": None},
                  {"_precision": "f32", "_dp_world": 1, "_dp_exchange": "rccl"}):
        tr = object.__new__(ImplicitQLearning)
        tr.__dict__.update(attrs)
        tr.__dict__["_ctx"] = None          # (nothing for __del__ to release)
        with pytest.raises(NotImplementedError, match="loss weights"):
            tr._loss_weight_args(8, torch.ones(8), False)
        with pytest.raises(NotImplementedError, match="loss weights"):
            tr._loss_weight_args(8, None, True)


def test_new_symbols_are_declared_in_the_header_and_bound():
    text = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    import iqlhip_binding as hb
    bound = {entry[0] for entry in hb.SYMBOLS}
    for sym in ("iqlhip_step_rw", "iqlhip_forward_backward_rw", "iqlhip_draw_indices_weighted_is",
                "iqlhip_train_steps_weighted_is", "iqlhip_train_steps_weighted_is_prepare"):
        assert re.search(r"\bint\s+" + sym + r"\s*\(", text), f"{sym} is not declared in include/iqlhip.h"
        assert sym in bound, f"{sym} is not bound"
