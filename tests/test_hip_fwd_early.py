"""The one-slice fp32 forward with preloaded arguments and the early W1 stream (iql_fwd_kernel_early, csrc/iqlhip_kernels.h)
against the project's own unchanged code.

The plain training forward of a step of up to 256 rows with state_dim + action_dim <= 32 is launched as
iql_fwd_kernel_early: the same loads, k-maps and summation orders as iql_fwd_kernel in another issue order.  The oracle
is the code this change leaves instruction for instruction as it was: the multi-slice layouts of the forward
(IQLHIP_FWD_SPB_L2 forced to 1 and 2), which are required to be bit-identical to the one-slice layout
(test_hip_parity.py::test_slices_per_block_layouts_are_bit_identical), and the old one-slice kernel itself
(IQLHIP_FWD_EARLY=0).  Per layout: the flat gradient of the batch (every slab word the update kernel reads, summed in its
fixed order), one eager step and a 3-step train_steps call; losses, gradient, and the parameter, target and moment arenas
must agree bit for bit.

Shapes: rows 1, 31, 32, 33, 256 (clamped row loads, partial and full tiles, one and several row tiles); (S, A) with the
layer-0 widths below, at and across multiples of 4 for all four nets, all with S + A <= 32 (the changed path); Gaussian and
deterministic policy; actor dropout off and on (the prologue's keep-bit loads).  One more pair of dims lies just past the
kernel's limit (S + A = 37): the host must keep the old kernel there.  The library counts the forwards it launches as
iql_fwd_kernel_early (iqlhip_debug_fwd_early_launches), so each case also shows which kernel it compared."""
import functools

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu

HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
N_BUF = 600
# (label, IQLHIP_FWD_SPB_L2, IQLHIP_FWD_EARLY): the first is the code under test, the others the unchanged kernels
LAYOUTS = (("early", None, None), ("one-slice", "0", "0"), ("two-slice", "1", None), ("four-slice", "2", None))


def _hip():
    import hip_helpers as H
    import iql
    return iql, H


def _early_launches(tr):
    """Training forwards the trainer's context has launched or captured as iql_fwd_kernel_early."""
    import iqlhip_binding as hb
    return int(hb.lib().iqlhip_debug_fwd_early_launches(tr._ctx))


@functools.lru_cache(maxsize=None)
def _params(S, A):
    return synth.synth_params(S, A, seed=31)


@functools.lru_cache(maxsize=None)
def _transitions(S, A):
    return synth.synth_transitions(N_BUF, S, A, seed=32)


def _run_layout(S, A, B, gaussian, dropout, spb, early, monkeypatch):
    iql, H = _hip()
    for var, val in (("IQLHIP_FWD_SPB_L2", spb), ("IQLHIP_FWD_EARLY", early)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)          # read when the library context is created (first use)
    tr = H.build_hip_trainer(_params(S, A), S, A, gaussian, dict(HYPER), dict(LRS), 1000, dropout=dropout)
    if dropout:
        tr.set_dropout_seed(11)
    d = _transitions(S, A)
    batch = {"s": d["observations"][:B], "a": d["actions"][:B], "r": d["rewards"][:B], "ns": d["next_observations"][:B],
             "d": d["terminals"][:B]}
    buf = iql.ReplayBuffer(S, A, N_BUF, "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in d.items()})
    out = {"grad": tr.flat_gradient(H.to_torch_batch(batch))}
    log = tr.train(H.to_torch_batch(batch))
    out["eager_losses"] = np.array([log["value_loss"], log["q_loss"], log["actor_loss"]], dtype=np.float64)
    out["eager_arenas"] = H.arenas(tr)
    out["graph_losses"] = np.asarray(tr.train_steps(buf, 3, B, seed=5))
    torch.cuda.synchronize()
    out["graph_arenas"] = H.arenas(tr)
    out["early_launches"] = _early_launches(tr)
    return out


@pytest.mark.parametrize("dropout", [0.0, 0.1])
@pytest.mark.parametrize("gaussian", [True, False])
@pytest.mark.parametrize("B", [1, 31, 32, 33, 256])
# (29, 8): S + A = 37, one step past the kernel's limit of 32 — the step must take the old kernel (and give its bits)
@pytest.mark.parametrize("S,A", [(1, 1), (3, 1), (17, 6), (24, 8), (29, 8)])
def test_early_forward_is_bit_identical_to_the_unchanged_layouts(S, A, B, gaussian, dropout, monkeypatch):
    outs = {label: _run_layout(S, A, B, gaussian, dropout, spb, early, monkeypatch) for label, spb, early in LAYOUTS}
    new = outs.pop("early")
    # the code under test did run: the gradient pass, the eager step and the train_steps call (steps launched directly or
    # captured into a chunk graph) took iql_fwd_kernel_early where the dims allow it, and no forward of any other layout did
    if S + A <= 32:
        assert new["early_launches"] >= 3, new["early_launches"]
    else:
        assert new["early_launches"] == 0, new["early_launches"]
    assert all(ref["early_launches"] == 0 for ref in outs.values()), {k: v["early_launches"] for k, v in outs.items()}
    assert np.all(np.isfinite(new["graph_arenas"])) and np.all(np.isfinite(new["grad"]))
    for label, ref in outs.items():
        for key in ("eager_losses", "graph_losses", "grad", "eager_arenas", "graph_arenas"):
            assert new[key].shape == ref[key].shape, (label, key)
            assert np.array_equal(new[key].view(np.uint8), ref[key].view(np.uint8)), (label, key)
