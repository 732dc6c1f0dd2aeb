"""GPU tests of the variance learner's step kernels (csrc/iqlhip_variance_kernels.h; DESIGN.md 6l "Widths, row counts and
trained-like values") at every state-width class, at the row counts where the backward's row loops end, and at
trained-like values: the generated cases of tests/variance_cases.py (checked on the CPU by test_variance_cases_cpu.py)
against the float64 restatement (tests/variance_ref.py).  Bounds per case and quantity: variance_ref.bounds of the float32
restatement's own deviation from float64 — the larger of the project's fp32 bound and four times that deviation, never
anything the device computed.  Next to the bounds, what must hold exactly: zero gradients of the constructed dead and
zero units, the other net untouched, zero padding words.  With IQLHIP_VARIANCE_MARGINS set to a file name, each comparison
appends its margins there (profiles/variance_shapes_margins.txt)."""
import numpy as np
import pytest
import torch

import test_hip_variance as TV
import test_hip_variance_buffer as TB
import variance_cases as VC
import variance_ref as R
import variance_window_ref as W

pytestmark = pytest.mark.gpu

WIDTH_CASES = [f"S{S}_B31_mixed" for S in VC.WIDTHS]
ROW_CASES = [f"S{S}_B{B}_mixed" for S in VC.ROW_WIDTHS for B in VC.ROW_COUNTS if B != 31]
OTHER_CASES = ["S64_B63_mixed_aligned", "S16_B16_mixed_alldone", "S16_B16_mixed_nodone"]


def _padding(L, k):
    """The words of net k's segment that belong to no tensor, as a mask over the segment."""
    lay, net = L._layout[k], (L.mf, L.vf)[k]
    lo, hi = int(lay.seg_begin), int(lay.seg_end)
    used = np.zeros(hi - lo, bool)
    for key, p in zip(R.KEYS, net.parameters()):
        off = int(getattr(lay, key)) - lo
        assert not used[off: off + p.numel()].any()
        used[off: off + p.numel()] = True
    assert not used.all()                    # (b2 is one word and a segment a multiple of 64)
    return ~used


def _padding_is_zero(L, k):
    pad = _padding(L, k)
    return all(not seg[pad].any() for seg in TV._segment_bytes(L, k))


def _device_step(L, c, which):
    """get_values, the flat gradient, then the step on case c: the results in variance_ref.step's form, and the flat
    gradient."""
    batch = TV._batch(c["obs"], c["last"], c["rewards"], c["nd"])
    samp, pred, var = L.get_values(batch[0], batch[2], batch[4], batch[3], batch[5])
    loss_fb, flat = L.flat_gradient(batch, bool(which))
    got = dict(samp=samp.numpy(), pred=pred.numpy(), var=var.numpy(),
               grads={k: v.numpy() for k, v in L.net_gradients(flat, bool(which)).items()})
    log = L._update_v(batch, bool(which))
    assert log["value_loss"] == loss_fb      # the step's forward is the forward_backward's
    got["loss"] = np.float32(log["value_loss"])
    got.update(TV._net_state(L, which))
    return got, flat.numpy()


def _within(name, got, s32, s64):
    bound = R.bounds(R.deviations(s32, s64, full_w1=True))
    dev = R.deviations(got, s64, full_w1=True)
    TV._note(name, dev, bound)
    for k in dev:
        assert dev[k] <= bound[k], (name, k, dev[k], bound[k])
    # the gate: the rows the device clipped are the rows float64 clips
    assert np.array_equal(got["var"] == np.float32(R.CLIP_LO), s64["e"] < R.CLIP_LO)
    assert np.array_equal(got["var"] == np.float32(R.CLIP_HI), s64["e"] > R.CLIP_HI)


def _constructed_gradients_are_zero(g, sets):
    d0 = np.concatenate([sets["dead0"], sets["zero0"]])
    for what, a in (("dW0 rows", g["w0"][d0]), ("db0", g["b0"][d0]), ("dW1 columns", g["w1"][:, d0]),
                    ("dW1 rows", g["w1"][sets["dead1"]]), ("db1 dead", g["b1"][sets["dead1"]]),
                    ("dW2", g["w2"][0, sets["dead1"]]), ("db1 at w2 == 0", g["b1"][sets["w2zero"]])):
        assert a.size and not a.any(), (what, np.abs(a).max())


def _run_case(name, which):
    c = VC.case(name)
    s32, s64, _ = VC.reference(name, which)
    L = TV._learner(c["S"], c["mf"], c["vf"], aligned=c["aligned"])
    other_before = TV._segment_bytes(L, 1 - which)
    assert _padding_is_zero(L, 0) and _padding_is_zero(L, 1)
    got, flat = _device_step(L, c, which)
    _within(f"{name}_net{which}", got, s32, s64)
    _constructed_gradients_are_zero(got["grads"], c["sets"][which])
    assert not flat[_padding(L, which)].any(), "a padding word of the gradient segment is not zero"
    assert _padding_is_zero(L, 0) and _padding_is_zero(L, 1)
    for a, b in zip(other_before, TV._segment_bytes(L, 1 - which)):
        assert np.array_equal(a, b), "the other net's parameters or moments changed"
    return L, got, flat


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", WIDTH_CASES)
def test_state_widths(name, which):
    """Every S % 4 (score_l0's masked k-tail), both sides of its 32-column trip, njt = 1, 2, 4, 5, 8 column tiles of the
    dW0 / db0 part with the bias column alone in a tile (S = 16, 32, 64) and a tile's last lane (S = 15, 31, 63, 127)."""
    _run_case(name, which)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", ROW_CASES)
def test_row_counts(name, which):
    """n = B + 1 (mf) and n = B (vf) over every n % 4, n = 16 and 32 exactly, n = 1024 and 1025, at a width with a
    bias-only tile and at the widest."""
    _run_case(name, which)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", OTHER_CASES)
def test_aligned_rewards_and_done_patterns(name, which):
    _run_case(name, which)


@pytest.mark.parametrize("name", list(VC.CLOSED))
def test_closed_gate_leaves_vf_as_it_is(name):
    """Every row clipped: dy = 0, Adam at g = 0 — vf bit for bit as before, both moments and the gradient zero; the loss
    still meets its bound, and an mf step on the same case meets every bound (the gate does not touch mf)."""
    c = VC.case(name)
    s32, s64, bound = VC.reference(name, 1)
    L = TV._learner(c["S"], c["mf"], c["vf"])
    before = TV._segment_bytes(L, 1)
    other_before = TV._segment_bytes(L, 0)
    got, flat = _device_step(L, c, 1)
    assert not flat.any(), "a gradient word is not zero under a closed gate"
    after = TV._segment_bytes(L, 1)
    assert np.array_equal(before[0], after[0]), "vf's parameters changed under a closed gate"
    assert not after[1].view(np.float32).any() and not after[2].view(np.float32).any(), "a moment is not zero under a closed gate"
    dev = {"loss": R.rel(got["loss"], s64["loss"]), "forward": max(R.rel(got[k], s64[k]) for k in ("samp", "pred", "var"))}
    TV._note(f"{name}_net1", dev, bound)
    assert dev["loss"] <= bound["loss"] and dev["forward"] <= bound["forward"], (dev, bound)
    assert ((got["var"] == np.float32(R.CLIP_LO)) | (got["var"] == np.float32(R.CLIP_HI))).all()      # every row clipped
    for a, b in zip(other_before, TV._segment_bytes(L, 0)):
        assert np.array_equal(a, b)
    assert L._adam_t == [0, 1]
    _run_case(name, 0)


def test_chain_of_steps_carries_the_adam_state():
    """Three mf steps, then three vf steps, each on another clean case at S = 65: against the float64 restatement chained
    with t_adam, m and v; per step the bound rule on the float32 chain's deviation."""
    steps = VC.chain()
    c0 = steps[0][0]
    L = TV._learner(c0["S"], c0["mf"], c0["vf"])
    for k, ((c, s32, s64), which) in enumerate(zip(steps, VC.CHAIN["which"])):
        got, _ = _device_step(L, c, which)
        _within(f"chain_S{c['S']}_B{c['B']}_step{k}_net{which}", got, s32, s64)
    assert L._adam_t == [3, 3] and _padding_is_zero(L, 0) and _padding_is_zero(L, 1)


@pytest.mark.parametrize("uv", [False, True])
def test_update_from_buffer_at_the_widest_row(uv):
    """S + A = 128, the row limit: a window update is _update_v on the downloaded window, bit for bit."""
    S, A, B, start = 127, 1, 33, 5
    rows, buf = TB._make(S, A, 100, seed=17)
    a, b = TB._learner(S, A, B), TB._learner(S, A, B)
    for step in range(2):
        la = a.update_from_buffer(buf, start + step, uv)
        lb = b._update_v(W.window_tensors(buf._rows.cpu().numpy(), start + step, B, S, A), uv)
        assert set(la) == set(lb) and la["value_loss"] == lb["value_loss"] and np.isfinite(la["value_loss"])
        for key in ("values_samp_vec", "values_pred_vec", "variance_pred_vec"):
            assert np.array_equal(TB._bits(la[key]), TB._bits(lb[key])), key
    assert TB._same(TB._state(a), TB._state(b)) and a._adam_t == ([0, 2] if uv else [2, 0])
    assert not torch.equal(a._params_arena, TB._learner(S, A, B)._params_arena)
