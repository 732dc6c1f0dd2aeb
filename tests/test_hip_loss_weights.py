"""Per-row loss weights in the IQL step (trainer.train(batch, loss_weights=c, return_td=...)) and the importance-sampling
weights of a weighted draw (draw_weighted_indices(..., is_beta=...)).

Bounds: the fixtures g20_loss_weights_* (tools/make_loss_weight_goldens.py: the reference's modules and optimisers on the
weighted-mean losses) are held to the project's parity bounds (tests/test_hip_parity.py header) — losses rel <= 1e-5,
gradients |dg|inf <= 1e-5 |g|inf per tensor, parameters abs <= 2e-6 (+ the Adam amplification of helpers), moments 1e-5
of max, target 1e-7; TD errors at the target_q / adv bound of check_step_against_golden (2e-5 of max).  Observed margins:
profiles/loss_weights_parity_margins.txt.
c of the draw against float64 (q_min / q_r) ** beta from leaves(): rel <= 1e-5 — fp32 exp2 / log2 at about 1 ulp each
times beta |log2 ratio| <= 20 is about 2e-6, plus margin."""
import numpy as np
import pytest
import torch

import synth
from burst_twins import eager_is_segment as _eager_is, fourth_power_weights      # (shared with the shape table's tests)
from helpers import assert_losses, check_step_against_golden, load_golden, rel_err, single_step_inputs, step_batch
from loss_weights_ref import GOLDENS

pytestmark = pytest.mark.gpu

HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}


def _trainer(S, A, gaussian=True, seed=3, dropout=0.0):
    from hip_helpers import build_hip_trainer
    params = synth.synth_params(S, A, seed=seed, gaussian=gaussian)
    return build_hip_trainer(params, S, A, gaussian, HYPER, LRS, 1000, dropout=dropout)


def _losses(log):
    return np.array([log["value_loss"], log["q_loss"], log["actor_loss"]], dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("S,A,B", [(17, 6, 256), (17, 6, 3), (39, 28, 10)])
def test_ones_weights_are_bit_for_bit_the_plain_step(S, A, B):
    from hip_helpers import assert_same_trainer_state, to_torch_batch
    plain, weighted = _trainer(S, A), _trainer(S, A)
    ones = torch.ones(B, device="cuda")
    for k in range(2):
        tb = to_torch_batch(step_batch(S, A, B, seed=20 + k))
        a = plain.train(tb)
        b = weighted.train(tb, loss_weights=ones if k == 0 else ones.reshape(B, 1))
        assert np.array_equal(_losses(a), _losses(b)), (k, a, b)
    assert_same_trainer_state(plain, weighted, "ones weights")


def test_ones_weights_with_statistics_clipping_and_dropout():
    from hip_helpers import assert_same_trainer_state, to_torch_batch
    S, A, B = 17, 6, 256
    trs = [_trainer(S, A, dropout=0.1) for _ in range(2)]
    for tr in trs:
        tr.set_dropout_seed(77)
        tr.set_step_stats(True)
        tr.set_grad_clip((0.5, 0.5, 0.5))
    ones = torch.ones(B, device="cuda")
    for k in range(2):
        tb = to_torch_batch(step_batch(S, A, B, seed=30 + k))
        a = trs[0].train(tb)
        b = trs[1].train(tb, loss_weights=ones)
        assert a.keys() == b.keys() and len(a) > 3
        for key in a:
            assert np.float32(a[key]) == np.float32(b[key]) or (np.isnan(a[key]) and np.isnan(b[key])), (k, key)
        assert trs[0].last_grad_clip() == trs[1].last_grad_clip()
    assert_same_trainer_state(trs[0], trs[1], "ones weights, all options")


# ------------------------------------------------------------------------------------------------------------- 2 and 3
MARGINS = {}


@pytest.mark.parametrize("name", GOLDENS)
def test_weighted_step_matches_weighted_reference(name):
    from hip_helpers import (assert_same_trainer_state, build_hip_trainer, head_values, read_moments, read_params,
                             to_torch_batch, unflatten_grads)
    z, meta = load_golden(name)
    params, batch, hyper = single_step_inputs(meta)
    B = meta["B"]

    def build():
        return build_hip_trainer(params, meta["S"], meta["A"], meta["gaussian"], hyper, meta["lrs"], meta["max_steps"])
    tr = build()
    tb = to_torch_batch(batch)
    c = torch.from_numpy(z["weights"]).cuda()
    grads, lw = unflatten_grads(tr, tr.flat_gradient(tb, loss_weights=c))
    hv = head_values(tr, params, B)
    tq = np.minimum(hv["qt1"], hv["qt2"])
    info = {"value_loss": lw[0], "q_loss": lw[1], "actor_loss": lw[2], "next_v": hv["next_v"], "target_q": tq,
            "adv": tq - hv["v"], "grads": grads}
    worst = check_step_against_golden(z, meta, info, None, None, grad_rtol=1e-5, loss_rtol=1e-5)
    log = tr.train(tb, loss_weights=c, return_td=True)
    got = [log["value_loss"], log["q_loss"], log["actor_loss"]]
    worst["losses"] = float(np.max(np.abs(np.array(got, dtype=np.float64) - z["losses"]) / np.abs(z["losses"])))
    td = tr.last_td_errors()
    assert tuple(td.shape) == (B, 2) and td.dtype == torch.float32 and td.is_cuda
    worst["td"] = rel_err(td.cpu().numpy(), z["inter.td"])
    worst.update(check_step_against_golden(z, meta, None, read_params(tr), read_moments(tr), param_atol=2e-6,
                                           moment_rtol=1e-5, target_atol=1e-7))
    MARGINS[name] = worst
    print(f"margins {name}: " + " ".join(f"{k}={v:.3g}" for k, v in sorted(worst.items())))
    assert_losses(got, z["losses"], 1e-5)
    assert worst["td"] <= 2e-5, worst["td"]
    assert tr.total_it == 1
    assert abs(tr.actor_optimizer.param_groups[0]["lr"] - float(z["lr_after"][0])) < 1e-18
    # return_td changes nothing else: the same step without it, bit for bit
    twin = build()
    log2 = twin.train(tb, loss_weights=c)
    assert np.array_equal(_losses(log), _losses(log2))
    assert_same_trainer_state(tr, twin, "return_td")
    with pytest.raises(RuntimeError):
        twin.last_td_errors()


def test_return_td_without_weights_is_the_plain_step():
    from hip_helpers import assert_same_trainer_state, head_values, to_torch_batch
    S, A, B = 17, 6, 300
    plain, tdtr = _trainer(S, A), _trainer(S, A)
    b = step_batch(S, A, B, seed=40)
    tb = to_torch_batch(b)
    a = plain.train(tb)
    c = tdtr.train(tb, return_td=True)
    assert np.array_equal(_losses(a), _losses(c))
    assert_same_trainer_state(plain, tdtr, "return_td alone")
    hv = head_values(tdtr, None, B)                    # the step's own head values: the TD errors are theirs
    y = b["r"] + ((np.float32(1.0) - b["d"]) * np.float32(HYPER["discount"])) * hv["next_v"]
    want = np.stack([hv["q1"] - y, hv["q2"] - y], axis=1)
    # (numpy rounds the product and the sum separately, the kernel may fuse them: a few fp32 ulps of the largest value)
    assert rel_err(tdtr.last_td_errors().cpu().numpy(), want) <= 1e-6
    plain.train(tb)
    with pytest.raises(RuntimeError):
        plain.last_td_errors()


# ------------------------------------------------------------------------------------------------------------------ 4
def _pow2_weights(n=1000, seed=9):
    rng = np.random.RandomState(seed)
    w = np.exp2(rng.randint(0, 21, size=n)).astype(np.float32)
    w[rng.rand(n) < 0.1] = 0.0
    w[0], w[1] = 1.0, 2.0 ** 20                       # both ends of the range are present
    return w


@pytest.mark.parametrize("updatable", [False, True])
@pytest.mark.parametrize("beta", [0.0, 0.4, 1.0])
def test_importance_weights_of_the_draw(updatable, beta):
    import iqlhip_weighted as wtd
    B, n_batches = 64, 3
    n = B * n_batches
    tab = wtd.SampleWeights(_pow2_weights(), updatable=updatable)
    q = tab.leaves().astype(np.float64)
    plain = tab.draw_indices(n, 11, 5).cpu().numpy()
    idx, c = tab.draw_indices(n, 11, 5, is_beta=beta, batch_size=B)
    assert c.dtype == torch.float32 and tuple(c.shape) == (n,) and c.is_cuda
    idx, c = idx.cpu().numpy(), c.cpu().numpy()
    assert np.array_equal(idx, plain)
    qr = q[idx].reshape(n_batches, B)
    assert qr.min() > 0
    want = (qr.min(axis=1, keepdims=True) / qr) ** beta
    got = c.reshape(n_batches, B).astype(np.float64)
    err = np.max(np.abs(got - want) / want)
    print(f"is weights updatable={updatable} beta={beta}: max rel err {err:.3g}, c range [{got.min():.3g}, {got.max():.3g}]")
    assert err <= 1e-5, err
    assert np.all(got.max(axis=1) == 1.0)
    if beta == 0.0:
        assert np.all(c == 1.0)
    else:
        assert got.min() < 1.0
    # one batch over all n indices (the default), and a short last batch
    _, c_all = tab.draw_indices(n, 11, 5, is_beta=beta)
    assert rel_err(c_all.cpu().numpy(), (q[idx].min() / q[idx]) ** beta) <= 1e-5
    _, c_short = tab.draw_indices(n - 10, 11, 5, is_beta=beta, batch_size=B)
    c_short = c_short.cpu().numpy().astype(np.float64)
    assert np.array_equal(c_short[: 2 * B], got[:2].ravel())
    last = q[idx[2 * B: n - 10]]
    assert np.max(np.abs(c_short[2 * B:] - (last.min() / last) ** beta) / ((last.min() / last) ** beta)) <= 1e-5


def test_buffer_draw_with_is_beta_feeds_a_weighted_step():
    """The buffer's surface: (idx, c) -> gather -> train(batch, loss_weights=c); the weighted losses are finite and differ
    from the unweighted ones of the same batch."""
    import iql
    S, A, N, B = 17, 6, 2000, 64
    data = synth.synth_transitions(N, S, A, seed=5)
    buf = iql.ReplayBuffer(S, A, N, "cuda")
    buf.load_d4rl_dataset(data)
    w = np.random.RandomState(2).rand(N).astype(np.float32) ** 4 + np.float32(1e-3)
    buf.set_sample_weights(w)
    idx, c = buf.draw_weighted_indices(B, 3, 0, is_beta=0.5)
    assert np.array_equal(idx.cpu().numpy(), buf.draw_weighted_indices(B, 3, 0).cpu().numpy())
    assert float(c.max()) == 1.0 and float(c.min()) > 0.0 and float(c.min()) < 1.0
    a, b = _trainer(S, A), _trainer(S, A)
    la = a.train(buf.gather(idx))
    lb = b.train(buf.gather(idx), loss_weights=c)
    assert np.all(np.isfinite(_losses(lb))) and np.all(_losses(lb) < _losses(la))
    with pytest.raises(ValueError):
        buf.draw_weighted_indices(B, 3, 0, batch_size=8)


# ------------------------------------------------------------------------------------------------------------- 5 and 6
BURST_S, BURST_A, BURST_N = 17, 6, 2000


def _burst_buffer():
    import iql
    buf = iql.ReplayBuffer(BURST_S, BURST_A, BURST_N, "cuda")
    buf.load_d4rl_dataset(synth.synth_transitions(BURST_N, BURST_S, BURST_A, seed=5))
    buf.set_sample_weights(fourth_power_weights(BURST_N))
    return buf


@pytest.mark.parametrize("B", [64, 300])
def test_burst_with_is_beta_equals_the_eager_loop(B):
    from hip_helpers import assert_same_trainer_state
    buf = _burst_buffer()
    burst, small, eager = (_trainer(BURST_S, BURST_A) for _ in range(3))
    lb = burst.train_steps_weighted(buf, 5, B, seed=9, is_beta=0.5)
    le = _eager_is(eager, buf, 5, B, 9, 0.5)
    assert lb.dtype == np.float32 and lb.shape == (5, 3)
    assert np.array_equal(lb, le), (lb, le)
    assert np.any(lb != _trainer(BURST_S, BURST_A).train_steps_weighted(buf, 5, B, seed=9))      # (the weights do something)
    assert_same_trainer_state(burst, eager, "burst vs eager")
    ls = small.train_steps_weighted(buf, 5, B, seed=9, is_beta=0.5, chunk=2)        # chunk=2 against chunk=64
    assert np.array_equal(ls, lb)
    assert_same_trainer_state(small, burst, "chunk=2 vs chunk=64")


def test_burst_continuation_with_another_is_beta():
    """Two calls with different is_beta against the eager loop with the same two: 3 + 2 steps (the issue's split; an odd
    first call ends on the other staging half, so the second call gathers again) and 4 + 2 (an even first call: the second
    starts on the rows and q the first one's last forward staged — a continuation)."""
    from hip_helpers import assert_same_trainer_state
    B = 64
    buf = _burst_buffer()
    for first, second in ((3, 2), (4, 2)):
        burst, eager = _trainer(BURST_S, BURST_A), _trainer(BURST_S, BURST_A)
        l1 = burst.train_steps_weighted(buf, first, B, seed=4, is_beta=0.3)
        l2 = burst.train_steps_weighted(buf, second, B, seed=4, is_beta=0.9)
        e1 = _eager_is(eager, buf, first, B, 4, 0.3)
        e2 = _eager_is(eager, buf, second, B, 4, 0.9)
        assert np.array_equal(l1, e1) and np.array_equal(l2, e2), (first, second)
        assert_same_trainer_state(burst, eager, f"{first} + {second} steps, two betas")
        # the second call's beta mattered
        other = _trainer(BURST_S, BURST_A)
        other.train_steps_weighted(buf, first, B, seed=4, is_beta=0.3)
        assert np.any(other.train_steps_weighted(buf, second, B, seed=4, is_beta=0.3) != l2)


@pytest.mark.parametrize("B", [64, 300])
def test_burst_with_is_beta_zero_is_the_weighted_burst(B):
    from hip_helpers import assert_same_trainer_state
    buf = _burst_buffer()
    a, b = _trainer(BURST_S, BURST_A), _trainer(BURST_S, BURST_A)
    la = a.train_steps_weighted(buf, 6, B, seed=9)
    lb = b.train_steps_weighted(buf, 6, B, seed=9, is_beta=0.0)
    assert np.array_equal(la, lb)
    assert_same_trainer_state(a, b, "is_beta = 0")
    # a call without is_beta does not continue one with it (no q staged), nor the reverse: both stay right
    la2 = a.train_steps_weighted(buf, 2, B, seed=9, is_beta=0.0)
    lb2 = b.train_steps_weighted(buf, 2, B, seed=9)
    assert np.array_equal(la2, lb2)
    assert_same_trainer_state(a, b, "kinds swapped")


def test_burst_is_beta_arguments_and_bf16():
    from hip_helpers import arenas
    buf = _burst_buffer()
    tr = _trainer(BURST_S, BURST_A)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            tr.train_steps_weighted(buf, 2, 64, seed=1, is_beta=bad)
    tr.set_precision("bf16")
    before, it = arenas(tr), tr.total_it
    with pytest.raises(NotImplementedError, match="bf16"):
        tr.train_steps_weighted(buf, 2, 64, seed=1, is_beta=0.5)
    with pytest.raises(NotImplementedError, match="bf16"):
        tr.prepare_train_steps_weighted(buf, 64, is_beta=0.5)
    torch.cuda.synchronize()
    assert np.array_equal(arenas(tr), before) and tr.total_it == it
    tr.set_precision("f32")
    tr.prepare_train_steps_weighted(buf, 64, is_beta=0.5)             # rehearses the graphs, trains nothing
    assert np.array_equal(arenas(tr), before) and tr.total_it == it


def test_last_td_errors_go_stale_with_any_later_step():
    from hip_helpers import to_torch_batch
    tr = _trainer(17, 6)
    tb = to_torch_batch(step_batch(17, 6, 32, seed=60))
    tr.train(tb, return_td=True)
    assert tuple(tr.last_td_errors().shape) == (32, 2)
    tr.train(tb)
    with pytest.raises(RuntimeError):
        tr.last_td_errors()
    tr.train(tb, return_td=True)
    tr.train_steps_weighted(_burst_buffer(), 2, 64, seed=1)
    with pytest.raises(RuntimeError):
        tr.last_td_errors()


# ------------------------------------------------------------------------------------------------------------------ 7
def test_bf16_refuses_loss_weights_and_leaves_the_trainer_untouched():
    import ctypes as C
    import iqlhip_binding as hb
    from hip_helpers import arenas, to_torch_batch
    S, A, B = 17, 6, 64
    tr = _trainer(S, A)
    tb = to_torch_batch(step_batch(S, A, B, seed=50))
    tr.train(tb)
    tr.set_precision("bf16")
    before, it, adam_t, lr = arenas(tr), tr.total_it, dict(tr._adam_t), tr.actor_optimizer.param_groups[0]["lr"]
    ones = torch.ones(B, device="cuda")
    with pytest.raises(NotImplementedError, match="bf16"):
        tr.train(tb, loss_weights=ones)
    with pytest.raises(NotImplementedError, match="bf16"):
        tr.train(tb, return_td=True)
    # ... and the library itself: IQLHIP_EUNSUPPORTED before anything is launched; a NULL weight pointer is IQLHIP_EINVAL
    b, keep, _ = tr._batch_struct(tb)
    sc = hb.StepScalars()
    tr._fill_scalars(sc, {g: t + 1 for g, t in tr._adam_t.items()}, tr._current_lrs(), 1.0 / B)
    rc = hb.lib().iqlhip_step_rw(tr._ctx, C.byref(b), C.byref(sc), ones.data_ptr(), None, tr._stream())
    assert rc == hb.E_UNSUPPORTED, rc
    tr.set_precision("f32")
    rc = hb.lib().iqlhip_step_rw(tr._ctx, C.byref(b), C.byref(sc), None, None, tr._stream())
    assert rc == hb.E_INVAL, rc
    torch.cuda.synchronize()
    assert np.array_equal(arenas(tr), before)
    assert (tr.total_it, tr._adam_t, tr.actor_optimizer.param_groups[0]["lr"]) == (it, adam_t, lr)
    with pytest.raises(ValueError):
        tr.train(tb, loss_weights=torch.ones(B + 1, device="cuda"))
    with pytest.raises(TypeError):
        tr.train(tb, loss_weights=torch.ones(B, device="cuda", dtype=torch.float64))
    assert np.array_equal(arenas(tr), before) and tr.total_it == it
