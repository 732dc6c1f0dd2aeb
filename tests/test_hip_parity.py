"""GPU parity tests: the HIP step (through the C ABI, via the drop-in Python surface)
against (i) the committed reference-generated goldens and (ii) the oracle on the
same seeded inputs.  Tolerances are SURVEY.md §8(d)'s teacher-forced single-step
protocol, set from the observed margins in profiles/r02_parity_margins.txt
(tools/gpu_parity_report.py): losses rel <= 1e-5 (observed 2e-7), gradients
|dg|inf <= 1e-5 * |g|inf per tensor (observed 2.6e-6; stricter than SURVEY's
1e-5 * max(1, |g|inf)), post-step parameters abs <= 2e-6 (observed 1.5e-8) plus Adam's
documented amplification for elements whose gradient is within noise of eps, Adam
moments rel-to-max <= 1e-5 (observed 5.4e-6), target abs <= 1e-7 (observed 2.6e-8).
"""
import os

import numpy as np
import pytest
import torch

import synth
from helpers import (ACT_CASES, FREERUN_CASES, SINGLE_STEP_CASES, act_case_params, assert_losses,
                     assert_params_after_free_run, batch_from,
                     check_step_against_golden,
                     load_golden, single_step_inputs, sub)

pytestmark = pytest.mark.gpu


def _hip():
    from hip_helpers import (build_hip_trainer, head_values, read_moments, read_params, to_torch_batch,
                             unflatten_grads)
    return build_hip_trainer, head_values, read_moments, read_params, to_torch_batch, unflatten_grads


@pytest.mark.parametrize("name", SINGLE_STEP_CASES)
def test_single_step_matches_reference_golden(name):
    build, head_values, read_moments, read_params, to_tb, unflat = _hip()
    z, meta = load_golden(name)
    params, batch, hyper = single_step_inputs(meta)
    tr = build(params, meta["S"], meta["A"], meta["gaussian"], hyper, meta["lrs"], meta["max_steps"])
    tb = to_tb(batch)
    flat = tr.flat_gradient(tb)
    grads, lw = unflat(tr, flat)
    hv = head_values(tr, params, meta["B"])
    tq = np.minimum(hv["qt1"], hv["qt2"])
    info = {"value_loss": lw[0], "q_loss": lw[1], "actor_loss": lw[2], "next_v": hv["next_v"],
            "target_q": tq, "adv": tq - hv["v"], "grads": grads}
    check_step_against_golden(z, meta, info, None, None, grad_rtol=1e-5, loss_rtol=1e-5)
    log = tr.train(tb)
    assert_losses([log["value_loss"], log["q_loss"], log["actor_loss"]], z["losses"], 1e-5)
    assert tr.total_it == 1
    check_step_against_golden(z, meta, None, read_params(tr), read_moments(tr), param_atol=2e-6,
                              moment_rtol=1e-5, target_atol=1e-7)
    # the cosine schedule advanced exactly like the reference's
    assert abs(tr.actor_optimizer.param_groups[0]["lr"] - float(z["lr_after"][0])) < 1e-18


@pytest.mark.parametrize("name", FREERUN_CASES)
def test_free_run_10_steps_matches_reference(name):
    build, _, _, read_params, to_tb, _ = _hip()
    z, meta = load_golden(name)
    S, A = meta["S"], meta["A"]
    params = synth.synth_params(S, A, seed=meta["seed"], gaussian=meta["gaussian"])
    data = synth.synth_transitions(meta["N"], S, A, seed=2000 + meta["seed"])
    hyper = dict(meta["hyper"])
    tr = build(params, S, A, meta["gaussian"], hyper, meta["lrs"], meta["max_steps"])
    for k in range(meta["n_steps"]):
        assert abs(tr.actor_optimizer.param_groups[0]["lr"] - z["actor_lr_used"][k]) < 1e-18
        log = tr.train(to_tb(batch_from(data, z["indices"][k])))
        assert_losses([log["value_loss"], log["q_loss"], log["actor_loss"]], z["losses"][k], 1e-5, what=f"step {k}")
    got = read_params(tr)
    for net, tensors in got.items():
        for t, p in tensors.items():
            want = z[f"param.{net}.{t}"]
            lr = meta["lrs"]["pi" if net == "pi" else ("v" if net == "vf" else "q")]
            assert_params_after_free_run(sub(p, meta["stride"]).reshape(want.shape), want, meta["n_steps"], lr, (net, t))


def test_free_run_through_replay_buffer_and_numpy_rng():
    """The loop call site H1: np.random.seed -> buffer.sample -> train reproduces
    the reference's index stream and losses."""
    import iql
    build, _, _, _, _, _ = _hip()
    z, meta = load_golden("g2_freerun_S17A6")
    S, A, N = meta["S"], meta["A"], meta["N"]
    params = synth.synth_params(S, A, seed=meta["seed"], gaussian=True)
    data = synth.synth_transitions(N, S, A, seed=2000 + meta["seed"])
    tr = build(params, S, A, True, dict(meta["hyper"]), meta["lrs"], meta["max_steps"])
    buf = iql.ReplayBuffer(S, A, N, "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in data.items()})
    np.random.seed(meta["seed"])
    for k in range(meta["n_steps"]):
        batch = buf.sample(meta["B"])
        assert batch[2].shape == (meta["B"], 1) and batch[4].shape == (meta["B"], 1)
        log = tr.train(batch)
        assert_losses([log["value_loss"], log["q_loss"], log["actor_loss"]], z["losses"][k], 1e-5, what=f"step {k}")


def test_step_matches_oracle_on_fresh_seeds():
    """Oracle comparison on inputs no fixture covers (B=64 and B=512, S=11, A=3)."""
    from oracle import iql_oracle as O
    build, _, read_moments, read_params, to_tb, unflat = _hip()
    for B, gaussian, seed in ((64, True, 301), (512, False, 302), (33, True, 303)):
        S, A = 11, 3
        params = synth.synth_params(S, A, seed=seed, gaussian=gaussian)
        d = synth.synth_transitions(B, S, A, seed=seed + 1)
        batch = {"s": d["observations"], "a": d["actions"], "r": d["rewards"], "ns": d["next_observations"],
                 "d": d["terminals"]}
        hyper = {"iql_tau": 0.8, "beta": 5.0, "discount": 0.97, "tau": 0.01, "deterministic": not gaussian}
        lrs = {"v": 1e-3, "q": 2e-4, "pi": 5e-4}
        tr = build(params, S, A, gaussian, hyper, lrs, None)
        newp, newo, info = O.iql_step(params, O.new_opt_state(params), batch, hyper, lrs)
        grads, lw = unflat(tr, tr.flat_gradient(to_tb(batch)))
        for n, t in grads.items():
            for k, g in t.items():
                want = info["grads"][n][k]
                assert np.max(np.abs(g - want)) <= 3e-5 * max(np.max(np.abs(want)), 1e-30), (B, n, k)
        log = tr.train(to_tb(batch))
        assert_losses([log["value_loss"], log["q_loss"], log["actor_loss"]],
                      [info["value_loss"], info["q_loss"], info["actor_loss"]], 1e-5)
        got = read_params(tr)
        for n, t in got.items():
            for k, p in t.items():
                assert np.max(np.abs(p - newp[n][k])) <= 2e-6, (B, n, k)
        assert tr.actor_lr_schedule is None


def test_step_is_deterministic_and_batch_agnostic_to_padding():
    """Bitwise run-to-run determinism (slab reductions, no float atomics) and no leakage from
    a previous larger batch into a smaller one (rows >= B are masked)."""
    build, _, _, read_params, to_tb, _ = _hip()
    S, A = 17, 6
    params = synth.synth_params(S, A, seed=5)
    hyper = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    big = synth.synth_transitions(256, S, A, seed=6)
    small = {k: v[:100].copy() for k, v in big.items()}
    bb = {"s": big["observations"], "a": big["actions"], "r": big["rewards"], "ns": big["next_observations"],
          "d": big["terminals"]}
    sb = {"s": small["observations"], "a": small["actions"], "r": small["rewards"],
          "ns": small["next_observations"], "d": small["terminals"]}
    outs = []
    for warm in (False, True):
        tr = build(params, S, A, True, hyper, lrs, 1000)
        if warm:
            tr.flat_gradient(to_tb(bb))   # fills scratch rows 100..255 with other data
        tr.train(to_tb(sb))
        outs.append(read_params(tr))
    for n in outs[0]:
        for k in outs[0][n]:
            assert np.array_equal(outs[0][n][k], outs[1][n][k]), (n, k)


def test_error_behaviour_matches_reference():
    import iql
    build, _, _, _, to_tb, _ = _hip()
    S, A = 17, 6
    params = synth.synth_params(S, A, seed=5, gaussian=False)
    tr = build(params, S, A, False, {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005},
               {"v": 3e-4, "q": 3e-4, "pi": 3e-4}, 1000)
    d = synth.synth_transitions(32, S, A, seed=6)
    bad = [torch.from_numpy(d["observations"]).cuda(), torch.zeros(32, A + 1).cuda(),
           torch.zeros(32, 1).cuda(), torch.from_numpy(d["next_observations"]).cuda(), torch.zeros(32, 1).cuda()]
    with pytest.raises(RuntimeError, match="Actions shape missmatch"):
        tr.train(bad)
    buf = iql.ReplayBuffer(S, A, 16, "cuda")
    with pytest.raises(ValueError, match="smaller than the dataset"):
        buf.load_d4rl_dataset(d)


def test_split_step_equals_fused_step():
    """forward_backward -> flat gradient -> apply_update (the data-parallel path, world = 1, no
    collective) lands bitwise on the same parameters as the fused single-GPU step."""
    build, _, _, read_params, to_tb, _ = _hip()
    import ctypes as C
    import iqlhip_binding as hb
    S, A = 17, 6
    params = synth.synth_params(S, A, seed=9)
    hyper = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    d = synth.synth_transitions(256, S, A, seed=10)
    batch = {"s": d["observations"], "a": d["actions"], "r": d["rewards"], "ns": d["next_observations"],
             "d": d["terminals"]}
    fused = build(params, S, A, True, hyper, lrs, 1000)
    log = fused.train(to_tb(batch))
    split = build(params, S, A, True, hyper, lrs, 1000)
    b, keep, B = split._batch_struct(to_tb(batch))
    split.total_it += 1
    for g in split._adam_t:
        split._adam_t[g] += 1
    sc = hb.StepScalars()
    split._fill_scalars(sc, split._adam_t, split._current_lrs(), 1.0 / B)
    flat = split._dp_flat()
    lib = hb.lib()
    hb.check(lib.iqlhip_forward_backward(split._ctx, C.byref(b), C.byref(sc), flat.data_ptr(), split._stream()))
    hb.check(lib.iqlhip_apply_update(split._ctx, flat.data_ptr(), C.byref(sc), split._stream()))
    out = (C.c_float * 3)()
    hb.check(lib.iqlhip_read_losses(split._ctx, out, split._stream()))
    assert [float(x) for x in out] == [log["value_loss"], log["q_loss"], log["actor_loss"]]
    pa, pb = read_params(fused), read_params(split)
    for n in pa:
        for k in pa[n]:
            assert np.array_equal(pa[n][k], pb[n][k]), (n, k)


@pytest.mark.parametrize("K,B", [(7, 256), (1, 100), (4, 33), (5, 600), (18, 1024)])
def test_train_steps_graph_matches_eager_steps_on_same_indices(K, B):
    """K steps replayed as one hipGraph (device index draw; the rows of step k+1 staged by the idle blocks of forward
    k into the other staging buffer) equal K eager steps fed with the same indices — bitwise.  Odd and even K, K = 1,
    ragged batches; 600 and 1 024 rows run the multi-slice block layouts (fewer idle forward blocks stage the next
    rows; 18 steps = one 16-step chunk graph + 2 direct steps)."""
    import ctypes as C
    import iql
    import iqlhip_binding as hb
    build, _, _, read_params, _, _ = _hip()
    S, A, N = 17, 6, 5000
    params = synth.synth_params(S, A, seed=21)
    hyper = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    data = synth.synth_transitions(N, S, A, seed=22)
    buf = iql.ReplayBuffer(S, A, N, "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in data.items()})
    g = build(params, S, A, True, hyper, lrs, 1000)
    losses = g.train_steps(buf, K, B, seed=77)
    assert losses.shape == (K, 3) and np.all(np.isfinite(losses)) and g.total_it == K
    # replay the same index stream eagerly
    e = build(params, S, A, True, hyper, lrs, 1000)
    idx = torch.empty(K * B, dtype=torch.int64, device="cuda")
    hb.check(hb.lib().iqlhip_draw_indices(idx.data_ptr(), K * B, N, 77, 0, torch.cuda.current_stream().cuda_stream))
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    for k in range(K):
        log = e.train(buf.gather(idx[k * B:(k + 1) * B]))
        assert [log["value_loss"], log["q_loss"], log["actor_loss"]] == [float(x) for x in losses[k]]
    pa, pb = read_params(g), read_params(e)
    for n in pa:
        for kk in pa[n]:
            assert np.array_equal(pa[n][kk], pb[n][kk]), (n, kk)
    assert g.actor_optimizer.param_groups[0]["lr"] == e.actor_optimizer.param_groups[0]["lr"]
    sd = g.state_dict()
    assert float(sd["q_optimizer"]["state"][0]["step"]) == K
    # a second chunk on the same trainer continues from the first (graph cache hit, fresh indices)
    more = g.train_steps(buf, K, B, seed=78)
    assert more.shape == (K, 3) and np.all(np.isfinite(more)) and g.total_it == 2 * K


def test_device_index_draw_is_uniform():
    import iqlhip_binding as hb
    n, size = 1 << 20, 1000
    idx = torch.empty(n, dtype=torch.int64, device="cuda")
    hb.check(hb.lib().iqlhip_draw_indices(idx.data_ptr(), n, size, 123, 0, torch.cuda.current_stream().cuda_stream))
    c = torch.bincount(idx, minlength=size).double().cpu().numpy()
    assert c.sum() == n and c.min() > 0
    chi2 = float(((c - n / size) ** 2 / (n / size)).sum())
    assert 800 < chi2 < 1250, chi2      # 999 dof: mean 999, sd ~45


def test_dp_multi_step_loop_world1_equals_graph_steps():
    """train_steps_dp (the loop bench.py runs under torch.distributed) at world = 1 walks the same
    device index stream as train_steps and lands on the same parameters bitwise."""
    import iql
    build, _, _, read_params, _, _ = _hip()
    S, A, N, B, K = 17, 6, 5000, 256, 5
    params = synth.synth_params(S, A, seed=31)
    hyper = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    data = synth.synth_transitions(N, S, A, seed=32)
    buf = iql.ReplayBuffer(S, A, N, "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in data.items()})
    g = build(params, S, A, True, hyper, lrs, 1000)
    g.train_steps(buf, K, B, seed=5, return_losses=False)
    d = build(params, S, A, True, hyper, lrs, 1000)
    d.train_steps_dp(buf, K, B, seed=5)
    torch.cuda.synchronize()
    assert d.total_it == K
    pa, pb = read_params(g), read_params(d)
    for n in pa:
        for kk in pa[n]:
            assert np.array_equal(pa[n][kk], pb[n][kk]), (n, kk)


@pytest.mark.parametrize("name", ["g9_dropout_S39A28_gauss", "g9_dropout_S17A6_det"])
def test_dropout_step_with_injected_masks_matches_reference(name):
    """Actor dropout arithmetic: the same keep-masks were injected into the reference's nn.Dropout."""
    build, _, read_moments, read_params, to_tb, unflat = _hip()
    z, meta = load_golden(name)
    params, batch, hyper = single_step_inputs(meta)
    p = meta["dropout"]
    tr = build(params, meta["S"], meta["A"], meta["gaussian"], hyper, meta["lrs"], meta["max_steps"], dropout=p)
    assert list(tr.actor.state_dict().keys()) == meta["actor_state_keys"]     # net.net.{0,3,6}.* with dropout
    k0, k1 = synth.synth_dropout_keep(meta["B"], p, seed=meta["seed"])
    tr.inject_dropout_masks(k0, k1)
    tb = to_tb(batch)
    grads, lw = unflat(tr, tr.flat_gradient(tb))
    info = {"value_loss": lw[0], "q_loss": lw[1], "actor_loss": lw[2], "grads": grads}
    check_step_against_golden(z, meta, info, None, None, grad_rtol=1e-5, loss_rtol=1e-5)
    log = tr.train(tb)
    assert_losses([log["value_loss"], log["q_loss"], log["actor_loss"]], z["losses"], 1e-5)
    check_step_against_golden(z, meta, None, read_params(tr), read_moments(tr), param_atol=2e-6, moment_rtol=1e-5,
                              target_atol=1e-7)


def test_dropout_device_masks_statistics_and_eval_mode():
    """Device-drawn keep-bits: rate 1-p, independent across steps/layers; eval() switches dropout off."""
    build, _, _, read_params, to_tb, _ = _hip()
    S, A, B, p = 17, 6, 256, 0.1
    params = synth.synth_params(S, A, seed=41)
    hyper = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    d = synth.synth_transitions(B, S, A, seed=42)
    batch = {"s": d["observations"], "a": d["actions"], "r": d["rewards"], "ns": d["next_observations"],
             "d": d["terminals"]}
    tr = build(params, S, A, True, hyper, lrs, 1000, dropout=p)
    tr.train(to_tb(batch))
    bits1 = tr.debug_read("drop_bits").view(np.uint32).reshape(2, tr._max_batch, 8)[:, :B].copy()
    tr.train(to_tb(batch))
    bits2 = tr.debug_read("drop_bits").view(np.uint32).reshape(2, tr._max_batch, 8)[:, :B].copy()
    ones = np.unpackbits(bits1.view(np.uint8)).mean()
    assert abs(ones - (1 - p)) < 0.01, ones                      # 131072 bits: sd 0.0008
    assert not np.array_equal(bits1, bits2) and not np.array_equal(bits1[0], bits1[1])
    # the masks really are applied: post-dropout h1 of the policy has ~p more zeros than relu alone
    h1 = tr.debug_read("h1").reshape(4, tr._max_batch, 256)[3, :B]
    keep = np.unpackbits(bits2[1].view(np.uint8), bitorder="little").reshape(B, 256).astype(bool)
    assert np.all(h1[~keep] == 0.0)
    # eval mode: no dropout -> equals a dropout-free trainer
    a = build(params, S, A, True, hyper, lrs, 1000, dropout=p)
    a.actor.eval()
    b = build(params, S, A, True, hyper, lrs, 1000, dropout=0.0)
    la, lb = a.train(to_tb(batch)), b.train(to_tb(batch))
    assert la == lb


def test_dropout_in_graph_steps_is_seeded_and_varies_per_step():
    import iql
    build, _, _, read_params, _, _ = _hip()
    S, A, N, B, K = 17, 6, 4000, 256, 6
    params = synth.synth_params(S, A, seed=51)
    hyper = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    buf = iql.ReplayBuffer(S, A, N, "cuda")
    buf.load_d4rl_dataset(synth.synth_transitions(N, S, A, seed=52))
    runs = []
    for rep in range(2):
        torch.manual_seed(1234)
        tr = build(params, S, A, True, hyper, lrs, 1000, dropout=0.2)
        runs.append((tr.train_steps(buf, K, B, seed=9), read_params(tr)))
    torch.manual_seed(1234)
    base = build(params, S, A, True, hyper, lrs, 1000, dropout=0.0)
    l0 = base.train_steps(buf, K, B, seed=9)
    assert np.array_equal(runs[0][0], runs[1][0])                      # same torch seed -> same masks
    for n in runs[0][1]:
        for k in runs[0][1][n]:
            assert np.array_equal(runs[0][1][n][k], runs[1][1][n][k])
    assert np.allclose(runs[0][0][0, :2], l0[0, :2], rtol=0, atol=0)      # step 0: identical V and Q losses
    assert not np.allclose(runs[0][0][:, 2], l0[:, 2])                   # actor loss differs (masks applied)


@pytest.mark.parametrize("name", ["g1_S17A6_gauss_b3", "g1_S39A28_gauss_b10", "g1_S29A8_det_b10"])
def test_bf16_operand_mode_tracks_fp32_reference(name):
    """BASELINE config 5's "MFMA bf16 path": bf16 operands / fp32 accumulate in the layer-0 / layer-1 / dW1 / dH0 / dW0
    products.  Tolerance: losses rel <= 5e-3 single-step vs the fp32 reference fixture (observed worst 9e-4);
    gradients within 8.5e-2 in relative L2 norm per tensor (bf16 operands carry 8 significant bits; observed worst 7.55e-2)."""
    build, _, _, _, to_tb, unflat = _hip()
    z, meta = load_golden(name)
    params, batch, hyper = single_step_inputs(meta)
    tr = build(params, meta["S"], meta["A"], meta["gaussian"], hyper, meta["lrs"], meta["max_steps"])
    tr.set_precision("bf16")
    tb = to_tb(batch)
    grads, lw = unflat(tr, tr.flat_gradient(tb))
    assert_losses(lw, z["losses"], 5e-3)
    from oracle import iql_oracle as O
    info = O.iql_losses_and_grads(params, batch, hyper)
    worst = 0.0
    for n, t in grads.items():
        for k, g in t.items():
            want = info["grads"][n][k]
            if want.size <= 32:
                # head-bias / log_std gradients are means of signed residuals (heavy cancellation): their own
                # norm is no yardstick — bound the absolute error against the residual scale (O(1)) instead
                assert np.max(np.abs(g - want)) <= 2e-2 * max(1.0, float(np.max(np.abs(want)))), (n, k)
                continue
            rel = float(np.linalg.norm(g - want) / max(np.linalg.norm(want), 1e-30))
            worst = max(worst, rel)
            assert rel <= 8.5e-2, (n, k, rel)
    assert worst > 1e-5          # the mode really is active (fp32 would sit at ~1e-7)
    worst_l = max(abs(float(g) - float(w)) / abs(float(w)) for g, w in zip(lw, z["losses"]))
    print(f"{name}: bf16 worst relative-L2 gradient error {worst:.3e}, worst loss error {worst_l:.3e}")
    log = tr.train(tb)
    assert_losses([log["value_loss"], log["q_loss"], log["actor_loss"]], z["losses"], 5e-3)
    tr.set_precision("f32")
    log2 = tr.train(tb)
    assert all(np.isfinite(v) for v in log2.values())


def test_bf16_large_batch_config5_shape():
    """obs=39, act=28, 1024 rows per GPU (config 5 at 8 GPUs), Gaussian policy with dropout 0.1: runs, finite,
    and the bf16 losses track the fp32 losses of the same step."""
    build, _, _, _, to_tb, _ = _hip()
    S, A, B = 39, 28, 1024
    params = synth.synth_params(S, A, seed=61)
    hyper = {"iql_tau": 0.8, "beta": 3.0, "discount": 0.99, "tau": 0.005}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    d = synth.synth_transitions(B, S, A, seed=62)
    batch = {"s": d["observations"], "a": d["actions"], "r": d["rewards"], "ns": d["next_observations"],
             "d": d["terminals"]}
    k0, k1 = synth.synth_dropout_keep(B, 0.1, seed=63)
    a = build(params, S, A, True, hyper, lrs, 1000, dropout=0.1)
    a.inject_dropout_masks(k0, k1)
    la = a.train(to_tb(batch))
    b = build(params, S, A, True, hyper, lrs, 1000, dropout=0.1)
    b.set_precision("bf16")
    b.inject_dropout_masks(k0, k1)
    lb = b.train(to_tb(batch))
    for k in la:
        assert np.isfinite(lb[k]) and abs(lb[k] - la[k]) <= 2e-2 * abs(la[k]), (k, la[k], lb[k])


@pytest.mark.parametrize("S,A,B,bf16", [(17, 6, 300, False), (39, 28, 1024, False), (39, 28, 600, True)])
def test_slices_per_block_layouts_are_bit_identical(S, A, B, bf16, monkeypatch):
    """Large batches run forward blocks / backward (b) blocks that walk 2 or 4 column slices (launch_fwd / launch_bwd in
    csrc/iqlhip.hip).  The layout must not change a single bit: every layout forced through the library's diagnostic
    switches gives the parameters, moments and losses of the one-slice layout after two steps (ragged batches too)."""
    build, _, _, read_params, to_tb, _ = _hip()
    from hip_helpers import read_moments
    params = synth.synth_params(S, A, seed=71)
    hyper = {"iql_tau": 0.8, "beta": 3.0, "discount": 0.99, "tau": 0.005}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    d = synth.synth_transitions(B, S, A, seed=72)
    batch = {"s": d["observations"], "a": d["actions"], "r": d["rewards"], "ns": d["next_observations"],
             "d": d["terminals"]}
    outs = {}
    for fwd, bwd in (("0", "0"), ("1", "1"), ("2", "2"), (None, None)):
        for var, val in (("IQLHIP_FWD_SPB_L2", fwd), ("IQLHIP_BWD_SPB_L2", bwd)):
            if val is None:
                monkeypatch.delenv(var, raising=False)
            else:
                monkeypatch.setenv(var, val)              # read when the library context is created (first step)
        tr = build(params, S, A, True, hyper, lrs, 1000)
        if bf16:
            tr.set_precision("bf16")
        logs = [tr.train(to_tb(batch)) for _ in range(2)]
        outs[(fwd, bwd)] = (logs, read_params(tr), read_moments(tr))
    if bf16:
        # bf16 path: the multi-slice layouts share ONE backward structure (a (b) block takes the whole row tile: the waves
        # split the columns, not the k range) — they must agree bit for bit; the one-slice layout sums dH0's k range in
        # another order (four waves' partial sums), equally valid: it must agree to bf16-path accuracy
        # (without the switches a bf16 batch of 600 rows takes the LARGE-BATCH kernels, iqlhip_lb_kernels.h — a third valid
        #  bf16 evaluation of the step, held to the same accuracy; tests/test_hip_lb.py checks it against the oracle)
        ref = outs[("1", "1")]
        for other in (outs.pop(("0", "0")), outs.pop((None, None))):
            for a_, b_ in zip(other[0], ref[0]):
                for k in a_:
                    assert abs(a_[k] - b_[k]) <= 2e-3 * abs(b_[k]), (k, a_[k], b_[k])
            for n in ref[1]:
                for k in ref[1][n]:
                    assert np.max(np.abs(other[1][n][k] - ref[1][n][k])) <= 2.5 * 2 * 3e-4, (n, k)     # within two Adam steps' reach
    else:
        ref = outs[("0", "0")]
    for key, (logs, prm, mom) in outs.items():
        assert logs == ref[0], key
        for n in prm:
            for k in prm[n]:
                assert np.array_equal(prm[n][k], ref[1][n][k]), (key, n, k)
        for which in ("m", "v"):
            for n in mom[which]:
                for k in mom[which][n]:
                    assert np.array_equal(mom[which][n][k], ref[2][which][n][k]), (key, which, n, k)


_EDGE_W0_LDS_K = {(100, 28): 0, (96, 32): 0, (50, 10): 60, (65, 31): 65, (64, 32): 64, (72, 28): 72, (127, 1): 0,
                  (39, 28): 67, (17, 6): 23}


@pytest.mark.parametrize("S,A,B,gaussian", [
    (100, 28, 64, True),     # k_in = 128 (limit): layer-0 weights streamed from global, 8 k-tiles in dW0
    (96, 32, 40, False),     # action_dim = 32 (limit): two 16-wide head tiles, four pi chunks
    (2, 1, 256, True),       # smallest dims
    (17, 6, 1, True),        # single row
    (17, 6, 257, True),      # one row past a 256-row chunk
    (50, 10, 300, True),     # k_in = 60 (V: 50): LDS-staged W0 through the generic k loop
    (65, 31, 70, True),      # k_in = 96 does not fit LDS beside a 32-wide head tile: w0_lds_k = 65, V and pi staged by
                             # LDS-DMA, the critics from global; 31 action dims (ragged last chunk of 8)
    (64, 32, 256, False),    # k_in = 96 and action_dim = 32 together, deterministic policy: w0_lds_k = 64, V and pi staged
                             # through registers (the widest such copy), the critics from global
    (72, 28, 70, True),      # k_in = 100 > 96, S = 72 fits: split staging inside the LDS-DMA kernel, 44 float4 per row
    (127, 1, 40, True),      # the widest packed row: 260 floats, 65 float4 (a 32-row tile fills the forward's ninth
    (127, 1, 300, True),     # register); A = 1; every W0 from global; 300 rows: ragged chunk and several column slices
    (40, 17, 256, True),     # 17 action dims: Dp = 32 with 15 padding dims; Q inputs 57 wide (register-staged)
    (3, 9, 33, True),        # 9 action dims: second 8-dim group holds a single dim
    (39, 28, 1024, True),    # config 5 per-GPU shape: 4 chunks, 32 row tiles
    (39, 28, 8192, True),    # config 5's whole global batch on one GPU: 32 chunk slabs, 256 row-tile partials
    (17, 6, 16384, False),   # the library's largest batch (64 chunks: the loss-partials table is full)
])
def test_edge_shapes_match_oracle(S, A, B, gaussian):
    from oracle import iql_oracle as O
    from helpers import w0_lds_k
    build, _, _, read_params, to_tb, unflat = _hip()
    if (S, A) in _EDGE_W0_LDS_K:           # the staging the case's comment names, checked against the host rule's restatement
        assert w0_lds_k(S, A) == _EDGE_W0_LDS_K[(S, A)]
    params = synth.synth_params(S, A, seed=7 * S + A, gaussian=gaussian)
    d = synth.synth_transitions(B, S, A, seed=S + A + B)
    batch = {"s": d["observations"], "a": d["actions"], "r": d["rewards"], "ns": d["next_observations"],
             "d": d["terminals"]}
    hyper = {"iql_tau": 0.9, "beta": 10.0, "discount": 0.99, "tau": 0.005, "deterministic": not gaussian}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    tr = build(params, S, A, gaussian, hyper, lrs, 1000)
    newp, newo, info = O.iql_step(params, O.new_opt_state(params), batch, hyper, lrs)
    # losses and gradients against the oracle evaluated in float64 (two fp32 evaluations of a cancelling sum can each
    # sit 1e-5 from the truth; against the float64 value the fp32 kernels hold north_star's 1e-5 on the losses and
    # SURVEY §8d's |dg|inf <= 1e-5 * max(1, |g|inf) on every gradient tensor)
    i64 = O.iql_losses_and_grads(params, batch, hyper, dtype=np.float64)
    want_l = [i64["value_loss"], i64["q_loss"], i64["actor_loss"]]
    grads, lw = unflat(tr, tr.flat_gradient(to_tb(batch)))
    assert_losses(lw, want_l, 1e-5)
    for n, t in grads.items():
        for k, g in t.items():
            want = i64["grads"][n][k]
            gmax = float(np.max(np.abs(want)))
            err = float(np.max(np.abs(g.astype(np.float64) - want)))
            assert err <= 1e-5 * max(1.0, gmax), (n, k, err, gmax)
            # ... and relative to the tensor's own max — up to 2 048 rows: with 16 384 rows x 256 units some
            # pre-activation lies within fp32 rounding of zero, its ReLU takes the other branch than in float64 and that
            # one row's term (|x dH0| / B ~ 1e-6) shows against a mean gradient that has shrunk to ~1e-3 (DESIGN §2,
            # "ReLU-flip"); the absolute bound above still holds there
            if B <= 2048:
                assert err <= 2e-5 * max(gmax, 1e-30), (n, k, err / max(gmax, 1e-30))
    log = tr.train(to_tb(batch))
    assert_losses([log["value_loss"], log["q_loss"], log["actor_loss"]], want_l, 1e-5)
    got = read_params(tr)
    for n, t in got.items():
        for k, p in t.items():
            diff = np.abs(p - newp[n][k])
            if n in ("qt1", "qt2"):
                assert diff.max() <= 1e-7, (n, k)
            else:   # Adam amplifies rounding of near-eps gradients: allow it exactly there (see helpers.py)
                gref = np.abs(info["grads"][n][k])
                tol = 2e-6 + 3e-4 * np.minimum(1.0, 1e-8 * (2e-6 * max(gref.max(), 1e-30)) / (gref + 1e-8) ** 2)
                assert np.all(diff <= tol), (n, k, float(diff.max()))


# ---------------------------------------------------------------------------
# Policy inference: iqlhip_actor_forward behind actor.act() / trainer.actor_forward()
_HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
_LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}


def _act_trainer(meta, z, dropout=0.0):
    from hip_helpers import build_hip_trainer
    params = synth.synth_params(meta["S"], meta["A"], seed=meta["seed"], gaussian=meta["gaussian"])
    params["pi"] = act_case_params(meta, z)
    return build_hip_trainer(params, meta["S"], meta["A"], meta["gaussian"], _HYPER, _LRS, 1000, dropout=dropout,
                             max_action=meta["max_action"])


@pytest.mark.parametrize("name", ACT_CASES)
def test_actor_act_matches_reference(name):
    """G10: actor.act(state, "cuda") one state at a time (eval mode) and the batched forward, against the
    reference's GaussianPolicy.act / DeterministicPolicy.act outputs; abs 2e-6 * max_action (tanh at 1 ulp)."""
    import torch
    z, meta = load_golden(name)
    tr = _act_trainer(meta, z)
    tol = 2e-6 * max(1.0, meta["max_action"])
    tr.actor.eval()
    calls = []
    orig = tr.act_one
    tr.act_one = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    for i in range(0, meta["n"], 5):
        a = tr.actor.act(z["states"][i], "cuda")
        assert a.shape == (meta["A"],) and a.dtype == np.float32
        assert np.max(np.abs(a - z["actions_eval"][i])) <= tol, i
    assert len(calls) == len(range(0, meta["n"], 5))          # the library path served every call
    got = tr.actor_forward(torch.from_numpy(z["states"]).cuda()).cpu().numpy()
    assert np.max(np.abs(got - z["actions_eval"])) <= tol
    if meta["gaussian"]:       # training-mode formula with the fixture's noise through the C ABI directly
        import ctypes as C
        import iqlhip_binding as hb
        x = torch.from_numpy(z["states"]).cuda()
        nz = torch.from_numpy(z["noise"]).cuda()
        out = torch.empty((meta["n"], meta["A"]), device="cuda")
        hb.check(hb.lib().iqlhip_actor_forward(tr._ctx, x.data_ptr(), meta["S"], meta["n"], nz.data_ptr(), meta["A"],
                                               float(meta["max_action"]), out.data_ptr(), meta["A"], tr._stream()))
        torch.cuda.synchronize()
        # sigma up to e^2: the noise term amplifies nothing, but |a| reaches ~20 before the clamp -> relative bound
        assert np.max(np.abs(out.cpu().numpy() - z["actions_noise"])) <= 4e-6 * max(1.0, meta["max_action"])


def test_actor_forward_chunks_ragged_and_after_training():
    """n = 1, a ragged tile, and n > max_batch (chunked) against the oracle with the CURRENT parameters — i.e. the
    inference path reads the same arena the training step updates."""
    import torch
    from oracle import iql_oracle as O
    from hip_helpers import read_params
    z, meta = load_golden("g10_act_S17A6_gauss")
    tr = _act_trainer(meta, z)
    S, A = meta["S"], meta["A"]
    data = synth.synth_transitions(256, S, A, seed=5)
    from hip_helpers import to_torch_batch
    for _ in range(3):
        tr.train(to_torch_batch({"s": data["observations"], "a": data["actions"], "r": data["rewards"],
                                 "ns": data["next_observations"], "d": data["terminals"]}))
    pi = read_params(tr)["pi"]
    rng = np.random.default_rng(3)
    for n in (1, 33, 700, 5000):
        x = rng.standard_normal((n, S)).astype(np.float32)
        got = tr.actor_forward(torch.from_numpy(x).cuda()).cpu().numpy()
        want = O.actor_act(pi, x, meta["max_action"])
        assert got.shape == (n, A)
        assert np.max(np.abs(got - want)) <= 2e-6
    # sampling mode: mean + sigma * N(0,1), clamped; statistics only (device RNG stream)
    x = np.repeat(rng.standard_normal((1, S)).astype(np.float32), 4096, axis=0)
    smp = tr.actor_forward(torch.from_numpy(x).cuda(), sample=True).cpu().numpy()
    mean = O.actor_act(pi, x[:1], meta["max_action"])[0]
    sigma = np.exp(np.clip(pi["log_std"], -20, 2))
    free = (np.abs(mean) + 4 * sigma < meta["max_action"]) & (sigma > 1e-3)   # dims the clamp leaves alone
    assert np.all(np.abs(smp).max(0) <= meta["max_action"])
    if free.any():
        assert np.max(np.abs(smp.mean(0)[free] - mean[free]) / (sigma[free] / 64 + 1e-6)) < 5.0
        assert np.max(np.abs(smp.std(0)[free] / sigma[free] - 1.0)) < 0.1
        zs = (smp[:, free] - mean[free]) / sigma[free]                      # device Box-Muller draws: N(0,1) shape
        assert abs(float(np.mean(zs ** 3))) < 0.15 and abs(float(np.mean(zs ** 4)) - 3.0) < 0.4
        assert abs(float(np.corrcoef(zs[:-1, 0], zs[1:, 0])[0, 1])) < 0.08  # consecutive rows uncorrelated (5 sigma)
    again = tr.actor_forward(torch.from_numpy(x).cuda(), sample=True).cpu().numpy()
    assert not np.array_equal(again, smp)                                   # the call counter advances the stream


@pytest.mark.parametrize("S,A,gaussian", [(72, 28, True), (127, 1, True)])
def test_actor_forward_at_the_staging_edges_against_the_float64_policy(S, A, gaussian):
    """The one-instance forward (the ONE = true instantiations of the training forward's body) where layer-0 staging
    splits — (72, 28): the policy staged by LDS-DMA in the kernel whose critics are not — and at the widest state,
    (127, 1): W0 from global, one action dim.  Against the policy forward in float64, at
    test_actor_forward_chunks_ragged_and_after_training's bound (abs 2e-6 on an action in [-1, 1]: tanh at about an ulp);
    one row, a ragged tile, several tiles."""
    import torch
    from oracle import iql_oracle as O
    from hip_helpers import build_hip_trainer
    params = synth.synth_params(S, A, seed=7 * S + A, gaussian=gaussian)
    tr = build_hip_trainer(params, S, A, gaussian, _HYPER, _LRS, 1000)
    rng = np.random.default_rng(S + A)
    for n in (1, 33, 300):
        x = rng.standard_normal((n, S)).astype(np.float32)
        got = tr.actor_forward(torch.from_numpy(x).cuda()).cpu().numpy()
        want = O.actor_act(params["pi"], x, 1.0, dtype=np.float64)
        assert got.shape == (n, A) and got.dtype == np.float32
        assert np.max(np.abs(got - want)) <= 2e-6, (n, float(np.max(np.abs(got - want))))


def test_actor_act_falls_back_to_torch_where_the_library_cannot_serve():
    """CPU device string and training-mode dropout stay on the module's own forward (no library call)."""
    import torch
    z, meta = load_golden("g10_act_S29A8_det")
    tr = _act_trainer(meta, z, dropout=0.1)
    calls = []
    tr.act_one = lambda *a, **k: calls.append(1)
    tr.actor.train()
    a = tr.actor.act(z["states"][0], "cuda")          # dropout active -> PyTorch path (random masks)
    assert a.shape == (meta["A"],) and not calls
    tr.actor.eval()
    del tr.act_one
    a = tr.actor.act(z["states"][0], "cuda")
    assert np.max(np.abs(a - z["actions_eval"][0])) <= 2e-6 * meta["max_action"]


def test_packed_sample_views_equal_contiguous_batches_bitwise():
    """ReplayBuffer.sample returns five views of one packed block (consumed in place by the step); the same rows
    as five contiguous tensors (gather_split), and as oddly strided views, must give bitwise the same step."""
    import torch
    import iql
    from hip_helpers import build_hip_trainer, read_params
    S, A, N, B = 17, 6, 4096, 256
    data = synth.synth_transitions(N, S, A, seed=21)
    buf = iql.ReplayBuffer(S, A, N, "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in data.items()})
    params = synth.synth_params(S, A, seed=22)
    trs = [build_hip_trainer(params, S, A, True, _HYPER, _LRS, 1000) for _ in range(3)]
    np.random.seed(5)
    for k in range(3):
        idx = buf.sample_indices(B)
        views = buf.gather(idx)
        assert [tuple(v.shape) for v in views] == [(B, S), (B, A), (B, 1), (B, S), (B, 1)]
        assert views[0].stride(0) == buf._ld and views[0].data_ptr() + 4 * S == views[1].data_ptr()
        split = buf.gather_split(idx)
        for v, c in zip(views, split):
            assert c.is_contiguous() and torch.equal(v, c)
        wide = [torch.zeros((B, t.shape[1] + 3), device="cuda") for t in split]      # arbitrary row strides
        for w, c in zip(wide, split):
            w[:, : c.shape[1]] = c
        strided = [w[:, : c.shape[1]] for w, c in zip(wide, split)]
        logs = [trs[0].train(views), trs[1].train(split), trs[2].train(strided)]
        assert logs[0] == logs[1] == logs[2]
    p0, p1, p2 = (read_params(t) for t in trs)
    for net in p0:
        for t in p0[net]:
            assert np.array_equal(p0[net][t], p1[net][t]) and np.array_equal(p0[net][t], p2[net][t]), (net, t)


def test_full_size_buffer_graph_equals_eager_and_reaches_the_last_row():
    """BASELINE configs[1] geometry (1 M rows x 176 B): the device index draw covers the whole buffer (the last
    row included over a few chunks' worth of draws), the packed gather reads the right rows at the far end, and
    graph steps equal eager steps on the same indices — size-independent properties checked at full size."""
    import iql
    import iqlhip_binding as hb
    from hip_helpers import build_hip_trainer, read_params
    S, A, N, B, K = 17, 6, 1_000_000, 256, 5
    data = synth.synth_transitions(N, S, A, seed=0)
    buf = iql.ReplayBuffer(S, A, N, "cuda")
    buf.load_d4rl_dataset(data)
    # gather at the extremes against the host arrays
    idx_np = np.array([0, 1, N - 1, N - 2, N // 2, N - 1], dtype=np.int64)
    got = buf.gather(torch.from_numpy(idx_np).cuda())
    for t, key in zip(got, ("observations", "actions", "rewards", "next_observations", "terminals")):
        want = data[key][idx_np].reshape(len(idx_np), -1)
        assert np.array_equal(t.cpu().numpy(), want), key
    # device draw: bounds and coverage of both ends
    n = 1 << 22
    idx = torch.empty(n, dtype=torch.int64, device="cuda")
    hb.check(hb.lib().iqlhip_draw_indices(idx.data_ptr(), n, N, 5, 0, torch.cuda.current_stream().cuda_stream))
    assert int(idx.min()) == 0 and int(idx.max()) == N - 1
    # graph == eager on the same index stream
    params = synth.synth_params(S, A, seed=3)
    g = build_hip_trainer(params, S, A, True, _HYPER, _LRS, 1000)
    e = build_hip_trainer(params, S, A, True, _HYPER, _LRS, 1000)
    losses = g.train_steps(buf, K, B, seed=11)
    kidx = torch.empty(K * B, dtype=torch.int64, device="cuda")
    hb.check(hb.lib().iqlhip_draw_indices(kidx.data_ptr(), K * B, N, 11, 0, torch.cuda.current_stream().cuda_stream))
    for k in range(K):
        log = e.train(buf.gather(kidx[k * B:(k + 1) * B]))
        assert [log["value_loss"], log["q_loss"], log["actor_loss"]] == [float(x) for x in losses[k]]
    pa, pb = read_params(g), read_params(e)
    for net in pa:
        for t in pa[net]:
            assert np.array_equal(pa[net][t], pb[net][t]), (net, t)


def test_online_loop_body_runs_on_the_device_and_keeps_ring_semantics():
    """The reference's online iteration (iql.py:725-778; configs[2] dims) against a numpy stand-in env: act ->
    env.step -> add_transition -> sample -> train.  The ring wraps, samples only see written rows, every loss is
    finite and the rows the buffer holds are the rows that were added."""
    import iql
    sys_path_tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gpu_online_loop", os.path.join(sys_path_tools, "gpu_online_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    S, A, ring = 29, 8, 300
    qf, vf, actor = iql.TwinQ(S, A).cuda(), iql.ValueFunction(S).cuda(), iql.DeterministicPolicy(S, A, 1.0).cuda()
    tr = iql.ImplicitQLearning(1.0, actor, torch.optim.Adam(actor.parameters(), lr=3e-4), qf,
                               torch.optim.Adam(qf.parameters(), lr=3e-4), vf, torch.optim.Adam(vf.parameters(), lr=3e-4),
                               iql_tau=0.9, beta=10.0, max_steps=None, device="cuda")
    buf = iql.ReplayBuffer(S, A, ring, "cuda")
    env = mod.ToyEnv(S, A, seed=4)
    state = env.reset()
    added = []
    np.random.seed(2)
    for it in range(450):                           # 1.5 x the ring: the pointer wraps
        a = actor.act(state, "cuda")
        assert a.shape == (A,) and np.all(np.abs(a) <= 1.0)
        ns, r, d, _ = env.step(a)
        buf.add_transition(state, a, r, ns, d)
        added.append((state.copy(), a.copy(), np.float32(r), ns.copy(), np.float32(d)))
        if it >= 40:
            log = tr.train([b.to("cuda") for b in buf.sample(64)])
            assert all(np.isfinite(v) for v in log.values())
        state = env.reset() if d else ns
    assert buf._size == ring and buf._pointer == 450 % ring and tr.total_it == 410
    rows = buf._rows.cpu().numpy()
    for i in (0, 149, 150, ring - 1):               # row i holds the LAST transition written there
        k = i + ring if i < 450 - ring else i
        s_, a_, r_, ns_, d_ = added[k]
        want = np.concatenate([s_, a_, ns_, [r_, d_]])
        assert np.array_equal(rows[i, : 2 * S + A + 2], want), i


def test_thousand_step_run_tracks_the_cpu_port_statistically():
    """BASELINE configs[0] flavour (offline loop, halfcheetah dims, batch 256, 1 k steps) on synthetic data: beyond
    ~50 steps two fp32 trajectories diverge chaotically even for the reference against itself, so the
    library's 1 000-step run (device indices, hipGraph chunks) is compared with the PyTorch-CPU port of the reference
    step (numpy indices) on the statistics of the loss curves: window means of all three losses within 10 %."""
    import iql
    from hip_helpers import build_hip_trainer
    from oracle.iql_torch_port import CpuIQL
    S, A, N, B, K = 17, 6, 20000, 256, 1000
    data = synth.synth_transitions(N, S, A, seed=31)
    params = synth.synth_params(S, A, seed=32, perturb_target=False)
    buf = iql.OfflineReplayBuffer(S, A, N, "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in data.items()})
    tr = build_hip_trainer(params, S, A, True, _HYPER, _LRS, K)
    got = tr.train_steps(buf, K, B, seed=3)                       # [K, 3]
    torch.set_num_threads(4)
    cpu = CpuIQL(S, A, params, gaussian=True, max_steps=K)
    rng = np.random.default_rng(3)
    want = np.zeros((K, 3))
    for k in range(K):
        idx = rng.integers(0, N, size=B)
        tb = [torch.from_numpy(data["observations"][idx]), torch.from_numpy(data["actions"][idx]),
              torch.from_numpy(data["rewards"][idx][:, None]), torch.from_numpy(data["next_observations"][idx]),
              torch.from_numpy(data["terminals"][idx][:, None])]
        log = cpu.train(tb)
        want[k] = [log["value_loss"], log["q_loss"], log["actor_loss"]]
    assert np.all(np.isfinite(got))
    for lo, hi in ((0, 100), (400, 600), (800, 1000)):
        g, w = got[lo:hi].mean(0), want[lo:hi].mean(0)
        assert np.all(np.abs(g - w) <= 0.10 * np.abs(w) + 1e-3), (lo, hi, g, w)
