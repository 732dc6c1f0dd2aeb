"""GPU tests of the variance learner (iqlhip_var_*, jsrl-corl_amd/iqlhip_variance.py) against the fixtures
recorded from the reference (g17_var_*): get_values, the loss, the flat gradient, then the step — parameters and moments of
the stepped net, the other net bit for bit untouched.  Bounds per quantity and fixture: the larger of the project's fp32
bound and four times the reference's own fp32 deviation from float64, stored in the fixture (variance_ref.bounds) — never
anything the device computed.  With IQLHIP_VARIANCE_MARGINS set to a file name, each comparison appends its margins there
(profiles/variance_parity_margins.txt)."""
import glob
import os

import numpy as np
import pytest
import torch

import synth
import variance_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STEP_FIXTURES = sorted(os.path.basename(p)[:-4] for pat in ("g17_var_step_*", "g17_var_clip_*", "g17_var_boot_*")
                       for p in glob.glob(os.path.join(GOLDEN, pat + ".npz")))
_NAMES = {f"{k}{i}": f"v.net.{2 * i}.{n}" for i in range(3) for n, k in (("weight", "w"), ("bias", "b"))}


def _note(name, dev, bound):
    line = f"{name}: " + "  ".join(f"{k} {dev[k]:.2e} (bound {bound[k]:.2e})" for k in dev)
    print(line)
    out = os.environ.get("IQLHIP_VARIANCE_MARGINS")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _learner(S, mf, vf, aligned=False, batch_size=256):
    import variance_learner as VL
    L = VL.VarianceLearner(S, 1, None, None, batch_size=batch_size, device="cuda", aligned_rewards=aligned)
    for net, P in ((L.mf, mf), (L.vf, vf)):
        net.load_state_dict({n: torch.from_numpy(P[k].copy()) for k, n in _NAMES.items()})
    return L


def _batch(obs, last, rewards, nd):
    B = obs.shape[0]
    nxt = [np.zeros(obs.shape[1], np.float32)] * (B - 1) + [last]
    return ([torch.from_numpy(o.copy()) for o in obs], [None] * B, [float(r) for r in rewards], [False] * B, nxt,
            [bool(d) for d in nd])


def _net_state(L, k):
    """{params, m, v} of net k as numpy dicts keyed like the restatement's, read from the arenas."""
    out = {"params": {}, "m": {}, "v": {}}
    net = (L.mf, L.vf)[k]
    shapes = {key: tuple(p.shape) for key, p in zip(("w0", "b0", "w1", "b1", "w2", "b2"), net.parameters())}
    for grp, arena in (("params", L._params_arena), ("m", L._m_arena), ("v", L._v_arena)):
        a = arena.cpu().numpy()
        for key, shape in shapes.items():
            off = int(getattr(L._layout[k], key))
            out[grp][key] = a[off: off + int(np.prod(shape))].reshape(shape).copy()
    return out


def _segment_bytes(L, k):
    lo, hi = int(L._layout[k].seg_begin), int(L._layout[k].seg_end)
    return [a[lo:hi].cpu().numpy().view(np.uint32).copy() for a in (L._params_arena, L._m_arena, L._v_arena)]


@pytest.mark.parametrize("name", STEP_FIXTURES)
def test_step_fixture(name):
    z, mf, vf, want = R.load_step(os.path.join(GOLDEN, name + ".npz"))
    which, S = int(z["which"]), int(z["S"])
    bound = R.bounds({k: z["refdev_" + k] for k in R.PROJECT})
    L = _learner(S, mf, vf)
    batch = _batch(z["obs"], z["next_last"], z["rewards"], z["next_dones"])
    samp, pred, var = L.get_values(batch[0], batch[2], batch[4], batch[3], batch[5])
    got = dict(samp=samp.numpy(), pred=pred.numpy(), var=var.numpy())
    if "_clip_" in name:      # the fixture's condition: no row within 1e-3 of a clip bound, so the gate bits are the reference's
        e = z["e64"]
        assert np.minimum(np.abs(e / R.CLIP_LO - 1.0), np.abs(e / R.CLIP_HI - 1.0)).min() > 1e-3
        assert np.array_equal(got["var"] == np.float32(R.CLIP_LO), z["var"] == np.float32(R.CLIP_LO))
        assert np.array_equal(got["var"] == np.float32(R.CLIP_HI), z["var"] == np.float32(R.CLIP_HI))
    loss_fb, flat = L.flat_gradient(batch, bool(which))
    got["grads"] = {k: v.numpy() for k, v in L.net_gradients(flat, bool(which)).items()}
    other_before = _segment_bytes(L, 1 - which)
    log = L._update_v(batch, bool(which))
    assert log["value_loss"] == loss_fb          # the step's forward is the forward_backward's
    got["loss"] = np.float32(log["value_loss"])
    got.update(_net_state(L, which))
    dev = R.deviations(got, want)
    _note(name, dev, bound)
    for k in dev:
        assert dev[k] <= bound[k], (k, dev[k], bound[k])
    n5 = min(5, samp.shape[0])
    assert set(log) == {"variance_pred_vec", "value_loss", "values_pred_vec", "values_samp_vec"}
    assert torch.equal(log["values_samp_vec"], samp[:n5]) and torch.equal(log["values_pred_vec"], pred[:n5])
    assert torch.equal(log["variance_pred_vec"], var[:n5]) and log["values_samp_vec"].device.type == "cpu"
    for a, b in zip(other_before, _segment_bytes(L, 1 - which)):
        assert np.array_equal(a, b), "the other net's parameters or moments changed"
    opt = (L.m_optimizer, L.mv_optimizer)[which]
    assert all(float(st["step"]) == 1.0 for st in opt.state.values()) and len(opt.state) == 6


def _free_run(L, z):
    losses = []
    for n in range(10):
        b = _batch(z[f"obs{n}"], z[f"next_last{n}"], z[f"rewards{n}"], z[f"next_dones{n}"])
        losses.append(L._update_v(b, n >= 5)["value_loss"])
    return losses


def test_free_run():
    z = np.load(os.path.join(GOLDEN, "g17_var_freerun.npz"))
    S, seed = int(z["S"]), int(z["seed"])
    L = _learner(S, R.synth_net(S, 2 * seed + 1), R.synth_net(S, 2 * seed + 2))
    losses = _free_run(L, z)
    dev = {"loss": max(R.rel(a, b) for a, b in zip(losses, z["losses"])), "param": 0.0}
    bound = {"loss": max(R.PROJECT["loss"], 4 * float(z["refdev_loss"])), "param": max(R.PROJECT["param"], 4 * float(z["refdev_param"]))}
    for i, tag in enumerate(("mf", "vf")):
        st = _net_state(L, i)["params"]
        dev["param"] = max([dev["param"]] + [R.absmax(R.sub(k, st[k]), z[f"final_{tag}_{k}"]) for k in R.KEYS])
    _note("g17_var_freerun", dev, bound)
    assert dev["loss"] <= bound["loss"] and dev["param"] <= bound["param"], (dev, bound)
    assert L._adam_t == [5, 5]


def test_two_learners_end_bit_identical():
    z = np.load(os.path.join(GOLDEN, "g17_var_freerun.npz"))
    S, seed = int(z["S"]), int(z["seed"])
    runs = []
    for _ in range(2):
        L = _learner(S, R.synth_net(S, 2 * seed + 1), R.synth_net(S, 2 * seed + 2))
        losses = _free_run(L, z)
        runs.append((losses, _segment_bytes(L, 0), _segment_bytes(L, 1)))
    assert runs[0][0] == runs[1][0]
    for k in (1, 2):
        for a, b in zip(runs[0][k], runs[1][k]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("S,B,which", [(17, 33, 0), (17, 33, 1), (3, 1, 0), (29, 257, 0)])
def test_aligned_rewards_against_the_restatement(S, B, which):
    """aligned_rewards=1 (rewards[t]; the reference has no such mode): against the fp32 restatement, bounded by the
    project's bounds or four times the fp32 restatement's own deviation from the float64 one."""
    mf, vf = R.synth_net(S, 301), R.synth_net(S, 302)
    rng = np.random.RandomState(303 + B)
    obs, last = rng.standard_normal((B, S)).astype(np.float32), rng.standard_normal(S).astype(np.float32)
    rewards, nd = rng.uniform(-1, 1, size=B).astype(np.float32), rng.uniform(size=B) < 0.1
    want = R.step(mf, vf, obs, last, rewards, nd, which, np.float32, aligned=True)
    bound = R.bounds(R.deviations(want, R.step(mf, vf, obs, last, rewards, nd, which, np.float64, aligned=True)))
    L = _learner(S, mf, vf, aligned=True)
    batch = _batch(obs, last, rewards, nd)
    samp, pred, var = L.get_values(batch[0], batch[2], batch[4], batch[3], batch[5])
    _, flat = L.flat_gradient(batch, bool(which))
    got = dict(samp=samp.numpy(), pred=pred.numpy(), var=var.numpy(),
               grads={k: v.numpy() for k, v in L.net_gradients(flat, bool(which)).items()})
    got["loss"] = np.float32(L._update_v(batch, bool(which))["value_loss"])
    got.update(_net_state(L, which))
    dev = R.deviations(got, want)
    _note(f"aligned_S{S}_B{B}_net{which}", dev, bound)
    for k in dev:
        assert dev[k] <= bound[k], (k, dev[k], bound[k])
    if B > 1:      # ... and the mode matters: the reference's alignment gives other sampled values
        plain = R.values(mf, vf, obs, last, rewards, nd, np.float32)["samp"]
        assert R.rel(plain, want["samp"]) > 1e-3


def test_run_training_equals_the_manual_loop_and_feeds_the_gate(tmp_path):
    import iql
    import variance_learner as VL
    from hip_helpers import build_hip_trainer
    cfg = type("Cfg", (), {"device": "cuda", "variance_learn_frac": 0.5})()
    S, A, n_updates, bs = 5, 2, 6, 16

    def fresh():
        torch.manual_seed(7)
        np.random.seed(8)
        return VL.VarianceLearner(S, A, cfg, R.fake_actor, batch_size=bs), R.FakeEnv()

    saved = np.random.get_state()
    try:
        L1, env1 = fresh()
        vf = L1.run_training(env1, env1.horizon, R.fake_actor, n_updates=n_updates, save_dir=str(tmp_path))
        L2, env2 = fresh()
        for n in range(n_updates):
            batch = VL.run_episodes(env2, env2.horizon, n, R.fake_actor, batch_size=bs, random_frac=0.5)
            L2._update_v(batch, update_vf=(n > n_updates / 2))
    finally:
        np.random.set_state(saved)
    assert vf is L1.vf and not vf.training and not hasattr(L1, "mf")
    assert L1._adam_t == L2._adam_t == [4, 2]
    for a, b in zip((L1._params_arena, L1._m_arena, L1._v_arena), (L2._params_arena, L2._m_arena, L2._v_arena)):
        assert torch.equal(a, b)
    stem = tmp_path / "FakeEnv_guide_6_0-5"
    sd = torch.load(str(stem) + "_vf.pt")
    assert os.path.exists(str(stem) + "_mf.pt") and all(v.device.type == "cpu" for v in sd.values())
    f = VL.StateDepFunction(S)
    f.load_state_dict(sd)
    assert all(torch.equal(a, b.cpu()) for a, b in zip(f.state_dict().values(), vf.state_dict().values()))
    # the saved file as a device gate, and the learner's own gate(): the horizon is the trained vf's value
    x = np.random.RandomState(9).standard_normal((33, S)).astype(np.float32)
    with torch.no_grad():
        want = f(torch.from_numpy(x)).numpy()
    hyper = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    learner = build_hip_trainer(synth.synth_params(S, A, seed=1), S, A, True, hyper, lrs, 1000)
    guide = build_hip_trainer(synth.synth_params(S, A, seed=2), S, A, True, hyper, lrs, 1000)
    for gate in (iql.load_gate(sd, action_dim=A), L1.gate()):
        acts, use, h = iql.JsrlActors(learner, guide, gate).act([x], [2], gate_max=[0.0])[0]
        assert acts.shape == (33, A) and R.rel(h, want) <= R.PROJECT["forward"], R.rel(h, want)
        assert np.array_equal(use, (h <= 0.0).astype(np.int32))


def test_learner_and_trainer_do_not_disturb_each_other():
    from hip_helpers import build_hip_trainer, to_torch_batch
    S, A, B = 17, 6, 64
    hyper = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005, "deterministic": False}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    data = synth.synth_transitions(B, S, A, seed=21)
    tb = to_torch_batch({"s": data["observations"], "a": data["actions"], "r": data["rewards"],
                         "ns": data["next_observations"], "d": data["terminals"]}, "cuda:0")
    z = np.load(os.path.join(GOLDEN, "g17_var_step_S17_B32_last_mf.npz"))
    vb = _batch(z["obs"], z["next_last"], z["rewards"], z["next_dones"])

    def run(with_learner):
        tr = build_hip_trainer(synth.synth_params(S, A, seed=20), S, A, True, hyper, lrs, 1000, device="cuda:0")
        L = _learner(S, R.synth_net(S, 1), R.synth_net(S, 2)) if with_learner else None
        logs = [tr.train(tb)]
        vlog = L._update_v(vb, False)["value_loss"] if L is not None else None
        logs.append(tr.train(tb))
        torch.cuda.synchronize()
        arenas = [a.cpu().numpy().view(np.uint32).copy() for a in (tr._params_arena, tr._target_arena, tr._m_arena, tr._v_arena)]
        return logs, arenas, vlog

    a, b = run(True), run(False)
    assert a[0] == b[0]
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y)
    # ... and the learner's step next to a trainer is its step alone
    alone = _learner(S, R.synth_net(S, 1), R.synth_net(S, 2))._update_v(vb, False)["value_loss"]
    assert a[2] == alone
