"""CPU tests of the variance learner: the numpy restatement (tests/variance_ref.py) reproduces every
reference-recorded fixture g17_var_* within the fixture's own bound; run_episodes reproduces g17_run_episodes including
the np.random state it leaves; the drop-in surface, the packed block, the host's Adam scalars and the C ABI's checks."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

import iqlhip_binding as hb
import variance_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STEP_FIXTURES = sorted(os.path.basename(p)[:-4] for pat in ("g17_var_step_*", "g17_var_clip_*", "g17_var_boot_*")
                       for p in glob.glob(os.path.join(GOLDEN, pat + ".npz")))
SYMBOLS = ("iqlhip_var_layout", "iqlhip_var_create", "iqlhip_var_destroy", "iqlhip_var_bind", "iqlhip_var_step",
           "iqlhip_var_values", "iqlhip_var_forward_backward", "iqlhip_var_read_loss")


def test_fixture_list_covers_the_shapes_and_done_patterns():
    assert len(STEP_FIXTURES) == 20
    shapes = {tuple(map(int, re.match(r"g17_var_step_S(\d+)_B(\d+)_", n).groups())) for n in STEP_FIXTURES if "_step_" in n}
    assert shapes == {(17, 256), (17, 257), (29, 33), (3, 1), (17, 2), (17, 32), (17, 1024)}
    kinds = {n.split("_")[5] for n in STEP_FIXTURES if "_step_" in n}
    assert kinds == {"none", "all", "first", "last", "pair", "random"}


@pytest.mark.parametrize("name", STEP_FIXTURES)
def test_restatement_reproduces_fixture(name):
    z, mf, vf, want = R.load_step(os.path.join(GOLDEN, name + ".npz"))
    got = R.step(mf, vf, z["obs"], z["next_last"], z["rewards"], z["next_dones"], int(z["which"]), np.float32)
    dev = R.deviations(got, want)
    bound = R.bounds({k: z["refdev_" + k] for k in R.PROJECT})
    print(name, {k: f"{dev[k]:.2e} / {bound[k]:.2e}" for k in dev})
    for k in dev:
        assert dev[k] <= bound[k], (k, dev[k], bound[k])


@pytest.mark.parametrize("name", [n for n in STEP_FIXTURES if "_clip_" in n])
def test_clip_fixture_keeps_its_distance_from_the_bounds(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    e = z["e64"]
    lo, hi = int((e < R.CLIP_LO).sum()), int((e > R.CLIP_HI).sum())
    assert lo > 0 and hi > 0 and lo + hi < e.size
    assert np.minimum(np.abs(e / R.CLIP_LO - 1.0), np.abs(e / R.CLIP_HI - 1.0)).min() > 1e-3
    assert (z["var"] == np.float32(R.CLIP_LO)).sum() == lo and (z["var"] == np.float32(R.CLIP_HI)).sum() == hi


def test_boot_fixture_fails_without_the_bootstrap_gradient():
    """B = 4 without dones: the bootstrap row's output gradient is about 0.96 of a row's; a backward that drops it (a
    detached bootstrap value) misses the gradient bound by orders of magnitude."""
    z, mf, vf, want = R.load_step(os.path.join(GOLDEN, "g17_var_boot_mf.npz"))
    f = R.values(mf, vf, z["obs"], z["next_last"], z["rewards"], z["next_dones"], np.float32)
    gp = (f["pred"] - f["samp"]) / f["var"] / np.float32(4)
    dropped = R.backward(mf, f["rows"], *f["act_m"], np.concatenate([gp, [np.float32(0)]]), np.float32)
    bound = R.bounds({k: z["refdev_" + k] for k in R.PROJECT})["grad"]
    worst = max(R.rel(R.sub(k, dropped[k].reshape(mf[k].shape)), want["grads"][k]) for k in R.KEYS)
    assert worst > 1000 * bound, (worst, bound)


def test_freerun_fixture_restated():
    z = np.load(os.path.join(GOLDEN, "g17_var_freerun.npz"))
    S, seed = int(z["S"]), int(z["seed"])
    P = [R.synth_net(S, 2 * seed + 1), R.synth_net(S, 2 * seed + 2)]
    M, V, T = [None, None], [None, None], [0, 0]
    losses = []
    for n in range(10):
        which = int(n >= 5)
        T[which] += 1
        r = R.step(P[0], P[1], z[f"obs{n}"], z[f"next_last{n}"], z[f"rewards{n}"], z[f"next_dones{n}"], which, np.float32,
                   t_adam=T[which], m=M[which], v=V[which])
        P[which], M[which], V[which] = r["params"], r["m"], r["v"]
        losses.append(float(r["loss"]))
    assert max(R.rel(a, b) for a, b in zip(losses, z["losses"])) <= max(R.PROJECT["loss"], 4 * float(z["refdev_loss"]))
    bound = max(R.PROJECT["param"], 4 * float(z["refdev_param"]))
    for i, tag in enumerate(("mf", "vf")):
        for k in R.KEYS:
            assert R.absmax(R.sub(k, P[i][k]), z[f"final_{tag}_{k}"]) <= bound, (tag, k)


# (name, seeds, with actor, batch_size, random_frac, np.random seed): tools/make_variance_goldens.py EPISODE_SCENARIOS
EPISODE_SCENARIOS = (("a", 3, False, 20, 0, 11), ("b", 0, True, 20, 0, 12), ("c", 5, True, 33, 0.5, 13),
                     ("d", [0, 1, 2], True, None, 0.5, 14), ("e", [1, 2, 3], False, None, 0, 15), ("f", [0, 1], True, 5, 0, 16))


@pytest.mark.parametrize("tag,seeds,with_actor,batch_size,frac,np_seed", EPISODE_SCENARIOS)
def test_run_episodes_reproduces_the_reference(tag, seeds, with_actor, batch_size, frac, np_seed):
    import variance_learner as VL
    z = np.load(os.path.join(GOLDEN, "g17_run_episodes.npz"))
    saved = np.random.get_state()
    try:
        np.random.seed(np_seed)
        env = R.FakeEnv()
        s, a, r, d, ns, nd = VL.run_episodes(env, env.horizon, seeds, R.fake_actor if with_actor else None, batch_size, frac)
        st = np.random.get_state()
    finally:
        np.random.set_state(saved)
    assert all(t.dtype == torch.float32 for t in s + ns)
    assert np.array_equal(torch.stack(s).numpy(), z[f"{tag}_states"])
    assert np.array_equal(np.stack(a).astype(np.float32), z[f"{tag}_actions"])
    assert np.array_equal(np.asarray(r, np.float64), z[f"{tag}_rewards"])
    assert np.array_equal(np.asarray(d, bool), z[f"{tag}_dones"]) and np.array_equal(np.asarray(nd, bool), z[f"{tag}_next_dones"])
    assert np.array_equal(torch.stack(ns).numpy(), z[f"{tag}_next_states"])
    assert np.array_equal(st[1], z[f"{tag}_rng_keys"]) and st[2] == int(z[f"{tag}_rng_pos"])
    if batch_size is not None:
        assert len(s) == batch_size


def test_run_episodes_antmaze_reward_shift():
    import variance_learner as VL
    plain, ant = R.FakeEnv(), R.FakeEnv(name="antmaze-fake")
    r0 = VL.run_episodes(plain, plain.horizon, 2, None, 6)[2]
    r1 = VL.run_episodes(ant, ant.horizon, 2, None, 6)[2]
    assert [x - 1 for x in r0] == r1


# ---------------------------------------------------------------- the drop-in surface
def test_drop_in_module_exports():
    import variance_learner as VL
    for name in ("StateDepFunction", "VarianceLearner", "run_episodes", "nll_loss", "mse_loss", "to_tensor", "GAMMA"):
        assert hasattr(VL, name), name
    assert VL.GAMMA == 0.99
    assert VL.to_tensor(np.arange(3)).dtype == torch.float32
    p, t, v = torch.tensor([1.0, 2.0]), torch.tensor([0.5, 2.5]), torch.tensor([0.3, 2.0])
    assert torch.equal(VL.nll_loss(p, t, v), torch.nn.functional.gaussian_nll_loss(p, t, v))
    assert torch.equal(VL.mse_loss(p, t), 0.5 * ((p - t) ** 2).mean())


def test_state_dep_function_keys_and_files(tmp_path):
    import variance_learner as VL
    f = VL.StateDepFunction(17)
    assert hasattr(f, "v")
    assert list(f.state_dict()) == [f"v.net.{i}.{n}" for i in (0, 2, 4) for n in ("weight", "bias")]
    assert f(torch.zeros(17)).shape == () and f(torch.zeros(5, 17)).shape == (5,)
    torch.save(f.state_dict(), tmp_path / "x_vf.pt")
    g = VL.StateDepFunction(17)
    g.load_state_dict(torch.load(tmp_path / "x_vf.pt"))
    assert all(torch.equal(a, b) for a, b in zip(f.state_dict().values(), g.state_dict().values()))


def test_learner_attributes_and_refusals_on_a_cpu_device():
    import variance_learner as VL
    cfg = type("Cfg", (), {"device": "cpu", "variance_learn_frac": 0.5})()
    L = VL.VarianceLearner(17, 6, cfg, None)          # device from config.device
    assert L.device == "cpu" and L.batch_size == 256 and L.aligned_rewards is False
    for name in ("mf", "vf", "m_optimizer", "mv_optimizer"):
        assert hasattr(L, name)
    assert L.m_optimizer.param_groups[0]["lr"] == 1e-4 and L.mv_optimizer.param_groups[0]["lr"] == 1e-4
    batch = ([np.zeros(17)] * 3, [None] * 3, [0.0] * 3, [False] * 3, [np.zeros(17)] * 3, [False] * 3)
    with pytest.raises(RuntimeError, match="GPU"):
        L._update_v(batch, False)
    with pytest.raises(RuntimeError, match="GPU"):
        L.get_values(batch[0], batch[2], batch[4], batch[3], batch[5])
    L.m_optimizer.param_groups[0]["weight_decay"] = 0.1
    with pytest.raises(NotImplementedError):
        L._update_v(batch, False)
    L.mv_optimizer.param_groups[0]["amsgrad"] = True
    with pytest.raises(NotImplementedError):
        L._update_v(batch, True)
    with pytest.raises(ValueError):
        VL.VarianceLearner(17, 6, cfg, None, batch_size=1025)
    with pytest.raises(ValueError):
        VL.VarianceLearner(17, 6, cfg, None, batch_size=0)


def test_packed_block_layout_and_refusals():
    from iqlhip_variance import pack_block
    S, B = 3, 4
    obs = [torch.arange(S, dtype=torch.float32) + 10 * t for t in range(B)]
    nxt = [np.full(S, -1.0)] * (B - 1) + [np.array([7.0, 8.0, 9.0])]
    blk, n = pack_block(S, obs, [0.5, 1.5, 2.5, 3.5], nxt, [False, True, False, True])
    assert n == B and blk.dtype == np.float32 and blk.shape == (B * S + S + 2 * B,)
    assert np.array_equal(blk[:B * S].reshape(B, S), torch.stack(obs).numpy())
    assert np.array_equal(blk[B * S:(B + 1) * S], [7.0, 8.0, 9.0])          # of the next states only the last
    assert np.array_equal(blk[(B + 1) * S:(B + 1) * S + B], [0.5, 1.5, 2.5, 3.5])
    assert np.array_equal(blk[(B + 1) * S + B:], [0.0, 1.0, 0.0, 1.0])
    blk2, _ = pack_block(S, torch.stack(obs).numpy(), np.array([0.5, 1.5, 2.5, 3.5]), np.stack(nxt), np.array([0, 1, 0, 1], bool))
    assert np.array_equal(blk, blk2)
    with pytest.raises(ValueError):
        pack_block(S, obs, [0.5] * 3, nxt, [False] * B)
    with pytest.raises(ValueError):
        pack_block(S + 1, obs, [0.5] * B, nxt, [False] * B)
    with pytest.raises(ValueError):
        pack_block(S, np.zeros((1025, S)), [0.0] * 1025, np.zeros((1025, S)), [False] * 1025)
    with pytest.raises(ValueError):
        pack_block(S, obs, [0.5] * B, nxt[:2], [False] * B)


def test_host_adam_scalars_are_float64_values():
    from iqlhip_variance import adam_scalars
    for t in (1, 2, 1000, 100000):
        sc = adam_scalars(1e-4, (0.9, 0.999), 1e-8, t, aligned_rewards=(t == 2))
        assert sc.step_size == np.float32(1e-4 / (1.0 - 0.9 ** t)) and sc.bc2_sqrt == np.float32((1.0 - 0.999 ** t) ** 0.5)
        assert sc.beta2 == np.float32(0.999) and sc.one_minus_beta1 == np.float32(1.0 - 0.9)
        assert sc.one_minus_beta2 == np.float32(1.0 - 0.999) and sc.eps == np.float32(1e-8)
        assert sc.aligned_rewards == int(t == 2)


# ---------------------------------------------------------------- the C ABI
def test_symbols_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    bound = {name: args for name, _, args in hb.SYMBOLS}
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in bound and hasattr(hb.lib(), name), name
    assert C.sizeof(hb.VarScalars) == 32


def test_layout_is_the_value_nets_rule_twice():
    for S in (3, 17, 29, 127):
        L, n = hb.var_layout(S)
        v = hb.arena_layout(S, 1, False).net[hb.NET_V]
        seg = v.seg_end - v.seg_begin
        assert n == 2 * seg and seg % 64 == 0
        for k in range(2):
            assert (L[k].k_in, L[k].d_out, L[k].log_std) == (S, 1, -1)
            assert L[k].seg_begin == k * seg and L[k].seg_end == (k + 1) * seg
            for key in ("w0", "b0", "w1", "b1", "w2", "b2"):
                assert getattr(L[k], key) - L[k].seg_begin == getattr(v, key) - v.seg_begin


def test_arguments_are_checked_before_any_device_work():
    lib = hb.lib()
    h = C.c_void_p()
    assert lib.iqlhip_var_create(0, 256, 0, C.byref(h)) == hb.E_INVAL
    assert lib.iqlhip_var_create(128, 256, 0, C.byref(h)) == hb.E_UNSUPPORTED
    assert lib.iqlhip_var_create(17, 0, 0, C.byref(h)) == hb.E_INVAL
    assert lib.iqlhip_var_create(17, 1025, 0, C.byref(h)) == hb.E_INVAL
    assert lib.iqlhip_var_create(17, 256, 0, None) == hb.E_INVAL
    assert h.value is None
    with pytest.raises(ValueError):
        hb.var_layout(0)
    with pytest.raises(NotImplementedError):
        hb.var_layout(128)
    sc = hb.VarScalars()
    assert lib.iqlhip_var_step(None, None, 4, 0, C.byref(sc), None) == hb.E_INVAL
    assert lib.iqlhip_var_bind(None, None, None, None) == hb.E_INVAL
    assert lib.iqlhip_var_destroy(None) == 0
