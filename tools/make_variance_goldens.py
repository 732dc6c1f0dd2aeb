"""Record the variance-learner fixtures (tests/golden/g17_*) from the reference's variance_learner.py:

    python tools/make_variance_goldens.py /path/to/reference/algorithms/finetune/variance_learner.py

The reference module is imported by path with `gym` (and matplotlib, where absent) stubbed and this repository's `iql` on
the path; it runs on the CPU.  Inputs are synthetic and seeded (tests/variance_ref.py: synth_net, FakeEnv).  Next to the
reference's results every fixture stores `refdev_*`: the reference's own fp32 deviation from the float64 restatement,
per quantity class — the tests' bounds are max(project bound, 4 x that) (variance_ref.bounds).  W1-shaped tensors are
stored on variance_ref.W1_ROWS only; parameters are regenerated from their seeds (a float64 checksum is stored)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "jsrl-corl_amd"), os.path.join(ROOT, "tests")]
import variance_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_reference(path):
    for name in ("gym", "matplotlib", "matplotlib.pyplot"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["gym"], "Env"):
        sys.modules["gym"].Env = object
    if "matplotlib.pyplot" in sys.modules and not hasattr(sys.modules["matplotlib"], "pyplot"):
        sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    spec = importlib.util.spec_from_file_location("reference_variance_learner", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def set_params(module, P):
    sd = {f"v.net.{2 * i}.{n}": torch.from_numpy(P[f"{k}{i}"].copy()) for i in range(3) for n, k in (("weight", "w"), ("bias", "b"))}
    module.load_state_dict(sd)


def get_params(module):
    sd = module.state_dict()
    return {f"{k}{i}": sd[f"v.net.{2 * i}.{n}"].detach().numpy().copy() for i in range(3) for n, k in (("weight", "w"), ("bias", "b"))}


def done_pattern(kind, B, rng):
    nd = np.zeros(B, bool)
    if kind == "all":
        nd[:] = True
    elif kind == "first":
        nd[0] = True
    elif kind == "last":
        nd[B - 1] = True
    elif kind == "pair":
        nd[B // 2] = True
        nd[min(B // 2 + 1, B - 1)] = True
    elif kind == "random":
        nd = rng.uniform(size=B) < 0.05
    return nd


def rollout(S, B, seed, kind):
    rng = np.random.RandomState(seed)
    obs = rng.standard_normal((B, S)).astype(np.float32)
    last = rng.standard_normal(S).astype(np.float32)
    rewards = rng.uniform(-1.0, 1.0, size=B).astype(np.float32)
    return obs, last, rewards, done_pattern(kind, B, rng)


def as_batch(obs, last, rewards, nd):
    B = obs.shape[0]
    nxt = [torch.zeros(obs.shape[1]) for _ in range(B - 1)] + [torch.from_numpy(last.copy())]
    return ([torch.from_numpy(o.copy()) for o in obs], [None] * B, [float(r) for r in rewards], [False] * B, nxt,
            [bool(d) for d in nd])


def reference_step(ref, learner, batch, which):
    """get_values and one _update_v of the reference: the result in variance_ref.step's form."""
    with torch.no_grad():
        samp, pred, var = learner.get_values(batch[0], batch[2], batch[4], batch[3], batch[5])
    log = learner._update_v(batch, update_vf=bool(which))
    net, opt = (learner.vf, learner.mv_optimizer) if which else (learner.mf, learner.m_optimizer)
    names = {f"{k}{i}": f"v.net.{2 * i}.{n}" for i in range(3) for n, k in (("weight", "w"), ("bias", "b"))}
    ps = dict(net.named_parameters())
    out = dict(samp=samp.numpy().copy(), pred=pred.numpy().copy(), var=var.numpy().copy(), loss=np.float32(log["value_loss"]),
               grads={}, params={}, m={}, v={})
    for k, n in names.items():
        p = ps[n]
        out["grads"][k] = p.grad.detach().numpy().copy()
        out["params"][k] = p.detach().numpy().copy()
        out["m"][k] = opt.state[p]["exp_avg"].numpy().copy()
        out["v"][k] = opt.state[p]["exp_avg_sq"].numpy().copy()
    return out


def flatten(res, prefix=""):
    arrays = {prefix + k: np.asarray(res[k]) for k in ("samp", "pred", "var", "loss")}
    for grp in ("grads", "params", "m", "v"):
        for k in R.KEYS:
            arrays[f"{prefix}{grp}_{k}"] = R.sub(k, res[grp][k])
    return arrays


def make_step(ref, name, S, B, which, kind, seed, vf_scale=1.0, vf_shift=0.0, check=None):
    mfP, vfP = R.synth_net(S, 2 * seed + 1), R.synth_net(S, 2 * seed + 2, vf_scale, vf_shift)
    obs, last, rewards, nd = rollout(S, B, seed, kind)
    learner = ref.VarianceLearner(S, 1, None, None)
    set_params(learner.mf, mfP)
    set_params(learner.vf, vfP)
    got = reference_step(ref, learner, as_batch(obs, last, rewards, nd), which)
    f64 = R.step(mfP, vfP, obs, last, rewards, nd, which, np.float64)
    f32 = R.step(mfP, vfP, obs, last, rewards, nd, which, np.float32)
    if check:
        check(f64)
    dev = R.deviations(got, f64)
    print(f"{name}: S={S} B={B} net={which} dones={kind} loss={float(got['loss']):.6g}  reference vs float64: "
          + " ".join(f"{k}={v:.2e}" for k, v in dev.items())
          + "  fp32 restatement vs reference: " + " ".join(f"{k}={v:.2e}" for k, v in R.deviations(f32, got).items()))
    arrays = flatten(got)
    arrays.update(obs=obs, next_last=last, rewards=rewards, next_dones=nd, which=np.int32(which), S=np.int32(S),
                  seed=np.int32(seed), vf_scale=np.float32(vf_scale), vf_shift=np.float32(vf_shift),
                  checksum_mf=np.float64(R.checksum(mfP)), checksum_vf=np.float64(R.checksum(vfP)),
                  e64=f64["e"], **{"refdev_" + k: np.float64(v) for k, v in dev.items()})
    np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), **arrays)


def check_clip(f64):
    e = f64["e"]
    lo, hi = (e < R.CLIP_LO).sum(), (e > R.CLIP_HI).sum()
    assert lo > 0 and hi > 0 and lo + hi < e.size, (lo, hi, e.size)
    near = np.minimum(np.abs(e / R.CLIP_LO - 1.0), np.abs(e / R.CLIP_HI - 1.0))
    assert near.min() > 1e-3, f"a row's exp(s) lies within 1e-3 of a clip bound ({near.min():.2e})"


def make_freerun(ref, name="g17_var_freerun", S=17, B=100, seed=70):
    mfP, vfP = R.synth_net(S, 2 * seed + 1), R.synth_net(S, 2 * seed + 2)
    learner = ref.VarianceLearner(S, 1, None, None)
    set_params(learner.mf, mfP)
    set_params(learner.vf, vfP)
    P64 = [{k: v.astype(np.float64) for k, v in mfP.items()}, {k: v.astype(np.float64) for k, v in vfP.items()}]
    M64, V64, T = [None, None], [None, None], [0, 0]
    arrays, losses, losses64 = {}, [], []
    for n in range(10):
        which = int(n >= 5)
        obs, last, rewards, nd = rollout(S, B, 1000 + n, "random")
        log = learner._update_v(as_batch(obs, last, rewards, nd), update_vf=bool(which))
        losses.append(log["value_loss"])
        T[which] += 1
        r = R.step(P64[0], P64[1], obs, last, rewards, nd, which, np.float64, t_adam=T[which], m=M64[which], v=V64[which])
        P64[which], M64[which], V64[which] = r["params"], r["m"], r["v"]
        losses64.append(float(r["loss"]))
        arrays.update({f"obs{n}": obs, f"next_last{n}": last, f"rewards{n}": rewards, f"next_dones{n}": nd})
    final = [get_params(learner.mf), get_params(learner.vf)]
    dev_loss = max(R.rel(a, b) for a, b in zip(losses, losses64))
    dev_param = max(R.absmax(final[i][k], P64[i][k]) for i in range(2) for k in R.KEYS)
    print(f"{name}: losses {losses}  reference vs float64: loss={dev_loss:.2e} param={dev_param:.2e}")
    for i, tag in enumerate(("mf", "vf")):
        for k in R.KEYS:
            arrays[f"final_{tag}_{k}"] = R.sub(k, final[i][k])
    arrays.update(losses=np.asarray(losses, np.float32), S=np.int32(S), seed=np.int32(seed),
                  checksum_mf=np.float64(R.checksum(mfP)), checksum_vf=np.float64(R.checksum(vfP)),
                  refdev_loss=np.float64(dev_loss), refdev_param=np.float64(dev_param))
    np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), **arrays)


# (name, seeds, with actor, batch_size, random_frac, np.random seed)
EPISODE_SCENARIOS = (("a", 3, False, 20, 0, 11), ("b", 0, True, 20, 0, 12), ("c", 5, True, 33, 0.5, 13),
                     ("d", [0, 1, 2], True, None, 0.5, 14), ("e", [1, 2, 3], False, None, 0, 15), ("f", [0, 1], True, 5, 0, 16))


def make_run_episodes(ref, name="g17_run_episodes"):
    arrays = {}
    for tag, seeds, with_actor, batch_size, frac, np_seed in EPISODE_SCENARIOS:
        np.random.seed(np_seed)
        env = R.FakeEnv()
        s, a, r, d, ns, nd = ref.run_episodes(env, env.horizon, seeds, R.fake_actor if with_actor else None, batch_size, frac)
        st = np.random.get_state()
        arrays.update({f"{tag}_states": torch.stack(s).numpy(), f"{tag}_actions": np.stack(a).astype(np.float32),
                       f"{tag}_rewards": np.asarray(r, np.float64), f"{tag}_dones": np.asarray(d, bool),
                       f"{tag}_next_states": torch.stack(ns).numpy(), f"{tag}_next_dones": np.asarray(nd, bool),
                       f"{tag}_rng_keys": st[1], f"{tag}_rng_pos": np.int64(st[2])})
        print(f"{name}/{tag}: {len(s)} rows, {int(np.sum(nd))} terminals")
    np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), **arrays)


# the single-update fixtures: (S, B) and a next_dones pattern each; both phases of every one
STEP_CASES = ((17, 256, "random"), (17, 257, "none"), (29, 33, "pair"), (3, 1, "none"), (17, 2, "first"), (17, 32, "last"),
              (17, 1024, "random"), (17, 32, "all"))


def main():
    ref = load_reference(sys.argv[1])
    torch.manual_seed(0)
    for i, (S, B, kind) in enumerate(STEP_CASES):
        for which in (0, 1):
            make_step(ref, f"g17_var_step_S{S}_B{B}_{kind}_{'vf' if which else 'mf'}", S, B, which, kind, 10 + i)
    for which in (0, 1):
        make_step(ref, f"g17_var_clip_{'vf' if which else 'mf'}", 17, 64, which, "random", 40, vf_scale=300.0, vf_shift=4.0, check=check_clip)
        make_step(ref, f"g17_var_boot_{'vf' if which else 'mf'}", 17, 4, which, "none", 50)
    make_freerun(ref)
    make_run_episodes(ref)


if __name__ == "__main__":
    main()
