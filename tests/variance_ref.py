"""numpy restatement of one variance-learner step (include/iqlhip.h "the JSRL variance learner"): forward
of mf and vf, the reverse recurrence of the sampled values, torch's gaussian_nll_loss, the closed-form backward and
torch.optim.Adam — in float32 (every operation rounded as the reference rounds it) or in float64 (the yardstick the
fixtures' own error is measured against).  Also what the fixtures, the generator and the tests share: the synthetic
parameters, the sub-sampling of W1-shaped tensors, the error measures and the bound rule."""
import numpy as np

KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")
GAMMA = 0.99
CLIP_LO, CLIP_HI = 1e-4, 1e8
LR, BETAS, EPS = 1e-4, (0.9, 0.999), 1e-8
# W1-shaped tensors (256 x 256) are stored in the fixtures as these 32 rows: two per block of 16, every residue mod 8
W1_ROWS = np.array([8 * i + (i % 8) for i in range(32)])
# the project's fp32 bounds (tests/test_hip_parity.py)
PROJECT = {"forward": 1e-5, "loss": 1e-5, "grad": 1e-5, "param": 2e-6, "moment": 1e-5}


def synth_net(S, seed, scale=1.0, bias_shift=0.0):
    """A scalar net's parameters from a seed: torch's default Linear ranges (uniform +-1/sqrt(fan_in)), float32."""
    r = np.random.RandomState(seed)
    u = lambda shape, fan: r.uniform(-1.0, 1.0, size=shape).astype(np.float32) * np.float32(1.0 / np.sqrt(fan))
    P = {"w0": u((256, S), S), "b0": u((256,), S), "w1": u((256, 256), 256), "b1": u((256,), 256),
         "w2": u((1, 256), 256) * np.float32(scale), "b2": u((1,), 256) * np.float32(scale) + np.float32(bias_shift)}
    return P


def sub(key, a):
    return a[W1_ROWS] if key == "w1" else a


def forward(P, x, dt):
    h0 = np.maximum(x.astype(dt) @ P["w0"].astype(dt).T + P["b0"].astype(dt), 0)
    h1 = np.maximum(h0 @ P["w1"].astype(dt).T + P["b1"].astype(dt), 0)
    return (h1 @ P["w2"].astype(dt).T + P["b2"].astype(dt))[:, 0], h0, h1


def backward(P, x, h0, h1, dy, dt):
    """Gradients of sum_t dy[t] out[t] for out = the net's head over the rows x."""
    dy = dy.astype(dt)[:, None]
    g = {"w2": dy.T @ h1, "b2": dy.sum(0)}
    d1 = (dy @ P["w2"].astype(dt)) * (h1 > 0)
    g["w1"], g["b1"] = d1.T @ h0, d1.sum(0)
    d0 = (d1 @ P["w1"].astype(dt)) * (h0 > 0)
    g["w0"], g["b0"] = d0.T @ x.astype(dt), d0.sum(0)
    return g


def values(mf, vf, obs, next_last, rewards, next_dones, dt, aligned=False):
    B = obs.shape[0]
    rows = np.concatenate([obs, next_last[None]], 0)
    pm, h0m, h1m = forward(mf, rows, dt)
    s, h0v, h1v = forward(vf, obs, dt)
    e = np.exp(s)
    lo, hi = dt(CLIP_LO), dt(CLIP_HI)
    var = np.clip(e, lo, hi)
    nnt = dt(1.0) - next_dones.astype(dt)
    rew = rewards.astype(dt) if aligned else np.roll(rewards.astype(dt), 1)       # rewards[t - 1]; row 0: rewards[B - 1]
    gamma = dt(GAMMA)
    samp = np.zeros(B, dt)
    nxt = pm[B]
    for t in range(B - 1, -1, -1):
        samp[t] = rew[t] + (gamma * nxt) * nnt[t]
        nxt = samp[t]
    return dict(samp=samp, pred=pm[:B], var=var, e=e, open=(e >= lo) & (e <= hi), nnt=nnt, rows=rows,
                act_m=(h0m, h1m), act_v=(h0v, h1v))


def step(mf, vf, obs, next_last, rewards, next_dones, which, dt=np.float32, aligned=False, t_adam=1, m=None, v=None):
    """One _update_v: returns samp, pred, var, loss, grads of net `which` (0 mf, 1 vf), its params / m / v afterwards."""
    B = obs.shape[0]
    f = values(mf, vf, obs, next_last, rewards, next_dones, dt, aligned)
    d = f["pred"] - f["samp"]
    q = d * d / f["var"]
    loss = (dt(0.5) * (np.log(f["var"]) + q)).sum() / dt(B)
    if which == 0:
        gp = d / f["var"] / dt(B)
        G = np.zeros(B, dt)
        G[0] = -gp[0]
        for t in range(1, B):
            G[t] = -gp[t] + (dt(GAMMA) * f["nnt"][t - 1]) * G[t - 1]
        dy = np.concatenate([gp, [(dt(GAMMA) * f["nnt"][B - 1]) * G[B - 1]]])
        P, grads = mf, backward(mf, f["rows"], *f["act_m"], dy, dt)
    else:
        dy = np.where(f["open"], dt(0.5) * (dt(1.0) - q), dt(0.0)) / dt(B)
        P, grads = vf, backward(vf, obs, *f["act_v"], dy, dt)
    b1, b2 = BETAS
    out = dict(samp=f["samp"], pred=f["pred"], var=f["var"], e=f["e"], loss=loss, grads=grads, params={}, m={}, v={})
    for k in KEYS:
        g = grads[k].reshape(P[k].shape).astype(dt)
        grads[k] = g
        m0 = np.zeros_like(g) if m is None else m[k].astype(dt)
        v0 = np.zeros_like(g) if v is None else v[k].astype(dt)
        mk = m0 + dt(1.0 - b1) * (g - m0)
        vk = v0 * dt(b2) + dt(1.0 - b2) * g * g
        denom = np.sqrt(vk) / dt((1.0 - b2 ** t_adam) ** 0.5) + dt(EPS)
        out["params"][k] = P[k].astype(dt) - dt(LR / (1.0 - b1 ** t_adam)) * (mk / denom)
        out["m"][k], out["v"][k] = mk, vk
    return out


# ---------------------------------------------------------------- error measures and the bound rule
def rel(a, b):
    """max |a - b| over max |b|: a tensor-relative error."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def absmax(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


MEASURE = {"forward": rel, "loss": rel, "grad": rel, "param": absmax, "moment": rel}


def deviations(got, want, full_w1=False):
    """Per quantity class the largest error of `got` (a step() result or a fixture's arrays in the same form) against
    `want`: {"forward", "loss", "grad", "param", "moment"}.  W1-shaped tensors are compared on W1_ROWS (the rows a fixture
    stores), or whole with full_w1 (generated cases: both sides hold all 256 rows)."""
    dev = {"forward": max(rel(got[k], want[k]) for k in ("samp", "pred", "var")), "loss": rel(got["loss"], want["loss"])}
    pick = lambda d, k: sub(k, d[k]) if d[k].shape == (256, 256) and not full_w1 else d[k]
    dev["grad"] = max(rel(pick(got["grads"], k), pick(want["grads"], k)) for k in KEYS)
    dev["param"] = max(absmax(pick(got["params"], k), pick(want["params"], k)) for k in KEYS)
    dev["moment"] = max(rel(pick(got[mv], k), pick(want[mv], k)) for mv in ("m", "v") for k in KEYS)
    return dev


def bounds(ref_dev):
    """The larger of the project's fp32 bound and four times the reference's own deviation from float64."""
    return {k: max(PROJECT[k], 4.0 * float(ref_dev[k])) for k in PROJECT}


def checksum(P):
    return float(sum(np.asarray(P[k], np.float64).sum() for k in KEYS))


def load_step(path):
    """A g17_var_step / _clip / _boot fixture: (z, mf, vf, want) — the npz, both nets' parameters regenerated from the
    stored seeds (checked against the stored checksums), and the reference's results in step()'s form."""
    z = np.load(path)
    S, seed = int(z["S"]), int(z["seed"])
    mf, vf = synth_net(S, 2 * seed + 1), synth_net(S, 2 * seed + 2, float(z["vf_scale"]), float(z["vf_shift"]))
    assert checksum(mf) == float(z["checksum_mf"]) and checksum(vf) == float(z["checksum_vf"]), "synth_net changed"
    want = dict(samp=z["samp"], pred=z["pred"], var=z["var"], loss=z["loss"])
    for grp in ("grads", "params", "m", "v"):
        want[grp] = {k: z[f"{grp}_{k}"] for k in KEYS}
    return z, mf, vf, want


# ---------------------------------------------------------------- a deterministic fake environment (fixtures and tests)
class _Space:
    def __init__(self, n):
        self.n, self.rng = n, np.random.RandomState(0)

    def seed(self, s):
        self.rng = np.random.RandomState(s)

    def sample(self):
        return self.rng.uniform(-1.0, 1.0, size=self.n).astype(np.float32)


class _Spec:
    def __init__(self, name):
        self.name = name


class FakeEnv:
    """S-dimensional linear dynamics, old gym API (seed(), reset() -> state, step() -> 4-tuple).  Episodes end after
    `horizon` steps, or early when the first state coordinate exceeds `goal` (a terminal, not a time-out)."""

    def __init__(self, S=5, A=2, horizon=7, goal=0.45, name="FakeEnv"):
        self.S, self.A, self.horizon, self.goal = S, A, horizon, goal
        self.action_space = _Space(A)
        self.spec = _Spec(name)
        self.unwrapped = self
        self._rng = np.random.RandomState(0)
        self._M = np.random.RandomState(99).uniform(-0.3, 0.3, size=(A, S)).astype(np.float32)
        self._t, self._s = 0, np.zeros(S, np.float32)

    def seed(self, s):
        self._rng = np.random.RandomState(s)

    def reset(self):
        self._t = 0
        self._s = self._rng.uniform(-1.0, 1.0, size=self.S).astype(np.float32)
        return self._s.copy()

    def step(self, action):
        a = np.asarray(action, np.float32).reshape(-1)
        self._s = (np.float32(0.9) * self._s + a @ self._M).astype(np.float32)
        self._t += 1
        reward = float(self._s[0] - 0.1 * np.abs(a).sum())
        done = bool(self._t >= self.horizon or self._s[0] > self.goal)
        return self._s.copy(), reward, done, {}


def fake_actor(env, state):
    return np.tanh(np.asarray(state, np.float32)[:env.A] * np.float32(2.0))
