"""Generated cases for the variance learner's step at every state width and at trained-like values (DESIGN.md 6l
"Widths, row counts and trained-like values"): numpy only, no torch, no GPU.  tests/test_variance_cases_cpu.py checks
that every case is what it claims to be; tests/test_hip_variance_shapes.py runs them on the device against the float64
restatement (tests/variance_ref.py).

A case is two trained-like nets and a rollout whose rows are CLEAN: no ReLU mask and no clip bit of the step depends on
the order of a summation, so a mask that differs between the device and float64 is a device error."""
import functools

import numpy as np

import variance_ref as R

N_DEAD, N_ZERO = 40, 8
S_INF = 89.5                  # expf overflows above 88.73: a row with s > S_INF has e = inf in float32
S_HI_MAX = 88.0               # ... and a finite high-clipped row stays clear of that
ROUNDS = 20
KINDS = ("open", "mixed", "closed")
LO, HI, OPEN, INF, ANY = 0, 1, 2, 3, -1
TARGETS = {"open": (OPEN,), "mixed": (LO, HI, OPEN, INF), "closed": (LO, HI, INF)}


def trained_net(S, seed, kind):
    """(parameters, index sets) of a scalar net made trained-like from variance_ref.synth_net(S, seed).  kind: "mf", or
    for vf "open" / "mixed" / "closed".  w0 x 3, w1 x 2; N_DEAD units of each hidden layer with bias -50 (dead on every
    row); N_ZERO layer-0 units with a zero weight row and a zero bias (pre-activation exactly 0 in any precision); N_ZERO
    head weights exactly 0.  mf: w2 x 20, b2 + 30.  vf: the head rescaled so that s has a standard deviation of 3
    ("open") or 8 (the others) around 4.6, the middle of the open range (ln 1e-4, ln 1e8), over standard-normal rows;
    "mixed" and "closed" also give one live unit (the spike) a head weight that lifts s beyond S_INF on many of the
    rows where it is active."""
    assert kind in ("mf",) + KINDS
    P = R.synth_net(S, seed)
    r = np.random.RandomState(seed + 7919)
    p0, p1 = r.permutation(256), r.permutation(256)
    sets = {"dead0": np.sort(p0[:N_DEAD]), "zero0": np.sort(p0[N_DEAD:N_DEAD + N_ZERO]),
            "dead1": np.sort(p1[:N_DEAD]), "w2zero": np.sort(p1[N_DEAD:N_DEAD + N_ZERO]), "spike": int(p1[N_DEAD + N_ZERO])}
    P["w0"] = P["w0"] * np.float32(3)
    P["w1"] = P["w1"] * np.float32(2)
    P["b0"][sets["dead0"]] = np.float32(-50)
    P["b1"][sets["dead1"]] = np.float32(-50)
    P["w0"][sets["zero0"]] = 0
    P["b0"][sets["zero0"]] = 0
    P["w2"][0, sets["w2zero"]] = 0
    if kind == "mf":
        P["w2"] = P["w2"] * np.float32(20)
        P["b2"] = P["b2"] + np.float32(30)
        return P, sets
    # the head from a calibration sample: the base output a u + c puts u's 10 % / 90 % quantiles one unit outside the
    # open range, and the spike is the first live unit that leaves every class the kind wants reachable
    x = r.standard_normal((2048, S)).astype(np.float32)
    _, z1, _ = preacts(P, x, np.float64)
    h1 = np.maximum(z1, 0)
    u = h1 @ P["w2"].astype(np.float64)[0]
    if kind == "open":
        a = 3.0 / float(u.std())
        c = 4.6 - a * float(u.mean())
    else:
        q10, q90 = np.quantile(u, [0.1, 0.9])
        a = (np.log(R.CLIP_HI) - np.log(R.CLIP_LO) + 2.0) / float(q90 - q10)
        c = np.log(R.CLIP_LO) - 1.0 - a * float(q10)
    P["w2"] = (P["w2"] * a).astype(np.float32)
    P["b2"] = np.array([c], np.float32)
    if kind != "open":
        for cand in p1[N_DEAD + N_ZERO:]:
            live = h1[:, cand]
            if not 0.1 <= (live > 0).mean() <= 0.6:
                continue
            w2 = P["w2"].copy()
            w2[0, cand] = np.float32(110.0 / float(live[live > 0].mean()))
            cls = classify(h1 @ w2.astype(np.float64)[0] + float(P["b2"][0]), z1[:, cand])
            if all((cls == t).mean() >= 0.02 for t in TARGETS[kind]):
                P["w2"], sets["spike"] = w2, int(cand)
                break
        else:
            raise AssertionError(f"no spike unit leaves every class reachable (S {S}, seed {seed}, {kind})")
    return P, sets


def preacts(P, x, dt):
    """Pre-activations of both hidden layers and the head output, with variance_ref.forward's operations in dt."""
    z0 = x.astype(dt) @ P["w0"].astype(dt).T + P["b0"].astype(dt)
    z1 = np.maximum(z0, 0) @ P["w1"].astype(dt).T + P["b1"].astype(dt)
    s = (np.maximum(z1, 0) @ P["w2"].astype(dt).T + P["b2"].astype(dt))[:, 0]
    return z0, z1, s


def clip_distance(s64):
    """Relative distance of e = exp(s) from the nearer clip bound, in float64."""
    with np.errstate(over="ignore"):
        e = np.exp(np.asarray(s64, np.float64))
    return np.minimum(np.abs(e / R.CLIP_LO - 1.0), np.abs(e / R.CLIP_HI - 1.0))


def classify(s64, spike64):
    """Per row LO / HI / OPEN / INF, or ANY for a row no target accepts: within 1e-3 of a clip bound, between
    S_HI_MAX and S_INF, or open with the spike unit active (its head weight would amplify the activation's rounding)."""
    s64 = np.asarray(s64, np.float64)
    cls = np.full(s64.shape, ANY)
    cls[s64 < np.log(R.CLIP_LO)] = LO
    cls[(s64 > np.log(R.CLIP_HI)) & (s64 < S_HI_MAX)] = HI
    cls[s64 > S_INF] = INF
    cls[(s64 > np.log(R.CLIP_LO)) & (s64 < np.log(R.CLIP_HI)) & (spike64 <= 0)] = OPEN
    cls[clip_distance(s64) <= 1e-3] = ANY
    return cls


def _free(sets, layer):
    keep = np.ones(256, bool)
    keep[sets["dead0" if layer == 0 else "dead1"]] = False
    if layer == 0:
        keep[sets["zero0"]] = False
    return keep


def dirty_rows(nets32, nets64, sets, rows, B, targets):
    """(bad [B + 1] bool, tau [2]): the rows that are not clean under the nets given — mf over all B + 1 rows, vf over
    the first B.  tau[l] = 16 x the largest |float32 - float64| pre-activation of layer l over both nets and all rows;
    a row is bad with a non-constructed pre-activation within tau of zero (in either precision), a constructed dead
    unit that is not dead, a ReLU mask the two precisions disagree on, or a vf output outside its target class."""
    bad = np.zeros(B + 1, bool)
    pre = []
    for k, x in ((0, rows), (1, rows[:B])):
        z32, z64 = preacts(nets32[k], x, np.float32), preacts(nets64[k], x, np.float64)
        pre.append((z32, z64, x.shape[0]))
    tau = [16.0 * max(float(np.abs(z32[l] - z64[l]).max()) for z32, z64, _ in pre) for l in (0, 1)]
    for k, (z32, z64, n) in enumerate(pre):
        for l in (0, 1):
            free = _free(sets[k], l)
            near = (np.abs(z64[l][:, free]) <= tau[l]) | (np.abs(z32[l][:, free].astype(np.float64)) <= tau[l])
            bad[:n] |= near.any(1) | ((z32[l] > 0) != (z64[l] > 0)).any(1)
            dead = sets[k]["dead0" if l == 0 else "dead1"]
            bad[:n] |= (z64[l][:, dead] > -1.0).any(1) | (z32[l][:, dead] > -1.0).any(1)
    s32, s64 = pre[1][0][2], pre[1][1][2]
    cls = classify(s64, pre[1][1][1][:, sets[1]["spike"]])
    bad[:B] |= cls != targets
    with np.errstate(over="ignore"):
        e32 = np.exp(s32)
    lo, hi = np.float32(R.CLIP_LO), np.float32(R.CLIP_HI)
    bad[:B] |= ((e32 >= lo) & (e32 <= hi)) != (cls == OPEN)
    return bad, tau


def make_case(S, B, seed, kind, aligned=False, dones="random", nets32=None, nets64=None, rows_seed=None):
    """A clean case: dict(mf, vf, sets, obs [B][S], last [S], rewards [B] (uniform, scale 10), nd [B] bool (dones:
    "random" p = 0.1, "none", "all"), aligned, rounds, tau, targets).  Row t of vf is made to fall into class
    TARGETS[kind][t % len] (an INF row only from B >= 4 on).  The cleaning: dirty rows are redrawn from a pool of
    standard-normal rows whose float64 vf output is in the row's class, for at most ROUNDS rounds.  nets32 / nets64
    ((mf, vf) each) replace the generated nets on the float32 and the float64 side: a chain's evolved parameters, with
    rows_seed (default: seed) another rollout for the same nets."""
    assert kind in KINDS and dones in ("random", "none", "all")
    mf, sets_m = trained_net(S, 2 * seed + 1, "mf")
    vf, sets_v = trained_net(S, 2 * seed + 2, kind)
    n32 = (mf, vf) if nets32 is None else nets32
    n64 = (mf, vf) if nets64 is None else nets64
    sets = (sets_m, sets_v)
    r = np.random.RandomState((seed if rows_seed is None else rows_seed) + 104729 * B + 31 * S)
    tg = TARGETS[kind]
    targets = np.array([tg[t % len(tg)] for t in range(B)])
    if B < 4 and kind == "mixed":
        targets = np.array([LO, HI, OPEN][:B])
    draw = lambda n: r.standard_normal((n, S)).astype(np.float32)
    rows = draw(B + 1)
    bad = np.ones(B + 1, bool)
    rounds, tau = 0, [0.0, 0.0]
    while True:
        # redraw: rows of the wanted class from a pool, in the pool's order (row B, the bootstrap row, takes any)
        todo, pools = list(np.flatnonzero(bad)), 0
        while todo:
            pools += 1
            assert pools <= 400, f"no row of class {targets[todo[0]]} in {pools} pools (S {S}, seed {seed}, {kind})"
            pool = draw(max(64, 8 * len(todo)))
            _, z1, s = preacts(n64[1], pool, np.float64)
            cls = classify(s, z1[:, sets_v["spike"]])
            used = np.zeros(len(pool), bool)
            left = []
            for t in todo:
                ok = ~used if t == B else (~used & (cls == targets[t]))
                i = int(np.argmax(ok))
                if ok[i]:
                    rows[t], used[i] = pool[i], True
                else:
                    left.append(t)
            todo = left
        bad, tau = dirty_rows(n32, n64, sets, rows, B, targets)
        if not bad.any():
            break
        rounds += 1
        assert rounds <= ROUNDS, f"the cleaning did not end in {ROUNDS} rounds (S {S}, B {B}, seed {seed}, {kind})"
    rewards = (r.uniform(-1.0, 1.0, size=B) * 10.0).astype(np.float32)
    nd = {"random": r.uniform(size=B) < 0.1, "none": np.zeros(B, bool), "all": np.ones(B, bool)}[dones]
    return dict(mf=mf, vf=vf, sets=sets, obs=rows[:B].copy(), last=rows[B].copy(), rewards=rewards, nd=nd, aligned=aligned,
                rounds=rounds, tau=tau, targets=targets, S=S, B=B, kind=kind)


# ---------------------------------------------------------------- the cases of tests/test_hip_variance_shapes.py
WIDTHS = (1, 2, 4, 15, 16, 31, 32, 33, 63, 64, 65, 126, 127)          # every S % 4, both sides of score_l0's 32-column
ROW_COUNTS = (3, 15, 16, 31, 63, 1023, 1024)                           # trip, njt = 1, 2, 4, 5, 8, the bias column alone
ROW_WIDTHS = (64, 127)                                                 # in a tile and as a tile's last lane
# id -> (S, B, seed, kind, aligned, dones)
CASES = {f"S{S}_B31_mixed": (S, 31, 1000 + S, "mixed", False, "random") for S in WIDTHS}
CASES.update({f"S{S}_B{B}_mixed": (S, B, 1000 + S, "mixed", False, "random") for S in ROW_WIDTHS for B in ROW_COUNTS})
CASES["S64_B63_mixed_aligned"] = (64, 63, 2064, "mixed", True, "random")
CASES["S16_B16_mixed_alldone"] = (16, 16, 2016, "mixed", False, "all")
CASES["S16_B16_mixed_nodone"] = (16, 16, 2016, "mixed", False, "none")
CLOSED = {"S17_B33_closed": (17, 33, 3017, "closed", False, "random"), "S64_B256_closed": (64, 256, 3064, "closed", False, "random")}
CASES.update(CLOSED)
CHAIN = dict(S=65, B=63, seed=4065, kind="mixed", which=(0, 0, 0, 1, 1, 1))


@functools.lru_cache(maxsize=None)
def case(name):
    S, B, seed, kind, aligned, dones = CASES[name]
    return make_case(S, B, seed, kind, aligned, dones)


@functools.lru_cache(maxsize=None)
def reference(name, which):
    """(float32 step, float64 step, bounds) of net `which` on a case: computed once, shared, left unchanged."""
    c = case(name)
    with np.errstate(over="ignore"):
        s32, s64 = (R.step(c["mf"], c["vf"], c["obs"], c["last"], c["rewards"], c["nd"], which, dt, aligned=c["aligned"])
                    for dt in (np.float32, np.float64))
    return s32, s64, R.bounds(R.deviations(s32, s64, full_w1=True))


@functools.lru_cache(maxsize=None)
def chain():
    """The chain's six steps: [(case, float32 step, float64 step)] — step k's case is clean under the parameters the
    two restatements hold after k steps (float32 chain on one side, float64 chain on the other), and both chains carry
    t_adam, m and v of the stepped net."""
    out = []
    P = {dt: None for dt in (np.float32, np.float64)}
    M = {dt: [None, None] for dt in P}
    V = {dt: [None, None] for dt in P}
    T = [0, 0]
    for k, which in enumerate(CHAIN["which"]):
        c = make_case(CHAIN["S"], CHAIN["B"], CHAIN["seed"], CHAIN["kind"], nets32=P[np.float32], nets64=P[np.float64],
                      rows_seed=CHAIN["seed"] + 100 * k)
        T[which] += 1
        steps = {}
        for dt in P:
            if P[dt] is None:
                P[dt] = (c["mf"], c["vf"])
            with np.errstate(over="ignore"):
                st = R.step(P[dt][0], P[dt][1], c["obs"], c["last"], c["rewards"], c["nd"], which, dt, t_adam=T[which],
                            m=M[dt][which], v=V[dt][which])
            nets = list(P[dt])
            nets[which] = st["params"]
            P[dt], M[dt][which], V[dt][which] = tuple(nets), st["m"], st["v"]
            steps[dt] = st
        out.append((c, steps[np.float32], steps[np.float64]))
    return out
