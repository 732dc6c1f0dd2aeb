"""Trained-like inputs for the IQL step and wrong references to hold the tests against (not a test module).

synth.py draws nn.Linear-initialised weights, log_std = 0 and N(0, 1) rewards: at those values the advantage weight
never reaches its clamp, log_std never leaves [-20, 2] and tanh never saturates.  trained_like() edits such inputs in
place until every one of those branches fires for a share of the rows or dims, and mutants() yields the references a
kernel that got one of the branches wrong would agree with — built from oracle.iql_oracle's own functions, so that a
test can show its assertions tell the right reference from each wrong one (tests/test_value_edges_cpu.py) before it
holds the kernels to them (tests/test_hip_value_edges.py).  DESIGN.md section 2, "Value edges"."""
import collections
import contextlib
import math

import numpy as np

from oracle import iql_oracle as O

HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}

# The smallest shape that reaches each path.  lb (large-batch kernels), w0k (w0_lds_k) and bwd (the backward instantiation)
# are checked against tests/helpers.py's restatements of the host's dispatch rules.
Case = collections.namedtuple("Case", "name S A B gaussian precision lb w0k bwd")
CASES = [Case(*c) for c in [
    # fp32
    ("f32_S17A6_B40", 17, 6, 40, True, "f32", False, 23, "iql_bwd_kernel<BF16=0, FULL=0, MULTI=0>"),
    # Dp = 32, two ragged chunks (256 + 44 rows)
    ("f32_S39A28_B300", 39, 28, 300, True, "f32", False, 67, "iql_bwd_kernel<BF16=0, FULL=0, MULTI=0>"),
    # two head tiles, deterministic, one row past a row tile
    ("f32_S20A32_B33_det", 20, 32, 33, False, "f32", False, 52, "iql_bwd_kernel<BF16=0, FULL=0, MULTI=0>"),
    # 513 rows: 4 * (32 * 3 chunks + 4 * 17 row tiles) = 656 blocks > two rounds of 256 CUs, the smallest batch with
    # the multi-round backward (512 rows: 4 * (64 + 64) = 512, still one slice per block)
    ("f32_S17A6_B513_multi", 17, 6, 513, True, "f32", False, 23, "iql_bwd_kernel<BF16=0, FULL=0, MULTI=1>"),
    # bf16, small-batch kernels
    ("bf16_S39A28_B256", 39, 28, 256, True, "bf16", False, 67, "iql_bwd_kernel<BF16=1, FULL=1, MULTI=0>"),
    # S + A + 1 = 81: off the large-batch path at any batch size
    ("bf16_S52A28_B1024", 52, 28, 1024, True, "bf16", False, 80, "iql_bwd_kernel<BF16=1, FULL=1, MULTI=1>"),
    # bf16, large-batch kernels: NKB = 1 / 2 / 3 forward, the row kernel with and without its column split, SPREAD
    ("lb_S17A6_B513_det", 17, 6, 513, False, "bf16", True, 23, "iql_bwd_rows_kernel<CSPLIT=1> + iql_bwd_gemm_kernel"),
    ("lb_S29A8_B600", 29, 8, 600, True, "bf16", True, 37, "iql_bwd_rows_kernel<CSPLIT=1> + iql_bwd_gemm_kernel"),
    ("lb_S39A28_B1024", 39, 28, 1024, True, "bf16", True, 67, "iql_bwd_rows_kernel<CSPLIT=1> + iql_bwd_gemm_kernel"),
    ("lb_S39A28_B2080", 39, 28, 2080, True, "bf16", True, 67, "iql_bwd_rows_kernel<CSPLIT=0> + iql_bwd_gemm_kernel"),
]]
CASE_NAMES = [c.name for c in CASES]
CASE = {c.name: c for c in CASES}
FP32_CASE_NAMES = [c.name for c in CASES if c.precision == "f32"]

LOG_STD_CYCLE = (2.5, 2.0, 0.5, -20.0, -1.0, 3.0, 0.0)     # period 7: the classes shift against the kernels' groups of 8 dims
LOG_STD_BELOW = -25.0                                       # on ONE dim: 1 / var = exp(40) there swamps every other dim
PRE_SATURATED = 12.0                                        # |pre| from which 1 - tanh(pre)^2 < 2e-10
PI_W2_SCALE = 5.0                                          # (fp32 rounding of pre grows with it: test_value_edges_cpu (d))
PI_B2_CYCLE = (0.5, 14.0, -2.5, 1.0, -14.0)                 # period 5: two dims of five saturated for every row
QT_W2_SCALE = 12.0
# on every fifth row.  (Not what puts the bf16 critics' gradients near GRAD_RL2: at 10 they lie no lower — the bf16-rounded-
# operand oracle alone stands at 5e-2 .. 8e-2 either way, profiles/value_edges_margins.txt section 1.)
REWARD_SCALE = 50.0
CLAMPED_SHARE = 0.3
ALL_CLAMPED_SHIFTS = (60.0, 70.0)


def below_dim(A):
    return A - 2


def overflow_dims(A):
    """(dim with pre = +60 for every row, dim with pre = -60): exp(2 pre) overflows fp32 on one, underflows on the other."""
    return 0, A - 1 if LOG_STD_CYCLE[(A - 1) % 7] > -20.0 else A - 3


def log_std_values(A):
    ls = np.array([LOG_STD_CYCLE[d % len(LOG_STD_CYCLE)] for d in range(A)], dtype=np.float32)
    ls[below_dim(A)] = LOG_STD_BELOW
    return ls


def log_std_classes(ls):
    """{class: dims}.  at_max / at_min hold exactly 2.0 / -20.0: the clamp is inclusive, they are inside."""
    ls = np.asarray(ls, dtype=np.float64)
    mid = (ls > O.LOG_STD_MIN) & (ls < O.LOG_STD_MAX)
    return {"above": np.flatnonzero(ls > O.LOG_STD_MAX), "at_max": np.flatnonzero(ls == O.LOG_STD_MAX),
            "at_min": np.flatnonzero(ls == O.LOG_STD_MIN), "below": np.flatnonzero(ls < O.LOG_STD_MIN),
            "ordinary": np.flatnonzero(mid)}


def inside_dims(ls):
    ls = np.asarray(ls, dtype=np.float64)
    return (ls >= O.LOG_STD_MIN) & (ls <= O.LOG_STD_MAX)


def trained_like(params, data, meta):
    """Edits synthetic params ({net: {tensor: array}}) and rows (synth_transitions' dict) in place; meta: B, A, gaussian
    and, optionally, target_shift (added to the target critics' output bias: ALL_CLAMPED_SHIFTS put every row's weight
    on the clamp)."""
    B, A, gaussian = meta["B"], meta["A"], meta["gaussian"]
    f = np.float32
    # rows: every fourth terminal, every fifth reward REWARD_SCALE times larger, actions exactly on +-1, 16 rows twice
    rows = np.arange(B)
    data["terminals"][:] = (rows % 4 == 1).astype(f)
    data["rewards"][rows % 5 == 2] *= f(REWARD_SCALE)
    data["actions"][rows % 7 == 0, ::3] = f(1.0)
    data["actions"][rows % 7 == 3, 1::3] = f(-1.0)
    for k in data:
        data[k][B // 2: B // 2 + 16] = data[k][:16]
    # clamp straddle: rewards do not enter adv = min(tQ1, tQ2) - V(s), so the target critics' output layer is scaled
    # and shifted until beta * adv lies on both sides of log(EXP_ADV_MAX), as tests/test_hip_step_stats.py's CLAMP_CASE
    # does; where the advantages lie depends on the drawn weights, so the shift puts these rows' CLAMPED_SHARE quantile
    # on the clamp (both critics' biases move by the same amount, and with them min(tQ1, tQ2))
    for n in ("qt1", "qt2"):
        params[n]["w2"] = params[n]["w2"] * f(QT_W2_SCALE)
    d = np.float64
    s64 = data["observations"].astype(d)
    sa = O.q_input(s64, data["actions"].astype(d))
    tq = np.minimum(*(O.mlp_forward({k: v.astype(d) for k, v in params[n].items()}, sa)[0][:, 0] for n in ("qt1", "qt2")))
    adv = tq - O.mlp_forward({k: v.astype(d) for k, v in params["vf"].items()}, s64)[0][:, 0]
    shift = math.log(O.EXP_ADV_MAX) / meta.get("beta", HYPER["beta"]) - np.quantile(adv, 1.0 - CLAMPED_SHARE)
    for n in ("qt1", "qt2"):
        params[n]["b2"] = params[n]["b2"] + f(shift + meta.get("target_shift", 0.0))
    # saturated policy head: pre-activations of several units' size, the biases spread over the dims, and two dims where
    # exp(2 pre) leaves fp32's range for every row
    pi = params["pi"]
    pi["w2"] = pi["w2"] * f(PI_W2_SCALE)
    pi["b2"] = np.array([PI_B2_CYCLE[d % len(PI_B2_CYCLE)] for d in range(A)], dtype=f)
    hi, lo = overflow_dims(A)
    pi["w2"][hi] = 0.0
    pi["w2"][lo] = 0.0
    pi["b2"][hi], pi["b2"][lo] = f(60.0), f(-60.0)
    if gaussian:
        pi["log_std"] = log_std_values(A)


def case_inputs(name, target_shift=0.0):
    """(params, batch, hyper) of a case of CASES: synthetic inputs, then trained_like."""
    import synth
    c = CASE[name]
    S, A, B, gaussian = c.S, c.A, c.B, c.gaussian
    params = synth.synth_params(S, A, seed=300 + 3 * S + A, gaussian=gaussian)
    data = synth.synth_transitions(B, S, A, seed=400 + S + A + B)
    trained_like(params, data, {"B": B, "A": A, "gaussian": gaussian, "target_shift": target_shift})
    batch = {"s": data["observations"], "a": data["actions"], "r": data["rewards"], "ns": data["next_observations"],
             "d": data["terminals"]}
    hyper = dict(HYPER)
    hyper["deterministic"] = not gaussian
    return params, batch, hyper


def with_other_next_states(batch):
    """The batch with the next state of every terminal row replaced by another row's (finite) state: (1 - d) = 0
    multiplies V(s') there, nothing else reads it."""
    out = {k: v.copy() for k, v in batch.items()}
    term = np.flatnonzero(batch["d"] > 0)
    out["ns"][term] = 3.0 * batch["s"][(term + 1) % batch["s"].shape[0]] - 1.0
    return out


def pre_activations(params, batch):
    f = np.float64
    return O.mlp_forward({k: v.astype(f) for k, v in params["pi"].items() if k != "log_std"}, batch["s"].astype(f))[0]


# ---------------------------------------------------------------------------------------------------------- mutants
@contextlib.contextmanager
def _patched(**consts):
    """Oracle constants replaced for the duration, then put back."""
    old = {k: getattr(O, k) for k in consts}
    for k, v in consts.items():
        setattr(O, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(O, k, v)


def _base(params, batch, hyper, c):
    """The float64 oracle, or tests/loss_weights_ref.py's row-weighted restatement of it when row weights c are given."""
    if c is None:
        return O.iql_losses_and_grads(params, batch, hyper, dtype=np.float64)
    from loss_weights_ref import weighted_losses_and_grads
    return weighted_losses_and_grads(params, batch, hyper, c, dtype=np.float64)


def _drop_last_dims(params, batch, hyper, c=None, n_drop=8):
    """The reference of a policy loss that leaves out the last n_drop action dims: the oracle's step with the policy's
    head gradient zeroed there (mlp_backward on the rest), its loss and log_std gradient taken over the kept dims."""
    f = np.float64
    ref = _base(params, batch, hyper, c)
    P = {k: v.astype(f) for k, v in params["pi"].items()}
    s, a = batch["s"].astype(f), batch["a"].astype(f)
    B, A = a.shape
    keep = np.arange(A) < max(0, A - n_drop)
    w, mu = ref["exp_adv"] * (1.0 if c is None else np.asarray(c, dtype=f)), ref["mu"]
    diff = a - mu
    if hyper.get("deterministic", False):
        bc = diff * diff
        dmu = -2.0 * w[:, None] * diff / B
        extra = {}
    else:
        ls = np.clip(P["log_std"], O.LOG_STD_MIN, O.LOG_STD_MAX)
        var = np.exp(ls) ** 2
        bc = diff * diff / (2.0 * var) + ls + math.log(math.sqrt(2.0 * math.pi))
        dmu = -w[:, None] * diff / var / B
        extra = {"log_std": ref["grads"]["pi"]["log_std"] * keep}
    dpre = dmu * (1.0 - mu * mu) * keep
    out = dict(ref)
    out["grads"] = dict(ref["grads"])
    out["grads"]["pi"] = O.mlp_backward({k: v for k, v in P.items() if k != "log_std"}, s, *ref["acts"]["pi"], dpre)
    out["grads"]["pi"].update(extra)
    out["actor_loss"] = np.sum(w * (bc * keep).sum(1)) / B
    return out


MUTANTS = ("no_weight_clamp", "no_log_std_clamp", "inside_exclusive", "terminals_ignored", "last8_dims_dropped")


def mutant_applies(name, hyper):
    return not hyper.get("deterministic", False) or name not in ("no_log_std_clamp", "inside_exclusive")


def mutant(name, params, batch, hyper, c=None):
    """The float64 result a step with one branch wrong would give (c: row weights, the row-weighted step)."""
    if name == "no_weight_clamp":
        with _patched(EXP_ADV_MAX=np.inf):
            return _base(params, batch, hyper, c)
    if name == "no_log_std_clamp":         # neither the clip nor the mask
        with _patched(LOG_STD_MIN=-np.inf, LOG_STD_MAX=np.inf):
            return _base(params, batch, hyper, c)
    if name == "inside_exclusive":         # `<` for `<=`: the dims exactly on a bound get no log_std gradient
        out = _base(params, batch, hyper, c)
        ls = params["pi"]["log_std"].astype(np.float64)
        out["grads"]["pi"]["log_std"] = out["grads"]["pi"]["log_std"] * ((ls > O.LOG_STD_MIN) & (ls < O.LOG_STD_MAX))
        return out
    if name == "terminals_ignored":
        b = dict(batch)
        b["d"] = np.zeros_like(batch["d"])
        return _base(params, b, hyper, c)
    assert name == "last8_dims_dropped", name
    return _drop_last_dims(params, batch, hyper, c)


def mutant_free(params, batch, hyper, c=None):
    """The right reference, through the same door as the wrong ones."""
    return _base(params, batch, hyper, c)


def mutants(params, batch, hyper, c=None):
    """Yields (name, float64 oracle-style result) for every wrong reference that applies to the case."""
    for name in MUTANTS:
        if mutant_applies(name, hyper):
            yield name, mutant(name, params, batch, hyper, c)


def row_weights(B):
    """Loss weights in {0, 0.25, 1, 1000} for the row-weighted backward, every value in every row tile."""
    return np.array([0.0, 0.25, 1.0, 1000.0, 1.0], dtype=np.float32)[np.arange(B) % 5]


def with_other_zero_weight_rows(batch, c):
    """The batch with every zero-weight row's contents replaced by other finite values."""
    out = {k: v.copy() for k, v in batch.items()}
    z = np.flatnonzero(np.asarray(c) == 0.0)
    n = batch["s"].shape[0]
    out["s"][z] = -2.0 * batch["s"][(z + 2) % n] + 0.5
    out["ns"][z] = batch["ns"][(z + 3) % n] * 1.5
    out["a"][z] = -batch["a"][(z + 1) % n]
    out["r"][z] = batch["r"][(z + 1) % n] + 7.0
    out["d"][z] = 1.0 - batch["d"][z]
    return out


# ------------------------------------------------------------------------------------- the oracle check, as a function
# The bounds of the GPU tests' oracle check, stated once so that the CPU test can ask what they can see.
F32_LOSS_RTOL = 1e-5          # tests/test_hip_parity.py::test_edge_shapes_match_oracle
F32_GRAD_ABS = 1e-5           # |dg|inf <= 1e-5 * max(1, |g|inf)
F32_GRAD_REL = 2e-5           # ... and <= 2e-5 * |g|inf
BF16_LOSS_RTOL = 5e-3         # tests/test_hip_lb.py: LOSS_RTOL
BF16_GRAD_RL2 = 8.5e-2        # GRAD_RL2
BF16_SMALL_ABS = 2e-2         # tensors of <= 32 elements: |dg|inf <= 2e-2 * max(1, |g|inf)
TD_RTOL = 2e-5               # tests/test_hip_loss_weights.py: TD errors, of the largest
LOSS_NAMES = ("value_loss", "q_loss", "actor_loss")


def oracle_check_errors(got_losses, got_grads, ref, precision):
    """{assertion: error / its tolerance} for every tolerance-based assertion of the oracle check: a value above 1 fails.
    got_grads: {net: {tensor: array}}; ref: the float64 oracle's result."""
    out = {}
    assert precision in ("f32", "f32rw", "bf16"), precision
    f32 = precision != "bf16"
    for name, got in zip(LOSS_NAMES, got_losses):
        want = float(ref[name])
        out["loss." + name] = abs(float(got) - want) / ((F32_LOSS_RTOL if f32 else BF16_LOSS_RTOL) * abs(want))
    for net, tensors in ({} if got_grads is None else ref["grads"]).items():
        for t, want in tensors.items():
            g = np.asarray(got_grads[net][t], dtype=np.float64).reshape(want.shape)
            gmax = float(np.max(np.abs(want)))
            err = float(np.max(np.abs(g - want)))
            key = f"grad.{net}.{t}"
            if precision == "f32rw":      # the row-weighted step: tests/test_hip_loss_weights.py, |dg|inf <= 1e-5 |g|inf
                out[key] = err / (F32_GRAD_ABS * max(gmax, 1e-30))
            elif f32:
                out[key] = err / min(F32_GRAD_ABS * max(1.0, gmax), F32_GRAD_REL * max(gmax, 1e-30))
            elif want.size <= 32:
                out[key] = err / (BF16_SMALL_ABS * max(1.0, gmax))
            else:
                den = float(np.linalg.norm(want))
                if den >= 1e-20:
                    out[key] = float(np.linalg.norm(g - want)) / den / BF16_GRAD_RL2
    return out
