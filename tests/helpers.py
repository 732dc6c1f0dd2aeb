"""Shared test helpers: fixture loading, input reconstruction, comparisons."""
from __future__ import annotations

import json
import os

import numpy as np

import synth  # jsrl-corl_amd/synth.py (on sys.path via conftest)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

SINGLE_STEP_CASES = sorted(
    f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz") and f[:3] in ("g1_", "g7_", "g8_"))
FREERUN_CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("g2_"))


ACT_CASES = ["g10_act_S17A6_gauss", "g10_act_S29A8_det", "g10_act_S39A28_gauss"]


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    return z, meta


def sub(arr, stride):
    a = np.asarray(arr)
    if a.size > 4096:
        return a.ravel()[::stride].copy()
    return a.copy()


def apply_edge(params, data, meta):
    """Same input surgery tools/make_goldens.py applies for the g7 edge cases."""
    B, A, gaussian = meta["B"], meta["A"], meta["gaussian"]
    params["qt1"]["b2"] = params["qt1"]["b2"] + np.float32(60.0)
    params["qt2"]["b2"] = params["qt2"]["b2"] + np.float32(60.0)
    if gaussian:
        ls = np.zeros(A, dtype=np.float32)
        ls[:6] = np.array([3.0, -25.0, 0.5, 2.0, -20.0, -1.0], dtype=np.float32)[: min(6, A)]
        params["pi"]["log_std"] = ls
    data["terminals"][: B // 4] = 1.0
    for k in data:
        data[k][B // 2: B // 2 + 16] = data[k][:16]


def single_step_inputs(meta):
    params = synth.synth_params(meta["S"], meta["A"], seed=meta["seed"], gaussian=meta["gaussian"])
    data = synth.synth_transitions(meta["B"], meta["S"], meta["A"], seed=1000 + meta["seed"])
    if meta.get("edge"):
        apply_edge(params, data, meta)
    batch = {"s": data["observations"], "a": data["actions"], "r": data["rewards"],
             "ns": data["next_observations"], "d": data["terminals"]}
    hyper = dict(meta["hyper"])
    hyper["deterministic"] = not meta["gaussian"]
    return params, batch, hyper


def batch_from(data, idx):
    return {"s": data["observations"][idx], "a": data["actions"][idx], "r": data["rewards"][idx],
            "ns": data["next_observations"][idx], "d": data["terminals"][idx]}


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-30, np.max(np.abs(b))))


def assert_losses(got, want, rtol=1e-5, what=""):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-12)
    assert np.all(err <= rtol), f"{what} losses {got} vs {want}: rel err {err}"


def assert_params_after_free_run(got, want, n_steps, lr, what=""):
    """Parameters after n free-running Adam steps against the reference's.

    Two mechanisms legitimately turn a different (equally valid) fp32 summation order into visible differences:
      * Adam's update lr*m/(sqrt(v)+eps) maps a ~1e-8 gradient perturbation to O(1e-7) for the few elements whose
        gradient is itself ~eps, and
      * such a 1e-7 parameter difference can flip the ReLU mask of ONE hidden unit for ONE row on the next batch,
        which changes that unit's gradient by a row's share and then its whole weight row by O(lr) per step
        (observed: fixture g2_freerun_S29A8_det, Q2 unit 169 at step 1 — see DESIGN.md "free-run tolerance").
    So the per-element bound is the hard cap 1.5*n_steps*lr, and the bulk must agree: RMS <= 5e-6 and at most 2 %
    of the elements (a couple of units' rows) off by more than 2e-6.  Single-step fixtures stay at ~1e-7."""
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).ravel()
    assert d.max() <= 1.5 * n_steps * lr, (what, "max", d.max())
    assert np.sqrt(np.mean(d * d)) <= 5e-6, (what, "rms", np.sqrt(np.mean(d * d)))
    assert np.sum(d > 2e-6) <= max(2, 0.02 * d.size), (what, "outliers", np.mean(d > 2e-6))
    assert np.median(d) <= 5e-7, (what, "median", np.median(d))


def check_step_against_golden(z, meta, info, newp, newo, *, grad_rtol=1e-5, param_atol=2e-6,
                              moment_rtol=1e-5, target_atol=1e-7, loss_rtol=1e-5, check_moments=True):
    """Teacher-forced single-step tolerances of SURVEY.md §8(d).

    info: losses/intermediates/grads (oracle-style dict); newp/newo: post-step
    params and Adam moments as {net:{tensor:array}}.  Any of them may be None.
    """
    stride = meta["stride"]
    worst = {}
    if info is not None:
        assert_losses([info["value_loss"], info["q_loss"], info["actor_loss"]], z["losses"], loss_rtol)
        for k, key in (("next_v", "next_v"), ("target_q", "target_q"), ("adv", "adv")):
            if key in info and info[key] is not None:
                e = rel_err(info[key], z[f"inter.{k}"])
                worst[f"inter.{k}"] = e
                assert e <= 2e-5, f"{k}: rel err {e}"
        if info.get("grads") is not None:
            for net, tensors in info["grads"].items():
                for t, g in tensors.items():
                    key = f"grad.{net}.{t}"
                    if key not in z:
                        continue
                    want = z[key]
                    got = sub(g, stride).reshape(want.shape)
                    # SURVEY §8d asks |dg|_inf <= 1e-5*max(1,|g|_inf); we hold the stricter
                    # |dg|_inf <= grad_rtol*|g|_inf (relative to the tensor's own max).
                    scale = max(float(np.max(np.abs(want))), 1e-30)
                    e = float(np.max(np.abs(got.astype(np.float64) - want))) / scale
                    worst[key] = e
                    assert e <= grad_rtol, f"{key}: rel-to-max err {e} > {grad_rtol}"
    if newp is not None:
        for net, tensors in newp.items():
            for t, p in tensors.items():
                key = f"param.{net}.{t}"
                if key not in z:
                    continue
                want = z[key]
                got = sub(p, stride).reshape(want.shape)
                diff = np.abs(got.astype(np.float64) - want)
                atol = target_atol if net in ("qt1", "qt2") else param_atol
                tol = np.full(diff.shape, atol)
                gkey = f"grad.{net}.{t}"
                if gkey in z and net not in ("qt1", "qt2"):
                    # Adam's first step is u(g) = -lr*g/(|g|+eps): an element whose gradient is
                    # within fp32 summation noise (dg ~ 2e-6*|g|_inf) of eps=1e-8 legitimately moves
                    # by up to lr*eps*dg/(|g|+eps)^2 (<= lr) more.  Everything else holds param_atol.
                    g = np.abs(z[gkey].astype(np.float64)).reshape(diff.shape)
                    dg = 2e-6 * max(float(g.max()), 1e-30)
                    lr = max(meta["lrs"].values())
                    tol = tol + lr * np.minimum(1.0, 1e-8 * dg / (g + 1e-8) ** 2)
                e = float(np.max(diff))
                worst[key] = e
                bad = diff > tol
                assert not bad.any(), f"{key}: {int(bad.sum())} elements beyond tolerance, worst abs err {e}"
    if newo is not None and check_moments:
        for mv in ("m", "v"):
            for net, tensors in newo[mv].items():
                for t, a in tensors.items():
                    key = f"{mv}.{net}.{t}"
                    if key not in z:
                        continue
                    want = z[key]
                    got = sub(a, stride).reshape(want.shape)
                    scale = max(float(np.max(np.abs(want))), 1e-30)
                    e = float(np.max(np.abs(got.astype(np.float64) - want))) / scale
                    worst[key] = e
                    assert e <= moment_rtol, f"{key}: rel-to-max err {e} > {moment_rtol}"
    return worst


def act_case_params(meta, z):
    """Policy parameters of a G10 fixture: synth_params(seed)["pi"] with the fixture's log_std."""
    pi = synth.synth_params(meta["S"], meta["A"], seed=meta["seed"], gaussian=meta["gaussian"])["pi"]
    if meta["gaussian"]:
        pi["log_std"] = z["log_std"].copy()
    return pi


def check_state_against_golden(z, meta, prefix, newp, newo, *, param_atol=2e-6, moment_rtol=1e-5, target_atol=1e-7,
                               grad_prefix=None):
    """Parameters / Adam moments / target under fixture keys `<prefix>.param.*`, `<prefix>.m.*`, `<prefix>.v.*`
    (fixtures g11: state after several steps, where no single-step gradient is stored).  Tolerances as in
    check_step_against_golden; the Adam allowance for near-zero gradients does not apply after the first step (the
    moments carry history), so parameters get param_atol plus the documented free-run slack of one lr per ReLU-flip
    bifurcation is NOT granted here: these are teacher-forced continuations of a few steps."""
    stride = meta["stride"]
    worst = {}
    for net, tensors in newp.items():
        for t, p in tensors.items():
            key = f"{prefix}.param.{net}.{t}"
            if key not in z:
                continue
            want = z[key]
            got = sub(p, stride).reshape(want.shape)
            e = float(np.max(np.abs(got.astype(np.float64) - want)))
            worst[key] = e
            atol = target_atol if net in ("qt1", "qt2") else param_atol
            assert e <= atol, f"{key}: abs err {e} > {atol}"
    if newo is not None:
        for mv in ("m", "v"):
            for net, tensors in newo[mv].items():
                for t, a in tensors.items():
                    key = f"{prefix}.{mv}.{net}.{t}"
                    if key not in z:
                        continue
                    want = z[key]
                    got = sub(a, stride).reshape(want.shape)
                    scale = max(float(np.max(np.abs(want))), 1e-30)
                    e = float(np.max(np.abs(got.astype(np.float64) - want))) / scale
                    worst[key] = e
                    assert e <= moment_rtol, f"{key}: rel-to-max err {e} > {moment_rtol}"
    return worst


def step_batch(S, A, B, seed, **kw):
    d = synth.synth_transitions(B, S, A, seed=seed, **kw)
    return {"s": d["observations"], "a": d["actions"], "r": d["rewards"], "ns": d["next_observations"],
            "d": d["terminals"]}


# ---------------------------------------------------------------------------
# Which kernels a shape takes: Python restatements of the host's dispatch rules in csrc/iqlhip.hip, so that a test case's
# comment about its path is checked rather than asserted.

def w0_lds_k(S, A):
    """iqlhip_create's layer-0 staging rule: the widest layer-0 input whose weights the forward stages in LDS (through
    registers up to 64, by LDS-DMA above that: the forward's DMA=true instantiations); 0 = every W0 read from global."""
    row_ld = (2 * S + A + 2 + 3) // 4 * 4
    fixed = 4 * (32 * 260 + 32 * 68 + 32 * row_ld + ((A + 15) // 16 * 16) * 68 + 32 + 512 + 16)

    def fits(k):
        return fixed + 256 * k * 4 + 4096 <= 160 * 1024 - 1024
    if S + A <= 96 and fits(S + A):
        return S + A
    if S <= 96 and fits(S):
        return S
    return 0


def fwd_spb_l2(n_row_tiles, n_cus=256):
    """fwd_spb_l2: the forward's column slices per block (log2); > 0 selects the MULTI instantiations."""
    if 8 * n_row_tiles * 4 <= n_cus:
        return 0
    return 1 if 8 * n_row_tiles * 2 <= n_cus else 2


def uses_large_batch_kernels(S, A, B):
    """use_lb for a bf16 step: more than 512 rows and S + A + 1 <= 80."""
    return B > 512 and S + A + 1 <= 80


def bwd_spb_l2(n_chunk, n_rt, n_cus=256):
    """bwd_spb_l2: the backward's column slices per (b) block (log2); > 0 selects the MULTI instantiations."""
    return 0 if 4 * (32 * n_chunk + 4 * n_rt) <= 2 * n_cus else 2


def bwd_instantiation(S, A, B, precision, row_weighted=False, n_cus=256):
    """launch_bwd's choice for a step of B rows, by name: the large-batch pair (row kernel with or without its column
    split + the GEMM kernel) for a bf16 step that use_lb takes, else iql_bwd_kernel<BF16, FULL, MULTI> — FULL: the batch
    is whole 256-row chunks; MULTI: bwd_spb_l2 > 0 — or, with row weights (fp32 only), iql_bwd_rw_kernel<FULL, MULTI>."""
    n_rt, n_chunk = (B + 31) // 32, (B + 255) // 256
    bf = precision == "bf16"
    if bf and uses_large_batch_kernels(S, A, B):
        assert not row_weighted
        return f"iql_bwd_rows_kernel<CSPLIT={int(((n_rt + 1) & ~1) <= 32)}> + iql_bwd_gemm_kernel"
    full, multi = int(B % 256 == 0), int(bwd_spb_l2(n_chunk, n_rt, n_cus) > 0)
    if row_weighted:
        assert not bf
        return f"iql_bwd_rw_kernel<FULL={full}, MULTI={multi}>"
    return f"iql_bwd_kernel<BF16={int(bf)}, FULL={full}, MULTI={multi}>"


def row_f4(S, A):
    """float4s of one packed replay row (s, a, ns, r, d: 2 S + A + 2 floats, padded to a multiple of 4): what a gather's
    loop over a row copies, 64 per pass of a wave, and what the forward's xr registers hold of a 32-row tile."""
    return (2 * S + A + 2 + 3) // 4


# The five chunk-graph kinds of the multi-step driver (ChunkKind in csrc/iqlhip.hip) and the training forward of each.
CHUNK_KINDS = ("plain", "mixed", "weighted", "weighted_is", "prioritized")
_FWD_OF_KIND = {"plain": "iql_fwd_kernel", "mixed": "iql_fwd_mixed_kernel", "weighted": "iql_fwd_weighted_kernel",
                "weighted_is": "iql_fwd_weighted_is_kernel", "prioritized": "iql_fwd_prio_kernel"}


def fwd_instantiation(kind, S, A, B, precision, n_cus=256):
    """launch_fwd_grid / fwd_kernel_of's choice for a training step of B rows inside a chunk of `kind`, by name:
    iql_fwd*_kernel<BF16, W0DMA, MULTI> — W0DMA: w0_lds_k > 64 (some instance stages layer 0 by LDS-DMA); MULTI:
    fwd_spb_l2 > 0 — without BF16 for the two fp32-only kinds.  A bf16 step that use_lb takes runs iql_fwd_lb_kernel<NKB>
    instead (plain kind only: the others refuse such a batch; its policy-spread flag is not restated here)."""
    bf = precision == "bf16"
    if bf and uses_large_batch_kernels(S, A, B):
        assert kind == "plain", (kind, B)
        return f"iql_fwd_lb_kernel<NKB={1 if S + A <= 32 else 2 if S + A <= 64 else 3}>"
    dma, multi = int(w0_lds_k(S, A) > 64), int(fwd_spb_l2((B + 31) // 32, n_cus) > 0)
    if kind in ("weighted_is", "prioritized"):
        assert not bf, kind
        return f"{_FWD_OF_KIND[kind]}<W0DMA={dma}, MULTI={multi}>"
    return f"{_FWD_OF_KIND[kind]}<BF16={int(bf)}, W0DMA={dma}, MULTI={multi}>"


# ---------------------------------------------------------------------------
# Row-permutation checks.  Every IQL loss is a mean of per-row terms (adv is detached, there is no batch statistic), so a
# batch's gradient is the sum of its rows' terms and must not change, beyond fp32 summation order, when the rows are
# permuted — whatever precision the kernels use for a row's own values.  An fp32 sum of terms x_r taken in an order of
# depth d lies within d * u * sum_r |x_r| of the exact sum (u = 2^-24); two orders differ by at most twice that.

FP32_U = 2.0 ** -24
PERM_DEPTH = 16       # summation depth granted per gradient element


def rows_of(batch, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in batch.items()}


def row_abs_grad_sums(params, batch, hyper):
    """{net: {tensor: sum over rows of |that row's term of the gradient|}} in float64 — the scale of each gradient
    element's fp32 summation error (the oracle's per-row deltas, combined with absolute values)."""
    from oracle import iql_oracle as O
    f = np.float64
    n = f(batch["s"].shape[0])
    ref = O.iql_losses_and_grads(params, batch, hyper, dtype=f)
    P = {k: {t: v.astype(f) for t, v in p.items()} for k, p in params.items()}
    s, a = batch["s"].astype(f), batch["a"].astype(f)
    r, d = batch["r"].astype(f), batch["d"].astype(f)
    adv, w, mu = ref["adv"], ref["exp_adv"], ref["mu"]
    wgt = np.abs(f(hyper["iql_tau"]) - (adv < 0).astype(f))
    y = r + (1.0 - d) * f(hyper["discount"]) * ref["next_v"]
    diff = a - mu
    if hyper.get("deterministic", False):
        dmu = -2.0 * w[:, None] * diff / n
    else:
        var = np.exp(np.clip(P["pi"]["log_std"], O.LOG_STD_MIN, O.LOG_STD_MAX)) ** 2
        dmu = -w[:, None] * diff / var / n
    douts = {"vf": (-2.0 * wgt * adv / n)[:, None], "q1": ((ref["q1"] - y) / n)[:, None],
             "q2": ((ref["q2"] - y) / n)[:, None], "pi": dmu * (1.0 - mu * mu)}
    sa = np.concatenate([s, a], 1)
    xs = {"vf": s, "q1": sa, "q2": sa, "pi": s}
    out = {}
    for net, dout in douts.items():
        h0, h1 = ref["acts"][net]
        p = P[net]
        dh1 = (dout @ p["w2"]) * (h1 > 0)
        dh0 = (dh1 @ p["w1"]) * (h0 > 0)
        out[net] = {"w2": np.abs(dout).T @ np.abs(h1), "b2": np.abs(dout).sum(0),
                    "w1": np.abs(dh1).T @ np.abs(h0), "b1": np.abs(dh1).sum(0),
                    "w0": np.abs(dh0).T @ np.abs(xs[net]), "b0": np.abs(dh0).sum(0)}
    if not hyper.get("deterministic", False):
        inside = (P["pi"]["log_std"] >= O.LOG_STD_MIN) & (P["pi"]["log_std"] <= O.LOG_STD_MAX)
        out["pi"]["log_std"] = (np.abs(w[:, None] * (1.0 - diff * diff / var)) / n).sum(0) * inside
    return out


def smallest_row_groups(B):
    """The smallest row groups the kernels handle separately: the ragged remainder of the 32-row tiles (one row when B
    is a multiple of 32), at the end of the batch and — where a reversal moves them there — at its start."""
    tail = B % 32 or 1
    out = [np.arange(B - tail, B)]
    if B > tail:
        out.append(np.arange(0, tail))
    return out


def permutation_bounds(params, batch, hyper):
    """{(net, tensor): (tolerance, contribution)}, both max-abs over the tensor's elements.
    tolerance = 2 * PERM_DEPTH * u * max_ij sum_r |g_rij|: two fp32 orders of the same per-row terms.
    contribution = the smaller, over smallest_row_groups, of that group's own gradient (float64 oracle with the batch's
    divisor: the oracle is row-additive, tests/test_oracle_rows.py) — what the gradient moves by if the kernels drop or
    double the group."""
    from oracle import iql_oracle as O
    B = batch["s"].shape[0]
    sums = row_abs_grad_sums(params, batch, hyper)
    contrib = {}
    for grp in smallest_row_groups(B):
        g = O.iql_losses_and_grads(params, rows_of(batch, grp), hyper, dtype=np.float64, grad_scale_rows=B)["grads"]
        for net, ts in g.items():
            for t, v in ts.items():
                contrib[(net, t)] = min(contrib.get((net, t), np.inf), float(np.max(np.abs(v))))
    return {(net, t): (2.0 * PERM_DEPTH * FP32_U * float(np.max(v)), contrib[(net, t)])
            for net, ts in sums.items() for t, v in ts.items()}


# ---------------------------------------------------------------------------
# How iqlhip_train_steps (csrc/iqlhip.hip) composes a call, restated: the first 2 or 4 steps are launched directly
# (through the idle-work records of the plain chunk of that size), the rest as replays of fixed chunk graphs.  Each
# distinct chunk is one entry of the context's graph cache, keyed by what its captured kernel arguments froze.

GRAPH_STEPS = 64
GRAPH_CACHE_ENTRIES = 12      # chunk_graph evicts the least recently used entry beyond this


def _n_chunks_for(rem):
    n, rem = divmod(rem, GRAPH_STEPS)
    for c in (16, 4, 2, 1):
        n += rem // c
        rem %= c
    return n


def train_steps_decomposition(K):
    """(head, chunks): the steps launched directly at the head of a K-step call (4 when that leaves fewer chunk launches
    behind it than 2 does, else 2; 1 for a one-step call) and the chunk sizes replayed after it, in launch order — the
    even sizes below 64 ascending, the 64-step chunk as often as it fits, a one-step chunk last."""
    assert K >= 1
    head = 4 if (K >= 4 and _n_chunks_for(K - 4) < _n_chunks_for(K - 2)) else (2 if K >= 2 else 1)
    n64, rem = divmod(K - head, GRAPH_STEPS)
    small = []
    for c in (16, 4, 2, 1):
        while rem >= c:
            small.append(c)
            rem -= c
    chunks = [c for c in reversed(small) if c != 1] + [GRAPH_STEPS] * n64 + [c for c in small if c == 1]
    return head, chunks


def train_steps_graph_keys(K, B, rows=0, drop_p=0.0, stats=False):
    """The graph-cache keys a K-step call at batch size B asks for, in request order (without repeats): the GraphKey
    fields that vary on one trainer without a data-parallel exchange — (rows, B, chunk steps, drop_p, inv_batch, stats).
    The head's steps use the plain chunk of their size."""
    head, chunks = train_steps_decomposition(K)
    keys = []
    for k in [head] + chunks:
        key = (rows, int(B), int(k), float(np.float32(drop_p)), float(np.float32(1.0 / B)), int(bool(stats)))
        if key not in keys:
            keys.append(key)
    return keys


def graph_cache_requests(calls, capacity=GRAPH_CACHE_ENTRIES):
    """Replays the LRU cache over a list of calls (each a list of keys): (distinct keys requested, evictions)."""
    cache, distinct, evictions = [], set(), 0
    for keys in calls:
        for key in keys:
            distinct.add(key)
            if key in cache:
                cache.remove(key)
            elif len(cache) >= capacity:
                cache.pop(0)
                evictions += 1
            cache.append(key)
    return len(distinct), evictions


# Case 6 of tests/test_hip_between_calls.py (rows written between two train_steps calls), shared with its CPU companion:
# a 40-row buffer sampled 256 rows at a time, calls of 8 / 6 / 8 steps under one seed, and the rows the single-row
# writers touch (add_transition's ring pointer stands at row 0; the in-place reward write goes to row 3).
SMALL_BUFFER = {"N": 40, "B": 256, "segments": (8, 6, 8), "seed": 5, "pointer_row": 0, "reward_row": 3}
