"""GPU tests of the Adam / Polyak update from a trained-like optimiser state.  Every other step test starts Adam from
m = v = 0, where m / sqrt(v) is +-1 whatever the betas and bias corrections are; here the update kernels get moments of
mixed sign and size (1e-12 .. 1e2), second moments from 0 and denormals up to 1e4 (v = 0 under m != 0 included),
gradients of the same range with exact zeros, step counts 1 / 10 / 1000 / 1e6 set through the resume path
(load_state_dict), an actor learning rate inside the cosine schedule, grad_scale != 1 and a binding clip.

Reference: oracle.adam_update and oracle.polyak in float64, elementwise over the whole arena.  Bound per element:
k * 2^-24 relative to the quantity — for exp_avg and the target, whose two terms can cancel (g near -9 m), to the sum
of the two terms' magnitudes, the scale their roundings have, and for the parameter's change, which is a multiple of
the new exp_avg, to the same multiple of that scale — plus 2^-149 (the spacing of fp32 denormals) and, for the
parameter's change, half an ulp of the new parameter.  k = 4 x the largest error, in those units, of the SAME oracle run in fp32
against its float64 run on the same inputs: reference only, computed and printed here (profiles/value_edges_margins.txt).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import synth
import value_edges as ve
from oracle import iql_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -149
K_MARGIN = 4.0
EPOCH, T_MAX = 400, 1000          # the actor's cosine schedule stands at 400 of 1000 steps
GROUPS = ("v", "q", "q", "pi")    # optimizer group of the nets V, Q1, Q2, PI


def _hip():
    import iqlhip_binding as hb
    from hip_helpers import assert_same_trainer_state, build_hip_trainer, eager_segment
    return hb, build_hip_trainer, assert_same_trainer_state, eager_segment


def _trained_like_params(S, A):
    params = synth.synth_params(S, A, seed=50 + S, gaussian=True)
    data = synth.synth_transitions(64, S, A, seed=51 + S)
    ve.trained_like(params, data, {"B": 64, "A": A, "gaussian": True})
    return params


def _covered(L):
    """True where an arena element belongs to a tensor; the rest is alignment padding."""
    m = np.zeros(int(L.n_params), dtype=bool)
    for i in range(4):
        nl = L.net[i]
        k, d = int(nl.k_in), int(nl.d_out)
        for off, n in ((nl.w1, 65536), (nl.w0, 256 * k), (nl.b0, 256), (nl.b1, 256), (nl.w2, 256 * d), (nl.b2, d)):
            m[int(off): int(off) + n] = True
        if nl.log_std >= 0:
            m[int(nl.log_std): int(nl.log_std) + d] = True
    return m


def _state(L, seed, params_arena):
    """(m, v, g) over the arena, zero in the padding (the update rewrites it: only zeros come back as they were). |m| <= 100 (sqrt(v) + eps) keeps one update within a hundred
    step sizes, so the state stays trained-like after it."""
    rng = np.random.default_rng(seed)
    n = int(L.n_params)
    cov = _covered(L)

    def logu(lo, hi):
        return np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    v = logu(1e-30, 1e4)
    kind = rng.integers(0, 16, n)
    v[kind == 0] = 0.0
    v[kind == 1] = rng.uniform(1.0, 8e6, (kind == 1).sum()) * 2.0 ** -149       # denormals
    v[kind == 2] = 1e-30
    v[kind == 3] = 1e4
    v = v.astype(np.float32)
    m = logu(1e-12, 1e2) * rng.choice([-1.0, 1.0], n)
    m = np.sign(m) * np.minimum(np.abs(m), 100.0 * (np.sqrt(v.astype(np.float64)) + 1e-8))
    m = m.astype(np.float32)
    g = (logu(1e-12, 1e2) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g[rng.integers(0, 8, n) == 0] = 0.0
    first = np.flatnonzero(cov)[:4]
    v[first], m[first], g[first] = 0.0, np.float32([1e-7, -1e-7, 1e-12, -1e-6]), np.float32([0.0, 1.0, 0.0, -1e-12])
    for a in (m, v, g):
        a[~cov] = 0.0
    assert np.any((v == 0) & (m != 0) & cov) and np.any((g == 0) & cov) and np.any((v > 0) & (v < 2.0 ** -126))
    assert params_arena.shape == (n,) and np.all(params_arena[~cov] == 0.0)
    return m, v, g


def _resume(tr, t_before, epoch=EPOCH):
    """Put the trainer where a checkpoint taken after `t_before` Adam steps and `epoch` scheduler steps would: through
    state_dict() / load_state_dict(), the resume path.  The moments it loads are zeros; the arenas are written after."""
    sd = tr.state_dict()
    for key, opt in (("v_optimizer", tr.v_optimizer), ("q_optimizer", tr.q_optimizer), ("actor_optimizer", tr.actor_optimizer)):
        ps = opt.param_groups[0]["params"]
        sd[key]["state"] = {i: {"step": torch.tensor(float(t_before)), "exp_avg": torch.zeros(p.shape),
                                "exp_avg_sq": torch.zeros(p.shape)} for i, p in enumerate(ps)}
    lr = O.cosine_lr(ve.LRS["pi"], epoch, T_MAX)
    sd["actor_optimizer"]["param_groups"][0]["lr"] = lr
    sd["actor_lr_schedule"].update({"last_epoch": epoch, "_step_count": epoch + 1, "_last_lr": [lr]})
    sd["total_it"] = epoch
    tr.load_state_dict(sd)
    assert tr._adam_t == {"v": t_before, "q": t_before, "pi": t_before} and tr.total_it == epoch
    assert 0.0 < tr._current_lrs()["pi"] < ve.LRS["pi"] and tr._current_lrs()["pi"] == lr


def _write_arenas(tr, p, t, m, v):
    with torch.no_grad():
        for arena, host in ((tr._params_arena, p), (tr._target_arena, t), (tr._m_arena, m), (tr._v_arena, v)):
            arena.copy_(torch.from_numpy(host))


def _reference(L, p, tgt, m, v, g, lrs, t, tau, dtype):
    """One update over the whole arena: (p, m, v, target) after it, in `dtype`."""
    f = dtype
    p2, m2, v2 = p.astype(f), m.astype(f), v.astype(f)
    for i in range(4):
        a, b = int(L.net[i].seg_begin), int(L.net[i].seg_end)
        p2[a:b], m2[a:b], v2[a:b] = O.adam_update(p[a:b].astype(f), g[a:b].astype(f), m[a:b].astype(f), v[a:b].astype(f),
                                                  lrs[GROUPS[i]], t, dtype=f)
    src = int(L.target_src)
    t2 = O.polyak(tgt.astype(f), p2[src: src + int(L.n_target)], tau, dtype=f)
    return p2, m2, v2, t2


def _errors(got, ref64, inputs, tau):
    """{quantity: per-element error in units of 2^-24 x its scale (+ 2^-149; + half an ulp of p for the change of p)}."""
    p, tgt, m, v, g = (x.astype(np.float64) for x in inputs[:5])
    gp, gm, gv, gt = (x.astype(np.float64) for x in got)
    rp, rm, rv, rt = ref64
    half_ulp = 0.5 * np.spacing(np.abs(rp).astype(np.float32)).astype(np.float64)
    src, n_t = inputs[5], tgt.size
    m_scale = 0.9 * np.abs(m) + 0.1 * np.abs(g)
    # (the change of p is step_size / denom times the new exp_avg and inherits its rounding scale: |dp| * m_scale / |m'|)
    dp_scale = np.abs(rp - p) * np.divide(m_scale, np.abs(rm), out=np.ones_like(rm), where=rm != 0)
    return {
        "dp": np.maximum(np.abs((gp - p) - (rp - p)) - half_ulp, 0.0) / (U * dp_scale + TINY),
        "m": np.abs(gm - rm) / (U * m_scale + TINY),
        "v": np.abs(gv - rv) / (U * np.abs(rv) + TINY),
        "target": np.abs(gt - rt) / (U * ((1.0 - tau) * np.abs(tgt) + tau * np.abs(rp[src: src + n_t])) + TINY),
    }


CASES = [(17, 6, 1, 1.0), (17, 6, 10, 1.0), (39, 28, 1000, 1.0), (39, 28, 1000000, 1.0), (17, 6, 10, 0.25)]


@pytest.mark.parametrize("S,A,t,grad_scale", CASES)
def test_update_from_a_trained_like_state(S, A, t, grad_scale):
    hb, build, _, _ = _hip()
    params = _trained_like_params(S, A)
    tr = build(params, S, A, True, ve.HYPER, ve.LRS, T_MAX)
    L = tr._layout
    n, n_t, src = int(L.n_params), int(L.n_target), int(L.target_src)
    _resume(tr, t - 1)
    p = tr._params_arena.cpu().numpy()
    tgt = p[src: src + n_t] * np.float32(0.97) + np.float32(0.01) * (p[src: src + n_t] != 0)      # a target away from Q
    m, v, g = _state(L, 7 * S + t % 1000, p)
    cov = _covered(L)
    # arenas of the test's own, 256 sentinel floats past n_params / n_target, bound in place of the trainer's
    GUARD = 256
    dev = []
    for host, size in ((p, n), (tgt, n_t), (m, n), (v, n), (np.concatenate([g, np.float32([1.0, 2.0, 3.0, 0.0])]), n + 4)):
        a = torch.full((size + GUARD,), 12345.0, dtype=torch.float32, device="cuda")
        a[: host.size] = torch.from_numpy(host)
        dev.append(a)
    hb.check(hb.lib().iqlhip_bind(tr._ctx, *(a.data_ptr() for a in dev[:4])))
    t_now = {grp: t for grp in ("v", "q", "pi")}
    lrs = tr._current_lrs()
    sc = hb.StepScalars()
    tr._fill_scalars(sc, t_now, lrs, 1.0 / 256)
    sc.grad_scale = grad_scale
    hb.check(hb.lib().iqlhip_apply_update(tr._ctx, dev[4].data_ptr(), C.byref(sc), tr._stream()))
    torch.cuda.synchronize()
    out = [a.cpu().numpy() for a in dev]
    for a, size in zip(out, (n, n_t, n, n, n + 4)):
        assert np.all(a[size:] == 12345.0)                      # nothing written past the arenas
    gp, gt, gm, gv = out[0][:n], out[1][:n_t], out[2][:n], out[3][:n]
    assert np.array_equal(out[4][: n + 4], np.concatenate([g, np.float32([1.0, 2.0, 3.0, 0.0])]))
    # alignment padding: zero before, zero after.  The update kernel walks every element of [seg_begin, seg_end) and
    # REWRITES the padding with Adam's and Polyak's result on it; on zeros that is +0.0 again, which is all this holds
    # (zero padding stays zero, as a real arena's does) — not that the padding is left unwritten.  What may not be
    # written at all is checked by the sentinels above.
    for a, b in ((gp, p), (gm, m), (gv, v)):
        assert np.array_equal(a[~cov].view(np.uint32), b[~cov].view(np.uint32))
    assert np.array_equal(gt[~cov[src: src + n_t]].view(np.uint32), tgt[~cov[src: src + n_t]].view(np.uint32))
    assert all(np.all(np.isfinite(a)) for a in (gp, gt, gm, gv))
    # the reference: the scaled gradient is what Adam sees (an exact product here: grad_scale is a power of two)
    ge = (g.astype(np.float64) * grad_scale).astype(np.float32)
    assert np.array_equal(ge.astype(np.float64), g.astype(np.float64) * grad_scale)
    ref64 = _reference(L, p, tgt, m, v, ge, lrs, t, ve.HYPER["tau"], np.float64)
    ref32 = _reference(L, p, tgt, m, v, ge, lrs, t, ve.HYPER["tau"], np.float32)
    inputs = (p, tgt, m, v, ge, src)
    floor = _errors(ref32, ref64, inputs, ve.HYPER["tau"])
    errs = _errors((gp, gm, gv, gt), ref64, inputs, ve.HYPER["tau"])
    k = K_MARGIN * max(float(e.max()) for e in floor.values())
    print(f"adam S={S} A={A} t={t} grad_scale={grad_scale}: fp32 oracle vs float64 oracle "
          + " ".join(f"{q}={float(e.max()):.3g}" for q, e in floor.items()) + f" -> k = {k:.3g}; kernel "
          + " ".join(f"{q}={float(e.max()):.3g}" for q, e in errs.items()) + " (units of 2^-24 of the quantity)")
    for q, e in errs.items():
        assert float(e.max()) <= k, (q, float(e.max()), k, int(np.argmax(e)))
    # the update did something (exp_avg_sq moves wherever it is not at its fixed point v = g^2)
    assert np.mean(gv[cov] != v[cov]) > 0.9 and np.mean(gm[cov] != m[cov]) > 0.9 and np.any(gp != p) and np.any(gt != tgt)


def test_clipped_update_from_a_trained_like_state():
    """A binding clip (set_grad_clip) in front of the same update: train() from trained-like moments against the
    reference fed with the step's own gradient (flat_gradient) times the step's own coefficients, which
    tests/test_hip_grad_clip.py holds to the formula — the CLIP instantiation's arithmetic at nonzero m and v."""
    import clip_ref
    from hip_helpers import to_torch_batch
    from helpers import step_batch
    hb, build, _, _ = _hip()
    S, A, B, t = 17, 6, 100, 10
    params = _trained_like_params(S, A)
    tr = build(params, S, A, True, ve.HYPER, ve.LRS, T_MAX)
    tr.set_grad_clip((0.05, 0.05, 0.05))
    L = tr._layout
    n, n_t, src = int(L.n_params), int(L.n_target), int(L.target_src)
    _resume(tr, t - 1)
    p = tr._params_arena.cpu().numpy()
    tgt = p[src: src + n_t] * np.float32(0.97)
    m, v, _ = _state(L, 5, p)
    _write_arenas(tr, p, tgt, m, v)
    tb = to_torch_batch(step_batch(S, A, B, seed=8))
    g = tr.flat_gradient(tb)[:n].copy()
    lrs = tr._current_lrs()
    tr.train(tb)
    clip = tr.last_grad_clip()
    coef = {"v": clip["coef_vf"], "q": clip["coef_qf"], "pi": clip["coef_actor"]}
    for grp, key in (("v", "vf"), ("q", "qf"), ("pi", "actor")):
        assert coef[grp] < 1.0                                                    # binding
        assert abs(coef[grp] - float(clip_ref.coef(clip["norm_" + key], 0.05))) <= 1e-6 * coef[grp]
    ge = g.copy()
    for i in range(4):
        a, b = int(L.net[i].seg_begin), int(L.net[i].seg_end)
        ge[a:b] = g[a:b] * np.float32(coef[GROUPS[i]])                            # one rounded product, like the kernel's
    got = tuple(x.cpu().numpy() for x in (tr._params_arena, tr._m_arena, tr._v_arena, tr._target_arena))
    ref64 = _reference(L, p, tgt, m, v, ge, lrs, t, ve.HYPER["tau"], np.float64)
    ref32 = _reference(L, p, tgt, m, v, ge, lrs, t, ve.HYPER["tau"], np.float32)
    inputs = (p, tgt, m, v, ge, src)
    floor = _errors(ref32, ref64, inputs, ve.HYPER["tau"])
    errs = _errors(got, ref64, inputs, ve.HYPER["tau"])
    k = K_MARGIN * max(float(e.max()) for e in floor.values())
    print(f"adam clipped S={S} A={A} t={t} coefficients {coef}: fp32 oracle vs float64 oracle "
          + " ".join(f"{q}={float(e.max()):.3g}" for q, e in floor.items()) + f" -> k = {k:.3g}; kernel "
          + " ".join(f"{q}={float(e.max()):.3g}" for q, e in errs.items()))
    for q, e in errs.items():
        assert float(e.max()) <= k, (q, float(e.max()), k, int(np.argmax(e)))


@pytest.mark.parametrize("S,A,B,precision,clip", [
    (17, 6, 100, "f32", None),          # iql_update_kernel<FROM_TABLE> in the chunk graphs against the eager kernel
    (17, 6, 100, "f32", 0.05),          # iql_update_clip_kernel<FROM_TABLE> against <false>, the clip binding
    (39, 28, 600, "bf16", None),        # the LB instantiations: their weight images feed the next step's forward
])
def test_three_train_steps_from_a_trained_like_state_equal_eager_steps(S, A, B, precision, clip):
    import iql
    hb, build, same_state, eager_segment = _hip()
    N, K, t = 1500, 3, 1000
    params = _trained_like_params(S, A)
    data = synth.synth_transitions(N, S, A, seed=31)
    buf = iql.ReplayBuffer(S, A, N, "cuda")
    buf.load_d4rl_dataset(data)
    from helpers import uses_large_batch_kernels
    assert uses_large_batch_kernels(S, A, B) == (precision == "bf16")      # (the bf16 case is a large-batch one)

    def trainer(prec):
        tr = build(params, S, A, True, ve.HYPER, ve.LRS, T_MAX)
        if prec == "bf16":
            tr.set_precision("bf16")
        if clip:
            tr.set_grad_clip(clip)
        tr.reserve_batch(B)
        _resume(tr, t - 1)
        L = tr._layout
        src, n_t = int(L.target_src), int(L.n_target)
        p = tr._params_arena.cpu().numpy()
        m, v, _ = _state(L, 9, p)
        _write_arenas(tr, p, p[src: src + n_t] * np.float32(0.97), m, v)
        return tr
    burst, eager = trainer(precision), trainer(precision)
    before = burst._params_arena.cpu().numpy()
    lb = burst.train_steps(buf, K, B, seed=13)
    le = eager_segment(eager, buf, K, B, 13)
    assert np.all(np.isfinite(lb)) and np.array_equal(lb, le), (lb, le)
    same_state(burst, eager, f"{precision} B={B} clip={clip}")
    assert burst._adam_t == {"v": t - 1 + K, "q": t - 1 + K, "pi": t - 1 + K} and burst.total_it == EPOCH + K
    assert np.any(burst._params_arena.cpu().numpy() != before)
    if clip:
        assert all(burst.last_grad_clip()[k] < 1.0 for k in ("coef_vf", "coef_qf", "coef_actor"))
    if precision == "bf16":
        # the bf16 kernels really ran: the same first step in fp32 gives other loss words
        l32 = eager_segment(trainer("f32"), buf, K, B, 13)
        assert np.all(lb[0] != l32[0]), (lb[0], l32[0])
