"""Numpy restatement of the row-weighted IQL step (trainer.train(batch, loss_weights=c)), built on the oracle's pieces:
mlp_forward / mlp_backward for the nets, iql_step(grads_override=...) for Adam and the target update.

    value_loss = 1/B sum_r c_r |tau - 1(u_r < 0)| u_r^2      q_loss = 1/B sum_r c_r (e1_r^2 + e2_r^2) / 2
    actor_loss = 1/B sum_r c_r exp_adv_r bc_r

Every head gradient of row r is the unweighted one times c_r, so the oracle's per-row quantities are reused as they are."""
import math

import numpy as np

from oracle import iql_oracle as O

GOLDENS = ["g20_loss_weights_S17A6_gauss_B100", "g20_loss_weights_S39A28_gauss_B10", "g20_loss_weights_S29A8_det_B256",
           "g20_loss_weights_S17A6_gauss_B300"]


def weighted_losses_and_grads(params, batch, hyper, c, dtype=np.float32):
    """iql_losses_and_grads with per-row loss weights c[B]; adds info["td"] = (q1 - y, q2 - y) as [B, 2]."""
    f = dtype
    info = O.iql_losses_and_grads(params, batch, hyper, dtype=dtype)
    P = {n: {k: v.astype(f) for k, v in t.items()} for n, t in params.items()}
    s, a, r, d = (batch[k].astype(f) for k in ("s", "a", "r", "d"))
    c = np.asarray(c, dtype=f).reshape(-1)
    B = s.shape[0]
    assert c.shape == (B,)
    Bf = f(B)
    adv, w, mu = info["adv"], info["exp_adv"], info["mu"]
    wgt = np.abs(f(hyper["iql_tau"]) - (adv < 0).astype(f))
    y = r + ((f(1.0) - d) * f(hyper["discount"])) * info["next_v"]
    e1, e2 = info["q1"] - y, info["q2"] - y
    v_loss = np.sum(c * (wgt * adv * adv), dtype=f) / Bf
    q_loss = (np.sum(c * (e1 * e1), dtype=f) / Bf + np.sum(c * (e2 * e2), dtype=f) / Bf) / f(2.0)
    dv = c * ((f(-2.0) * wgt * adv) / Bf)
    dq1, dq2 = c * (e1 / Bf), c * (e2 / Bf)
    diff = a - mu
    wc = w * c
    extra = {}
    if hyper.get("deterministic", False):
        bc = np.sum(diff * diff, axis=1, dtype=f)
        dmu = (f(-2.0) * wc[:, None] * diff) / Bf
    else:
        ls_raw = P["pi"]["log_std"]
        ls = np.clip(ls_raw, f(O.LOG_STD_MIN), f(O.LOG_STD_MAX))
        var = np.exp(ls) ** 2
        nlp = diff * diff / (f(2.0) * var) + ls + f(math.log(math.sqrt(2.0 * math.pi)))
        bc = np.sum(nlp, axis=1, dtype=f)
        dmu = (-(wc[:, None]) * diff / var) / Bf
        inside = ((ls_raw >= f(O.LOG_STD_MIN)) & (ls_raw <= f(O.LOG_STD_MAX))).astype(f)
        extra["log_std"] = np.sum(wc[:, None] * (f(1.0) - diff * diff / var), axis=0, dtype=f) / Bf * inside
    pi_loss = np.sum(wc * bc, dtype=f) / Bf
    dpre = dmu * (f(1.0) - mu * mu)
    sa = O.q_input(batch["s"].astype(f), a)
    acts = info["acts"]
    grads = {
        "vf": O.mlp_backward(P["vf"], batch["s"].astype(f), *acts["vf"], dv[:, None]),
        "q1": O.mlp_backward(P["q1"], sa, *acts["q1"], dq1[:, None]),
        "q2": O.mlp_backward(P["q2"], sa, *acts["q2"], dq2[:, None]),
        "pi": O.mlp_backward(P["pi"], batch["s"].astype(f), *acts["pi"], dpre),
    }
    grads["pi"].update(extra)
    out = dict(info)
    out.update({"value_loss": v_loss, "q_loss": q_loss, "actor_loss": pi_loss, "grads": grads,
                "td": np.stack([e1, e2], axis=1)})
    return out


def weighted_step(params, opt, batch, hyper, lrs, c, dtype=np.float32):
    """One weighted step: (new_params, new_opt, info) like O.iql_step."""
    info = weighted_losses_and_grads(params, batch, hyper, c, dtype=dtype)
    newp, newo, _ = O.iql_step(params, opt, batch, hyper, lrs, dtype=dtype, grads_override=info["grads"])
    return newp, newo, info
