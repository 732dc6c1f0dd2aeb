"""Reference of the scoring call (ImplicitQLearning.score_buffer / score / evaluate): the eight per-row columns, the
three losses and the column means, built from the dict oracle.iql_oracle.iql_losses_and_grads returns — the names in
the issue's table are that dict's.  Everything is computed in the dtype the oracle ran in (pass dtype=np.float64 to the
oracle for the fp64 value a tolerance is derived from)."""
from __future__ import annotations

import math

import numpy as np

from oracle import iql_oracle as O

SCORE_NAMES = ("v", "next_v", "q1", "q2", "target_q", "adv", "exp_adv", "bc")
LOSS_NAMES = ("value_loss", "q_loss", "actor_loss")


def bc_term(info, batch, hyper, log_std=None):
    """The row's behaviour-cloning term (iql.py:526-532): Gaussian policy: the row sum of -Normal.log_prob(a) with the
    clamped log_std (log_std: the policy's raw parameter); deterministic: the row sum of (a - mu)^2."""
    mu = info["mu"]
    f = mu.dtype.type
    diff = batch["a"].astype(f) - mu
    if hyper.get("deterministic", False):
        return np.sum(diff * diff, axis=1, dtype=f)
    ls = np.clip(np.asarray(log_std).astype(f), f(O.LOG_STD_MIN), f(O.LOG_STD_MAX))
    sig = np.exp(ls)
    nlp = diff * diff / (f(2.0) * (sig * sig)) + ls + f(math.log(math.sqrt(2.0 * math.pi)))
    return np.sum(nlp, axis=1, dtype=f)


def columns(info, batch, hyper, log_std=None):
    """{"cols": [n, 8] in SCORE_NAMES order, "losses": [3] in LOSS_NAMES order, "means": [8]} from the oracle's dict
    `info` for `batch` (the oracle's batch dict) under `hyper`."""
    f = info["v"].dtype.type
    bc = bc_term(info, batch, hyper, log_std)
    cols = np.stack([info["v"], info["next_v"], info["q1"], info["q2"], info["target_q"], info["adv"], info["exp_adv"],
                     bc], axis=1).astype(f)
    n = f(cols.shape[0])
    adv, nv, w = info["adv"], info["next_v"], info["exp_adv"]
    wgt = np.abs(f(hyper["iql_tau"]) - (adv < 0).astype(f))
    y = batch["r"].astype(f) + ((f(1.0) - batch["d"].astype(f)) * f(hyper["discount"])) * nv
    e1, e2 = info["q1"] - y, info["q2"] - y
    losses = np.array([np.sum(wgt * adv * adv, dtype=f) / n,
                       np.sum(e1 * e1 + e2 * e2, dtype=f) / n / f(2.0),
                       np.sum(w * bc, dtype=f) / n], dtype=f)
    return {"cols": cols, "losses": losses, "means": np.sum(cols, axis=0, dtype=f) / n}


def reference(params, batch, hyper, dtype=np.float32):
    """columns() of the oracle run on (params, batch, hyper) in `dtype`."""
    info = O.iql_losses_and_grads(params, batch, hyper, dtype=dtype)
    return columns(info, batch, hyper, params["pi"].get("log_std"))
