"""float64 numpy restatement of the per-step training statistics (include/iqlhip.h).

Not a test module: the step-statistics tests import it.  Everything is computed in float64 from the values it is
given; nothing here knows about the device's summation order.
"""
import numpy as np

STAT_NAMES = ("v_mean", "next_v_mean", "q1_mean", "q2_mean", "target_q_mean", "td_target_mean", "q_gap_mean",
              "adv_mean", "adv_min", "adv_max", "adv_pos_frac", "exp_adv_mean", "exp_adv_clamped_frac",
              "grad_norm_vf", "grad_norm_qf", "grad_norm_actor")
EXP_ADV_MAX = 100.0


def row_terms(next_v, v, tq1, tq2, q1, q2, r, d, beta, discount, exp_adv_max=EXP_ADV_MAX):
    """Per-row quantities from the six head values of every row plus r and d: a dict of float64 arrays."""
    f = lambda x: np.asarray(x, dtype=np.float64).reshape(-1)
    next_v, v, tq1, tq2, q1, q2, r, d = map(f, (next_v, v, tq1, tq2, q1, q2, r, d))
    tq = np.minimum(tq1, tq2)
    adv = tq - v
    y = r + (1.0 - d) * float(discount) * next_v
    ex = np.exp(float(beta) * adv)
    return {"v": v, "next_v": next_v, "q1": q1, "q2": q2, "tq": tq, "adv": adv, "y": y, "exp": ex,
            "w": np.minimum(ex, float(exp_adv_max)), "clamped": ex >= float(exp_adv_max)}


def row_stats(next_v, v, tq1, tq2, q1, q2, r, d, beta, discount, exp_adv_max=EXP_ADV_MAX):
    """The 13 row statistics (float64), in STAT_NAMES order."""
    t = row_terms(next_v, v, tq1, tq2, q1, q2, r, d, beta, discount, exp_adv_max)
    adv = t["adv"]
    return np.array([t["v"].mean(), t["next_v"].mean(), t["q1"].mean(), t["q2"].mean(), t["tq"].mean(), t["y"].mean(),
                     np.abs(t["q1"] - t["q2"]).mean(), adv.mean(), adv.min(), adv.max(),
                     np.mean(~(adv < 0.0)),          # the side the value loss's weight takes: u < 0 is the other one
                     t["w"].mean(), np.mean(t["clamped"])], dtype=np.float64)


def losses_from_terms(t, iql_tau):
    """value_loss = mean(|iql_tau - 1(adv < 0)| adv^2) and q_loss = (mse(q1, y) + mse(q2, y)) / 2 from row_terms' own
    adv and y — what ties the restatement to the reference's recorded losses."""
    adv = t["adv"]
    value_loss = np.mean(np.abs(float(iql_tau) - (adv < 0.0).astype(np.float64)) * adv * adv)
    q_loss = 0.5 * (np.mean((t["q1"] - t["y"]) ** 2) + np.mean((t["q2"] - t["y"]) ** 2))
    return float(value_loss), float(q_loss)


def grad_norms(flat, segments):
    """The three gradient norms from a flat gradient and the layout's net segments: segments = [(begin, end)] in the
    library's net order V, Q1, Q2, pi; groups V | Q1 + Q2 | pi (log_std lives in pi's segment)."""
    g = np.asarray(flat, dtype=np.float64)
    ss = [float(np.sum(g[b:e] ** 2)) for b, e in segments]
    return np.sqrt(np.array([ss[0], ss[1] + ss[2], ss[3]], dtype=np.float64))
