"""The CPU statement of the ORDER of the prioritised loop (DESIGN.md 6j "Prioritised replay inside the chunk graphs") over
weighted_update_ref.Table: which table a draw sees.  Priorities are float64 (max(|e1|, |e2|) + eps) ** alpha rounded to
float32 — the order is what this module states, not the device's log2 / exp2 bits.

  lag-1 (the burst, and the eager loop it equals):     idx_0 = draw(0)
                                                       for t: idx_{t+1} = draw(t + 1); step t; table[idx_t] <- prio_t
  update first (what a loop WITHOUT the lag would do):  for t: step t; table[idx_t] <- prio_t; idx_{t+1} = draw(t + 1)

The TD errors of a step come from a network on the device; here a stand-in td_fn(t, idx, state) supplies them, `state`
a float the steps carry along (as parameters are): it depends on every batch so far, so two orders that draw different
batches see different TD errors for the same row, as on the device.
"""
import numpy as np

import weighted_update_ref as U


def priority64(td, alpha, eps):
    """float64 (max(|e1|, |e2|) + eps) ** alpha of TD errors [m, 2]."""
    td = np.asarray(td, dtype=np.float64)
    return (np.max(np.abs(td), axis=1) + float(eps)) ** float(alpha)


def model_td(base):
    """A TD model over per-row magnitudes base[n]: td[j] = (base[i] (1 + state), -base[i] / 2), and the new state."""
    base = np.asarray(base, dtype=np.float64)

    def td_fn(t, idx, state):
        e1 = base[idx] * (1.0 + state)
        td = np.stack([e1, -0.5 * base[idx]], axis=1)
        return td, state + 0.01 * float(np.mean(base[idx])) * (t + 1)
    return td_fn


def run_loop(table, n_steps, B, seed, offset, td_fn, alpha, eps, lag=True, state=0.0):
    """n_steps of the loop on `table` (a weighted_update_ref.Table, changed in place); step t's rows are indices
    [t B, (t + 1) B) of the stream (seed, offset).  Returns the list of index arrays the steps ran on."""
    bound = table.n
    batches = []
    idx = table.draw_indices(B, seed, offset, 0)
    for t in range(n_steps):
        nxt = table.draw_indices(B, seed, offset, (t + 1) * B) if lag else None
        td, state = td_fn(t, idx, state)
        batches.append(idx)
        table.update(idx, priority64(td, alpha, eps).astype(np.float32), bound)
        idx = nxt if lag else table.draw_indices(B, seed, offset, (t + 1) * B)
    return batches


# ---- the inputs of tests/test_hip_prioritized.py test 2, shared with tests/test_prioritized_cpu.py ---------------------
DUP_N, DUP_B, DUP_STEPS, DUP_SEED = 2000, 64, 6, 21
DUP_ROWS = np.array([3, 64, 65, 700, 701, 1300, 1919, 1999], dtype=np.int64)
DUP_MAX_WEIGHT = 64.0
DUP_ALPHA, DUP_EPS, DUP_BETA = 0.6, 1e-3, 0.5


def dup_weights():
    """Weight on 8 rows, the rest 0: every batch of 64 holds duplicates, every step redraws re-prioritised rows."""
    w = np.zeros(DUP_N, dtype=np.float32)
    w[DUP_ROWS] = np.array([0.5, 1.0, 2.0, 4.0, 0.25, 8.0, 1.5, 3.0], dtype=np.float32)
    return w
