"""CPU restatement of iqlhip_rows_episode_returns (include/iqlhip.h; DESIGN.md "Episode spans, returns and
return-to-go") in numpy and Python floats, written for this project.  It restates get_return_to_go of the reference's
finetune/cal_ql.py and the episodes of keep_best_trajectories of offline/any_percent_bc.py.

  break         d[i] != 0, or (tol is not None) i + 1 < n and ss > tol * tol, where ss is the float64 sum, columns
                ascending, of the squared float32 differences s[i+1][c] - s'[i][c]
  episode end   a break, the T-th row of an episode, or (keep_tail) the last row of the range
  tail rows     of a trailing run that ends no episode: spans -1, values 0.0
  ep_return     Python float sum of the episode's float32 rewards, first row to last, from 0.0
  return_to_go  G[last] = r[last]; G[i] = r[i] + discount * G[i+1] in Python floats, downwards
  sparse        an episode whose last reward equals sparse_value: r[last] / (1.0 - discount) on all its rows
"""
from __future__ import annotations

import numpy as np


def breaks_ref(d, s=None, ns=None, tol=None):
    """Boolean break flags of n rows: done flags d, and (tol given) the state-discontinuity rule on states s [n, S] and
    next states ns [n, S]."""
    brk = np.asarray(d).reshape(-1) != 0
    n = brk.shape[0]
    if tol is not None and n > 1:
        s, ns = np.asarray(s, dtype=np.float32), np.asarray(ns, dtype=np.float32)
        delta = (s[1:] - ns[:-1]).astype(np.float64)            # the float32 difference, then exact in float64
        ss = np.zeros(n - 1, dtype=np.float64)
        for c in range(delta.shape[1]):                         # columns ascending; product and sum rounded separately
            ss = ss + delta[:, c] * delta[:, c]
        brk = brk.copy()
        brk[:-1] |= ss > float(tol) * float(tol)
    return brk


def episode_returns_rows_ref(r, brk, T, discount, keep_tail=False, sparse_value=None):
    """(ep_return float64[n], return_to_go float64[n], ep_first int64[n], ep_last int64[n], episodes) of rewards r with
    break flags brk (breaks_ref)."""
    r = np.asarray(r, dtype=np.float32).reshape(-1)
    brk = np.asarray(brk, dtype=bool).reshape(-1)
    n, T, discount = r.shape[0], int(T), float(discount)
    assert brk.shape == r.shape and T >= 1
    ep_return, rtg = np.zeros(n, np.float64), np.zeros(n, np.float64)
    ep_first, ep_last = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    rewards = r.tolist()                                        # (the exact float32 values as Python floats)
    episodes, first = 0, 0
    for i in range(n):
        if not (brk[i] or i - first + 1 == T or (keep_tail and i == n - 1)):
            continue
        acc = 0.0
        for j in range(first, i + 1):
            acc += rewards[j]
        if sparse_value is not None and rewards[i] == float(sparse_value):
            rtg[first: i + 1] = rewards[i] / (1.0 - discount)
        else:
            g = rewards[i]
            rtg[i] = g
            for j in range(i - 1, first - 1, -1):
                g = rewards[j] + discount * g
                rtg[j] = g
        ep_return[first: i + 1] = acc
        ep_first[first: i + 1], ep_last[first: i + 1] = first, i
        episodes += 1
        first = i + 1
    return ep_return, rtg, ep_first, ep_last, episodes


def rows_episode_returns_ref(rows, S, A, T, discount, tol=None, keep_tail=False, sparse_value=None):
    """The same from packed rows [s | a | s' | r | d | pad] (a numpy array [n, ld])."""
    rows = np.asarray(rows, dtype=np.float32)
    brk = breaks_ref(rows[:, 2 * S + A + 1], rows[:, :S], rows[:, S + A: 2 * S + A], tol)
    return episode_returns_rows_ref(rows[:, 2 * S + A], brk, T, discount, keep_tail, sparse_value)


def episode_table_ref(ep_return, rtg, ep_first, ep_last):
    """(first[E], last[E], ep_return[E], return_to_go at the first row [E]), one entry per episode in row order."""
    last = np.flatnonzero(np.asarray(ep_last) == np.arange(len(ep_last)))
    first = np.asarray(ep_first)[last]
    return first, last, np.asarray(ep_return)[last], np.asarray(rtg)[first]


def top_fraction_weights_ref(ep_return, rtg, ep_first, ep_last, frac, by="return_to_go"):
    """float32 [n]: 1.0 on the rows of the best max(1, int(frac * E)) episodes ranked by `by` descending, ties to the
    earlier episode; 0.0 elsewhere.  ValueError without an episode."""
    first, last, ret, g0 = episode_table_ref(ep_return, rtg, ep_first, ep_last)
    E = len(last)
    if E == 0:
        raise ValueError("no episode")
    value = {"return_to_go": g0, "ep_return": ret}[by]
    order = sorted(range(E), key=lambda e: (-value[e], e))
    w = np.zeros(len(ep_last), np.float32)
    for e in order[: max(1, int(frac * E))]:
        w[first[e]: last[e] + 1] = 1.0
    return w
