"""CPU restatement of the reward ingest (iqlhip_rows_return_range / _reward_scale / _reward_shift; DESIGN.md "Reward
ingest"): the semantics of return_reward_range / modify_reward (algorithms/finetune/iql.py:262-289) in numpy and Python
floats, written for this project.

  episode ends      at a row whose done flag is non-zero, or at the max_episode_steps-th row of its episode
  episode return    Python float (float64) sum of the episode's float32 rewards, added row after row from 0.0
  trailing rows     that end neither way are no episode
  rescaling         float32: r / float32(max_ret - min_ret), then * float32(max_episode_steps)   (two roundings)
  antmaze           float32: r - 1
"""
from __future__ import annotations

import numpy as np

LOCOMOTION = ("halfcheetah", "hopper", "walker2d")


def episode_returns_ref(r, d, T):
    """The returns of the complete episodes of rewards r / done flags d in row order, as a list of Python floats."""
    r = np.asarray(r, dtype=np.float32).reshape(-1)
    d = np.asarray(d).reshape(-1)
    assert r.shape == d.shape and int(T) >= 1
    returns, acc, length = [], 0.0, 0
    for reward, done in zip(r.tolist(), (d != 0).tolist()):       # (tolist of float32 -> the exact values as Python floats)
        acc += reward
        length += 1
        if done or length == int(T):
            returns.append(acc)
            acc, length = 0.0, 0
    return returns


def return_reward_range_ref(r, d, T):
    """(min, max) of the episode returns; ValueError when there is no complete episode (the reference's min([]))."""
    returns = episode_returns_ref(r, d, T)
    if not returns:
        raise ValueError("no complete episode")
    return min(returns), max(returns)


def modify_reward_ref(r, d, env_name, T=1000):
    """(modified float32 rewards — a new array —, the dict modify_reward returns)."""
    r = np.array(r, dtype=np.float32).reshape(-1)
    if any(s in env_name for s in LOCOMOTION):
        min_ret, max_ret = return_reward_range_ref(r, d, T)
        r = r / np.float32(max_ret - min_ret)
        r = r * np.float32(T)
        assert r.dtype == np.float32
        return r, {"max_ret": max_ret, "min_ret": min_ret, "max_episode_steps": T}
    if "antmaze" in env_name:
        return r - np.float32(1.0), {}
    return r, {}
