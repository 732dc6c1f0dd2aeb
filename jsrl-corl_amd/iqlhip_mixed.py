"""Mixed offline / online batches: what a batch drawn from two replay buffers means.

The reference's Cal-QL fine-tuning loop (algorithms/finetune/cal_ql.py: `mixing_ratio`) builds every batch as
`vstack(offline_buffer.sample(n_off), online_buffer.sample(n_on))` with `n_off = int(batch_size * mixing_ratio)`.
ImplicitQLearning.online_step_mixed and train_steps_mixed do the same inside one library call; the split, the checks on
the two buffers and the host index draw live here, free of any GPU work, so they can be tested without one.

Batch rows [0, n_off) come from the offline buffer, rows [n_off, batch_size) from the online buffer (the vstack order).
"""
from __future__ import annotations

from typing import Tuple

import numpy as np


def split(batch_size: int, mixing_ratio: float) -> Tuple[int, int]:
    """(n_off, n_on) of a batch: Cal-QL's `int(batch_size * mixing_ratio)` offline rows, the rest online.  Both parts
    must be non-empty — a batch from one buffer only is what the plain calls are for."""
    batch_size = int(batch_size)
    n_off = int(batch_size * mixing_ratio)
    if not 1 <= n_off <= batch_size - 1:
        raise ValueError(f"iqlhip: mixing_ratio={mixing_ratio} gives {n_off} offline rows of batch_size={batch_size}; a "
                         "mixed batch needs 1 <= n_off <= batch_size - 1 — for a batch from a single buffer use the "
                         "plain call (online_step / train_steps)")
    return n_off, batch_size - n_off


def check_buffers(offline_buffer, online_buffer, device, state_dim: int, action_dim: int) -> None:
    """Both buffers: finetune-flavour ReplayBuffers on `device` (the trainer's GPU) with the trainer's dimensions — hence
    one packed row stride — and two distinct objects.  ValueError otherwise, before anything is launched or moves."""
    from iqlhip_replay import ReplayBuffer
    if offline_buffer is online_buffer:
        raise ValueError("iqlhip: a mixed batch needs two distinct replay buffers (got the same object twice)")
    for name, buf in (("offline_buffer", offline_buffer), ("online_buffer", online_buffer)):
        if not isinstance(buf, ReplayBuffer) or type(buf)._index_bound is not ReplayBuffer._index_bound \
                or type(buf).add_transition is not ReplayBuffer.add_transition:
            raise ValueError(f"iqlhip: {name} must be a finetune ReplayBuffer (the offline flavour bounds its draw "
                             "differently and has no add_transition)")
        if not getattr(buf, "_gpu", False) or buf._rows.device != device:
            raise ValueError(f"iqlhip: {name} must live on the trainer's GPU ({device})")
        if buf._state_dim != state_dim or buf._action_dim != action_dim:
            raise ValueError(f"iqlhip: {name} has state_dim={buf._state_dim}, action_dim={buf._action_dim}; the trainer "
                             f"has {state_dim}, {action_dim}")
    if offline_buffer._ld != online_buffer._ld:          # (follows from the dimensions; the kernels rely on it)
        raise ValueError("iqlhip: the two buffers have different packed row strides")


def draw_host_indices(size_off: int, n_off: int, size_on: int, n_on: int, rng=None) -> Tuple[np.ndarray, np.ndarray]:
    """The reference's draw from the global numpy RNG, in its order: the offline sample() first, then the online one
    (over the online buffer's size AFTER this iteration's insert).  int64 arrays (idx_off, idx_on).  rng: a
    np.random.RandomState to draw from instead (a trainer group's member with a stream of its own)."""
    if size_off < 1:
        raise ValueError("iqlhip: the offline replay buffer is empty")
    rng = np.random if rng is None else rng
    idx_off = rng.randint(0, size_off, size=n_off)
    idx_on = rng.randint(0, size_on, size=n_on)
    return idx_off.astype(np.int64, copy=False), idx_on.astype(np.int64, copy=False)
