"""Scoring transitions without a step: what ImplicitQLearning.score_buffer / score / evaluate check before they call
the library (iqlhip_score_rows).

Everything here is free of GPU work, so the refusals can be tested without one: the buffer and its row layout, the range
or index list that names the rows, the output tensor.  All of them are raised before anything is launched.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

import iqlhip_binding as hb

N_SCORE = hb.IQLHIP_N_SCORE
SUMMARY_KEYS = ("value_loss", "q_loss", "actor_loss") + tuple("mean_" + name for name in hb.SCORE_NAMES)


def check_buffer(buffer, device, state_dim: int, action_dim: int, row_stride: int) -> int:
    """A replay buffer on `device` (the trainer's GPU) with the trainer's dimensions and packed row stride that holds
    at least one row; returns the number of rows it holds.  ValueError otherwise."""
    rows = getattr(buffer, "_rows", None)
    if rows is None or not getattr(buffer, "_gpu", False) or rows.device != device:
        raise ValueError(f"iqlhip: score_buffer needs a ReplayBuffer that lives on the trainer's GPU ({device})")
    if buffer._state_dim != state_dim or buffer._action_dim != action_dim:
        raise ValueError(f"iqlhip: the buffer has state_dim={buffer._state_dim}, action_dim={buffer._action_dim}; the "
                         f"trainer has {state_dim}, {action_dim}")
    if buffer._ld != row_stride or rows.stride(0) != row_stride or rows.dtype != torch.float32:
        raise ValueError(f"iqlhip: the buffer's row stride {buffer._ld} is not the trainer's packed stride {row_stride}")
    size = int(buffer._size)
    if size < 1:
        raise ValueError("iqlhip: the replay buffer is empty")
    return size


def resolve_rows(size: int, start: int, n: Optional[int], indices) -> Tuple[int, int, Optional[object]]:
    """(start, n, indices) of the rows a call names: the range [start, start + n) of a buffer of `size` rows (n=None: to
    its end), or an index list — a 1-D int64 tensor or array, on the host or the device.  ValueError for an empty or
    overlong range and for both forms at once; IndexError for a host index outside [0, size) (a device list is checked
    by the library, on the device, in front of its first forward)."""
    if indices is not None:
        if start != 0 or n is not None:
            raise ValueError("iqlhip: give either start / n or indices, not both")
        if isinstance(indices, torch.Tensor):
            idx = indices
            if idx.dim() != 1 or idx.dtype != torch.int64:
                raise ValueError("iqlhip: indices must be a 1-D int64 tensor or array")
        else:
            idx = np.asarray(indices)
            if idx.ndim != 1 or idx.dtype != np.int64:
                raise ValueError("iqlhip: indices must be a 1-D int64 tensor or array")
        count = int(idx.shape[0])
        if count < 1:
            raise ValueError("iqlhip: an empty index list")
        if not (isinstance(idx, torch.Tensor) and idx.is_cuda):
            lo, hi = int(idx.min()), int(idx.max())
            if lo < 0 or hi >= size:
                raise IndexError(f"index {hi if hi >= size else lo} is out of bounds for dimension 0 with size {size}")
        return 0, count, idx
    start = int(start)
    count = size - start if n is None else int(n)
    if start < 0 or count < 1:
        raise ValueError(f"iqlhip: an empty range (start={start}, n={count})")
    if start + count > size:
        raise ValueError(f"iqlhip: rows [{start}, {start + count}) reach beyond the buffer's {size} rows")
    return start, count, None


def check_out(out, n: int, device) -> None:
    """A caller's output tensor: [n, 8] contiguous float32 on `device`."""
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != (n, N_SCORE):
        raise ValueError(f"iqlhip: out must be a [{n}, {N_SCORE}] tensor")
    if out.dtype != torch.float32 or out.device != device or not out.is_contiguous():
        raise ValueError(f"iqlhip: out must be a contiguous float32 tensor on {device}")


def check_chunk_rows(chunk_rows: Optional[int]) -> int:
    if chunk_rows is None:
        return 0
    chunk_rows = int(chunk_rows)
    if chunk_rows < 32 or chunk_rows % 32:
        raise ValueError(f"iqlhip: chunk_rows={chunk_rows} must be a positive multiple of 32")
    return chunk_rows


def summary_dict(words) -> Dict[str, float]:
    return {key: float(words[i]) for i, key in enumerate(SUMMARY_KEYS)}
