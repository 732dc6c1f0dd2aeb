"""Scoring transitions without a step: what ImplicitQLearning.score_buffer / score / evaluate — and their
ImplicitQLearningGroup forms — check before they call the library (iqlhip_score_rows, iqlhip_group_score_rows;
DESIGN.md 6h).

Everything here is free of GPU work, so the refusals can be tested without one: the buffer and its row layout, the range
or index list that names the rows, the output tensor.  All of them are raised before anything is launched.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

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


# ---- trainer groups (ImplicitQLearningGroup.score_buffer / score / evaluate) --------------------------------------
def group_buffers(buffers, K: int) -> Tuple[List[object], bool]:
    """`buffers` — one buffer for all K members, or a list of K — as K buffers, and whether all members read one."""
    if isinstance(buffers, (list, tuple)):
        bufs = list(buffers)
        if len(bufs) != K:
            raise ValueError(f"iqlhip: {len(bufs)} buffers for a group of {K} (one shared buffer, or one per member)")
    else:
        bufs = [buffers] * K
    return bufs, all(b is bufs[0] for b in bufs)


def _is_index_list(x) -> bool:
    return isinstance(x, (torch.Tensor, np.ndarray, list, tuple))


def group_rows(sizes: Sequence[int], start: int, n: Optional[int], indices) -> Tuple[int, int, Optional[List[object]], bool]:
    """(start, n, index lists, shared) of the rows a group call names in buffers of `sizes` rows.  A range must fit the
    smallest buffer.  indices: one list for all members, or a list / tuple of K lists (arrays or tensors) of equal
    length, each checked against its own member's buffer as resolve_rows checks one.  shared: all members use one list
    (or the range)."""
    K = len(sizes)
    if indices is None:
        start, count, _ = resolve_rows(min(sizes), start, n, None)
        return start, count, None, True
    per_member = isinstance(indices, (list, tuple)) and len(indices) > 0 and all(_is_index_list(x) for x in indices)
    if per_member:
        lists = list(indices)
        if len(lists) != K:
            raise ValueError(f"iqlhip: {len(lists)} index lists for a group of {K} (one shared list, or one per member)")
    else:
        lists = [indices] * K
    out, count = [], None
    for k, (size, lst) in enumerate(zip(sizes, lists)):
        if not per_member and k > 0 and size == sizes[0]:
            out.append(out[0])           # (one list, buffers of one size: checked once)
            continue
        _, c, idx = resolve_rows(size, start, n, lst)
        if count is not None and c != count:
            raise ValueError(f"iqlhip: index list {k} names {c} rows, list 0 names {count} (one length for all members)")
        count = c if count is None else count
        out.append(idx)
    return 0, count, out, not per_member


def check_group_out(out, K: int, n: int, device) -> None:
    """A caller's output tensor of a group call: [K, n, 8] contiguous float32 on `device`."""
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != (K, n, N_SCORE):
        raise ValueError(f"iqlhip: out must be a [{K}, {n}, {N_SCORE}] tensor")
    if out.dtype != torch.float32 or out.device != device or not out.is_contiguous():
        raise ValueError(f"iqlhip: out must be a contiguous float32 tensor on {device}")


def check_spread(spread, n: int, device) -> None:
    """A caller's spread tensor: [n, 16] contiguous float32 on `device`."""
    if not isinstance(spread, torch.Tensor) or tuple(spread.shape) != (n, 2 * N_SCORE):
        raise ValueError(f"iqlhip: spread must be True, False or a [{n}, {2 * N_SCORE}] tensor")
    if spread.dtype != torch.float32 or spread.device != device or not spread.is_contiguous():
        raise ValueError(f"iqlhip: spread must be a contiguous float32 tensor on {device}")


def check_group_outputs(out, summary: bool, spread, shared_rows: bool, K: int, n: int, device) -> None:
    """out / summary / spread of a group call.  The spread is across the members' scores of THE SAME rows: it is
    refused when the members name rows of their own."""
    wants_spread = spread is not None and spread is not False
    if wants_spread and not shared_rows:
        raise ValueError("iqlhip: spread needs all members to score the same rows (one buffer with one index list or a "
                         "range, or one shared batch)")
    if out is not None and out is not False:
        check_group_out(out, K, n, device)
    if wants_spread and spread is not True:
        check_spread(spread, n, device)
    if out is False and not summary and not wants_spread:
        raise ValueError("iqlhip: nothing to compute (out=False, summary=False and spread=False)")
