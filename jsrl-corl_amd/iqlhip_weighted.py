"""Weighted replay sampling: what a weight vector must look like and what the weighted calls refuse.

`ReplayBuffer.set_sample_weights(w)` attaches one float32 weight per row position to a GPU buffer; the library turns it
into a cumulative table of integers on the device (include/iqlhip.h "weighted replay sampling"), and
`draw_weighted_indices`, `sample_weighted` and `ImplicitQLearning.train_steps_weighted` draw rows by it from the index
stream of `train_steps`, unchanged.  Row i is drawn with probability q[i] / sum(q), q[i] = floor(w[i] * 2^(38 - e)),
e = floor(log2(max w)): a weight below max(w) * 2^-39 quantises to 0 and its row is never drawn.

Weights belong to row POSITIONS: writes into the buffer leave them alone; a change of the buffer's index bound makes the
weighted calls refuse until weights are set again.  Every other call (train_steps, sample, online_step, groups, mixed
batches) ignores them.

The argument checks live here, free of any GPU work, so they can be tested without one.
"""
from __future__ import annotations

import numpy as np

MAX_ROWS = 1 << 24            # IQLHIP_WEIGHTS_MAX_ROWS (include/iqlhip.h)


def check_vector(weights, n: int):
    """The shape, dtype and length checks of set_sample_weights (no look at the values, which may live on the device):
    a 1-D float32 torch tensor or ndarray of n = the buffer's index bound entries, 1 <= n <= 2^24.  ValueError
    otherwise.  Returns "torch" or "numpy"."""
    import torch
    if n < 1:
        raise ValueError("iqlhip: the replay buffer is empty: there is no row to weigh")
    if n > MAX_ROWS:
        raise ValueError(f"iqlhip: weighted sampling covers at most 2^24 rows (the buffer draws over {n})")
    if isinstance(weights, torch.Tensor):
        kind, is_f32 = "torch", weights.dtype == torch.float32
    elif isinstance(weights, np.ndarray):
        kind, is_f32 = "numpy", weights.dtype == np.float32
    else:
        raise ValueError(f"iqlhip: sample weights must be a torch tensor or a numpy array, not {type(weights).__name__}")
    if not is_f32:
        raise ValueError(f"iqlhip: sample weights must be float32 (got {weights.dtype})")
    if weights.ndim != 1:
        raise ValueError(f"iqlhip: sample weights must be one-dimensional (got shape {tuple(weights.shape)})")
    if weights.shape[0] != n:
        raise ValueError(f"iqlhip: {weights.shape[0]} sample weights for a buffer that draws over {n} rows")
    return kind


def check_host_values(w: np.ndarray) -> None:
    """The value checks on a host vector (the library makes the same ones on the device): all finite, all >= 0, at
    least one > 0.  ValueError otherwise."""
    if not np.all(np.isfinite(w)):
        raise ValueError("iqlhip: sample weights hold a NaN or an infinity")
    if np.any(w < 0):
        raise ValueError("iqlhip: sample weights hold a negative value")
    if not np.any(w > 0):
        raise ValueError("iqlhip: all sample weights are zero")


def check_call(buffer) -> int:
    """What every weighted call checks on the buffer before anything is launched: it lives on a GPU, has weights, and
    still draws over the number of rows they were set for.  Returns that number."""
    if not getattr(buffer, "_gpu", False):
        raise ValueError("iqlhip: weighted sampling needs a ReplayBuffer that lives on the GPU")
    n = buffer.sample_weights_n
    if n is None:
        raise ValueError("iqlhip: the replay buffer has no sample weights (set_sample_weights)")
    if buffer._index_bound() != n:
        raise ValueError(f"iqlhip: the sample weights were set for {n} rows, the buffer now draws over "
                         f"{buffer._index_bound()}: call set_sample_weights again")
    return n


def check_trainer(dp_world: int, dp_exchange, precision: str, batch_size: int, bf16_max_rows: int) -> None:
    """train_steps_weighted's refusals that need no library call: NotImplementedError under data parallelism and for
    bf16 batches beyond the small-batch kernels."""
    if dp_world > 1 or dp_exchange is not None:
        raise NotImplementedError("iqlhip: weighted sampling is not supported under data parallelism")
    if precision == "bf16" and batch_size > bf16_max_rows:
        raise NotImplementedError(f"iqlhip: weighted sampling is not supported for bf16 batches of more than "
                                  f"{bf16_max_rows} rows (got {batch_size}): the large-batch kernels draw uniformly")
