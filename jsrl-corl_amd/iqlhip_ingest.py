"""Dataset ingest on the device: the reduction behind `compute_mean_std`
(algorithms/finetune/iql.py:77-80) and the in-place `normalize_states` (:83-84) of a packed replay buffer, in
libiqlhip.so.  At 10 M rows the numpy forms cost seconds (two float32 passes plus temporaries of the dataset's size);
here the rows are uploaded once, reduced where they lie and normalised in place.

The reference's call order (finetune/iql.py:628-640: mean/std of the dataset -> normalise both state arrays -> load)
maps to:   buf.load_d4rl_dataset(raw);  mean, std = buf.state_mean_std(eps);  buf.normalize_states_(mean, std)
Numerics: the normalisation is bit-identical to numpy's given the same mean / std; the mean / std themselves are
float64-accumulated (deterministic, fixed order): within 1e-6 relative of a float64 evaluation, whereas numpy's own
float32 axis-0 reduction (row after row) drifts by ~2e-4 at 1 M rows — tolerances stated in tests/test_hip_ingest.py.  There is no CPU fallback here: the numpy functions of the reference's
surface (`compute_mean_std`, `normalize_states`) stay what they are for host arrays.

Reward ingest (`normalize_reward: true`, finetune/iql.py:262-289): `return_reward_range_device` scans the done column for
episode boundaries and sums every episode's rewards in float64 in row order, one thread per episode, so the (min, max)
it returns are the reference's Python floats bit for bit; `ReplayBuffer.modify_reward_` rescales the stored rewards with
them (load -> buf.modify_reward_(env_name, max_episode_steps)).  The host functions `return_reward_range` /
`modify_reward` of the drop-in modules stay what they are for host datasets.
"""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import numpy as np
import torch

import iqlhip_binding as hb


def _stream(dev: torch.device) -> int:
    return torch._C._cuda_getCurrentRawStream(dev.index)


def cols_mean_std(x: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """mean(0), std(0) + eps of a 2-D float32 device tensor whose rows may be strided (a column block of packed rows)."""
    if x.device.type != "cuda":
        raise RuntimeError("iqlhip: cols_mean_std needs a GPU tensor (numpy arrays: iql.compute_mean_std)")
    if x.dim() != 2 or x.dtype != torch.float32 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError("expected a float32 [n, cols] tensor with unit column stride")
    n, c = x.shape
    if n < 1:
        raise ValueError("no rows")
    mean = torch.empty(c, dtype=torch.float32, device=x.device)
    std = torch.empty(c, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        hb.check(hb.lib().iqlhip_cols_mean_std(x.data_ptr(), x.stride(0), c, n, float(eps), mean.data_ptr(),
                                               std.data_ptr(), _stream(x.device)))
    return mean, std


def compute_mean_std_device(states: np.ndarray, eps: float, device: str = "cuda") -> Tuple[np.ndarray, np.ndarray]:
    """compute_mean_std for a host array through the device reduction (chunked upload, float64 accumulation)."""
    x = torch.as_tensor(np.ascontiguousarray(states, dtype=np.float32)).to(device, non_blocking=False)
    mean, std = cols_mean_std(x, eps)
    return mean.cpu().numpy(), std.cpu().numpy()


def return_reward_range_device(rows: torch.Tensor, state_dim: int, action_dim: int, n: int,
                               max_episode_steps: int) -> Tuple[float, float]:
    """return_reward_range (finetune/iql.py:262-274) over the first n rows of a packed device row store
    [s | a | s' | r | d | pad]: (min, max) of the returns of the complete episodes, in storage order.  Raises ValueError
    when there is no complete episode, like the reference's min([]).  Synchronises the current stream."""
    if rows.device.type != "cuda":
        raise RuntimeError("iqlhip: return_reward_range_device needs a GPU tensor (host datasets: iql.return_reward_range)")
    if rows.dim() != 2 or rows.dtype != torch.float32 or rows.stride(1) != 1:
        raise ValueError("expected a float32 [rows, ld] tensor with unit column stride")
    if n < 1 or n > rows.shape[0]:
        raise ValueError("n outside the row store")
    out = (C.c_double * 2)()
    episodes = C.c_int64(0)
    with torch.cuda.device(rows.device):
        hb.check(hb.lib().iqlhip_rows_return_range(rows.data_ptr(), rows.stride(0), state_dim, action_dim, 0, n,
                                                   int(max_episode_steps), out, C.byref(episodes), _stream(rows.device)))
    return float(out[0]), float(out[1])
