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

Episode returns (`episode_returns_device`, `EpisodeReturns`): every row's episode span, episode return
and discounted return-to-go as device tensors — get_return_to_go of finetune/cal_ql.py and the episodes of
keep_best_trajectories of offline/any_percent_bc.py — for `set_sample_weights` or next to `score_buffer`'s columns.
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


class EpisodeReturns:
    """What `episode_returns_device` computed, as device tensors over the n rows it covered: `ep_return` and
    `return_to_go` (float64 [n]), `ep_first` and `ep_last` (int64 [n], -1 on tail rows that belong to no episode), and
    `episodes` (int)."""

    def __init__(self, ep_return, return_to_go, ep_first, ep_last, episodes: int):
        self.ep_return, self.return_to_go = ep_return, return_to_go
        self.ep_first, self.ep_last = ep_first, ep_last
        self.episodes = int(episodes)

    def episode_table(self):
        """(first[E], last[E], ep_return[E], return_to_go_at_first[E]): one entry per episode in row order, compacted on
        the device at the rows that end an episode.  return_to_go at an episode's first row is its discounted return."""
        n = self.ep_last.shape[0]
        last = torch.nonzero(self.ep_last == torch.arange(n, device=self.ep_last.device)).reshape(-1)
        first = self.ep_first[last]
        return first, last, self.ep_return[last], self.return_to_go[first]

    def top_fraction_weights(self, frac: float, by: str = "return_to_go") -> torch.Tensor:
        """float32 [n] sampling weights: 1.0 on the rows of the best max(1, int(frac * E)) episodes, 0.0 elsewhere —
        keep_best_trajectories (offline/any_percent_bc.py) as a distribution for set_sample_weights instead of a
        rewritten dataset.  Episodes are ranked by `by` descending ("return_to_go": the value at the episode's first
        row; or "ep_return"), ties going to the earlier episode."""
        if by not in ("return_to_go", "ep_return"):
            raise ValueError('by must be "return_to_go" or "ep_return"')
        if self.episodes == 0:
            raise ValueError("no episode to rank")
        _, last, ret, g0 = self.episode_table()
        order = torch.sort(g0 if by == "return_to_go" else ret, descending=True, stable=True).indices
        keep = order[: max(1, int(frac * last.shape[0]))]
        at_last = torch.zeros(self.ep_last.shape[0], dtype=torch.float32, device=self.ep_last.device)
        at_last[last[keep]] = 1.0
        w = at_last[self.ep_last.clamp(min=0)]
        return torch.where(self.ep_last >= 0, w, torch.zeros_like(w))


def episode_returns_device(rows: torch.Tensor, state_dim: int, action_dim: int, n: int, max_episode_steps: int,
                           discount: float, state_break_tol=None, keep_tail: bool = False, sparse_value=None,
                           row0: int = 0) -> EpisodeReturns:
    """Per-row episode spans, returns and discounted return-to-go of rows [row0, row0 + n) of a packed device row store,
    in storage order (iqlhip_rows_episode_returns; include/iqlhip.h states the arithmetic): get_return_to_go of the
    reference's finetune/cal_ql.py (state_break_tol=1e-6, keep_tail=True) and the episodes of keep_best_trajectories of
    offline/any_percent_bc.py (both off).  Reads only.  Synchronises the current stream."""
    if rows.device.type != "cuda":
        raise RuntimeError("iqlhip: episode_returns_device needs a GPU tensor")
    if rows.dim() != 2 or rows.dtype != torch.float32 or rows.stride(1) != 1:
        raise ValueError("expected a float32 [rows, ld] tensor with unit column stride")
    if n < 1 or row0 < 0 or row0 + n > rows.shape[0]:
        raise ValueError("[row0, row0 + n) outside the row store")
    dev = rows.device
    ep_return = torch.empty(n, dtype=torch.float64, device=dev)
    return_to_go = torch.empty(n, dtype=torch.float64, device=dev)
    ep_first = torch.empty(n, dtype=torch.int64, device=dev)
    ep_last = torch.empty(n, dtype=torch.int64, device=dev)
    episodes = C.c_int64(0)
    sparse = None if sparse_value is None else C.byref(C.c_double(float(sparse_value)))
    with torch.cuda.device(dev):
        hb.check(hb.lib().iqlhip_rows_episode_returns(
            rows.data_ptr(), rows.stride(0), state_dim, action_dim, int(row0), int(n), int(max_episode_steps),
            float(discount), -1.0 if state_break_tol is None else float(state_break_tol),
            hb.IQLHIP_EP_KEEP_TAIL if keep_tail else 0, sparse, ep_return.data_ptr(), return_to_go.data_ptr(),
            ep_first.data_ptr(), ep_last.data_ptr(), C.byref(episodes), _stream(dev)))
    return EpisodeReturns(ep_return, return_to_go, ep_first, ep_last, episodes.value)
