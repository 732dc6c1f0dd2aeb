"""N-step returns on the device (include/iqlhip.h "n-step rows"): a DERIVED replay buffer whose rows the
unchanged IQL step reads as k-step transitions, built and kept current in libiqlhip.so.

Every kernel that forms a TD target computes  y = r + ((1 - d) * discount) * V(s').  A derived row holds the discounted
reward sum of k <= n rows in r, the state k rows ahead in s' and  d = 1 - discount^(k - 1) * (1 - d_last),  so the same
expression yields  sum_t discount^t r_t + discount^k (1 - d_last) V(s_{t+k}).  `NStepReplay.buffer` is an ordinary GPU
ReplayBuffer: train, train_steps*, weighted and prioritised draws, mixed batches, score_buffer and trainer groups take
it as it is.  Its `sample().dones` therefore holds FRACTIONS by design (0 only for k = 1), not flags.

    nstep = raw.nstep(3, 0.99, episodes=raw.episode_returns(1000, 0.99, state_break_tol=1e-6, keep_tail=True))
    trainer.train_steps(nstep.buffer, 256, 1000)                       # offline, 3-step targets
    nstep.add_transition(s, a, r, s2, real_done, episode_end=done)     # online: raw ring write + ring refresh
    log, a = trainer.online_step_nstep(nstep, s, a, r, s2, real_done, 256, episode_end=done, act_next=s2)

The `discount` given here must be the trainer's.  There is no CPU path."""
from __future__ import annotations

import math
from typing import Optional

import torch

import iqlhip_binding as hb
import iqlhip_dp as dp
from iqlhip_replay import check_online_ring, draw_indices

MAX_HORIZON = hb.IQLHIP_NSTEP_MAX_HORIZON


def check_args(n, discount) -> tuple:
    """(n, discount) as (int, float); ValueError with the cause for a horizon outside [1, 64] or a discount that is not
    finite or outside (0, 1].  Nothing is launched."""
    if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= MAX_HORIZON:
        raise ValueError(f"iqlhip: n-step horizon n = {n!r} outside [1, {MAX_HORIZON}]")
    discount = float(discount)
    if not math.isfinite(discount) or not 0.0 < discount <= 1.0:
        raise ValueError(f"iqlhip: n-step discount = {discount!r} must be finite and in (0, 1]")
    return int(n), discount


def check_episodes(episodes, size: int):
    """The ep_last column of an EpisodeReturns over `size` rows (None: no table); ValueError for another length."""
    if episodes is None:
        return None
    ep_last = episodes.ep_last
    if ep_last.dim() != 1 or ep_last.shape[0] != size:
        raise ValueError(f"iqlhip: the episodes table covers {tuple(ep_last.shape)} rows, the replay buffer holds {size} "
                         "(take it from raw.episode_returns(...) of the same rows)")
    if ep_last.dtype != torch.int64:
        raise ValueError("iqlhip: episodes.ep_last must be int64")
    return ep_last.contiguous()


class NStepReplay:
    """A raw GPU ReplayBuffer and the n-step buffer derived from it.  `raw`: the source; `buffer`: a GPU ReplayBuffer of
    the same dimensions and capacity whose _size and _pointer follow the raw buffer's; `steps`: uint8 [capacity], the k
    of every derived row; `n`, `discount`: the parameters.  `episodes` (an EpisodeReturns of raw.episode_returns(...)):
    its ep_last keeps chains inside episodes that end by time limit or state discontinuity; without it only `done` and
    the end of the data break a chain.  Rows added later carry their own end flag (add_transition's episode_end)."""

    def __init__(self, raw_buffer, n: int, discount: float, episodes=None):
        if not getattr(raw_buffer, "_gpu", False):
            raise NotImplementedError("iqlhip: n-step rows are built in libiqlhip.so and need a ReplayBuffer that lives on the GPU")
        self.n, self.discount = check_args(n, discount)
        self.raw = raw_buffer
        raw = raw_buffer
        self.buffer = type(raw)(raw._state_dim, raw._action_dim, raw._buffer_size, raw._device)
        dev = raw._rows.device
        self.steps = torch.zeros(raw._buffer_size, dtype=torch.uint8, device=dev)
        # one byte per ring position: the stored row ends an episode (rows a build covered: from `episodes`)
        self.ends = torch.zeros(raw._buffer_size, dtype=torch.uint8, device=dev)
        self.rebuild(episodes)

    def _sync_counters(self) -> None:
        self.buffer._size, self.buffer._pointer = self.raw._size, self.raw._pointer

    def rebuild(self, episodes=None) -> None:
        """Build the derived rows [0, raw size) again, in storage order — after modify_reward_ or normalize_states_ on the
        raw buffer (a loaded dataset, not a wrapped ring).  One launch on the raw buffer's stream."""
        raw, buf = self.raw, self.buffer
        size = raw._size
        ep_last = check_episodes(episodes, size)
        self._sync_counters()
        if size < 1:
            return
        if ep_last is not None and ep_last.device != raw._rows.device:
            raise ValueError(f"iqlhip: the episodes table lives on {ep_last.device}, the buffer on {raw._rows.device}")
        buf._writes += 1
        with torch.cuda.device(raw._rows.device):
            hb.check(hb.lib().iqlhip_rows_nstep(raw._rows.data_ptr(), raw._ld, buf._rows.data_ptr(), buf._ld, raw._state_dim,
                                                raw._action_dim, 0, size, self.n, self.discount,
                                                None if ep_last is None else ep_last.data_ptr(), self.steps.data_ptr(),
                                                raw._stream()))
            if ep_last is None:
                self.ends[:size] = 0
            else:
                self.ends[:size] = (ep_last == torch.arange(size, device=ep_last.device)).to(torch.uint8)

    def add_transition(self, state, action, reward: float, next_state, done: bool, episode_end: Optional[bool] = None):
        """raw.add_transition(...), then the ring refresh on the same stream: the at most n derived rows the new
        transition extends.  episode_end (default: done): the environment's `done`, time-outs included, next to the
        stored real_done."""
        raw, buf = self.raw, self.buffer
        end = bool(done) if episode_end is None else bool(episode_end)
        pointer = raw._pointer
        raw.add_transition(state, action, reward, next_state, done)
        buf._writes += 1
        with torch.cuda.device(raw._rows.device):
            self.ends[pointer: pointer + 1].fill_(int(end))
            hb.check(hb.lib().iqlhip_rows_nstep_ring(raw._rows.data_ptr(), buf._rows.data_ptr(), raw._ld, raw._state_dim,
                                                     raw._action_dim, raw._buffer_size, raw._size, pointer,
                                                     self.ends.data_ptr(), self.n, self.discount, self.steps.data_ptr(),
                                                     raw._stream()))
        if buf._weights_tracks:              # behind the refresh, on the same stream: the new row at the running maximum
            buf.insert_max_sample_weight(pointer)
        self._sync_counters()


def online_step_nstep(trainer, nstep: NStepReplay, state, action, reward, next_state, done, batch_size: int,
                      episode_end=None, act_next=None):
    """ImplicitQLearning.online_step_nstep (iqlhip_trainer.py): nstep.add_transition(...), nstep.buffer.sample(B) and
    train() in one library call and under one synchronisation, bit for bit."""
    self = trainer
    if not isinstance(nstep, NStepReplay):
        raise ValueError("online_step_nstep needs an NStepReplay (raw.nstep(n, discount))")
    if self._dp_world > 1 or self._dp_exchange is not None:
        raise NotImplementedError("iqlhip: online_step_nstep is not supported under data parallelism "
                                  "(use nstep.add_transition / nstep.buffer.sample / train)")
    self._prepare(batch_size)
    raw, buf = nstep.raw, nstep.buffer
    check_online_ring(raw, self._dev, "online_step_nstep", holder="an NStepReplay")
    if buf._weights_tracks:
        raise NotImplementedError("iqlhip: online_step_nstep does not enter the new row into a tracking sample-weight table "
                                  "(use nstep.add_transition, then the prioritised calls)")
    end = bool(done) if episode_end is None else bool(episode_end)
    new_size = raw._insert_slot()[1]     # (the library takes it next to the pointer; the driver's draw runs over the same)

    def call(ring_args, row, idx, sc, out, act_args, stream):      # (the driver's ring is the raw one)
        raw_rows, ld, capacity, pointer = ring_args
        return hb.lib().iqlhip_online_step_nstep(self._ctx, raw_rows, buf._rows.data_ptr(), ld, capacity, pointer, row, idx,
                                                 batch_size, sc, out, *act_args, stream, nstep.ends.data_ptr(), int(end),
                                                 new_size, nstep.n, nstep.discount, nstep.steps.data_ptr())

    def commit_extra():                  # (the raw ring has moved: the derived one follows it)
        buf._writes += 1
        nstep._sync_counters()
    return self._run_online(raw, (state, action, reward, next_state, done), act_next,
                            lambda bound: draw_indices(bound, batch_size), dp.inv_batch(batch_size, self._dp_world),
                            call, commit_extra)
