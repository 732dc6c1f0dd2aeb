"""ReplayBuffer with the reference's surface (algorithms/finetune/iql.py:122-197)
on top of ONE packed row store  [s(S) | a(A) | s'(S) | r | d | pad]  (row stride
a multiple of 16 B) instead of five separate tensors, so that a sampled
transition is one contiguous 168..448-byte read instead of five 4..156-byte ones.

On a GPU device the row writes and the five-way gather of `sample` run in
libiqlhip.so (iqlhip_rows_write / iqlhip_rows_gather); the index draw stays
`np.random.randint` on the host exactly like the reference (iql.py:172), so a
seeded run draws the same index stream.  On a CPU device (no GPU in the
process: host-logic tests, config-1 plumbing) the same storage is addressed
with torch indexing; the training step itself has no CPU path.
"""
from __future__ import annotations

from typing import Dict, List

import ctypes as C
import os

import numpy as np
import torch

import iqlhip_binding as hb

TensorBatch = List[torch.Tensor]

# (data_ptr of the observations view, rows, S, A, row stride, device) of the block the last GPU sample() produced
_last_block = None
# sample(): packed blocks (and their five views) recycled per batch size; 0 = a fresh block per call
SAMPLE_RING = max(0, int(os.environ.get("IQLHIP_SAMPLE_RING", "8")))


def _is_gpu(device) -> bool:
    return torch.device(device).type == "cuda"


try:
    _raw_stream = torch._C._cuda_getCurrentRawStream          # (device_index) -> hipStream_t as int
except AttributeError:                                        # pragma: no cover - older torch
    def _raw_stream(index: int) -> int:
        return torch.cuda.current_stream(index).cuda_stream


class ReplayBuffer:
    def __init__(self, state_dim: int, action_dim: int, buffer_size: int, device: str = "cpu"):
        self._buffer_size = buffer_size
        self._pointer = 0
        self._size = 0
        self._state_dim = state_dim
        self._action_dim = action_dim
        self._device = device
        self._gpu = _is_gpu(device)
        w = 2 * state_dim + action_dim + 2
        self._ld = hb.row_stride(state_dim, action_dim) if self._gpu else (w + 3) // 4 * 4
        self._rows = torch.zeros((buffer_size, self._ld), dtype=torch.float32, device=device)
        self._rows_ptr = self._rows.data_ptr()
        pad = self._ld - w
        self._split_sizes = [state_dim, action_dim, state_dim, 1, 1] + ([pad] if pad else [])
        self._sample_ring = {}      # batch size -> [[(block, five views, block address)] * SAMPLE_RING, next slot]
        # bumped by every method that writes rows: ImplicitQLearning.train_steps may start a call on rows its previous
        # call staged ahead only while the buffer's contents are what they were then
        self._writes = 0

    # ---- views with the reference's attribute names (iql.py:134-146) ------
    @property
    def _states(self) -> torch.Tensor:
        return self._rows[:, : self._state_dim]

    @property
    def _actions(self) -> torch.Tensor:
        return self._rows[:, self._state_dim: self._state_dim + self._action_dim]

    @property
    def _next_states(self) -> torch.Tensor:
        o = self._state_dim + self._action_dim
        return self._rows[:, o: o + self._state_dim]

    @property
    def _rewards(self) -> torch.Tensor:
        o = 2 * self._state_dim + self._action_dim
        return self._rows[:, o: o + 1]

    @property
    def _dones(self) -> torch.Tensor:
        o = 2 * self._state_dim + self._action_dim + 1
        return self._rows[:, o: o + 1]

    def _to_tensor(self, data: np.ndarray) -> torch.Tensor:
        return torch.tensor(data, dtype=torch.float32, device=self._device)

    def _stream(self):
        return _raw_stream(self._rows.device.index)

    def _write_rows(self, row0: int, s, a, r, ns, d) -> None:
        n = s.shape[0]
        self._writes += 1
        if self._gpu:
            s, a, r, ns, d = (t.contiguous() for t in (s, a, r, ns, d))
            hb.check(hb.lib().iqlhip_rows_write(
                self._rows.data_ptr(), self._ld, self._state_dim, self._action_dim, row0, n,
                s.data_ptr(), a.data_ptr(), r.data_ptr(), ns.data_ptr(), d.data_ptr(), self._stream()))
        else:
            S, A = self._state_dim, self._action_dim
            blk = self._rows[row0: row0 + n]
            blk[:, :S] = s
            blk[:, S: S + A] = a
            blk[:, S + A: 2 * S + A] = ns
            blk[:, 2 * S + A] = r.reshape(-1)
            blk[:, 2 * S + A + 1] = d.reshape(-1)

    # Loads data in d4rl format, i.e. from Dict[str, np.array] (iql.py:153-169).
    def load_d4rl_dataset(self, data: Dict[str, np.ndarray]):
        if self._size != 0:
            raise ValueError("Trying to load data into non-empty replay buffer")
        n_transitions = data["observations"].shape[0]
        if n_transitions > self._buffer_size:
            raise ValueError("Replay buffer is smaller than the dataset you are trying to load!")
        chunk = 1 << 20  # bound the staging copies for 10M-row datasets
        for lo in range(0, n_transitions, chunk):
            hi = min(lo + chunk, n_transitions)
            self._write_rows(
                lo,
                self._to_tensor(data["observations"][lo:hi]),
                self._to_tensor(data["actions"][lo:hi]),
                self._to_tensor(data["rewards"][lo:hi]),
                self._to_tensor(data["next_observations"][lo:hi]),
                self._to_tensor(data["terminals"][lo:hi]),
            )
        self._size += n_transitions
        self._pointer = min(self._size, n_transitions)
        print(f"Dataset size: {n_transitions}")

    def fill_synthetic(self, n_transitions: int, seed: int = 0, p_done: float = 0.01, antmaze_rewards: bool = False) -> None:
        """Bench helper (not part of the reference's surface): fill the first n rows of an EMPTY buffer with synthetic
        D4RL-shaped transitions generated on the device (SURVEY §8d's distributions) and account for them like
        load_d4rl_dataset does (iql.py:153-169) — no host arrays, no upload; identical rows on every rank."""
        if not self._gpu:
            raise RuntimeError("iqlhip: fill_synthetic runs in libiqlhip.so and needs a GPU buffer")
        if self._size != 0:
            raise ValueError("Trying to load data into non-empty replay buffer")
        if n_transitions > self._buffer_size:
            raise ValueError("Replay buffer is smaller than the dataset you are trying to load!")
        self._writes += 1
        with torch.cuda.device(self._rows.device):
            hb.check(hb.lib().iqlhip_rows_fill_synth(self._rows.data_ptr(), self._ld, self._state_dim, self._action_dim, 0,
                                                     n_transitions, int(seed), float(p_done), int(antmaze_rewards),
                                                     self._stream()))
        self._size += n_transitions
        self._pointer = min(self._size, n_transitions)

    # ---- dataset ingest on the device (not part of the reference's surface) -------------------
    def state_mean_std(self, eps: float = 1e-3):
        """compute_mean_std (iql.py:77-80) of the stored `observations` column block, reduced on the device:
        (mean, std + eps) as float32 numpy arrays [state_dim]."""
        import iqlhip_ingest as ing
        if not self._gpu:
            raise RuntimeError("iqlhip: state_mean_std runs in libiqlhip.so and needs a GPU buffer")
        if self._size < 1:
            raise ValueError("replay buffer is empty")
        mean, std = ing.cols_mean_std(self._rows[: self._size, : self._state_dim], eps)
        return mean.cpu().numpy(), std.cpu().numpy()

    def normalize_states_(self, mean: np.ndarray, std: np.ndarray) -> None:
        """normalize_states (iql.py:83-84) applied IN PLACE to the s and s' columns of every stored row."""
        if not self._gpu:
            raise RuntimeError("iqlhip: normalize_states_ runs in libiqlhip.so and needs a GPU buffer")
        dev = self._rows.device
        m = torch.as_tensor(np.ascontiguousarray(mean, dtype=np.float32).reshape(-1)).to(dev)
        s = torch.as_tensor(np.ascontiguousarray(std, dtype=np.float32).reshape(-1)).to(dev)
        if m.numel() != self._state_dim or s.numel() != self._state_dim:
            raise ValueError("mean / std must have state_dim entries")
        self._writes += 1
        with torch.cuda.device(dev):
            hb.check(hb.lib().iqlhip_rows_normalize(self._rows.data_ptr(), self._ld, self._state_dim, self._action_dim,
                                                    0, self._size, m.data_ptr(), s.data_ptr(), self._stream()))

    def return_reward_range(self, max_episode_steps: int):
        """return_reward_range (iql.py:262-274) of the stored rows [0, size) in storage order — a freshly loaded dataset,
        not an online ring that has wrapped: (min, max) of the episode returns as Python floats, bit-identical to the
        reference's (float64 sums in row order).  ValueError when the rows hold no complete episode."""
        import iqlhip_ingest as ing
        if not self._gpu:
            raise RuntimeError("iqlhip: return_reward_range runs in libiqlhip.so and needs a GPU buffer")
        if self._size < 1:
            raise ValueError("replay buffer is empty")
        return ing.return_reward_range_device(self._rows, self._state_dim, self._action_dim, self._size, max_episode_steps)

    def modify_reward_(self, env_name: str, max_episode_steps: int = 1000) -> Dict:
        """modify_reward (iql.py:277-289) applied IN PLACE to the reward column of the stored rows [0, size) in storage
        order (a freshly loaded dataset, not a wrapped online ring).  Returns the reference's dict, for
        modify_reward_online(reward, env_name, **d) on the host: max_ret / min_ret / max_episode_steps for halfcheetah,
        hopper and walker2d (rewards divided by max_ret - min_ret, then multiplied by max_episode_steps, in fp32), {}
        for antmaze (rewards - 1) and for any other name (nothing done)."""
        if not self._gpu:
            raise RuntimeError("iqlhip: modify_reward_ runs in libiqlhip.so and needs a GPU buffer")
        locomotion = any(s in env_name for s in ("halfcheetah", "hopper", "walker2d"))
        if not locomotion and "antmaze" not in env_name:
            return {}
        if self._size < 1:
            raise ValueError("replay buffer is empty")
        geometry = (self._rows.data_ptr(), self._ld, self._state_dim, self._action_dim, 0, self._size)
        if not locomotion:
            self._writes += 1
            with torch.cuda.device(self._rows.device):
                hb.check(hb.lib().iqlhip_rows_reward_shift(*geometry, 1.0, self._stream()))
            return {}
        min_ret, max_ret = self.return_reward_range(max_episode_steps)
        self._writes += 1
        with torch.cuda.device(self._rows.device):
            hb.check(hb.lib().iqlhip_rows_reward_scale(*geometry, max_ret - min_ret, float(max_episode_steps), self._stream()))
        return {"max_ret": max_ret, "min_ret": min_ret, "max_episode_steps": max_episode_steps}

    def episode_returns(self, max_episode_steps: int = 1000, discount: float = 0.99, state_break_tol=None,
                        keep_tail: bool = False, sparse_value=None):
        """Per-row episode spans, episode returns and discounted return-to-go of the stored rows [0, size) in storage
        order (a freshly loaded dataset, not a wrapped online ring), as device tensors: an
        iqlhip_ingest.EpisodeReturns.  state_break_tol=1e-6, keep_tail=True: get_return_to_go of the reference's
        finetune/cal_ql.py; both off: the episodes of return_reward_range and of keep_best_trajectories.  Reads only:
        rows staged ahead by train_steps stay valid."""
        import iqlhip_ingest as ing
        if not self._gpu:
            raise RuntimeError("iqlhip: episode_returns runs in libiqlhip.so and needs a GPU buffer")
        if self._size < 1:
            raise ValueError("replay buffer is empty")
        return ing.episode_returns_device(self._rows, self._state_dim, self._action_dim, self._size, max_episode_steps,
                                          discount, state_break_tol, keep_tail, sparse_value)

    def nstep(self, n: int, discount: float, episodes=None):
        """An iqlhip_nstep.NStepReplay of this buffer: its rows as n-step transitions in a derived GPU ReplayBuffer that
        every training, sampling and scoring call takes as it is."""
        import iqlhip_nstep
        return iqlhip_nstep.NStepReplay(self, n, discount, episodes)

    def _index_bound(self) -> int:
        return self._size

    def sample_indices(self, batch_size: int) -> torch.Tensor:
        """The reference's host index draw (global numpy RNG), as a device int64 tensor."""
        indices = np.random.randint(0, self._index_bound(), size=batch_size)
        if not self._gpu:
            return torch.from_numpy(indices)
        # H2D through pinned staging buffers: a ring of 4, each guarded by an event so that a buffer is never
        # rewritten while its copy may still be queued behind earlier work on the stream
        ring = getattr(self, "_idx_ring", None)
        if ring is None or ring[0][0].shape[0] < batch_size:
            ring = [(torch.empty(max(batch_size, 256), dtype=torch.int64).pin_memory(), torch.cuda.Event())
                    for _ in range(4)]
            self._idx_ring, self._idx_slot = ring, 0
        host, done = ring[self._idx_slot]
        self._idx_slot = (self._idx_slot + 1) % len(ring)
        done.synchronize()            # no-op unless this slot's previous copy has not run yet
        host.numpy()[:batch_size] = indices
        dev = self._rows.device
        if torch.cuda.current_device() == dev.index:
            dev_idx = host[:batch_size].to(dev, non_blocking=True)
            done.record()
        else:
            with torch.cuda.device(dev):
                dev_idx = host[:batch_size].to(dev, non_blocking=True)
                done.record()
        return dev_idx

    def _checked_indices(self, idx: torch.Tensor) -> torch.Tensor:
        """The reference's `self._states[indices]` (iql.py:173-177) raises IndexError for an index outside
        [-buffer_size, buffer_size) and wraps negative ones; a gather kernel would read out of bounds.  Checked on the
        host before anything is launched (one small device reduction + read-back when the indices live on the GPU)."""
        cap = self._buffer_size
        if idx.dtype != torch.int64:
            idx = idx.to(torch.int64)
        if idx.numel() == 0:
            return idx
        lo, hi = (int(v) for v in torch.stack((idx.min(), idx.max())).tolist())
        if lo < -cap or hi >= cap:
            bad = hi if hi >= cap else lo
            raise IndexError(f"index {bad} is out of bounds for dimension 0 with size {cap}")
        if lo < 0:
            idx = torch.where(idx < 0, idx + cap, idx)
        return idx

    def gather(self, idx: torch.Tensor) -> TensorBatch:
        n = idx.shape[0]
        S, A = self._state_dim, self._action_dim
        if not self._gpu:
            rows = self._rows[idx]
            return [rows[:, :S].contiguous(), rows[:, S: S + A].contiguous(),
                    rows[:, 2 * S + A: 2 * S + A + 1].contiguous(), rows[:, S + A: 2 * S + A].contiguous(),
                    rows[:, 2 * S + A + 1: 2 * S + A + 2].contiguous()]
        # one coalesced copy of whole packed rows; the five tensors of the reference's contract are views of that
        # block (shapes as in iql.py:173-177, row stride = the packed stride) — ImplicitQLearning.train() hands
        # such a block to the library in place, with no re-packing
        idx = self._checked_indices(idx.to(self._rows.device))
        block = torch.empty((n, self._ld), dtype=torch.float32, device=self._rows.device)
        hb.check(hb.lib().iqlhip_rows_gather_packed(self._rows.data_ptr(), self._ld, self._buffer_size, idx.data_ptr(), n,
                                                    block.data_ptr(), self._stream()))
        return [block[:, :S], block[:, S: S + A], block[:, 2 * S + A: 2 * S + A + 1], block[:, S + A: 2 * S + A],
                block[:, 2 * S + A + 1: 2 * S + A + 2]]

    def gather_split(self, idx: torch.Tensor) -> TensorBatch:
        """The same sample as five separate contiguous tensors (iqlhip_rows_gather)."""
        n = idx.shape[0]
        S, A = self._state_dim, self._action_dim
        dev = self._rows.device
        idx = self._checked_indices(idx.to(dev))
        out = [torch.empty((n, S), dtype=torch.float32, device=dev),
               torch.empty((n, A), dtype=torch.float32, device=dev),
               torch.empty((n, 1), dtype=torch.float32, device=dev),
               torch.empty((n, S), dtype=torch.float32, device=dev),
               torch.empty((n, 1), dtype=torch.float32, device=dev)]
        hb.check(hb.lib().iqlhip_rows_gather(
            self._rows.data_ptr(), self._ld, self._buffer_size, S, A, idx.data_ptr(), n,
            out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr(),
            self._stream()))
        return out

    def sample(self, batch_size: int) -> TensorBatch:
        # order: states, actions, rewards(B,1), next_states, dones(B,1)  (iql.py:171-178)
        if not self._gpu:
            return self.gather(self.sample_indices(batch_size))
        # device side in ONE library call: numpy indices -> (library's pinned ring) -> H2D copy -> packed row gather
        # (same numpy draw, same rows as gather(sample_indices(n)))
        indices = np.random.randint(0, self._index_bound(), size=batch_size)
        if indices.dtype != np.int64:
            indices = indices.astype(np.int64)
        dev = self._rows.device
        # The packed block and its five views come from a ring of SAMPLE_RING pre-built ones per batch size (allocating
        # the block and splitting it cost ~8 us of host time per call — a third of sample()).  A returned batch therefore
        # stays untouched for the next SAMPLE_RING - 1 calls of sample() with that batch size; the reference's loops use
        # a batch in the train() call that follows and drop it (algorithms/finetune/iql.py:771-773, jsrl_w_iql.py:544-548).
        # IQLHIP_SAMPLE_RING=0 restores a fresh block per call.
        ring = self._sample_ring.get(batch_size) if SAMPLE_RING > 0 else None
        if ring is None:
            n_slots = max(SAMPLE_RING, 1)
            slots = []
            for _ in range(n_slots):
                block = torch.empty((batch_size, self._ld), dtype=torch.float32, device=dev)
                # five views of the block in ONE split (s, a, s', r, d[, pad]) -> the reference's order s, a, r, s', d
                parts = block.split(self._split_sizes, dim=1)
                slots.append((block, (parts[0], parts[1], parts[3], parts[2], parts[4]), block.data_ptr()))
            ring = [slots, 0]
            if SAMPLE_RING > 0:
                self._sample_ring[batch_size] = ring
        slots, k = ring
        ring[1] = (k + 1) % len(slots)
        block, views, block_ptr = slots[k]
        if torch.cuda.current_device() == dev.index:
            hb.check(hb.lib().iqlhip_rows_sample_packed(self._rows_ptr, self._ld, self._buffer_size,
                                                        indices.ctypes.data, batch_size, block_ptr, self._stream()))
        else:
            with torch.cuda.device(dev):
                hb.check(hb.lib().iqlhip_rows_sample_packed(self._rows_ptr, self._ld, self._buffer_size,
                                                            indices.ctypes.data, batch_size, block_ptr, self._stream()))
        batch = list(views)
        # ImplicitQLearning.train recognises a batch that IS such a freshly gathered block (it is consumed in place)
        global _last_block
        _last_block = (block_ptr, batch_size, self._state_dim, self._action_dim, self._ld, dev)
        return batch

    # ---- weighted sampling on the device (iqlhip_weighted.py; not part of the reference's surface) ----
    _weights = None              # the library's table (iqlhip_weights*), its n and its generation; None: no weights
    _weights_n = None
    _weights_gen = 0
    _weights_updatable = False   # an updatable table spans _buffer_size rows and is changed in place
    _weights_version = 0         # its content version: update_sample_weights adds 1
    _weights_tracks = False      # the table tracks its largest priority: add_transition enters the new row at it

    @property
    def sample_weights_n(self):
        """Rows the sample weights were set for; None when the buffer has none."""
        return self._weights_n

    def _free_weights(self) -> None:
        table, self._weights, self._weights_n, self._weights_gen = self._weights, None, None, 0
        self._weights_updatable, self._weights_version, self._weights_tracks = False, 0, False
        if table is not None:
            hb.lib().iqlhip_weights_free(table)

    def __del__(self):
        try:
            self._free_weights()
        except Exception:
            pass

    def set_sample_weights(self, weights, updatable: bool = False, max_weight=None, track_max: bool = False,
                           new_row_weight=None) -> None:
        """One float32 weight per row position [0, _index_bound()): a torch tensor on the buffer's device or on the host,
        or an ndarray; None clears them.  The library validates the values and builds its cumulative table on the device
        (8 bytes per row plus 1/63).  ValueError for a CPU buffer, a wrong length, dtype or shape, a NaN, an infinity, a
        negative value, all zeros, or more than 2^24 rows — the previous weights then stay in force.  A weight below
        max(weights) * 2^-39 quantises to 0: that row is never drawn.  Only the *_weighted calls look at weights.
        updatable=True builds a table that update_sample_weights changes in place: it spans the buffer's whole capacity
        (rows beyond the index bound weigh 0), so the weighted calls keep working while add_transition moves the index
        bound; its scale is fixed by max_weight (None: the largest weight given) — a later weight of
        2^(floor(log2(max_weight)) + 1) or more saturates.  12 bytes per row instead of 8.
        track_max=True (with updatable=True: ValueError otherwise): the table keeps the largest priority an applied
        update or the build has seen, at least new_row_weight (default 1.0, finite and > 0), and add_transition enters
        every new row at it — prioritised replay's rule that a new transition is trained on at least once."""
        import iqlhip_weighted as wtd
        if weights is None:
            self._free_weights()
            return
        new_row_weight = wtd.check_tracking_args(updatable, track_max, new_row_weight)
        if not self._gpu:
            raise ValueError("iqlhip: sample weights need a ReplayBuffer that lives on the GPU")
        n = self._index_bound()
        kind = wtd.check_vector(weights, n)
        dev = self._rows.device
        if kind == "numpy" or weights.device.type == "cpu":
            host = weights if kind == "numpy" else weights.numpy()
            wtd.check_host_values(host)
            w_dev = torch.tensor(host, dtype=torch.float32, device=dev)      # (a copy: the array may be read-only)
        elif weights.device != dev:
            raise ValueError(f"iqlhip: sample weights live on {weights.device}, the buffer on {dev}")
        else:
            w_dev = weights.contiguous()
        if not updatable and max_weight is not None:
            raise ValueError("iqlhip: max_weight belongs to an updatable table (updatable=True)")
        with torch.cuda.device(dev):
            table, gen = wtd.build_table(w_dev, n, self._stream(), updatable, self._buffer_size if updatable else None,
                                         max_weight, new_row_weight)
        self._free_weights()
        self._weights, self._weights_n, self._weights_gen = table, (self._buffer_size if updatable else n), gen
        self._weights_updatable, self._weights_tracks = bool(updatable), bool(track_max)

    @property
    def sample_weights_track_max(self) -> bool:
        """Whether the buffer's table tracks its largest priority (set_sample_weights(..., track_max=True))."""
        return self._weights_tracks

    def sample_weights_max(self) -> tuple:
        """(q_max, w_max) of the buffer's tracking table (waits for the device): the priority a new row enters at."""
        import iqlhip_weighted as wtd
        if self._weights is None or not self._weights_tracks:
            raise ValueError("iqlhip: the replay buffer's sample weights do not track their maximum "
                             "(set_sample_weights(..., updatable=True, track_max=True))")
        return wtd.table_max(self._weights)

    def insert_max_sample_weight(self, row: int) -> None:
        """w[row] = the table's largest priority, queued on the buffer's stream with no synchronisation (what
        add_transition does for the row it writes).  row in [0, capacity): ValueError otherwise, and without a tracking
        table."""
        import iqlhip_weighted as wtd
        if self._weights is None or not self._weights_tracks:
            raise ValueError("iqlhip: the replay buffer's sample weights do not track their maximum "
                             "(set_sample_weights(..., updatable=True, track_max=True))")
        row, bound = wtd.check_insert_args(row, None, self._buffer_size)
        with torch.cuda.device(self._rows.device):
            hb.check(hb.lib().iqlhip_weights_insert_max(self._weights, row, bound, self._stream()))
        self._weights_version += 1

    def update_sample_weights(self, indices, weights) -> None:
        """w[indices[j]] = weights[j] in the buffer's updatable table (set_sample_weights(..., updatable=True)): device
        tensors (int64, float32) of one length, queued on the buffer's stream with no synchronisation.  Duplicate indices:
        the last position wins.  A NaN, an infinity, a negative weight or an index outside [0, _index_bound()) is
        skipped and leaves a bit in sample_weights_flags().  A ring write (add_transition) touches the table only if
        it tracks its maximum (set_sample_weights(..., track_max=True)): the written row then enters at the largest
        priority seen so far.  Otherwise the overwritten — or newly filled — row keeps its old weight (0 for a row never
        weighed) until the caller follows the write with update_sample_weights([row], [w])."""
        import iqlhip_weighted as wtd
        if self._weights is None or not self._weights_updatable:
            raise ValueError("iqlhip: the replay buffer has no updatable sample weights "
                             "(set_sample_weights(..., updatable=True))")
        dev = self._rows.device
        m = wtd.check_update_args(indices, weights, dev)
        idx, w = indices.contiguous(), weights.contiguous()
        with torch.cuda.device(dev):
            hb.check(hb.lib().iqlhip_weights_update(self._weights, idx.data_ptr(), w.data_ptr(), m, self._index_bound(),
                                                    self._stream()))
        self._weights_version += 1

    def update_sample_weights_td(self, indices, td, alpha, eps) -> None:
        """update_sample_weights with weights[j] = (max(|td[j, 0]|, |td[j, 1]|) + eps) ** alpha formed on the device inside
        the update's own launches: td is the [m, 2] float32 tensor trainer.last_td_errors() returns for the batch
        gathered at `indices` — the priority refresh of prioritised replay without any torch arithmetic in between.
        ValueError for alpha or eps negative, not finite or both 0."""
        import iqlhip_weighted as wtd
        if self._weights is None or not self._weights_updatable:
            raise ValueError("iqlhip: the replay buffer has no updatable sample weights "
                             "(set_sample_weights(..., updatable=True))")
        dev = self._rows.device
        m = wtd.check_td_args(indices, td, dev)
        alpha, eps = wtd.check_priority_args(alpha, eps)
        idx, e = indices.contiguous(), td.contiguous()
        with torch.cuda.device(dev):
            hb.check(hb.lib().iqlhip_weights_update_td(self._weights, idx.data_ptr(), e.data_ptr(), m, self._index_bound(),
                                                       alpha, eps, self._stream()))
        self._weights_version += 1

    def sample_weights_flags(self) -> int:
        """The table's sticky flag word (waits for the device): bit 0 a non-finite weight was skipped by an update, bit 1
        a negative one, bit 2 an index out of range."""
        import iqlhip_weighted as wtd
        wtd.check_call(self)
        return wtd.table_state(self._weights)[1]

    def clear_sample_weights_flags(self) -> None:
        import iqlhip_weighted as wtd
        wtd.check_call(self)
        with torch.cuda.device(self._rows.device):
            hb.check(hb.lib().iqlhip_weights_clear_flags(self._weights, self._stream()))

    def draw_weighted_indices(self, n: int, seed: int, offset: int, is_beta=None, batch_size=None):
        """Indices 0 .. n - 1 of the weighted index stream (seed, offset) — the stream train_steps_weighted consumes — as
        a device int64 tensor.  With is_beta: (idx, c), c the float32 importance-sampling weights of the drawn rows,
        (q_min / q_row) ** is_beta normalised per batch of batch_size consecutive indices (default: all n) — what
        trainer.train(batch, loss_weights=c) takes."""
        import iqlhip_weighted as wtd
        wtd.check_call(self)
        if n < 1:
            raise ValueError("iqlhip: n must be at least 1")
        dev = self._rows.device
        if is_beta is not None:
            return wtd.draw_with_is(self._weights, dev, n, seed, offset, is_beta, batch_size, self._stream())
        if batch_size is not None:
            raise ValueError("iqlhip: batch_size only means something together with is_beta")
        idx = torch.empty(int(n), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            hb.check(hb.lib().iqlhip_draw_indices_weighted(idx.data_ptr(), int(n), self._weights,
                                                           int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF,
                                                           self._stream()))
        return idx

    def sample_weighted(self, batch_size: int, seed: int, offset: int) -> TensorBatch:
        """A batch drawn by weight on the device: gather(draw_weighted_indices(batch_size, seed, offset))."""
        return self.gather(self.draw_weighted_indices(batch_size, seed, offset))

    def add_transition(self, state: np.ndarray, action: np.ndarray, reward: float, next_state: np.ndarray,
                       done: bool):
        # one packed host row, one H2D copy (the reference issues five, iql.py:189-193)
        S, A = self._state_dim, self._action_dim
        self._writes += 1
        if self._gpu:
            # pinned staging rows (ring of 4, each guarded by an event) and an asynchronous copy
            ring = getattr(self, "_row_ring", None)
            if ring is None:
                ring = [(torch.zeros(self._ld, dtype=torch.float32).pin_memory(), torch.cuda.Event()) for _ in range(4)]
                self._row_ring, self._row_slot = ring, 0
            host, done_ev = ring[self._row_slot]
            self._row_slot = (self._row_slot + 1) % len(ring)
            done_ev.synchronize()
            row = host.numpy()
        else:
            host = None
            row = np.zeros((self._ld,), dtype=np.float32)
        pack_transition(row, S, A, state, action, reward, next_state, done)
        if host is not None:
            dev = self._rows.device
            if torch.cuda.current_device() == dev.index:
                self._rows[self._pointer].copy_(host, non_blocking=True)
                done_ev.record()
            else:
                with torch.cuda.device(dev):
                    self._rows[self._pointer].copy_(host, non_blocking=True)
                    done_ev.record()
        else:
            self._rows[self._pointer].copy_(torch.from_numpy(row))
        if self._weights_tracks:             # behind the ring write, on the same stream: the new row at the running maximum
            self.insert_max_sample_weight(self._pointer)
        self._advance(*self._insert_slot())

    def add_transitions(self, states, actions, rewards, next_states, dones) -> None:
        """E transitions at once — what a vector environment hands over per iteration: states / next_states [E, S],
        actions [E, A], rewards / dones [E], numpy arrays or sequences.  Everything is afterwards exactly what E calls of
        add_transition in row order leave (the rows bit for bit, pointer, size, the write count advanced by E, and with a
        tracking sample-weight table every new row at the running maximum), but a GPU buffer gets them in ONE packed
        upload and ONE launch that wraps at the capacity (iqlhip_rows_write_ring).  1 <= E <= min(capacity,
        IQLHIP_VEC_MAX_ENVS): ValueError otherwise, and for shapes that disagree.  Not part of the reference's surface."""
        S, A = self._state_dim, self._action_dim
        E = check_transitions(S, A, self._buffer_size, states, actions, rewards, next_states, dones)
        pointer, new_size = self._insert_slot(E)
        if self._gpu:
            # pinned staging blocks the kernel reads in place (ring of 4, each guarded by an event, as add_transition's rows)
            ring = getattr(self, "_rows_ring", None)
            if ring is None:
                ring = [(torch.zeros((hb.IQLHIP_VEC_MAX_ENVS, self._ld), dtype=torch.float32).pin_memory(), torch.cuda.Event())
                        for _ in range(4)]
                self._rows_ring, self._rows_slot = ring, 0
            host, done_ev = ring[self._rows_slot]
            self._rows_slot = (self._rows_slot + 1) % len(ring)
            done_ev.synchronize()
            pack_transitions(host.numpy()[:E], S, A, states, actions, rewards, next_states, dones)
            with torch.cuda.device(self._rows.device):
                hb.check(hb.lib().iqlhip_rows_write_ring(self._rows.data_ptr(), self._ld, self._buffer_size, pointer,
                                                         host.data_ptr(), E, self._stream()))
                done_ev.record()
        else:
            block = np.zeros((E, self._ld), dtype=np.float32)
            pack_transitions(block, S, A, states, actions, rewards, next_states, dones)
            self._rows[(pointer + torch.arange(E)) % self._buffer_size] = torch.from_numpy(block)
        self._writes += E
        if self._weights_tracks:             # behind the ring write, on the same stream: add_transition's insert, row by row
            for j in range(E):
                self.insert_max_sample_weight((pointer + j) % self._buffer_size)
        self._advance(pointer, new_size, E)

    # ---- what add_transition(s) and the fused online calls (online_step*, which write the rows in the library) share ----
    def _insert_slot(self, n: int = 1):
        """(the ring position the next row goes to, the size after the next n inserts)."""
        return self._pointer, min(self._size + n, self._buffer_size)

    def _advance(self, pointer: int, new_size: int, n: int = 1) -> None:
        """Behind n rows written from `pointer` on: the ring's pointer and size move past them."""
        self._pointer = (pointer + n) % self._buffer_size
        self._size = new_size


class OfflineReplayBuffer(ReplayBuffer):
    """algorithms/offline/iql.py:125-184 flavour: sample bounded by min(size, pointer),
    add_transition unimplemented."""

    def _index_bound(self) -> int:
        return min(self._size, self._pointer)

    def add_transition(self, *args, **kwargs):
        raise NotImplementedError

    def add_transitions(self, *args, **kwargs):
        raise NotImplementedError


def pack_transition(row: np.ndarray, S: int, A: int, state, action, reward, next_state, done) -> None:
    """One transition into a packed float32 host row [ld]: s | a | s' | r | d (the pad columns stay as they are)."""
    row[:S] = np.asarray(state, dtype=np.float32).reshape(-1)
    row[S: S + A] = np.asarray(action, dtype=np.float32).reshape(-1)
    row[S + A: 2 * S + A] = np.asarray(next_state, dtype=np.float32).reshape(-1)
    row[2 * S + A] = np.float32(reward)
    row[2 * S + A + 1] = np.float32(done)


def check_transitions(S: int, A: int, capacity: int, states, actions, rewards, next_states, dones) -> int:
    """E of the E transitions add_transitions and online_step_vec take: states / next_states [E, S], actions [E, A],
    rewards / dones [E] (or [E, 1]).  ValueError for shapes that disagree and for E outside [1, min(capacity,
    IQLHIP_VEC_MAX_ENVS)]."""
    s, a, ns = (np.asarray(x) for x in (states, actions, next_states))
    r, d = np.asarray(rewards), np.asarray(dones)
    E = s.shape[0] if s.ndim == 2 else -1
    if s.ndim != 2 or s.shape != (E, S) or ns.shape != (E, S) or a.shape != (E, A) or r.size != E or d.size != E \
            or r.ndim not in (1, 2) or d.ndim not in (1, 2):
        raise ValueError(f"iqlhip: E transitions are states / next_states [E, {S}], actions [E, {A}], rewards / dones [E]; got "
                         f"{list(s.shape)}, {list(ns.shape)}, {list(a.shape)}, {list(r.shape)}, {list(d.shape)}")
    if not 1 <= E <= min(capacity, hb.IQLHIP_VEC_MAX_ENVS):
        raise ValueError(f"iqlhip: {E} transitions per call outside [1, min(capacity={capacity}, {hb.IQLHIP_VEC_MAX_ENVS})]")
    return E


def pack_transitions(block: np.ndarray, S: int, A: int, states, actions, rewards, next_states, dones) -> None:
    """pack_transition for every row of block [E, ld] (the same float32 conversions; the pad columns stay as they are)."""
    block[:, :S] = np.asarray(states, dtype=np.float32)
    block[:, S: S + A] = np.asarray(actions, dtype=np.float32)
    block[:, S + A: 2 * S + A] = np.asarray(next_states, dtype=np.float32)
    block[:, 2 * S + A] = np.asarray(rewards, dtype=np.float32).reshape(-1)
    block[:, 2 * S + A + 1] = np.asarray(dones, dtype=np.float32).reshape(-1)


def check_online_ring(buf, device, what: str, holder: str = "a ReplayBuffer", member=None) -> None:
    """What every fused online call asks of the ring it inserts into: a finetune ReplayBuffer on `device`, the trainer's
    GPU.  what: the calling method, as the message names it; holder: what the caller was given (an NStepReplay wraps
    its ring); member: the group member the ring belongs to, named in the message.  ValueError for a ring elsewhere,
    NotImplementedError for the offline flavour — before anything is drawn or moves."""
    if not getattr(buf, "_gpu", False) or buf._rows.device != device:
        raise ValueError(f"{what} needs {holder} on the trainer's GPU" if member is None else
                         f"iqlhip: {what} needs {holder} on the trainer's GPU (member {member})")
    if type(buf)._index_bound is not ReplayBuffer._index_bound or type(buf).add_transition is not ReplayBuffer.add_transition:
        raise NotImplementedError(f"{what} needs the finetune ReplayBuffer (the offline flavour has no add_transition" +
                                  (")" if member is None else f"; member {member})"))


def draw_indices(bound: int, n: int, rng=None) -> np.ndarray:
    """sample()'s host draw as the fused online calls pass it to the library: n int64 indices below `bound`, from `rng`
    (a np.random.RandomState) or the global np.random."""
    idx = (np.random if rng is None else rng).randint(0, bound, size=n)
    return idx if idx.dtype == np.int64 else idx.astype(np.int64)
