"""Trainer groups: K independent ImplicitQLearning trainers of identical shape stepped together.

The reference runs seeds and hyper-parameter settings of one configuration side by side as separate processes
(algorithms/finetune/ray_trainer_4seed.py: four seeds per GPU; ray_hyperparam.py).  A group runs them in ONE process:
every HIP launch of a group step covers all K agents (iqlhip_group_* in include/iqlhip.h).  Each member keeps its own
parameters, Adam state, target nets, hyper-parameters, learning-rate schedule, index stream and replay buffer; after a
group call every member is exactly — bit for bit — where the same steps run alone (`train` / `train_steps`) would have
left it, so its state_dict, checkpoints, act() and later solo calls carry on unchanged.

    group = ImplicitQLearningGroup([trainer_seed0, trainer_seed1, trainer_seed2, trainer_seed3])
    losses = group.train_steps(buffer, n_steps=1000, batch_size=256, seeds=[0, 1, 2, 3])   # [4, 1000, 3]

The online fine-tuning loop (algorithms/finetune/iql.py:741-773, jsrl_w_iql.py:512-548) of all members is one call per
iteration (ImplicitQLearning.online_step for each member, in member order; one ring per member):

    logs, actions = group.online_step(buffers, states, actions, rewards, next_states, dones, 256, act_next=next_states)

Vector environments and an update-to-data ratio (ImplicitQLearning.online_step_vec for each member, in member order):
member k stores E_k transitions, takes U steps and acts on E2_k states, again in one call; updates=0 is the warm-up:

    logs, actions = group.online_step_vec(buffers, states, actions, rewards, next_states, dones, 256, updates=4,
                                          act_next=next_states)

Policy inference of all members is one call too (actor.act / ImplicitQLearning.actor_forward for each, in member
order): `group.act(states)` for one state per member (lockstep evaluation: iqlhip_hostutil.eval_actors),
`group.actor_forward(states)` for batches.

Actor dropout (the reference's adroit configurations: actor_dropout 0.1) is opt-in:

    for seed, t in zip(seeds, trainers):
        t.set_dropout_seed(seed)
    group = ImplicitQLearningGroup(trainers, actor_dropout=True)

Members may then train with dropout, each with its own rate (0 included) and its own train() / eval() mode; every
member's keep-bits are the ones its solo steps would draw, from its own stream position, so the bit-for-bit promise
above holds with dropout too.  A trainer keys its keep-bit stream with the process's torch.initial_seed() unless
ImplicitQLearning.set_dropout_seed(seed) was called: the members of a sweep share a process, so they should call it
with distinct seeds (as above), or they all draw the same masks.  Without actor_dropout=True a group behaves exactly
as before the option existed: a member in training mode with dropout > 0 is refused (NotImplementedError).  The
inference forwards are eval-mode: online_step(act_next=...) and act() for a member that is in training mode with
dropout > 0 raise NotImplementedError, as the solo online_step does — unless that member has opted in with
ImplicitQLearning.set_act_dropout(True): it then acts with keep-bits drawn on the device, exactly as its solo
act() / actor_forward() / online_step(act_next=...) would (its own rate, key and stream position).

Members may train at different batch sizes (the reference's hyper-parameter sweep samples batch_size per trial) in a
group that opted in:

    group = ImplicitQLearningGroup(trainers, mixed_batch=True)
    losses = group.train_steps(buffer, 1000, batch_size=[64, 128, 256, 512], seeds=[0, 1, 2, 3])

train() then takes batches of different row counts, and train_steps() / online_step() take batch_size as an int or as
one int per member; the launches are the same in number, and member k still ends where its solo steps at its own
size end.  Without mixed_batch=True unequal sizes are refused (ValueError), as before the option existed.

Batches mixed from an offline and an online replay buffer (the reference's Cal-QL mixing_ratio; for one trainer
ImplicitQLearning.online_step_mixed / train_steps_mixed) have group forms too — "replay mix", since "mixed" already
names the batch sizes above:

    logs = group.online_step_replay_mix(offline, rings, states, actions, rewards, next_states, dones, 256,
                                        mixing_ratio=[0.25, 0.5, 0.5, 0.75])
    losses = group.train_steps_replay_mix(offline, rings, 1000, 256, seeds=[0, 1, 2, 3], mixing_ratio=0.5)

Scoring without a step (ImplicitQLearning.score_buffer / score / evaluate) has group forms too: one set of launches
for all members, each member's numbers bit for bit its solo call's, and — what no solo call can give — the
across-member mean and standard deviation of every column per row:

    scores, summaries, spread = group.score_buffer(buffer, indices=idx, spread=True)    # [K, n, 8], K dicts, [n, 16]
    held_out = group.evaluate(batch)                                                     # K dicts of train()'s keys

Weighted replay sampling (ImplicitQLearning.train_steps_weighted) has a group form: every member draws by its buffer's
own table, by one free-standing iqlhip_weighted.SampleWeights table, or by a table of its own over a shared buffer (a
None entry: uniformly), and ends where its solo call ends:

    tables = [SampleWeights(w_k) for w_k in per_member_weights]                          # K tables, one shared buffer
    losses = group.train_steps_weighted(buffer, 1000, 256, seeds=[0, 1, 2, 3], weights=tables)

Per-row loss weights, importance-sampling weights and prioritised replay (ImplicitQLearning.train(loss_weights=,
return_td=), train_steps_weighted(is_beta=), train_steps_prioritized) have group forms, fp32 only: a sweep
over seeds or over alpha / eps / is_beta stays in the group, every member's table refreshed by its own TD errors:

    logs = group.train(batches, loss_weights=[c_0, c_1, None, c_3], return_td=True);  tds = group.last_td_errors()
    losses = group.train_steps_weighted(buffer, 1000, 256, seeds, weights=tables, is_beta=[0.4, 0.6, 0.8, 1.0])
    tables = [SampleWeights(w, updatable=True, max_weight=64.0) for _ in trainers]           # one table per member
    losses = group.train_steps_prioritized(buffer, 1000, 256, seeds, alpha=[0.4, 0.6, 0.8, 1.0], is_beta=0.5,
                                           weights=tables)

Not supported (NotImplementedError): data parallelism, bf16 batches of more than 512 rows.  Groups
capture no graphs, and their members train on the same iterations (a loop's warm-up before `batch_size` transitions
is online_step_vec(updates=0), or add_transition per member).  A group of one runs the solo entry points themselves (the same results; the solo
driver is faster for one agent).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

import iqlhip_binding as hb
from iqlhip_replay import check_online_ring, check_transitions, draw_indices, pack_transition, pack_transitions
from iqlhip_trainer import K_MAX, VEC_MAX_BATCH, ImplicitQLearning

BF16_MAX_ROWS = 512      # bf16 batches beyond this run the large-batch kernels, which have no group form


def _addr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


class ImplicitQLearningGroup:
    _mixed_batch = False      # (the option's default: online_step / train_steps read it before they look at a member)

    def __init__(self, trainers: Sequence[ImplicitQLearning], actor_dropout: bool = False, mixed_batch: bool = False):
        trainers = list(trainers)
        if not 1 <= len(trainers) <= hb.IQLHIP_MAX_GROUP:
            raise ValueError(f"iqlhip: a group has 1..{hb.IQLHIP_MAX_GROUP} trainers, got {len(trainers)}")
        self.trainers = trainers
        self._actor_dropout = bool(actor_dropout)
        self._mixed_batch = bool(mixed_batch)
        self._check_members()
        self._g = None
        self._ctxs = None
        self._act_bufs = None

    # ------------------------------------------------------------------ validation (no library call)
    def _check_members(self) -> None:
        trs = self.trainers
        for i, t in enumerate(trs):
            if not isinstance(t, ImplicitQLearning):
                raise ValueError(f"iqlhip: group member {i} is not an ImplicitQLearning trainer")
            if any(t is u for u in trs[:i]):
                raise ValueError(f"iqlhip: group member {i} is the same trainer as an earlier member")
        for i, t in enumerate(trs):
            if t._ctx is None:
                raise RuntimeError(f"iqlhip: group member {i} is not on a GPU device (device='cuda'); there is no CPU "
                                   "implementation of the step in this package")
        t0 = trs[0]
        for i, t in enumerate(trs):
            if t._dev != t0._dev:
                raise ValueError(f"iqlhip: group member {i} is on {t._dev}, member 0 on {t0._dev}")
            if (t._S, t._A, t._gaussian) != (t0._S, t0._A, t0._gaussian):
                raise ValueError(f"iqlhip: group member {i} has dims (S={t._S}, A={t._A}, gaussian={t._gaussian}), "
                                 f"member 0 (S={t0._S}, A={t0._A}, gaussian={t0._gaussian})")
            if getattr(t, "_precision", "f32") != getattr(t0, "_precision", "f32"):
                raise ValueError(f"iqlhip: group member {i} has another precision than member 0")
            if t._dp_world > 1 or t._dp_exchange is not None:
                raise NotImplementedError(f"iqlhip: group member {i} has data parallelism enabled (not supported in a group)")
            if not self._actor_dropout and t.actor.training and t._actor_dropout_p() > 0.0:
                raise NotImplementedError(f"iqlhip: group member {i} uses actor dropout (not supported in a group "
                                          "without actor_dropout=True)")

    def _check_eval_forward(self, members, what: str) -> None:
        """The library's inference forward is eval-mode for a member that has not opted in (set_act_dropout): refuse it
        for such a member that would act with dropout.  Then send every acting member's inference rate and key."""
        for i in members:
            t = self.trainers[i]
            if t.acts_with_dropout() and not t._act_dropout:
                raise NotImplementedError(f"iqlhip: {what}: the library's inference forward is eval-mode (no actor "
                                          f"dropout; member {i} is in training mode and has not called "
                                          "set_act_dropout(True))")
        for i in members:
            self.trainers[i]._prepare_act()

    def _check_batch_size(self, B: int) -> None:
        if getattr(self.trainers[0], "_precision", "f32") == "bf16" and B > BF16_MAX_ROWS:
            raise NotImplementedError(f"iqlhip: bf16 groups take batches of at most {BF16_MAX_ROWS} rows (got {B})")

    @staticmethod
    def _batch_sizes(K: int, batch_size, mixed_batch: bool) -> List[int]:
        """batch_size (an int, or one int per member) as K sizes.  Unequal sizes need a mixed_batch group."""
        if isinstance(batch_size, (int, np.integer)):
            sizes = [int(batch_size)] * K
        else:
            sizes = [int(b) for b in batch_size]
            if len(sizes) != K:
                raise ValueError(f"iqlhip: {len(sizes)} batch sizes for a group of {K}")
        if any(b < 1 for b in sizes):
            raise ValueError(f"iqlhip: batch sizes must be >= 1, got {sizes}")
        if not mixed_batch and any(b != sizes[0] for b in sizes):
            raise ValueError(f"iqlhip: batch sizes {sizes} differ (one batch size per group without mixed_batch=True)")
        return sizes

    # ------------------------------------------------------------------ the library group
    def _group(self):
        """The library group over the members' current contexts (re-created when a member re-attached)."""
        ctxs = tuple(int(t._ctx.value) for t in self.trainers)
        if self._g is not None and ctxs == self._ctxs:
            return self._g
        self._release()
        arr = (C.c_void_p * len(ctxs))(*ctxs)
        g = C.c_void_p()
        if self._actor_dropout:
            hb.check(hb.lib().iqlhip_group_create_flags(arr, len(ctxs), hb.IQLHIP_GROUP_DROPOUT, C.byref(g)))
        else:
            hb.check(hb.lib().iqlhip_group_create(arr, len(ctxs), C.byref(g)))
        self._g, self._ctxs = g, ctxs
        return g

    def _release(self) -> None:
        if self._g is not None:
            hb.check(hb.lib().iqlhip_group_destroy(self._g))
            self._g = None
            self._ctxs = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def __len__(self) -> int:
        return len(self.trainers)

    # ------------------------------------------------------------------ eager steps
    def _next_scalars(self, inv_batch: Sequence[float]):
        """Every member's scalars for its next step (inv_batch[k]: one over its batch's rows), and the Adam step counts
        they belong to (for _commit_step)."""
        scs, adam_next = (hb.StepScalars * len(self.trainers))(), []
        for k, t in enumerate(self.trainers):
            t1 = {g: n + 1 for g, n in t._adam_t.items()}
            t._fill_scalars(scs[k], t1, t._current_lrs(), inv_batch[k])
            adam_next.append(t1)
        return scs, adam_next

    def _group_stats(self, n: int) -> Optional[np.ndarray]:
        """[n, K, 16] statistics of the first n steps of the last library group call (NaN rows: members that have not
        called set_step_stats(True)); None when no member has."""
        if not any(t._step_stats for t in self.trainers):
            return None
        K = len(self.trainers)
        out = (C.c_float * (n * K * hb.IQLHIP_N_STATS))()
        hb.check(hb.lib().iqlhip_group_read_step_stats(self._g, out, n, self.trainers[0]._stream()))
        return np.frombuffer(out, dtype=np.float32).reshape(n, K, hb.IQLHIP_N_STATS).copy()

    def _commit_step(self, adam_next, out) -> List[Dict[str, float]]:
        """Move every member's counters and schedule past the step the library has taken; out: its losses [K][3].
        Members with step statistics on get their "stats/<name>" entries, as their solo train() would."""
        logs = []
        stats = self._group_stats(1)
        for k, t in enumerate(self.trainers):
            t.total_it += 1
            t._adam_t = adam_next[k]
            t._advance_schedule(1)
            t._ts_token = None
            t._eager_next = None
            logs.append({"value_loss": float(out[3 * k]), "q_loss": float(out[3 * k + 1]),
                         "actor_loss": float(out[3 * k + 2])})
            if t._step_stats:
                logs[-1].update({"stats/" + name: float(stats[0, k, i]) for i, name in enumerate(hb.STAT_NAMES)})
        return logs

    def _loss_weight_args(self, Bs, loss_weights, return_td: bool):
        """Every member's (weights or None, TD tensor or None) of a row-weighted step, checked on the host: loss_weights
        is None or K entries, each None (weights of one) or what ImplicitQLearning.train(loss_weights=) takes."""
        from iqlhip_trainer import check_loss_weights
        K = len(self.trainers)
        lws = [None] * K if loss_weights is None else list(loss_weights)
        if len(lws) != K:
            raise ValueError(f"iqlhip: {len(lws)} loss_weights entries for a group of {K} (a tensor or None per member)")
        pairs = []
        for t, B, lw in zip(self.trainers, Bs, lws):
            if getattr(t, "_precision", "f32") == "bf16":
                raise NotImplementedError("iqlhip: per-row loss weights (loss_weights / return_td) are not supported at "
                                          "bf16 precision: the row-weighted backward is an fp32 kernel")
            w = None if lw is None else check_loss_weights(lw, B, t._dev)
            td = torch.empty((B, 2), dtype=torch.float32, device=t._dev) if return_td else None
            pairs.append((w, td))
        return pairs

    def last_td_errors(self) -> List[torch.Tensor]:
        """K tensors [B_k, 2] on the device: every member's ImplicitQLearning.last_td_errors() — (q1 - y, q2 - y) of the
        rows of the last train(..., return_td=True) step.  RuntimeError once a member has stepped again."""
        return [t.last_td_errors() for t in self.trainers]

    def train(self, batches: Sequence, loss_weights=None, return_td: bool = False) -> List[Dict[str, float]]:
        """One step per member on its own batch (ImplicitQLearning.train for each, in one set of launches).  All batches
        have the same number of rows, unless the group was built with mixed_batch=True.  Returns one losses dict per
        member.
        loss_weights: None, or K entries — member k's [B_k] float32 device tensor, or None for weights of one — that
        multiply every row's loss terms (ImplicitQLearning.train(batch, loss_weights=) for each member; the returned
        losses are the weighted ones).  return_td: every member's TD errors are kept for last_td_errors().  fp32 only."""
        batches = list(batches)
        K = len(self.trainers)
        if len(batches) != K:
            raise ValueError(f"iqlhip: {len(batches)} batches for a group of {K}")
        self._check_members()
        Bs = [int(b[0].shape[0]) for b in batches]
        for i, B in enumerate(Bs):
            if B != Bs[0] and not self._mixed_batch:
                raise ValueError(f"iqlhip: batch {i} has {B} rows, batch 0 has {Bs[0]} (one batch size per group)")
        for B in Bs:
            self._check_batch_size(B)
        rw = loss_weights is not None or return_td
        pairs = self._loss_weight_args(Bs, loss_weights, return_td) if rw else None
        if K == 1:      # a group of one IS the solo step (whose eager path returns through host-mapped words: faster)
            if rw:
                return [self.trainers[0].train(batches[0], loss_weights=pairs[0][0], return_td=return_td)]
            return [self.trainers[0].train(batches[0])]
        for t, B in zip(self.trainers, Bs):
            t._prepare(B)
        structs, keep = (hb.Batch * K)(), []
        for i, (t, batch) in enumerate(zip(self.trainers, batches)):
            b, kp, _ = t._batch_struct(batch)
            structs[i] = b
            keep.append(kp)
        scs, adam_next = self._next_scalars([1.0 / B for B in Bs])
        out = (C.c_float * (3 * K))()
        g = self._group()
        if rw:
            for t in self.trainers:
                t._last_td = None
            w_ptrs = (C.c_void_p * K)(*[None if w is None else w.data_ptr() for w, _ in pairs])
            td_ptrs = (C.c_void_p * K)(*[None if td is None else td.data_ptr() for _, td in pairs])
            hb.check(hb.lib().iqlhip_group_step_rw(g, structs, scs, w_ptrs, td_ptrs, out, self.trainers[0]._stream()))
        else:
            step = hb.lib().iqlhip_group_step_mixed if self._mixed_batch else hb.lib().iqlhip_group_step
            hb.check(step(g, structs, scs, out, self.trainers[0]._stream()))
        del keep
        logs = self._commit_step(adam_next, out)
        if rw:
            for t, (_, td) in zip(self.trainers, pairs):
                t._last_td, t._last_td_it = td, t.total_it
        return logs

    # ------------------------------------------------------------------ device-drawn steps
    def _burst_args(self, buffers, seeds, n_steps: int):
        """What every burst checks first: (K buffers — a list of K or the one shared buffer; None for a replay-mix call,
        whose buffers _replay_mix_args takes — and K integer seeds), n_steps >= 1."""
        K = len(self.trainers)
        seeds = [int(s) for s in seeds]
        if buffers is None:
            bufs = None
            if len(seeds) != K:
                raise ValueError(f"iqlhip: a group of {K} needs {K} seeds")
        else:
            bufs = list(buffers) if isinstance(buffers, (list, tuple)) else [buffers] * K
            if len(bufs) != K or len(seeds) != K:
                raise ValueError(f"iqlhip: a group of {K} needs {K} buffers (or one shared buffer) and {K} seeds")
        if n_steps < 1:
            raise ValueError("n_steps must be >= 1")
        return bufs, seeds

    @staticmethod
    def _solo_burst_result(out, return_stats: bool):
        """What a group of one returns for its member's solo burst `out`: statistics [n, 16] as [n, 1, 16], losses
        [n, 3] as [1, n, 3]."""
        if return_stats:
            return out[1][:, None]
        return None if out is None else out[None]

    def _members_steps_args(self, bufs, Bs):
        """Every member's train_steps checks on its buffer; returns (index bounds, 1 / batch rows), each a list of K."""
        pairs = [t._train_steps_args(buf, B) for t, buf, B in zip(self.trainers, bufs, Bs)]
        return [size for size, _ in pairs], [ib for _, ib in pairs]

    def _run_burst(self, n_steps: int, Bs, inv, seeds, chunk: int, return_losses: bool, return_stats: bool, call,
                   continues: bool = False):
        """The multi-step loop behind train_steps, train_steps_weighted and train_steps_replay_mix, whose checks have
        all passed: n_steps in library calls of at most `chunk` steps.  Bs, inv, seeds: every member's batch size, one
        over it and seed.  call(g, B_arr, tab_ptrs, k, seed_arr, offs, stream) makes the kind's one library call for the
        next k steps — tab_ptrs the members' scalar tables, offs their places in their Philox streams — and returns
        its code.  A group call never continues staged rows and leaves none: every member's token is dropped, also by
        a call that fails.  continues (the bursts with importance-sampling weights): call takes an eighth argument, the
        library call's flags — IQLHIP_GROUP_TS_CONTINUE for every piece of this Python call but the first, so the pieces
        go on with each other's staged rows and nothing an earlier Python call staged is ever continued.  Returns the
        statistics [n_steps, K, 16] when return_stats, else losses [K, n_steps, 3] (None unless return_losses)."""
        K = len(self.trainers)
        chunk = max(1, min(int(chunk), K_MAX, hb.IQLHIP_GROUP_MAX_STEPS))
        lib, stream = hb.lib(), self.trainers[0]._stream()
        g = self._group()
        seed_arr = (C.c_uint64 * K)(*[s & 0xFFFFFFFFFFFFFFFF for s in seeds])
        B_arr = (C.c_int32 * K)(*Bs)
        halves = [(B + 1) // 2 for B in Bs]      # (Philox counters a step's draw of B indices consumes)
        losses = np.empty((K, n_steps, 3), dtype=np.float32) if return_losses else None
        stats = np.empty((n_steps, K, hb.IQLHIP_N_STATS), dtype=np.float32) if return_stats else None
        done = 0
        while done < n_steps:
            k = min(chunk, n_steps - done)
            offs = (C.c_uint64 * K)(*[t.total_it * half for t, half in zip(self.trainers, halves)])
            tabs = [np.ascontiguousarray(t._scalar_table(k, ib)) for t, ib in zip(self.trainers, inv)]
            tab_ptrs = (C.c_void_p * K)(*[tb.ctypes.data for tb in tabs])
            if continues:
                rc = call(g, B_arr, tab_ptrs, k, seed_arr, offs, stream, hb.IQLHIP_GROUP_TS_CONTINUE if done else 0)
            else:
                rc = call(g, B_arr, tab_ptrs, k, seed_arr, offs, stream)
            for t in self.trainers:
                t._ts_token = None
            hb.check(rc)
            for t in self.trainers:
                t.total_it += k
            if return_losses:
                out = (C.c_float * (K * k * 3))()
                hb.check(lib.iqlhip_group_read_losses(g, out, k, stream))
                losses[:, done:done + k] = np.frombuffer(out, dtype=np.float32).reshape(K, k, 3)
            if return_stats:
                stats[done:done + k] = self._group_stats(k)
            done += k
        return stats if return_stats else losses

    def train_steps(self, buffers, n_steps: int, batch_size, seeds: Sequence[int],
                    return_losses: bool = True, chunk: int = K_MAX, return_stats: bool = False):
        """n_steps `sample -> train` iterations per member (ImplicitQLearning.train_steps for each): member k draws its
        rows from buffers[k] (or the one shared buffer) under seeds[k] — exactly the rows its own train_steps(buffer,
        n_steps, batch_size, seed=seeds[k]) would draw.  batch_size: an int, or one int per member (unequal sizes:
        mixed_batch groups only; member k then draws what its train_steps at batch_size[k] would).  Returns losses
        [K, n_steps, 3] when return_losses, else None.  return_stats: returns the per-step statistics [n_steps, K, 16]
        instead (hb.STAT_NAMES order; the rows of members that have not called set_step_stats(True) are NaN;
        ValueError when no member has)."""
        K = len(self.trainers)
        bufs, seeds = self._burst_args(buffers, seeds, n_steps)
        Bs = self._batch_sizes(K, batch_size, self._mixed_batch)
        self._check_members()
        for B in Bs:
            self._check_batch_size(B)
        if return_stats and not any(t._step_stats for t in self.trainers):
            raise ValueError("iqlhip: train_steps(return_stats=True) needs set_step_stats(True) on at least one member")
        if K == 1:      # a group of one IS the solo call (chunk graphs, rows staged by idle forward blocks: faster)
            return self._solo_burst_result(
                self.trainers[0].train_steps(bufs[0], n_steps, Bs[0], seed=seeds[0], return_losses=return_losses,
                                             chunk=chunk, return_stats=return_stats), return_stats)
        sizes, inv = self._members_steps_args(bufs, Bs)
        if len({b._ld for b in bufs}) != 1:
            raise ValueError("iqlhip: the members' buffers have different row strides")
        lib, ld = hb.lib(), bufs[0]._ld
        rows = (C.c_void_p * K)(*[b._rows.data_ptr() for b in bufs])
        size_arr = (C.c_int64 * K)(*sizes)

        def call(g, B_arr, tab_ptrs, k, seed_arr, offs, stream):
            if self._mixed_batch:
                return lib.iqlhip_group_train_steps_mixed(g, rows, ld, size_arr, B_arr, tab_ptrs, k, seed_arr, offs, 0,
                                                          stream)
            return lib.iqlhip_group_train_steps(g, rows, ld, size_arr, Bs[0], tab_ptrs, k, seed_arr, offs, 0, stream)
        return self._run_burst(n_steps, Bs, inv, seeds, chunk, return_losses, return_stats, call)

    # ------------------------------------------------------------------ device-drawn steps, rows drawn by weight
    def train_steps_weighted(self, buffers, n_steps: int, batch_size, seeds: Sequence[int], weights=None,
                             return_losses: bool = True, chunk: int = K_MAX, return_stats: bool = False, is_beta=None):
        """train_steps with every member's rows drawn by a weight table (ImplicitQLearning.train_steps_weighted for
        each).  buffers, batch_size, seeds, chunk and the return value as train_steps.  weights: None —
        member k draws by buffers[k]'s own set_sample_weights table (ValueError for a buffer without one); one
        iqlhip_weighted.SampleWeights — every member draws by it; a list of K entries, each a SampleWeights or None —
        member k draws by its own table over the (possibly shared) buffer, a None member draws UNIFORMLY.  Afterwards
        member k is bit for bit where its solo train_steps_weighted(buffers[k], n_steps, batch_size[k], seed=seeds[k],
        weights=...) leaves it, a uniform member where its solo train_steps does.  Every table must stay alive until
        the queued steps have run (SampleWeights.free and set_sample_weights wait for the device).  Everything is
        checked before anything is launched or any counter moves; the refusals are train_steps' and
        train_steps_weighted's.
        is_beta (None: the call above, unchanged; else a float >= 0 or K of them): member k's loss terms are weighted by
        c = (q_min / q_row) ** is_beta[k] over each step's batch — its solo train_steps_weighted(..., is_beta=is_beta[k]),
        bit for bit; a uniform member gets c = 1 and still ends where its solo train_steps does.  fp32 only."""
        import iqlhip_weighted as wtd
        K = len(self.trainers)
        bufs, seeds = self._burst_args(buffers, seeds, n_steps)
        Bs = self._batch_sizes(K, batch_size, self._mixed_batch)
        betas = None
        if is_beta is not None:
            betas = wtd.check_group_is_beta(K, is_beta)
            for t in self.trainers:
                t._is_beta_arg(0.0)          # (fp32 only: NotImplementedError for a bf16 member)
        self._check_members()
        for B in Bs:
            self._check_batch_size(B)
        entries = wtd.check_group_call(bufs, weights, K)
        for i, (t, buf) in enumerate(zip(self.trainers, bufs)):
            if buf._rows.device != t._dev:
                raise ValueError(f"iqlhip: the replay buffer must live on the trainer's GPU ({t._dev}; member {i})")
        if return_stats and not any(t._step_stats for t in self.trainers):
            raise ValueError("iqlhip: train_steps_weighted(return_stats=True) needs set_step_stats(True) on at least one "
                             "member")
        for t in self.trainers:
            t._refuse_injected_masks()
        if K == 1:      # a group of one IS the solo call
            t, e = self.trainers[0], entries[0]
            if e is None:
                out = t.train_steps(bufs[0], n_steps, Bs[0], seed=seeds[0], return_losses=return_losses, chunk=chunk,
                                    return_stats=return_stats)
            else:
                out = t.train_steps_weighted(bufs[0], n_steps, Bs[0], seed=seeds[0], return_losses=return_losses,
                                             chunk=chunk, return_stats=return_stats,
                                             weights=None if e is bufs[0] else e,
                                             is_beta=None if betas is None else betas[0])
            return self._solo_burst_result(out, return_stats)
        sizes, inv = self._members_steps_args(bufs, Bs)
        # (an updatable table spans a capacity, and that is the size its member's draw is given: rows beyond the index
        #  bound weigh 0)
        for i, e in enumerate(entries):
            if isinstance(e, wtd.SampleWeights):
                if e.updatable:
                    sizes[i] = e.n
            elif e is not None and e._weights_updatable:
                sizes[i] = e.sample_weights_n
        if len({b._ld for b in bufs}) != 1:
            raise ValueError("iqlhip: the members' buffers have different row strides")
        fn, ld = hb.lib().iqlhip_group_train_steps_weighted, bufs[0]._ld
        rows = (C.c_void_p * K)(*[b._rows.data_ptr() for b in bufs])
        size_arr = (C.c_int64 * K)(*sizes)
        # (member k's table: its buffer's own, its SampleWeights', or NULL — the uniform draw)
        wt_arr = (C.c_void_p * K)(*[None if e is None else (e._table if isinstance(e, wtd.SampleWeights) else e._weights)
                                    for e in entries])

        if betas is not None:
            fn_is, beta_arr = hb.lib().iqlhip_group_train_steps_weighted_is, (C.c_float * K)(*betas)

            def call_is(g, B_arr, tab_ptrs, k, seed_arr, offs, stream, flags):
                return fn_is(g, rows, ld, size_arr, B_arr, tab_ptrs, k, seed_arr, offs, flags, stream, wt_arr, beta_arr)
            return self._run_burst(n_steps, Bs, inv, seeds, chunk, return_losses, return_stats, call_is, continues=True)

        def call(g, B_arr, tab_ptrs, k, seed_arr, offs, stream):
            return fn(g, rows, ld, size_arr, B_arr, tab_ptrs, k, seed_arr, offs, 0, stream, wt_arr)
        return self._run_burst(n_steps, Bs, inv, seeds, chunk, return_losses, return_stats, call)

    # ------------------------------------------------------------------ prioritised replay (DESIGN.md 6j "trainer groups")
    def train_steps_prioritized(self, buffers, n_steps: int, batch_size, seeds: Sequence[int], alpha=0.6, eps=1e-3,
                                is_beta=0.0, weights=None, chunk: int = K_MAX, return_losses: bool = True,
                                return_stats: bool = False):
        """ImplicitQLearning.train_steps_prioritized for every member in one set of launches: prioritised replay whose
        steps write their TD errors back into the member's own updatable table, lag of one step included, with no host
        round trip.  buffers, batch_size, seeds and the return value as train_steps_weighted.  weights: None — member k
        updates buffers[k]'s own updatable table — or a list of K updatable SampleWeights.  Every member needs a table of
        its OWN (ValueError for a None entry and for one table given to two members: their updates would race); sharing
        a buffer's rows is fine.  alpha, eps, is_beta: a float, or K of them — a sweep over the exponents is one call.
        chunk is rounded as in the solo call (down to an even number, at least 2); inside one call the pieces go on with
        the lag-1 chain, a member with an odd batch size draws afresh in every piece, and a call never starts on rows
        an earlier call staged.  Afterwards member k — parameters, Adam state, losses, statistics, its table — is bit for
        bit where its solo train_steps_prioritized(buffers[k], n_steps, batch_size[k], seed=seeds[k], alpha=alpha[k],
        eps=eps[k], is_beta=is_beta[k], chunk=chunk, weights=...) leaves it.  The tables' versions move as there.
        ValueError for a static table, for alpha, eps or is_beta negative or not finite, for alpha = eps = 0;
        NotImplementedError at bf16 precision, under data parallelism and with injected dropout masks pending — all
        before anything is launched or any counter moves."""
        import iqlhip_weighted as wtd
        K = len(self.trainers)
        bufs, seeds = self._burst_args(buffers, seeds, n_steps)
        Bs = self._batch_sizes(K, batch_size, self._mixed_batch)
        alphas, epss = wtd.check_group_priority_args(K, alpha, eps)
        betas = wtd.check_group_is_beta(K, is_beta)
        for t in self.trainers:
            t._is_beta_arg(0.0)              # (fp32 only: NotImplementedError for a bf16 member)
        self._check_members()
        for B in Bs:
            self._check_batch_size(B)
        entries = wtd.check_group_prioritized(bufs, weights, K)
        for i, (t, buf) in enumerate(zip(self.trainers, bufs)):
            if buf._rows.device != t._dev:
                raise ValueError(f"iqlhip: the replay buffer must live on the trainer's GPU ({t._dev}; member {i})")
        if return_stats and not any(t._step_stats for t in self.trainers):
            raise ValueError("iqlhip: train_steps_prioritized(return_stats=True) needs set_step_stats(True) on at least "
                             "one member")
        for t in self.trainers:
            t._refuse_injected_masks()
        if K == 1:      # a group of one IS the solo call
            e = entries[0]
            out = self.trainers[0].train_steps_prioritized(
                bufs[0], n_steps, Bs[0], seed=seeds[0], alpha=alphas[0], eps=epss[0], is_beta=betas[0], chunk=chunk,
                return_losses=return_losses, return_stats=return_stats, weights=None if e is bufs[0] else e)
            return self._solo_burst_result(out, return_stats)
        _, inv = self._members_steps_args(bufs, Bs)
        # (an updatable table spans a capacity, and that is the size its member's draw is given)
        sizes = [e.n if isinstance(e, wtd.SampleWeights) else e.sample_weights_n for e in entries]
        if len({b._ld for b in bufs}) != 1:
            raise ValueError("iqlhip: the members' buffers have different row strides")
        fn, ld = hb.lib().iqlhip_group_train_steps_prioritized, bufs[0]._ld
        rows = (C.c_void_p * K)(*[b._rows.data_ptr() for b in bufs])
        size_arr = (C.c_int64 * K)(*sizes)
        wt_arr = (C.c_void_p * K)(*[e._table if isinstance(e, wtd.SampleWeights) else e._weights for e in entries])
        beta_arr, alpha_arr, eps_arr = (C.c_float * K)(*betas), (C.c_float * K)(*alphas), (C.c_float * K)(*epss)

        def call(g, B_arr, tab_ptrs, k, seed_arr, offs, stream, flags):
            rc = fn(g, rows, ld, size_arr, B_arr, tab_ptrs, k, seed_arr, offs, flags, stream, wt_arr, beta_arr, alpha_arr,
                    eps_arr)
            if rc == 0:                    # (the library moved every table's content version: the Python mirrors follow)
                for e in entries:
                    if isinstance(e, wtd.SampleWeights):
                        e._version += 1
                    else:
                        e._weights_version += 1
            return rc
        chunk = max(2, min(int(chunk), K_MAX) & ~1)
        return self._run_burst(n_steps, Bs, inv, seeds, chunk, return_losses, return_stats, call, continues=True)

    # ------------------------------------------------------------------ the online loop
    def _online_rows(self, ld: int, states, actions, rewards, next_states, dones, act_next):
        """The host side of an online call's arguments: the K transitions as packed rows [K, ld]; the members that ask
        for their next action; and the act_next arrays in the library's argument order — (states in, member mask,
        max_action, sampling seeds, actions out), all None when no member asks."""
        K, t0 = len(self.trainers), self.trainers[0]
        S, A = t0._S, t0._A
        rows = np.zeros((K, ld), dtype=np.float32)
        for k in range(K):
            pack_transition(rows[k], S, A, states[k], actions[k], rewards[k], next_states[k], dones[k])
        want = [k for k in range(K) if act_next is not None and act_next[k] is not None]
        a_in = a_out = mask = max_a = seeds = None
        if want:
            a_in = np.zeros((K, S), dtype=np.float32)
            for k in want:
                a_in[k] = np.asarray(act_next[k], dtype=np.float32).reshape(-1)
            a_out = np.zeros((K, A), dtype=np.float32)
            mask = np.array([k in want for k in range(K)], dtype=np.int32)
            max_a = np.array([float(t.actor.max_action) for t in self.trainers], dtype=np.float32)
            seeds = np.array([t._act_seed() if (t.actor.training and t._gaussian) else 0 for t in self.trainers],
                             dtype=np.uint64)
        return rows, want, (a_in, mask, max_a, seeds, a_out)

    def _online_lists(self, what: str, act_next, rngs, **per) -> None:
        """Every per-member argument of an online call is a list of K entries (act_next and rngs when given)."""
        K = len(self.trainers)
        if act_next is not None:
            per["act_next"] = act_next
        if rngs is not None:
            per["rngs"] = rngs
        for name, v in per.items():
            if not isinstance(v, (list, tuple)) or len(v) != K:
                raise ValueError(f"iqlhip: {what} of a group of {K} needs {name} as a list of {K} entries")

    def _run_online(self, rings, transitions, Bs, act_next, rngs, draw, call):
        """Every member inserts one transition into its ring, draws its batch, takes one step and (where act_next asks)
        acts, in the one library call `call` makes — what both online methods do once their checks have passed.
        transitions: (states, actions, rewards, next_states, dones), K entries each.  draw(k, new_size, rng): member
        k's host index arrays over its size after the insert, in batch order, from rng (rngs[k]; None: the global
        np.random) — called in member order.  call(g, ring_args, rows, idx, scs, out, act_args, stream) returns the
        library's status: ring_args = (rings, ld, capacities, pointers) and act_args = (states in, member mask,
        max_action, seeds, actions out) are in the library's argument order, rows and idx are host addresses.  Only
        when the status is OK does anything move: every ring past its insert, every member past its step.  Returns the
        logs, or (logs, actions) when the call took act_next."""
        K, ld = len(self.trainers), rings[0]._ld
        rows, want, act = self._online_rows(ld, *transitions, act_next)
        slots = [b._insert_slot() for b in rings]
        idx = []                         # (the members' index lists one after another)
        for k in range(K):
            idx.extend(draw(k, slots[k][1], None if rngs is None else rngs[k]))
        idx = np.ascontiguousarray(np.concatenate(idx), dtype=np.int64)
        scs, adam_next = self._next_scalars([1.0 / B for B in Bs])
        out = (C.c_float * (3 * K))()
        ring_args = ((C.c_void_p * K)(*[b._rows.data_ptr() for b in rings]), ld,
                     (C.c_int64 * K)(*[b._buffer_size for b in rings]), (C.c_int64 * K)(*[p for p, _ in slots]))
        hb.check(call(self._group(), ring_args, rows.ctypes.data, idx.ctypes.data, scs, out, tuple(map(_addr, act)),
                      self.trainers[0]._stream()))
        for buf, slot in zip(rings, slots):
            buf._writes += 1
            buf._advance(*slot)
        logs = self._commit_step(adam_next, out)
        if act_next is None:
            return logs
        return logs, [act[4][k].copy() if k in want else None for k in range(K)]

    @staticmethod
    def _solo_online_result(res, act_next):
        """What a group of one returns for its member's solo online call `res`, made with act_next[0]."""
        if act_next is None:
            return [res]
        if act_next[0] is None:
            return [res], [None]
        return [res[0]], [res[1]]

    def online_step(self, buffers, states, actions, rewards, next_states, dones, batch_size,
                    act_next: Optional[Sequence] = None, rngs: Optional[Sequence[np.random.RandomState]] = None):
        """One iteration of the online loop for every member in ONE library call (ImplicitQLearning.online_step for
        each, in member order): member k stores its transition (states[k], actions[k], rewards[k], next_states[k],
        dones[k]) in buffers[k], draws `randint(0, size_k, batch_size)` over its size after the insert — from
        rngs[k] (a np.random.RandomState), or from the global np.random in member order when rngs is None — and takes
        one step on those rows.  batch_size: an int, or one int per member (unequal sizes: mixed_batch groups only).
        buffers are K distinct finetune ReplayBuffers on the members' GPU with one row stride.
        act_next: None, or K entries (a state or None): member k's entry gives actor.act(state) with its UPDATED
        policy, as the solo act_next does.  Returns one train()-style dict per member; with act_next, (logs, actions)
        where actions[k] is None for members that asked for none.  Buffers, step counts and schedules move only once
        the call has succeeded."""
        K = len(self.trainers)
        self._online_lists("online_step", act_next, rngs, buffers=buffers, states=states, actions=actions, rewards=rewards,
                           next_states=next_states, dones=dones)
        bufs = list(buffers)
        Bs = self._batch_sizes(K, batch_size, self._mixed_batch)
        self._check_members()
        for B in Bs:
            self._check_batch_size(B)
        if act_next is not None:         # (before any ring, counter or parameter moves)
            self._check_eval_forward([k for k in range(K) if act_next[k] is not None], "online_step(act_next=...)")
        if K == 1 and rngs is None:      # a group of one IS the solo call
            return self._solo_online_result(
                self.trainers[0].online_step(bufs[0], states[0], actions[0], rewards[0], next_states[0], dones[0], Bs[0],
                                             act_next=None if act_next is None else act_next[0]), act_next)
        for i, (t, buf) in enumerate(zip(self.trainers, bufs)):
            t._prepare(Bs[i])
            check_online_ring(buf, t._dev, "online_step", member=i)
            if any(buf is b or buf._rows.data_ptr() == b._rows.data_ptr() for b in bufs[:i]):
                raise ValueError(f"iqlhip: member {i} shares a replay buffer with an earlier member (one buffer each)")
        if any(b._ld != bufs[0]._ld for b in bufs):
            raise ValueError("iqlhip: the members' buffers have different row strides")

        def call(g, ring_args, rows, idx, scs, out, act_args, stream):
            if self._mixed_batch:
                return hb.lib().iqlhip_group_online_step_mixed(g, *ring_args, rows, idx, (C.c_int32 * K)(*Bs), scs, out,
                                                               *act_args, stream)
            return hb.lib().iqlhip_group_online_step(g, *ring_args, rows, idx, Bs[0], scs, out, *act_args, stream)
        return self._run_online(bufs, (states, actions, rewards, next_states, dones), Bs, act_next, rngs,
                                lambda k, new_size, rng: (draw_indices(new_size, Bs[k], rng),), call)

    # ------------------------------------------------------------------ the online loop over vector environments
    def _run_online_vec(self, rings, blocks, Bs, U: int, acts, rngs, peeks):
        """_run_online's sibling for E_k transitions per member and U steps in the one library call
        (iqlhip_group_online_step_vec), once every check has passed.  blocks[k]: member k's (states, actions, rewards,
        next_states, dones) of E_k rows; acts[k]: its [E2_k, S] float32 act states or None; peeks[k]: its
        _peek_schedule(U) (None for U <= 1 without a schedule to look ahead in).  The members' rows, indices and act
        states go to the library one member after another.  The indices are drawn per member in member order: U
        consecutive sample() draws over the member's size after all its E_k inserts, from rngs[k] (None: the global
        np.random).  The scalars are what U single steps of the member would use (ImplicitQLearning._run_online_vec).
        Only when the status is OK does anything move: every ring by E_k, every member by U steps.  Returns one list of
        U dicts per member, or (lists, actions) when the call took act_next."""
        K, ld = len(self.trainers), rings[0]._ld
        t0 = self.trainers[0]
        S, A = t0._S, t0._A
        Es = [len(b[0]) for b in blocks]
        rows = np.zeros((sum(Es), ld), dtype=np.float32)
        lo = 0
        for k, b in enumerate(blocks):
            pack_transitions(rows[lo: lo + Es[k]], S, A, *b)
            lo += Es[k]
        slots = [b._insert_slot(E) for b, E in zip(rings, Es)]
        idx = None
        if U:
            idx = np.ascontiguousarray(np.concatenate(
                [draw_indices(slots[k][1], Bs[k], None if rngs is None else rngs[k]) for k in range(K) for _ in range(U)]),
                dtype=np.int64)
        scs = (hb.StepScalars * max(K * U, 1))()
        for k, t in enumerate(self.trainers):
            lrs = t._current_lrs()
            lr_pi = [lrs["pi"]] if peeks[k] is None else peeks[k][0]      # (one step: the rate in force, whatever the schedule's state)
            for u in range(U):
                t._fill_scalars(scs[k * U + u], {g: n + u + 1 for g, n in t._adam_t.items()}, dict(lrs, pi=float(lr_pi[u])),
                                1.0 / Bs[k])
        out = (C.c_float * max(3 * K * U, 1))()
        want = [k for k in range(K) if acts is not None and acts[k] is not None]
        a_in = a_rows = max_a = seeds = a_out = None
        if want:
            a_rows = np.array([acts[k].shape[0] if k in want else 0 for k in range(K)], dtype=np.int32)
            a_in = np.ascontiguousarray(np.concatenate([acts[k].reshape(-1) for k in want]), dtype=np.float32)
            a_out = np.zeros((int(a_rows.sum()), A), dtype=np.float32)
            max_a = np.array([float(t.actor.max_action) for t in self.trainers], dtype=np.float32)
            seeds = np.array([t._act_seed() if (k in want and t.actor.training and t._gaussian) else 0
                              for k, t in enumerate(self.trainers)], dtype=np.uint64)
        hb.check(hb.lib().iqlhip_group_online_step_vec(
            self._group(), (C.c_void_p * K)(*[b._rows.data_ptr() for b in rings]), ld,
            (C.c_int64 * K)(*[b._buffer_size for b in rings]), (C.c_int64 * K)(*[p for p, _ in slots]), rows.ctypes.data,
            (C.c_int32 * K)(*Es), _addr(idx), (C.c_int32 * K)(*Bs), U, C.addressof(scs), C.addressof(out), _addr(a_in),
            _addr(a_rows), _addr(max_a), _addr(seeds), _addr(a_out), t0._stream()))
        for t, ring, (pointer, new_size), E in zip(self.trainers, rings, slots, Es):
            t._commit_online(ring, pointer, new_size, E, U, {g: n + U for g, n in t._adam_t.items()})
            if U:
                t._ts_token = None
                t._eager_next = None
        stats = self._group_stats(U) if U else None
        logs = []
        for k, t in enumerate(self.trainers):
            logs.append([{"value_loss": float(out[3 * (k * U + u)]), "q_loss": float(out[3 * (k * U + u) + 1]),
                          "actor_loss": float(out[3 * (k * U + u) + 2])} for u in range(U)])
            if t._step_stats and U:
                for u, log in enumerate(logs[-1]):
                    log.update({"stats/" + name: float(stats[u, k, i]) for i, name in enumerate(hb.STAT_NAMES)})
        if acts is None:
            return logs
        actions, lo = [None] * K, 0
        for k in want:
            actions[k] = a_out[lo: lo + int(a_rows[k])].copy()
            lo += int(a_rows[k])
        return logs, actions

    def online_step_vec(self, buffers, states, actions, rewards, next_states, dones, batch_size, updates: int = 1,
                        act_next: Optional[Sequence] = None, rngs: Optional[Sequence[np.random.RandomState]] = None):
        """One iteration of an online loop over vector environments, with an update-to-data ratio of `updates`, for every
        member in ONE library call, one upload and one synchronisation (ImplicitQLearning.online_step_vec for each, in
        member order; DESIGN.md 6b "Group vector-environment online step"): member k stores its E_k transitions
        (states[k] [E_k, S], actions[k] [E_k, A], rewards[k] / dones[k] [E_k], next_states[k] [E_k, S]) in buffers[k],
        makes `updates` consecutive sample() draws of batch_size rows over its size after all E_k inserts — from rngs[k]
        (a np.random.RandomState), or from the global np.random in member order when rngs is None — takes `updates` steps
        on them, and acts on act_next[k] ([E2_k, S], or None) with its UPDATED policy.  1 <= E_k <= min(capacity_k, 64)
        and E2_k in [1, 64] may differ between members; 0 <= updates <= 32 is common to the call (the members' steps run
        in lockstep); batch_size: an int, or one int per member (unequal sizes: mixed_batch groups only), each <= 512.
        updates = 0 is the loop's warm-up: rows in, actions out, an empty list per member, no step counter moves.
        Afterwards member k — ring and counters, parameters, Adam state, schedule, total_it, noise and keep-bit counters,
        per-step logs and statistics, clip record, actions — is bit for bit where its solo online_step_vec leaves it.
        Returns one list of `updates` train()-style dicts per member; with act_next, (lists, actions) where actions[k]
        is [E2_k, A] float32, or None for a member that asked for none.  The refusals are online_step's and the solo
        online_step_vec's, each naming the member, all before anything is launched, drawn or moved."""
        K = len(self.trainers)
        what = "online_step_vec"
        self._online_lists(what, act_next, rngs, buffers=buffers, states=states, actions=actions, rewards=rewards,
                           next_states=next_states, dones=dones)
        bufs = list(buffers)
        Bs = self._batch_sizes(K, batch_size, self._mixed_batch)
        U = int(updates)
        self._check_members()
        for B in Bs:
            self._check_batch_size(B)
        if not 0 <= U <= hb.IQLHIP_VEC_MAX_UPDATES:
            raise ValueError(f"iqlhip: updates = {U} outside [0, {hb.IQLHIP_VEC_MAX_UPDATES}]")
        if any(B > VEC_MAX_BATCH for B in Bs):
            raise ValueError(f"iqlhip: batch sizes {Bs} outside [1, {VEC_MAX_BATCH}]")
        acts = None if act_next is None else [None] * K
        for i, (t, buf) in enumerate(zip(self.trainers, bufs)):
            check_online_ring(buf, t._dev, what, member=i)
            if buf._weights_tracks:
                raise NotImplementedError(f"iqlhip: {what} has no insert for a tracking sample-weight table (member {i}); use "
                                          "add_transitions and the prioritised calls")
            try:
                check_transitions(t._S, t._A, buf._buffer_size, states[i], actions[i], rewards[i], next_states[i], dones[i])
            except ValueError as e:
                raise ValueError(f"{e} (member {i})") from None
            if act_next is not None and act_next[i] is not None:
                a = np.asarray(act_next[i], dtype=np.float32)
                if a.ndim != 2 or a.shape[1] != t._S or not 1 <= a.shape[0] <= hb.IQLHIP_VEC_MAX_ENVS:
                    raise ValueError(f"iqlhip: act_next must be [E2, {t._S}] with 1 <= E2 <= {hb.IQLHIP_VEC_MAX_ENVS}, got "
                                     f"{list(a.shape)} (member {i})")
                acts[i] = np.ascontiguousarray(a)
        if act_next is not None:         # (before any ring, counter or parameter moves)
            self._check_eval_forward([k for k in range(K) if acts[k] is not None], f"{what}(act_next=...)")
        if K == 1 and rngs is None:      # a group of one IS the solo call
            return self._solo_online_result(
                self.trainers[0].online_step_vec(bufs[0], states[0], actions[0], rewards[0], next_states[0], dones[0], Bs[0],
                                                 updates=U, act_next=None if act_next is None else act_next[0]), act_next)
        peeks = []
        for i, (t, buf) in enumerate(zip(self.trainers, bufs)):      # (every member's refusals, then every member's settings)
            # (injected masks are pending unless the member's _prepare is about to send another dropout rate, which clears them)
            p_eff = t._actor_dropout_p() if t.actor.training else 0.0
            if getattr(t, "_masks_injected", False) and p_eff == getattr(t, "_dropout_sent", p_eff):
                raise NotImplementedError(f"iqlhip: {what} draws every step's keep-bits and cannot use the masks written by "
                                          f"inject_dropout_masks (member {i}); step with train(), or clear them "
                                          "(set_dropout_seed)")
            if any(buf is b or buf._rows.data_ptr() == b._rows.data_ptr() for b in bufs[:i]):
                raise ValueError(f"iqlhip: member {i} shares a replay buffer with an earlier member (one buffer each)")
            pk = t._peek_schedule(U) if U else None
            if U > 1 and pk is None:
                raise NotImplementedError(f"iqlhip: {what} with updates > 1 needs an actor schedule whose rates can be looked "
                                          f"up ahead (CosineAnnealingLR with eta_min = 0, stepped by its trainer; member {i})")
            peeks.append(pk)
            t._check_step_stats(Bs[i])       # (what _prepare refuses, in front of any member's _prepare)
            t._check_grad_clip(Bs[i])
        if any(b._ld != bufs[0]._ld for b in bufs):
            raise ValueError("iqlhip: the members' buffers have different row strides")
        for t, B in zip(self.trainers, Bs):
            t._prepare(B)
        blocks = [(states[k], actions[k], rewards[k], next_states[k], dones[k]) for k in range(K)]
        return self._run_online_vec(bufs, blocks, Bs, U, acts, rngs, peeks)

    # ------------------------------------------------------------------ batches mixed from an offline and an online buffer
    def _replay_mix_args(self, offline_buffers, online_buffers, batch_size, mixing_ratio, burst: bool):
        """What both replay-mix calls check before anything is launched, drawn or moved.  Returns (offline buffers,
        online buffers, batch sizes, n_off), each a list of K."""
        import iqlhip_mixed as mixed
        K = len(self.trainers)
        offs = list(offline_buffers) if isinstance(offline_buffers, (list, tuple)) else [offline_buffers] * K
        if not isinstance(online_buffers, (list, tuple)) or len(online_buffers) != K or len(offs) != K:
            raise ValueError(f"iqlhip: a replay-mix call of a group of {K} needs online_buffers as a list of {K} entries "
                             f"and {K} offline buffers (or one shared offline buffer)")
        ons = list(online_buffers)
        if isinstance(mixing_ratio, (int, float, np.integer, np.floating)):
            ratios = [float(mixing_ratio)] * K
        else:
            ratios = [float(r) for r in mixing_ratio]
            if len(ratios) != K:
                raise ValueError(f"iqlhip: {len(ratios)} mixing ratios for a group of {K}")
        Bs = self._batch_sizes(K, batch_size, self._mixed_batch)
        self._check_members()
        n_offs = [mixed.split(B, r)[0] for B, r in zip(Bs, ratios)]
        for t, off, on in zip(self.trainers, offs, ons):
            mixed.check_buffers(off, on, t._dev, t._S, t._A)
        for B in Bs:
            self._check_batch_size(B)
        for i, (off, on) in enumerate(zip(offs, ons)):
            if off._size < 1:
                raise ValueError(f"iqlhip: the offline replay buffer is empty (member {i})")
            if burst and on._size < 1:
                raise ValueError(f"iqlhip: the online replay buffer is empty (member {i})")
        for i, on in enumerate(ons):      # (a ring is written in the launch that reads the offline rows)
            if any(on is b or on._rows.data_ptr() == b._rows.data_ptr() for b in ons[:i]):
                raise ValueError(f"iqlhip: member {i} shares an online replay buffer with an earlier member (one ring "
                                 "each)")
            if any(on is b or on._rows.data_ptr() == b._rows.data_ptr() for b in offs):
                raise ValueError(f"iqlhip: member {i}'s online replay buffer is a member's offline buffer (the offline "
                                 "rows are read only)")
        if len({b._ld for b in offs + ons}) != 1:
            raise ValueError("iqlhip: the members' buffers have different row strides")
        return offs, ons, Bs, n_offs

    def online_step_replay_mix(self, offline_buffers, online_buffers, states, actions, rewards, next_states, dones,
                               batch_size, mixing_ratio=0.5, act_next: Optional[Sequence] = None,
                               rngs: Optional[Sequence[np.random.RandomState]] = None):
        """online_step with every member's batch mixed from two buffers (ImplicitQLearning.online_step_mixed for each,
        in member order, in ONE library call): member k stores its transition in online_buffers[k] and trains on
        n_off[k] = int(batch_size[k] * mixing_ratio[k]) rows of offline_buffers[k] followed by batch_size[k] - n_off[k]
        rows of its ring.  offline_buffers: one buffer shared by all members, or a list of K (only read);
        online_buffers: K distinct rings, none of them any member's offline buffer.  batch_size: an int, or one int per
        member (unequal sizes: mixed_batch groups only); mixing_ratio: a float, or one per member (any group).  The
        host index draw is the solo call's — per member, the offline draw, then the online draw over the size after
        the insert — from rngs[k], or from the global np.random in member order when rngs is None.  act_next, rngs and
        the return value as online_step.  Everything is checked before anything is drawn, launched or moved."""
        import iqlhip_mixed as mixed
        K = len(self.trainers)
        self._online_lists("online_step_replay_mix", act_next, rngs, states=states, actions=actions, rewards=rewards,
                           next_states=next_states, dones=dones)
        offs, ons, Bs, n_offs = self._replay_mix_args(offline_buffers, online_buffers, batch_size, mixing_ratio, burst=False)
        if act_next is not None:         # (before any ring, counter or parameter moves)
            self._check_eval_forward([k for k in range(K) if act_next[k] is not None],
                                     "online_step_replay_mix(act_next=...)")
        if K == 1 and rngs is None:      # a group of one IS the solo call
            return self._solo_online_result(
                self.trainers[0].online_step_mixed(offs[0], ons[0], states[0], actions[0], rewards[0], next_states[0],
                                                   dones[0], Bs[0], mixing_ratio if np.isscalar(mixing_ratio)
                                                   else mixing_ratio[0], act_next=None if act_next is None else act_next[0]),
                act_next)
        for t, B in zip(self.trainers, Bs):
            t._prepare(B)

        def call(g, ring_args, rows, idx, scs, out, act_args, stream):
            return hb.lib().iqlhip_group_online_step_replay2(
                g, *ring_args, rows, idx, (C.c_int32 * K)(*Bs), scs, out, *act_args, stream,
                (C.c_void_p * K)(*[b._rows.data_ptr() for b in offs]), (C.c_int64 * K)(*[b._size for b in offs]),
                (C.c_int32 * K)(*n_offs))
        return self._run_online(ons, (states, actions, rewards, next_states, dones), Bs, act_next, rngs,
                                lambda k, new_size, rng: mixed.draw_host_indices(offs[k]._size, n_offs[k], new_size,
                                                                                 Bs[k] - n_offs[k], rng=rng), call)

    def train_steps_replay_mix(self, offline_buffers, online_buffers, n_steps: int, batch_size, seeds: Sequence[int],
                               mixing_ratio=0.5, return_losses: bool = True, chunk: int = K_MAX,
                               return_stats: bool = False):
        """train_steps with every member's batches mixed from two buffers (ImplicitQLearning.train_steps_mixed for each):
        member k draws train_steps_mixed's stream under seeds[k] — batch row r < n_off[k] over offline_buffers[k]'s
        size, the others over online_buffers[k]'s, both sizes read at the call.  Buffers, batch_size and mixing_ratio as
        online_step_replay_mix (the online buffers are only read here, but must hold rows); returns what train_steps
        returns.  As the solo call, a burst neither continues nor leaves staged rows."""
        K = len(self.trainers)
        _, seeds = self._burst_args(None, seeds, n_steps)
        offs, ons, Bs, n_offs = self._replay_mix_args(offline_buffers, online_buffers, batch_size, mixing_ratio, burst=True)
        if return_stats and not any(t._step_stats for t in self.trainers):
            raise ValueError("iqlhip: train_steps_replay_mix(return_stats=True) needs set_step_stats(True) on at least one "
                             "member")
        if K == 1:      # a group of one IS the solo call
            return self._solo_burst_result(
                self.trainers[0].train_steps_mixed(offs[0], ons[0], n_steps, Bs[0], mixing_ratio if np.isscalar(mixing_ratio)
                                                   else mixing_ratio[0], seed=seeds[0], return_losses=return_losses,
                                                   chunk=chunk, return_stats=return_stats), return_stats)
        for t, B in zip(self.trainers, Bs):
            t._prepare(B)
        for t in self.trainers:
            t._refuse_injected_masks()
        fn, ld = hb.lib().iqlhip_group_train_steps_replay2, offs[0]._ld
        rows_off = (C.c_void_p * K)(*[b._rows.data_ptr() for b in offs])
        size_off = (C.c_int64 * K)(*[b._size for b in offs])
        rows_on = (C.c_void_p * K)(*[b._rows.data_ptr() for b in ons])
        size_on = (C.c_int64 * K)(*[b._size for b in ons])
        n_off_arr = (C.c_int32 * K)(*n_offs)

        def call(g, B_arr, tab_ptrs, k, seed_arr, offsets, stream):
            return fn(g, rows_off, size_off, rows_on, size_on, ld, B_arr, n_off_arr, tab_ptrs, k, seed_arr, offsets, stream)
        return self._run_burst(n_steps, Bs, [1.0 / B for B in Bs], seeds, chunk, return_losses, return_stats, call)

    # ------------------------------------------------------------------ policy inference
    def _actor_call(self, rows: Sequence[int], in_ptrs, ld_s: int, out_ptrs, ld_a: int, seeds, max_action,
                    flags: int = 0) -> None:
        K = len(self.trainers)
        hb.check(hb.lib().iqlhip_group_actor_forward(self._group(), (C.c_void_p * K)(*in_ptrs), ld_s,
                                                     (C.c_int32 * K)(*rows), (C.c_uint64 * K)(*seeds),
                                                     (C.c_float * K)(*max_action), (C.c_void_p * K)(*out_ptrs), ld_a,
                                                     flags, self.trainers[0]._stream()))

    def act(self, states: Sequence) -> List[Optional[np.ndarray]]:
        """actor.act(states[k], "cuda") of every member with a state (None: no action), in ONE library call and one
        wait (a completion word the host spins on): member k samples iff its actor is in training mode and its
        policy is Gaussian, as actor.act decides.  Returns K actions (np.float32[A], or None) — bit for bit,
        random-stream counters included, what the K solo calls in member order return."""
        K = len(self.trainers)
        if not isinstance(states, (list, tuple)) or len(states) != K:
            raise ValueError(f"iqlhip: act of a group of {K} needs states as a list of {K} entries")
        self._check_members()
        self._check_eval_forward([k for k in range(K) if states[k] is not None], "act")
        if K == 1:      # a group of one IS the solo call
            t = self.trainers[0]
            if states[0] is None:
                return [None]
            return [t.act_one(states[0], float(t.actor.max_action), sample=t.actor.training)]
        t0 = self.trainers[0]
        S, A = t0._S, t0._A
        if self._act_bufs is None:
            h_in = torch.empty((K, S), dtype=torch.float32).pin_memory()
            h_out = torch.empty((K, A), dtype=torch.float32).pin_memory()
            self._act_bufs = (h_in, h_out, h_in.numpy(), h_out.numpy())
        h_in, h_out, in_np, out_np = self._act_bufs
        want = [s is not None for s in states]
        for k in range(K):
            if want[k]:
                in_np[k, :] = np.asarray(states[k], dtype=np.float32).reshape(-1)
        seeds = [t._act_seed() if (w and t.actor.training and t._gaussian) else 0 for t, w in zip(self.trainers, want)]
        base_in, base_out = h_in.data_ptr(), h_out.data_ptr()
        self._actor_call([int(w) for w in want], [base_in + 4 * S * k for k in range(K)], S,
                         [base_out + 4 * A * k for k in range(K)], A, seeds,
                         [float(t.actor.max_action) for t in self.trainers], flags=hb.IQLHIP_GROUP_ACT_WAIT)
        return [out_np[k].copy() if want[k] else None for k in range(K)]

    def actor_forward(self, states: Sequence[torch.Tensor], sample: bool = False,
                      max_action: Optional[float] = None) -> List[torch.Tensor]:
        """ImplicitQLearning.actor_forward(states[k], sample, max_action) of every member, one library call per
        chunk: states[k] is a [n_k, S] tensor (n_k may differ, and may be 0); returns K device tensors [n_k, A], bit
        for bit the solo results.  Inputs above a member's row cap are split as the solo method splits them, so each
        member's random-stream counter moves as it would alone."""
        K = len(self.trainers)
        if not isinstance(states, (list, tuple)) or len(states) != K:
            raise ValueError(f"iqlhip: actor_forward of a group of {K} needs states as a list of {K} tensors")
        self._check_members()
        for t in self.trainers:          # (members that have not opted in to act dropout keep the eval-mode forward)
            t._prepare_act()
        if K == 1:
            return [self.trainers[0].actor_forward(states[0], sample=sample, max_action=max_action)]
        t0 = self.trainers[0]
        S, A = t0._S, t0._A
        xs = [t._as_dev(x).reshape(-1, S) for t, x in zip(self.trainers, states)]
        outs = [torch.empty((x.shape[0], A), dtype=torch.float32, device=t._dev) for t, x in zip(self.trainers, xs)]
        caps = [max(t._max_batch, hb.IQLHIP_ACT_ROWS) for t in self.trainers]
        mas = [float(t.max_action if max_action is None else max_action) for t in self.trainers]
        n_calls = max([-(-x.shape[0] // c) for x, c in zip(xs, caps)] + [0])
        for j in range(n_calls):
            rows, ins, ptrs, seeds = [], [], [], []
            for t, x, out, cap in zip(self.trainers, xs, outs, caps):
                r0 = j * cap
                r1 = min(x.shape[0], r0 + cap)
                n = max(0, r1 - r0)
                rows.append(n)
                ins.append(x[r0:r1].data_ptr() if n else None)
                ptrs.append(out[r0:r1].data_ptr() if n else None)
                seeds.append(t._act_seed() if (n and sample and t._gaussian) else 0)
            self._actor_call(rows, ins, S, ptrs, A, seeds, mas)
        return outs

    # ------------------------------------------------------------------ scoring without a step
    def _score_call(self, row_ptrs, ld: int, sizes, start: int, n: int, idx_lists, out, summary: bool, spread,
                    chunk: int):
        """The library call behind score_buffer / score / evaluate; every argument has been checked."""
        K = len(self.trainers)
        t0 = self.trainers[0]
        dev = t0._dev
        for t in self.trainers:      # beta, discount, iql_tau of each member: what its next step would send too
            if t._hyper_tuple() != t._hyper_sent:
                h = t._hyper_struct()
                hb.check(hb.lib().iqlhip_set_hyper(t._ctx, C.byref(h)))
                t._hyper_sent = t._hyper_tuple()
        idx_arr, keep = None, []
        if idx_lists is not None:
            ptrs = []
            for k, idx in enumerate(idx_lists):
                same = next((j for j in range(k) if idx_lists[j] is idx), None)
                if same is not None:     # (one list for several members: one device copy)
                    ptrs.append(ptrs[same])
                    continue
                if not (isinstance(idx, torch.Tensor) and idx.device == dev):
                    idx = torch.as_tensor(idx).to(dev)
                idx = idx.contiguous()
                keep.append(idx)
                ptrs.append(idx.data_ptr())
            idx_arr = (C.c_void_p * K)(*ptrs)
        if out is None:
            out = torch.empty((K, n, hb.IQLHIP_N_SCORE), dtype=torch.float32, device=dev)
        if spread is True:
            spread = torch.empty((n, 2 * hb.IQLHIP_N_SCORE), dtype=torch.float32, device=dev)
        elif spread is False:
            spread = None
        out_arr = None if out is False else (C.c_void_p * K)(*[out[k].data_ptr() for k in range(K)])
        words = (C.c_float * (11 * K))() if summary else None
        hb.check(hb.lib().iqlhip_group_score_rows(
            self._group(), (C.c_void_p * K)(*row_ptrs), ld, (C.c_int64 * K)(*sizes), start, n, idx_arr, out_arr,
            None if spread is None else spread.data_ptr(), chunk, words, t0._stream()))
        del keep                     # (device copies of the lists: freed in stream order, behind the call's launches)
        import iqlhip_score as score
        summaries = [score.summary_dict(words[11 * k: 11 * k + 11]) for k in range(K)] if summary else None
        return (None if out is False else out), summaries, spread

    def score_buffer(self, buffers, start: int = 0, n: Optional[int] = None, indices=None, out=None, summary: bool = True,
                     spread=False, chunk_rows: Optional[int] = None):
        """ImplicitQLearning.score_buffer of every member in one set of launches: (scores, summaries, spread).
        buffers: one replay buffer for all members, or a list of K.  The rows are the range [start, start + n) — it must
        fit the smallest buffer; n=None: to its end — or the rows `indices` names: one list for all members, or a list
        of K lists of equal length (1-D int64 tensors or arrays, host or device), member k's into buffers[k].
        scores: a [K, n, 8] float32 device tensor (hb.SCORE_NAMES columns; out: a tensor to write into, or False: None);
        scores[k] is bit for bit what trainers[k].score_buffer returns for those rows.  summaries: K dicts with
        iqlhip_score.SUMMARY_KEYS, member k's equal to its solo call's at the same chunk_rows; None for summary=False.
        spread: False, True or an [n, 16] tensor to write into: per row the mean over members of each of the eight
        columns, then their population standard deviation (hb.SPREAD_NAMES), fp32, members in order; available with
        out=False.  It is accepted only when all members score the same rows (one buffer with a range or one index
        list): ValueError otherwise.  chunk_rows: rows of a member per launch sequence (at most 65 536 // K).  Each
        member scores with its own hyper-parameters, in eval mode, with its fp32 masters.  Nothing any member holds
        changes.  The refusals are score_buffer's, raised before anything is launched."""
        import iqlhip_score as score
        self._check_members()
        K = len(self.trainers)
        t0 = self.trainers[0]
        bufs, one_buffer = score.group_buffers(buffers, K)
        ld = hb.row_stride(t0._S, t0._A)
        sizes = [score.check_buffer(b, t._dev, t._S, t._A, ld) for t, b in zip(self.trainers, bufs)]
        start, count, idx_lists, one_list = score.group_rows(sizes, start, n, indices)
        score.check_group_outputs(out, summary, spread, one_buffer and one_list, K, count, t0._dev)
        chunk = score.check_chunk_rows(chunk_rows)
        return self._score_call([b._rows.data_ptr() for b in bufs], ld, sizes, start, count, idx_lists, out, summary,
                                spread, chunk)

    def score(self, batches, out=None, summary: bool = True, spread=False, chunk_rows: Optional[int] = None):
        """score_buffer for five-tensor batches as train() takes them: one batch for all members (packed once), or a
        list of K batches of equal length (spread: the shared form only).  Returns (scores, summaries, spread)."""
        import iqlhip_score as score
        self._check_members()
        K = len(self.trainers)
        t0 = self.trainers[0]
        shared = len(batches) > 0 and isinstance(batches[0], torch.Tensor)
        blist = [batches] if shared else list(batches)
        if not shared and len(blist) != K:
            raise ValueError(f"iqlhip: {len(blist)} batches for a group of {K} (one shared batch, or one per member)")
        structs, keep, Bs = [], [], []
        for t, batch in zip(self.trainers, blist):
            b, kp, B = t._batch_struct(batch)
            structs.append(b)
            keep.append(kp)
            Bs.append(B)
        if any(B != Bs[0] for B in Bs):
            raise ValueError(f"iqlhip: the batches have {Bs} rows (one length for all members)")
        B = Bs[0]
        if B < 1:
            raise ValueError("iqlhip: an empty batch")
        score.check_group_outputs(out, summary, spread, shared, K, B, t0._dev)
        chunk = score.check_chunk_rows(chunk_rows)
        ld = hb.row_stride(t0._S, t0._A)
        block = torch.empty((len(blist), B, ld), dtype=torch.float32, device=t0._dev)
        for k, (t, b) in enumerate(zip(self.trainers, structs)):
            hb.check(hb.lib().iqlhip_pack_rows(t._ctx, C.byref(b), block[k].data_ptr(), t0._stream()))
        ptrs = [block[0 if shared else k].data_ptr() for k in range(K)]
        res = self._score_call(ptrs, ld, [B] * K, 0, B, None, out, summary, spread, chunk)
        if not summary:      # (with a summary the call has waited for the stream; otherwise the block must outlive it)
            block.record_stream(torch.cuda.current_stream(t0._dev))
        del keep
        return res

    def evaluate(self, batches) -> List[Dict[str, float]]:
        """train()'s three keys of every member for its batch (or the one shared batch), computed without a step."""
        _, summaries, _ = self.score(batches, out=False, summary=True)
        return [{k: s[k] for k in ("value_loss", "q_loss", "actor_loss")} for s in summaries]
