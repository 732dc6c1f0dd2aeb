"""ImplicitQLearning with the reference's constructor, attributes and checkpoint
format (algorithms/finetune/iql.py:445-606) whose train() runs the whole step
— 7 MLP forwards, 3 losses, backward, 3 Adam updates, Polyak — in libiqlhip.so
(hand-written HIP for gfx950) instead of ~700 aten calls.

Ownership model: the caller constructs the nn.Modules and the
torch.optim.Adam objects and passes them in.  On a GPU device this class
re-homes every nn.Parameter's storage into ONE flat fp32 arena (layout:
iqlhip_arena_layout) and the Adam moments into two more, so the C ABI sees
three pointers; the Parameter / optimizer objects the caller holds stay the
same Python objects and stay usable (actor.act(), state_dict(), isinstance).

There is no CPU implementation of the step: with a CPU device the object can
be constructed, checkpointed and inspected (host logic), but train() raises.
"""
from __future__ import annotations

import copy
import ctypes as C
import warnings
from typing import Any, Dict, List, Optional, Tuple

import weakref

import numpy as np
import torch
import torch.nn as nn
from torch.optim.lr_scheduler import CosineAnnealingLR

import iqlhip_binding as hb
import iqlhip_dp as dp
from iqlhip_replay import check_online_ring, check_transitions, draw_indices, pack_transition, pack_transitions
from iqlhip_networks import (DeterministicPolicy, GaussianPolicy, LOG_STD_MAX, LOG_STD_MIN, dropout_p, register_actor_owner,
                             linear_layers)

TensorBatch = List[torch.Tensor]
EXP_ADV_MAX = 100.0
K_MAX = 1024  # steps per captured hipGraph chunk (library limit)
STATS_BF16_MAX_ROWS = 512  # bf16 batches beyond this take the large-batch kernels, which keep no step statistics
VEC_MAX_BATCH = 512        # rows per step of online_step_vec: the small-batch kernels, fp32 or bf16


def _is_gpu(device) -> bool:
    return torch.device(device).type == "cuda"


try:
    _raw_stream = torch._C._cuda_getCurrentRawStream          # (device_index) -> hipStream_t as int
except AttributeError:                                        # pragma: no cover - older torch
    def _raw_stream(index: int) -> int:
        return torch.cuda.current_stream(index).cuda_stream


def check_loss_weights(loss_weights, B: int, device) -> torch.Tensor:
    """train(batch, loss_weights=...): a float32 tensor of shape [B] or [B, 1] on the trainer's device -> contiguous [B].
    Nothing is converted or moved silently: a wrong dtype, shape or device is the caller's mistake."""
    if not isinstance(loss_weights, torch.Tensor):
        raise TypeError(f"iqlhip: loss_weights must be a torch.Tensor, not {type(loss_weights).__name__}")
    if loss_weights.dtype != torch.float32:
        raise TypeError(f"iqlhip: loss_weights must be float32, not {loss_weights.dtype}")
    if tuple(loss_weights.shape) not in ((B,), (B, 1)):
        raise ValueError(f"iqlhip: loss_weights must have shape [{B}] or [{B}, 1], not {list(loss_weights.shape)}")
    if loss_weights.device != torch.device(device):
        raise ValueError(f"iqlhip: loss_weights live on {loss_weights.device}, the trainer on {device}")
    return loss_weights.reshape(B).contiguous()


def _mlp_tensors(module: nn.Module) -> Dict[str, nn.Parameter]:
    lin = linear_layers(module)
    if len(lin) != 3:
        raise NotImplementedError(
            f"iqlhip kernels are built for 2 hidden layers (3 Linear layers); this network has {len(lin)}")
    return {"w0": lin[0].weight, "b0": lin[0].bias, "w1": lin[1].weight, "b1": lin[1].bias,
            "w2": lin[2].weight, "b2": lin[2].bias}


class ImplicitQLearning:
    def __init__(self, max_action: float, actor: nn.Module, actor_optimizer: torch.optim.Optimizer,
                 q_network: nn.Module, q_optimizer: torch.optim.Optimizer, v_network: nn.Module,
                 v_optimizer: torch.optim.Optimizer, iql_tau: float = 0.7, beta: float = 3.0,
                 max_steps: int = 1000000, discount: float = 0.99, tau: float = 0.005, device: str = "cpu"):
        self.max_action = max_action
        self.qf = q_network
        self.q_target = copy.deepcopy(self.qf).requires_grad_(False).to(device)
        self.vf = v_network
        self.actor = actor
        self.v_optimizer = v_optimizer
        self.q_optimizer = q_optimizer
        self.actor_optimizer = actor_optimizer
        if max_steps is not None:
            self.actor_lr_schedule = CosineAnnealingLR(self.actor_optimizer, max_steps)
        else:
            self.actor_lr_schedule = None
        self.iql_tau = iql_tau
        self.beta = beta
        self.discount = discount
        self.tau = tau

        self.total_it = 0
        self.device = device

        # data-parallel state (set by enable_data_parallel)
        self._dp_group = None
        self._dp_world = 1
        self._dp_rank = 0
        self._dp_exchange = None      # None | "rccl" | "p2p" (in-library) | "torch" (torch.distributed.all_reduce)
        self._table_cache = None
        self._ts_token = None         # (buffer, its write count) of the last train_steps call
        self._eager_next = None       # scalars of the next eager step, computed ahead (train() on a fresh sample() block)
        self._loss_out = (C.c_float * 3)()
        self._on_scalars = hb.StepScalars()     # the online calls' step scalars, filled anew by every call

        self._ctx = None
        self._max_batch = 0
        self._adam_t = {"v": 0, "q": 0, "pi": 0}
        self._hyper_sent = None
        self._act_bufs = None
        self._act_dropout = False     # set_act_dropout: actor dropout inside the device inference forward (opt-in)
        self._act_dropout_sent = None  # (rate, key) the context's inference side holds; None: never sent (rate 0)
        self._act_key_stale = False   # set_dropout_seed since: the next inference call sends the new key
        self._step_stats = False      # set_step_stats: per-step training statistics (opt-in)
        self._step_stats_sent = False  # ... as the current context holds it
        self._grad_clip = None        # set_grad_clip: (vf, qf, actor) max norms, inf = no limit; None: off (opt-in)
        self._grad_clip_sent = None   # ... as the current context holds it
        self._masks_injected = False  # inject_dropout_masks since the last iqlhip_set_dropout: train_steps refuses
        if _is_gpu(device):
            self._attach(max_batch=256)
            register_actor_owner(self.actor, self)

    # ------------------------------------------------------------------ arenas
    def _net_tensors(self) -> Dict[str, Dict[str, nn.Parameter]]:
        nets = {"vf": _mlp_tensors(self.vf), "q1": _mlp_tensors(self.qf.q1), "q2": _mlp_tensors(self.qf.q2),
                "pi": _mlp_tensors(self.actor.net)}
        if hasattr(self.actor, "log_std"):
            nets["pi"]["log_std"] = self.actor.log_std
        return nets

    def _target_tensors(self) -> Dict[str, Dict[str, nn.Parameter]]:
        return {"q1": _mlp_tensors(self.q_target.q1), "q2": _mlp_tensors(self.q_target.q2)}

    def _probe_dims(self) -> Tuple[int, int, bool]:
        nets = self._net_tensors()
        S = nets["vf"]["w0"].shape[1]
        A = nets["pi"]["w2"].shape[0]
        hid = nets["vf"]["w0"].shape[0]
        ok = (nets["q1"]["w0"].shape[1] == S + A and nets["q2"]["w0"].shape[1] == S + A
              and nets["pi"]["w0"].shape[1] == S and nets["vf"]["w2"].shape[0] == 1)
        for t in nets.values():
            ok = ok and t["w0"].shape[0] == hid and tuple(t["w1"].shape) == (hid, hid) and t["w2"].shape[1] == hid
        if not ok:
            raise NotImplementedError("network shapes are not the IQL TwinQ / ValueFunction / policy MLP family")
        if hid != hb.IQLHIP_HIDDEN:
            raise NotImplementedError(f"iqlhip kernels are tiled for hidden_dim={hb.IQLHIP_HIDDEN}, got {hid}")
        if dropout_p(self.vf) > 0.0 or dropout_p(self.qf) > 0.0:
            raise NotImplementedError("dropout is implemented for the actor only (the reference has none elsewhere)")
        gaussian = "log_std" in nets["pi"]
        if not gaussian and not isinstance(self.actor, DeterministicPolicy) and not hasattr(self.actor, "net"):
            raise NotImplementedError("unknown policy class")
        return S, A, gaussian

    def _segments(self, L, nets, which: str):
        """yield (parameter, offset_in_arena) for every tensor of `nets`."""
        order = {"vf": hb.NET_V, "q1": hb.NET_Q1, "q2": hb.NET_Q2, "pi": hb.NET_PI}
        for name, tensors in nets.items():
            nl = L.net[order[name]]
            shift = L.target_src if which == "target" else 0
            for key, p in tensors.items():
                yield p, int(getattr(nl, key)) - shift

    def _attach(self, max_batch: int) -> None:
        """(Re)build the flat arenas + the library context for `max_batch` rows."""
        S, A, gaussian = self._probe_dims()
        dev = torch.device(self.device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if not 1 <= max_batch <= 16384:
            raise ValueError(f"iqlhip: batch of {max_batch} rows is outside the library's range [1, 16384]")
        L = hb.arena_layout(S, A, gaussian, max_batch)
        old = None
        if self._ctx is not None:
            if self._dp_world > 1:
                raise RuntimeError("iqlhip: the batch size cannot grow after enable_data_parallel(); construct the "
                                   "trainer's first step (or call reserve_batch) with the largest batch first")
            old = (self._params_arena, self._target_arena, self._m_arena, self._v_arena)
        self._S, self._A, self._gaussian, self._layout = S, A, gaussian, L
        self._on_row = np.zeros(hb.row_stride(S, A), dtype=np.float32)      # the online calls' packed host row
        if old is None:
            self._params_arena = torch.zeros(L.n_params, dtype=torch.float32, device=dev)
            self._target_arena = torch.zeros(L.n_target, dtype=torch.float32, device=dev)
            self._m_arena = torch.zeros(L.n_params, dtype=torch.float32, device=dev)
            self._v_arena = torch.zeros(L.n_params, dtype=torch.float32, device=dev)
            self._rehome(self._net_tensors(), self._params_arena, "params")
            self._rehome(self._target_tensors(), self._target_arena, "target")
            self._absorb_opt_state()
        else:
            self._params_arena, self._target_arena, self._m_arena, self._v_arena = old
        self._dev = dev
        d = hb.Dims(S, A, hb.IQLHIP_HIDDEN, 2, hb.POLICY_GAUSSIAN if gaussian else hb.POLICY_DETERMINISTIC, max_batch)
        h = self._hyper_struct()
        ctx = C.c_void_p()
        hb.check(hb.lib().iqlhip_create(C.byref(d), C.byref(h), dev.index, C.byref(ctx)))
        if self._ctx is not None:       # carry the Philox stream positions (dropout masks, act() noise) over
            ctr = (C.c_uint64 * 2)()
            hb.check(hb.lib().iqlhip_get_counters(self._ctx, ctr))
            hb.check(hb.lib().iqlhip_set_counters(ctx, ctr))
            n_act = C.c_uint64(0)       # ... and the inference keep-bit stream's position, rate and key
            hb.check(hb.lib().iqlhip_get_act_dropout_counter(self._ctx, C.byref(n_act)))
            hb.check(hb.lib().iqlhip_set_act_dropout_counter(ctx, n_act))
            if self._act_dropout_sent is not None:
                hb.check(hb.lib().iqlhip_set_act_dropout(ctx, *self._act_dropout_sent))
        self._release()                 # the previous (smaller) context, only now that the new one exists
        self._ctx = ctx
        self._table_cache = None
        self._hyper_sent = self._hyper_tuple()
        self._dropout_sent = 0.0
        self._masks_injected = False
        self._step_stats_sent = False
        self._grad_clip_sent = None
        self._max_batch = max_batch
        if getattr(self, "_precision", "f32") == "bf16":     # survives a re-attach for a larger batch
            hb.check(hb.lib().iqlhip_set_precision(self._ctx, 1))
        hb.check(hb.lib().iqlhip_bind(self._ctx, self._params_arena.data_ptr(), self._target_arena.data_ptr(),
                                      self._m_arena.data_ptr(), self._v_arena.data_ptr()))

    def _rehome(self, nets, arena: torch.Tensor, which: str) -> None:
        with torch.no_grad():
            for p, off in self._segments(self._layout, nets, which):
                view = arena[off: off + p.numel()].view(p.shape)
                view.copy_(p.data.to(arena.device, torch.float32))
                p.data = view

    def _param_offsets(self):
        return list(self._segments(self._layout, self._net_tensors(), "params"))

    def _optimizer_of(self, p) -> torch.optim.Optimizer:
        for opt in (self.v_optimizer, self.q_optimizer, self.actor_optimizer):
            for grp in opt.param_groups:
                if any(p is q for q in grp["params"]):
                    return opt
        raise ValueError("parameter is not owned by any of the three optimizers")

    def _absorb_opt_state(self) -> None:
        """Copy existing Adam moments (e.g. after optimizer.load_state_dict) into the flat
        arenas and re-point the optimizer's state tensors at the arena views."""
        with torch.no_grad():
            for grp_name, opt in (("v", self.v_optimizer), ("q", self.q_optimizer), ("pi", self.actor_optimizer)):
                t = 0
                for st in opt.state.values():
                    if "step" in st:
                        t = max(t, int(float(st["step"])))
                self._adam_t[grp_name] = t
            for p, off in self._param_offsets():
                opt = self._optimizer_of(p)
                st = opt.state.get(p, None)
                mv = self._m_arena[off: off + p.numel()].view(p.shape)
                vv = self._v_arena[off: off + p.numel()].view(p.shape)
                if st and "exp_avg" in st:
                    mv.copy_(st["exp_avg"].to(mv.device, torch.float32))
                    vv.copy_(st["exp_avg_sq"].to(vv.device, torch.float32))
                    st["exp_avg"], st["exp_avg_sq"] = mv, vv
                else:
                    mv.zero_()
                    vv.zero_()

    def _sync_opt_state(self) -> None:
        """Make optimizer.state look like torch.optim.Adam's after `t` steps (for state_dict())."""
        if self._ctx is None:
            return
        groups = {"v": self.v_optimizer, "q": self.q_optimizer, "pi": self.actor_optimizer}
        for p, off in self._param_offsets():
            opt = self._optimizer_of(p)
            grp_name = next(k for k, o in groups.items() if o is opt)
            t = self._adam_t[grp_name]
            if t == 0 and p not in opt.state:
                continue  # torch creates Adam state lazily at the first step
            st = opt.state[p]
            st["step"] = torch.tensor(float(t), dtype=torch.float32)
            st["exp_avg"] = self._m_arena[off: off + p.numel()].view(p.shape)
            st["exp_avg_sq"] = self._v_arena[off: off + p.numel()].view(p.shape)

    def _release(self) -> None:
        if self._ctx is not None:
            hb.check(hb.lib().iqlhip_destroy(self._ctx))
            self._ctx = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    # ------------------------------------------------------------------ scalars
    def _hyper_tuple(self):
        return (float(self.iql_tau), float(self.beta), float(self.discount), float(self.tau))

    def _hyper_struct(self) -> hb.Hyper:
        return hb.Hyper(self.iql_tau, self.beta, self.discount, self.tau, 1.0 - self.tau, EXP_ADV_MAX,
                        LOG_STD_MIN, LOG_STD_MAX)

    def _adam_hyper(self):
        ref = None
        for opt in (self.v_optimizer, self.q_optimizer, self.actor_optimizer):
            if len(opt.param_groups) != 1:
                raise NotImplementedError("one param group per optimizer expected (reference iql.py:673-675)")
            g = opt.param_groups[0]
            if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
                raise NotImplementedError("iqlhip implements torch.optim.Adam defaults only (no weight decay/amsgrad)")
            cur = (float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]))
            if ref is None:
                ref = cur
            elif cur != ref:
                raise NotImplementedError("the three optimizers must share betas and eps")
        return ref

    def _fill_scalars(self, sc: hb.StepScalars, t: Dict[str, int], lrs: Dict[str, float], inv_batch: float) -> None:
        b1, b2, eps = self._adam_hyper()
        for i, g in enumerate(("v", "q", "pi")):
            bc1 = 1.0 - b1 ** t[g]
            bc2 = 1.0 - b2 ** t[g]
            sc.step_size[i] = lrs[g] / bc1
            sc.bc2_sqrt[i] = bc2 ** 0.5
        sc.beta2 = b2
        sc.one_minus_beta1 = 1.0 - b1
        sc.one_minus_beta2 = 1.0 - b2
        sc.eps = eps
        sc.grad_scale = 1.0
        sc.inv_batch = inv_batch

    def _current_lrs(self) -> Dict[str, float]:
        return {"v": float(self.v_optimizer.param_groups[0]["lr"]),
                "q": float(self.q_optimizer.param_groups[0]["lr"]),
                "pi": float(self.actor_optimizer.param_groups[0]["lr"])}

    def _step_schedule(self) -> None:
        if self.actor_lr_schedule is not None:
            self.actor_optimizer._opt_called = True  # the Adam step ran inside libiqlhip
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                self.actor_lr_schedule.step()

    def _require_gpu(self) -> None:
        if self._ctx is None:
            raise RuntimeError(
                "iqlhip: ImplicitQLearning.train needs a GPU device (device='cuda'); there is no CPU "
                "implementation of the step in this package")

    def reserve_batch(self, rows: int) -> None:
        """Size the library's scratch for batches of up to `rows` rows now (otherwise it grows on first use)."""
        self._require_gpu()
        if rows > self._max_batch:
            self._attach(max_batch=(rows + 255) // 256 * 256)

    def set_step_stats(self, enabled: bool) -> None:
        """Opt in to (or out of) per-step training statistics: the 16 numbers of hb.STAT_NAMES (Q / V / advantage
        means, the advantage weights' clamp share, the three gradient norms), computed on the device
        from the batch each step trained on.  Enabled, train() and online_step() add them to their dict as
        "stats/<name>" and train_steps(..., return_stats=True) returns them per step.  Parameters, losses and random
        streams are the same with and without.  Not supported under data parallelism or for bf16 batches of more
        than 512 rows (NotImplementedError from the step).  Not part of the reference's surface."""
        self._step_stats = bool(enabled)

    def _check_step_stats(self, rows: int) -> None:
        """The two cases statistics are not built for — refused before anything is launched."""
        if not self._step_stats:
            return
        if self._dp_world > 1 or self._dp_exchange is not None:
            raise NotImplementedError("iqlhip: step statistics are not supported under data parallelism (the local "
                                      "gradient is not what Adam receives)")
        if getattr(self, "_precision", "f32") == "bf16" and rows > STATS_BF16_MAX_ROWS:
            raise NotImplementedError(f"iqlhip: step statistics are not supported for bf16 batches of more than "
                                      f"{STATS_BF16_MAX_ROWS} rows (got {rows}): the large-batch path keeps its row "
                                      "state in another layout")

    def set_grad_clip(self, max_norm) -> None:
        """Opt in to (or, with None, out of) gradient-norm clipping on the device: what
        `torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm)` between `loss.backward()` and `optimizer.step()`
        does in the reference, for each of the three optimizers on its own.  max_norm: a float (all
        three), a dict with any of "vf" / "qf" / "actor", or a (vf, qf, actor) triple; a value that is None, <= 0 or
        inf leaves that optimizer unclipped.  train(), online_step(), train_steps(), train_on_buffer() and the group
        calls honour it; flat_gradient() keeps returning the unclipped gradient.  A trainer setting like
        set_step_stats: part of neither state_dict() nor the hyper-parameters.  Not supported under data parallelism
        or for bf16 batches of more than 512 rows (NotImplementedError from the step)."""
        self._require_gpu()
        if max_norm is None:
            self._grad_clip = None
            return
        if isinstance(max_norm, dict):
            unknown = set(max_norm) - {"vf", "qf", "actor"}
            if unknown:
                raise ValueError(f"iqlhip: set_grad_clip: unknown optimizer(s) {sorted(unknown)} (vf, qf, actor)")
            vals = [max_norm.get(k) for k in ("vf", "qf", "actor")]
        elif isinstance(max_norm, (tuple, list)):
            if len(max_norm) != 3:
                raise ValueError("iqlhip: set_grad_clip takes a float, a dict or a (vf, qf, actor) triple")
            vals = list(max_norm)
        else:
            vals = [max_norm] * 3
        lim = []
        for v in vals:
            v = float("inf") if v is None else float(v)
            if v != v:
                raise ValueError("iqlhip: set_grad_clip: max_norm is NaN")
            lim.append(v if v > 0.0 else float("inf"))
        self._grad_clip = None if all(v == float("inf") for v in lim) else tuple(lim)

    @property
    def grad_clip(self) -> Optional[Tuple[float, float, float]]:
        """The (vf, qf, actor) max norms in force (inf = that optimizer is not clipped), or None when clipping is off."""
        return self._grad_clip

    def last_grad_clip(self) -> Dict[str, float]:
        """The last step's gradient norms before clipping and its clip coefficients, per optimizer."""
        self._require_gpu()
        if self._grad_clip is None or self._grad_clip_sent != self._grad_clip:
            raise ValueError("iqlhip: last_grad_clip() needs set_grad_clip(...) and a step taken since")
        out = (C.c_float * 6)()
        hb.check(hb.lib().iqlhip_read_grad_clip(self._ctx, out, self._stream()))
        keys = ("norm_vf", "norm_qf", "norm_actor", "coef_vf", "coef_qf", "coef_actor")
        return {k: float(out[i]) for i, k in enumerate(keys)}

    def _check_grad_clip(self, rows: int) -> None:
        """The two cases clipping is not built for — refused before anything is launched."""
        if self._grad_clip is None:
            return
        if self._dp_world > 1 or self._dp_exchange is not None:
            raise NotImplementedError("iqlhip: gradient clipping is not supported under data parallelism (the norm "
                                      "would have to be taken after the exchange)")
        if getattr(self, "_precision", "f32") == "bf16" and rows > STATS_BF16_MAX_ROWS:
            raise NotImplementedError(f"iqlhip: gradient clipping is not supported for bf16 batches of more than "
                                      f"{STATS_BF16_MAX_ROWS} rows (got {rows})")

    def _stats_entries(self) -> Dict[str, float]:
        """The last step's statistics as dict entries; nothing when they are off."""
        if not self._step_stats:
            return {}
        out = (C.c_float * hb.IQLHIP_N_STATS)()
        hb.check(hb.lib().iqlhip_read_step_stats(self._ctx, out, self._stream()))
        return {"stats/" + name: float(out[i]) for i, name in enumerate(hb.STAT_NAMES)}

    def _prepare(self, rows: int) -> None:
        self._check_step_stats(rows)
        self._check_grad_clip(rows)
        self._require_gpu()
        if rows > self._max_batch:
            self._attach(max_batch=(rows + 255) // 256 * 256)
        if self._hyper_tuple() != self._hyper_sent:
            h = self._hyper_struct()
            hb.check(hb.lib().iqlhip_set_hyper(self._ctx, C.byref(h)))
            self._hyper_sent = self._hyper_tuple()
        # actor dropout follows the module's mode, like nn.Dropout (active in train(), off in eval())
        p_eff = self._actor_dropout_p() if self.actor.training else 0.0
        if p_eff != self._dropout_sent:
            hb.check(hb.lib().iqlhip_set_dropout(self._ctx, p_eff, self._dropout_key()))
            self._dropout_sent = p_eff
            self._masks_injected = False      # (iqlhip_set_dropout clears injected masks)
        if self._step_stats != self._step_stats_sent:
            hb.check(hb.lib().iqlhip_set_step_stats(self._ctx, 1 if self._step_stats else 0))
            self._step_stats_sent = self._step_stats
        if self._grad_clip != self._grad_clip_sent:
            lim = (C.c_float * 3)(*(self._grad_clip or (0.0, 0.0, 0.0)))
            hb.check(hb.lib().iqlhip_set_grad_clip(self._ctx, lim))
            self._grad_clip_sent = self._grad_clip

    def _dropout_key(self) -> int:
        """The key of this trainer's keep-bit streams: set_dropout_seed(seed), else torch.initial_seed(), per rank."""
        rank = self._dp_rank if self._dp_world > 1 else 0
        seed = getattr(self, "_dropout_seed", None)
        if seed is None:
            seed = torch.initial_seed()
        return dp.rank_seed(seed, rank)

    def set_act_dropout(self, enabled: bool) -> None:
        """Opt in to (or out of) actor dropout inside the device inference forward.  The reference's online loop asks
        a training-mode actor for its next action (algorithms/finetune/iql.py:725-738), so an actor built with dropout
        acts through live nn.Dropout layers.  With the opt-in, `actor.act(state, "cuda")`, `actor_forward` and
        `online_step(act_next=...)` of such an actor run on the device with keep-bits drawn there (a stream of its own
        under the dropout key, one position per library call; DESIGN.md "Random streams"); in eval() mode, or with rate
        0, they run exactly as without it.  Default off: a training-mode dropout actor then acts through its PyTorch
        modules and act_next is refused.  Not part of the reference's surface."""
        self._act_dropout = bool(enabled)

    def acts_with_dropout(self) -> bool:
        """True if the actor's next act() applies dropout (training mode, rate > 0)."""
        return bool(self.actor.training and self._actor_dropout_p() > 0.0)

    def _prepare_act(self) -> None:
        """Before an inference call: the rate the forward applies (the module's, in training mode, once opted in) and
        the key, sent when they change.  A trainer that never opted in sends nothing: the context's rate is 0."""
        sent = self._act_dropout_sent
        if not self._act_dropout and sent is None:
            return
        p_eff = self._actor_dropout_p() if (self._act_dropout and self.actor.training) else 0.0
        if sent is None or sent[0] != p_eff or self._act_key_stale:      # (cached like _dropout_sent)
            pair = (p_eff, self._dropout_key())
            hb.check(hb.lib().iqlhip_set_act_dropout(self._ctx, *pair))
            self._act_dropout_sent, self._act_key_stale = pair, False

    def act_dropout_calls(self) -> int:
        """Position of the inference keep-bit stream: library inference calls that have drawn so far."""
        self._require_gpu()
        n = C.c_uint64(0)
        hb.check(hb.lib().iqlhip_get_act_dropout_counter(self._ctx, C.byref(n)))
        return int(n.value)

    def set_dropout_seed(self, seed: int) -> None:
        """Key this trainer's actor-dropout keep-bit stream with `seed` instead of the process's torch.initial_seed().
        Solo sweeps run one process per seed, so their streams differ by themselves; the members of one
        ImplicitQLearningGroup share a process and would all draw the same masks without it.  Takes effect with the
        next step (the stream position is kept).  Not part of the reference's surface."""
        self._dropout_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._dropout_sent = None        # (the next _prepare sends the rate and the new key)
        self._act_key_stale = True       # (... and the next inference call of an opted-in trainer)

    def _actor_dropout_p(self) -> float:
        """max p over the actor's nn.Dropout layers; the layer list is cached (walking named_modules costs ~13 us a
        step), the p values are read live."""
        mods = getattr(self, "_actor_dropouts", None)
        if mods is None or self._actor_dropouts_of is not self.actor:
            mods = [m for m in self.actor.modules() if isinstance(m, nn.Dropout)]
            self._actor_dropouts, self._actor_dropouts_of = mods, self.actor
        return float(max((m.p for m in mods), default=0.0))

    def _stream(self):
        # the raw handle of torch's CURRENT stream on our device (torch.cuda.current_stream() builds a Stream
        # object: ~4 us per call, three calls per step)
        return _raw_stream(self._dev.index)

    def _as_dev(self, t: torch.Tensor) -> torch.Tensor:
        if t.device != self._dev or t.dtype != torch.float32:
            t = t.to(self._dev, torch.float32)
        return t.contiguous()

    def _rows_of(self, t: torch.Tensor) -> Tuple[torch.Tensor, int]:
        """(tensor on our device, row stride in floats).  Row-strided views (what ReplayBuffer.sample returns: five
        views of one packed block) are passed through as they are — the library consumes such a block in place."""
        if t.device != self._dev or t.dtype != torch.float32:
            t = t.to(self._dev, torch.float32)
        if t.dim() == 2 and t.stride(0) >= t.shape[1] and (t.shape[1] == 1 or t.stride(1) == 1):
            return t, t.stride(0)
        if t.dim() == 1 and t.stride(0) >= 1:
            return t, t.stride(0)
        t = t.contiguous()
        return t, (t.shape[1] if t.dim() == 2 else 1)

    def _batch_struct(self, batch: TensorBatch):
        observations, actions, rewards, next_observations, dones = batch
        if isinstance(self.actor, DeterministicPolicy) or not self._gaussian:
            if actions.dim() != 2 or actions.shape[1] != self._A:
                raise RuntimeError("Actions shape missmatch")
        rows = [self._rows_of(x) for x in (observations, actions, rewards, next_observations, dones)]
        keep = [t for t, _ in rows]
        o, a, r, no, d = keep
        B = o.shape[0]
        if o.dim() != 2 or o.shape[1] != self._S or tuple(no.shape) != (B, self._S) or tuple(a.shape) != (B, self._A):
            raise ValueError(f"batch shapes do not match state_dim={self._S}, action_dim={self._A}")
        if r.numel() != B or d.numel() != B:
            raise ValueError("rewards / dones must have one element per row")
        b = hb.Batch(o.data_ptr(), a.data_ptr(), r.data_ptr(), no.data_ptr(), d.data_ptr(),
                     rows[0][1], rows[1][1], rows[2][1], rows[3][1], rows[4][1], None, B)
        return b, keep, B

    # ------------------------------------------------------------------ the step
    def _run_step(self, b: "hb.Batch", B: int, sync: bool, rw=None):
        self.total_it += 1
        for g in self._adam_t:
            self._adam_t[g] += 1
        sc = hb.StepScalars()
        lib = hb.lib()
        if self._dp_world > 1 and self._dp_exchange == "torch":
            # the collective issued by torch.distributed between the two halves of the step (two library calls)
            self._fill_scalars(sc, self._adam_t, self._current_lrs(), dp.inv_batch(B, self._dp_world))
            flat = self._dp_flat()
            hb.check(lib.iqlhip_forward_backward(self._ctx, C.byref(b), C.byref(sc), flat.data_ptr(), self._stream()))
            dp.reduce_and_update(
                flat, lambda f: hb.check(lib.iqlhip_apply_update(self._ctx, f.data_ptr(), C.byref(sc), self._stream())),
                self._dp_group)
        elif self._dp_exchange is not None:
            # in-library exchange (RCCL all-reduce or direct peer reads) inside iqlhip_step
            self._fill_scalars(sc, self._adam_t, self._current_lrs(), dp.inv_batch(B, self._dp_world))
            hb.check(lib.iqlhip_step(self._ctx, C.byref(b), C.byref(sc), self._stream()))
        elif rw is not None:
            # per-row loss weights: the row-weighted backward (iqlhip_step_rw); refused before any counter has moved
            self._fill_scalars(sc, self._adam_t, self._current_lrs(), 1.0 / B)
            rc = lib.iqlhip_step_rw(self._ctx, C.byref(b), C.byref(sc), rw[0], rw[1], self._stream())
            if rc:
                self.total_it -= 1
                for g in self._adam_t:
                    self._adam_t[g] -= 1
                hb.check(rc)
        else:
            self._fill_scalars(sc, self._adam_t, self._current_lrs(), 1.0 / B)
            hb.check(lib.iqlhip_step(self._ctx, C.byref(b), C.byref(sc), self._stream()))
        self._advance_schedule(1)        # == actor_lr_schedule.step(), bit for bit, without torch's ~15 us of Python
        if not sync:
            return None
        out = (C.c_float * 3)()
        hb.check(lib.iqlhip_read_losses(self._ctx, out, self._stream()))
        log = {"value_loss": float(out[0]), "q_loss": float(out[1]), "actor_loss": float(out[2])}
        if self._step_stats:
            log.update(self._stats_entries())
        return log

    def _loss_weight_args(self, B: int, loss_weights, return_td: bool):
        """(row-weight pointer, TD pointer or None, tensors to keep alive) of a weighted step, checked on the host."""
        if self._dp_world > 1 or self._dp_exchange is not None:
            raise NotImplementedError("iqlhip: per-row loss weights (loss_weights / return_td) are not supported under "
                                      "data parallelism")
        if getattr(self, "_precision", "f32") == "bf16":
            raise NotImplementedError("iqlhip: per-row loss weights (loss_weights / return_td) are not supported at bf16 "
                                      "precision: the row-weighted backward is an fp32 kernel")
        if loss_weights is None:
            ones = getattr(self, "_rw_ones", None)
            if ones is None or ones.numel() < B:
                ones = self._rw_ones = torch.ones(max(B, 256), dtype=torch.float32, device=self._dev)
            w = ones
        else:
            w = check_loss_weights(loss_weights, B, self._dev)
        td = None
        if return_td:
            td = torch.empty((B, 2), dtype=torch.float32, device=self._dev)
        return w, td

    def last_td_errors(self) -> torch.Tensor:
        """[B, 2] float32 on the device: (q1 - y, q2 - y) of every row of the last train(..., return_td=True) step — the
        pre-update values its loss used.  Valid until the trainer's next step."""
        td = getattr(self, "_last_td", None)
        if td is not None and getattr(self, "_last_td_it", None) != self.total_it:
            td = self._last_td = None          # (a later step of any kind — train, train_steps*, online_step* — has run)
        if td is None:
            raise RuntimeError("iqlhip: no TD errors: the trainer's last step was not a train(..., return_td=True)")
        if isinstance(td, tuple):              # (online_step_prioritized: the library holds them; copied when asked for)
            rows = td[1]
            td = torch.empty((rows, 2), dtype=torch.float32, device=self._dev)
            hb.check(hb.lib().iqlhip_online_prioritized_batch(self._ctx, rows, None, td.data_ptr(), self._stream()))
            self._last_td = td
        return td

    def last_prioritized_indices(self) -> torch.Tensor:
        """[B] int64 on the device: the rows the last online_step_prioritized drew, in batch order (the rows of
        last_td_errors()).  Valid until the trainer's next step."""
        mark = getattr(self, "_last_prio_idx", None)
        if mark is None or mark[0] != self.total_it:
            raise RuntimeError("iqlhip: no drawn indices: the trainer's last step was not an online_step_prioritized")
        idx = torch.empty(mark[1], dtype=torch.int64, device=self._dev)
        hb.check(hb.lib().iqlhip_online_prioritized_batch(self._ctx, mark[1], idx.data_ptr(), None, self._stream()))
        return idx

    def train(self, batch: TensorBatch, loss_weights=None, return_td: bool = False) -> Dict[str, float]:
        """One IQL gradient step (iql.py:542-563).  Returns the three losses as floats
        (one host sync instead of the reference's three .item() calls).

        loss_weights ([B] or [B, 1] float32 on the trainer's device): every row's loss terms are multiplied by its
        weight — the importance-sampling correction of a weighted draw (buffer.draw_weighted_indices(..., is_beta=...)
        returns such weights); the returned losses are the weighted ones.  return_td: the rows' TD errors are kept for
        last_td_errors() (without loss_weights the weights are ones).  fp32 only, no data parallelism."""
        self._require_gpu()
        if loss_weights is not None or return_td:
            self._last_td = None
            b, keep, B = self._batch_struct(batch)
            w, td = self._loss_weight_args(B, loss_weights, return_td)
            self._prepare(B)
            log = self._run_step(b, B, sync=True, rw=(w.data_ptr(), None if td is None else td.data_ptr()))
            self._last_td, self._last_td_it = td, self.total_it
            del keep, w
            return log
        fast = self._fresh_block_batch(batch)
        if fast is not None:
            return self._train_fresh_block(*fast)
        b, keep, B = self._batch_struct(batch)
        self._prepare(B)
        log = self._run_step(b, B, sync=True)
        del keep
        return log

    # ---- the reference loop's `batch = buffer.sample(B); trainer.train(batch)` (finetune/iql.py:771-773): the batch IS
    # the block ReplayBuffer.sample just gathered — no per-tensor inspection, scalars computed while the GPU ran the
    # previous step, losses through host-mapped words the library spins on (iqlhip_step_sync)
    def _fresh_block_batch(self, batch):
        import iqlhip_replay as rp
        lb = rp._last_block
        if lb is None or self._dp_world > 1 or len(batch) != 5:
            return None
        ptr, B, S, A, ld, dev = lb
        o = batch[0]
        if o.data_ptr() != ptr or S != self._S or A != self._A or dev != self._dev or o.shape[0] != B:
            return None
        # the other four must be that block's views too (a caller may have swapped one for its own tensor)
        if (batch[1].data_ptr() != ptr + 4 * S or batch[3].data_ptr() != ptr + 4 * (S + A)
                or batch[2].data_ptr() != ptr + 4 * (2 * S + A) or batch[4].data_ptr() != ptr + 4 * (2 * S + A + 1)):
            return None
        return ptr, B, ld

    def _train_fresh_block(self, ptr: int, B: int, ld: int) -> Dict[str, float]:
        self._prepare(B)
        S, A = self._S, self._A
        b = hb.Batch(ptr, ptr + 4 * S, ptr + 4 * (2 * S + A), ptr + 4 * (S + A), ptr + 4 * (2 * S + A + 1),
                     ld, ld, ld, ld, ld, None, B)
        inv_batch = 1.0 / B
        pre = self._eager_next
        self._eager_next = None
        key = self._table_key(inv_batch)
        if pre is not None and pre[0] == key:
            sc, lr_after, sched_after = pre[1], pre[2], pre[3]
        else:
            t1 = {g: t + 1 for g, t in self._adam_t.items()}
            sc = hb.StepScalars()
            self._fill_scalars(sc, t1, self._current_lrs(), inv_batch)
            pk = self._peek_schedule(1)
            lr_after, sched_after = (None, None) if pk is None else (None, pk[1])
        lib, stream, out = hb.lib(), self._stream(), self._loss_out
        rc = lib.iqlhip_step_begin(self._ctx, C.byref(b), C.byref(sc), stream)
        if rc:
            hb.check(rc)
        # ---- the GPU runs the step: host bookkeeping and the NEXT step's scalars (float64 Adam bias corrections, the
        # cosine learning rate) now; a set computed ahead is used only if nothing it depends on has changed by then
        self.total_it += 1
        for g in self._adam_t:
            self._adam_t[g] += 1
        if sched_after is not None:
            self._commit_schedule(sched_after)
        else:
            self._advance_schedule(1)
        pk = self._peek_schedule(1)
        if pk is not None:
            t2 = {g: t + 1 for g, t in self._adam_t.items()}
            sc2 = hb.StepScalars()
            self._fill_scalars(sc2, t2, self._current_lrs(), inv_batch)
            self._eager_next = (self._table_key(inv_batch), sc2, None, pk[1])
        rc = lib.iqlhip_step_wait(self._ctx, out, stream)
        if rc:
            hb.check(rc)
        log = {"value_loss": float(out[0]), "q_loss": float(out[1]), "actor_loss": float(out[2])}
        if self._step_stats:
            log.update(self._stats_entries())
        return log

    # ---- the online iteration: one driver behind every online_step* method ---------------------------------------
    def _online_row(self, buf, state, action, reward, next_state, done) -> np.ndarray:
        """The new transition as one packed host row [ld] (pad columns zero)."""
        row = self._on_row
        if row.shape[0] != buf._ld:      # (a ring of another stride: the library reads ld floats of the row)
            row = self._on_row = np.zeros(buf._ld, dtype=np.float32)
        pack_transition(row, self._S, self._A, state, action, reward, next_state, done)
        return row

    def _act_next_args(self, act_next, rows: Optional[int] = None):
        """(state in, action out, noise seed) of the call's act forward; (None, None, 0) without act_next.  rows: the
        states of a vector call, [rows, S] in and [rows, A] out."""
        if act_next is None:
            return None, None, 0
        if self.acts_with_dropout() and not self._act_dropout:
            raise NotImplementedError("act_next: the library's inference forward is eval-mode (no actor dropout) "
                                      "unless set_act_dropout(True) was called")
        self._prepare_act()
        a_in = np.ascontiguousarray(np.asarray(act_next, dtype=np.float32).reshape(-1))
        a_out = np.empty(self._A if rows is None else (rows, self._A), dtype=np.float32)
        return a_in, a_out, (self._act_seed() if (self.actor.training and self._gaussian) else 0)

    def _commit_online(self, ring, pointer: int, new_size: int, rows: int, steps: int, adam_after, commit_extra=None) -> None:
        """What a successful online call moves — the one place for both drivers: the ring's counters past the `rows`
        written from `pointer` on, total_it, the Adam step counts and the schedule by `steps`, then commit_extra()."""
        ring._writes += rows
        ring._advance(pointer, new_size, rows)
        self.total_it += steps
        self._adam_t = adam_after
        if steps:
            self._advance_schedule(steps)
        if commit_extra is not None:
            commit_extra()

    def _run_online(self, ring, transition, act_next, draw, inv_batch: float, call, commit_extra=None):
        """Insert one transition into `ring`, draw a batch, take one step and (with act_next) act, in the one library
        call `call` makes — what every online_step* method does once its own checks have passed.
        transition: (state, action, reward, next_state, done).  draw(new_size): the batch's host indices over the size
        after the insert, an int64 array; None for a call that draws on the device.  inv_batch: what the step's
        scalars carry — dp.inv_batch(batch_size, world) from the callers that run under data parallelism, 1.0 /
        batch_size from those that refuse it (world = 1: the two coincide).  call(ring_args, row, idx, sc, out, act_args,
        stream) returns the library's status: ring_args = (rows, ld, capacity, pointer) and act_args = (state in,
        max_action, seed, action out) are in the library's argument order, row and idx are host addresses (idx None
        without draw), sc is the scalars by reference, out the three losses.  The global numpy stream is consumed
        by draw alone, behind the row and in front of the act seed.  Only when the status is OK does anything move:
        the ring's counters, total_it, the Adam step counts and the schedule — then commit_extra(), for what one
        variant moves besides.  Returns train()'s dict, or (dict, action) with act_next."""
        row = self._online_row(ring, *transition)
        pointer, new_size = ring._insert_slot()
        idx = None if draw is None else draw(new_size)
        adam_next = {g: t + 1 for g, t in self._adam_t.items()}
        sc, out = self._on_scalars, self._loss_out          # (both are read and written inside the call alone)
        self._fill_scalars(sc, adam_next, self._current_lrs(), inv_batch)
        a_in, a_out, seed = self._act_next_args(act_next)
        act_args = (None if a_in is None else a_in.ctypes.data, float(self.actor.max_action), seed,
                    None if a_out is None else a_out.ctypes.data)
        hb.check(call((ring._rows.data_ptr(), ring._ld, ring._buffer_size, pointer), row.ctypes.data,
                      None if idx is None else idx.ctypes.data, C.byref(sc), out, act_args, self._stream()))
        self._commit_online(ring, pointer, new_size, 1, 1, adam_next, commit_extra)
        log = {"value_loss": float(out[0]), "q_loss": float(out[1]), "actor_loss": float(out[2])}
        if self._step_stats:
            log.update(self._stats_entries())
        return log if a_out is None else (log, a_out)

    def _run_online_vec(self, ring, transitions, batch_size: int, updates: int, act_next, act_rows: int, call):
        """_run_online's sibling for E transitions and U = `updates` steps in the one library call `call` makes, once the
        caller's checks have passed.  transitions: (states, actions, rewards, next_states, dones) of E rows.
        call(ring_args, rows, n_rows, idx, scs, out, act_args, stream) returns the library's status: ring_args = (rows,
        ld, capacity, pointer), rows the E packed host rows, idx the U * batch_size host indices (None with U = 0), scs the
        U sets of step scalars, out [U][3]; act_args = (states in, rows, max_action, seed, actions out).  The global
        numpy stream is consumed by the U index draws alone — U consecutive sample() draws over the size after all E
        inserts — behind the packed rows and in front of the act seed.  The scalars are what U single steps would use:
        the Adam counts t + 1 .. t + U and the actor rates the schedule gives them, looked up ahead.  Only when the
        status is OK does anything move (_commit_online).  Returns the U dicts, or (dicts, actions) with act_next."""
        S, A = self._S, self._A
        E = len(transitions[0])
        rows = np.zeros((E, ring._ld), dtype=np.float32)
        pack_transitions(rows, S, A, *transitions)
        pointer, new_size = ring._insert_slot(E)
        U, B = updates, batch_size
        idx = np.concatenate([draw_indices(new_size, B) for _ in range(U)]) if U else None
        lrs = self._current_lrs()
        pk = self._peek_schedule(U) if U else None
        if U > 1 and pk is None:
            raise NotImplementedError("iqlhip: online_step_vec with updates > 1 needs an actor schedule whose rates can "
                                      "be looked up ahead (CosineAnnealingLR with eta_min = 0, stepped by this trainer)")
        lr_pi = [lrs["pi"]] if pk is None else pk[0]      # (one step: the rate in force, whatever the schedule's state)
        scs = (hb.StepScalars * max(U, 1))()
        for u in range(U):
            self._fill_scalars(scs[u], {g: t + u + 1 for g, t in self._adam_t.items()}, dict(lrs, pi=float(lr_pi[u])), 1.0 / B)
        out = (C.c_float * (3 * max(U, 1)))()
        a_in, a_out, seed = self._act_next_args(act_next, act_rows)
        act_args = (None if a_in is None else a_in.ctypes.data, act_rows, float(self.actor.max_action), seed,
                    None if a_out is None else a_out.ctypes.data)
        stream = self._stream()
        hb.check(call((ring._rows.data_ptr(), ring._ld, ring._buffer_size, pointer), rows.ctypes.data, E,
                      None if idx is None else idx.ctypes.data, scs, out, act_args, stream))
        self._commit_online(ring, pointer, new_size, E, U, {g: t + U for g, t in self._adam_t.items()})
        logs = [{"value_loss": float(out[3 * u]), "q_loss": float(out[3 * u + 1]), "actor_loss": float(out[3 * u + 2])}
                for u in range(U)]
        if self._step_stats and U:
            stats = np.empty((U, hb.IQLHIP_N_STATS), dtype=np.float32)
            self._read_rings(U, stream, None, stats)
            for u, log in enumerate(logs):
                log.update({"stats/" + name: float(stats[u, i]) for i, name in enumerate(hb.STAT_NAMES)})
        return logs if a_out is None else (logs, a_out)

    def online_step_vec(self, replay_buffer, states, actions, rewards, next_states, dones, batch_size: int,
                        updates: int = 1, act_next=None):
        """One iteration of an online loop over E environments with an update-to-data ratio of `updates`, in ONE library
        call and under one synchronisation (iqlhip_online_step_vec).  Bit for bit the sequence
            for e in range(E): replay_buffer.add_transition(states[e], actions[e], rewards[e], next_states[e], dones[e])
            logs = [trainer.train(replay_buffer.sample(batch_size)) for _ in range(updates)]
            acts = trainer.actor_forward(act_next, sample=trainer.actor.training)     # with act_next [E2, S]
        states / next_states [E, S], actions [E, A], rewards / dones [E]; 1 <= E <= min(capacity, 64), 0 <= updates <= 32,
        batch_size <= 512, 1 <= E2 <= 64 (E2 need not equal E: the caller resets the envs that ended).  updates = 0 is
        the loop's warm-up — rows in, actions out, no gradient step: returns [] and moves no step counter.  The indices are
        `updates` consecutive sample() draws from the global numpy stream over the size after all E inserts.  Returns the
        list of `updates` dicts like train()'s (each with its own step's statistics under set_step_stats), or (list,
        actions [E2, A] float32) with act_next; the act() noise counter and the act-dropout counter advance once.
        last_grad_clip() reports the last step.  ValueError for sizes out of range and shapes that disagree;
        NotImplementedError under data parallelism, with injected dropout masks pending, at bf16 precision above 512
        rows, for a ring with a tracking sample-weight table and for act_next of a training-mode dropout actor without
        set_act_dropout(True) — all before anything is launched, drawn or moved."""
        self._require_gpu()
        buf = replay_buffer
        check_online_ring(buf, self._dev, "online_step_vec")
        U, B = int(updates), int(batch_size)
        if self._dp_world > 1 or self._dp_exchange is not None:
            raise NotImplementedError("iqlhip: online_step_vec is not supported under data parallelism")
        if buf._weights_tracks:
            raise NotImplementedError("iqlhip: online_step_vec has no insert for a tracking sample-weight table; use "
                                      "add_transitions and online_step_prioritized's sequence")
        if getattr(self, "_precision", "f32") == "bf16" and B > STATS_BF16_MAX_ROWS:
            raise NotImplementedError(f"iqlhip: online_step_vec runs the small-batch kernels: bf16 batches of more than "
                                      f"{STATS_BF16_MAX_ROWS} rows are not supported (got {B})")
        if not 0 <= U <= hb.IQLHIP_VEC_MAX_UPDATES:
            raise ValueError(f"iqlhip: updates = {U} outside [0, {hb.IQLHIP_VEC_MAX_UPDATES}]")
        if not 1 <= B <= VEC_MAX_BATCH:
            raise ValueError(f"iqlhip: batch_size = {B} outside [1, {VEC_MAX_BATCH}]")
        check_transitions(self._S, self._A, buf._buffer_size, states, actions, rewards, next_states, dones)
        act_rows = 0
        if act_next is not None:
            act_next = np.asarray(act_next, dtype=np.float32)
            if act_next.ndim != 2 or act_next.shape[1] != self._S or not 1 <= act_next.shape[0] <= hb.IQLHIP_VEC_MAX_ENVS:
                raise ValueError(f"iqlhip: act_next must be [E2, {self._S}] with 1 <= E2 <= {hb.IQLHIP_VEC_MAX_ENVS}, got "
                                 f"{list(act_next.shape)}")
            act_rows = act_next.shape[0]
            if self.acts_with_dropout() and not self._act_dropout:      # (_act_next_args' refusal, in front of the index draw)
                raise NotImplementedError("act_next: the library's inference forward is eval-mode (no actor dropout) "
                                          "unless set_act_dropout(True) was called")
        self._prepare(B)
        if getattr(self, "_masks_injected", False):
            raise NotImplementedError("iqlhip: online_step_vec draws every step's keep-bits and cannot use the masks written "
                                      "by inject_dropout_masks; step with train(), or clear them (set_dropout_seed)")

        def call(ring_args, rows, n_rows, idx, scs, out, act_args, stream):
            a_in, a_rows, max_action, seed, a_out = act_args
            return hb.lib().iqlhip_online_step_vec(self._ctx, *ring_args, rows, n_rows, idx, B, U, C.addressof(scs), C.addressof(out),
                                                   a_in, a_rows, max_action, seed, a_out, stream)
        return self._run_online_vec(buf, (states, actions, rewards, next_states, dones), B, U, act_next, act_rows, call)

    def online_step(self, replay_buffer, state, action, reward: float, next_state, done: bool,
                    batch_size: int, act_next: Optional[np.ndarray] = None):
        """One iteration of the online loop's buffer + training work in ONE library call (reference sequence:
        `replay_buffer.add_transition(...)`, `batch = replay_buffer.sample(batch_size)`, `trainer.train(batch)` —
        algorithms/finetune/iql.py:741-773, jsrl_w_iql.py:512-548): the transition is stored at the ring pointer, the
        batch indices are drawn by np.random.randint over the NEW size (same global-RNG draw as sample()), the rows
        are gathered and the step runs; returns train()'s dict.  Equivalent to the three calls, bit for bit.
        `act_next` (a state, normally `next_state` unless the episode ended) additionally returns
        `self.actor.act(act_next, device)` evaluated with the UPDATED policy — what the loop's next iteration would
        compute first (iql.py:728) — under the same single synchronisation: returns (log, action)."""
        self._prepare(batch_size)
        check_online_ring(replay_buffer, self._dev, "online_step")
        if self._dp_world > 1 and self._dp_exchange == "torch":
            raise NotImplementedError("online_step runs the whole step in one library call: it needs an in-library "
                                      "exchange, enable_data_parallel(exchange='rccl'|'p2p') — with exchange='torch' "
                                      "use add_transition / sample / train")

        def call(ring_args, row, idx, sc, out, act_args, stream):
            return hb.lib().iqlhip_online_step(self._ctx, *ring_args, row, idx, batch_size, sc, out, *act_args, stream)
        return self._run_online(replay_buffer, (state, action, reward, next_state, done), act_next,
                                lambda new_size: draw_indices(new_size, batch_size),
                                dp.inv_batch(batch_size, self._dp_world), call)

    def online_step_nstep(self, nstep, state, action, reward: float, next_state, done: bool, batch_size: int,
                          episode_end: Optional[bool] = None, act_next: Optional[np.ndarray] = None):
        """online_step for a raw ring and the n-step buffer derived from it (an iqlhip_nstep.NStepReplay; DESIGN.md
        6c-3), in ONE library call and under one synchronisation.  Bit for bit the sequence
            nstep.add_transition(state, action, reward, next_state, done, episode_end)
            log = trainer.train(nstep.buffer.sample(batch_size))
            a = trainer.actor.act(act_next, device)  # with act_next
        The indices are sample()'s draw over the size after the insert.  Returns online_step's result.
        NotImplementedError under data parallelism and for a derived buffer with a tracking sample-weight table."""
        from iqlhip_nstep import online_step_nstep
        return online_step_nstep(self, nstep, state, action, reward, next_state, done, batch_size, episode_end, act_next)

    def online_step_prioritized(self, replay_buffer, state, action, reward: float, next_state, done: bool,
                                batch_size: int, seed: int, offset: Optional[int] = None, alpha: float = 0.6,
                                eps: float = 1e-6, is_beta: float = 0.4, act_next: Optional[np.ndarray] = None):
        """online_step with prioritised replay, in ONE library call and under one synchronisation.  The buffer's table
        must track its maximum (set_sample_weights(..., updatable=True, track_max=True)).  Bit for bit the sequence
            buf.add_transition(...)                  # the new row enters at the table's largest priority
            idx, c = buf.draw_weighted_indices(B, seed, offset, is_beta=is_beta, batch_size=B)
            log = trainer.train(buf.gather(idx), loss_weights=c, return_td=True)
            buf.update_sample_weights_td(idx, trainer.last_td_errors(), alpha, eps)
            a = trainer.actor.act(act_next, device)  # with act_next
        The draw runs behind the insert, so the new row can be drawn.  offset: the Philox counter the draw starts at;
        None continues a per-buffer counter that advances by ceil(batch_size / 2) per call (the counters one draw
        consumes); an explicit offset is used and sets the counter.  Returns online_step's result; last_td_errors()
        and last_prioritized_indices() work after the call.  ValueError for a buffer without a tracking table and for
        alpha, eps or is_beta negative, not finite (or alpha = eps = 0); NotImplementedError at bf16 precision, under
        data parallelism and with injected dropout masks pending — all before anything moves."""
        import iqlhip_weighted as wtd
        self._require_gpu()
        buf = replay_buffer
        check_online_ring(buf, self._dev, "online_step_prioritized")
        wtd.check_call(buf)
        if not buf._weights_updatable or not buf._weights_tracks:
            raise ValueError("iqlhip: online_step_prioritized needs sample weights that track their maximum "
                             "(set_sample_weights(..., updatable=True, track_max=True))")
        if self._dp_world > 1 or self._dp_exchange is not None:
            raise NotImplementedError("iqlhip: online_step_prioritized is not supported under data parallelism")
        alpha, eps = wtd.check_priority_args(alpha, eps)
        beta = self._is_beta_arg(is_beta)
        self._prepare(batch_size)
        self._refuse_injected_masks()
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        off = (getattr(buf, "_prio_online_offset", 0) if offset is None else int(offset)) & 0xFFFFFFFFFFFFFFFF

        def call(ring_args, row, idx, sc, out, act_args, stream):
            # (the one side effect of a `call`: the library may overwrite the device's TD errors before it fails, so the
            # previous ones are given up here, behind every check and immediately in front of the library call)
            self._last_td = None
            return hb.lib().iqlhip_online_step_prioritized(self._ctx, *ring_args, row, batch_size, sc, out, *act_args, stream,
                                                           buf._weights, seed, off, beta, alpha, eps)

        def commit_extra():
            buf._weights_version += 2            # (the insert and the update, as the library counts them)
            buf._prio_online_offset = (off + wtd.online_offset_step(batch_size)) & 0xFFFFFFFFFFFFFFFF
            self._last_td, self._last_td_it = ("online", batch_size), self.total_it
            self._last_prio_idx = (self.total_it, batch_size)
        return self._run_online(buf, (state, action, reward, next_state, done), act_next, None, 1.0 / batch_size, call,
                                commit_extra)

    def online_step_jsrl(self, jsrl, replay_buffer, state, action, reward: float, next_state, done: bool,
                         batch_size: int, act_next, who, gate_max=None):
        """online_step(...) plus the guide-or-learner selection of the next action (jsrl_utils.learner_or_guide_action)
        with the UPDATED learner, under one synchronisation: returns (log, action, use_learner, horizon).  `jsrl` is a
        JsrlActors of one member whose learner is this trainer (iqlhip_jsrl.py)."""
        from iqlhip_jsrl import online_step_jsrl
        return online_step_jsrl(self, jsrl, replay_buffer, state, action, reward, next_state, done, batch_size,
                                act_next, who, gate_max)

    # ---- scoring without a step (iqlhip_score.py) -------------------------------------------------
    def _score_call(self, rows_ptr: int, ld: int, n_rows: int, start: int, n: int, idx, out, summary: bool, chunk: int):
        """The library call behind score_buffer / score / evaluate; every argument has been checked."""
        if self._hyper_tuple() != self._hyper_sent:      # beta, discount, iql_tau: what the next step would send too
            h = self._hyper_struct()
            hb.check(hb.lib().iqlhip_set_hyper(self._ctx, C.byref(h)))
            self._hyper_sent = self._hyper_tuple()
        if idx is not None and not (isinstance(idx, torch.Tensor) and idx.device == self._dev):
            idx = torch.as_tensor(idx).to(self._dev)
        if idx is not None:
            idx = idx.contiguous()
        if out is None:
            out = torch.empty((n, hb.IQLHIP_N_SCORE), dtype=torch.float32, device=self._dev)
        words = (C.c_float * 11)() if summary else None
        hb.check(hb.lib().iqlhip_score_rows(
            self._ctx, rows_ptr, ld, n_rows, start, n, None if idx is None else idx.data_ptr(),
            None if out is False else out.data_ptr(), chunk, words, self._stream()))
        import iqlhip_score as score
        return (None if out is False else out), (score.summary_dict(words) if summary else None)

    def score_buffer(self, buffer, start: int = 0, n: Optional[int] = None, indices=None, out=None, summary: bool = True,
                     chunk_rows: Optional[int] = None):
        """What the networks think of transitions of `buffer`, without a gradient step: (scores, summary).  scores is an
        [n, 8] float32 tensor on the buffer's device with the columns hb.SCORE_NAMES — v, next_v, q1, q2, target_q
        (the target nets' minimum), adv, exp_adv (clamped at 100), bc (the row's behaviour-cloning term) — of the rows
        [start, start + n) (n=None: to the buffer's end) or of the rows `indices` names, in its order (a 1-D int64
        tensor or array, host or device).  out: a tensor to write into, or False to skip the per-row store.  summary: a
        dict of value_loss, q_loss, actor_loss — train()'s three, as means over the n rows — and mean_<column>; None when
        summary=False.  The policy is evaluated as actor.eval() would (no dropout); parameters are the fp32 masters and
        the arithmetic fp32, also after set_precision("bf16").  A row's eight numbers do not depend on n, chunk_rows,
        its place in the call or how it is addressed.  Nothing the trainer holds changes.  ValueError for a CPU buffer,
        foreign dims or stride, an empty buffer or range, a range beyond len(buffer), a wrong out, both start / n and
        indices; IndexError for an index outside the buffer; RuntimeError on a CPU trainer — all before any row is read.
        Not part of the reference's surface."""
        import iqlhip_score as score
        self._require_gpu()
        size = score.check_buffer(buffer, self._dev, self._S, self._A, hb.row_stride(self._S, self._A))
        start, count, idx = score.resolve_rows(size, start, n, indices)
        if out is not None and out is not False:
            score.check_out(out, count, self._dev)
        if out is False and not summary:
            raise ValueError("iqlhip: nothing to compute (out=False and summary=False)")
        chunk = score.check_chunk_rows(chunk_rows)
        return self._score_call(buffer._rows.data_ptr(), buffer._ld, size, start, count, idx, out, summary, chunk)

    def score(self, batch: TensorBatch, out=None, summary: bool = True, chunk_rows: Optional[int] = None):
        """score_buffer for a five-tensor batch as train() takes it, of any length: the batch is packed into a temporary
        block of rows and scored there."""
        import iqlhip_score as score
        self._require_gpu()
        b, keep, B = self._batch_struct(batch)
        if B < 1:
            raise ValueError("iqlhip: an empty batch")
        if out is not None and out is not False:
            score.check_out(out, B, self._dev)
        if out is False and not summary:
            raise ValueError("iqlhip: nothing to compute (out=False and summary=False)")
        chunk = score.check_chunk_rows(chunk_rows)
        ld = hb.row_stride(self._S, self._A)
        block = torch.empty((B, ld), dtype=torch.float32, device=self._dev)
        hb.check(hb.lib().iqlhip_pack_rows(self._ctx, C.byref(b), block.data_ptr(), self._stream()))
        res = self._score_call(block.data_ptr(), ld, B, 0, B, None, out, summary, chunk)
        if not summary:      # (with a summary the call has waited for the stream; otherwise the block must outlive it)
            block.record_stream(torch.cuda.current_stream(self._dev))
        del keep
        return res

    def evaluate(self, batch: TensorBatch) -> Dict[str, float]:
        """train()'s three keys for `batch`, computed without a step: nothing the trainer holds changes.  The policy is
        in eval mode (no dropout), as actor.eval() would be."""
        _, summary = self.score(batch, out=False, summary=True)
        return {k: summary[k] for k in ("value_loss", "q_loss", "actor_loss")}

    # ---- batches mixed from an offline and an online buffer (iqlhip_mixed.py) ----------------------
    def _mixed_args(self, offline_buffer, online_buffer, batch_size: int, mixing_ratio: float) -> Tuple[int, int]:
        """The checks both mixed calls make before anything is launched or any counter moves; returns (n_off, n_on)."""
        import iqlhip_mixed as mixed
        self._require_gpu()
        n_off, n_on = mixed.split(batch_size, mixing_ratio)
        mixed.check_buffers(offline_buffer, online_buffer, self._dev, self._S, self._A)
        if self._dp_world > 1 or self._dp_exchange is not None:
            raise NotImplementedError("iqlhip: mixed batches are not supported under data parallelism")
        if getattr(self, "_precision", "f32") == "bf16" and batch_size > STATS_BF16_MAX_ROWS:
            raise NotImplementedError(f"iqlhip: mixed batches are not supported for bf16 batches of more than "
                                      f"{STATS_BF16_MAX_ROWS} rows (got {batch_size}): the large-batch kernels stage "
                                      "their rows from one buffer")
        if offline_buffer._size < 1:
            raise ValueError("iqlhip: the offline replay buffer is empty")
        return n_off, n_on

    def online_step_mixed(self, offline_buffer, online_buffer, state, action, reward: float, next_state, done: bool,
                          batch_size: int, mixing_ratio: float = 0.5, act_next: Optional[np.ndarray] = None):
        """online_step with the batch mixed from two buffers, as the reference's Cal-QL loop builds it
        (algorithms/finetune/cal_ql.py: mixing_ratio): the transition goes into `online_buffer`, and the step trains on
        `n_off = int(batch_size * mixing_ratio)` rows of `offline_buffer` followed by `batch_size - n_off` rows of
        `online_buffer` — one library call.  Bit for bit `online_buffer.add_transition(...)`,
        `offline_buffer.sample(n_off)`, `online_buffer.sample(n_on)`, `train(vstack of the two)`, the global numpy RNG
        consumed in that order (the online draw over the size after the insert).  act_next, step statistics, clipping
        and set_act_dropout behave as in online_step.  ValueError unless 1 <= n_off <= batch_size - 1 and both buffers
        are distinct finetune ReplayBuffers of the trainer's dimensions on its GPU; NotImplementedError under data
        parallelism and for bf16 batches of more than 512 rows."""
        import iqlhip_mixed as mixed
        n_off, n_on = self._mixed_args(offline_buffer, online_buffer, batch_size, mixing_ratio)
        self._prepare(batch_size)
        idx_off = None

        def draw(new_size):
            nonlocal idx_off
            idx_off, idx_on = mixed.draw_host_indices(offline_buffer._size, n_off, new_size, n_on)
            return idx_on

        def call(ring_args, row, idx, sc, out, act_args, stream):
            return hb.lib().iqlhip_online_step_mixed(self._ctx, *ring_args, row, idx, n_on, sc, out, *act_args, stream,
                                                     offline_buffer._rows.data_ptr(), offline_buffer._size,
                                                     idx_off.ctypes.data, n_off)
        return self._run_online(online_buffer, (state, action, reward, next_state, done), act_next, draw, 1.0 / batch_size,
                                call)

    def prepare_train_steps_mixed(self, offline_buffer, online_buffer, batch_size: int, mixing_ratio: float = 0.5) -> None:
        """prepare_train_steps for the chunk graphs train_steps_mixed replays on this pair of buffers and this split."""
        n_off, _ = self._mixed_args(offline_buffer, online_buffer, batch_size, mixing_ratio)
        self._prepare(batch_size)
        self._refuse_injected_masks()
        hb.check(hb.lib().iqlhip_train_steps_mixed_prepare(
            self._ctx, offline_buffer._rows.data_ptr(), online_buffer._rows.data_ptr(), offline_buffer._ld, batch_size,
            n_off, 1.0 / batch_size, self._stream()))
        self._ts_token = None

    def train_steps_mixed(self, offline_buffer, online_buffer, n_steps: int, batch_size: int, mixing_ratio: float = 0.5,
                          seed: int = 0, return_losses: bool = True, chunk: int = K_MAX, return_stats: bool = False):
        """train_steps with every batch mixed from two buffers: the bursts of updates online fine-tuning runs after an
        episode (or an update-to-data ratio above 1) without a host round trip per step.  The device index stream is
        train_steps' own (Philox keyed by (seed, total_it); index k * batch_size + r of a call belongs to step k, batch
        row r); row r < n_off = int(batch_size * mixing_ratio) maps its 64 random bits over the offline buffer's size
        into `offline_buffer`, row r >= n_off over the online buffer's size into `online_buffer`.  Both sizes are read
        at the call, so the online buffer may grow between calls without a recapture.  Returns what train_steps
        returns.  A mixed call never continues a previous call's staged rows and leaves none behind: plain train_steps
        calls around it behave as if it had not happened, apart from the trained parameters.  Refusals as
        online_step_mixed, plus injected dropout masks (as train_steps)."""
        if return_stats and not self._step_stats:
            raise ValueError("iqlhip: train_steps_mixed(return_stats=True) needs set_step_stats(True) first")
        n_off, _ = self._mixed_args(offline_buffer, online_buffer, batch_size, mixing_ratio)
        if online_buffer._size < 1:
            raise ValueError("iqlhip: the online replay buffer is empty")
        self._prepare(batch_size)
        self._refuse_injected_masks()
        fn, stream = hb.lib().iqlhip_train_steps_mixed, self._stream()
        off_ptr, on_ptr, ld = offline_buffer._rows.data_ptr(), online_buffer._rows.data_ptr(), offline_buffer._ld
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF

        def call(tab, k, offset, flags):
            return fn(self._ctx, off_ptr, offline_buffer._size, on_ptr, online_buffer._size, ld, batch_size, n_off,
                      tab.ctypes.data, k, seed, offset, stream)
        # (no token: the library drops its continue token too)
        return self._run_burst(n_steps, batch_size, 1.0 / batch_size, chunk, return_losses, return_stats, stream, call)

    # ---- rows drawn by weight on the device (iqlhip_weighted.py) -----------------------------------
    def _weighted_args(self, replay_buffer, batch_size: int, weights=None):
        """The checks both weighted calls make before anything is launched or any counter moves; returns the rows the
        draw covers, the library's table and its (generation, content version) (weights: a SampleWeights used instead of the
        buffer's).  An updatable table spans a capacity: that is the size the library is given."""
        import iqlhip_weighted as wtd
        self._require_gpu()
        if weights is None:
            n = wtd.check_call(replay_buffer)
            table, gen = replay_buffer._weights, (replay_buffer._weights_gen, replay_buffer._weights_version)
        else:
            n = wtd.check_table(replay_buffer, weights)
            table, gen = weights._table, (weights.generation, weights.version)
        if replay_buffer._rows.device != self._dev:
            raise ValueError(f"iqlhip: the replay buffer must live on the trainer's GPU ({self._dev})")
        wtd.check_trainer(self._dp_world, self._dp_exchange, getattr(self, "_precision", "f32"), batch_size,
                          STATS_BF16_MAX_ROWS)
        return n, table, gen

    def _is_beta_arg(self, is_beta) -> float:
        """train_steps_weighted(..., is_beta=...): a finite float >= 0; fp32 only (the row-weighted backward is)."""
        import iqlhip_weighted as wtd
        beta, _ = wtd.check_is_args(1, is_beta, None)
        if getattr(self, "_precision", "f32") == "bf16":
            raise NotImplementedError("iqlhip: is_beta (per-row loss weights) is not supported at bf16 precision: the "
                                      "row-weighted backward is an fp32 kernel")
        return beta

    def prepare_train_steps_weighted(self, replay_buffer, batch_size: int, weights=None, is_beta=None) -> None:
        """prepare_train_steps for the chunk graphs train_steps_weighted replays on this buffer and its current weights
        (weights: a SampleWeights used instead of them).  is_beta not None (any valid value): the graphs of calls with
        is_beta, which are a kind of their own."""
        _, table, _ = self._weighted_args(replay_buffer, batch_size, weights)
        if is_beta is not None:
            self._is_beta_arg(is_beta)
        self._prepare(batch_size)
        self._refuse_injected_masks()
        fn = hb.lib().iqlhip_train_steps_weighted_prepare if is_beta is None else hb.lib().iqlhip_train_steps_weighted_is_prepare
        hb.check(fn(
            self._ctx, replay_buffer._rows.data_ptr(), replay_buffer._ld, batch_size, 1.0 / batch_size, self._stream(),
            table))
        self._ts_token = None

    def train_steps_weighted(self, replay_buffer, n_steps: int, batch_size: int, seed: int = 0,
                             return_losses: bool = True, chunk: int = K_MAX, return_stats: bool = False, weights=None,
                             is_beta=None):
        """train_steps with every row drawn by the buffer's sample weights (ReplayBuffer.set_sample_weights) instead of
        uniformly: advantage-, return- or TD-error-weighted resampling without a host draw per iteration.  The index
        stream is train_steps' own (Philox keyed by (seed, total_it)); only the mapping of its 64 random bits to a row
        differs, so a weighted call moves every counter as a plain call does, and with equal weights it IS the plain
        call, bit for bit.  The idle blocks of each step's forward draw and gather the next step's rows.  Returns what
        train_steps returns.  ValueError if the buffer has no weights or its index bound has changed since they were
        set; NotImplementedError under data parallelism, for bf16 batches of more than 512 rows and with injected
        dropout masks pending.  No priority exponent; without is_beta no importance-sampling correction of the loss.
        is_beta (None: today's call; else a float >= 0, annealed by the caller from call to call): every step's loss
        terms are weighted by c = (q_min / q_row) ** is_beta over that step's batch — bit for bit the eager loop
        draw_weighted_indices(B, ..., is_beta=is_beta) -> gather -> train(batch, loss_weights=c); the returned losses are
        the weighted ones.  Another is_beta on the next call neither re-captures a chunk nor ends a continuation.  fp32
        only (NotImplementedError at bf16 precision).
        weights: None, or an iqlhip_weighted.SampleWeights to draw by instead of the buffer's own table (its n must equal
        the buffer's index bound: ValueError otherwise); a continuation then keys on that object's generation.
        An updatable table (set_sample_weights(..., updatable=True), SampleWeights(..., updatable=True)) is taken like a
        static one and is not refused when the index bound has moved; an update of it between two calls ends the
        continuation (the rows staged for the next step were drawn by the old weights), the chunk graphs stay."""
        if return_stats and not self._step_stats:
            raise ValueError("iqlhip: train_steps_weighted(return_stats=True) needs set_step_stats(True) first")
        size, table, gen = self._weighted_args(replay_buffer, batch_size, weights)
        beta = None if is_beta is None else self._is_beta_arg(is_beta)
        self._prepare(batch_size)
        self._refuse_injected_masks()
        lib, stream = hb.lib(), self._stream()
        rows_ptr, ld = replay_buffer._rows.data_ptr(), replay_buffer._ld
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        buf_ref = weakref.ref(replay_buffer)
        if beta is None:
            fn, kind, tail = lib.iqlhip_train_steps_weighted, "weighted", (stream, table)
        else:
            fn, kind, tail = lib.iqlhip_train_steps_weighted_is, "weighted_is", (stream, table, beta)

        def call(tab, k, offset, flags):
            return fn(self._ctx, rows_ptr, ld, size, batch_size, tab.ctypes.data, k, seed, offset, flags, *tail)

        # (train_steps' token plus the table's generation: a plain call's token never equals it, nor the reverse;
        #  the library checks the generation too;
        #  a call with is_beta continues only such a call — its value is not part of the token)
        def token():
            return (buf_ref, replay_buffer._writes, replay_buffer._rows._version, kind, gen)
        return self._run_burst(n_steps, batch_size, 1.0 / batch_size, chunk, return_losses, return_stats, stream, call,
                               token)

    # ---- prioritised replay inside the chunk graphs (DESIGN.md 6j "Prioritised replay inside the chunk graphs") -------
    def _prioritized_args(self, replay_buffer, batch_size: int, weights, alpha, eps, is_beta):
        """The checks both prioritised calls make before anything is launched or any counter moves: train_steps_weighted's,
        an updatable table, valid alpha / eps / is_beta, fp32.  Returns (rows the table spans, table, alpha, eps, beta)."""
        import iqlhip_weighted as wtd
        size, table, _ = self._weighted_args(replay_buffer, batch_size, weights)
        updatable = replay_buffer._weights_updatable if weights is None else weights.updatable
        if not updatable:
            raise ValueError("iqlhip: prioritised replay needs updatable sample weights "
                             "(set_sample_weights(..., updatable=True) / SampleWeights(..., updatable=True))")
        alpha, eps = wtd.check_priority_args(alpha, eps)
        beta = self._is_beta_arg(is_beta)
        return size, table, alpha, eps, beta

    def prepare_train_steps_prioritized(self, replay_buffer, batch_size: int, weights=None) -> None:
        """prepare_train_steps for the chunk graphs train_steps_prioritized replays on this buffer and its updatable
        weights (weights: a SampleWeights used instead).  Trains nothing and leaves the table as it is: the rehearsal's
        update launches are switched off on the device."""
        _, table, _, _, _ = self._prioritized_args(replay_buffer, batch_size, weights, 1.0, 1.0, 0.0)
        self._prepare(batch_size)
        self._refuse_injected_masks()
        hb.check(hb.lib().iqlhip_train_steps_prioritized_prepare(
            self._ctx, replay_buffer._rows.data_ptr(), replay_buffer._ld, batch_size, 1.0 / batch_size, self._stream(), table))
        self._ts_token = None

    def train_steps_prioritized(self, replay_buffer, n_steps: int, batch_size: int, seed: int = 0, alpha: float = 0.6,
                                eps: float = 1e-3, is_beta: float = 0.0, chunk: int = K_MAX, return_losses: bool = True,
                                return_stats: bool = False, weights=None):
        """Prioritised experience replay without a host round trip: train_steps_weighted(..., is_beta=) whose steps write
        their TD errors back into the (updatable) table as new priorities, (max(|q1 - y|, |q2 - y|) + eps) ** alpha, inside
        the chunk graphs.  Per call: step 0's rows are drawn from the table as it stands; while step t runs, the rows of
        step t + 1 are drawn (they see the updates of steps < t: a lag of one step, which keeps the draw off the critical
        path); then table[rows of t] <- priorities of t.  Bit for bit the eager loop
            idx, c = draw(0);  for t: nxt = draw(t + 1); train(gather(idx), loss_weights=c, return_td=True);
                                      update_sample_weights_td(idx, last_td_errors(), alpha, eps); idx, c = nxt
        whatever `chunk` is.  A call never starts on rows an earlier call staged: its step 0 is always a fresh draw, so
        the result depends on how steps are cut into calls (3 + 2 steps differ from 5) but not on history; inside a call,
        pieces of `chunk` steps go on with the lag-1 chain (chunk is rounded down to an even number, at least 2: a piece
        must end on the staging half the next one starts on; with an odd batch_size the index stream skips half a counter
        between library calls, as in train_steps, so every piece then starts with a fresh draw).  alpha, eps and is_beta are per call and re-capture
        nothing.  The table's version moves with every library call: a train_steps_weighted call that follows gathers
        afresh.  Returns what train_steps returns.  ValueError for a static table, for alpha, eps or is_beta negative or
        not finite, for alpha = eps = 0; NotImplementedError at bf16 precision, under data parallelism and with injected
        dropout masks pending — all before anything moves.  Not covered: mixed batches, annealing inside a call.
        (The online iteration: online_step_prioritized; rows added between calls enter at the table's largest priority
        when it tracks it — set_sample_weights(..., track_max=True) — else follow add_transition with
        update_sample_weights.)"""
        if return_stats and not self._step_stats:
            raise ValueError("iqlhip: train_steps_prioritized(return_stats=True) needs set_step_stats(True) first")
        size, table, alpha, eps, beta = self._prioritized_args(replay_buffer, batch_size, weights, alpha, eps, is_beta)
        self._prepare(batch_size)
        self._refuse_injected_masks()
        fn, stream = hb.lib().iqlhip_train_steps_prioritized, self._stream()
        rows_ptr, ld = replay_buffer._rows.data_ptr(), replay_buffer._ld
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF

        def call(tab, k, offset, flags):
            rc = fn(self._ctx, rows_ptr, ld, size, batch_size, tab.ctypes.data, k, seed, offset, flags, stream, table, beta,
                    alpha, eps)
            if rc == 0:                    # (the library moved the table's content version: the Python mirror follows)
                if weights is None:
                    replay_buffer._weights_version += 1
                else:
                    weights._version += 1
            return rc

        # the token names THIS Python call: no earlier call's token ever equals it, so the first piece draws afresh and
        # only the pieces of this call continue each other
        self._prio_calls = getattr(self, "_prio_calls", 0) + 1
        tok = ("prioritized", self._prio_calls)
        chunk = max(2, min(int(chunk), K_MAX) & ~1)
        return self._run_burst(n_steps, batch_size, 1.0 / batch_size, chunk, return_losses, return_stats, stream, call,
                               lambda: tok)

    def _schedule_state(self):
        sch = self.actor_lr_schedule
        lr = float(self.actor_optimizer.param_groups[0]["lr"])
        if sch is None:
            return (lr, None, None)
        return (lr, sch.last_epoch, sch._step_count)

    def _peek_schedule(self, k: int):
        """(actor learning rates USED by the next k steps, scheduler state after them) without touching the
        CosineAnnealingLR object.  Same float64 recursion as torch's CosineAnnealingLR.get_lr (eta_min = 0), run as a
        plain loop instead of k scheduler.step() calls (~15 us each).  None when the scheduler is in a state only
        torch should advance."""
        lr = float(self.actor_optimizer.param_groups[0]["lr"])
        out = np.empty(k, dtype=np.float64)
        sch = self.actor_lr_schedule
        if sch is None:
            out[:] = lr
            return out, (lr, None, None)
        import math
        T = sch.T_max
        base = float(sch.base_lrs[0])
        eta_min = float(sch.eta_min)
        if eta_min != 0.0 or len(sch.base_lrs) != 1 or (sch._step_count == 1 and sch.last_epoch > 0):
            return None
        e = sch.last_epoch
        cos, pi = math.cos, math.pi
        for i in range(k):
            out[i] = lr
            e += 1
            if (e - 1 - T) % (2 * T) == 0:
                lr = lr + base * (1 - cos(pi / T)) / 2
            else:
                lr = (1 + cos(pi * e / T)) / (1 + cos(pi * (e - 1) / T)) * lr
        return out, (lr, e, sch._step_count + k)

    def _commit_schedule(self, state) -> None:
        lr, e, count = state
        sch = self.actor_lr_schedule
        if sch is None:
            return
        sch.last_epoch = e
        sch._step_count = count
        self.actor_optimizer.param_groups[0]["lr"] = lr
        sch._last_lr = [lr]
        self.actor_optimizer._opt_called = True

    def _advance_schedule(self, k: int) -> np.ndarray:
        """Actor learning rates USED by the next k steps; advances the CosineAnnealingLR object by k steps."""
        pk = self._peek_schedule(k)
        if pk is None:
            out = np.empty(k, dtype=np.float64)
            for i in range(k):     # unusual scheduler state: let torch do it
                out[i] = float(self.actor_optimizer.param_groups[0]["lr"])
                self._step_schedule()
            return out
        out, state = pk
        self._commit_schedule(state)
        return out

    def _build_table(self, k: int, inv_batch: float, adam_t: Dict[str, int], lr_pi: np.ndarray) -> np.ndarray:
        """[k,12] float32 rows laid out like iqlhip_step_scalars for k steps after Adam step counts `adam_t`."""
        b1, b2, eps = self._adam_hyper()
        lrs = self._current_lrs()
        tab = np.empty((k, 12), dtype=np.float32)
        steps = np.arange(1, k + 1, dtype=np.float64)
        for i, g in enumerate(("v", "q", "pi")):
            t = adam_t[g] + steps
            lr = lr_pi if g == "pi" else lrs[g]
            tab[:, i] = lr / (1.0 - np.power(b1, t))
            tab[:, 3 + i] = np.sqrt(1.0 - np.power(b2, t))
        tab[:, 6] = b2
        tab[:, 7] = 1.0 - b1
        tab[:, 8] = 1.0 - b2
        tab[:, 9] = eps
        tab[:, 10] = 1.0
        tab[:, 11] = inv_batch
        return tab

    def _table_key(self, inv_batch: float):
        """Everything a precomputed scalar table depends on (plain attribute reads: this runs on the critical path of
        every train_steps call, in front of the first launch)."""
        t = self._adam_t
        gv, gq, gp = (self.v_optimizer.param_groups[0], self.q_optimizer.param_groups[0],
                      self.actor_optimizer.param_groups[0])
        sch = self.actor_lr_schedule
        return (inv_batch, t["v"], t["q"], t["pi"], gv["lr"], gq["lr"], gp["lr"],
                None if sch is None else (sch.last_epoch, sch._step_count, sch.T_max),
                gv["betas"], gv["eps"], gq["betas"], gq["eps"], gp["betas"], gp["eps"])

    def _scalar_table(self, k: int, inv_batch: float) -> np.ndarray:
        """The per-step scalars of the next k steps (float64 Adam bias corrections and cosine learning rates, cast to
        float32 once per step like torch does); advances the Adam step counts and the scheduler.  A table computed
        ahead of time by _lookahead_table (while the GPU was busy with the previous chunk) is used when the state it
        was computed for is still the current one."""
        key = self._table_key(inv_batch)
        cached = self._table_cache
        self._table_cache = None
        if cached is not None and cached[0] == key and cached[1].shape[0] >= k:
            # rows depend on the absolute step only: the first k rows of a longer look-ahead are this call's table
            # (passed as it is: the library copies the first k rows before it returns)
            _, tab, lr_after, (e0, c0) = cached
            self._commit_schedule((float(lr_after[k - 1]), None if e0 is None else e0 + k, None if c0 is None else c0 + k))
        else:
            lr_pi = self._advance_schedule(k)
            tab = self._build_table(k, inv_batch, self._adam_t, lr_pi)
        for g in self._adam_t:
            self._adam_t[g] += k
        return tab

    def _lookahead_table(self, k: int, inv_batch: float) -> None:
        """Precompute the table of the steps AFTER the ones just launched (host work overlapped with the GPU): at least
        64 rows, so that a following call of any length up to that finds its rows ready."""
        k = max(int(k), 64)
        pk = self._peek_schedule(k + 1)
        if pk is None:
            return
        lr_used, _ = pk                     # lr_used[i] = learning rate step i uses = the rate AFTER i steps
        sch = self.actor_lr_schedule
        state0 = (None, None) if sch is None else (sch.last_epoch, sch._step_count)
        tab = self._build_table(k, inv_batch, self._adam_t, lr_used[:k])       # (_adam_hyper inside: raises on optimizer
        self._table_cache = (self._table_key(inv_batch), tab, lr_used[1:], state0)  #  settings the kernels do not implement)

    def _train_steps_args(self, replay_buffer, batch_size: int):
        self._prepare(batch_size)
        if self._dp_world > 1 and self._dp_exchange == "torch":
            raise NotImplementedError("train_steps needs an in-library exchange: enable_data_parallel(exchange='rccl'|'p2p')")
        if not getattr(replay_buffer, "_gpu", False):
            raise ValueError("train_steps needs a ReplayBuffer that lives on the GPU")
        size = replay_buffer._index_bound()
        if size < 1:
            raise ValueError("replay buffer is empty")
        return size, dp.inv_batch(batch_size, self._dp_world)

    def _refuse_injected_masks(self) -> None:
        """train_steps draws its own keep-bits (two halves, the next step's drawn by the step before) and cannot use
        masks written by inject_dropout_masks.  The library refuses too (IQLHIP_EUNSUPPORTED); raised here, before the
        scalar table moves the Adam step counts and the actor's schedule."""
        if getattr(self, "_masks_injected", False):
            raise NotImplementedError("iqlhip: train_steps draws its own keep-bits and cannot use the masks written by "
                                      "inject_dropout_masks; step with train(), or clear them (set_dropout_seed)")

    def _read_rings(self, k: int, stream, losses, stats) -> None:
        """The last k steps' losses [k, 3] and statistics [k, 16] from the library's rings into the given arrays (None: not
        wanted) — what train_steps and train_steps_mixed do after each library call."""
        lib = hb.lib()
        if losses is not None:
            buf = (C.c_float * (3 * k))()
            hb.check(lib.iqlhip_read_loss_ring(self._ctx, buf, k, stream))
            losses[:] = np.frombuffer(buf, dtype=np.float32).reshape(k, 3)
        if stats is not None:
            sbuf = (C.c_float * (hb.IQLHIP_N_STATS * k))()
            hb.check(lib.iqlhip_read_stats_ring(self._ctx, sbuf, k, stream))
            stats[:] = np.frombuffer(sbuf, dtype=np.float32).reshape(k, hb.IQLHIP_N_STATS)

    def _run_burst(self, n_steps: int, batch_size: int, inv_batch: float, chunk: int, return_losses: bool,
                   return_stats: bool, stream, call, token=None):
        """The multi-step loop behind train_steps, train_steps_mixed and train_steps_weighted, whose checks have all
        passed: n_steps in library calls of at most `chunk` steps.  call(tab, k, offset, flags) makes the kind's one
        library call for the next k steps — tab their scalar table, offset their place in the Philox stream — and
        returns its code.  token: None for a kind that never continues staged rows (the trainer's token is dropped and
        TS_CONTINUE never passed), or a callable giving the continuation token of the chunk about to run (evaluated per
        chunk: it reads the buffer's write counts); the call gets TS_CONTINUE iff that equals the token the previous
        successful call left.  A failed call leaves no token.  Returns losses [n_steps, 3] (None unless return_losses),
        or (losses, stats) when return_stats."""
        stats = np.empty((n_steps, hb.IQLHIP_N_STATS), dtype=np.float32) if return_stats else None
        losses = np.empty((n_steps, 3), dtype=np.float32) if return_losses else None
        chunk = max(1, min(int(chunk), K_MAX))
        half = (batch_size + 1) // 2
        if token is None:
            self._ts_token = None
        done, tok, flags = 0, None, 0
        while done < n_steps:
            k = min(chunk, n_steps - done)
            tab = self._scalar_table(k, inv_batch)
            if token is not None:
                tok = token()
                flags = hb.TS_CONTINUE if self._ts_token == tok else 0
            rc = call(tab, k, self.total_it * half, flags)
            if rc:
                self._ts_token = None
                hb.check(rc)
            self._ts_token = tok
            self.total_it += k
            done += k
            # the GPU is busy with these k steps: compute the scalars of the next k now
            self._lookahead_table(min(chunk, n_steps - done) if done < n_steps else k, inv_batch)
            self._read_rings(k, stream, None if losses is None else losses[done - k: done],
                             None if stats is None else stats[done - k: done])
        return (losses, stats) if return_stats else losses

    def prepare_train_steps(self, replay_buffer, batch_size: int) -> None:
        """Capture and upload the hipGraph chunk train_steps replays for this buffer / batch size now, so that no later
        train_steps call pays for it (it is captured lazily otherwise, by the first call of >= 64 steps)."""
        _, inv_batch = self._train_steps_args(replay_buffer, batch_size)
        self._refuse_injected_masks()
        hb.check(hb.lib().iqlhip_train_steps_prepare(self._ctx, replay_buffer._rows.data_ptr(), replay_buffer._ld,
                                                      batch_size, inv_batch, self._stream()))
        self._ts_token = None

    def train_steps(self, replay_buffer, n_steps: int, batch_size: int, seed: int = 0,
                    return_losses: bool = True, chunk: int = K_MAX, return_stats: bool = False):
        """n_steps consecutive `sample -> train` iterations without host round trips
        (the offline loop body, algorithms/offline/iql.py:631-635): indices are drawn on
        the device (uniform with replacement, Philox keyed by (seed, total_it)); the library
        launches the call's first 2 or 4 steps directly and replays fixed chunk graphs of 64 /
        16 / 4 / 2 / 1 steps for the rest (nothing is captured per value of n_steps); per-step
        Adam / cosine-LR scalars are precomputed on the host (the next call's while the GPU
        runs this one's).  Under data parallelism every rank draws its own rows (rank-offset
        stream) and the gradient exchange runs inside the same stream / graph.  Returns losses
        [n_steps,3] (value, q, actor) when return_losses, else None (fully asynchronous).
        return_stats (needs set_step_stats(True), else ValueError): returns (losses, stats) instead, stats the
        [n_steps, 16] per-step statistics in hb.STAT_NAMES order."""
        if return_stats and not self._step_stats:
            raise ValueError("iqlhip: train_steps(return_stats=True) needs set_step_stats(True) first")
        size, inv_batch = self._train_steps_args(replay_buffer, batch_size)
        self._refuse_injected_masks()
        fn = hb.lib().iqlhip_train_steps
        rank = self._dp_rank if self._dp_world > 1 else 0
        seed = dp.rank_seed(seed, rank)
        rows_ptr, ld, stream = replay_buffer._rows.data_ptr(), replay_buffer._ld, self._stream()
        buf_ref = weakref.ref(replay_buffer)

        def call(tab, k, offset, flags):
            return fn(self._ctx, rows_ptr, ld, size, batch_size, tab.ctypes.data, k, seed, offset, flags, stream)

        # IQLHIP_TS_CONTINUE: nothing has written this buffer's rows since our previous call on it (the buffer
        # counts its writes); the library itself checks that this call starts where that one's index stream ended
        # (a weak reference: the token must not keep a multi-GB buffer alive; the tensor's version counter sees in-place
        #  writes through the reference-named views _states / _rewards / ..., which alias the packed rows)
        def token():
            return (buf_ref, replay_buffer._writes, replay_buffer._rows._version)
        return self._run_burst(n_steps, batch_size, inv_batch, chunk, return_losses, return_stats, stream, call, token)

    def train_steps_dp(self, replay_buffer, n_steps: int, batch_size: int, seed: int = 0) -> None:
        """Data-parallel multi-step run without host syncs (= train_steps(..., return_losses=False))."""
        self.train_steps(replay_buffer, n_steps, batch_size, seed=seed, return_losses=False)

    def train_on_buffer(self, replay_buffer, batch_size: int, seed: int = 0, sync: bool = False):
        """One step on rows drawn ON THE DEVICE from `replay_buffer` (no host index draw, no
        host sync unless `sync`).  Data-parallel aware: each rank draws its own rows (seed is
        offset by the rank), gradients are all-reduced before the update."""
        self._prepare(batch_size)
        size = replay_buffer._index_bound()
        lib = hb.lib()
        idx = getattr(self, "_idx_buf", None)
        if idx is None or idx.numel() != batch_size:
            idx = torch.empty(batch_size, dtype=torch.int64, device=self._dev)
            self._idx_buf = idx
        rank = self._dp_rank if self._dp_world > 1 else 0
        hb.check(lib.iqlhip_draw_indices(idx.data_ptr(), batch_size, size, dp.rank_seed(seed, rank),
                                         int(self.total_it) * ((batch_size + 1) // 2), self._stream()))
        S, A = self._S, self._A
        base = replay_buffer._rows.data_ptr()
        ld = replay_buffer._ld
        b = hb.Batch(base, base + 4 * S, base + 4 * (2 * S + A), base + 4 * (S + A), base + 4 * (2 * S + A + 1),
                     ld, ld, ld, ld, ld, idx.data_ptr(), batch_size)
        return self._run_step(b, batch_size, sync)

    # ------------------------------------------------------------------ data parallel
    def enable_data_parallel(self, process_group=None, exchange: str = "rccl", timeout_ms: int = 5000) -> None:
        """One process per GPU: parameters replicated (rank 0's are broadcast once), each rank trains
        on its own rows, the flat gradient (+3 loss words) is summed over the ranks between the backward and the
        fused Adam/Polyak launch.  `exchange`:
          "rccl"  ncclAllReduce issued by the library in-stream (and inside the captured chunk graphs);
          "p2p"   the ranks' gradient buffers are mapped into each other (hipIpc) and the update kernel reads them
                  directly over xGMI after a flag handshake — no collective call per step (one node, <= 8 ranks);
          "both"  attach both (select with select_exchange(); "p2p" is selected);
          "torch" torch.distributed.all_reduce between two library calls per step (any backend; eager train() only).
        Call after torch.distributed is up; batch sizes must not grow afterwards (reserve_batch first)."""
        import torch.distributed as dist
        self._require_gpu()
        if exchange not in ("rccl", "p2p", "both", "torch"):
            raise ValueError("exchange must be 'rccl', 'p2p', 'both' or 'torch'")
        self._dp_group = process_group
        self._dp_world = dist.get_world_size(process_group)
        self._dp_rank = dist.get_rank(process_group)
        world, rank = self._dp_world, self._dp_rank
        if world > 1 and not (exchange == "p2p" and dist.get_backend(process_group) == "gloo"):
            dp.broadcast_state((self._params_arena, self._target_arena, self._m_arena, self._v_arena), process_group,
                               src=dist.get_global_rank(process_group, 0) if process_group else 0)
        elif world > 1:
            dp.broadcast_state_host((self._params_arena, self._target_arena, self._m_arena, self._v_arena), process_group)
        lib = hb.lib()
        if exchange == "torch":
            self._dp_exchange = "torch"
            return
        src = dist.get_global_rank(process_group, 0) if process_group else 0
        if exchange in ("rccl", "both"):
            # collective-safe like the peer mapping below: a failure on any rank (no librccl, communicator init) is
            # agreed on by all ranks before anyone relies on the collective
            err = None
            uid = (C.c_char * hb.IQLHIP_UNIQUE_ID_BYTES)()
            if rank == 0:
                try:
                    hb.check(lib.iqlhip_comm_unique_id(uid))
                except Exception as e:      # noqa: BLE001 - reported after the collective
                    err = e
            box = [None if err is not None else bytes(uid.raw)]
            dist.broadcast_object_list(box, src=src, group=process_group)
            if box[0] is None:
                err = err or RuntimeError("rank 0 could not create a communicator id")
            else:
                ubuf = C.create_string_buffer(box[0], hb.IQLHIP_UNIQUE_ID_BYTES)
                try:
                    hb.check(lib.iqlhip_allreduce_init(self._ctx, ubuf, rank, world))
                except Exception as e:      # noqa: BLE001
                    err = e
            oks = [None] * world
            dist.all_gather_object(oks, err is None, group=process_group)
            if all(oks):
                self._dp_exchange = "rccl"
            else:
                self._rccl_error = f"RCCL exchange unavailable on ranks {[i for i, o in enumerate(oks) if not o]}: {err}"
                if exchange == "rccl":
                    raise RuntimeError("iqlhip: " + self._rccl_error)
        if exchange in ("p2p", "both"):
            if world > hb.IQLHIP_MAX_WORLD:
                raise ValueError(f"the p2p exchange serves one node (<= {hb.IQLHIP_MAX_WORLD} ranks), got {world}")
            # collective-safe: every rank exports, gathers and TRIES to map its peers; the outcome is agreed on before
            # anyone relies on it, so a rank whose mapping failed (no peer access between two GPUs) cannot leave the
            # others waiting for its flags
            err = None
            h = (C.c_char * hb.IQLHIP_IPC_HANDLE_BYTES)()
            try:
                hb.check(lib.iqlhip_p2p_export(self._ctx, h, rank, world))
            except Exception as e:          # noqa: BLE001 - reported below, after the collective
                err = e
            handles = [None] * world
            dist.all_gather_object(handles, None if err is not None else bytes(h.raw), group=process_group)
            if err is None and all(x is not None for x in handles):
                blob = C.create_string_buffer(b"".join(handles), world * hb.IQLHIP_IPC_HANDLE_BYTES)
                try:
                    hb.check(lib.iqlhip_p2p_attach(self._ctx, blob, int(timeout_ms)))
                except Exception as e:      # noqa: BLE001
                    err = e
            oks = [None] * world
            dist.all_gather_object(oks, err is None, group=process_group)   # (doubles as the barrier: all blocks mapped)
            if all(oks):
                self._dp_exchange = "p2p"
            else:
                self._p2p_error = f"p2p exchange unavailable on ranks {[i for i, o in enumerate(oks) if not o]}: {err}"
                if self._dp_exchange == "rccl":          # "both": keep the collective library's exchange
                    hb.check(lib.iqlhip_xch_select(self._ctx, hb.XCH_RCCL))
                elif exchange == "p2p":
                    raise RuntimeError("iqlhip: " + self._p2p_error)
        if exchange == "both" and self._dp_exchange not in ("rccl", "p2p"):
            # neither in-library exchange came up: the eager torch.distributed exchange still trains correctly
            # (train() / train_on_buffer(); train_steps needs an in-library exchange)
            self._dp_exchange = "torch"

    def resync_replicas(self) -> None:
        """Collective: make rank 0's state the common one again — the four arenas, the step counters and the actor's
        schedule — and forget a recorded exchange timeout.  For a caller that found the replicas diverged (a probe of
        an exchange that does not work on this machine) and is about to continue on another exchange."""
        import torch.distributed as dist
        self._require_gpu()
        torch.cuda.synchronize(self._dev)
        g = self._dp_group
        src = dist.get_global_rank(g, 0) if g else 0
        if dist.get_backend(g) == "gloo":
            dp.broadcast_state_host((self._params_arena, self._target_arena, self._m_arena, self._v_arena), g, src)
        else:
            dp.broadcast_state((self._params_arena, self._target_arena, self._m_arena, self._v_arena), g, src)
        box = [(self.total_it, dict(self._adam_t), self._schedule_state())] if self._dp_rank == 0 else [None]
        dist.broadcast_object_list(box, src=src, group=g)
        total_it, adam_t, (lr, e, count) = box[0]
        self.total_it, self._adam_t = int(total_it), dict(adam_t)
        if self.actor_lr_schedule is not None:
            self._commit_schedule((lr, e, count))
        else:
            self.actor_optimizer.param_groups[0]["lr"] = lr
        self._table_cache = None
        self._ts_token = None
        hb.check(hb.lib().iqlhip_xch_clear_status(self._ctx, self._stream()))

    def select_exchange(self, exchange: str) -> None:
        """Switch between attached in-library exchanges ("rccl" / "p2p"); collective: every rank must do the same."""
        if exchange == "torch":           # the eager fallback: local steps in the library, torch.distributed in between
            hb.check(hb.lib().iqlhip_xch_select(self._ctx, hb.XCH_NONE))
            self._dp_exchange = "torch"
            return
        mode = {"rccl": hb.XCH_RCCL, "p2p": hb.XCH_P2P}[exchange]
        hb.check(hb.lib().iqlhip_xch_select(self._ctx, mode))
        self._dp_exchange = exchange

    def exchange_status(self) -> Dict[str, int]:
        """{"mode", "timed_out_step" (0 = no P2P wait ever timed out), "steps"}; synchronises the stream."""
        st = (C.c_int64 * 3)()
        hb.check(hb.lib().iqlhip_xch_status(self._ctx, st, self._stream()))
        return {"mode": int(st[0]), "timed_out_step": int(st[1]), "steps": int(st[2])}

    def _dp_flat(self) -> torch.Tensor:
        n = int(hb.lib().iqlhip_grad_words(self._ctx))
        f = getattr(self, "_dp_flat_buf", None)
        if f is None or f.numel() != n:
            f = torch.zeros(n, dtype=torch.float32, device=self._dev)
            self._dp_flat_buf = f
        return f

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self) -> Dict[str, Any]:
        self._sync_opt_state()
        if self.actor_lr_schedule is None:
            lr_state_dict = {}
        else:
            lr_state_dict = self.actor_lr_schedule.state_dict()
        return {
            "qf": self.qf.state_dict(),
            "q_optimizer": self.q_optimizer.state_dict(),
            "vf": self.vf.state_dict(),
            "v_optimizer": self.v_optimizer.state_dict(),
            "actor": self.actor.state_dict(),
            "actor_optimizer": self.actor_optimizer.state_dict(),
            "actor_lr_schedule": lr_state_dict,
            "total_it": self.total_it,
        }

    def _reset_target_from_qf(self) -> None:
        # reference: q_target = copy.deepcopy(qf) WITHOUT requires_grad_(False) (iql.py:584, Appendix A quirk)
        if self._ctx is None:
            self.q_target = copy.deepcopy(self.qf)
            return
        L = self._layout
        with torch.no_grad():
            self._target_arena.copy_(self._params_arena[L.target_src: L.target_src + L.n_target])
        new_t = copy.deepcopy(self.qf)   # fresh module object, like the reference
        self.q_target = new_t
        self._rehome(self._target_tensors(), self._target_arena, "target")

    def load_state_dict(self, state_dict: Dict[str, Any]):
        self.qf.load_state_dict(state_dict["qf"])
        self.q_optimizer.load_state_dict(state_dict["q_optimizer"])
        self._reset_target_from_qf()

        self.vf.load_state_dict(state_dict["vf"])
        self.v_optimizer.load_state_dict(state_dict["v_optimizer"])
        self.actor.load_state_dict(state_dict["actor"])
        self.actor_optimizer.load_state_dict(state_dict["actor_optimizer"])
        if self.actor_lr_schedule is not None:
            self.actor_lr_schedule.load_state_dict(state_dict["actor_lr_schedule"])

        self.total_it = state_dict["total_it"]
        if self._ctx is not None:
            self._absorb_opt_state()

    def partial_load_state_dict(self, state_dict: Dict[str, Any]):
        """Load state dict, but don't load optimisers (iql.py:595-606)."""
        self.qf.load_state_dict(state_dict["qf"])
        self._reset_target_from_qf()

        self.vf.load_state_dict(state_dict["vf"])

        self.actor.load_state_dict(state_dict["actor"])
        if self.actor_lr_schedule is not None:
            self.actor_lr_schedule.load_state_dict(state_dict["actor_lr_schedule"])

        self.total_it = state_dict["total_it"]

    # ------------------------------------------------------------------ introspection for tests / bench
    # ------------------------------------------------------------------ policy inference
    def can_act_on(self, device) -> bool:
        """True if the library context can serve actor.act(state, device) (same GPU as the arenas)."""
        if self._ctx is None or not _is_gpu(device):
            return False
        d = torch.device(device)
        return d.index is None or d.index == self._dev.index

    def actor_forward(self, states: torch.Tensor, sample: bool = False, max_action: Optional[float] = None) -> torch.Tensor:
        """Batched policy forward on the device: [n, S] float32 -> actions [n, A]
        = clamp(max_action * (tanh(MLP(s)) [+ sigma * N(0,1) if `sample` and the policy is Gaussian]), +-max_action).
        The batched form of GaussianPolicy.act / DeterministicPolicy.act (iql.py:371-379, 404-413) for evaluation
        loops.  Eval-mode forward (no dropout) unless set_act_dropout(True) was called and the actor is in training
        mode: then every library call (a chunk of at most the row cap) draws its rows' keep-bits."""
        self._require_gpu()
        self._prepare_act()
        x = self._as_dev(states).reshape(-1, self._S)
        n = x.shape[0]
        ma = float(self.max_action if max_action is None else max_action)
        out = torch.empty((n, self._A), dtype=torch.float32, device=self._dev)
        draw = sample and self._gaussian          # dist.sample(): noise drawn on the device, seeded from torch's seed
        st = self._stream()
        cap = max(self._max_batch, hb.IQLHIP_ACT_ROWS)
        for r0 in range(0, n, cap):
            r1 = min(n, r0 + cap)
            if draw:
                hb.check(hb.lib().iqlhip_actor_sample(self._ctx, x[r0:r1].data_ptr(), x.stride(0), r1 - r0,
                                                      self._act_seed(), ma, out[r0:r1].data_ptr(), out.stride(0), st))
            else:
                hb.check(hb.lib().iqlhip_actor_forward(self._ctx, x[r0:r1].data_ptr(), x.stride(0), r1 - r0, None,
                                                       self._A, ma, out[r0:r1].data_ptr(), out.stride(0), st))
        return out

    def _act_seed(self) -> int:
        """Non-zero 64-bit key of the device noise stream of act(): torch's seed at first use (so that
        torch.manual_seed(s) before training gives a reproducible exploration stream)."""
        k = getattr(self, "_act_key", None)
        if k is None:
            k = (int(torch.initial_seed()) * 0x9E3779B97F4A7C15 + 0xAC7) & 0xFFFFFFFFFFFFFFFF
            self._act_key = k = (k or 1)
        return k

    def act_one(self, state: np.ndarray, max_action: float, sample: bool) -> np.ndarray:
        """actor.act(state): one state in, one action out.  The state is written into a pinned host buffer that the
        pack kernel reads directly and the action lands in a pinned host buffer the finish kernel writes directly
        (host-mapped memory over PCIe: ~120 B each way), so the call is three launches and one stream
        synchronisation — no staging copies, no per-call allocation."""
        self._require_gpu()
        self._prepare_act()
        if self._act_bufs is None:
            h_in = torch.empty((1, self._S), dtype=torch.float32).pin_memory()
            h_out = torch.empty((1, self._A), dtype=torch.float32).pin_memory()
            self._act_bufs = (h_in, h_out, h_in.numpy(), h_out.numpy())
        h_in, h_out, in_np, out_np = self._act_bufs
        in_np[0, :] = np.asarray(state, dtype=np.float32).reshape(-1)
        st = self._stream()
        if sample and self._gaussian:
            hb.check(hb.lib().iqlhip_actor_sample(self._ctx, h_in.data_ptr(), self._S, 1, self._act_seed(),
                                                  float(max_action), h_out.data_ptr(), self._A, st))
        else:
            hb.check(hb.lib().iqlhip_actor_forward(self._ctx, h_in.data_ptr(), self._S, 1, None, self._A,
                                                   float(max_action), h_out.data_ptr(), self._A, st))
        hb.check(hb.lib().iqlhip_stream_synchronize(st))
        return out_np[0].copy()

    def set_timing(self, enabled: bool) -> None:
        self._require_gpu()
        hb.check(hb.lib().iqlhip_set_timing(self._ctx, 1 if enabled else 0))

    def get_timing_us(self):
        out = (C.c_float * 4)()
        hb.check(hb.lib().iqlhip_get_timing(self._ctx, out))
        return [float(x) for x in out]

    def time_kernel(self, batch: TensorBatch, which: int, repeat: int = 200) -> float:
        """Average microseconds per launch of one kernel of the step, launched back to back."""
        b, keep, B = self._batch_struct(batch)
        self._prepare(B)
        out = C.c_float(0)
        hb.check(hb.lib().iqlhip_debug_time_kernel(self._ctx, C.byref(b), which, repeat, C.byref(out), self._stream()))
        return float(out.value)

    def set_precision(self, mode: str) -> None:
        """"f32" (default, the parity path) or "bf16": bf16 operands / fp32 accumulate for the layer
        and weight-gradient products (BASELINE config 5's MFMA bf16 path; heads, losses, Adam stay fp32).  Not part of the reference's surface."""
        self._require_gpu()
        if mode not in ("f32", "bf16"):
            raise ValueError("precision must be 'f32' or 'bf16'")
        self._precision = mode
        hb.check(hb.lib().iqlhip_set_precision(self._ctx, 1 if mode == "bf16" else 0))

    def inject_dropout_masks(self, keep0: np.ndarray, keep1: np.ndarray) -> None:
        """Tests: use these keep-masks (bool [rows,256] per layer) for the following steps instead of device draws."""
        from synth import pack_keep_bits
        self._prepare(keep0.shape[0])
        b0 = np.ascontiguousarray(pack_keep_bits(keep0))
        b1 = np.ascontiguousarray(pack_keep_bits(keep1))
        hb.check(hb.lib().iqlhip_debug_write_masks(self._ctx, b0.ctypes.data, b1.ctypes.data, keep0.shape[0],
                                                   self._stream()))
        self._masks_injected = True

    def debug_read(self, name: str) -> np.ndarray:
        self._require_gpu()
        cap = max(4 * self._max_batch * 256, 16 * max(self._max_batch, hb.IQLHIP_ACT_ROWS)) + 64
        buf = (C.c_float * cap)()
        n = C.c_int64(0)
        hb.check(hb.lib().iqlhip_debug_read(self._ctx, name.encode(), buf, cap, C.byref(n), self._stream()))
        return np.frombuffer(buf, dtype=np.float32)[: n.value].copy()

    def flat_gradient(self, batch: TensorBatch, loss_weights=None) -> np.ndarray:
        """Forward+backward only; returns the flat gradient (+4 tail words) as numpy (tests).  loss_weights: train()'s."""
        b, keep, B = self._batch_struct(batch)
        self._prepare(B)
        sc = hb.StepScalars()
        t1 = {g: max(1, v) for g, v in self._adam_t.items()}
        self._fill_scalars(sc, t1, self._current_lrs(), dp.inv_batch(B, self._dp_world))
        flat = self._dp_flat()
        if loss_weights is not None:
            w, _ = self._loss_weight_args(B, loss_weights, False)
            hb.check(hb.lib().iqlhip_forward_backward_rw(self._ctx, C.byref(b), C.byref(sc), w.data_ptr(), None, flat.data_ptr(),
                                                         self._stream()))
            torch.cuda.synchronize(self._dev)
            return flat.cpu().numpy()
        hb.check(hb.lib().iqlhip_forward_backward(self._ctx, C.byref(b), C.byref(sc), flat.data_ptr(), self._stream()))
        torch.cuda.synchronize(self._dev)
        return flat.cpu().numpy()
