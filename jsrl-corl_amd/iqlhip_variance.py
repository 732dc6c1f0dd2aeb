"""The JSRL variance learner on the device (include/iqlhip.h "the JSRL variance learner"): the reference's
variance_learner.py VarianceLearner — the two scalar networks behind the `variance` horizon — with `_update_v` as one
packed upload, one library step (forward, recurrence, backward, Adam: four launches) and one synchronisation.

The step is the reference's as written, quirks included: sampled values use rewards[t - 1] (row 0 takes rewards[B - 1];
`aligned_rewards=True` is this project's opt-in for rewards[t]), the bootstrap value keeps its gradient, `actions` and
`dones` are unused, of `next_observations` only the last row is.  Not ported: StateActionVarianceLearner (its get_values
cannot run in the reference) and test_model (mismatched signatures, plotting).  There is no CPU fall-back: a learner on a
CPU device holds its networks and optimizers, and raises when asked to step.

Beyond the reference: B consecutive rows of a GPU ReplayBuffer are a rollout (a dataset is stored in trajectory order,
an online ring fills in time order), so pack_window / update_from_buffer / get_values_window build the packed block with
one launch instead of the host, and train_on_buffer / run_training_on_buffer queue whole bursts of updates whose
windows are drawn on the device (DESIGN.md 6l "From a replay buffer"); VarianceLearnerGroup does every one of these calls
for up to 16 learners with one set of launches, each member's result its solo call's bit for bit (DESIGN.md 6l "Groups of
learners")."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from torch import nn

import iqlhip_binding as hb
from iqlhip_networks import MLP, linear_layers

GAMMA = 0.99
VAR_MAX_ROWS = 1024           # rows of one step (csrc/iqlhip_variance_kernels.h)
TRAIN_MAX_STEPS = hb.IQLHIP_VAR_TRAIN_MAX_STEPS      # updates per library call of train_on_buffer (the rings' length)
NET_MF, NET_VF = 0, 1
SAVE_DIR = "jsrl-CORL/algorithms/finetune/var_functions"      # the reference's save path
_KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")


def to_tensor(data) -> torch.Tensor:
    return torch.tensor(data, dtype=torch.float32)


def nll_loss(pred: torch.Tensor, target: torch.Tensor, var: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.gaussian_nll_loss(pred, target, var)


def mse_loss(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return 0.5 * ((pred - target) ** 2).mean()


@torch.no_grad()
def run_episodes(env, max_steps: int, seeds, actor=None, batch_size=None, random_frac=0):
    """Roll `env` out (variance_learner.py:16-78): returns (states, actions, rewards, dones, next_states, next_dones),
    lists with one entry per environment step; states and next_states hold float32 tensors.  seeds: an int (the first
    episode is seeded with it, later ones continue unseeded, the rollout ends at `batch_size` rows) or a list (every
    episode ep is seeded, while ep < len(seeds), starting at ep = seeds[0], as the reference writes it).  An actor
    consumes one np.random.random() per step — none without one; `actor(env, state)` or `actor.act(state, device)`.
    next_dones is the env's done unless the episode ran into max_steps (a time-out is not a terminal)."""
    states, next_states, next_dones, actions, rewards, dones = [], [], [], [], [], []
    listed = isinstance(seeds, list)
    ep = seeds[0] if listed else seeds
    while (ep < len(seeds)) if listed else True:
        if listed or ep == seeds:
            try:
                env.seed(ep)
                next_state = env.reset()
            except AttributeError:
                next_state, _ = env.reset(seed=ep)
                env.action_space.seed(ep)
        else:
            next_state = env.reset()
            if isinstance(next_state, tuple):
                next_state, _ = next_state
        ts, next_done = 0, False
        while not next_done:
            states.append(to_tensor(next_state))
            dones.append(next_done)
            if actor is None or np.random.random() <= random_frac:
                action = env.action_space.sample()
            else:
                try:
                    action = actor(env, next_state)
                except TypeError:
                    try:
                        action = actor.act(next_state, "cpu")
                    except RuntimeError:
                        action = actor.act(next_state, "cuda")
            next_state, reward, next_done, _ = env.step(action)
            if "antmaze" in env.unwrapped.spec.name:
                reward -= 1
            real_done = bool(next_done and ts < max_steps - 1)
            actions.append(action)
            rewards.append(reward)
            next_states.append(to_tensor(next_state))
            next_dones.append(real_done)
            if batch_size is not None and len(states) == batch_size:
                return states, actions, rewards, dones, next_states, next_dones
            ts += 1
        ep += 1
    return states, actions, rewards, dones, next_states, next_dones


class StateDepFunction(nn.Module):
    """A scalar function of the state (variance_learner.py:363-370): state-dict keys v.net.{0,2,4}.{weight,bias}."""

    def __init__(self, state_dim: int, hidden_dim: int = 256, n_hidden: int = 2):
        super().__init__()
        self.v = MLP([state_dim, *([hidden_dim] * n_hidden), 1], squeeze_output=True)

    def forward(self, state: torch.Tensor) -> torch.Tensor:
        return self.v(state)


def _rows(x, S: Optional[int] = None) -> np.ndarray:
    """A list of tensors / arrays, or a 2-D array -> float32 [n, S]."""
    if isinstance(x, torch.Tensor):
        a = x.detach().cpu().numpy()
    elif isinstance(x, np.ndarray):
        a = x
    else:
        a = np.stack([np.asarray(r.detach().cpu() if isinstance(r, torch.Tensor) else r, dtype=np.float32).reshape(-1) for r in x])
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or (S is not None and a.shape[1] != S):
        raise ValueError(f"iqlhip: expected rows of {S} floats, got an array of shape {list(a.shape)}")
    return a


def _column(x, B: int, what: str) -> np.ndarray:
    a = np.asarray([float(v) for v in x], dtype=np.float32) if not isinstance(x, np.ndarray) else x.astype(np.float32).reshape(-1)
    if a.shape != (B,):
        raise ValueError(f"iqlhip: {what} must hold {B} values, got {a.shape[0]}")
    return a


def pack_block(state_dim: int, observations, rewards, next_observations, next_dones) -> Tuple[np.ndarray, int]:
    """The step's packed block (include/iqlhip.h): B states [B][S], the last next-state [S], B rewards, B next-done
    flags as 0 / 1 — B * S + S + 2 B float32 — and B."""
    S = state_dim
    obs = _rows(observations, S)
    B = obs.shape[0]
    if not 1 <= B <= VAR_MAX_ROWS:
        raise ValueError(f"iqlhip: a variance-learner step takes 1..{VAR_MAX_ROWS} rows, got {B}")
    if len(next_observations) != B:
        raise ValueError(f"iqlhip: next_observations must hold {B} rows, got {len(next_observations)}")
    last = _rows([next_observations[B - 1]], S)
    out = np.empty(B * S + S + 2 * B, dtype=np.float32)
    out[:B * S] = obs.reshape(-1)
    out[B * S:(B + 1) * S] = last.reshape(-1)
    out[(B + 1) * S:(B + 1) * S + B] = _column(rewards, B, "rewards")
    out[(B + 1) * S + B:] = _column(next_dones, B, "next_dones")
    return out, B


def adam_scalars(lr: float, betas, eps: float, t: int, aligned_rewards: bool = False) -> hb.VarScalars:
    """Adam's scalars of step t (>= 1) of one net, in float64 as the trainer computes its own."""
    b1, b2 = float(betas[0]), float(betas[1])
    return hb.VarScalars(lr / (1.0 - b1 ** t), (1.0 - b2 ** t) ** 0.5, b2, 1.0 - b1, 1.0 - b2, eps, int(bool(aligned_rewards)), 0)


def _mlp_tensors(module: nn.Module) -> Dict[str, nn.Parameter]:
    lin = linear_layers(module)
    if len(lin) != 3 or lin[0].weight.shape[0] != hb.IQLHIP_HIDDEN or tuple(lin[1].weight.shape) != (hb.IQLHIP_HIDDEN,) * 2 \
            or tuple(lin[2].weight.shape) != (1, hb.IQLHIP_HIDDEN):
        raise NotImplementedError(f"iqlhip: the variance learner's kernels are built for S -> {hb.IQLHIP_HIDDEN} -> "
                                  f"{hb.IQLHIP_HIDDEN} -> 1 networks")
    return {"w0": lin[0].weight, "b0": lin[0].bias, "w1": lin[1].weight, "b1": lin[1].bias, "w2": lin[2].weight, "b2": lin[2].bias}


class VarianceLearner:
    """variance_learner.py VarianceLearner with the gradient step on the GPU.  mf / vf and the two optimizers are the
    reference's attributes; on a GPU device their parameters and Adam moments are views of the library's arenas."""

    def __init__(self, state_dim, action_dim, config, actor, batch_size=256, device=None, aligned_rewards: bool = False):
        self.state_dim = state_dim
        self.action_dim = action_dim
        self.config = config
        self.batch_size = batch_size
        self.actor = actor
        self.aligned_rewards = bool(aligned_rewards)
        if not 1 <= int(batch_size) <= VAR_MAX_ROWS:
            raise ValueError(f"iqlhip: batch_size must be in [1, {VAR_MAX_ROWS}], got {batch_size}")
        self.device = device if device is not None else getattr(config, "device", "cuda")

        self.mf = StateDepFunction(state_dim)
        self.vf = StateDepFunction(state_dim)
        self.m_optimizer = torch.optim.Adam(self.mf.parameters(), lr=.0001)
        self.mv_optimizer = torch.optim.Adam(self.vf.parameters(), lr=.0001)

        self._h = None
        self._adam_t = [0, 0]
        if torch.device(self.device).type == "cuda":
            self._attach()

    # ------------------------------------------------------------------ arenas
    def _nets(self):
        return (self.mf, self.m_optimizer), (self.vf, self.mv_optimizer)

    def _attach(self) -> None:
        dev = torch.device(self.device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self._dev = dev
        L, n = hb.var_layout(self.state_dim)
        self._layout, self._n_params = L, n
        self._params_arena = torch.zeros(n, dtype=torch.float32, device=dev)
        self._m_arena = torch.zeros(n, dtype=torch.float32, device=dev)
        self._v_arena = torch.zeros(n, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for k, (net, opt) in enumerate(self._nets()):
                t = 0
                for key, p in _mlp_tensors(net).items():
                    off = int(getattr(L[k], key))
                    view = lambda arena: arena[off: off + p.numel()].view(p.shape)
                    pv, mv, vv = view(self._params_arena), view(self._m_arena), view(self._v_arena)
                    pv.copy_(p.data.to(dev, torch.float32))
                    p.data = pv
                    st = opt.state.get(p)
                    if st and "exp_avg" in st:
                        mv.copy_(st["exp_avg"].to(dev, torch.float32))
                        vv.copy_(st["exp_avg_sq"].to(dev, torch.float32))
                        st["exp_avg"], st["exp_avg_sq"] = mv, vv
                        t = max(t, int(float(st["step"])))
                self._adam_t[k] = t
        h = C.c_void_p()
        hb.check(hb.lib().iqlhip_var_create(self.state_dim, VAR_MAX_ROWS, dev.index, C.byref(h)))
        self._h = h
        hb.check(hb.lib().iqlhip_var_bind(h, self._params_arena.data_ptr(), self._m_arena.data_ptr(), self._v_arena.data_ptr()))
        words = VAR_MAX_ROWS * self.state_dim + self.state_dim + 2 * VAR_MAX_ROWS
        self._pin = torch.empty(words, dtype=torch.float32).pin_memory()
        self._pin_np = self._pin.numpy()
        self._blk = torch.empty(words, dtype=torch.float32, device=dev)

    def _release(self) -> None:
        if getattr(self, "_h", None) is not None:
            hb.lib().iqlhip_var_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _need_gpu(self):
        if self._h is None:
            raise RuntimeError("iqlhip: the variance learner steps on the GPU only (device='cuda'); there is no CPU fall-back")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self._dev.index).cuda_stream)

    def _adam_hyper(self, opt):
        if len(opt.param_groups) != 1:
            raise NotImplementedError("one param group per optimizer expected (variance_learner.py:246-247)")
        g = opt.param_groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
            raise NotImplementedError("iqlhip implements torch.optim.Adam defaults only (no weight decay/amsgrad)")
        return float(g["lr"]), g["betas"], float(g["eps"])

    def _sync_opt_state(self, k: int) -> None:
        """optimizer.state as torch.optim.Adam leaves it after the net's t steps: the moments are the arena's views."""
        net, opt = self._nets()[k]
        for key, p in _mlp_tensors(net).items():
            off = int(getattr(self._layout[k], key))
            st = opt.state[p]
            st["step"] = torch.tensor(float(self._adam_t[k]), dtype=torch.float32)
            st["exp_avg"] = self._m_arena[off: off + p.numel()].view(p.shape)
            st["exp_avg_sq"] = self._v_arena[off: off + p.numel()].view(p.shape)

    # ------------------------------------------------------------------ the step
    def _upload(self, observations, rewards, next_observations, next_dones) -> int:
        blk, B = pack_block(self.state_dim, observations, rewards, next_observations, next_dones)
        with torch.cuda.device(self._dev):
            torch.cuda.current_stream().synchronize()        # (the pinned words may still feed the previous upload)
            self._pin_np[:blk.size] = blk
            self._blk[:blk.size].copy_(self._pin[:blk.size], non_blocking=True)
        return B

    def _read(self, n_head: int):
        loss = C.c_float(0.0)
        head = (C.c_float * (3 * max(n_head, 1)))()
        hb.check(hb.lib().iqlhip_var_read_loss(self._h, C.byref(loss), head, n_head, self._stream()))
        return float(loss.value), np.ctypeslib.as_array(head).reshape(3, -1)[:, :n_head].copy()

    def _update_v(self, batch, update_vf) -> dict:
        observations, _actions, rewards, _dones, next_observations, next_dones = batch
        k = NET_VF if update_vf else NET_MF
        lr, betas, eps = self._adam_hyper(self._nets()[k][1])
        self._need_gpu()
        B = self._upload(observations, rewards, next_observations, next_dones)
        return self._step_block(B, k, lr, betas, eps)

    def _step_block(self, B: int, k: int, lr, betas, eps) -> dict:
        """The library step of net k on the packed block in self._blk, its read-back and _update_v's dict."""
        t = self._adam_t[k] + 1
        sc = adam_scalars(lr, betas, eps, t, self.aligned_rewards)
        with torch.cuda.device(self._dev):
            hb.check(hb.lib().iqlhip_var_step(self._h, self._blk.data_ptr(), B, k, C.byref(sc), self._stream()))
            loss, head = self._read(min(5, B))
        self._adam_t[k] = t
        self._sync_opt_state(k)
        return {"variance_pred_vec": torch.from_numpy(head[2]), "value_loss": loss,
                "values_pred_vec": torch.from_numpy(head[1]), "values_samp_vec": torch.from_numpy(head[0])}

    def get_values(self, obs, rewards, next_obs, dones, next_dones):
        """(values_samp, values_pred, variance_pred), CPU tensors of B entries: forward and recurrence, no gradient."""
        self._need_gpu()
        B = self._upload(obs, rewards, next_obs, next_dones)
        out = torch.empty((3, B), dtype=torch.float32, device=self._dev)
        with torch.cuda.device(self._dev):
            hb.check(hb.lib().iqlhip_var_values(self._h, self._blk.data_ptr(), B, int(self.aligned_rewards), out.data_ptr(),
                                                self._stream()))
        out = out.cpu()
        return out[0], out[1], out[2]

    # ------------------------------------------------------------------ from a replay buffer
    def _window_source(self, buffer):
        """(rows address, ld, size, action_dim) of a GPU replay buffer whose rows this learner may read as windows."""
        if self._h is None:
            raise NotImplementedError("iqlhip: the variance learner reads replay-buffer windows on the GPU only "
                                      "(device='cuda'); there is no CPU fall-back")
        rows = buffer._rows
        if rows.device != self._dev:
            raise ValueError(f"iqlhip: the replay buffer lives on {rows.device}, the variance learner on {self._dev}")
        if int(buffer._state_dim) != int(self.state_dim):
            raise ValueError(f"iqlhip: the replay buffer's state_dim is {buffer._state_dim}, the learner's {self.state_dim}")
        return rows.data_ptr(), int(buffer._ld), int(buffer._size), int(buffer._action_dim)

    def pack_window(self, buffer, start: int) -> torch.Tensor:
        """The packed block (pack_block's layout) of the batch_size consecutive rows of `buffer` from row `start`, as a
        device tensor: one launch, nothing downloaded.  0 <= start <= size - batch_size, size the rows the buffer holds;
        a window does not wrap."""
        ptr, ld, size, A = self._window_source(buffer)
        B, S = int(self.batch_size), int(self.state_dim)
        out = torch.empty(B * S + S + 2 * B, dtype=torch.float32, device=self._dev)
        with torch.cuda.device(self._dev):
            hb.check(hb.lib().iqlhip_var_pack_window(self._h, ptr, ld, size, S, A, int(start), B, out.data_ptr(), self._stream()))
        return out

    def update_from_buffer(self, buffer, start: int, update_vf) -> dict:
        """_update_v on the window of `buffer` that starts at row `start`: one pack launch, the step, one
        synchronisation.  Bit for bit _update_v on the same rows downloaded."""
        k = NET_VF if update_vf else NET_MF
        lr, betas, eps = self._adam_hyper(self._nets()[k][1])
        ptr, ld, size, A = self._window_source(buffer)
        B = int(self.batch_size)
        with torch.cuda.device(self._dev):
            hb.check(hb.lib().iqlhip_var_pack_window(self._h, ptr, ld, size, int(self.state_dim), A, int(start), B,
                                                     self._blk.data_ptr(), self._stream()))
        return self._step_block(B, k, lr, betas, eps)

    def get_values_window(self, buffer, start: int):
        """get_values on the window of `buffer` that starts at row `start`: (values_samp, values_pred, variance_pred)."""
        ptr, ld, size, A = self._window_source(buffer)
        B = int(self.batch_size)
        out = torch.empty((3, B), dtype=torch.float32, device=self._dev)
        with torch.cuda.device(self._dev):
            hb.check(hb.lib().iqlhip_var_values_window(self._h, ptr, ld, size, int(self.state_dim), A, int(start), B,
                                                       int(self.aligned_rewards), out.data_ptr(), self._stream()))
        out = out.cpu()
        return out[0], out[1], out[2]

    def _window_starts(self, starts, last_start: int):
        """starts= of train_on_buffer as an int64 device tensor, every entry checked once to lie in [0, last_start]."""
        if isinstance(starts, np.ndarray):
            starts = torch.from_numpy(np.ascontiguousarray(starts))
        if not isinstance(starts, torch.Tensor) or starts.dtype != torch.int64:
            raise ValueError("iqlhip: starts must be an int64 tensor or array")
        t = starts.reshape(-1).to(self._dev).contiguous()
        if t.numel() < 1:
            raise ValueError("iqlhip: starts is empty")
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi > last_start:
            raise ValueError(f"iqlhip: starts must lie in [0, size - batch_size = {last_start}], got {lo} .. {hi}")
        return t

    def train_on_buffer(self, buffer, n_updates: int, seed: int, offset: int = 0, update_vf=False, starts=None) -> dict:
        """n_updates updates of mf (or vf) on windows of `buffer`, drawn and packed on the device: five launches per
        update, no host work between updates, one synchronisation per TRAIN_MAX_STEPS updates.  Update k takes the
        window whose start is index offset + k of iqlhip_draw_indices' stream under `seed` (counter offset 0) over
        size - batch_size + 1 values — or, with starts= (an int64 tensor or array, checked once), that index of the
        stream over len(starts) picks the entry.  Update k depends on offset + k alone, so neither the split into
        library calls nor a split into several train_on_buffer calls changes a result.  Returns {"losses": float32 [n],
        "starts": int64 [n]}, the windows used.

        `size` is the number of rows the buffer holds.  In a ring that has wrapped, the window that straddles the write
        pointer is not consecutive in time: pass starts= to exclude it — the first rows of
        buffer.episode_returns(...).episode_table() make windows begin at episode starts, as run_episodes' rollouts do."""
        k = NET_VF if update_vf else NET_MF
        lr, betas, eps = self._adam_hyper(self._nets()[k][1])
        ptr, ld, size, A = self._window_source(buffer)
        B, n = int(self.batch_size), int(n_updates)
        if n < 1:
            raise ValueError(f"iqlhip: n_updates must be >= 1, got {n_updates}")
        if size < B:
            raise ValueError(f"iqlhip: the replay buffer holds {size} rows, a window takes batch_size = {B}")
        st = None if starts is None else self._window_starts(starts, size - B)
        st_ptr, n_st = (None, 0) if st is None else (st.data_ptr(), st.numel())
        losses, used = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.int64)
        m64 = (1 << 64) - 1
        with torch.cuda.device(self._dev):
            done = 0
            while done < n:
                m = min(TRAIN_MAX_STEPS, n - done)
                t0 = self._adam_t[k]
                sc = (hb.VarScalars * m)(*[adam_scalars(lr, betas, eps, t0 + i + 1, self.aligned_rewards) for i in range(m)])
                hb.check(hb.lib().iqlhip_var_train_steps(self._h, ptr, ld, size, A, B, m, k, sc, int(seed) & m64,
                                                         (int(offset) + done) & m64, st_ptr, n_st, self._stream()))
                self._adam_t[k] = t0 + m
                hb.check(hb.lib().iqlhip_var_read_train_ring(self._h, losses[done:].ctypes.data_as(C.POINTER(C.c_float)),
                                                             used[done:].ctypes.data_as(C.POINTER(C.c_int64)), m, self._stream()))
                done += m
        self._sync_opt_state(k)
        return {"losses": losses, "starts": used}

    def run_training_on_buffer(self, buffer, n_updates=10000, seed=0, save_dir=SAVE_DIR, env_name="buffer", starts=None):
        """run_training with windows of a replay buffer in place of rollouts: mf is stepped for the updates
        n <= n_updates / 2 and vf for the rest (the reference's `n > n_updates / 2`), as two train_on_buffer bursts on one
        start stream (update n uses index n).  Every 100th update's loss is printed; all losses and starts are kept in
        self.buffer_log.  Saves run_training's files (`<env_name>_<guide|None>_<n_updates>_<frac>_{vf,mf}.pt`) unless
        save_dir is None; returns self.vf in eval mode, and mf is deleted."""
        n_updates = int(n_updates)
        n_mf = min(n_updates, n_updates // 2 + 1)          # the n in [0, n_updates) with n <= n_updates / 2
        logs = []
        if n_mf:
            logs.append(self.train_on_buffer(buffer, n_mf, seed, 0, False, starts))
        if n_updates - n_mf:
            logs.append(self.train_on_buffer(buffer, n_updates - n_mf, seed, n_mf, True, starts))
        self.buffer_log = {key: np.concatenate([l[key] for l in logs]) if logs else np.empty(0) for key in ("losses", "starts")}
        return self._finish_buffer_training(n_updates, save_dir, env_name)

    def _finish_buffer_training(self, n_updates: int, save_dir, env_name: str):
        """run_training_on_buffer behind its bursts (self.buffer_log holds their losses and starts): the printed losses,
        eval mode, the saved files, mf deleted; returns self.vf.  (VarianceLearnerGroup ends every member's run with it.)"""
        for n in range(0, n_updates, 100):
            print(f"Iteration {n}/{n_updates}:\nvalue_loss: {float(self.buffer_log['losses'][n])}")
        self.mf.eval()
        self.vf.eval()
        if save_dir is not None:
            os.makedirs(save_dir, exist_ok=True)
            actor_name = "guide" if self.actor is not None else None
            frac = getattr(self.config, "variance_learn_frac", 0.0)
            stem = f"{save_dir}/{env_name}_{actor_name}_{n_updates}_{str(frac).replace('.', '-')}"
            cpu = lambda m: {k: v.detach().cpu() for k, v in m.state_dict().items()}
            torch.save(cpu(self.vf), stem + "_vf.pt")
            torch.save(cpu(self.mf), stem + "_mf.pt")
        del self.mf
        return self.vf

    def flat_gradient(self, batch, update_vf):
        """Tests: (loss, the flat gradient of mf or vf in arena order) of one batch, nothing updated."""
        self._need_gpu()
        observations, _actions, rewards, _dones, next_observations, next_dones = batch
        k = NET_VF if update_vf else NET_MF
        B = self._upload(observations, rewards, next_observations, next_dones)
        n = int(self._layout[k].seg_end - self._layout[k].seg_begin)
        g = torch.empty(n, dtype=torch.float32, device=self._dev)
        with torch.cuda.device(self._dev):
            hb.check(hb.lib().iqlhip_var_forward_backward(self._h, self._blk.data_ptr(), B, k, int(self.aligned_rewards),
                                                          g.data_ptr(), self._stream()))
            loss, _ = self._read(0)
        return loss, g.cpu()

    def net_gradients(self, flat: torch.Tensor, update_vf) -> Dict[str, torch.Tensor]:
        """A flat_gradient split into {w0, b0, w1, b1, w2, b2}, shaped like the parameters."""
        k = NET_VF if update_vf else NET_MF
        L, base = self._layout[k], int(self._layout[k].seg_begin)
        return {key: flat[int(getattr(L, key)) - base: int(getattr(L, key)) - base + p.numel()].view(p.shape)
                for key, p in _mlp_tensors(self._nets()[k][0]).items()}

    def gate(self, device=None):
        """A GateHolder over a COPY of the current vf, ready for JsrlActors(..., gates=...)."""
        from iqlhip_jsrl import load_gate
        sd = {k: v.detach().cpu().clone() for k, v in self.vf.state_dict().items()}
        return load_gate(sd, action_dim=self.action_dim, device=str(self._dev) if device is None else device)

    # ------------------------------------------------------------------ the reference's loop
    def run_training(self, env, max_steps, actor, n_updates=10000, evaluate=False, save_dir=SAVE_DIR):
        """variance_learner.py:297-328: n_updates rollouts and updates, mf in the first half and vf once n > n_updates / 2;
        every 100th update is printed and its loss kept.  Saves `<env>_<guide|None>_<n_updates>_<frac>_{vf,mf}.pt` (CPU
        tensors) under save_dir unless it is None; returns self.vf in eval mode, and mf is deleted.  evaluate=True only
        saves the loss curve, when matplotlib is there (the reference's test_model is not ported)."""
        vf_losses: List[float] = []
        log_freq = 100
        log_dict: dict = {}
        for n in range(n_updates):
            batch = run_episodes(env, max_steps, n, actor, batch_size=self.batch_size, random_frac=self.config.variance_learn_frac)
            log_dict = self._update_v(batch, update_vf=(n > n_updates / 2))
            if n % log_freq == 0:
                print(f"Iteration {n}/{n_updates}:")
                for k, v in log_dict.items():
                    if "loss" in k:
                        vf_losses.append(v)
                    print(f"{k}: {v}")
        log_dict["var_learner/loss"] = vf_losses
        self.mf.eval()
        self.vf.eval()
        if save_dir is not None:
            os.makedirs(save_dir, exist_ok=True)
            name = env.unwrapped.spec.name
            if evaluate:
                try:
                    from matplotlib import pyplot as plt
                    plt.plot(vf_losses)
                    plt.savefig(f"{save_dir}/losses_vf_{name}.png")
                except ImportError:
                    pass
            actor_name = "guide" if self.actor is not None else None
            stem = f"{save_dir}/{name}_{actor_name}_{n_updates}_{str(self.config.variance_learn_frac).replace('.', '-')}"
            cpu = lambda m: {k: v.detach().cpu() for k, v in m.state_dict().items()}
            torch.save(cpu(self.vf), stem + "_vf.pt")
            torch.save(cpu(self.mf), stem + "_mf.pt")
        del self.mf
        return self.vf


# ---------------------------------------------------------------------- groups of learners
MAX_GROUP = hb.IQLHIP_MAX_GROUP


def per_member(x, K: int, what: str) -> list:
    """An argument given once for all members, or as a list / tuple of K entries: the K entries."""
    if isinstance(x, (list, tuple)):
        if len(x) != K:
            raise ValueError(f"iqlhip: {what} must hold one entry per member ({K}), got {len(x)}")
        return list(x)
    return [x] * K


def per_member_starts(starts, K: int) -> list:
    """starts= of a group burst as K entries.  None: every member draws from its whole buffer.  A tensor, an array or a
    list of integers: that one list for every member.  A list / tuple with a None, a tensor, an array or a list in it:
    one entry per member, None for a member that draws from its whole buffer."""
    if starts is None:
        return [None] * K
    if isinstance(starts, (list, tuple)) and any(s is None or isinstance(s, (torch.Tensor, np.ndarray, list, tuple)) for s in starts):
        if len(starts) != K:
            raise ValueError(f"iqlhip: starts must hold one entry per member ({K}), got {len(starts)}")
        return [None if s is None else (np.asarray(s, dtype=np.int64) if isinstance(s, (list, tuple)) else s) for s in starts]
    if isinstance(starts, (list, tuple)):
        starts = np.asarray(starts, dtype=np.int64)
    return [starts] * K


def burst_chunks(n_updates: int) -> List[int]:
    """The library calls of a burst of n_updates: at most TRAIN_MAX_STEPS updates each, as train_on_buffer splits it."""
    return [min(TRAIN_MAX_STEPS, n_updates - done) for done in range(0, n_updates, TRAIN_MAX_STEPS)]


def group_scalar_table(hypers, t0s, m: int, aligned):
    """Adam's scalars of m updates of K members, update-major [m][K] (iqlhip_var_group_train_steps): entry [i][k] is
    adam_scalars of member k's step t0s[k] + i + 1 under hypers[k] = (lr, betas, eps)."""
    K = len(hypers)
    return (hb.VarScalars * (m * K))(*[adam_scalars(*hypers[k], t0s[k] + i + 1, aligned[k]) for i in range(m) for k in range(K)])


class VarianceLearnerGroup:
    """K VarianceLearners of one state_dim and batch_size on one GPU, updated by one set of launches per update
    (iqlhip_var_group).  Every call is the solo call of the same name for every member, bit for bit: `update` is K
    `_update_v`s, `train_on_buffer` K bursts.  A member stays a VarianceLearner: it may be stepped alone before and
    after a group call; step counts and optimizer state are kept per member."""

    def __init__(self, learners):
        self.learners = list(learners)
        K = len(self.learners)
        if K < 1 or K > MAX_GROUP:
            raise ValueError(f"iqlhip: a variance-learner group takes 1..{MAX_GROUP} members, got {K}")
        for i, l in enumerate(self.learners):
            if getattr(l, "_h", None) is None:
                raise NotImplementedError(f"iqlhip: member {i}: the variance learner steps on the GPU only (device='cuda'); "
                                          "there is no CPU fall-back")
            for j in range(i):
                if self.learners[j] is l:
                    raise ValueError(f"iqlhip: member {i}: the learner is member {j} too")
            first = self.learners[0]
            if int(l.state_dim) != int(first.state_dim):
                raise ValueError(f"iqlhip: member {i}: state_dim = {l.state_dim}, member 0's is {first.state_dim}")
            if l._dev != first._dev:
                raise ValueError(f"iqlhip: member {i}: device {l._dev}, member 0's is {first._dev}")
        self._dev = self.learners[0]._dev
        self._g = None
        self._members = None          # the library handles the group was built over

    # ------------------------------------------------------------------ the handle
    def _release(self) -> None:
        if getattr(self, "_g", None) is not None:
            hb.lib().iqlhip_var_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _group(self):
        """The library group over the members' current handles (rebuilt when a member has re-attached)."""
        for i, l in enumerate(self.learners):
            if l._h is None:
                raise RuntimeError(f"iqlhip: member {i} has released its library handle")
        now = [int(l._h.value) for l in self.learners]
        if self._g is None or now != self._members:
            self._release()
            g = C.c_void_p()
            hb.check(hb.lib().iqlhip_var_group_create((C.c_void_p * len(now))(*now), len(now), C.byref(g)))
            self._g, self._members = g, now
        return self._g

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self._dev.index).cuda_stream)

    @property
    def K(self) -> int:
        return len(self.learners)

    def _hypers(self, k: int):
        return [l._adam_hyper(l._nets()[k][1]) for l in self.learners]

    def _aligned(self):
        return [l.aligned_rewards for l in self.learners]

    def _batch_size(self) -> int:
        B = int(self.learners[0].batch_size)
        for i, l in enumerate(self.learners):
            if int(l.batch_size) != B:
                raise ValueError(f"iqlhip: member {i}: batch_size = {l.batch_size}, member 0's is {B}")
        return B

    @staticmethod
    def _ptrs(values):
        return (C.c_void_p * len(values))(*values)

    def _windows(self, buffers):
        """(rows[K], ld[K], size[K], action_dim[K]) as the library's host arrays, and the sizes."""
        K = self.K
        src = [l._window_source(b) for l, b in zip(self.learners, per_member(buffers, K, "buffers"))]
        return (self._ptrs([s[0] for s in src]), (C.c_int64 * K)(*[s[1] for s in src]), (C.c_int64 * K)(*[s[2] for s in src]),
                (C.c_int32 * K)(*[s[3] for s in src])), [s[2] for s in src]

    # ------------------------------------------------------------------ eager
    def _read(self, n_head: int):
        K = self.K
        losses = (C.c_float * K)()
        heads = (C.c_float * (K * 3 * max(n_head, 1)))()
        hb.check(hb.lib().iqlhip_var_group_read_loss(self._g, losses, heads, n_head, self._stream()))
        return list(losses), np.ctypeslib.as_array(heads)[:K * 3 * n_head].reshape(K, 3, n_head).copy()

    def _stepped(self, B: int, k: int, launch) -> List[dict]:
        """`launch(scalars)` (a library step of net k for every member), the read-back, and the members' _update_v dicts."""
        sc = group_scalar_table(self._hypers(k), [l._adam_t[k] for l in self.learners], 1, self._aligned())
        with torch.cuda.device(self._dev):
            hb.check(launch(sc))
            losses, heads = self._read(min(5, B))
        out = []
        for i, l in enumerate(self.learners):
            l._adam_t[k] += 1
            l._sync_opt_state(k)
            out.append({"variance_pred_vec": torch.from_numpy(heads[i][2]), "value_loss": float(losses[i]),
                        "values_pred_vec": torch.from_numpy(heads[i][1]), "values_samp_vec": torch.from_numpy(heads[i][0])})
        return out

    def _upload(self, packed) -> int:
        """packed[K] = (observations, rewards, next_observations, next_dones): every member's block, of one length."""
        lengths = [len(p[0]) for p in packed]
        for i, b in enumerate(lengths):
            if b != lengths[0]:
                raise ValueError(f"iqlhip: member {i}: the batch holds {b} rows, member 0's {lengths[0]}")
        return [l._upload(*p) for l, p in zip(self.learners, packed)][0]

    def _values(self, B: int, call):
        K = self.K
        out = torch.empty((K, 3, B), dtype=torch.float32, device=self._dev)
        with torch.cuda.device(self._dev):
            hb.check(call((C.c_int32 * K)(*[int(a) for a in self._aligned()]), self._ptrs([out[i].data_ptr() for i in range(K)])))
        out = out.cpu()
        return [(out[i][0], out[i][1], out[i][2]) for i in range(K)]

    def update(self, batches, update_vf) -> List[dict]:
        """_update_v for every member: batches[K] are run_episodes-shaped batches of one length; K _update_v dicts."""
        k = NET_VF if update_vf else NET_MF
        batches = per_member(list(batches), self.K, "batches")
        self._hypers(k)
        g = self._group()
        B = self._upload([(b[0], b[2], b[4], b[5]) for b in batches])
        blocks = self._ptrs([l._blk.data_ptr() for l in self.learners])
        return self._stepped(B, k, lambda sc: hb.lib().iqlhip_var_group_step(g, blocks, B, k, sc, self._stream()))

    def get_values(self, batches):
        """get_values for every member: batches[K] = (obs, rewards, next_obs, dones, next_dones); K triples of CPU tensors."""
        batches = per_member(list(batches), self.K, "batches")
        g = self._group()
        B = self._upload([(b[0], b[1], b[2], b[4]) for b in batches])
        blocks = self._ptrs([l._blk.data_ptr() for l in self.learners])
        return self._values(B, lambda al, outs: hb.lib().iqlhip_var_group_values(g, blocks, B, al, outs, self._stream()))

    # ------------------------------------------------------------------ windows of replay buffers
    def _starts(self, starts):
        K = self.K
        return (C.c_int64 * K)(*[int(s) for s in per_member(starts, K, "starts")])

    def update_from_buffer(self, buffers, starts, update_vf) -> List[dict]:
        """update_from_buffer for every member: buffers is one buffer or K, starts an int or K."""
        k = NET_VF if update_vf else NET_MF
        self._hypers(k)
        B = self._batch_size()
        win, _ = self._windows(buffers)
        st = self._starts(starts)
        g = self._group()
        return self._stepped(B, k, lambda sc: hb.lib().iqlhip_var_group_step_windows(g, *win, st, B, k, sc, self._stream()))

    def get_values_window(self, buffers, starts):
        """get_values_window for every member: K triples (values_samp, values_pred, variance_pred)."""
        B = self._batch_size()
        win, _ = self._windows(buffers)
        st = self._starts(starts)
        g = self._group()
        return self._values(B, lambda al, outs: hb.lib().iqlhip_var_group_values_windows(g, *win, st, B, al, outs, self._stream()))

    def train_on_buffer(self, buffers, n_updates: int, seeds, offsets=0, update_vf=False, starts=None) -> dict:
        """train_on_buffer for every member, as one burst: five launches per update for all K.  buffers: one buffer or K;
        seeds, offsets: an int or K; starts: per_member_starts' forms.  Member i's update j uses index offsets[i] + j of
        the stream under seeds[i], as its solo burst does.  Returns {"losses": float32 [K, n_updates], "starts": int64
        [K, n_updates]}."""
        k = NET_VF if update_vf else NET_MF
        K, n = self.K, int(n_updates)
        hypers = self._hypers(k)
        B = self._batch_size()
        win, sizes = self._windows(buffers)
        seeds, offsets = per_member(seeds, K, "seeds"), per_member(offsets, K, "offsets")
        lists = per_member_starts(starts, K)
        if n < 1:
            raise ValueError(f"iqlhip: n_updates must be >= 1, got {n_updates}")
        for i, size in enumerate(sizes):
            if size < B:
                raise ValueError(f"iqlhip: member {i}: the replay buffer holds {size} rows, a window takes batch_size = {B}")
        for i, (l, s) in enumerate(zip(self.learners, lists)):
            if s is not None:
                try:
                    lists[i] = l._window_starts(s, sizes[i] - B)
                except ValueError as e:
                    raise ValueError(f"iqlhip: member {i}: {e}") from None
        st_ptrs = self._ptrs([None if s is None else s.data_ptr() for s in lists])
        n_st = (C.c_int64 * K)(*[0 if s is None else s.numel() for s in lists])
        m64 = (1 << 64) - 1
        seeds_c = (C.c_uint64 * K)(*[int(s) & m64 for s in seeds])
        g = self._group()
        losses, used = np.empty((K, n), dtype=np.float32), np.empty((K, n), dtype=np.int64)
        with torch.cuda.device(self._dev):
            done = 0
            for m in burst_chunks(n):
                sc = group_scalar_table(hypers, [l._adam_t[k] for l in self.learners], m, self._aligned())
                offs = (C.c_uint64 * K)(*[(int(o) + done) & m64 for o in offsets])
                hb.check(hb.lib().iqlhip_var_group_train_steps(g, *win, B, m, k, sc, seeds_c, offs, st_ptrs, n_st, self._stream()))
                for l in self.learners:
                    l._adam_t[k] += m
                lo, so = np.empty((K, m), dtype=np.float32), np.empty((K, m), dtype=np.int64)
                hb.check(hb.lib().iqlhip_var_group_read_train_ring(g, lo.ctypes.data_as(C.POINTER(C.c_float)),
                                                                   so.ctypes.data_as(C.POINTER(C.c_int64)), m, self._stream()))
                losses[:, done:done + m], used[:, done:done + m] = lo, so
                done += m
        for l in self.learners:
            l._sync_opt_state(k)
        return {"losses": losses, "starts": used}

    def run_training_on_buffer(self, buffers, n_updates=10000, seeds=0, env_names="buffer", save_dir=SAVE_DIR, starts=None):
        """run_training_on_buffer for every member as two bursts: mf for the updates n <= n_updates / 2, vf for the rest.
        env_names: one name or K (members that share a name, an actor setting and a variance_learn_frac write the same
        files, as their solo runs would).  Every member's buffer_log, printed losses, saved files and deleted mf are the
        solo call's; returns the K vf networks in eval mode."""
        K, n_updates = self.K, int(n_updates)
        names = per_member(env_names, K, "env_names")
        n_mf = min(n_updates, n_updates // 2 + 1)
        logs = []
        if n_mf:
            logs.append(self.train_on_buffer(buffers, n_mf, seeds, 0, False, starts))
        if n_updates - n_mf:
            logs.append(self.train_on_buffer(buffers, n_updates - n_mf, seeds, n_mf, True, starts))
        out = []
        for i, l in enumerate(self.learners):
            l.buffer_log = {key: np.concatenate([x[key][i] for x in logs]) if logs else np.empty(0) for key in ("losses", "starts")}
            out.append(l._finish_buffer_training(n_updates, save_dir, names[i]))
        return out

    def gates(self, device=None) -> list:
        """The members' gate()s, in member order: JsrlActors(learners, guides, gates=group.gates())."""
        return [l.gate(device) for l in self.learners]
