"""JSRL action selection on the device (include/iqlhip.h iqlhip_jsrl_act): at every environment step a
guide policy or the learner acts (jsrl_utils.learner_or_guide_action).  The host-known part of the reference's four
horizon rules is restated here (who_from_config) and folded into one byte per row; the library evaluates the
state-dependent gate (the `variance` horizon's network), both policies and the per-row choice in one set of launches.
A fourth byte, WHO_CRITIC, lets a member's twin critic pick between the two proposed actions (iqlhip_jsrl_act_q).
Curriculum stages, goal distances, heuristics and the variance learner's training stay host logic."""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence

import numpy as np
import torch

import iqlhip_binding as hb
from iqlhip_replay import check_online_ring, draw_indices

WHO_GUIDE, WHO_LEARNER, WHO_GATE, WHO_CRITIC = 0, 1, 2, 3
HORIZON_FNS = ("time_step", "agent_type", "goal_dist", "variance")


def _listed(x, K=None):
    return list(x) if isinstance(x, (list, tuple)) else [x] * (1 if K is None else K)


def who_from_config(config, horizon_fn: str, steps, states, envs, goal_dist=None):
    """The host-known part of the reference's horizon functions (jsrl_utils.py:359-496) for K members: `config` (one,
    or one per member) carries curriculum_stage, curriculum_stage_idx, n_curriculum_stages, ep_agent_type and
    agent_type_stage; steps[k], states[k], envs[k] are the member's time step, state and env.  Returns (who, horizon):
    who[k] an int8 array of one byte — 0 guide, 1 learner, 2 "the device gate decides" — and horizon[k] the host
    horizon value (the time step, the goal distance `goal_dist(state, env)`, ep_agent_type), or None for `variance`,
    whose horizon is the gate's output.  A NaN stage gives 1.  `agent_type` draws np.random.sample() exactly when the
    reference does."""
    if horizon_fn not in HORIZON_FNS:
        raise ValueError(f"iqlhip: unknown horizon function {horizon_fn!r} (one of {HORIZON_FNS})")
    steps = _listed(steps)
    K = len(steps)
    configs, states, envs = _listed(config, K), _listed(states, K) if isinstance(states, (list, tuple)) else [states] * K, _listed(envs, K)
    if len(configs) != K or len(states) != K or len(envs) != K:
        raise ValueError(f"iqlhip: who_from_config needs one config, step, state and env per member ({K})")
    if horizon_fn == "goal_dist" and goal_dist is None:
        raise ValueError("iqlhip: the goal_dist horizon needs goal_dist(state, env), the caller's distance function")
    who, horizon = [], []
    for cfg, step, s, env in zip(configs, steps, states, envs):
        stage = cfg.curriculum_stage
        last = cfg.curriculum_stage_idx == (cfg.n_curriculum_stages - 1)
        allowed = cfg.ep_agent_type <= cfg.agent_type_stage
        h = {"time_step": lambda: step, "agent_type": lambda: cfg.ep_agent_type,
             "goal_dist": lambda: goal_dist(s, env), "variance": lambda: None}[horizon_fn]()
        if np.isnan(stage):
            w = WHO_LEARNER
        elif horizon_fn == "time_step":
            w = int((step >= stage or last) and allowed)
        elif horizon_fn == "goal_dist":
            w = int((h <= stage or last) and allowed)
        elif horizon_fn == "agent_type":
            w = WHO_GUIDE
            if last or cfg.ep_agent_type <= stage:
                w = int(np.random.sample() < stage)
        else:
            w = WHO_GUIDE if not allowed else (WHO_LEARNER if last else WHO_GATE)
        who.append(np.array([w], dtype=np.int8))
        horizon.append(h)
    return who, horizon


class GateHolder:
    """A value network on the device behind a library context of its own: what a JSRL gate needs.  Built by load_gate
    from a StateDepFunction / ValueFunction state dict; the policy and Q networks of the context are placeholders."""

    def __init__(self, trainer):
        self.trainer = trainer

    @property
    def vf(self):
        return self.trainer.vf


def load_gate(state_dict, action_dim: int = 1, device: str = "cuda") -> GateHolder:
    """A gate from the state dict of the reference's StateDepFunction (variance_learner.py) or of a ValueFunction — keys
    `v.net.*` — so that its saved `*_vf.pt` files load.  action_dim: the learner's, so that gate and learner share one
    packed copy of the states (any value works)."""
    import iql
    S = int(state_dict["v.net.0.weight"].shape[1])
    vf = iql.ValueFunction(S)
    vf.load_state_dict(state_dict)
    qf, actor = iql.TwinQ(S, action_dim), iql.DeterministicPolicy(S, action_dim, 1.0)
    vf, qf, actor = vf.to(device), qf.to(device), actor.to(device)
    tr = iql.ImplicitQLearning(max_action=1.0, actor=actor, actor_optimizer=torch.optim.Adam(actor.parameters(), lr=0.0),
                               q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=0.0), v_network=vf,
                               v_optimizer=torch.optim.Adam(vf.parameters(), lr=0.0), max_steps=None, device=device)
    return GateHolder(tr)


def _trainer_of(x):
    return x.trainer if isinstance(x, GateHolder) else x


class JsrlActors:
    """K (learner, guide, gate) triples that act together.  learners / guides: ImplicitQLearning trainers on one GPU
    (or a single one of each); a guide may be None ("guide is None" of the reference: the learner always acts);
    gates: None, or per member None / a GateHolder / any trainer — its value network is the gate.  critics: None, True
    (every member's learner), or per member None / True / a trainer — its twin Q decides the rows whose byte is
    WHO_CRITIC (3); a member without one refuses a 3 as before."""

    def __init__(self, learners, guides, gates=None, critics=None):
        self.learners = _listed(learners)
        K = len(self.learners)
        self.guides = _listed(guides, K)
        self.gates = [None] * K if gates is None else _listed(gates, K)
        if K < 1 or K > hb.IQLHIP_MAX_GROUP:
            raise ValueError(f"iqlhip: JsrlActors takes 1..{hb.IQLHIP_MAX_GROUP} members, got {K}")
        if len(self.guides) != K or len(self.gates) != K:
            raise ValueError(f"iqlhip: JsrlActors needs one guide (and gate) per learner: {K} learners, "
                             f"{len(self.guides)} guides, {len(self.gates)} gates")
        self.critics = [None] * K if critics is None else ([True] * K if critics is True else list(critics))
        if len(self.critics) != K:
            raise ValueError(f"iqlhip: JsrlActors needs one critic entry per learner: {K} learners, {len(self.critics)} critics")
        self._h = None
        self._ctxs = None
        self._bufs = None
        self._gate_only = None

    # ------------------------------------------------------------------ the library handle
    def _members(self):
        ls = self.learners
        gs = [l if g is None else g for l, g in zip(ls, self.guides)]
        vs = [None if v is None else _trainer_of(v) for v in self.gates]
        return ls, gs, vs

    def _critic_trainers(self):
        """Per member: None (no critic), else the trainer whose twin Q decides a 3 (True: the learner itself)."""
        return [None if c is None else (l if c is True else c) for l, c in zip(self.learners, self.critics)]

    def _check_members(self):
        ls, gs, vs = self._members()
        for k, (l, g, v, c) in enumerate(zip(ls, gs, vs, self._critic_trainers())):
            if c is not None and (getattr(c, "_ctx", None) is None or c._S != l._S or c._A != l._A):
                raise ValueError(f"iqlhip: JSRL member {k}: the critic must be a GPU trainer of the learner's state_dim and action_dim")
            for t in (l, g, v):
                if t is not None and getattr(t, "_ctx", None) is None:
                    raise RuntimeError(f"iqlhip: JSRL member {k} needs trainers on the GPU (device='cuda')")
            if g._S != l._S or (v is not None and v._S != l._S):
                raise ValueError(f"iqlhip: JSRL member {k}: state_dim differs between learner, guide and gate")
            if g._A != l._A:
                raise ValueError(f"iqlhip: JSRL member {k}: action_dim differs between learner and guide")

    def _handle(self):
        ls, gs, vs = self._members()
        cs = self._critic_trainers()
        ctxs = tuple(None if t is None else t._ctx.value for t in ls + gs + vs + cs)
        if self._h is not None and ctxs == self._ctxs:
            return self._h
        self._release()
        K = len(ls)
        arr = lambda ts: (C.c_void_p * K)(*[None if t is None else t._ctx for t in ts])
        h = C.c_void_p()
        hb.check(hb.lib().iqlhip_jsrl_create(arr(ls), arr(gs), arr(vs), K, C.byref(h)))
        self._h, self._ctxs = h, ctxs
        if any(c is not None and c is not l for c, l in zip(cs, ls)):
            hb.check(hb.lib().iqlhip_jsrl_set_critics(h, arr(cs)))
        return h

    def _release(self):
        if getattr(self, "_h", None) is not None:
            hb.lib().iqlhip_jsrl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def eval(self):
        for l in self.learners:
            l.actor.eval()

    def train(self):
        for l in self.learners:
            l.actor.train()

    who_from_config = staticmethod(who_from_config)

    # ------------------------------------------------------------------ arguments
    def _who_arrays(self, who, rows: Sequence[int]) -> List[Optional[np.ndarray]]:
        K = len(self.learners)
        who = _listed(who, K) if not isinstance(who, np.ndarray) or K == 1 else list(who)
        if len(who) != K:
            raise ValueError(f"iqlhip: JSRL act of {K} members needs who as a list of {K} entries")
        out = []
        for k, (w, n) in enumerate(zip(who, rows)):
            if n == 0:
                out.append(None)
                continue
            w = np.ascontiguousarray(np.broadcast_to(np.asarray(w, dtype=np.int8).reshape(-1), (n,)) if np.size(w) == 1
                                     else np.asarray(w, dtype=np.int8).reshape(-1))
            if w.shape[0] != n:
                raise ValueError(f"iqlhip: JSRL member {k}: {w.shape[0]} who entries for {n} rows")
            if w.min() < 0 or w.max() > (2 if self.critics[k] is None else 3):
                raise ValueError(f"iqlhip: JSRL member {k}: who values must be 0 (guide), 1 (learner) or 2 (gate)" +
                                 ("" if self.critics[k] is None else " or 3 (critic)"))
            if self.guides[k] is None:
                w = np.ones_like(w)                 # "guide is None": the learner acts, the horizon is still reported
            if (w == WHO_GATE).any() and self.gates[k] is None:
                raise ValueError(f"iqlhip: JSRL member {k}: who == 2 needs a gate")
            out.append(w)
        return out

    def _gate_max(self, gate_max, who) -> List[float]:
        K = len(self.learners)
        gm = [0.0] * K if gate_max is None else [float(np.float32(x)) for x in _listed(gate_max, K)]
        if len(gm) != K:
            raise ValueError(f"iqlhip: JSRL act of {K} members needs gate_max as {K} values")
        if gate_max is None and any(w is not None and (w == WHO_GATE).any() for w in who):
            raise ValueError("iqlhip: who == 2 needs gate_max (the curriculum stage the gate's value is compared with)")
        return gm

    def _q_inv_temp(self, q_inv_temp) -> List[float]:
        """One inverse temperature per member: None or math.inf is the argmax."""
        K = len(self.learners)
        qt = [math.inf] * K if q_inv_temp is None else [float(np.float32(x)) for x in _listed(q_inv_temp, K)]
        if len(qt) != K:
            raise ValueError(f"iqlhip: JSRL act of {K} members needs q_inv_temp as {K} values")
        if any(not x >= 0.0 for x in qt):
            raise ValueError("iqlhip: q_inv_temp must be >= 0 (None or inf: argmax)")
        return qt

    def _uses_dropout(self) -> bool:
        ls, gs, _ = self._members()
        return any(t.acts_with_dropout() and t._act_dropout for t in ls + gs)

    def _call(self, rows, in_ptrs, out_ptrs, who, gm, flag_ptrs, h_ptrs, sample: Optional[bool], flags: int,
              qt=None, q_ptrs=None):
        K = len(self.learners)
        ls, gs, _ = self._members()
        for t in ls + gs:
            t._prepare_act()
        seeds = []
        for l, n in zip(ls, rows):
            draw = (l.actor.training if sample is None else sample) and l._gaussian
            seeds.append(l._act_seed() if (n and draw) else 0)
        if qt is not None:
            hb.check(hb.lib().iqlhip_jsrl_act_q(
                self._handle(), (C.c_void_p * K)(*in_ptrs), ls[0]._S, (C.c_int32 * K)(*rows),
                (C.c_void_p * K)(*[None if w is None else w.ctypes.data for w in who]), (C.c_float * K)(*gm),
                (C.c_uint64 * K)(*seeds), (C.c_float * K)(*[float(l.actor.max_action) for l in ls]),
                (C.c_float * K)(*[float(g.actor.max_action) for g in gs]), (C.c_void_p * K)(*out_ptrs), ls[0]._A,
                (C.c_void_p * K)(*flag_ptrs), (C.c_void_p * K)(*h_ptrs), (C.c_float * K)(*qt), (C.c_void_p * K)(*q_ptrs),
                flags, ls[0]._stream()))
            return
        hb.check(hb.lib().iqlhip_jsrl_act(
            self._handle(), (C.c_void_p * K)(*in_ptrs), ls[0]._S, (C.c_int32 * K)(*rows),
            (C.c_void_p * K)(*[None if w is None else w.ctypes.data for w in who]), (C.c_float * K)(*gm),
            (C.c_uint64 * K)(*seeds), (C.c_float * K)(*[float(l.actor.max_action) for l in ls]),
            (C.c_float * K)(*[float(g.actor.max_action) for g in gs]), (C.c_void_p * K)(*out_ptrs), ls[0]._A,
            (C.c_void_p * K)(*flag_ptrs), (C.c_void_p * K)(*h_ptrs), flags, ls[0]._stream()))

    # ------------------------------------------------------------------ acting
    def act(self, states: Sequence, who, gate_max=None, q_inv_temp=None):
        """learner_or_guide_action for every member with states (None: skipped) in ONE library call and one wait:
        states[k] is [S] or [n_k, S]; who[k] a byte or n_k bytes (0 guide, 1 learner, 2 the gate decides against
        gate_max[k]).  Returns per member (actions [n_k, A], use_learner [n_k] int32, horizon [n_k] float32 — the
        gate's value, None for a member without a gate), or None.  A learner row samples iff the learner's actor is in
        training mode and Gaussian, as actor.act decides; its act() counter then advances by one per call.
        A member with a critic also takes who == 3 (its twin Q picks the candidate: argmax, or a Boltzmann draw at
        q_inv_temp — a float or one per member; None or inf: argmax) and returns a fourth entry q [n_k, 4] float32 =
        (Q1g, Q2g, Q1l, Q2l), NaN on rows whose byte is not 3."""
        K = len(self.learners)
        if not isinstance(states, (list, tuple)) or len(states) != K:
            raise ValueError(f"iqlhip: JSRL act of {K} members needs states as a list of {K} entries")
        self._check_members()
        S, A = self.learners[0]._S, self.learners[0]._A
        if any(l._S != S or l._A != A for l in self.learners):
            raise ValueError("iqlhip: JSRL members must share state_dim and action_dim")
        xs = [None if s is None else np.asarray(s, dtype=np.float32).reshape(-1, S) for s in states]
        rows = [0 if x is None else x.shape[0] for x in xs]
        who = self._who_arrays(who, rows)
        gm = self._gate_max(gate_max, who)
        qt = self._q_inv_temp(q_inv_temp)
        with_q = any(c is not None for c in self.critics)
        if self._uses_dropout():
            if any(w is not None and (w == WHO_CRITIC).any() for w in who):
                raise NotImplementedError("iqlhip: who == 3 has no form with inference dropout (the fall-back composes "
                                          "solo calls and has no critic stage)")
            got = self._act_separately(xs, who, gm)
            return [g if (g is None or self.critics[k] is None) else g + (np.full((rows[k], 4), np.nan, np.float32),)
                    for k, g in enumerate(got)]
        total = sum(rows)
        if total == 0:
            return [None] * K
        if self._bufs is None or self._bufs[0].shape[0] < total:
            n = max(total, K)
            bufs = [torch.empty((n, S), dtype=torch.float32).pin_memory(), torch.empty((n, A), dtype=torch.float32).pin_memory(),
                    torch.empty((n,), dtype=torch.int32).pin_memory(), torch.empty((n,), dtype=torch.float32).pin_memory(),
                    torch.empty((n, 4), dtype=torch.float32).pin_memory()]
            self._bufs = bufs + [b.numpy() for b in bufs]
        h_in, h_out, h_flag, h_h, h_q, in_np, out_np, flag_np, h_np, q_np = self._bufs
        ins, outs, flags, hs, qs, off, offs = [], [], [], [], [], 0, []
        for k in range(K):
            n = rows[k]
            offs.append(off)
            if n:
                in_np[off:off + n] = xs[k]
            ins.append(h_in.data_ptr() + 4 * S * off if n else None)
            outs.append(h_out.data_ptr() + 4 * A * off if n else None)
            flags.append(h_flag.data_ptr() + 4 * off if n else None)
            hs.append(h_h.data_ptr() + 4 * off if (n and self.gates[k] is not None) else None)
            has3 = n and (who[k] == WHO_CRITIC).any()
            qs.append(h_q.data_ptr() + 16 * off if has3 else None)
            if n and not has3:
                q_np[off:off + n] = np.nan
            off += n
        if with_q:
            self._call(rows, ins, outs, who, gm, flags, hs, None, hb.IQLHIP_GROUP_ACT_WAIT, qt, qs)
        else:
            self._call(rows, ins, outs, who, gm, flags, hs, None, hb.IQLHIP_GROUP_ACT_WAIT)
        return [None if not rows[k] else
                (out_np[offs[k]:offs[k] + rows[k]].copy(), flag_np[offs[k]:offs[k] + rows[k]].copy(),
                 h_np[offs[k]:offs[k] + rows[k]].copy() if self.gates[k] is not None else None) +
                (() if self.critics[k] is None else (q_np[offs[k]:offs[k] + rows[k]].copy(),)) for k in range(K)]

    def actor_forward(self, states: Sequence[torch.Tensor], who, gate_max=None, sample: bool = False, q_inv_temp=None):
        """The same for [n_k, S] device tensors (n_k up to the members' row cap; half of it for a member with a 3):
        returns per member device tensors (actions [n_k, A], use_learner [n_k] int32, horizon [n_k] float32 or None,
        and q [n_k, 4] for a member with a critic), queued on the trainers' stream."""
        K = len(self.learners)
        if not isinstance(states, (list, tuple)) or len(states) != K:
            raise ValueError(f"iqlhip: JSRL actor_forward of {K} members needs states as a list of {K} tensors")
        self._check_members()
        if self._uses_dropout():
            raise NotImplementedError("iqlhip: JSRL actor_forward has no form with inference dropout; use act()")
        l0 = self.learners[0]
        S, A = l0._S, l0._A
        xs = [l._as_dev(x).reshape(-1, S) for l, x in zip(self.learners, states)]
        rows = [x.shape[0] for x in xs]
        who = self._who_arrays(who, rows)
        gm = self._gate_max(gate_max, who)
        qt = self._q_inv_temp(q_inv_temp)
        outs = [torch.empty((n, A), dtype=torch.float32, device=l0._dev) for n in rows]
        flags = [torch.empty((n,), dtype=torch.int32, device=l0._dev) for n in rows]
        hs = [torch.empty((n,), dtype=torch.float32, device=l0._dev) if v is not None else None for n, v in zip(rows, self.gates)]
        ptr = lambda ts: [t.data_ptr() if (t is not None and t.shape[0]) else None for t in ts]
        if any(x.shape[0] and x.stride(0) != S for x in xs):
            xs = [x.contiguous() for x in xs]
        if all(c is None for c in self.critics):
            self._call(rows, ptr(xs), ptr(outs), who, gm, ptr(flags), ptr(hs), sample, 0)
            return list(zip(outs, flags, hs))
        qs = [None if c is None else torch.full((n, 4), math.nan, dtype=torch.float32, device=l0._dev)
              for n, c in zip(rows, self.critics)]
        has3 = [w is not None and bool((w == WHO_CRITIC).any()) for w in who]
        self._call(rows, ptr(xs), ptr(outs), who, gm, ptr(flags), ptr(hs), sample, 0, qt,
                   ptr([q if h3 else None for q, h3 in zip(qs, has3)]))
        return [(o, f, h) if q is None else (o, f, h, q) for o, f, h, q in zip(outs, flags, hs, qs)]

    def _gate_values(self, xs):
        """h of every member with a gate and rows, by a handle of the gates alone (the dropout fall-back's first call)."""
        idx = [k for k, x in enumerate(xs) if x is not None and self.gates[k] is not None]
        if not idx:
            return {}
        if self._gate_only is None:
            vs = [_trainer_of(self.gates[k]) for k in range(len(xs)) if self.gates[k] is not None]
            self._gate_only = JsrlActors(vs, vs, vs)
        where = [k for k in range(len(xs)) if self.gates[k] is not None]
        got = self._gate_only.act([xs[k] for k in where], [WHO_GUIDE] * len(where))
        return {k: g[2] for k, g in zip(where, got) if g is not None}

    def _act_separately(self, xs, who, gm):
        """Members with inference dropout (set_act_dropout) are outside the fused call: the gate's values first, then
        each member's learner rows and guide rows by the trainers' own batched forwards."""
        hval = self._gate_values(xs)
        ls, gs, _ = self._members()
        out = []
        for k, x in enumerate(xs):
            if x is None:
                out.append(None)
                continue
            h = hval.get(k)
            use = who[k] == WHO_LEARNER
            if h is not None:
                use = use | ((who[k] == WHO_GATE) & (h <= np.float32(gm[k])))
            acts = np.empty((x.shape[0], ls[k]._A), dtype=np.float32)
            for t, rows_, smp in ((ls[k], np.flatnonzero(use), ls[k].actor.training), (gs[k], np.flatnonzero(~use), False)):
                if rows_.size:
                    a = t.actor_forward(torch.from_numpy(x[rows_]), sample=smp, max_action=float(t.actor.max_action))
                    acts[rows_] = a.cpu().numpy()
            out.append((acts, use.astype(np.int32), h))
        return out


def online_step_jsrl(trainer, jsrl: JsrlActors, replay_buffer, state, action, reward, next_state, done, batch_size: int,
                     act_next, who, gate_max=None):
    """ImplicitQLearning.online_step_jsrl: online_step(...) plus the next action's guide-or-learner selection under one
    synchronisation (iqlhip_jsrl_online_step).  `jsrl` is a JsrlActors of one member whose learner is `trainer`;
    who: 0, 1 or 2 (3, the critic's choice, has no fused form: ValueError); gate_max: the stage the gate's value is
    compared with (who == 2).  Returns (log, action, use_learner, horizon) — horizon None without a gate."""
    import iqlhip_dp as dp
    if len(jsrl.learners) != 1 or jsrl.learners[0] is not trainer:
        raise ValueError("iqlhip: online_step_jsrl needs a JsrlActors of one member whose learner is this trainer")
    if act_next is None:
        raise ValueError("iqlhip: online_step_jsrl selects the next action: act_next is required")
    if jsrl.critics[0] is not None and np.size(who) == 1 and int(np.asarray(who).reshape(-1)[0]) == WHO_CRITIC:
        raise ValueError("iqlhip: online_step_jsrl has no who == 3; call online_step, then JsrlActors.act")
    w = jsrl._who_arrays([who], [1])[0]
    gm = jsrl._gate_max(gate_max, [w])[0]
    self = trainer
    self._prepare(batch_size)
    jsrl._check_members()
    if jsrl._uses_dropout() or self._dp_world > 1:
        # outside the fused call: the iteration, then the selection with the updated learner
        log = self.online_step(replay_buffer, state, action, reward, next_state, done, batch_size)
        a, u, h = jsrl.act([act_next], [w], None if gate_max is None else [gm])[0]
        return log, a[0], int(u[0]), (None if h is None else float(h[0]))
    check_online_ring(replay_buffer, self._dev, "online_step")
    _, gs, _ = jsrl._members()
    gs[0]._prepare_act()                 # (at most sends the guide's inference rate and key: no random stream is consumed)
    flag, h = C.c_int32(0), C.c_float(0.0)
    has_gate = jsrl.gates[0] is not None

    def call(ring_args, row, idx, sc, out, act_args, stream):
        a_in, max_action, seed, a_out = act_args
        return hb.lib().iqlhip_jsrl_online_step(jsrl._handle(), *ring_args, row, idx, batch_size, sc, out, a_in, int(w[0]), gm,
                                                seed, max_action, float(gs[0].actor.max_action), a_out, C.byref(flag),
                                                C.byref(h) if has_gate else None, stream)
    log, a = self._run_online(replay_buffer, (state, action, reward, next_state, done), act_next,
                              lambda new_size: draw_indices(new_size, batch_size), dp.inv_batch(batch_size, self._dp_world),
                              call)
    return log, a, int(flag.value), (float(h.value) if has_gate else None)
