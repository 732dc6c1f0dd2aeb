"""Iterations/s of the online loop for K agents: one ImplicitQLearningGroup.online_step per iteration against the K
solo ImplicitQLearning.online_step calls one after another (GPU).

configs[2]'s dims (S=29, A=8, B=256, fp32), one 10 k-row ring per agent, the numpy stand-in environment of
tools/gpu_online_loop.py (one per agent).  An iteration is env.step for every agent plus the online call(s):
  --act:    the fused loop — the next action rides in the call (act_next = the next state; an agent whose episode ended
            acts through actor.act on its reset state), as tools/gpu_online_loop.py's fused mode does;
  no --act: uniform random actions, nothing but the online step on the GPU.
Group and solo windows of `--iters` iterations alternate in one process; the medians over `--rounds` windows of each
are reported, one JSON line per (K, act).

    python tools/gpu_group_online_bench.py [--ks 1,2,4,8] [--iters 300] [--rounds 7] [--modes 0,1] [--no-solo]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "jsrl-corl_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import iql  # noqa: E402
from gpu_online_loop import ToyEnv  # noqa: E402

S, A, B, RING = 29, 8, 256, 10_000


def make_trainer(seed: int) -> "iql.ImplicitQLearning":
    torch.manual_seed(seed)
    actor = iql.GaussianPolicy(S, A, 1.0).cuda()
    qf, vf = iql.TwinQ(S, A).cuda(), iql.ValueFunction(S).cuda()
    return iql.ImplicitQLearning(max_action=1.0, actor=actor,
                                 actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                 q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                                 v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 iql_tau=0.9, beta=10.0, max_steps=1_000_000, device="cuda")


class Agents:
    """K trainers, their rings, their environments and the loop state (state, next action) of each."""

    def __init__(self, K: int, seed0: int):
        self.trainers = [make_trainer(seed0 + k) for k in range(K)]
        self.bufs = [iql.ReplayBuffer(S, A, RING, "cuda") for _ in range(K)]
        self.envs = [ToyEnv(S, A, seed=seed0 + k) for k in range(K)]
        self.rng = np.random.default_rng(seed0)
        self.states = [e.reset() for e in self.envs]
        for buf, env, k in zip(self.bufs, self.envs, range(K)):      # enough rows to sample from
            s = self.states[k]
            for _ in range(B):
                a = self.rng.uniform(-1, 1, A).astype(np.float32)
                ns, r, d, _ = env.step(a)
                buf.add_transition(s, a, r, ns, d)
                s = env.reset() if d else ns
            self.states[k] = s
        self.next_a = [None] * K

    def actions(self, act: bool):
        if not act:
            return [self.rng.uniform(-1, 1, A).astype(np.float32) for _ in self.trainers]
        return [a if a is not None else t.actor.act(s, "cuda")
                for a, t, s in zip(self.next_a, self.trainers, self.states)]

    def env_steps(self, acts):
        return [env.step(a) for env, a in zip(self.envs, acts)]

    def advance(self, outs, next_a):
        self.next_a = next_a
        self.states = [env.reset() if o[2] else o[0] for env, o in zip(self.envs, outs)]


def group_iters(ag: Agents, group, n: int, act: bool) -> None:
    K = len(ag.trainers)
    for _ in range(n):
        acts = ag.actions(act)
        outs = ag.env_steps(acts)
        an = [None if o[2] else o[0] for o in outs] if act else None
        res = group.online_step(ag.bufs, ag.states, acts, [o[1] for o in outs], [o[0] for o in outs],
                                [o[2] for o in outs], B, act_next=an)
        ag.advance(outs, res[1] if act else [None] * K)


def solo_iters(ag: Agents, n: int, act: bool) -> None:
    K = len(ag.trainers)
    for _ in range(n):
        acts = ag.actions(act)
        outs = ag.env_steps(acts)
        nxt = [None] * K
        for k, (t, buf, s, a, o) in enumerate(zip(ag.trainers, ag.bufs, ag.states, acts, outs)):
            if act and not o[2]:
                _, nxt[k] = t.online_step(buf, s, a, o[1], o[0], o[2], B, act_next=o[0])
            else:
                t.online_step(buf, s, a, o[1], o[0], o[2], B)
        ag.advance(outs, nxt)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--modes", default="0,1", help="act_next off (0) / on (1)")
    ap.add_argument("--no-solo", action="store_true", help="group only (profiler runs)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_group_online_bench needs a GPU"
    np.random.seed(0)
    n = a.iters
    for K in [int(x) for x in a.ks.split(",")]:
        g_ag = Agents(K, 100)
        group = iql.ImplicitQLearningGroup(g_ag.trainers)
        s_ag = None if a.no_solo else Agents(K, 200)
        for act in [bool(int(m)) for m in a.modes.split(",")]:
            def timed(fn) -> float:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            group_iters(g_ag, group, 20, act)           # warm-up
            if s_ag:
                solo_iters(s_ag, 20, act)
            tg, ts = [], []
            for _ in range(a.rounds):
                tg.append(timed(lambda: group_iters(g_ag, group, n, act)))
                if s_ag:
                    ts.append(timed(lambda: solo_iters(s_ag, n, act)))
            g = statistics.median(tg)
            out = {"K": K, "act_next": act, "S": S, "A": A, "B": B, "ring": RING, "dtype": "f32", "iters": n,
                   "rounds": a.rounds, "group_iters_per_s": round(n / g, 1),
                   "group_agent_iters_per_s": round(K * n / g, 1), "group_us_per_iter": round(g / n * 1e6, 2),
                   "group_window_s": [round(x, 5) for x in tg]}
            if s_ag:
                s = statistics.median(ts)
                out.update({"solo_seq_iters_per_s": round(n / s, 1), "solo_seq_agent_iters_per_s": round(K * n / s, 1),
                            "solo_seq_us_per_iter": round(s / n * 1e6, 2), "solo_window_s": [round(x, 5) for x in ts],
                            "group_over_solo": round(s / g, 3)})
            print(json.dumps(out), flush=True)
        del group, g_ag, s_ag
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
