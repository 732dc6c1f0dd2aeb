"""Policy inference for K agents: one ImplicitQLearningGroup call against K solo calls (GPU).

configs[2]'s dims (S=29, A=8, fp32, Gaussian policy).  Three measurements per K, group and solo windows alternating in
one process, medians over `--rounds` windows of each; one JSON line per (what, K, mode):
  act:           one action per agent — group.act(states) against K actor.act(state, "cuda") calls, in eval mode and in
                 sampling mode (training-mode actors: device noise);
  eval:          eval_actors(envs, actors, ...) against K sequential eval_actor runs, `--episodes` episodes of
                 `--ep-len` steps each, the numpy stand-in env of tools/gpu_online_loop.py (one per agent); the time
                 per lockstep round = one env step of every agent;
  actor_forward: group.actor_forward on `rows` states per agent against K solo actor_forward calls (256 and 4 096).

    python tools/gpu_group_act_bench.py [--ks 1,2,4,8,16] [--parts act,eval,actor_forward] [--rounds 7] [--no-solo]
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

S, A = 29, 8


class SeededToyEnv(ToyEnv):
    """ToyEnv with the gym-style seed() eval_actor calls; every episode runs `ep_len` steps (no goal ends it early, so
    every member's evaluation has the same length and the timings divide by a known step count)."""

    def __init__(self, ep_len: int):
        super().__init__(S, A, seed=0)
        self.ep_len = ep_len

    def seed(self, s):
        self.rng = np.random.default_rng(s)

    def step(self, a):
        s, r, _, info = super().step(a)
        return s, r, self.t >= self.ep_len, info


def make_trainer(seed: int) -> "iql.ImplicitQLearning":
    torch.manual_seed(seed)
    actor = iql.GaussianPolicy(S, A, 1.0).cuda()
    qf, vf = iql.TwinQ(S, A).cuda(), iql.ValueFunction(S).cuda()
    return iql.ImplicitQLearning(max_action=1.0, actor=actor,
                                 actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                 q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                                 v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 iql_tau=0.9, beta=10.0, max_steps=1_000_000, device="cuda")


def timed(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def windows(group_fn, solo_fn, rounds: int):
    group_fn()          # warm-up
    if solo_fn:
        solo_fn()
    tg, ts = [], []
    for _ in range(rounds):
        tg.append(timed(group_fn))
        if solo_fn:
            ts.append(timed(solo_fn))
    return tg, ts


def report(base: dict, tg, ts, per: int, unit: str) -> None:
    g = statistics.median(tg)
    out = dict(base)
    out.update({f"group_{unit}": round(g / per * 1e6, 2), "group_window_s": [round(x, 5) for x in tg]})
    if ts:
        s = statistics.median(ts)
        out.update({f"solo_seq_{unit}": round(s / per * 1e6, 2), "solo_window_s": [round(x, 5) for x in ts],
                    "group_over_solo": round(s / g, 3)})
    print(json.dumps(out), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--parts", default="act,eval,actor_forward")
    ap.add_argument("--iters", type=int, default=300, help="act calls per window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--ep-len", type=int, default=500)
    ap.add_argument("--fwd-iters", type=int, default=50, help="actor_forward calls per window")
    ap.add_argument("--no-solo", action="store_true", help="group only (profiler runs)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_group_act_bench needs a GPU"
    parts = a.parts.split(",")
    rng = np.random.default_rng(0)
    for K in [int(x) for x in a.ks.split(",")]:
        trainers = [make_trainer(100 + k) for k in range(K)]
        group = iql.ImplicitQLearningGroup(trainers)
        actors = [t.actor for t in trainers]
        common = {"K": K, "S": S, "A": A, "dtype": "f32", "rounds": a.rounds}
        if "act" in parts:
            states = [rng.standard_normal(S).astype(np.float32) for _ in range(K)]
            for sample in (False, True):
                for t in trainers:
                    t.actor.train() if sample else t.actor.eval()

                def g_fn():
                    for _ in range(a.iters):
                        group.act(states)

                def s_fn():
                    for _ in range(a.iters):
                        for act, s in zip(actors, states):
                            act.act(s, "cuda")

                tg, ts = windows(g_fn, None if a.no_solo else s_fn, a.rounds)
                report(dict(common, what="act", sample=sample, iters=a.iters), tg, ts, a.iters, "us_per_call")
            for t in trainers:
                t.actor.train()
        if "eval" in parts:
            envs = [SeededToyEnv(a.ep_len) for _ in range(K)]
            seeds = list(range(K))

            def g_fn():
                iql.eval_actors(envs, actors, "cuda", a.episodes, seeds)

            def s_fn():
                for env, act, s in zip(envs, actors, seeds):
                    iql.eval_actor(env, act, "cuda", a.episodes, s)

            rounds = max(1, a.rounds // 2)
            tg, ts = windows(g_fn, None if a.no_solo else s_fn, rounds)
            report(dict(common, rounds=rounds, what="eval", episodes=a.episodes, ep_len=a.ep_len), tg, ts,
                   a.episodes * a.ep_len, "us_per_lockstep_round")
        if "actor_forward" in parts:
            for rows in (256, 4096):
                xs = [torch.from_numpy(rng.standard_normal((rows, S)).astype(np.float32)).cuda() for _ in range(K)]

                def g_fn():
                    for _ in range(a.fwd_iters):
                        group.actor_forward(xs)

                def s_fn():
                    for _ in range(a.fwd_iters):
                        for t, x in zip(trainers, xs):
                            t.actor_forward(x)

                tg, ts = windows(g_fn, None if a.no_solo else s_fn, a.rounds)
                report(dict(common, what="actor_forward", rows=rows, iters=a.fwd_iters), tg, ts, a.fwd_iters,
                       "us_per_call")
        del group, trainers, actors
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
