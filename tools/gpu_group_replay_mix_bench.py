"""Batches mixed from an offline and an online buffer for K agents (GPU): the trainer groups' replay-mix calls against
the K solo mixed calls they stand for.

bench.py's single-GPU configuration (S=17, A=6, batch 256, fp32, Gaussian policy), mixing_ratio 0.5, one offline
buffer shared by every agent and one online ring per agent.  For each K, two comparisons, each between identically
built sets of agents in one process whose windows alternate after a warm-up window of each; medians over `--rounds`
windows, with every window listed (the spread):
  online   iterations/s of one ImplicitQLearningGroup.online_step_replay_mix call per iteration against K solo
           online_step_mixed calls one after another (the same fixed transition every iteration: nothing but the
           calls is timed);
  steps    agent-steps/s of one train_steps_replay_mix call of `--steps` steps against K solo train_steps_mixed calls
           of as many steps one after another (chunk graphs prepared; losses not returned, one synchronisation a window).
One JSON line per K.

    python tools/gpu_group_replay_mix_bench.py [--ks 1,2,4,8] [--iters 1000] [--steps 1024] [--rounds 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jsrl-corl_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import iql  # noqa: E402

S, A, B, RATIO = 17, 6, 256, 0.5


def make_trainer(seed: int) -> "iql.ImplicitQLearning":
    torch.manual_seed(seed)
    actor = iql.GaussianPolicy(S, A, 1.0).cuda()
    qf, vf = iql.TwinQ(S, A).cuda(), iql.ValueFunction(S).cuda()
    return iql.ImplicitQLearning(max_action=1.0, actor=actor,
                                 actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                 q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                                 v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 iql_tau=0.7, beta=3.0, max_steps=1_000_000, device="cuda")


def rings(K: int, rows: int, cap: int):
    out = []
    for k in range(K):
        buf = iql.ReplayBuffer(S, A, cap, "cuda")
        buf.fill_synthetic(rows, seed=1 + k)
        out.append(buf)
    return out


def window(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(sides, rounds: int):
    """Warm up each side once, then `rounds` windows of each in turn; seconds per window, per side."""
    for fn in sides.values():
        window(fn)
    ts = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ts[k].append(window(fn))
    return ts


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--iters", type=int, default=1000, help="online iterations per window")
    ap.add_argument("--steps", type=int, default=1024, help="steps per window (one burst per agent)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1_000_000, help="offline rows")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_group_replay_mix_bench needs a GPU"
    assert a.rounds >= 5, "medians of at least 5 windows"
    off = iql.ReplayBuffer(S, A, a.rows, "cuda")
    off.fill_synthetic(a.rows, seed=0)
    rng = np.random.default_rng(0)
    s, ns = rng.standard_normal((2, S)).astype(np.float32)
    act = rng.uniform(-1, 1, A).astype(np.float32)
    np.random.seed(0)
    for K in [int(x) for x in a.ks.split(",")]:
        out = {"tool": "gpu_group_replay_mix_bench", "K": K, "S": S, "A": A, "batch": B, "mixing_ratio": RATIO,
               "dtype": "f32", "iters": a.iters, "steps": a.steps, "rounds": a.rounds}
        seeds = list(range(K))

        # ---- one online iteration of every agent
        g_tr, s_tr = [make_trainer(100 + k) for k in range(K)], [make_trainer(200 + k) for k in range(K)]
        g_on, s_on = rings(K, 1000, 100_000), rings(K, 1000, 100_000)
        group = iql.ImplicitQLearningGroup(g_tr)
        per = ([s] * K, [act] * K, [0.5] * K, [ns] * K, [False] * K)

        def group_iters():
            for _ in range(a.iters):
                group.online_step_replay_mix(off, g_on, *per, B, RATIO)

        def solo_iters():
            for _ in range(a.iters):
                for t, on in zip(s_tr, s_on):
                    t.online_step_mixed(off, on, s, act, 0.5, ns, False, B, RATIO)

        ts = alternate({"group": group_iters, "solo": solo_iters}, a.rounds)
        med = {k: statistics.median(v) for k, v in ts.items()}
        for k in ts:
            out[f"online_iters_per_s_{k}"] = round(a.iters / med[k], 1)
            out[f"online_us_per_iter_{k}"] = round(med[k] / a.iters * 1e6, 2)
            out[f"online_windows_us_{k}"] = [round(x / a.iters * 1e6, 2) for x in ts[k]]
        out["online_group_over_solo"] = round(med["solo"] / med["group"], 3)

        # ---- bursts of steps (fresh online buffers: only read from here on)
        b_on = rings(K, 50_000, 100_000)
        for t, on in zip(s_tr, b_on):
            t.prepare_train_steps_mixed(off, on, B, RATIO)

        def group_burst():
            group.train_steps_replay_mix(off, b_on, a.steps, B, seeds, RATIO, return_losses=False)

        def solo_bursts():
            for t, on, seed in zip(s_tr, b_on, seeds):
                t.train_steps_mixed(off, on, a.steps, B, RATIO, seed=seed, return_losses=False)

        ts = alternate({"group": group_burst, "solo": solo_bursts}, a.rounds)
        med = {k: statistics.median(v) for k, v in ts.items()}
        for k in ts:
            out[f"steps_agent_steps_per_s_{k}"] = round(K * a.steps / med[k], 1)
            out[f"steps_us_per_agent_step_{k}"] = round(med[k] / (K * a.steps) * 1e6, 3)
            out[f"steps_windows_s_{k}"] = [round(x, 5) for x in ts[k]]
        out["steps_group_over_solo"] = round(med["solo"] / med["group"], 3)
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del group, g_tr, s_tr, g_on, s_on, b_on
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
