"""Weighted replay sampling for K agents (GPU): ImplicitQLearningGroup.train_steps_weighted against the uniform group
call of the same build and against the K solo weighted calls it stands for.

bench.py's single-GPU configuration (S=17, A=6, batch 256, fp32, Gaussian policy), one `--rows`-row buffer shared by
every agent, log-normal weights.  For each K, four sides between identically built sets of agents in one process whose
windows alternate after a warm-up window of each; medians over `--rounds` windows of `--steps` steps, with every window
listed (the spread).  Agent-steps/s of
  shared    group.train_steps_weighted, one table for all members;
  tables    group.train_steps_weighted, a table per member;
  uniform   group.train_steps (the gather the weighted one replaces, in the same launches otherwise);
  solo      K solo train_steps_weighted calls one after another (chunk graphs prepared).
Losses are not returned: one synchronisation a window.  The weighted gather sits between a group's steps, so its whole
cost shows as `gather_us_per_group_step` = (shared - uniform) per step of the group.  One JSON line per K.

    python tools/gpu_group_weighted_bench.py [--ks 1,2,4,8] [--steps 1024] [--rounds 7] [--rows 1000000] [--out FILE]
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
import iqlhip_weighted as wtd  # noqa: E402

S, A, B = 17, 6, 256


def make_trainer(seed: int) -> "iql.ImplicitQLearning":
    torch.manual_seed(seed)
    actor = iql.GaussianPolicy(S, A, 1.0).cuda()
    qf, vf = iql.TwinQ(S, A).cuda(), iql.ValueFunction(S).cuda()
    return iql.ImplicitQLearning(max_action=1.0, actor=actor,
                                 actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                 q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                                 v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 iql_tau=0.7, beta=3.0, max_steps=1_000_000, device="cuda")


def lognormal(n: int, seed: int) -> np.ndarray:
    return np.exp(np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


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
    ap.add_argument("--steps", type=int, default=1024, help="steps per window (one call per side)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1_000_000, help="rows of the shared buffer")
    ap.add_argument("--note", default=None, help="free text copied into every line (e.g. the gather geometry built)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_group_weighted_bench needs a GPU"
    assert a.rounds >= 5, "medians of at least 5 windows"
    buf = iql.ReplayBuffer(S, A, a.rows, "cuda")
    buf.fill_synthetic(a.rows, seed=0)
    buf.set_sample_weights(lognormal(a.rows, 0))
    for K in [int(x) for x in a.ks.split(",")]:
        out = {"tool": "gpu_group_weighted_bench", "K": K, "S": S, "A": A, "batch": B, "rows": a.rows, "dtype": "f32",
               "steps": a.steps, "rounds": a.rounds}
        if a.note:
            out["note"] = a.note
        seeds = list(range(K))
        shared = wtd.SampleWeights(lognormal(a.rows, 0))
        tables = [wtd.SampleWeights(lognormal(a.rows, 10 + k)) for k in range(K)]
        sets = {name: [make_trainer(100 * j + k) for k in range(K)] for j, name in
                enumerate(("shared", "tables", "uniform", "solo"))}
        groups = {name: iql.ImplicitQLearningGroup(sets[name]) for name in ("shared", "tables", "uniform")}
        for t in sets["solo"]:
            t.prepare_train_steps_weighted(buf, B)

        def solo():
            for t, seed in zip(sets["solo"], seeds):
                t.train_steps_weighted(buf, a.steps, B, seed=seed, return_losses=False)

        sides = {
            "shared": lambda: groups["shared"].train_steps_weighted(buf, a.steps, B, seeds, weights=shared, return_losses=False),
            "tables": lambda: groups["tables"].train_steps_weighted(buf, a.steps, B, seeds, weights=tables, return_losses=False),
            "uniform": lambda: groups["uniform"].train_steps(buf, a.steps, B, seeds, return_losses=False),
            "solo": solo,
        }
        ts = alternate(sides, a.rounds)
        med = {k: statistics.median(v) for k, v in ts.items()}
        for k in ts:
            out[f"agent_steps_per_s_{k}"] = round(K * a.steps / med[k], 1)
            out[f"us_per_group_step_{k}"] = round(med[k] / a.steps * 1e6, 3)
            out[f"windows_s_{k}"] = [round(x, 5) for x in ts[k]]
        out["gather_us_per_group_step"] = round((med["shared"] - med["uniform"]) / a.steps * 1e6, 3)
        out["gather_us_per_group_step_tables"] = round((med["tables"] - med["uniform"]) / a.steps * 1e6, 3)
        out["shared_over_uniform"] = round(med["uniform"] / med["shared"], 3)
        out["shared_over_solo"] = round(med["solo"] / med["shared"], 3)
        out["tables_over_solo"] = round(med["solo"] / med["tables"], 3)
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del groups, sets
        torch.cuda.synchronize()
        shared.free()
        for t in tables:
            t.free()


if __name__ == "__main__":
    main()
