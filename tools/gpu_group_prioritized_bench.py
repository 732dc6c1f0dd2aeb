"""Prioritised replay and importance-sampling weights in trainer groups (ImplicitQLearningGroup.train_steps_prioritized /
train_steps_weighted(is_beta=); DESIGN.md 6j "trainer groups"): agent-steps/s of the group calls against the same K
members' solo calls run one after another (GPU).

bench.py's workload (S=17, A=6, fp32, batch 256) on a 1 M-row buffer shared by the members, one updatable table per
member.  The two sides alternate in one process, medians over `--rounds` windows of each; one JSON line per kind and K.

    python tools/gpu_group_prioritized_bench.py [--ks 2,4,8] [--rows 1000000] [--steps 1024] [--rounds 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jsrl-corl_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import iql  # noqa: E402
import iqlhip_weighted as wtd  # noqa: E402
from gpu_prioritized_bench import ALPHA, BETA, EPS, A, B, S, make_trainer, spread, windows  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="2,4,8")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=1024, help="steps per member and window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_group_prioritized_bench needs a GPU"
    assert a.rounds >= 5, "medians of at least 5 windows"
    lines = []
    buf = iql.ReplayBuffer(S, A, a.rows, "cuda")
    buf.fill_synthetic(a.rows, seed=0)
    ones = torch.ones(a.rows, device="cuda")
    for K in (int(k) for k in a.ks.split(",")):
        seeds = list(range(7, 7 + K))
        for kind in ("prioritized", "weighted_is"):
            # side 0: the group; side 1: the same members' solo calls one after another (tables and trainers of its own)
            tabs = [[wtd.SampleWeights(ones, updatable=True, max_weight=64.0) for _ in range(K)] for _ in range(2)]
            trs = [[make_trainer(1 + i) for i in range(K)] for _ in range(2)]
            group = iql.ImplicitQLearningGroup(trs[0])
            for t, tab in zip(trs[1], tabs[1]):
                if kind == "prioritized":
                    t.prepare_train_steps_prioritized(buf, B, weights=tab)
                else:
                    t.prepare_train_steps_weighted(buf, B, weights=tab, is_beta=BETA)

            def grouped():
                if kind == "prioritized":
                    group.train_steps_prioritized(buf, a.steps, B, seeds, alpha=ALPHA, eps=EPS, is_beta=BETA, weights=tabs[0],
                                                  return_losses=False)
                else:
                    group.train_steps_weighted(buf, a.steps, B, seeds, weights=tabs[0], is_beta=BETA, return_losses=False)

            def solo():
                for t, tab, seed in zip(trs[1], tabs[1], seeds):
                    if kind == "prioritized":
                        t.train_steps_prioritized(buf, a.steps, B, seed=seed, alpha=ALPHA, eps=EPS, is_beta=BETA, weights=tab,
                                                  return_losses=False)
                    else:
                        t.train_steps_weighted(buf, a.steps, B, seed=seed, weights=tab, is_beta=BETA, return_losses=False)

            tg, ts = windows([grouped, solo], a.rounds)
            g_rate, s_rate = (K * a.steps / statistics.median(t) for t in (tg, ts))
            out = dict(kind=kind, K=K, rows=a.rows, S=S, A=A, batch=B, dtype="f32", rounds=a.rounds, steps_per_window=a.steps,
                       alpha=ALPHA, eps=EPS, is_beta=BETA, group_agent_steps_per_s=round(g_rate, 1),
                       solo_agent_steps_per_s=round(s_rate, 1), group_over_solo=round(g_rate / s_rate, 3),
                       group_spread=spread(tg), solo_spread=spread(ts), group_window_s=[round(x, 5) for x in tg],
                       solo_window_s=[round(x, 5) for x in ts], flags=[t.flags() for t in tabs[0]])
            print(json.dumps(out), flush=True)
            lines.append(json.dumps(out))
            del group, trs
            for t in tabs[0] + tabs[1]:
                t.free()
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
