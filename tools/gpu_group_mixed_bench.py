"""Aggregate agent-steps/s of a trainer group whose members train at different batch sizes (GPU).

Three configurations at configs[1]'s dims (S=17, A=6, fp32) on one shared 1 M-row synthetic replay buffer:

  sweep4    K = 4 at the reference sweep's batch sizes (ray_hyperparam.py: 64, 128, 256, 512), as ONE mixed_batch
            group (group.train_steps) against the same four members stepped solo, one after another, each at its own
            size (trainer.train_steps)
  sweep8    K = 8, every size twice, the same comparison
  control   K = 4 at 256 rows: a plain group (the uniform entry point) against a mixed_batch group (the mixed one)

The two sides of a configuration alternate in the same process.  Each timed window is `--steps` steps per agent, ended
by a device synchronise.  Prints one JSON line per configuration (medians over `--rounds` alternating pairs).

    python tools/gpu_group_mixed_bench.py [--steps 200] [--rounds 5] [--only sweep4,sweep8,control] [--no-solo]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jsrl-corl_amd"))

import torch  # noqa: E402

import iql  # noqa: E402

S, A, N = 17, 6, 1_000_000
SWEEP = [64, 128, 256, 512]


def make_trainer(seed: int) -> "iql.ImplicitQLearning":
    torch.manual_seed(seed)
    actor = iql.GaussianPolicy(S, A, 1.0).cuda()
    qf, vf = iql.TwinQ(S, A).cuda(), iql.ValueFunction(S).cuda()
    return iql.ImplicitQLearning(max_action=1.0, actor=actor,
                                 actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                 q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                                 v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 max_steps=1_000_000, device="cuda")


def timed(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(first, second, rounds: int):
    """Warm both up, then `rounds` alternating timed windows of each (second may be None)."""
    first()
    if second:
        second()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(first))
        if second:
            tb.append(timed(second))
    return ta, tb


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="sweep4,sweep8,control")
    ap.add_argument("--no-solo", action="store_true", help="the mixed group only (profiler runs)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_group_mixed_bench needs a GPU"
    buf = iql.ReplayBuffer(S, A, N, "cuda")
    buf.fill_synthetic(N, seed=1)
    n = a.steps
    only = a.only.split(",")
    for name, sizes in (("sweep4", SWEEP), ("sweep8", SWEEP + SWEEP)):
        if name not in only:
            continue
        K = len(sizes)
        seeds = list(range(K))
        group = iql.ImplicitQLearningGroup([make_trainer(100 + i) for i in range(K)], mixed_batch=True)
        solo = [] if a.no_solo else [make_trainer(200 + i) for i in range(K)]

        def run_group():
            group.train_steps(buf, n, sizes, seeds, return_losses=False)

        def run_solo():
            for i, t in enumerate(solo):
                t.train_steps(buf, n, sizes[i], seed=seeds[i], return_losses=False)

        tg, ts = alternate(run_group, run_solo if solo else None, a.rounds)
        g = statistics.median(tg)
        out = {"config": name, "K": K, "S": S, "A": A, "batch_sizes": sizes, "dtype": "f32", "steps_per_agent": n,
               "rounds": a.rounds, "group_agent_steps_per_s": round(K * n / g, 1),
               "group_us_per_group_step": round(g / n * 1e6, 2), "group_window_s": [round(x, 5) for x in tg]}
        if solo:
            s = statistics.median(ts)
            out.update({"solo_seq_agent_steps_per_s": round(K * n / s, 1),
                        "solo_seq_us_per_agent_step": round(s / (K * n) * 1e6, 2),
                        "solo_window_s": [round(x, 5) for x in ts], "group_over_solo": round(s / g, 3)})
        print(json.dumps(out), flush=True)
        del group, solo
        torch.cuda.synchronize()
    if "control" in only:
        K, B = 4, 256
        seeds = list(range(K))
        uniform = iql.ImplicitQLearningGroup([make_trainer(300 + i) for i in range(K)])
        mixed = iql.ImplicitQLearningGroup([make_trainer(400 + i) for i in range(K)], mixed_batch=True)
        tu, tm = alternate(lambda: uniform.train_steps(buf, n, B, seeds, return_losses=False),
                           lambda: mixed.train_steps(buf, n, [B] * K, seeds, return_losses=False), a.rounds)
        u, m = statistics.median(tu), statistics.median(tm)
        print(json.dumps({"config": "control", "K": K, "S": S, "A": A, "batch_sizes": [B] * K, "dtype": "f32",
                          "steps_per_agent": n, "rounds": a.rounds,
                          "uniform_agent_steps_per_s": round(K * n / u, 1), "mixed_agent_steps_per_s": round(K * n / m, 1),
                          "uniform_window_s": [round(x, 5) for x in tu], "mixed_window_s": [round(x, 5) for x in tm],
                          "mixed_over_uniform": round(u / m, 3)}), flush=True)


if __name__ == "__main__":
    main()
