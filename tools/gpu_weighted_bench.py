"""Weighted replay sampling (ImplicitQLearning.train_steps_weighted): what it costs against plain train_steps and what it
replaces (GPU).

bench.py's workload (S=17, A=6, fp32, batch 256) on a buffer of 1 M and of 10 M rows.  The sides of every measurement
alternate in one process, medians over `--rounds` windows of each; one JSON line per measurement:
  steps:  steps/s of train_steps (plain) against train_steps_weighted with equal and with log-normal weights — windows
          of --steps steps, every chunk graph prepared and warmed up beforehand;
  build:  set_sample_weights(device tensor) — validation, scan and levels, with its two host synchronisations;
  host:   the loop the device sampler replaces, per iteration: np.random.choice(n, B, p=w / w.sum()) on the host, the
          index upload and gather, and an eager train().

    python tools/gpu_weighted_bench.py [--rows 1000000,10000000] [--steps 4096] [--rounds 7] [--out FILE]
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

S, A, B = 17, 6, 256


def make_trainer(seed: int) -> "iql.ImplicitQLearning":
    torch.manual_seed(seed)
    actor, qf, vf = iql.GaussianPolicy(S, A, 1.0).cuda(), iql.TwinQ(S, A).cuda(), iql.ValueFunction(S).cuda()
    return iql.ImplicitQLearning(max_action=1.0, actor=actor,
                                 actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                 q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                                 v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 iql_tau=0.7, beta=3.0, max_steps=1_000_000, discount=0.99, tau=0.005, device="cuda")


def timed(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def windows(fns, rounds: int):
    """Alternate the sides' windows `rounds` times after one warm-up window of each; the windows of every side."""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            ts[i].append(timed(fn))
    return ts


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--steps", type=int, default=4096, help="steps per window of the train_steps sides")
    ap.add_argument("--host-iters", type=int, default=20, help="iterations per window of the host loop")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_weighted_bench needs a GPU"
    assert a.rounds >= 5, "medians of at least 5 windows"
    lines = []

    def report(out: dict) -> None:
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))

    for rows in (int(r) for r in a.rows.split(",")):
        plain, equal, skewed = (iql.ReplayBuffer(S, A, rows, "cuda") for _ in range(3))
        for buf in (plain, equal, skewed):
            buf.fill_synthetic(rows, seed=0)
        g = torch.Generator(device="cuda").manual_seed(1)
        lognormal = torch.exp(torch.randn(rows, device="cuda", generator=g))
        equal.set_sample_weights(torch.ones(rows, device="cuda"))
        skewed.set_sample_weights(lognormal)
        base = dict(rows=rows, S=S, A=A, batch=B, dtype="f32", rounds=a.rounds)

        # ---- steps/s: three trainers, one per side (each keeps its own chunk graphs and its own stream position)
        trs = [make_trainer(s) for s in (1, 2, 3)]
        trs[0].prepare_train_steps(plain, B)
        trs[1].prepare_train_steps_weighted(equal, B)
        trs[2].prepare_train_steps_weighted(skewed, B)
        sides = [lambda: trs[0].train_steps(plain, a.steps, B, seed=7, return_losses=False),
                 lambda: trs[1].train_steps_weighted(equal, a.steps, B, seed=7, return_losses=False),
                 lambda: trs[2].train_steps_weighted(skewed, a.steps, B, seed=7, return_losses=False)]
        ts = windows(sides, a.rounds)
        out = dict(base, part="steps", steps_per_window=a.steps)
        for name, t in zip(("plain", "weighted_equal", "weighted_lognormal"), ts):
            out[f"{name}_steps_per_s"] = round(a.steps / statistics.median(t), 1)
            out[f"{name}_us_per_step"] = round(statistics.median(t) / a.steps * 1e6, 3)
            out[f"{name}_window_s"] = [round(x, 5) for x in t]
        report(out)

        # ---- table build
        t = windows([lambda: skewed.set_sample_weights(lognormal)], a.rounds)[0]
        report(dict(base, part="build", build_ms=round(statistics.median(t) * 1e3, 3), window_s=[round(x, 5) for x in t],
                    table_bytes=8 * sum(_level_sizes(rows))))

        # ---- the host loop it replaces
        w_host = lognormal.cpu().numpy().astype(np.float64)
        p = w_host / w_host.sum()
        tr = make_trainer(4)
        parts = {"choice": 0.0, "gather": 0.0, "train": 0.0}

        def host_loop():
            for _ in range(a.host_iters):
                t0 = time.perf_counter()
                idx = np.random.choice(rows, B, p=p)
                t1 = time.perf_counter()
                batch = plain.gather(torch.from_numpy(idx))
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                tr.train(batch)
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                parts["choice"] += t1 - t0
                parts["gather"] += t2 - t1
                parts["train"] += t3 - t2

        host_loop()
        for k in parts:
            parts[k] = 0.0
        t = windows([host_loop], a.rounds)[0]
        n_it = a.host_iters * (a.rounds + 1)            # (windows' own warm-up window included in `parts`)
        report(dict(base, part="host", iters_per_window=a.host_iters,
                    host_us_per_iteration=round(statistics.median(t) / a.host_iters * 1e6, 1),
                    choice_us=round(parts["choice"] / n_it * 1e6, 1), gather_us=round(parts["gather"] / n_it * 1e6, 1),
                    train_us=round(parts["train"] / n_it * 1e6, 1), window_s=[round(x, 5) for x in t]))
        for buf in (equal, skewed):
            buf.set_sample_weights(None)
        del plain, equal, skewed, trs, tr, lognormal
        torch.cuda.empty_cache()

    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def _level_sizes(n: int):
    sizes = [n]
    while sizes[-1] > 64:
        sizes.append((sizes[-1] + 63) // 64)
    return [(s + 63) // 64 * 64 for s in sizes]


if __name__ == "__main__":
    main()
