"""Time variance-learner groups (DESIGN.md 6l "Groups of learners") on the GPU at B = 256, S = 17 on a 1 M-row synthetic
buffer: member-updates per second of VarianceLearnerGroup.train_on_buffer for K members against the same K members'
solo train_on_buffer bursts run one after another (the yardstick: same process, the two alternated round by round, every
member on its own seed).  Wall clock, one synchronisation per burst; medians, quartiles and the min .. max spread over
--rounds rounds after one warm-up round.

One process measures one K and appends its lines to --out, so that every GPU step has a time limit of its own and a step
that fails ends the chain:

    rm -f profiles/variance_group_bench.txt && \\
    timeout -k 10 300 python tools/gpu_variance_group_bench.py --k 1 && \\
    timeout -k 10 300 python tools/gpu_variance_group_bench.py --k 2 && \\
    timeout -k 10 300 python tools/gpu_variance_group_bench.py --k 4 && \\
    timeout -k 10 300 python tools/gpu_variance_group_bench.py --k 8 && \\
    timeout -k 10 300 python tools/gpu_variance_group_bench.py --k 16
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "jsrl-corl_amd")]


def stats(ts):
    q = np.percentile(ts, [25, 50, 75])
    return f"median {q[1]:9.1f} us  (quartiles {q[0]:.1f} .. {q[2]:.1f}, min {min(ts):.1f}, max {max(ts):.1f}, n = {len(ts)})", q[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, required=True)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--burst", type=int, default=500)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variance_group_bench.txt"))
    args = ap.parse_args()
    import iql
    import variance_learner as VL
    K, B, S, A = args.k, 256, 17, 6
    lines = []
    if not (args.out and os.path.exists(args.out)):
        lines += [f"variance-learner groups, B = {B}, S = {S}, {args.rows} rows, wall clock; torch {torch.__version__}",
                  f"device: {torch.cuda.get_device_name(0)}",
                  f"per K, rounds alternate: one group burst of {args.burst} updates of K members, then K solo bursts of "
                  f"{args.burst} updates one after another; one warm-up round, {args.rounds} timed; us per MEMBER-update"]
    buf = iql.ReplayBuffer(S, A, args.rows, "cuda")
    buf.fill_synthetic(args.rows, seed=S)
    torch.manual_seed(0)
    members = [VL.VarianceLearner(S, A, None, None, batch_size=B, device="cuda") for _ in range(K)]
    solos = [VL.VarianceLearner(S, A, None, None, batch_size=B, device="cuda") for _ in range(K)]
    group = VL.VarianceLearnerGroup(members)
    seeds = list(range(1, K + 1))
    t_group, t_solo = [], []
    for rnd in range(args.rounds + 1):
        off = rnd * args.burst
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        group.train_on_buffer(buf, args.burst, seeds, off)
        tg = (time.perf_counter() - t0) * 1e6 / (args.burst * K)
        t0 = time.perf_counter()
        for L, s in zip(solos, seeds):
            L.train_on_buffer(buf, args.burst, s, off)
        ts = (time.perf_counter() - t0) * 1e6 / (args.burst * K)
        if rnd > 0:
            t_group.append(tg)
            t_solo.append(ts)
    (txt_g, us_g), (txt_s, us_s) = stats(t_group), stats(t_solo)
    lines.append(f"K={K:2d} group burst, per member-update  {txt_g}")
    lines.append(f"K={K:2d} K solo bursts, per member-update {txt_s}")
    lines.append(f"K={K:2d} member-updates/s: group {1e6 / us_g:9.0f}, solo loop {1e6 / us_s:9.0f}: group {us_s / us_g:.2f} x the solo loop"
                 f"  (a group update of all {K}: {us_g * K:.1f} us)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
