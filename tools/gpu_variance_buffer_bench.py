"""Time the variance learner trained from a replay buffer (DESIGN.md 6l "From a replay buffer") on the GPU, at B = 256 for
S = 17 and 29 on a 1 M-row synthetic buffer: microseconds per update of train_on_buffer (bursts of --burst updates, one
synchronisation per burst), per update_from_buffer call, and per _update_v call on the same windows downloaded to host
tensors (the yardstick: same process, the three alternated round by round).  Wall clock, medians and quartiles over
--rounds rounds (bursts) and --rounds * --calls calls, after one warm-up round.

    python tools/gpu_variance_buffer_bench.py [--rounds 9] [--burst 1000] [--calls 40] [--out profiles/variance_buffer_bench.txt]
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
    return f"median {q[1]:9.1f} us  (quartiles {q[0]:.1f} .. {q[2]:.1f}, min {min(ts):.1f}, n = {len(ts)})", q[1]


def host_window(rows, start, B, S, A):
    """The window as run_episodes hands a rollout over: lists with one entry per row, states as float32 tensors."""
    w = rows[start:start + B].cpu()
    return ([r.clone() for r in w[:, :S]], [None] * B, [float(x) for x in w[:, 2 * S + A]], [False] * B,
            [r.clone() for r in w[:, S + A:2 * S + A]], [bool(x) for x in w[:, 2 * S + A + 1]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--burst", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variance_buffer_bench.txt"))
    args = ap.parse_args()
    import iql
    import variance_learner as VL
    B, A = 256, 6
    lines = [f"variance learner from a replay buffer, B = {B}, {args.rows} rows, wall clock; torch {torch.__version__}",
             f"device: {torch.cuda.get_device_name(0)}",
             f"rounds alternate: one burst of {args.burst} updates, {args.calls} update_from_buffer calls, {args.calls} _update_v calls "
             f"on the same windows as host tensors; one warm-up round, {args.rounds} timed"]
    for S in (17, 29):
        buf = iql.ReplayBuffer(S, A, args.rows, "cuda")
        buf.fill_synthetic(args.rows, seed=S)
        L = VL.VarianceLearner(S, A, None, None, batch_size=B, device="cuda")
        starts = np.random.RandomState(S).randint(0, args.rows - B + 1, size=args.calls)
        windows = [host_window(buf._rows, int(s), B, S, A) for s in starts]
        t_burst, t_win, t_host = [], [], []
        for rnd in range(args.rounds + 1):
            keep = rnd > 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            L.train_on_buffer(buf, args.burst, seed=S, offset=rnd * args.burst)
            dt = (time.perf_counter() - t0) * 1e6 / args.burst
            if keep:
                t_burst.append(dt)
            for s in starts:
                t0 = time.perf_counter()
                L.update_from_buffer(buf, int(s), False)
                if keep:
                    t_win.append((time.perf_counter() - t0) * 1e6)
            for w in windows:
                t0 = time.perf_counter()
                L._update_v(w, False)
                if keep:
                    t_host.append((time.perf_counter() - t0) * 1e6)
        (txt_b, us_b), (txt_w, us_w), (txt_h, us_h) = stats(t_burst), stats(t_win), stats(t_host)
        lines.append(f"S={S:3d} train_on_buffer, per update      {txt_b}")
        lines.append(f"S={S:3d} update_from_buffer, per call      {txt_w}")
        lines.append(f"S={S:3d} _update_v (host tensors), per call {txt_h}")
        lines.append(f"S={S:3d} per update against _update_v: burst {us_h / us_b:.1f} x faster ({us_h - us_b:.1f} us less), "
                     f"update_from_buffer {us_h / us_w:.1f} x faster ({us_h - us_w:.1f} us less)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
