"""What scoring one replay buffer with K trainers costs: one ImplicitQLearningGroup.score_buffer call against K solo
ImplicitQLearning.score_buffer calls, and the group's spread against the solo calls + torch.stack + mean / std.

bench.py's single-GPU shape (S=17, A=6, fp32, Gaussian policy), one shared `--rows`-row buffer.  K = 1, 2, 4, 8; n = 256,
n = 4 096 and the whole buffer.  Per (K, n) four cases: group call; K solo calls; group call with spread=True; K solo
calls, stacked and reduced by torch.  One process; after one warm-up of each the cases alternate, `--runs` timed runs
each (wall time around a device synchronisation); medians, min-max spreads, ratios.  Writes a text table.

    python tools/gpu_group_score_bench.py [--rows 1000000] [--runs 5] [--out profiles/group_score_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jsrl-corl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import iql  # noqa: E402
from gpu_score_bench import A, S, make_trainer  # noqa: E402

KS = (1, 2, 4, 8)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the table to this file too")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_group_score_bench needs a GPU"
    buf = iql.ReplayBuffer(S, A, a.rows, "cuda")
    buf.fill_synthetic(a.rows, seed=0)
    trainers = [make_trainer(i) for i in range(max(KS))]
    for i, t in enumerate(trainers):      # a sweep: the members differ in their hyper-parameters too
        t.beta, t.iql_tau = 3.0 + i, 0.7 + 0.02 * i

    def timed(f) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    lines = [f"gpu_group_score_bench: S={S} A={A} fp32, one shared buffer of {a.rows} rows, {a.runs} timed runs per case "
             "after one warm-up, cases interleaved; microseconds, median [min - max]",
             f"{'K':>2} {'n':>8}  {'group':>26}  {'K solo calls':>26}  {'solo/group':>10}  {'group spread':>26}  "
             f"{'solo + stack + mean/std':>26}  {'torch/group':>11}"]
    for K in KS:
        members = trainers[:K]
        group = iql.ImplicitQLearningGroup(members)
        for n in (256, 4096, a.rows):
            out = torch.empty((K, n, 8), dtype=torch.float32, device="cuda")
            spread = torch.empty((n, 16), dtype=torch.float32, device="cuda")

            def solo():
                return [t.score_buffer(buf, n=n, out=out[k]) for k, t in enumerate(members)]

            def solo_spread():
                solo()
                x = out                      # (the K solo outputs already lie in one [K, n, 8] tensor: the stack is free)
                return torch.cat((x.mean(0), x.std(0, unbiased=False)), dim=1)

            cases = {
                "group": lambda: group.score_buffer(buf, n=n, out=out),
                "solo": solo,
                "group_spread": lambda: group.score_buffer(buf, n=n, out=out, spread=spread),
                "solo_spread": solo_spread,
            }
            for f in cases.values():
                timed(f)
            ts = {k: [] for k in cases}
            for _ in range(a.runs):
                for k, f in cases.items():
                    ts[k].append(timed(f) * 1e6)
            # the two sides computed the same thing
            g_scores, g_sum, _ = group.score_buffer(buf, n=n)
            for k, t in enumerate(members):
                s_scores, s_sum = t.score_buffer(buf, n=n)
                assert torch.equal(g_scores[k], s_scores) and g_sum[k] == s_sum, (K, n, k)
            med = {k: statistics.median(v) for k, v in ts.items()}
            cell = lambda k: f"{med[k]:10.1f} [{min(ts[k]):.1f} - {max(ts[k]):.1f}]"
            lines.append(f"{K:>2} {n:>8}  {cell('group'):>26}  {cell('solo'):>26}  {med['solo'] / med['group']:>10.2f}  "
                         f"{cell('group_spread'):>26}  {cell('solo_spread'):>26}  "
                         f"{med['solo_spread'] / med['group_spread']:>11.2f}")
        del group
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
