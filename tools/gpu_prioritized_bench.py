"""Prioritised replay inside the chunk graphs (train_steps_prioritized): what the in-graph table update costs a
step, and what the burst gains over the eager prioritised loop (GPU).

bench.py's workload (S=17, A=6, fp32, batch 256).  The sides of every measurement alternate in one process, medians over
`--rounds` windows of each; one JSON line per measurement and table size:
  steps: us/step of train_steps_prioritized against train_steps_weighted(..., is_beta=) on an updatable table of the same
         weights (the difference is the three update launches per step).
  loop:  us/iteration of the eager prioritised loop — draw with is_beta, gather, train(loss_weights, return_td), refresh —
         old form (torch (max |td| + eps) ** alpha, then update_sample_weights) and new form (update_sample_weights_td).

    python tools/gpu_prioritized_bench.py [--rows 1000000,10000000] [--steps 4096] [--rounds 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "jsrl-corl_amd")
sys.path.insert(0, PKG)

import torch  # noqa: E402

import iql  # noqa: E402

S, A, B = 17, 6, 256
ALPHA, EPS, BETA = 0.6, 1e-3, 0.5


def make_trainer(seed: int):
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


def spread(t):
    return round((max(t) - min(t)) / statistics.median(t), 4)


def make_buffer(rows: int):
    buf = iql.ReplayBuffer(S, A, rows, "cuda")
    buf.fill_synthetic(rows, seed=0)
    buf.set_sample_weights(torch.ones(rows, device="cuda"), updatable=True, max_weight=64.0)
    return buf


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--steps", type=int, default=4096, help="steps per window of the burst sides")
    ap.add_argument("--loop-iters", type=int, default=20, help="iterations per window of the eager loops")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parts", default="steps,loop")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_prioritized_bench needs a GPU"
    assert a.rounds >= 5, "medians of at least 5 windows"
    parts = a.parts.split(",")
    lines = []

    def report(out: dict) -> None:
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))

    for rows in (int(r) for r in a.rows.split(",")):
        base = dict(rows=rows, S=S, A=A, batch=B, dtype="f32", rounds=a.rounds, alpha=ALPHA, eps=EPS, is_beta=BETA)

        # ---- (a) us/step: the prioritised burst against the weighted burst with is_beta
        if "steps" in parts:
            bufs = [make_buffer(rows), make_buffer(rows)]
            trs = [make_trainer(1), make_trainer(1)]
            trs[0].prepare_train_steps_prioritized(bufs[0], B)
            trs[1].prepare_train_steps_weighted(bufs[1], B, is_beta=BETA)

            def prioritized():
                trs[0].train_steps_prioritized(bufs[0], a.steps, B, seed=7, alpha=ALPHA, eps=EPS, is_beta=BETA,
                                               return_losses=False)

            def weighted_is():
                trs[1].train_steps_weighted(bufs[1], a.steps, B, seed=7, is_beta=BETA, return_losses=False)

            tp, tw = windows([prioritized, weighted_is], a.rounds)
            p_us, w_us = (statistics.median(t) / a.steps * 1e6 for t in (tp, tw))
            report(dict(base, part="steps", steps_per_window=a.steps, prioritized_us_per_step=round(p_us, 3),
                        weighted_is_us_per_step=round(w_us, 3), update_nodes_us_per_step=round(p_us - w_us, 3),
                        prioritized_spread=spread(tp), weighted_is_spread=spread(tw),
                        prioritized_window_s=[round(x, 5) for x in tp], weighted_is_window_s=[round(x, 5) for x in tw],
                        flags=bufs[0].sample_weights_flags()))
            for buf in bufs:
                buf.set_sample_weights(None)
            del bufs, trs

        # ---- (b) the eager prioritised loop: torch pow + update_sample_weights against update_sample_weights_td
        if "loop" in parts:
            bufs = [make_buffer(rows), make_buffer(rows)]
            trs = [make_trainer(4), make_trainer(4)]
            it = [0, 0]

            def iteration(k):
                buf, tr = bufs[k], trs[k]
                idx, c = buf.draw_weighted_indices(B, 7, it[k] * (B // 2), is_beta=BETA)
                it[k] += 1
                tr.train(buf.gather(idx), loss_weights=c, return_td=True)
                td = tr.last_td_errors()
                if k == 0:
                    buf.update_sample_weights(idx, (td.abs().amax(dim=1) + EPS) ** ALPHA)
                else:
                    buf.update_sample_weights_td(idx, td, ALPHA, EPS)

            def loop(k):
                return lambda: [iteration(k) for _ in range(a.loop_iters)]

            to, tn = windows([loop(0), loop(1)], a.rounds)
            report(dict(base, part="loop", iters_per_window=a.loop_iters,
                        torch_pow_us_per_iteration=round(statistics.median(to) / a.loop_iters * 1e6, 1),
                        update_td_us_per_iteration=round(statistics.median(tn) / a.loop_iters * 1e6, 1),
                        torch_pow_window_s=[round(x, 5) for x in to], update_td_window_s=[round(x, 5) for x in tn],
                        flags=[buf.sample_weights_flags() for buf in bufs]))
            for buf in bufs:
                buf.set_sample_weights(None)
            del bufs, trs
        torch.cuda.empty_cache()

    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
