"""Per-row loss weights (trainer.train(batch, loss_weights=c, return_td=True)): what the row-weighted backward costs an
eager step, what the draw with is_beta costs, and what the prioritised loop gains from last_td_errors() (GPU).

bench.py's workload (S=17, A=6, fp32, batch 256, 1 M rows).  The sides of every measurement alternate in one process,
medians over `--rounds` windows of each; one JSON line per measurement:
  step:  train(batch) against train(batch, loss_weights=c) and train(batch, loss_weights=c, return_td=True) on one
         gathered batch, us per call (each call ends on the host read of its losses).
  steps: train_steps_weighted(buffer, --steps, B) against the same call with is_beta=0.5 (the row-weighted backward and
         the idle blocks' q staging and c inside the chunk graphs), us per step, on two trainers after prepare.
  draw:  draw_weighted_indices(B, ...) against draw_weighted_indices(B, ..., is_beta=0.5), us per call.
  loop:  one iteration of the prioritised eager loop — draw with is_beta, gather, weighted train with
         return_td, update_sample_weights(idx, (|td| + eps) ** alpha) — against the loop it replaces: plain draw, train,
         score(batch), the TD error from the score columns, update.

    python tools/gpu_loss_weights_bench.py [--rows 1000000] [--iters 200] [--steps 4096] [--rounds 7] [--out FILE]
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

S, A, B = 17, 6, 256


def make_trainer(seed: int):
    torch.manual_seed(seed)
    actor, qf, vf = iql.GaussianPolicy(S, A, 1.0).cuda(), iql.TwinQ(S, A).cuda(), iql.ValueFunction(S).cuda()
    return iql.ImplicitQLearning(max_action=1.0, actor=actor, actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
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


def report(out, what, names, ts, per):
    rec = {"bench": what}
    for n, t in zip(names, ts):
        rec[n + "_us"] = round(statistics.median(t) / per * 1e6, 2)
        rec[n + "_spread"] = round((max(t) - min(t)) / statistics.median(t), 4)
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=200, help="calls per window")
    ap.add_argument("--steps", type=int, default=4096, help="steps per window of the train_steps_weighted sides")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_loss_weights_bench needs a GPU"
    assert a.rounds >= 5, "medians of at least 5 windows"
    import iqlhip_binding as hb
    buf = iql.ReplayBuffer(S, A, a.rows, "cuda")
    buf.fill_synthetic(a.rows, seed=0)
    w = torch.rand(a.rows, device="cuda") ** 4 + 1e-3
    buf.set_sample_weights(w, updatable=True, max_weight=64.0)
    tr = make_trainer(0)
    idx, c = buf.draw_weighted_indices(B, 3, 0, is_beta=0.5)
    batch = buf.gather(idx)
    n = a.iters

    report(a.out, "step", ["plain", "weighted", "weighted_td"], windows([
        lambda: [tr.train(batch) for _ in range(n)],
        lambda: [tr.train(batch, loss_weights=c) for _ in range(n)],
        lambda: [tr.train(batch, loss_weights=c, return_td=True) for _ in range(n)]], a.rounds), n)

    tp, ti = make_trainer(1), make_trainer(1)
    tp.prepare_train_steps_weighted(buf, B)
    ti.prepare_train_steps_weighted(buf, B, is_beta=0.5)
    report(a.out, "steps", ["plain", "is_beta"], windows([
        lambda: tp.train_steps_weighted(buf, a.steps, B, seed=7, return_losses=False),
        lambda: ti.train_steps_weighted(buf, a.steps, B, seed=7, return_losses=False, is_beta=0.5)], a.rounds), a.steps)

    report(a.out, "draw", ["plain", "is_beta"], windows([
        lambda: [buf.draw_weighted_indices(B, 3, k) for k in range(n)],
        lambda: [buf.draw_weighted_indices(B, 3, k, is_beta=0.5) for k in range(n)]], a.rounds), n)

    alpha, eps, disc = 0.6, 1e-3, 0.99
    nxt, q1 = hb.SCORE_NAMES.index("next_v"), hb.SCORE_NAMES.index("q1")

    def loop_td():
        for k in range(n):
            i, cw = buf.draw_weighted_indices(B, 5, k * (B // 2), is_beta=0.5)
            tr.train(buf.gather(i), loss_weights=cw, return_td=True)
            buf.update_sample_weights(i, (tr.last_td_errors()[:, 0].abs() + eps) ** alpha)

    def loop_score():
        for k in range(n):
            i = buf.draw_weighted_indices(B, 5, k * (B // 2))
            bt = buf.gather(i)
            tr.train(bt)
            sc, _ = tr.score(bt, summary=False)
            td = bt[2][:, 0] + (1.0 - bt[4][:, 0]) * disc * sc[:, nxt] - sc[:, q1]
            buf.update_sample_weights(i, (td.abs() + eps) ** alpha)

    report(a.out, "loop", ["last_td_errors", "score"], windows([loop_td, loop_score], a.rounds), n)


if __name__ == "__main__":
    main()
