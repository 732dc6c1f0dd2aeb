"""The prioritised online iteration (trainer.online_step_prioritized; DESIGN.md 6j "Online prioritised replay"): what one
library call costs against the eager sequence it equals and against the plain online_step (GPU).

bench.py's workload (S=17, A=6, fp32, batch 256) on a ring of `rows` rows, all but 8 192 filled, whose table tracks its maximum.  The three
sides alternate in one process, medians over `--rounds` windows of each; one JSON line per table size:
  online_step_prioritized   the one call
  eager                     add_transition (ring write + insert at the maximum) -> draw_weighted_indices(is_beta) ->
                            gather -> train(loss_weights, return_td) -> update_sample_weights_td -> actor.act
  online_step               the plain one-call iteration (uniform host draw, no table)
every side with act_next, the policy in eval mode.  A second line: the stand-alone insert_max launch, timed over a
window of back-to-back launches, next to a three-launch update of one row.

    python tools/gpu_online_prio_bench.py [--rows 1000000,10000000] [--iters 200] [--rounds 7] [--out FILE]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

import iql  # noqa: E402

S, A, B = 17, 6, 256
ALPHA, EPS, BETA, SEED = 0.6, 1e-3, 0.4, 7
HEADROOM = 8192


def make_trainer(seed: int):
    torch.manual_seed(seed)
    actor, qf, vf = iql.GaussianPolicy(S, A, 1.0).cuda(), iql.TwinQ(S, A).cuda(), iql.ValueFunction(S).cuda()
    tr = iql.ImplicitQLearning(max_action=1.0, actor=actor,
                               actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                               q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                               v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                               iql_tau=0.7, beta=3.0, max_steps=1_000_000, discount=0.99, tau=0.005, device="cuda")
    tr.actor.eval()
    return tr


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


def make_buffer(rows: int, track: bool):
    """A ring of `rows` rows, all but HEADROOM filled: the measured iterations append (none wraps)."""
    buf = iql.ReplayBuffer(S, A, rows, "cuda")
    buf.fill_synthetic(rows - HEADROOM, seed=0)
    if track:
        buf.set_sample_weights(torch.ones(rows - HEADROOM, device="cuda"), updatable=True, max_weight=64.0, track_max=True,
                               new_row_weight=1.0)
    return buf


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--iters", type=int, default=200, help="iterations per window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_online_prio_bench needs a GPU"
    assert a.rounds >= 5, "medians of at least 5 windows"
    assert (a.rounds + 1) * a.iters <= HEADROOM, "the windows' iterations must fit the ring's free rows"
    lines = []

    def report(out: dict) -> None:
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))

    rng = np.random.default_rng(0)
    s, s2 = rng.standard_normal(S).astype(np.float32), rng.standard_normal(S).astype(np.float32)
    act = rng.uniform(-1, 1, A).astype(np.float32)
    for rows in (int(r) for r in a.rows.split(",")):
        bufs = [make_buffer(rows, True), make_buffer(rows, True), make_buffer(rows, False)]
        trs = [make_trainer(4) for _ in range(3)]
        it = [0]

        def one_call():
            for _ in range(a.iters):
                trs[0].online_step_prioritized(bufs[0], s, act, 1.0, s2, False, B, SEED, alpha=ALPHA, eps=EPS, is_beta=BETA,
                                               act_next=s2)

        def eager():
            buf, tr = bufs[1], trs[1]
            for _ in range(a.iters):
                buf.add_transition(s, act, 1.0, s2, False)
                idx, c = buf.draw_weighted_indices(B, SEED, it[0] * (B // 2), is_beta=BETA, batch_size=B)
                it[0] += 1
                tr.train(buf.gather(idx), loss_weights=c, return_td=True)
                buf.update_sample_weights_td(idx, tr.last_td_errors(), ALPHA, EPS)
                tr.actor.act(s2, "cuda")

        def plain():
            for _ in range(a.iters):
                trs[2].online_step(bufs[2], s, act, 1.0, s2, False, B, act_next=s2)

        to, te, tp = windows([one_call, eager, plain], a.rounds)
        us = [statistics.median(t) / a.iters * 1e6 for t in (to, te, tp)]
        report(dict(rows=rows, S=S, A=A, batch=B, dtype="f32", rounds=a.rounds, iters_per_window=a.iters, part="iteration",
                    online_step_prioritized_us=round(us[0], 1), eager_us=round(us[1], 1), online_step_us=round(us[2], 1),
                    gap_to_online_step_us=round(us[0] - us[2], 1), gain_over_eager_us=round(us[1] - us[0], 1),
                    prioritized_window_s=[round(x, 5) for x in to], eager_window_s=[round(x, 5) for x in te],
                    online_step_window_s=[round(x, 5) for x in tp], flags=[bufs[0].sample_weights_flags(),
                                                                          bufs[1].sample_weights_flags()]))

        # ---- the stand-alone insert_max launch next to a three-launch update of one row (back to back on the stream)
        n_launch = 2000
        idx1 = torch.tensor([5], device="cuda")
        w1 = torch.tensor([0.5], device="cuda")

        def inserts():
            for k in range(n_launch):
                bufs[0].insert_max_sample_weight(k)

        def updates():
            for _ in range(n_launch):
                bufs[0].update_sample_weights(idx1, w1)

        ti, tu = windows([inserts, updates], a.rounds)
        report(dict(rows=rows, part="insert_max", launches_per_window=n_launch, rounds=a.rounds,
                    insert_max_us=round(statistics.median(ti) / n_launch * 1e6, 2),
                    update_one_row_us=round(statistics.median(tu) / n_launch * 1e6, 2)))
        for buf in bufs[:2]:
            buf.set_sample_weights(None)
        del bufs, trs
        torch.cuda.empty_cache()

    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
