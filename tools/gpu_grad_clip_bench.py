"""What gradient-norm clipping (ImplicitQLearning.set_grad_clip) costs per step (GPU).

bench.py's single-GPU configuration (S=17, A=6, batch 256, fp32, Gaussian policy): steps/s of train_steps with clipping
on against clipping off, with the per-step statistics off and on (they share the gradient block partials with the clip
kernel).  Four identically built trainers, one per setting, share one buffer and one process; their windows of
`--steps` steps (one train_steps call each, losses not returned) alternate, after prepare_train_steps and one warm-up
window of each; medians over `--rounds` windows.  The limits are far below the norms: every group is clipped on every
step (the arithmetic is the same either way).  One JSON line.

    python tools/gpu_grad_clip_bench.py [--steps 1024] [--rounds 9] [--rows 1000000] [--out profiles/grad_clip_bench.jsonl]
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
MAX_NORM = 1e-3


def make_trainer(seed: int, stats: bool, clip: bool) -> "iql.ImplicitQLearning":
    torch.manual_seed(seed)
    actor = iql.GaussianPolicy(S, A, 1.0).cuda()
    qf, vf = iql.TwinQ(S, A).cuda(), iql.ValueFunction(S).cuda()
    t = iql.ImplicitQLearning(max_action=1.0, actor=actor,
                              actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                              q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                              v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                              iql_tau=0.7, beta=3.0, max_steps=1_000_000, device="cuda")
    t.set_step_stats(stats)
    t.set_grad_clip(MAX_NORM if clip else None)
    return t


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1024, help="steps per window (one train_steps call)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=None, help="append the JSON line to this file too")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_grad_clip_bench needs a GPU"
    assert a.rounds >= 5, "medians of at least 5 windows"
    buf = iql.ReplayBuffer(S, A, a.rows, "cuda")
    buf.fill_synthetic(a.rows, seed=0)
    sides = {f"stats_{'on' if st else 'off'}_clip_{'on' if cl else 'off'}": make_trainer(0, st, cl)
             for st in (False, True) for cl in (False, True)}
    for t in sides.values():
        t.prepare_train_steps(buf, B)

    def window(t) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t.train_steps(buf, a.steps, B, seed=1234, return_losses=False)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for t in sides.values():
        window(t)
    ts = {k: [] for k in sides}
    for _ in range(a.rounds):
        for k, t in sides.items():
            ts[k].append(window(t))
    for k, t in sides.items():
        if k.endswith("clip_on"):
            c = t.last_grad_clip()
            assert all(0.0 < c["coef_" + g] < 1.0 for g in ("vf", "qf", "actor")), c
    med = {k: statistics.median(v) for k, v in ts.items()}
    out = {"tool": "gpu_grad_clip_bench", "S": S, "A": A, "batch": B, "dtype": "f32", "steps": a.steps, "rounds": a.rounds}
    for k in sides:
        out["steps_per_s_" + k] = round(a.steps / med[k], 1)
        out["us_per_step_" + k] = round(med[k] / a.steps * 1e6, 3)
    for st in ("stats_off", "stats_on"):
        on, off = med[st + "_clip_on"], med[st + "_clip_off"]
        out["clip_cost_us_per_step_" + st] = round((on - off) / a.steps * 1e6, 3)
        out["clip_on_over_off_" + st] = round(on / off, 4)
    out["window_s"] = {k: [round(x, 5) for x in v] for k, v in ts.items()}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
