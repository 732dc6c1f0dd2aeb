"""What the vector-environment online call costs (GPU): ImplicitQLearning.online_step_vec against the eager sequence it
equals — E add_transition calls, U times train(sample(B)), one actor_forward over E states — at (E, U) in {(1, 1), (8, 1),
(8, 8), (32, 1), (1, 8)}, and at (1, 1) against online_step(act_next=...) as well.

bench.py's single-GPU shapes (S=17, A=6, batch 256, fp32, Gaussian policy in training mode), a ring of 1 M rows.
Identically built trainers, one per side, each with a ring of its own, in one process and on one build; their windows
alternate after a warm-up window of each; medians over `--rounds` windows.  Also: gradient steps per second of
online_step_vec at U = 8 and U = 32 (E = 1, with the act) beside train_steps' (one call of `--steps` steps per window,
losses not returned).  One JSON line; --out writes a readable table as well.

    python tools/gpu_online_vec_bench.py [--iters 300] [--steps 1024] [--rounds 7] [--out profiles/online_vec_bench.txt]
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
POINTS = [(1, 1), (8, 1), (8, 8), (32, 1), (1, 8)]
RING_ROWS = 1_000_000


def make_trainer(seed: int = 0) -> "iql.ImplicitQLearning":
    torch.manual_seed(seed)
    actor = iql.GaussianPolicy(S, A, 1.0).cuda()
    qf, vf = iql.TwinQ(S, A).cuda(), iql.ValueFunction(S).cuda()
    return iql.ImplicitQLearning(max_action=1.0, actor=actor,
                                 actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                 q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                                 v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 iql_tau=0.7, beta=3.0, max_steps=1_000_000, device="cuda")


def ring() -> "iql.ReplayBuffer":
    buf = iql.ReplayBuffer(S, A, RING_ROWS, "cuda")
    buf.fill_synthetic(RING_ROWS // 2, seed=1)
    return buf


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300, help="calls per window")
    ap.add_argument("--steps", type=int, default=1024, help="steps per train_steps window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="write the table and the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_online_vec_bench needs a GPU"
    assert a.rounds >= 5, "medians of at least 5 windows"
    rng = np.random.default_rng(0)
    E_MAX = max(e for e, _ in POINTS)
    s, ns = rng.standard_normal((2, E_MAX, S)).astype(np.float32)
    act = rng.uniform(-1, 1, (E_MAX, A)).astype(np.float32)
    r, d = rng.standard_normal(E_MAX).astype(np.float32), np.zeros(E_MAX, dtype=np.float32)
    ns_dev = torch.from_numpy(ns).cuda()

    def vec_call(t, buf, E, U):
        return lambda: t.online_step_vec(buf, s[:E], act[:E], r[:E], ns[:E], d[:E], B, updates=U, act_next=ns[:E])

    def eager_calls(t, buf, E, U):
        def it():
            for e in range(E):
                buf.add_transition(s[e], act[e], float(r[e]), ns[e], False)
            logs = [t.train(buf.sample(B)) for _ in range(U)]
            return logs, t.actor_forward(ns_dev[:E], sample=t.actor.training).cpu().numpy()
        return it

    def single_call(t, buf):
        return lambda: t.online_step(buf, s[0], act[0], float(r[0]), ns[0], False, B, act_next=ns[0])

    def window(fn, n) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6

    out = {"tool": "gpu_online_vec_bench", "S": S, "A": A, "batch": B, "ring_rows": RING_ROWS, "dtype": "f32",
           "iters": a.iters, "steps": a.steps, "rounds": a.rounds}
    lines = [f"online_step_vec against the eager sequence it equals: S={S} A={A} B={B} fp32, ring of {RING_ROWS} rows",
             f"us per call, medians of {a.rounds} alternating windows of {a.iters} calls (act_next of E states on both sides)",
             f"{'E':>3} {'U':>3} {'vec':>10} {'eager':>10} {'eager/vec':>10} {'online_step':>12}"]
    for E, U in POINTS:
        fns = {"vec": vec_call(make_trainer(), ring(), E, U), "eager": eager_calls(make_trainer(), ring(), E, U)}
        if (E, U) == (1, 1):
            fns["online_step"] = single_call(make_trainer(), ring())
        n = max(20, a.iters // max(1, (E + 3 * U) // 4))          # (the long points take fewer calls per window)
        for fn in fns.values():
            window(fn, n)
        ts = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ts[k].append(window(fn, n))
        med = {k: statistics.median(v) for k, v in ts.items()}
        for k, v in ts.items():
            out[f"E{E}_U{U}_us_per_call_{k}"] = round(med[k], 2)
            out[f"E{E}_U{U}_windows_us_{k}"] = [round(x, 2) for x in v]
        out[f"E{E}_U{U}_eager_over_vec"] = round(med["eager"] / med["vec"], 3)
        single = f"{med['online_step']:12.2f}" if "online_step" in med else f"{'-':>12}"
        lines.append(f"{E:3d} {U:3d} {med['vec']:10.2f} {med['eager']:10.2f} {med['eager'] / med['vec']:10.3f} {single}")
        del fns
        torch.cuda.empty_cache()

    # ---- gradient steps per second: the call at U = 8 and 32 beside a train_steps burst
    lines.append("gradient steps per second (E = 1, with the act; train_steps: one call of --steps steps, no losses)")
    for U in (8, 32):
        fn = vec_call(make_trainer(), ring(), 1, U)
        n = max(10, a.iters // U)
        window(fn, n)
        med = statistics.median(window(fn, n) for _ in range(a.rounds))
        out[f"steps_per_s_vec_U{U}"] = round(U / med * 1e6, 1)
        out[f"us_per_step_vec_U{U}"] = round(med / U, 3)
        lines.append(f"online_step_vec U={U:2d}: {U / med * 1e6:10.1f} steps/s  ({med / U:.2f} us per step)")
    t, buf = make_trainer(), ring()
    t.prepare_train_steps(buf, B)
    burst = lambda: t.train_steps(buf, a.steps, B, seed=1234, return_losses=False)  # noqa: E731
    window(burst, 1)
    med = statistics.median(window(burst, 1) for _ in range(a.rounds))
    out["steps_per_s_train_steps"] = round(a.steps / med * 1e6, 1)
    out["us_per_step_train_steps"] = round(med / a.steps, 3)
    lines.append(f"train_steps          : {a.steps / med * 1e6:10.1f} steps/s  ({med / a.steps:.2f} us per step)")
    line = json.dumps(out)
    print("\n".join(lines))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
