"""What the JSRL critic selection costs (GPU): JsrlActors.act with who == 3 against the composition it replaces and
against the gate form (who == 2), for K members of n states each.

bench.py's single-GPU dims (S=17, A=6, fp32, Gaussian policies in eval mode).  One K per process; the variants' windows
alternate after a warm-up window of each; medians over `--rounds` windows.  `jsrl_q` appears twice (a, b): the spread
between two identical variants is the run-to-run spread to allow.
  jsrl_q_a/b   one JsrlActors.act, who == 3 on every row (argmax);
  composed     per member: guide act, learner act (two host round trips), trainer.score on the hand-built batch of
               [s | a_g] and [s | a_l] rows, the argmax in numpy, the selected rows assembled by hand;
  jsrl_gate    one JsrlActors.act, who == 2 on every row (the variance gate): the launch shape this one extends by two.

    python tools/gpu_jsrl_q_bench.py --K 4 [--iters 1000] [--rounds 7] [--out profiles/jsrl_q_bench.txt]
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

S, A = 17, 6


def make_trainer(seed: int) -> "iql.ImplicitQLearning":
    torch.manual_seed(seed)
    actor = iql.GaussianPolicy(S, A, 1.0).cuda()
    qf, vf = iql.TwinQ(S, A).cuda(), iql.ValueFunction(S).cuda()
    return iql.ImplicitQLearning(max_action=1.0, actor=actor,
                                 actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                 q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                                 v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 iql_tau=0.7, beta=3.0, max_steps=1_000_000, device="cuda")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, required=True, help="members (one K per process)")
    ap.add_argument("--iters", type=int, default=1000, help="calls per window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the JSON line to this file too")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_jsrl_q_bench needs a GPU"
    assert a.rounds >= 5, "medians of at least 5 windows"
    K = a.K
    learners = [make_trainer(10 + k) for k in range(K)]
    guide, gate = make_trainer(1), make_trainer(2)
    for t in learners:
        t.actor.eval()
    jq = iql.JsrlActors(learners, guide, critics=True)
    jg = iql.JsrlActors(learners, guide, gate)
    out = {"tool": "gpu_jsrl_q_bench", "S": S, "A": A, "K": K, "dtype": "f32", "iters": a.iters, "rounds": a.rounds}

    def window(fn, iters) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e6

    for n in (1, 256):
        x = np.random.default_rng(n).standard_normal((n, S)).astype(np.float32)
        xs = [x] * K
        zeros = torch.zeros((2 * n, 1), device="cuda")

        def composed():
            res = []
            for t in learners:
                xd = torch.from_numpy(x).cuda()
                a_g = guide.actor_forward(xd).cpu().numpy()
                a_l = t.actor_forward(xd).cpu().numpy()
                s2 = torch.cat([xd, xd])
                a2 = torch.from_numpy(np.concatenate([a_g, a_l])).cuda()
                cols, _ = t.score([s2, a2, zeros, s2, zeros], summary=False)
                q = cols[:, 2:4].min(dim=1).values.cpu().numpy()
                use = q[n:] >= q[:n]
                res.append((np.where(use[:, None], a_l, a_g), use))
            return res

        fns = {"jsrl_q_a": lambda: jq.act(xs, [3] * K), "composed": composed,
               "jsrl_gate": lambda: jg.act(xs, [2] * K, gate_max=[0.0] * K), "jsrl_q_b": lambda: jq.act(xs, [3] * K)}
        # the fused call and the composition agree on the decision (same fp32 masters; the values differ by rounding)
        got, want = fns["jsrl_q_a"](), composed()
        out[f"n{n}_decisions_equal"] = float(np.mean([np.mean((g[1] != 0) == w[1]) for g, w in zip(got, want)]))
        iters = max(a.iters // (8 if n == 256 else 1), 20)
        for fn in fns.values():
            window(fn, iters)
        ts = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ts[k].append(window(fn, iters))
        for k, v in ts.items():
            out[f"n{n}_us_{k}"] = round(statistics.median(v), 2)
            out[f"n{n}_windows_us_{k}"] = [round(v_, 2) for v_ in v]
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
