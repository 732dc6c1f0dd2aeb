"""What the JSRL guide-or-learner selection costs (GPU): ImplicitQLearning.online_step_jsrl and JsrlActors.act against
the same work composed from the calls that existed before them.

bench.py's single-GPU configuration (S=17, A=6, batch 256, fp32, Gaussian policy).  Identically built trainers, one set
per side, in one process; the sides' windows alternate after a warm-up window of each; medians over `--rounds` windows.
`fused_act_next` appears twice (a, b): the spread between two identical variants is the run-to-run spread to allow.
  online   us per online iteration, for who = 0 (guide), 1 (learner), 2 (the gate decides):
             composed   online_step without act_next, then guide.actor.act or learner.actor.act — chosen on the host,
                        for who = 2 after a torch forward of the gate network on the host (the reference's config.vf);
             jsrl       online_step_jsrl;
             fused_act_next_a/b   online_step(act_next=...): the learner's action only (the lower bound);
  act      us per JsrlActors.act of K = 1, 4, 8 members (one state each, who = 2) against the K x 3 solo calls it
           replaces (learner.actor.act, guide.actor.act and the gate's torch forward on the host).

    python tools/gpu_jsrl_bench.py [--iters 2000] [--rounds 9] [--out profiles/jsrl_act_bench.txt]
"""
import argparse
import copy
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
    buf = iql.ReplayBuffer(S, A, 100_000, "cuda")
    buf.fill_synthetic(1000, seed=1)
    return buf


def host_gate(gate):
    """The gate network as the reference holds it: a torch module on the host, evaluated per environment step."""
    vf = copy.deepcopy(gate.vf).cpu()
    return lambda s: float(vf(torch.Tensor(s)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000, help="iterations per window")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None, help="append the JSON line to this file too")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_jsrl_bench needs a GPU"
    assert a.rounds >= 5, "medians of at least 5 windows"
    rng = np.random.default_rng(0)
    s, ns = rng.standard_normal((2, S)).astype(np.float32)
    act = rng.uniform(-1, 1, A).astype(np.float32)
    guide, gate = make_trainer(1), make_trainer(2)
    vf_host = host_gate(gate)

    def window(fn) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.iters * 1e6

    def race(fns) -> dict:
        for fn in fns.values():
            window(fn)
        ts = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ts[k].append(window(fn))
        return ts

    out = {"tool": "gpu_jsrl_bench", "S": S, "A": A, "batch": B, "dtype": "f32", "iters": a.iters, "rounds": a.rounds}

    def composed(t, on, who):
        def it():
            log = t.online_step(on, s, act, 0.5, ns, False, B)
            use = who == 1 or (who == 2 and vf_host(ns) <= 0.0)
            return log, (t if use else guide).actor.act(ns, "cuda")
        return it

    def fused(t, on, who):
        j = iql.JsrlActors(t, guide, gate)
        return lambda: t.online_step_jsrl(j, on, s, act, 0.5, ns, False, B, ns, who, gate_max=0.0)

    def act_next(t, on):
        return lambda: t.online_step(on, s, act, 0.5, ns, False, B, act_next=ns)

    for who in (0, 1, 2):
        fns = {"composed": composed(make_trainer(), ring(), who), "jsrl": fused(make_trainer(), ring(), who),
               "fused_act_next_a": act_next(make_trainer(), ring()), "fused_act_next_b": act_next(make_trainer(), ring())}
        for k, v in race(fns).items():
            out[f"online_who{who}_us_{k}"] = round(statistics.median(v), 2)
            out[f"online_who{who}_windows_us_{k}"] = [round(x, 2) for x in v]

    for K in (1, 4, 8):
        learners = [make_trainer(10 + k) for k in range(K)]
        j = iql.JsrlActors(learners, guide, gate)
        states, who = [ns] * K, [2] * K

        def solo():
            for t in learners:
                vf_host(ns)
                t.actor.act(ns, "cuda")
                guide.actor.act(ns, "cuda")

        fns = {"jsrl_a": lambda: j.act(states, who, gate_max=[0.0] * K), "solo_calls": solo,
               "jsrl_b": lambda: j.act(states, who, gate_max=[0.0] * K)}
        for k, v in race(fns).items():
            out[f"act_K{K}_us_{k}"] = round(statistics.median(v), 2)
            out[f"act_K{K}_windows_us_{k}"] = [round(x, 2) for x in v]
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
