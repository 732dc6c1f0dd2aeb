"""Actor dropout inside device policy inference (ImplicitQLearning.set_act_dropout): what the opt-in costs and buys (GPU).

door's dims (S=39, A=28, fp32, Gaussian policy, actor dropout 0.1, training-mode actors).  The two sides of every
measurement alternate in one process; medians over `--rounds` windows of each; one JSON line per measurement:
  act:         actor.act(state, "cuda") — the opted-in device path against the PyTorch fallback (what a trainer that
               has not opted in does), with two device figures of the same build beside them: the same training-mode
               (sampling) call with the dropout layers' rate set to 0, and the eval-mode call (no noise either);
  online:      online_step(..., act_next=s) against online_step(...) + the fallback actor.act(s), and the same two;
  group_act:   group.act(states) at K agents against K opted-in solo act() calls, and the same two for the group;
  group_online: group.online_step(..., act_next=...) against K opted-in solo online_step(act_next=...) calls.

    python tools/gpu_act_dropout_bench.py [--ks 1,4,8] [--parts act,online,group_act,group_online] [--rounds 7]
                                          [--out profiles/r09_act_dropout_bench.jsonl]
    python tools/gpu_act_dropout_bench.py --trace-only      # a K = 4 group act loop alone (kernel-trace runs)
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

S, A, P, B = 39, 28, 0.1, 256


def make_trainer(seed: int, opt_in: bool) -> "iql.ImplicitQLearning":
    torch.manual_seed(seed)
    actor = iql.GaussianPolicy(S, A, 1.0, dropout=P).cuda()
    qf, vf = iql.TwinQ(S, A).cuda(), iql.ValueFunction(S).cuda()
    t = iql.ImplicitQLearning(max_action=1.0, actor=actor,
                              actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                              q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                              v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                              iql_tau=0.8, beta=3.0, max_steps=1_000_000, device="cuda")
    t.set_dropout_seed(seed)
    t.set_act_dropout(opt_in)
    return t


def set_rate(trainers, p: float) -> None:
    """The rate of the actors' dropout layers (0: a training-mode actor samples its noise but drops nothing)."""
    for t in trainers:
        for m in t.actor.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = p


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


class Online:
    """A trainer's online loop on a stand-in stream of transitions (its own ring; batches of B rows)."""

    def __init__(self, seed: int):
        self.buf = iql.ReplayBuffer(S, A, 4096, "cuda")
        self.rng = np.random.default_rng(seed)
        self.s = self.rng.standard_normal(S).astype(np.float32)

    def transition(self):
        s, a = self.s, self.rng.uniform(-1, 1, A).astype(np.float32)
        self.s = ns = self.rng.standard_normal(S).astype(np.float32)
        return s, a, float(self.rng.standard_normal()), ns, False


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,4,8")
    ap.add_argument("--parts", default="act,online,group_act,group_online")
    ap.add_argument("--iters", type=int, default=300, help="calls per window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--trace-only", action="store_true", help="K = 4 group act calls alone, no timing (profiler runs)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_act_dropout_bench needs a GPU"
    assert a.rounds >= 5, "medians of at least 5 windows"
    parts = a.parts.split(",")
    rng = np.random.default_rng(0)
    lines = []

    def report(base: dict, names, ts, per: int) -> None:
        out = dict(base, S=S, A=A, dropout=P, dtype="f32", rounds=a.rounds, iters=per)
        for name, t in zip(names, ts):
            out[f"{name}_us_per_call"] = round(statistics.median(t) / per * 1e6, 2)
            out[f"{name}_window_s"] = [round(x, 5) for x in t]
        out["speedup"] = round(statistics.median(ts[1]) / statistics.median(ts[0]), 3)      # second side over first
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))

    if a.trace_only:
        trainers = [make_trainer(100 + k, True) for k in range(4)]
        group = iql.ImplicitQLearningGroup(trainers, actor_dropout=True)
        states = [rng.standard_normal(S).astype(np.float32) for _ in range(4)]
        for _ in range(20):
            group.act(states)
        torch.cuda.synchronize()
        return

    if "act" in parts:
        dev, fb = make_trainer(1, True), make_trainer(1, False)
        s = rng.standard_normal(S).astype(np.float32)

        def loop(t):
            def fn():
                for _ in range(a.iters):
                    t.actor.act(s, "cuda")
            return fn

        def eval_fn():
            dev.actor.eval()
            for _ in range(a.iters):
                dev.actor.act(s, "cuda")
            dev.actor.train()

        def rate0_fn():
            set_rate([dev], 0.0)
            loop(dev)()
            set_rate([dev], P)

        ts = windows([loop(dev), loop(fb), rate0_fn, eval_fn], a.rounds)
        report({"what": "act"}, ["device_dropout", "torch_fallback", "device_rate0_sampling", "device_eval"], ts, a.iters)

    if "online" in parts:
        dev, fb = make_trainer(2, True), make_trainer(2, False)
        od, of = Online(5), Online(5)
        # (rings start empty: online_step samples with replacement from the rows stored so far, as the loop's first steps do)

        def dev_fn():
            for _ in range(a.iters):
                tr = od.transition()
                dev.online_step(od.buf, *tr, B, act_next=tr[3])

        def fb_fn():
            for _ in range(a.iters):
                tr = of.transition()
                fb.online_step(of.buf, *tr, B)
                fb.actor.act(tr[3], "cuda")

        dev_e, oe = make_trainer(2, True), Online(5)
        dev_e.actor.eval()

        def eval_fn():
            for _ in range(a.iters):
                tr = oe.transition()
                dev_e.online_step(oe.buf, *tr, B, act_next=tr[3])

        dev_0, o0 = make_trainer(2, True), Online(5)
        set_rate([dev_0], 0.0)

        def rate0_fn():
            for _ in range(a.iters):
                tr = o0.transition()
                dev_0.online_step(o0.buf, *tr, B, act_next=tr[3])

        ts = windows([dev_fn, fb_fn, rate0_fn, eval_fn], a.rounds)
        report({"what": "online_step+act", "B": B},
               ["device_dropout", "torch_fallback", "device_rate0_actor", "device_eval_actor"], ts, a.iters)

    for K in [int(x) for x in a.ks.split(",")]:
        if "group_act" in parts:
            members = [make_trainer(100 + k, True) for k in range(K)]
            solos = [make_trainer(100 + k, True) for k in range(K)]
            group = iql.ImplicitQLearningGroup(members, actor_dropout=True)
            states = [rng.standard_normal(S).astype(np.float32) for _ in range(K)]

            def g_fn():
                for _ in range(a.iters):
                    group.act(states)

            def s_fn():
                for _ in range(a.iters):
                    for t, s in zip(solos, states):
                        t.actor.act(s, "cuda")

            def e_fn():
                for t in members:
                    t.actor.eval()
                for _ in range(a.iters):
                    group.act(states)
                for t in members:
                    t.actor.train()

            def r0_fn():
                set_rate(members, 0.0)
                g_fn()
                set_rate(members, P)

            ts = windows([g_fn, s_fn, r0_fn, e_fn], a.rounds)
            report({"what": "group_act", "K": K},
                   ["group_dropout", "solo_seq_dropout", "group_rate0_sampling", "group_eval"], ts, a.iters)
            del group, members, solos
        if "group_online" in parts:
            members = [make_trainer(200 + k, True) for k in range(K)]
            solos = [make_trainer(200 + k, True) for k in range(K)]
            group = iql.ImplicitQLearningGroup(members, actor_dropout=True)
            og, os_ = [Online(300 + k) for k in range(K)], [Online(300 + k) for k in range(K)]
            iters = max(1, a.iters // 2)

            def g_fn():
                for _ in range(iters):
                    trs = [o.transition() for o in og]
                    group.online_step([o.buf for o in og], *[list(x) for x in zip(*trs)], B,
                                      act_next=[tr[3] for tr in trs])

            def s_fn():
                for _ in range(iters):
                    for t, o in zip(solos, os_):
                        tr = o.transition()
                        t.online_step(o.buf, *tr, B, act_next=tr[3])

            ts = windows([g_fn, s_fn], a.rounds)
            report({"what": "group_online_step+act", "K": K, "B": B}, ["group_dropout", "solo_seq_dropout"], ts, iters)
            del group, members, solos
        torch.cuda.synchronize()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
