"""Updatable weight tables (SampleWeights(..., updatable=True) / iqlhip_weights_update): what an in-place update costs
against a rebuild, what the second table layout costs the weighted step, and what a prioritised loop gains (GPU).

bench.py's workload (S=17, A=6, fp32, batch 256).  The sides of every measurement alternate in one process, medians over
`--rounds` windows of each; one JSON line per measurement:
  update: SampleWeights.update of 256 and of 4 096 rows (random rows, with replacement) on a table of 1 M and of 10 M rows,
          against a rebuild of the same table (SampleWeights(w, updatable=True): validation, node scans, two host
          synchronisations).  An update window is --update-calls calls and one synchronise.
  steps:  train_steps_weighted us/step on a static table and on an updatable table of the same weights; with
          --parent-tree DIR (a built checkout of the parent commit) also on a static table with the parent's library and
          package, loaded next to this one's, its windows alternating with the other two.
  loop:   one iteration of the prioritised eager loop — draw_weighted_indices, gather, train, score,
          update_sample_weights(idx, (|td| + eps) ** alpha) — against the same loop with set_sample_weights (a rebuild of
          the static table from a full weight vector) in the update's place.

    python tools/gpu_weighted_update_bench.py [--rows 1000000,10000000] [--steps 4096] [--rounds 7]
                                              [--parent-tree DIR] [--out FILE]
"""
import argparse
import glob
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "jsrl-corl_amd")
sys.path.insert(0, PKG)

import numpy as np  # noqa: E402,F401
import torch  # noqa: E402

import iql  # noqa: E402
import iqlhip_weighted as wtd  # noqa: E402

S, A, B = 17, 6, 256


def package_modules(pkg_dir: str) -> dict:
    """The package under pkg_dir imported as a module set of its own (its modules find each other by name in
    sys.modules, so a side is entered by putting its set there: enter())."""
    names = [os.path.basename(p)[:-3] for p in glob.glob(os.path.join(pkg_dir, "*.py"))]
    saved = {k: sys.modules.pop(k) for k in names if k in sys.modules}
    sys.path.insert(0, pkg_dir)
    try:
        for k in names:
            try:
                importlib.import_module(k)
            except Exception:       # (a module with an optional dependency: not needed here)
                pass
        mods = {k: sys.modules.pop(k) for k in names if k in sys.modules}
    finally:
        sys.path.remove(pkg_dir)
        sys.modules.update(saved)
    return mods


def enter(mods: dict) -> None:
    sys.modules.update(mods)


def make_trainer(pkg, seed: int):
    torch.manual_seed(seed)
    actor, qf, vf = pkg.GaussianPolicy(S, A, 1.0).cuda(), pkg.TwinQ(S, A).cuda(), pkg.ValueFunction(S).cuda()
    return pkg.ImplicitQLearning(max_action=1.0, actor=actor,
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--steps", type=int, default=4096, help="steps per window of the train_steps sides")
    ap.add_argument("--update-calls", type=int, default=50, help="update calls per window")
    ap.add_argument("--loop-iters", type=int, default=20, help="iterations per window of the prioritised loop")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (steps part)")
    ap.add_argument("--parts", default="update,steps,loop")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpu_weighted_update_bench needs a GPU"
    assert a.rounds >= 5, "medians of at least 5 windows"
    parts = a.parts.split(",")
    lines = []
    for p in glob.glob(os.path.join(PKG, "*.py")):     # (every module now: a later lazy import must not find the other side's)
        try:
            importlib.import_module(os.path.basename(p)[:-3])
        except Exception:
            pass
    this_mods = {k: m for k, m in list(sys.modules.items())
                 if getattr(m, "__file__", None) and os.path.dirname(os.path.abspath(m.__file__)) == PKG}
    parent = None
    if a.parent_tree:
        parent_mods = package_modules(os.path.join(os.path.abspath(a.parent_tree), "jsrl-corl_amd"))
        parent = parent_mods["iql"]
        assert os.path.dirname(parent.__file__) != PKG

    def report(out: dict) -> None:
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))

    for rows in (int(r) for r in a.rows.split(",")):
        g = torch.Generator(device="cuda").manual_seed(1)
        lognormal = torch.exp(torch.randn(rows, device="cuda", generator=g))
        wmax = float(lognormal.max()) * 4.0
        base = dict(rows=rows, S=S, A=A, batch=B, dtype="f32", rounds=a.rounds)

        # ---- (a) update against rebuild
        if "update" in parts:
            tab = wtd.SampleWeights(lognormal, updatable=True, max_weight=wmax)
            holder = [None]

            def rebuild():
                holder[0] = None        # (free first: two 10 M-row tables need not coexist)
                holder[0] = wtd.SampleWeights(lognormal, updatable=True, max_weight=wmax)

            for m in (256, 4096):
                idx = torch.randint(0, rows, (m,), device="cuda", generator=g)
                w_new = torch.exp(torch.randn(m, device="cuda", generator=g))

                def update():
                    for _ in range(a.update_calls):
                        tab.update(idx, w_new)

                tu, tb = windows([update, rebuild], a.rounds)
                report(dict(base, part="update", m=m, calls_per_window=a.update_calls,
                            update_us=round(statistics.median(tu) / a.update_calls * 1e6, 2),
                            rebuild_us=round(statistics.median(tb) * 1e6, 1),
                            update_window_s=[round(x, 6) for x in tu], rebuild_window_s=[round(x, 6) for x in tb],
                            table_bytes=8 * sum(_level_sizes(rows)) + 4 * rows))
            assert tab.flags() == 0
            holder[0] = None
            del tab

        # ---- (b) us/step: a static and an updatable table of the same weights (and the parent's static table)
        if "steps" in parts:
            names, sides, keep = [], [], []
            if parent is not None:
                enter(parent_mods)
                pbuf = parent.ReplayBuffer(S, A, rows, "cuda")
                pbuf.fill_synthetic(rows, seed=0)
                pbuf.set_sample_weights(lognormal)
                ptr = make_trainer(parent, 1)
                ptr.prepare_train_steps_weighted(pbuf, B)

                def parent_side():
                    enter(parent_mods)
                    ptr.train_steps_weighted(pbuf, a.steps, B, seed=7, return_losses=False)

                names.append("parent_static")
                sides.append(parent_side)
                keep += [pbuf, ptr]
                enter(this_mods)
            for name, kw in (("static", {}), ("updatable", dict(updatable=True))):
                buf = iql.ReplayBuffer(S, A, rows, "cuda")
                buf.fill_synthetic(rows, seed=0)
                buf.set_sample_weights(lognormal, **kw)
                tr = make_trainer(iql, 1)
                tr.prepare_train_steps_weighted(buf, B)

                def side(tr=tr, buf=buf):
                    enter(this_mods)
                    tr.train_steps_weighted(buf, a.steps, B, seed=7, return_losses=False)

                names.append(name)
                sides.append(side)
                keep += [buf, tr]
            ts = windows(sides, a.rounds)
            out = dict(base, part="steps", steps_per_window=a.steps)
            for name, t in zip(names, ts):
                out[f"{name}_us_per_step"] = round(statistics.median(t) / a.steps * 1e6, 3)
                out[f"{name}_spread"] = spread(t)
                out[f"{name}_window_s"] = [round(x, 5) for x in t]
            report(out)
            for b_ in keep[::2]:
                b_.set_sample_weights(None)
            del keep, sides
            enter(this_mods)

        # ---- (c) the prioritised eager loop: update in place against a rebuild per iteration
        if "loop" in parts:
            eps, alpha = 1e-3, 0.6
            bufs = [iql.ReplayBuffer(S, A, rows, "cuda") for _ in range(2)]
            for buf in bufs:
                buf.fill_synthetic(rows, seed=0)
            prio = torch.ones(rows, device="cuda")
            bufs[0].set_sample_weights(prio, updatable=True, max_weight=64.0)
            bufs[1].set_sample_weights(prio)
            trs = [make_trainer(iql, 4), make_trainer(iql, 4)]
            full = prio.clone()
            it = [0, 0]

            def iteration(k):
                buf, tr = bufs[k], trs[k]
                idx = buf.draw_weighted_indices(B, 7, it[k] * (B // 2))
                it[k] += 1
                batch = buf.gather(idx)
                tr.train(batch)
                sc, _ = tr.score(batch, summary=False)
                s_, a_, r_, ns_, d_ = batch
                td = r_[:, 0] + (1.0 - d_[:, 0]) * 0.99 * sc[:, 1] - sc[:, 2]
                p = (td.abs() + eps) ** alpha
                if k == 0:
                    buf.update_sample_weights(idx, p)
                else:
                    full[idx] = p
                    buf.set_sample_weights(full)

            def loop(k):
                return lambda: [iteration(k) for _ in range(a.loop_iters)]

            tu, tb = windows([loop(0), loop(1)], a.rounds)
            report(dict(base, part="loop", iters_per_window=a.loop_iters,
                        update_us_per_iteration=round(statistics.median(tu) / a.loop_iters * 1e6, 1),
                        rebuild_us_per_iteration=round(statistics.median(tb) / a.loop_iters * 1e6, 1),
                        update_window_s=[round(x, 5) for x in tu], rebuild_window_s=[round(x, 5) for x in tb],
                        flags=bufs[0].sample_weights_flags()))
            for buf in bufs:
                buf.set_sample_weights(None)
            del bufs, trs, prio, full
        del lognormal
        torch.cuda.empty_cache()

    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def _level_sizes(n: int):
    sizes = [n]
    while sizes[-1] > 64:
        sizes.append((sizes[-1] + 63) // 64)
    return [(s + 63) // 64 * 64 for s in sizes]


if __name__ == "__main__":
    main()
