"""N-step rows on the device: what the build, the ring refresh and the fused online call cost (GPU).

  build     NStepReplay.rebuild of a 1 M-row and a 10 M-row device buffer at configs[1]'s dims (S=17, A=6), filled in
            place with fill_synthetic(p_done=0.001); horizons 3 and 10, with and without the ep_last column of
            episode_returns(1000, 0.99, keep_tail=True); one launch, reads and writes every row once
  host      what a caller had to do before: download the rows, tests/nstep_ref.py's loop, upload — at --host-rows rows
            (the restatement is a Python loop of ~10 us per row: the 10 M-row buffer is not waited for), horizon 3
  ring      iqlhip_rows_nstep_ring alone on a full 10 000-row ring: enqueue cost per call over 2 000 calls, one
            synchronise at the end
  online    per iteration on a full 10 000-row ring at B = 256: trainer.online_step_nstep, the eager sequence it equals
            (nstep.add_transition, nstep.buffer.sample, train) and the plain online_step on a raw ring; windows of
            --iters iterations alternate, medians over --repeats windows

Every window ends in a device synchronise; window 0 of each side is its warm-up.  Prints one JSON line per part.

    python tools/gpu_nstep_bench.py [--rows 1000000,10000000] [--host-rows 1000000] [--repeats 7] [--iters 300]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "jsrl-corl_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import iql  # noqa: E402
import iqlhip_binding as hb  # noqa: E402

S, A, DISCOUNT, B, RING = 17, 6, 0.99, 256, 10_000


def timed(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def med(times):
    return {"s": statistics.median(times), "min_s": min(times), "max_s": max(times)}


def build_part(n, repeats, host_rows):
    buf = iql.ReplayBuffer(S, A, n, "cuda")
    buf.fill_synthetic(n, seed=1, p_done=0.001)
    episodes = buf.episode_returns(1000, DISCOUNT, keep_tail=True)
    out = {"part": "build", "rows": n, "state_dim": S, "action_dim": A, "repeats": repeats,
           "bytes_read_and_written": 2 * n * buf._ld * 4}
    sides = {}
    for N in (3, 10):
        ns = buf.nstep(N, DISCOUNT)
        sides[f"n{N}"] = (lambda ns=ns: ns.rebuild())
        sides[f"n{N}_ep_last"] = (lambda ns=ns: ns.rebuild(episodes))
    times = {k: [] for k in sides}
    for rep in range(repeats + 1):
        for name, fn in sides.items():
            t = timed(fn)
            if rep:
                times[name].append(t)
    for k, v in times.items():
        out[k] = med(v)
        out[k]["GB_per_s"] = out["bytes_read_and_written"] / out[k]["s"] / 1e9
    if n == host_rows:
        import nstep_ref
        ns = buf.nstep(3, DISCOUNT)
        t0 = time.perf_counter()
        rows = buf._rows[:n].cpu().numpy()
        t1 = time.perf_counter()
        want, steps = nstep_ref.build(rows, S, A, 3, DISCOUNT)
        t2 = time.perf_counter()
        up = torch.from_numpy(want).cuda()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        out["host_n3"] = {"download_s": t1 - t0, "nstep_ref_s": t2 - t1, "upload_s": t3 - t2, "s": t3 - t0}
        out["host_over_device_n3"] = out["host_n3"]["s"] / out["n3"]["s"]
        out["host_equals_device_bitwise"] = bool(torch.equal(up.view(torch.int32), ns.buffer._rows[:n].view(torch.int32)))
    print(json.dumps(out), flush=True)


def full_ring(N):
    raw = iql.ReplayBuffer(S, A, RING, "cuda")
    raw.fill_synthetic(RING, seed=2, p_done=0.01)
    raw._pointer = 0                       # a ring that has just wrapped: the oldest row at position 0
    return raw, raw.nstep(N, DISCOUNT)


def ring_part(calls):
    out = {"part": "ring", "ring_rows": RING, "calls": calls}
    for N in (3, 10):
        raw, ns = full_ring(N)
        lib, stream = hb.lib(), raw._stream()
        args = (raw._rows.data_ptr(), ns.buffer._rows.data_ptr(), raw._ld, S, A, RING, RING)

        def window():
            for i in range(calls):
                lib.iqlhip_rows_nstep_ring(*args, i % RING, ns.ends.data_ptr(), N, DISCOUNT, ns.steps.data_ptr(), stream)

        timed(window)
        out[f"n{N}_us_per_call"] = statistics.median(timed(window) for _ in range(5)) / calls * 1e6
    print(json.dumps(out), flush=True)


def trainer():
    qf, vf, actor = iql.TwinQ(S, A).cuda(), iql.ValueFunction(S).cuda(), iql.GaussianPolicy(S, A, 1.0).cuda()
    return iql.ImplicitQLearning(1.0, actor, torch.optim.Adam(actor.parameters(), lr=3e-4), qf,
                                 torch.optim.Adam(qf.parameters(), lr=3e-4), vf, torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 max_steps=1000000, discount=DISCOUNT, device="cuda")


def online_part(iters, repeats):
    rng = np.random.default_rng(0)
    s, a, s2 = (rng.standard_normal(S).astype(np.float32), rng.uniform(-1, 1, A).astype(np.float32),
                rng.standard_normal(S).astype(np.float32))
    out = {"part": "online", "ring_rows": RING, "batch": B, "iters_per_window": iters, "repeats": repeats}
    for N in (3, 10):
        (_, ns_f), (_, ns_e), (raw_p, _) = full_ring(N), full_ring(N), full_ring(N)
        tr_f, tr_e, tr_p = trainer(), trainer(), trainer()

        def fused():
            for i in range(iters):
                tr_f.online_step_nstep(ns_f, s, a, 0.5, s2, False, B, episode_end=(i % 50 == 49))

        def eager():
            for i in range(iters):
                ns_e.add_transition(s, a, 0.5, s2, False, episode_end=(i % 50 == 49))
                tr_e.train(ns_e.buffer.sample(B))

        def plain():
            for i in range(iters):
                tr_p.online_step(raw_p, s, a, 0.5, s2, False, B)

        sides = {"fused": fused, "eager": eager, "plain_online_step": plain}
        times = {k: [] for k in sides}
        for rep in range(repeats + 1):
            for name, fn in sides.items():
                t = timed(fn)
                if rep:
                    times[name].append(t / iters * 1e6)
        for k, v in times.items():
            out[f"n{N}_{k}_us_per_iter"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        out[f"n{N}_eager_over_fused"] = out[f"n{N}_eager_us_per_iter"]["median"] / out[f"n{N}_fused_us_per_iter"]["median"]
        out[f"n{N}_fused_over_plain"] = out[f"n{N}_fused_us_per_iter"]["median"] / out[f"n{N}_plain_online_step_us_per_iter"]["median"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--host-rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--ring-calls", type=int, default=2000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    for n in (int(x) for x in args.rows.split(",")):
        build_part(n, args.repeats, args.host_rows)
        torch.cuda.empty_cache()
    ring_part(args.ring_calls)
    online_part(args.iters, args.repeats)


if __name__ == "__main__":
    main()
