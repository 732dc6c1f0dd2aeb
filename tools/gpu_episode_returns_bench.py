"""Per-row episode returns and return-to-go of a replay buffer that lives on the GPU: the device call against the host
round trip it replaces (GPU).

A 1 M-row and a 10 M-row device buffer at configs[1]'s dims (S=17, A=6), filled in place with
fill_synthetic(p_done=0.001) and made continuous (s[i+1] = s'[i]) so that the state-discontinuity rule finds the same
episodes as the done column; max_episode_steps = 1000, discount 0.99:

  device        buffer.episode_returns(T, discount): break flags, prefix-max scan, one thread per episode walking its
                rewards forward and backward in float64, row-parallel spans; four [n] device arrays
  device_rule   the same with state_break_tol=1e-6 (every row reads its 2 S state floats)
  range         buffer.return_reward_range(T) on the same rows: the yardstick (one ordered pass, three scalars out)
  host          what a caller had to do before: download the reward and done columns, the restatement's loop in numpy —
                breaks, spans vectorised; the two ordered recurrences advanced one row per step for all episodes at once,
                which keeps every rounding where the definition puts it — and upload of the four arrays
  host_rule     the same with the s and s' columns downloaded and the rule evaluated in numpy

Every window ends in a device synchronise; the three device sides alternate in one process after a warm-up of each, then
the two host sides do (a device window right behind a host window of seconds would measure an idle GPU waking up);
medians over `--repeats` windows (`--host-repeats` for the host sides).  The host results are compared with the device's bit for bit
once, outside the timed windows.  Prints one JSON line per size.

    python tools/gpu_episode_returns_bench.py [--rows 1000000,10000000] [--repeats 7] [--host-repeats 3] [--device-only]
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

S, A, T, DISCOUNT, TOL = 17, 6, 1000, 0.99, 1e-6


def timed(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def host_episode_returns(r, d, s, ns, tol):
    """The definition of include/iqlhip.h in numpy (tail flag clear): (ep_return, return_to_go, ep_first, ep_last)."""
    n = r.shape[0]
    brk = d != 0
    if tol is not None and n > 1:
        delta = (s[1:] - ns[:-1]).astype(np.float64)
        ss = np.zeros(n - 1)
        for c in range(delta.shape[1]):
            ss = ss + delta[:, c] * delta[:, c]
        brk[:-1] |= ss > tol * tol
    rows = np.arange(n)
    prev = np.maximum.accumulate(np.where(brk, rows, -1))
    p = np.concatenate(([-1], prev[:-1]))
    o = rows - p - 1
    last = np.flatnonzero(brk | ((o + 1) % T == 0))
    first = (p + 1 + (o // T) * T)[last]
    length = last - first + 1
    r64 = r.astype(np.float64)
    ep_return, rtg = np.zeros(n), np.zeros(n)
    ep_first, ep_last = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    if len(last):
        by_length = np.argsort(-length, kind="stable")                 # the episodes still running at step k: a prefix
        f, l, ln = first[by_length], last[by_length], length[by_length]
        acc, g = np.zeros(len(l)), r64[l]
        rtg[l] = g
        for k in range(int(ln[0])):
            m = int(np.searchsorted(-ln, -k, side="left"))              # episodes longer than k
            acc[:m] = acc[:m] + r64[f[:m] + k]
            if k:
                g[:m] = r64[l[:m] - k] + DISCOUNT * g[:m]
                rtg[l[:m] - k] = g[:m]
        covered = last[-1] + 1
        ep_first[:covered], ep_last[:covered] = np.repeat(first, length), np.repeat(last, length)
        per_episode = np.empty(len(l))
        per_episode[by_length] = acc
        ep_return[:covered] = np.repeat(per_episode, length)
    return ep_return, rtg, ep_first, ep_last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--device-only", action="store_true", help="skip the host sides (kernel traces)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    for n in (int(x) for x in args.rows.split(",")):
        buf = iql.ReplayBuffer(S, A, n, "cuda")
        buf.fill_synthetic(n, seed=1, p_done=0.001)
        buf._rows[1:n, :S] = buf._rows[: n - 1, S + A: 2 * S + A]            # continuous states: s[i+1] = s'[i]
        buf._writes += 1
        results = {}

        def device(tol=None):
            results["device" if tol is None else "device_rule"] = buf.episode_returns(T, DISCOUNT, state_break_tol=tol)

        def host(tol=None):
            r, d = buf._rewards[:n, 0].cpu().numpy(), buf._dones[:n, 0].cpu().numpy()
            s = ns = None
            if tol is not None:
                s, ns = buf._states[:n].cpu().numpy(), buf._next_states[:n].cpu().numpy()
            out = host_episode_returns(r, d, s, ns, tol)
            results["host" if tol is None else "host_rule"] = [torch.from_numpy(x).cuda() for x in out]

        # the device sides alternate among themselves, then the host sides: a device window behind a host window of
        # 0.1 - 2 s finds the GPU idle and measures its wake-up
        device_sides = {"device": device, "device_rule": lambda: device(TOL), "range": lambda: buf.return_reward_range(T)}
        host_sides = {} if args.device_only else {"host": host, "host_rule": lambda: host(TOL)}
        sides = {**device_sides, **host_sides}
        times = {k: [] for k in sides}
        for group, repeats in ((device_sides, args.repeats), (host_sides, min(args.repeats, args.host_repeats))):
            for rep in range(repeats + 1):                   # window 0 of each side is its warm-up
                for name, fn in group.items():
                    t = timed(fn)
                    if rep:
                        times[name].append(t)
        med = {k: statistics.median(v) for k, v in times.items()}
        er = results["device"]
        out = {"rows": n, "state_dim": S, "action_dim": A, "max_episode_steps": T, "discount": DISCOUNT,
               "repeats": args.repeats, "episodes": er.episodes}
        for k in sides:
            out[k + "_s"], out[k + "_min_s"], out[k + "_max_s"] = med[k], min(times[k]), max(times[k])
        out["device_over_range"] = med["device"] / med["range"]
        out["device_rule_over_range"] = med["device_rule"] / med["range"]
        assert results["device_rule"].episodes == er.episodes
        if not args.device_only:
            out["host_repeats"] = min(args.repeats, args.host_repeats)
            out["host_over_device"] = med["host"] / med["device"]
            out["host_rule_over_device_rule"] = med["host_rule"] / med["device_rule"]
            for side, dev in (("host", er), ("host_rule", results["device_rule"])):
                for got, want in zip(results[side], (dev.ep_return, dev.return_to_go, dev.ep_first, dev.ep_last)):
                    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), side
            out["host_equals_device_bitwise"] = True
        print(json.dumps(out), flush=True)
        del buf, results, er
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
