"""Reward normalisation of a replay buffer that lives on the GPU: device ingest against the host round trip (GPU).

A 1 M-row and a 10 M-row device buffer at configs[1]'s dims (S=17, A=6), filled in place with
fill_synthetic(p_done=0.001), max_episode_steps = 1000 (the locomotion YAMLs' `normalize_reward: true`):

  device   buffer.modify_reward_("hopper-medium-v2"): previous-terminal scan, one thread per episode summing in
           float64 in row order, min / max read back, reward column rescaled in place
  host     what a caller had to do before: download the reward and done columns, run the host modify_reward of the
           drop-in iql.py on them, upload the rewards again

Both sides start from the same reward column (restored outside the timed window) and end in a device synchronise.  The
two alternate in one process after a warm-up of each; medians over `--repeats` windows.  Prints one JSON line per size;
`range_s` is buffer.return_reward_range alone (scan + episode sums + read-back).

    python tools/gpu_reward_ingest_bench.py [--rows 1000000,10000000] [--repeats 7] [--device-only]
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

S, A, T, ENV = 17, 6, 1000, "hopper-medium-v2"


def timed(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--device-only", action="store_true", help="skip the host side (kernel traces)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    for n in (int(x) for x in args.rows.split(",")):
        buf = iql.ReplayBuffer(S, A, n, "cuda")
        buf.fill_synthetic(n, seed=1, p_done=0.001)
        rewards = buf._rewards[:n, 0]
        snapshot = rewards.clone()
        results = {}

        def device():
            results["device"] = buf.modify_reward_(ENV, T)

        def host():
            data = {"rewards": rewards.cpu().numpy(), "terminals": buf._dones[:n, 0].cpu().numpy()}
            results["host"] = iql.modify_reward(data, ENV, T)
            rewards.copy_(torch.from_numpy(data["rewards"]).cuda())
            buf._writes += 1

        sides = {"device": device} if args.device_only else {"device": device, "host": host}
        times = {k: [] for k in sides}
        times["range"] = []
        for rep in range(args.repeats + 1):                  # window 0 of each side is its warm-up
            for name, fn in sides.items():
                rewards.copy_(snapshot)
                t = timed(fn)
                if rep:
                    times[name].append(t)
            rewards.copy_(snapshot)
            t = timed(lambda: buf.return_reward_range(T))
            if rep:
                times["range"].append(t)
        out = {"rows": n, "state_dim": S, "action_dim": A, "max_episode_steps": T, "repeats": args.repeats,
               "device_s": statistics.median(times["device"]), "range_s": statistics.median(times["range"]),
               "device_min_s": min(times["device"]), "device_max_s": max(times["device"]),
               "min_ret": results["device"]["min_ret"], "max_ret": results["device"]["max_ret"]}
        if not args.device_only:
            out.update({"host_s": statistics.median(times["host"]), "host_min_s": min(times["host"]),
                        "host_max_s": max(times["host"]),
                        "host_over_device": statistics.median(times["host"]) / statistics.median(times["device"]),
                        # the drop-in's host sums are segmented numpy reductions: equal to rounding, not bit for bit
                        "host_min_ret": results["host"]["min_ret"], "host_max_ret": results["host"]["max_ret"]})
        print(json.dumps(out), flush=True)
        del buf, rewards, snapshot
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
