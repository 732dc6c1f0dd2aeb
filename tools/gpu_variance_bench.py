"""Time the variance learner's step (jsrl-corl_amd/iqlhip_variance.py) on the GPU: microseconds per _update_v and per
get_values at B = 256 for S = 17 and 29, the share of a step that is packing and uploading the block, and — with
--reference PATH/variance_learner.py on a host that has the reference — the reference's _update_v on that host's CPU.
Wall-clock per call (each call ends in its own synchronisation), median and quartiles over --iters calls after --warmup.

    python tools/gpu_variance_bench.py [--iters 300] [--warmup 30] [--reference PATH] [--out profiles/variance_learner_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "jsrl-corl_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def rollout(S, B, seed):
    rng = np.random.RandomState(seed)
    obs = rng.standard_normal((B, S)).astype(np.float32)
    nxt = rng.standard_normal((B, S)).astype(np.float32)
    rewards = rng.uniform(-1, 1, size=B).astype(np.float32)
    nd = rng.uniform(size=B) < 0.05
    return ([torch.from_numpy(o.copy()) for o in obs], [None] * B, [float(r) for r in rewards], [False] * B,
            [torch.from_numpy(o.copy()) for o in nxt], [bool(d) for d in nd])


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    q = np.percentile(ts, [25, 50, 75])
    return f"median {q[1]:9.1f} us  (quartiles {q[0]:.1f} .. {q[2]:.1f}, min {min(ts):.1f}, n = {iters})", q[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variance_learner_bench.txt"))
    args = ap.parse_args()
    lines = [f"variance learner, B = 256, wall clock per call; torch {torch.__version__}"]
    gpu = torch.cuda.is_available()
    if gpu:
        import ctypes as C
        import iqlhip_binding as hb
        import variance_learner as VL
        from iqlhip_variance import adam_scalars
        lines.append(f"device: {torch.cuda.get_device_name(0)}")
    for S in (17, 29):
        batch = rollout(S, 256, S)
        if gpu:
            L = VL.VarianceLearner(S, 6, None, None, device="cuda")
            sync = torch.cuda.synchronize
            for phase, flag in (("mf", False), ("vf", True)):
                txt, _ = timed(lambda: L._update_v(batch, flag), args.iters, args.warmup)
                lines.append(f"S={S:3d} _update_v ({phase})       {txt}")
            txt, step_us = timed(lambda: L._update_v(batch, False), args.iters, args.warmup)
            txt_v, _ = timed(lambda: L.get_values(batch[0], batch[2], batch[4], batch[3], batch[5]), args.iters, args.warmup)
            lines.append(f"S={S:3d} get_values            {txt_v}")
            txt_u, up_us = timed(lambda: (L._upload(batch[0], batch[2], batch[4], batch[5]), sync()), args.iters, args.warmup)
            lines.append(f"S={S:3d} pack + upload alone   {txt_u}  = {100.0 * up_us / step_us:.0f} % of an _update_v (mf)")
            sc = adam_scalars(0.0, (0.9, 0.999), 1e-8, 1)

            def device_only():
                hb.check(hb.lib().iqlhip_var_step(L._h, L._blk.data_ptr(), 256, 0, C.byref(sc), L._stream()))
                sync()
            txt_d, _ = timed(device_only, args.iters, args.warmup)
            lines.append(f"S={S:3d} library step + sync   {txt_d}  (block already on the device, lr = 0)")
        if args.reference and os.path.exists(args.reference):
            from make_variance_goldens import load_reference
            ref = load_reference(args.reference)
            torch.manual_seed(0)
            Lr = ref.VarianceLearner(S, 6, None, None)
            txt_r, _ = timed(lambda: Lr._update_v(batch, False), max(3, args.iters // 30), 1)
            lines.append(f"S={S:3d} reference _update_v on this host's CPU ({os.cpu_count()} CPUs, torch threads {torch.get_num_threads()}): {txt_r}")
        else:
            lines.append(f"S={S:3d} reference _update_v: the reference is not on this host")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
