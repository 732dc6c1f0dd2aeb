#!/usr/bin/env python
"""Reference fixtures for the row-weighted IQL step (tests/golden/g20_loss_weights_*.npz).

    python tools/make_loss_weight_goldens.py --ref REFERENCE_CHECKOUT [--out tests/golden]

The reference has no per-row loss weights, so its train() cannot be called as it is.  This tool imports the reference's
finetune/iql.py by path at run time (tools/make_goldens.py's importer; nothing of it is copied), builds its
ValueFunction, TwinQ and policy from `synth` parameters, and runs ONE step of the reference's own modules, optimisers,
learning-rate schedule and soft update on the three weighted-mean losses, formed here with torch autograd:

    value_loss = mean_r c_r |tau - 1(u_r < 0)| u_r^2
    q_loss     = (mean_r c_r e1_r^2 + mean_r c_r e2_r^2) / 2
    actor_loss = mean_r c_r exp_adv_r bc_r

in the order of the reference's train(): V, then Q and the target update, then the policy.  The fixtures have the layout
of the g1_* single-step fixtures (tests/helpers.check_step_against_golden reads them) plus `weights` and `inter.td`.
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _load("iqlhip_make_goldens", os.path.join(HERE, "make_goldens.py"))
synth = G.synth

# name, S, A, gaussian, B, seed — the smallest shapes that reach each code path of the row-weighted backward
CASES = [
    ("g20_loss_weights_S17A6_gauss_B100", 17, 6, True, 100, 41),     # ragged tile
    ("g20_loss_weights_S39A28_gauss_B10", 39, 28, True, 10, 42),     # action dims >= 8
    ("g20_loss_weights_S29A8_det_B256", 29, 8, False, 256, 43),      # full tile
    ("g20_loss_weights_S17A6_gauss_B300", 17, 6, True, 300, 44),     # multi-chunk
]


def loss_weights(B: int, seed: int) -> np.ndarray:
    """Uniform in [0.05, 1], float32 (tests rebuild them from the fixture's `weights` array, not from this)."""
    rng = np.random.RandomState(7000 + seed)
    return (0.05 + 0.95 * rng.rand(B)).astype(np.float32)


def weighted_step(ref, tr, batch, c):
    """One step of trainer `tr` on the weighted-mean losses; returns (losses, td [B, 2])."""
    s, a, r, ns, d = batch
    tr.total_it += 1
    with torch.no_grad():
        next_v = tr.vf(ns)
        target_q = tr.q_target(s, a)
    # V
    v = tr.vf(s)
    adv = target_q - v
    wgt = torch.abs(tr.iql_tau - (adv < 0).float())
    v_loss = torch.mean(c * (wgt * adv ** 2))
    tr.v_optimizer.zero_grad()
    v_loss.backward()
    tr.v_optimizer.step()
    # Q, then the target update
    r1, d1 = r.squeeze(dim=-1), d.squeeze(dim=-1)
    targets = r1 + (1.0 - d1.float()) * tr.discount * next_v.detach()
    qs = tr.qf.both(s, a)
    td = torch.stack([(q - targets).detach() for q in qs], dim=1)
    q_loss = sum(torch.mean(c * (q - targets) ** 2) for q in qs) / len(qs)
    tr.q_optimizer.zero_grad()
    q_loss.backward()
    tr.q_optimizer.step()
    ref.soft_update(tr.q_target, tr.qf, tr.tau)
    # policy
    exp_adv = torch.exp(tr.beta * adv.detach()).clamp(max=ref.EXP_ADV_MAX)
    out = tr.actor(s)
    if isinstance(out, torch.distributions.Distribution):
        bc = -out.log_prob(a).sum(-1, keepdim=False)
    else:
        bc = torch.sum((out - a) ** 2, dim=1)
    pi_loss = torch.mean(c * (exp_adv * bc))
    tr.actor_optimizer.zero_grad()
    pi_loss.backward()
    tr.actor_optimizer.step()
    if tr.actor_lr_schedule is not None:
        tr.actor_lr_schedule.step()
    return np.array([v_loss.item(), q_loss.item(), pi_loss.item()], dtype=np.float64), td.numpy()


def case(ref, name, S, A, gaussian, B, seed, stride, outdir):
    hyper = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    params = synth.synth_params(S, A, seed=seed, gaussian=gaussian)
    data = synth.synth_transitions(B, S, A, seed=1000 + seed)
    tr = G.build_trainer(ref, S, A, params, gaussian, hyper, lrs, max_steps=1000)
    batch = G.to_batch(data)
    inter = G.ref_intermediates(tr, batch)
    c = loss_weights(B, seed)
    losses, td = weighted_step(ref, tr, batch, torch.from_numpy(c))
    out = G.grab(tr, stride, gaussian)
    out.update({f"inter.{k}": v for k, v in inter.items()})
    out["inter.td"] = td
    out["weights"] = c
    out["losses"] = losses
    out["lr_after"] = np.array([tr.actor_optimizer.param_groups[0]["lr"]], dtype=np.float64)
    meta = {"kind": "single_step", "S": S, "A": A, "gaussian": gaussian, "B": B, "seed": seed, "stride": stride,
            "hyper": hyper, "lrs": lrs, "max_steps": 1000, "edge": False, "loss_weights": True}
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(outdir, name + ".npz"), **out)
    print(f"{name}: losses={losses}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--stride", type=int, default=13)
    args = ap.parse_args()
    torch.set_num_threads(1)
    ref = G.import_reference(args.ref)
    for name, S, A, gaussian, B, seed in CASES:
        case(ref, name, S, A, gaussian, B, seed, args.stride, args.out)


if __name__ == "__main__":
    main()
