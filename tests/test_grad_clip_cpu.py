"""CPU-only tests of gradient-norm clipping (no GPU in the process): the fp32 restatement the GPU tests compare
against (tests/clip_ref.py) is tied to torch.nn.utils.clip_grad_norm_; the three entry points are declared, exported
and bound; NULL and NaN are rejected before anything is touched; a CPU trainer refuses the setting."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import clip_ref
import iql
import iqlhip_binding as hb
import synth
from helpers import step_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"iqlhip_set_grad_clip": 2, "iqlhip_get_grad_clip": 2, "iqlhip_read_grad_clip": 3}
HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}


def _oracle_grads(S=17, A=6, B=33):
    from oracle import iql_oracle as O
    params = synth.synth_params(S, A, seed=5)
    return O.iql_losses_and_grads(params, step_batch(S, A, B, seed=6), dict(HYPER, deterministic=False))["grads"]


@pytest.mark.parametrize("scale", [0.125, 0.999, 2.0, None], ids=["hard", "barely", "above", "no_limit"])
def test_restatement_is_torchs_clip_grad_norm(scale):
    """A limit far below the norm, just below it, above it, and none: total norm and scaled gradients within 2 fp32
    ulp of the norm (torch reduces norms of norms in fp32; the restatement may sum in another order)."""
    grads = _oracle_grads()
    torch.set_num_threads(1)              # (clip_ref.tensor_norm restates torch's single-thread reduction order)
    for grp, nets in clip_ref.GROUPS.items():
        tensors = [torch.nn.Parameter(torch.from_numpy(g.copy())) for n in nets for g in grads[n].values()]
        for p in tensors:
            p.grad = p.detach().clone()
        norm0 = float(clip_ref.group_norm(grads, nets))
        m = None if scale is None else norm0 * scale
        want_norm = float(torch.nn.utils.clip_grad_norm_(tensors, float("inf") if m is None else m))
        scaled, norms, coefs = clip_ref.clip_coefs(grads, {grp: m})
        ulp = float(np.spacing(np.float32(want_norm)))
        assert abs(float(norms[grp]) - want_norm) <= 2 * ulp, (grp, norms[grp], want_norm)
        if scale in (2.0, None):
            assert coefs[grp] == np.float32(1.0)
        else:
            assert coefs[grp] < np.float32(1.0)
        got = [scaled[n][k] for n in nets for k in grads[n]]
        for p, g in zip(tensors, got):
            # a 2-ulp difference of the norm moves the coefficient by 2 ulp relative: the same share of each element
            tol = 2 * ulp / want_norm * np.abs(p.grad.numpy()) + 2.0 ** -24 * np.abs(p.grad.numpy())
            assert np.all(np.abs(p.grad.numpy().astype(np.float64) - g) <= tol), grp
        for other in clip_ref.ORDER:          # the other groups carry no limit: untouched
            if other != grp:
                assert coefs[other] == np.float32(1.0)
                for n in clip_ref.GROUPS[other]:
                    for k in grads[n]:
                        assert np.array_equal(scaled[n][k], grads[n][k])


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    m = re.search(r"#define\s+IQLHIP_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == hb.lib().iqlhip_version() >= 330
    m = re.search(r"#define\s+IQLHIP_N_STATS\s+(\d+)", header)
    assert m and int(m.group(1)) == 16 == hb.IQLHIP_N_STATS == len(hb.STAT_NAMES)
    bound = {name: args for name, _, args in hb.SYMBOLS}
    for name, n_args in SYMBOLS.items():
        d = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert d and len(d.group(1).split(",")) == n_args, name
        assert len(bound[name]) == n_args, name
        fn = getattr(hb.lib(), name)                 # (AttributeError if the built library does not export it)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args


def test_null_and_nan_are_rejected_without_a_gpu():
    lib = hb.lib()
    lim, out = (C.c_float * 3)(1.0, 1.0, 1.0), (C.c_float * 6)()
    fake = 4096       # never dereferenced
    for g in range(3):
        bad = (C.c_float * 3)(1.0, 1.0, 1.0)
        bad[g] = float("nan")
        assert lib.iqlhip_set_grad_clip(fake, bad) == hb.E_INVAL
        assert "NaN" in hb.last_error()
    for rc in (lib.iqlhip_set_grad_clip(None, lim), lib.iqlhip_set_grad_clip(fake, None),
               lib.iqlhip_get_grad_clip(None, lim), lib.iqlhip_get_grad_clip(fake, None),
               lib.iqlhip_read_grad_clip(None, out, None), lib.iqlhip_read_grad_clip(fake, None, None)):
        assert rc == hb.E_INVAL


def _cpu_trainer(S=17, A=6):
    actor = iql.GaussianPolicy(S, A, 1.0)
    qf, vf = iql.TwinQ(S, A), iql.ValueFunction(S)
    return iql.ImplicitQLearning(max_action=1.0, actor=actor,
                                 actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                 q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                                 v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 max_steps=1000, device="cpu")


def test_cpu_trainer_refuses_the_setting():
    tr = _cpu_trainer()
    assert tr.grad_clip is None
    for arg in (1.0, {"vf": 1.0}, (1.0, None, 2.0), None):
        with pytest.raises(RuntimeError, match="GPU"):
            tr.set_grad_clip(arg)
    with pytest.raises(RuntimeError, match="GPU"):
        tr.last_grad_clip()
    assert tr.grad_clip is None and "grad_clip" not in str(sorted(tr.state_dict()))
