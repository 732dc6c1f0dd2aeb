"""CPU-only tests of scoring without a step (no GPU in the process): the reference the GPU tests compare against
(tests/score_ref.py) is tied to the reference's recorded intermediates and losses; the entry points are declared,
exported and bound; the Python surface refuses what it must before any library call."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import iql
import iqlhip_binding as hb
import iqlhip_score as score
import score_ref
from helpers import SINGLE_STEP_CASES, assert_losses, load_golden, rel_err, single_step_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"iqlhip_score_rows": 11, "iqlhip_pack_rows": 4}


@pytest.mark.parametrize("name", SINGLE_STEP_CASES)
def test_score_ref_meets_the_recorded_intermediates_and_losses(name):
    z, meta = load_golden(name)
    params, batch, hyper = single_step_inputs(meta)
    ref = score_ref.reference(params, batch, hyper)
    cols = {k: ref["cols"][:, i] for i, k in enumerate(score_ref.SCORE_NAMES)}
    for k in ("next_v", "target_q", "adv"):
        e = rel_err(cols[k], z[f"inter.{k}"])
        assert e <= 2e-5, (name, k, e)
    assert_losses(ref["losses"], z["losses"], 1e-5, what=name)
    assert ref["cols"].shape == (meta["B"], 8) and ref["means"].shape == (8,)
    assert np.all(cols["exp_adv"] <= 100.0) and np.all(cols["exp_adv"] > 0.0)
    assert np.array_equal(cols["adv"], cols["target_q"] - cols["v"])


def test_score_ref_bc_by_hand():
    info = {"mu": np.array([[0.5, -0.25]], dtype=np.float64)}
    batch = {"a": np.array([[1.0, 0.25]], dtype=np.float64)}
    assert score_ref.bc_term(info, batch, {"deterministic": True})[0] == 0.5
    ls = np.array([0.0, -30.0])                                         # the second one sits on the clamp, -20
    want = 0.25 / 2 + 0.25 / (2 * np.exp(-40.0)) - 20.0 + 2 * np.log(np.sqrt(2 * np.pi))
    got = score_ref.bc_term(info, batch, {"deterministic": False}, log_std=ls)[0]
    assert abs(got - want) <= 1e-12 * abs(want)


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    m = re.search(r"#define\s+IQLHIP_N_SCORE\s+(\d+)", header)
    assert m and int(m.group(1)) == 8 == hb.IQLHIP_N_SCORE == len(hb.SCORE_NAMES)
    assert tuple(hb.SCORE_NAMES) == score_ref.SCORE_NAMES
    m = re.search(r"#define\s+IQLHIP_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == hb.lib().iqlhip_version() >= 360
    bound = {name: (res, args) for name, res, args in hb.SYMBOLS}
    for name, nargs in NEW.items():
        d = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert d and len(d.group(1).split(",")) == nargs, name
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == nargs, name
        fn = getattr(hb.lib(), name)                 # (AttributeError if the built library does not export it)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
    assert score.SUMMARY_KEYS == ("value_loss", "q_loss", "actor_loss") + tuple("mean_" + n for n in hb.SCORE_NAMES)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = hb.lib()
    fake = 4096       # never dereferenced: every rejection below comes before a context is looked at
    out = (C.c_float * 11)()
    assert lib.iqlhip_score_rows(None, fake, 44, 8, 0, 8, None, fake, 0, out, None) == hb.E_INVAL
    assert lib.iqlhip_score_rows(fake, None, 44, 8, 0, 8, None, fake, 0, out, None) == hb.E_INVAL
    assert lib.iqlhip_pack_rows(None, C.byref(hb.Batch()), fake, None) == hb.E_INVAL
    assert lib.iqlhip_pack_rows(fake, None, fake, None) == hb.E_INVAL
    assert lib.iqlhip_pack_rows(fake, C.byref(hb.Batch()), None, None) == hb.E_INVAL


# ---- the Python refusals, through a stub in place of the library: none of them may reach it
class _Stub:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            return 0
        return call


def _trainer(monkeypatch, S=17, A=6):
    """A trainer that believes it is attached (a context word, its device = where the fake buffers live) over a stub
    library that records every call."""
    stub = _Stub()
    actor = iql.GaussianPolicy(S, A, 1.0)
    qf, vf = iql.TwinQ(S, A), iql.ValueFunction(S)
    tr = iql.ImplicitQLearning(max_action=1.0, actor=actor, actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                               q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                               v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                               max_steps=1000, device="cpu")
    monkeypatch.setattr(hb, "lib", lambda: stub)
    monkeypatch.setattr(hb, "row_stride", lambda s, a: (2 * s + a + 2 + 3) // 4 * 4)
    monkeypatch.setattr(tr, "_stream", lambda: None)
    return tr, stub


def _buffer(S=17, A=6, rows=64, size=40, gpu=True, ld=None):
    ld = (2 * S + A + 2 + 3) // 4 * 4 if ld is None else ld
    return types.SimpleNamespace(_rows=torch.zeros((rows, ld)), _gpu=gpu, _state_dim=S, _action_dim=A, _ld=ld, _size=size,
                                 _buffer_size=rows)


def test_cpu_trainer_raises_runtime_error(monkeypatch):
    tr, stub = _trainer(monkeypatch)
    batch = [torch.zeros(4, 17), torch.zeros(4, 6), torch.zeros(4, 1), torch.zeros(4, 17), torch.zeros(4, 1)]
    for call in (lambda: tr.score_buffer(_buffer()), lambda: tr.score(batch), lambda: tr.evaluate(batch)):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    assert stub.calls == []


def test_python_refusals_never_reach_the_library(monkeypatch):
    tr, stub = _trainer(monkeypatch)
    tr._ctx, tr._dev, tr._S, tr._A, tr._gaussian = C.c_void_p(4096), torch.device("cpu"), 17, 6, True
    try:
        ok = _buffer()
        cases = [
            (ValueError, "lives on", lambda: tr.score_buffer(_buffer(gpu=False))),                  # a CPU buffer
            (ValueError, "lives on", lambda: tr.score_buffer(object())),
            (ValueError, "state_dim", lambda: tr.score_buffer(_buffer(S=11, A=3))),                  # foreign dims
            (ValueError, "stride", lambda: tr.score_buffer(_buffer(ld=48))),                         # foreign stride
            (ValueError, "empty", lambda: tr.score_buffer(_buffer(size=0))),                         # an empty buffer
            (ValueError, "empty range", lambda: tr.score_buffer(ok, start=40)),
            (ValueError, "empty range", lambda: tr.score_buffer(ok, start=3, n=0)),
            (ValueError, "empty range", lambda: tr.score_buffer(ok, start=-1, n=2)),
            (ValueError, "beyond", lambda: tr.score_buffer(ok, start=30, n=11)),                     # start + n > len
            (ValueError, "beyond", lambda: tr.score_buffer(ok, n=41)),
            (ValueError, "not both", lambda: tr.score_buffer(ok, start=1, indices=np.arange(3))),
            (ValueError, "not both", lambda: tr.score_buffer(ok, n=3, indices=np.arange(3))),
            (ValueError, "int64", lambda: tr.score_buffer(ok, indices=np.arange(3, dtype=np.int32))),
            (ValueError, "int64", lambda: tr.score_buffer(ok, indices=torch.zeros((2, 2), dtype=torch.int64))),
            (ValueError, "empty index", lambda: tr.score_buffer(ok, indices=np.zeros(0, dtype=np.int64))),
            (IndexError, "index 40 is out of bounds", lambda: tr.score_buffer(ok, indices=np.array([0, 40, 3]))),
            (IndexError, "index -1 is out of bounds", lambda: tr.score_buffer(ok, indices=torch.tensor([5, -1]))),
            (ValueError, r"\[10, 8\]", lambda: tr.score_buffer(ok, n=10, out=torch.zeros(9, 8))),    # a wrong out: shape,
            (ValueError, r"\[10, 8\]", lambda: tr.score_buffer(ok, n=10, out=torch.zeros(10, 7))),
            (ValueError, "float32", lambda: tr.score_buffer(ok, n=10, out=torch.zeros(10, 8, dtype=torch.float64))),  # dtype,
            (ValueError, "float32", lambda: tr.score_buffer(ok, n=10, out=torch.zeros(10, 8, device="meta"))),        # device
            (ValueError, "contiguous", lambda: tr.score_buffer(ok, n=10, out=torch.zeros(10, 16)[:, ::2])),
            (ValueError, "nothing to compute", lambda: tr.score_buffer(ok, out=False, summary=False)),
            (ValueError, "multiple of 32", lambda: tr.score_buffer(ok, chunk_rows=48)),
            (ValueError, "multiple of 32", lambda: tr.score_buffer(ok, chunk_rows=0)),
            (ValueError, "multiple of 32", lambda: tr.score_buffer(ok, chunk_rows=-64)),
        ]
        for exc, match, call in cases:
            with pytest.raises(exc, match=match):
                call()
        batch = [torch.zeros(4, 17), torch.zeros(4, 6), torch.zeros(4, 1), torch.zeros(4, 17), torch.zeros(4, 1)]
        with pytest.raises(ValueError, match="shapes"):
            tr.score([batch[0], torch.zeros(4, 5)] + batch[2:])
        with pytest.raises(ValueError, match=r"\[4, 8\]"):
            tr.score(batch, out=torch.zeros(5, 8))
        with pytest.raises(ValueError, match="multiple of 32"):
            tr.score(batch, chunk_rows=33)
        assert stub.calls == []
        # and a call that passes every check reaches the library exactly once, with the range it named
        seen = []
        stub.iqlhip_score_rows = lambda *a: seen.append(a) or 0
        scores, summary = tr.score_buffer(ok, start=8, n=16, chunk_rows=64)
        assert len(seen) == 1 and seen[0][2:6] == (ok._ld, 40, 8, 16) and seen[0][6] is None and seen[0][8] == 64
        assert tuple(scores.shape) == (16, 8) and list(summary) == list(score.SUMMARY_KEYS)
        assert tr.score_buffer(ok, out=False)[0] is None and seen[1][7] is None and seen[1][4:6] == (0, 40)
        assert tr.score_buffer(ok, indices=np.array([3, 3, 39]), summary=False)[1] is None and seen[2][5] == 3
    finally:
        tr._ctx = None            # (nothing for __del__ to release)
