"""CPU-only tests of the per-step training statistics (no GPU in the process): the float64 restatement the GPU tests
compare against (tests/stats_ref.py) is tied to the reference's recorded losses; the four entry points are declared,
exported and bound; the Python surface refuses what it must before any library call and leaves train()'s dict alone
while statistics are off."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import iql
import iqlhip_binding as hb
import stats_ref
from helpers import SINGLE_STEP_CASES, assert_losses, load_golden, single_step_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"iqlhip_set_step_stats": 2, "iqlhip_read_step_stats": 3, "iqlhip_read_stats_ring": 4,
           "iqlhip_group_read_step_stats": 4}
G1_CASES = [n for n in SINGLE_STEP_CASES if n.startswith("g1_")]


@pytest.mark.parametrize("name", G1_CASES)
def test_restatement_reproduces_the_recorded_losses(name):
    """Head values from the CPU port on a g1 fixture's inputs -> stats_ref's own adv and y -> value_loss and q_loss,
    against the losses the reference recorded, at the loss tolerance tests/test_oracle_golden.py holds the single-step
    fixtures to (1e-5 relative).  The 13 statistics are then consistent with those terms by construction."""
    from oracle import iql_torch_port as port
    z, meta = load_golden(name)
    params, batch, hyper = single_step_inputs(meta)
    torch.set_num_threads(1)
    tr = port.CpuIQL(meta["S"], meta["A"], params=params, gaussian=meta["gaussian"], iql_tau=hyper["iql_tau"],
                     beta=hyper["beta"], discount=hyper["discount"], tau=hyper["tau"], lrs=meta["lrs"],
                     max_steps=meta["max_steps"])
    s, a, ns = (torch.from_numpy(batch[k]) for k in ("s", "a", "ns"))
    with torch.no_grad():
        v, next_v = tr.vf(s).numpy(), tr.vf(ns).numpy()
        q1, q2 = (x.numpy() for x in tr.qf.both(s, a))
        tq1, tq2 = (x.numpy() for x in tr.q_target.both(s, a))
    t = stats_ref.row_terms(next_v, v, tq1, tq2, q1, q2, batch["r"], batch["d"], hyper["beta"], hyper["discount"])
    value_loss, q_loss = stats_ref.losses_from_terms(t, hyper["iql_tau"])
    assert_losses([value_loss, q_loss], z["losses"][:2], 1e-5, what=name)
    st = stats_ref.row_stats(next_v, v, tq1, tq2, q1, q2, batch["r"], batch["d"], hyper["beta"], hyper["discount"])
    assert st.shape == (13,) and np.all(np.isfinite(st))
    assert st[8] <= st[7] <= st[9] and 0.0 <= st[10] <= 1.0 and 0.0 <= st[12] <= 1.0
    assert 0.0 < st[11] <= stats_ref.EXP_ADV_MAX
    assert abs(st[7] - (st[4] - st[0])) <= 1e-12 * max(1.0, abs(st[4]), abs(st[0]))     # mean adv = mean tq - mean v


def test_restatement_counts_and_norms_on_hand_made_rows():
    z = np.zeros(4)
    # adv = tq - v = [-1, 0, 2, 10]: u < 0 is the lower side (row 0 only); beta 1: exp(10) sits on the clamp
    st = stats_ref.row_stats(z, -np.array([-1.0, 0.0, 2.0, 10.0]), z, z + 5.0, z + 1.0, z - 1.0, z + 1.0,
                             np.array([0.0, 1.0, 0.0, 1.0]), beta=1.0, discount=0.5)
    assert st[8] == -1.0 and st[9] == 10.0 and st[10] == 0.75 and st[12] == 0.25 and st[6] == 2.0
    assert st[5] == 1.0                                   # next_v = 0: y = r
    assert abs(st[11] - (np.exp(-1.0) + 1.0 + np.exp(2.0) + 100.0) / 4) < 1e-12
    flat = np.arange(10, dtype=np.float32)
    n = stats_ref.grad_norms(flat, [(0, 2), (2, 4), (4, 6), (6, 10)])
    assert np.allclose(n, np.sqrt([1.0, 4 + 9 + 16 + 25, 36 + 49 + 64 + 81]), rtol=1e-15)


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    m = re.search(r"#define\s+IQLHIP_N_STATS\s+(\d+)", header)
    assert m and int(m.group(1)) == 16 == hb.IQLHIP_N_STATS
    m = re.search(r"#define\s+IQLHIP_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == hb.lib().iqlhip_version() >= 320
    bound = {name: args for name, _, args in hb.SYMBOLS}
    for name, n_args in SYMBOLS.items():
        d = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert d and len(d.group(1).split(",")) == n_args, name
        assert len(bound[name]) == n_args, name
        fn = getattr(hb.lib(), name)                 # (AttributeError if the built library does not export it)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args


def test_stat_names():
    assert len(hb.STAT_NAMES) == 16 == len(set(hb.STAT_NAMES))
    assert tuple(hb.STAT_NAMES) == stats_ref.STAT_NAMES
    assert hb.STAT_NAMES[0] == "v_mean" and hb.STAT_NAMES[12] == "exp_adv_clamped_frac"
    assert hb.STAT_NAMES[13:] == ("grad_norm_vf", "grad_norm_qf", "grad_norm_actor")


def test_entry_points_reject_null_arguments():
    lib = hb.lib()
    out = (C.c_float * 16)()
    fake = 4096       # never dereferenced
    for rc in (lib.iqlhip_set_step_stats(None, 1), lib.iqlhip_read_step_stats(None, out, None),
               lib.iqlhip_read_step_stats(fake, None, None), lib.iqlhip_read_stats_ring(None, out, 1, None),
               lib.iqlhip_read_stats_ring(fake, None, 1, None), lib.iqlhip_group_read_step_stats(None, out, 1, None),
               lib.iqlhip_group_read_step_stats(fake, None, 1, None)):
        assert rc == hb.E_INVAL


def _cpu_trainer(S=17, A=6):
    actor = iql.GaussianPolicy(S, A, 1.0)
    qf, vf = iql.TwinQ(S, A), iql.ValueFunction(S)
    return iql.ImplicitQLearning(max_action=1.0, actor=actor,
                                 actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                 q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                                 v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 max_steps=1000, device="cpu")


def test_return_stats_needs_the_opt_in():
    tr = _cpu_trainer()
    buf = iql.ReplayBuffer(17, 6, 8, "cpu")
    with pytest.raises(ValueError, match="set_step_stats"):
        tr.train_steps(buf, 4, 2, return_stats=True)
    assert tr.total_it == 0
    g = object.__new__(iql.ImplicitQLearningGroup)
    g.trainers, g._g, g._ctxs, g._actor_dropout, g._mixed_batch = [tr, _cpu_trainer()], None, None, False, False
    with pytest.raises(RuntimeError, match="GPU"):           # (the members are looked at first, as always)
        g.train_steps([buf, buf], 2, 4, [1, 2], return_stats=True)


def test_unsupported_cases_are_refused_before_any_library_call():
    # data parallelism: refused with statistics on, untouched with them off (a CPU trainer then fails on "no GPU")
    tr = _cpu_trainer()
    tr._dp_world, tr._dp_exchange = 2, "rccl"
    with pytest.raises(RuntimeError, match="GPU"):
        tr._prepare(256)
    tr.set_step_stats(True)
    with pytest.raises(NotImplementedError, match="data parallelism"):
        tr._prepare(256)
    with pytest.raises(NotImplementedError, match="data parallelism"):
        tr.train_steps(iql.ReplayBuffer(17, 6, 8, "cpu"), 4, 2, return_stats=True)
    tr._dp_world, tr._dp_exchange = 1, "torch"
    with pytest.raises(NotImplementedError, match="data parallelism"):
        tr._prepare(256)
    # large-batch bf16: above 512 rows only
    tr = _cpu_trainer()
    tr.set_step_stats(True)
    tr._precision = "bf16"
    with pytest.raises(NotImplementedError, match="512 rows"):
        tr._prepare(1024)
    with pytest.raises(NotImplementedError, match="512 rows"):
        tr._prepare(513)
    with pytest.raises(RuntimeError, match="GPU"):            # 512 rows are supported: the next check is the device
        tr._prepare(512)
    tr._precision = "f32"
    with pytest.raises(RuntimeError, match="GPU"):
        tr._prepare(1024)
    tr.set_step_stats(False)
    tr._precision = "bf16"
    with pytest.raises(RuntimeError, match="GPU"):
        tr._prepare(1024)
    assert tr.total_it == 0


class _StubLib:
    """The library calls of one synchronous eager step, recorded; losses 1, 2, 3 and statistics 0..15."""
    def __init__(self):
        self.calls = []

    def iqlhip_step(self, ctx, b, sc, stream):
        self.calls.append("step")
        return 0

    def iqlhip_read_losses(self, ctx, out, stream):
        self.calls.append("read_losses")
        out[0], out[1], out[2] = 1.0, 2.0, 3.0
        return 0

    def iqlhip_read_step_stats(self, ctx, out, stream):
        self.calls.append("read_step_stats")
        for i in range(16):
            out[i] = float(i)
        return 0


def test_train_dict_is_unchanged_while_statistics_are_off(monkeypatch):
    stub = _StubLib()
    monkeypatch.setattr(hb, "lib", lambda: stub)
    tr = _cpu_trainer()
    tr._ctx = C.c_void_p(4096)
    monkeypatch.setattr(tr, "_stream", lambda: None)
    try:
        log = tr._run_step(hb.Batch(), 256, sync=True)
        assert log == {"value_loss": 1.0, "q_loss": 2.0, "actor_loss": 3.0}
        assert list(log) == ["value_loss", "q_loss", "actor_loss"] and stub.calls == ["step", "read_losses"]
        tr.set_step_stats(True)
        log = tr._run_step(hb.Batch(), 256, sync=True)
        assert list(log)[:3] == ["value_loss", "q_loss", "actor_loss"] and len(log) == 3 + 16
        assert [log["stats/" + n] for n in hb.STAT_NAMES] == [float(i) for i in range(16)]
        assert stub.calls[2:] == ["step", "read_losses", "read_step_stats"]
        assert tr._run_step(hb.Batch(), 256, sync=False) is None
        tr.set_step_stats(False)
        assert list(tr._run_step(hb.Batch(), 256, sync=True)) == ["value_loss", "q_loss", "actor_loss"]
    finally:
        tr._ctx = None            # (nothing for __del__ to release)
