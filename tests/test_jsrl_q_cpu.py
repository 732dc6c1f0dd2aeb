"""CPU-only tests of the JSRL critic selection (who == 3; no GPU in the process): the two ABI symbols exist in the
header and the library, the numpy restatement of the rule (tests/jsrl_q_ref.py) gives the known uniforms, p = 0.5 at a
tie, the argmax at infinite inverse temperature and the right learner share, and the Python layer checks its arguments
before any library call."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import iql
import iqlhip_binding as hb
import jsrl_q_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_jsrl_q_symbols_in_header_and_library():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    for name, n_args in {"iqlhip_jsrl_set_critics": 2, "iqlhip_jsrl_act_q": 17}.items():
        assert f"int {name}(" in header, name
        fn = getattr(hb.lib(), name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args, name
    assert iql.WHO_CRITIC == 3


def test_jsrl_q_null_handle_is_refused():
    lib = hb.lib()
    with pytest.raises(ValueError, match="NULL"):
        hb.check(lib.iqlhip_jsrl_set_critics(None, None))
    with pytest.raises(ValueError, match="NULL"):
        hb.check(lib.iqlhip_jsrl_act_q(None, None, 17, None, None, None, None, None, None, None, 6, None, None, None, None, 0, None))


# (seed, call, row, A) -> u, from the scalar Philox4x32-10 of oracle/philox_ref.py (pinned to Random123's known
# answers by tests/test_philox_ref_cpu.py): word 2 of the block at counter (row * A, lo32 call, hi32 call, 0xAC7)
KNOWN_U = [((1, 0, 0, 6), 0x956E6422, "0x1.2adcc80000000p-1"),
           ((0x9E3779B97F4A7C15, 7, 5, 6), 0x0139B904, "0x1.39b9800000000p-8"),
           ((12345, 2 ** 32 + 3, 255, 8), 0x852FB857, "0x1.0a5f700000000p-1"),
           ((2 ** 63 + 11, 1, 4095, 28), 0xEEBBE5FA, "0x1.dd77cc0000000p-1")]


@pytest.mark.parametrize("args,word,u_hex", KNOWN_U)
def test_row_uniform_known_answers(args, word, u_hex):
    seed, call, row, A = args
    u = R.row_uniform(seed, call, row + 1, A)
    assert u.dtype == np.float32 and u.shape == (row + 1,)
    assert float(u[row]).hex() == u_hex
    assert float(u[row]) == float((np.float32(word >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24))


def test_tie_gives_exactly_one_half():
    for q, t in ((0.0, 0.0), (1.25, 3.0), (-7.5, 1e6), (3.0, 0.0)):
        assert R.p_learner(q, q, t) == np.float32(0.5)
    assert R.p_learner(1.0, 0.0, 0.0) == np.float32(0.5)          # (a zero inverse temperature: a fair coin)
    assert R.p_learner(1.0, 0.0, 1e9) == np.float32(1.0) and R.p_learner(0.0, 1.0, 1e9) == np.float32(0.0)


def test_infinite_inverse_temperature_is_the_argmax():
    rng = np.random.default_rng(4)
    q = rng.standard_normal((512, 4)).astype(np.float32)
    q[:16, 2:] = q[:16, :2]                  # ties: the learner
    want = np.minimum(q[:, 2], q[:, 3]) >= np.minimum(q[:, 0], q[:, 1])
    assert want[:16].all() and 0 < want.sum() < 512
    assert np.array_equal(R.decide(q, math.inf, seed=99, call=3, A=6), want)
    assert np.array_equal(R.decide(q, 2.0, seed=0, call=3, A=6), want)          # seed 0: the argmax too
    # a very large finite inverse temperature agrees wherever the two values differ
    got = R.decide(q, 1e12, seed=99, call=3, A=6)
    assert np.array_equal(got[16:], want[16:])
    a_g, a_l = rng.standard_normal((512, 6)).astype(np.float32), rng.standard_normal((512, 6)).astype(np.float32)
    out = R.assemble(a_g, a_l, want)
    assert np.array_equal(out[want], a_l[want]) and np.array_equal(out[~want], a_g[~want])


@pytest.mark.parametrize("diff,inv_temp", [(0.3, 2.0), (-0.8, 1.5), (0.05, 10.0), (2.0, 0.0)])
def test_learner_share_is_binomial_around_p(diff, inv_temp):
    n = 10000
    q = np.zeros((n, 4), np.float32)
    q[:, 2:] = np.float32(diff)
    p = float(R.p_learner(np.float32(diff), np.float32(0.0), inv_temp))
    assert abs(p - 1.0 / (1.0 + math.exp(-diff * inv_temp))) < 1e-6
    share = R.decide(q, inv_temp, seed=0xC0FFEE, call=11, A=6).mean()
    assert abs(share - p) <= 4.0 * math.sqrt(p * (1.0 - p) / n), (share, p)


def test_python_layer_checks_before_any_library_call(monkeypatch):
    def cpu_trainer(S=17, A=6):
        import torch
        actor, qf, vf = iql.GaussianPolicy(S, A, 1.0), iql.TwinQ(S, A), iql.ValueFunction(S)
        return iql.ImplicitQLearning(max_action=1.0, actor=actor, actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                     q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4), v_network=vf,
                                     v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4), max_steps=1000, device="cpu")
    monkeypatch.setattr(hb, "lib", lambda: (_ for _ in ()).throw(AssertionError("a library call was made")))
    a, b = cpu_trainer(), cpu_trainer()
    with pytest.raises(ValueError, match="one critic"):
        iql.JsrlActors([a, b], [b, a], critics=[True])
    for t in (a, b):
        t._S, t._A = 17, 6                  # (what a GPU trainer knows of its dims)
    s = np.zeros(17, np.float32)
    j = iql.JsrlActors([a, b], [b, a], critics=[True, None])
    j._check_members = lambda: None         # past the device check: the per-row arguments
    with pytest.raises(ValueError, match=r"member 1: who values must be 0 \(guide\), 1 \(learner\) or 2 \(gate\)$"):
        j.act([s, s], [3, 3])               # a member without a critic: the old message
    with pytest.raises(ValueError, match="or 3 .critic."):
        j.act([s, s], [4, 0])
    for bad in (-1.0, math.nan, [1.0, -0.5], [math.nan, 1.0]):
        with pytest.raises(ValueError, match="q_inv_temp must be"):
            j.act([s, s], [3, 0], q_inv_temp=bad)
    with pytest.raises(ValueError, match="q_inv_temp as 2"):
        j.act([s, s], [3, 0], q_inv_temp=[1.0, 2.0, 3.0])
    assert j._q_inv_temp(None) == [math.inf, math.inf] and j._q_inv_temp(math.inf) == [math.inf, math.inf]
    assert j._q_inv_temp(2.5) == [2.5, 2.5] and j._q_inv_temp([0.0, math.inf]) == [0.0, math.inf]
    jc = iql.JsrlActors([a], [b], critics=True)
    with pytest.raises(ValueError, match="no who == 3"):
        a.online_step_jsrl(jc, None, s, s[:6], 0.0, s, False, 16, s, 3)
    with pytest.raises(ValueError, match="who values must be"):
        a.online_step_jsrl(iql.JsrlActors([a], [b]), None, s, s[:6], 0.0, s, False, 16, s, 3)
