"""CPU-only tests of the JSRL action selection (no GPU in the process): the ABI symbols exist in the header and the
library, who_from_config reproduces every recorded decision and host horizon of g19, eval_actors_jsrl equals a plain
per-member restatement of jsrl_w_iql.eval_actor on scripted envs with fake actors, and the Python layer checks its
arguments before any library call."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest

import iql
import iqlhip_binding as hb
import iqlhip_jsrl as J
import jsrl_ref
from helpers import load_golden
from test_group_act_cpu import RecEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNS = ("time_step", "goal_dist", "variance")


def test_jsrl_symbols_in_header_and_library():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    want = {"iqlhip_jsrl_create": 5, "iqlhip_jsrl_destroy": 1, "iqlhip_jsrl_act": 15, "iqlhip_jsrl_online_step": 20}
    for name, n_args in want.items():
        assert f"int {name}(" in header, name
        fn = getattr(hb.lib(), name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args, name
    assert "typedef struct iqlhip_jsrl iqlhip_jsrl;" in header


def test_jsrl_null_arguments_are_refused():
    lib = hb.lib()
    out = C.c_void_p()
    with pytest.raises(ValueError, match="NULL"):
        hb.check(lib.iqlhip_jsrl_create(None, None, None, 1, C.byref(out)))
    with pytest.raises(ValueError, match="NULL"):
        hb.check(lib.iqlhip_jsrl_destroy(None))
    with pytest.raises(ValueError, match="NULL"):
        hb.check(lib.iqlhip_jsrl_act(None, None, 17, None, None, None, None, None, None, None, 6, None, None, 0, None))


def _cfg(row):
    _, _, stage, idx, ns, ept, ats, _, _ = row
    return types.SimpleNamespace(curriculum_stage=stage, curriculum_stage_idx=int(idx), n_curriculum_stages=int(ns),
                                 ep_agent_type=ept, agent_type_stage=ats)


def test_who_from_config_reproduces_g19():
    z, meta = load_golden("g19_jsrl_selection")
    n_gate = 0
    for st in meta["sets"]:
        tag = st["tag"]
        rows, states = z[tag + ".rows"], z[tag + ".states"]
        use, horizon = z[tag + ".use_learner"], z[tag + ".horizon"]
        vmax = np.abs(horizon[rows[:, 0] == 2]).max()      # (the v tolerance is relative to the largest value)
        for i, row in enumerate(rows):
            fn = FNS[int(row[0])]
            env = types.SimpleNamespace(dist=row[8])
            who, hz = J.who_from_config(_cfg(row), fn, [int(row[1])], [states[i]], [env], goal_dist=lambda s, e: e.dist)
            w = int(who[0][0])
            if row[7]:                      # guide is None: the learner acts whatever the rule says
                w = 1
            if fn == "variance":
                assert hz[0] is None
                if w == 2:                  # the device decides: h <= stage, on the recorded variance
                    n_gate += 1
                    assert abs(horizon[i] - row[2]) >= 0.5 * 100 * 2e-5 * vmax
                    w = int(horizon[i] <= row[2])
            else:
                assert float(hz[0]) == horizon[i], (tag, i)
            assert w == use[i], (tag, i, fn)
    assert n_gate >= 20


def test_who_from_config_agent_type_draws_like_the_reference():
    cfg = types.SimpleNamespace(curriculum_stage=0.5, curriculum_stage_idx=1, n_curriculum_stages=5, ep_agent_type=0.25,
                                agent_type_stage=1.0)
    np.random.seed(3)
    got = [int(J.who_from_config(cfg, "agent_type", [t], [None], [None])[0][0][0]) for t in range(50)]
    np.random.seed(3)
    want = [int(jsrl_ref.horizon_decision("agent_type", t, cfg)[0]) for t in range(50)]
    assert got == want and 0 < sum(got) < 50
    cfg.ep_agent_type = 0.75                # above the stage, not the last stage: the guide, and no draw
    state = np.random.get_state()[1].copy()
    assert int(J.who_from_config(cfg, "agent_type", [0], [None], [None])[0][0][0]) == 0
    assert np.array_equal(np.random.get_state()[1], state)
    with pytest.raises(ValueError, match="horizon function"):
        J.who_from_config(cfg, "nope", [0], [None], [None])
    with pytest.raises(ValueError, match="goal_dist"):
        J.who_from_config(cfg, "goal_dist", [0], [None], [None])


class FakeJsrl:
    """Fixed policies (linear maps of the state) and a fixed gate, decided as the library decides."""

    def __init__(self, K, S, A, no_guide=()):
        rng = np.random.default_rng(5)
        self.L = [rng.standard_normal((S, A)).astype(np.float32) * 0.3 for _ in range(K)]
        self.G = [rng.standard_normal((S, A)).astype(np.float32) * 0.3 for _ in range(K)]
        self.V = [rng.standard_normal(S).astype(np.float32) for _ in range(K)]
        self.learners = [object()] * K
        self.guides = [None if k in no_guide else object() for k in range(K)]
        self.calls, self.modes = 0, []

    def eval(self):
        self.modes.append("eval")

    def train(self):
        self.modes.append("train")

    def gate(self, k, s):
        return np.float32(np.tanh(s @ self.V[k]))

    def act(self, states, who, gate_max):
        self.calls += 1
        out = []
        for k, s in enumerate(states):
            if s is None:
                out.append(None)
                continue
            h = self.gate(k, s)
            w = int(who[k][0]) if self.guides[k] is not None else 1
            use = w == 1 or (w == 2 and h <= np.float32(gate_max[k]))
            a = np.tanh(s @ (self.L[k] if use else self.G[k])).astype(np.float32)
            out.append((a[None], np.array([int(use)], np.int32), np.array([h], np.float32)))
        return out


@pytest.mark.parametrize("fn", ["time_step", "goal_dist", "variance", "agent_type"])
def test_eval_actors_jsrl_equals_eval_actor_per_member(fn):
    K, S, A, n_ep = 3, 9, 3, 3
    fake = FakeJsrl(K, S, A, no_guide=(2,))
    stage = {"time_step": 4.0, "goal_dist": 1.2, "variance": 0.1, "agent_type": 0.5}[fn]

    def cfgs():
        return [types.SimpleNamespace(curriculum_stage=stage, curriculum_stage_idx=1, n_curriculum_stages=5, ep_agent_type=0,
                                      agent_type_stage=1.0 if k != 1 else 0.6, max_init_horizon=(k == 2), discrete=False)
                for k in range(K)]
    dist = lambda s, env: float(np.abs(s[:2]).sum())
    envs = [RecEnv(S, A, base=3 + 5 * k) for k in range(K)]
    twins = [RecEnv(S, A, base=3 + 5 * k) for k in range(K)]
    seeds = [21, 22, 23]
    if fn == "agent_type":                  # the host draws interleave across members in lockstep: one member alone
        K = 1
        fake.learners, fake.guides = fake.learners[:1], fake.guides[:1]
        envs, twins, seeds = envs[:1], twins[:1], seeds[:1]
    np.random.seed(9)
    got = iql.eval_actors_jsrl(envs, fake, cfgs()[:K], fn, n_ep, seeds, goal_dist=dist)
    assert fake.modes == ["eval", "train"]
    np.random.seed(9)
    for k in range(K):
        value = {"goal_dist": dist, "variance": lambda s, env, k=k: fake.gate(k, s)}.get(fn)
        want = jsrl_ref.eval_member(twins[k], lambda s, k=k: np.tanh(s @ fake.L[k]).astype(np.float32),
                                    None if fake.guides[k] is None else (lambda s, k=k: np.tanh(s @ fake.G[k]).astype(np.float32)),
                                    cfgs()[k], fn, n_ep, seeds[k], value)
        assert np.array_equal(got[k][0], want[0]), k
        assert got[k][1] == want[1] and got[k][2] == want[2] and got[k][3] == want[3], (k, got[k], want)
        assert envs[k].calls == twins[k].calls, k
    if fn in ("time_step", "variance"):
        assert 0.0 < got[0][3] < 1.0        # guide and learner really mix within the episodes
    steps = max(sum(1 for c in e.calls if c[0] == "step") for e in envs)
    assert fake.calls == steps              # one act per round


def test_python_layer_checks_before_any_library_call(monkeypatch):
    def cpu_trainer(S=17, A=6):
        import torch
        actor, qf, vf = iql.GaussianPolicy(S, A, 1.0), iql.TwinQ(S, A), iql.ValueFunction(S)
        return iql.ImplicitQLearning(max_action=1.0, actor=actor, actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                     q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4), v_network=vf,
                                     v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4), max_steps=1000, device="cpu")
    monkeypatch.setattr(hb, "lib", lambda: (_ for _ in ()).throw(AssertionError("a library call was made")))
    a, b = cpu_trainer(), cpu_trainer()
    with pytest.raises(ValueError, match="one guide"):
        iql.JsrlActors([a, b], [a])
    with pytest.raises(ValueError, match="1.."):
        iql.JsrlActors([], [])
    j = iql.JsrlActors([a, b], [b, a])
    s = np.zeros(17, np.float32)
    with pytest.raises(ValueError, match="list of 2"):
        j.act([s], [0, 0])
    with pytest.raises(RuntimeError, match="GPU"):
        j.act([s, s], [0, 1])
    j._check_members = lambda: None         # past the device check: the per-row arguments
    for t in (a, b):
        t._S, t._A = 17, 6                  # (what a GPU trainer knows of its dims)
    with pytest.raises(ValueError, match="list of 2"):
        j.act([s, s], [0])
    with pytest.raises(ValueError, match="0 .guide."):
        j.act([s, s], [0, 3])
    with pytest.raises(ValueError, match="needs a gate"):
        j.act([s, s], [0, 2], gate_max=[0.0, 0.0])
    with pytest.raises(ValueError, match="who entries"):
        j.act([np.zeros((3, 17), np.float32), s], [[0, 1], 0])
    jg = iql.JsrlActors([a], [b], [b])
    jg._check_members = lambda: None
    with pytest.raises(ValueError, match="gate_max"):
        jg.act([s], [2])
    with pytest.raises(ValueError, match="whose learner"):
        a.online_step_jsrl(iql.JsrlActors([b], [a]), None, s, s[:6], 0.0, s, False, 16, s, 0)
    with pytest.raises(ValueError, match="act_next"):
        a.online_step_jsrl(iql.JsrlActors([a], [b]), None, s, s[:6], 0.0, s, False, 16, None, 0)
