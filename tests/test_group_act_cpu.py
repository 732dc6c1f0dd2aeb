"""CPU-only tests of group policy inference and lockstep evaluation (no GPU in the process): the library exports
iqlhip_group_actor_forward and refuses NULL arguments before any device work; ImplicitQLearningGroup.act /
actor_forward check their arguments; eval_actors equals eval_actor per member — returns, success rates, each env's
call sequence — on its per-actor fallback with PyTorch actors."""
import ctypes as C

import numpy as np
import pytest
import torch

import iql
import iql_offline
import iqlhip_binding as hb


class RecEnv:
    """A stand-in env that records every call made to it.  Dynamics depend on the action (so the actor matters);
    episode lengths differ by env (`base`) and episode."""

    def __init__(self, S, A, base, seed_offset=0):
        self.S, self.A, self.base, self.off = S, A, base, seed_offset
        self.calls = []
        self.rng = None
        self.M = np.random.default_rng(1000 + base).standard_normal((A, S)).astype(np.float32) * 0.2
        self.episode = 0

    def seed(self, s):
        self.calls.append(("seed", int(s)))
        self.rng = np.random.default_rng(int(s) + self.off)

    def reset(self):
        self.calls.append(("reset",))
        self.s = self.rng.standard_normal(self.S).astype(np.float32)
        self.t = 0
        self.len = self.base + 2 * (self.episode % 3) + int(self.rng.integers(0, 3))
        self.episode += 1
        return self.s

    def step(self, a):
        a = np.asarray(a, dtype=np.float32)
        self.calls.append(("step", a.tobytes()))
        self.s = (0.9 * self.s + a @ self.M).astype(np.float32)
        self.t += 1
        r = float(-np.abs(self.s[:2]).sum())
        info = {"success": bool(self.s[0] > 0.5)} if self.base % 2 else {}
        return self.s, r, self.t >= self.len, info


def _cpu_trainer(S=17, A=6):
    actor = iql.GaussianPolicy(S, A, 1.0)
    qf, vf = iql.TwinQ(S, A), iql.ValueFunction(S)
    return iql.ImplicitQLearning(max_action=1.0, actor=actor,
                                 actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                 q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                                 v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 max_steps=1000, device="cpu")


def test_group_actor_forward_symbol_is_exported():
    fn = hb.lib().iqlhip_group_actor_forward
    assert fn.restype is C.c_int and len(fn.argtypes) == 10


def test_group_actor_forward_rejects_null_arguments():
    lib = hb.lib()
    K = 2
    ins = (C.c_void_p * K)(4096, 8192)          # never dereferenced: every call below is refused first
    outs = (C.c_void_p * K)(4096, 8192)
    rows = (C.c_int32 * K)(1, 1)
    seeds = (C.c_uint64 * K)(0, 0)
    max_a = (C.c_float * K)(1.0, 1.0)
    full = dict(g=None, ins=ins, ld_s=17, rows=rows, seeds=seeds, max_a=max_a, outs=outs, ld_a=6, flags=0, st=None)

    def call(**kw):
        a = dict(full, **kw)
        return lib.iqlhip_group_actor_forward(*a.values())

    for kw in ({}, dict(g=1, ins=None), dict(g=1, rows=None), dict(g=1, seeds=None), dict(g=1, max_a=None),
               dict(g=1, outs=None)):
        with pytest.raises(ValueError, match="NULL"):
            hb.check(call(**kw))


def test_group_act_checks_its_arguments_first():
    a, b = _cpu_trainer(), _cpu_trainer()
    for name in ("act", "actor_forward"):
        assert callable(getattr(iql.ImplicitQLearningGroup, name, None))
    assert callable(getattr(iql_offline.ImplicitQLearningGroup, "act", None))
    g = object.__new__(iql.ImplicitQLearningGroup)      # a group of CPU trainers cannot be formed at all
    g.trainers, g._g, g._ctxs, g._act_bufs = [a, b], None, None, None
    s = np.zeros(17, np.float32)
    with pytest.raises(ValueError, match="list of 2"):
        g.act([s])                                      # a bad number of entries
    with pytest.raises(ValueError, match="list of 2"):
        g.act(s)
    with pytest.raises(ValueError, match="list of 2"):
        g.actor_forward([torch.zeros(3, 17)] * 3)
    with pytest.raises(RuntimeError, match="GPU"):      # then the members
        g.act([s, s])
    with pytest.raises(RuntimeError, match="GPU"):
        g.actor_forward([torch.zeros(3, 17)] * 2)


def _actors(K, S, A, seed=0):
    torch.manual_seed(seed)
    out = []
    for k in range(K):
        if k % 2:
            out.append(iql.DeterministicPolicy(S, A, 1.0 + 0.5 * k))
        else:
            p = iql.GaussianPolicy(S, A, 1.0 + 0.5 * k)
            with torch.no_grad():
                p.log_std.fill_(-0.5)
            out.append(p)
    return out


@pytest.mark.parametrize("n_episodes", [0, 1, 3])
def test_eval_actors_equals_eval_actor_per_member(n_episodes):
    K, S, A = 4, 9, 3
    actors = _actors(K, S, A)
    actors[1].eval()                                   # any starting mode: eval_actor leaves every actor training
    seeds = [11, 12, 13, 14]
    envs = [RecEnv(S, A, base=3 + 7 * k) for k in range(K)]
    twins = [RecEnv(S, A, base=3 + 7 * k) for k in range(K)]
    with _nowarn():
        got = iql.eval_actors(envs, actors, "cpu", n_episodes, seeds)
    assert all(a.training for a in actors)
    assert len(got) == K
    for k in range(K):
        with _nowarn():
            want = iql.eval_actor(twins[k], actors[k], "cpu", n_episodes, seeds[k])
        assert np.array_equal(got[k][0], want[0]), k
        assert np.array_equal(got[k][1], want[1], equal_nan=True), k
        assert envs[k].calls == twins[k].calls, k
        assert len(envs[k].calls) > 1 + n_episodes or n_episodes == 0
    if n_episodes:
        lens = [sum(1 for c in e.calls if c[0] == "step") for e in envs]
        assert len(set(lens)) == K                     # members really finish in different rounds


def test_eval_actors_offline_flavour_returns_the_returns():
    K, S, A = 3, 9, 3
    actors = _actors(K, S, A, seed=1)
    envs = [RecEnv(S, A, base=4 + k) for k in range(K)]
    twins = [RecEnv(S, A, base=4 + k) for k in range(K)]
    got = iql_offline.eval_actors(envs, actors, "cpu", 2, [5, 6, 7])
    for k in range(K):
        assert np.array_equal(got[k], iql_offline.eval_actor(twins[k], actors[k], "cpu", 2, [5, 6, 7][k]))
        assert envs[k].calls == twins[k].calls


def test_eval_actors_rejects_mismatched_lists():
    actors = _actors(2, 9, 3)
    with pytest.raises(ValueError):
        iql.eval_actors([RecEnv(9, 3, 3)], actors, "cpu", 1, [1, 2])
    with pytest.raises(ValueError):
        iql.eval_actors([RecEnv(9, 3, 3), RecEnv(9, 3, 3)], actors, "cpu", 1, [1])


class _nowarn:
    """np.mean of no successes (n_episodes = 0) warns, as in eval_actor; the comparison does not care."""

    def __enter__(self):
        import warnings
        self._w = warnings.catch_warnings()
        self._w.__enter__()
        warnings.simplefilter("ignore", RuntimeWarning)

    def __exit__(self, *exc):
        return self._w.__exit__(*exc)
