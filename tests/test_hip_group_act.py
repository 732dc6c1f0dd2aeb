"""GPU tests of group policy inference (ImplicitQLearningGroup.act / actor_forward, iqlhip_group_actor_forward) and of
lockstep evaluation (eval_actors): every member's actions are — bit for bit — what a solo twin with the same parameters
and the same random-stream counters returns from actor.act / actor_forward, and the counters move exactly as the solo
calls move them.  Bad calls are refused before any counter or output moves."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth
from helpers import act_case_params, load_golden
from test_group_act_cpu import RecEnv

pytestmark = pytest.mark.gpu

DIMS = [(17, 6, True), (29, 8, False), (39, 28, True)]


def _hip():
    import iql
    import iqlhip_binding as hb
    from hip_helpers import build_hip_trainer, to_torch_batch
    return iql, hb, build_hip_trainer, to_torch_batch


def _pair(i, S, A, gaussian, precision="f32", params=None, max_action=None):
    _, _, build, _ = _hip()
    params = params or synth.synth_params(S, A, seed=600 + i, gaussian=gaussian)
    hyper = {"iql_tau": 0.6 + 0.05 * i, "beta": 2.0 + i, "discount": 0.99, "tau": 0.005 * (1 + i % 3)}
    lrs = {"v": 3e-4 * (1 + i % 4), "q": 2e-4 * (1 + i % 4), "pi": 1e-4 * (1 + i % 4)}
    ma = (1.0 + 0.25 * i) if max_action is None else max_action
    out = []
    for _ in range(2):
        t = build(params, S, A, gaussian, hyper, lrs, 1000, max_action=ma)
        if precision != "f32":
            t.set_precision(precision)
        out.append(t)
    return out


def _setup(K, S, A, gaussian, precision="f32"):
    pairs = [_pair(i, S, A, gaussian, precision) for i in range(K)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _batches(K, S, A, B, seed):
    to_torch_batch = _hip()[3]
    out = []
    for k in range(K):
        d = synth.synth_transitions(B, S, A, seed=seed + k)
        out.append(to_torch_batch({"s": d["observations"], "a": d["actions"], "r": d["rewards"],
                                   "ns": d["next_observations"], "d": d["terminals"]}))
    return out


def _train_both(group, members, twins, steps, B, seed):
    """`steps` group steps on the members, the same solo steps on the twins: the members' parameters differ from each
    other, each equals its twin's."""
    for s in range(steps):
        bs = _batches(len(members), members[0]._S, members[0]._A, B, seed + 50 * s)
        group.train(bs)
        for t, b in zip(twins, bs):
            t.train(b)


def _counters(t):
    hb = _hip()[1]
    c = (C.c_uint64 * 2)()
    hb.check(hb.lib().iqlhip_get_counters(t._ctx, c))
    return int(c[0]), int(c[1])


def _solo_acts(twins, states):
    return [None if s is None else t.actor.act(s, "cuda") for t, s in zip(twins, states)]


def _assert_acts(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g is None, (what, k)
        else:
            assert g.dtype == np.float32 and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, k)


def _modes(ts, pattern):
    for k, t in enumerate(ts):
        t.actor.train() if pattern(k) else t.actor.eval()


class _CountingLib:
    """hb.lib() stand-in that counts which library entry points are called."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        self.calls[name] = self.calls.get(name, 0) + 1
        return getattr(self._lib, name)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: f"S{d[0]}A{d[1]}{'g' if d[2] else 'd'}")
@pytest.mark.parametrize("K", [2, 4, 16])
def test_act_equals_solo_act(K, dims, precision):
    iql = _hip()[0]
    S, A, gaussian = dims
    members, twins = _setup(K, S, A, gaussian, precision)
    group = iql.ImplicitQLearningGroup(members)
    _train_both(group, members, twins, 2, 64, seed=40 + K)          # members now differ in parameters
    rng = np.random.default_rng(K * 100 + S)
    rounds = [(lambda k: False, lambda r, k: True),                # eval mode, every member
              (lambda k: True, lambda r, k: True),                 # sampling mode (Gaussian), every member
              (lambda k: k % 2 == 0, lambda r, k: (r + k) % 3 != 1),   # mixed modes, some entries None
              (lambda k: k % 3 == 1, lambda r, k: k != 0)]
    for r in range(9):
        train_mode, ask = rounds[r % len(rounds)]
        _modes(members, train_mode)
        _modes(twins, train_mode)
        states = [rng.standard_normal(S).astype(np.float32) if ask(r, k) else None for k in range(K)]
        got = group.act(states)
        _assert_acts(got, _solo_acts(twins, states), (r, precision))
        assert [_counters(t) for t in members] == [_counters(t) for t in twins], r
    if gaussian:
        assert any(_counters(t)[1] > 0 for t in members)           # the sampling rounds drew device noise


@pytest.mark.parametrize("sample", [False, True])
def test_actor_forward_uneven_rows_equals_solo(sample):
    iql = _hip()[0]
    S, A = 17, 6
    members, twins = _setup(4, S, A, True)
    group = iql.ImplicitQLearningGroup(members)
    _train_both(group, members, twins, 1, 128, seed=70)
    rng = np.random.default_rng(5)
    for rows in ([1, 4096, 0, 33], [31, 32, 700, 5000], [5000, 1, 33, 0], [0, 0, 0, 32], [0, 0, 0, 0]):
        xs = [torch.from_numpy(rng.standard_normal((n, S)).astype(np.float32)).cuda() for n in rows]
        got = group.actor_forward(xs, sample=sample)
        for k in range(4):
            want = twins[k].actor_forward(xs[k], sample=sample)
            assert got[k].shape == (rows[k], A) and got[k].device == want.device, (rows, k)
            assert torch.equal(got[k], want), (rows, k)
        assert [_counters(t) for t in members] == [_counters(t) for t in twins], rows
    if sample:      # one call number per solo call: 5000 rows are two calls
        assert _counters(members[1])[1] == 3 and _counters(members[3])[1] == 4
    # a max_action override and a host (CPU) tensor input, as the solo method takes them
    xs = [torch.from_numpy(rng.standard_normal((n, S)).astype(np.float32)) for n in (3, 0, 64, 1)]
    got = group.actor_forward(xs, sample=sample, max_action=0.5)
    for k in range(4):
        assert torch.equal(got[k], twins[k].actor_forward(xs[k], sample=sample, max_action=0.5)), k


def test_actor_forward_bf16_and_deterministic():
    iql = _hip()[0]
    for S, A, gaussian in DIMS[1:]:
        members, twins = _setup(3, S, A, gaussian, "bf16")
        group = iql.ImplicitQLearningGroup(members)
        _train_both(group, members, twins, 1, 256, seed=80)
        rng = np.random.default_rng(S)
        xs = [torch.from_numpy(rng.standard_normal((n, S)).astype(np.float32)).cuda() for n in (33, 700, 1)]
        for sample in (False, True):
            got = group.actor_forward(xs, sample=sample)
            for k in range(3):
                assert torch.equal(got[k], twins[k].actor_forward(xs[k], sample=sample)), (S, sample, k)
            assert [_counters(t) for t in members] == [_counters(t) for t in twins]


@pytest.mark.parametrize("name", ["g10_act_S17A6_gauss", "g10_act_S29A8_det", "g10_act_S39A28_gauss"])
def test_member0_matches_reference_fixture(name):
    iql = _hip()[0]
    z, meta = load_golden(name)
    S, A, gaussian = meta["S"], meta["A"], meta["gaussian"]
    params = synth.synth_params(S, A, seed=meta["seed"], gaussian=gaussian)
    params["pi"] = act_case_params(meta, z)
    m0 = _pair(0, S, A, gaussian, params=params, max_action=meta["max_action"])[0]
    others = [_pair(i, S, A, gaussian)[0] for i in (1, 2)]
    group = iql.ImplicitQLearningGroup([m0] + others)
    for t in group.trainers:
        t.actor.eval()
    tol = 2e-6 * max(1.0, meta["max_action"])
    rng = np.random.default_rng(1)
    for i in range(0, meta["n"], 5):
        a = group.act([z["states"][i], rng.standard_normal(S).astype(np.float32), None])[0]
        assert np.max(np.abs(a - z["actions_eval"][i])) <= tol, i
    x = torch.from_numpy(z["states"]).cuda()
    got = group.actor_forward([x, x[:7], x[:0]])[0].cpu().numpy()
    assert np.max(np.abs(got - z["actions_eval"])) <= tol


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_actions_follow_group_and_solo_training(precision):
    iql = _hip()[0]
    K, S, A, B, cap = 3, 29, 8, 128, 300
    members, twins = _setup(K, S, A, True, precision)
    group = iql.ImplicitQLearningGroup(members)
    tgroup = iql.ImplicitQLearningGroup(twins)
    bufs = [iql.ReplayBuffer(S, A, cap, "cuda") for _ in range(K)]
    tbufs = [iql.ReplayBuffer(S, A, cap, "cuda") for _ in range(K)]
    rng = np.random.default_rng(9)
    streams = [synth.synth_transitions(8, S, A, seed=300 + k) for k in range(K)]

    def check(what):
        for mode in (False, True):
            _modes(members, lambda k: mode)
            _modes(twins, lambda k: mode)
            states = [rng.standard_normal(S).astype(np.float32) for _ in range(K)]
            _assert_acts(group.act(states), _solo_acts(twins, states), what)
            x = [torch.from_numpy(rng.standard_normal((n, S)).astype(np.float32)).cuda() for n in (40, 1, 300)]
            got = group.actor_forward(x, sample=mode)
            for k in range(K):
                assert torch.equal(got[k], twins[k].actor_forward(x[k], sample=mode)), (what, k)
        assert [_counters(t) for t in members] == [_counters(t) for t in twins], what
        _modes(members + twins, lambda k: False)

    check("initial")
    # group online steps (the twins: solo online steps in member order)
    for it in range(5):
        tr = [(streams[k]["observations"][it], streams[k]["actions"][it], float(streams[k]["rewards"][it]),
               streams[k]["next_observations"][it], bool(streams[k]["terminals"][it])) for k in range(K)]
        np.random.seed(it)
        group.online_step(bufs, *[list(x) for x in zip(*tr)], B)
        np.random.seed(it)
        for k in range(K):
            twins[k].online_step(tbufs[k], *tr[k], B)
    check("after online_step")
    group.train_steps(bufs, 6, B, seeds=[1, 2, 3])
    tgroup.train_steps(tbufs, 6, B, seeds=[1, 2, 3])
    check("after train_steps")
    # solo training of one member between group calls
    bs = _batches(1, S, A, B, seed=77)[0]
    members[1].train(bs)
    twins[1].train(bs)
    check("after solo train")


def test_eval_actors_uses_the_group_and_equals_eval_actor(monkeypatch):
    iql, hb, _, _ = _hip()
    K, S, A = 4, 17, 6
    members, twins = _setup(K, S, A, True)
    group = iql.ImplicitQLearningGroup(members)
    _train_both(group, members, twins, 1, 64, seed=90)
    for t in members + twins:
        t.actor.train()
    envs = [RecEnv(S, A, base=3 + 7 * k) for k in range(K)]
    tenvs = [RecEnv(S, A, base=3 + 7 * k) for k in range(K)]
    seeds = [21, 22, 23, 24]
    counting = _CountingLib(hb.lib())
    monkeypatch.setattr(hb, "lib", lambda: counting)
    got = iql.eval_actors(envs, [t.actor for t in members], "cuda", 3, seeds)
    monkeypatch.undo()
    steps = sorted(sum(1 for c in e.calls if c[0] == "step") for e in envs)
    # the group path ran: one group call per round with two or more members left, a solo act() call per round with one
    assert steps[-2] < steps[-1]
    assert counting.calls.get("iqlhip_group_actor_forward", 0) == steps[-2]
    assert counting.calls.get("iqlhip_actor_forward", 0) == steps[-1] - steps[-2]
    assert counting.calls.get("iqlhip_actor_sample", 0) == 0
    assert all(t.actor.training for t in members)
    for k in range(K):
        want = iql.eval_actor(tenvs[k], twins[k].actor, "cuda", 3, seeds[k])
        assert np.array_equal(got[k][0], want[0]) and got[k][1] == want[1], k
        assert envs[k].calls == tenvs[k].calls, k
    assert [_counters(t) for t in members] == [_counters(t) for t in twins]


@pytest.mark.parametrize("trained", [False, True])
def test_eval_actors_with_actor_dropout(monkeypatch, trained):
    """Actors built with dropout (the adroit configs).  Untrained, their contexts carry no dropout rate and the group
    path runs; after one training-mode step each context keeps rate 0.1, the library refuses the group, and the
    evaluation runs per actor.  Either way the results equal eval_actor per member."""
    iql, hb, build, to_torch_batch = _hip()
    K, S, A = 3, 17, 6
    hyper = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    members = [build(synth.synth_params(S, A, seed=40 + k, gaussian=True), S, A, True, hyper, lrs, 1000, dropout=0.1)
               for k in range(K)]
    if trained:
        for t, b in zip(members, _batches(K, S, A, 64, seed=120)):
            t.actor.train()
            t.train(b)
    for t in members:
        t.actor.train()
    envs = [RecEnv(S, A, base=3 + 7 * k) for k in range(K)]
    seeds = [31, 32, 33]
    counting = _CountingLib(hb.lib())
    monkeypatch.setattr(hb, "lib", lambda: counting)
    got = iql.eval_actors(envs, [t.actor for t in members], "cuda", 2, seeds)
    monkeypatch.undo()
    steps = sorted(sum(1 for c in e.calls if c[0] == "step") for e in envs)
    if trained:
        assert counting.calls.get("iqlhip_group_actor_forward", 0) == 0
        assert counting.calls.get("iqlhip_actor_forward", 0) == sum(steps)
    else:
        assert counting.calls.get("iqlhip_group_actor_forward", 0) == steps[-2]
    assert all(t.actor.training for t in members)
    for k in range(K):           # (eval mode reads the parameters only: the same actors again)
        env = RecEnv(S, A, base=3 + 7 * k)
        want = iql.eval_actor(env, members[k].actor, "cuda", 2, seeds[k])
        assert np.array_equal(got[k][0], want[0]) and got[k][1] == want[1], k
        assert envs[k].calls == env.calls, k


def test_refusals_leave_counters_and_outputs_unchanged():
    iql, hb, _, _ = _hip()
    K, S, A = 3, 17, 6
    members, _ = _setup(K, S, A, True)
    group = iql.ImplicitQLearningGroup(members)
    for t in members:
        t.actor.train()
    rng = np.random.default_rng(2)
    group.act([rng.standard_normal(S).astype(np.float32) for _ in range(K)])       # counters at 1
    before = [_counters(t) for t in members]
    g, lib, st = group._group(), hb.lib(), members[0]._stream()
    cap = max(members[0]._max_batch, hb.IQLHIP_ACT_ROWS)
    x = torch.from_numpy(rng.standard_normal((cap + 1, S)).astype(np.float32)).cuda()
    outs = [torch.full((cap + 1, A), 7.0, device="cuda") for _ in range(K)]
    seeds = (C.c_uint64 * K)(*[members[0]._act_seed()] * K)
    max_a = (C.c_float * K)(*[1.0] * K)

    def c_call(rows, ins=None, outs_=None, ld_s=S, ld_a=A, flags=0):
        ins = ins if ins is not None else [x.data_ptr()] * K
        outs_ = outs_ if outs_ is not None else [o.data_ptr() for o in outs]
        return lib.iqlhip_group_actor_forward(g, (C.c_void_p * K)(*ins), ld_s, (C.c_int32 * K)(*rows), seeds, max_a,
                                              (C.c_void_p * K)(*outs_), ld_a, flags, st)

    for rows, kw in (([1, cap + 1, 1], {}), ([1, -1, 1], {}), ([1, 1, 1], dict(ld_s=S - 1)),
                     ([1, 1, 1], dict(ld_a=A - 1)), ([1, 1, 1], dict(ins=[x.data_ptr(), None, x.data_ptr()])),
                     ([1, 1, 1], dict(outs_=[outs[0].data_ptr(), outs[1].data_ptr(), None])),
                     ([1, 1, 1], dict(flags=2))):
        with pytest.raises(ValueError):
            hb.check(c_call(rows, **kw))
        torch.cuda.synchronize()
        assert [_counters(t) for t in members] == before, rows
        assert all(bool((o == 7.0).all()) for o in outs), rows
    # a NULL pointer is fine where a member asks for no rows
    hb.check(c_call([0, 2, 0], ins=[None, x.data_ptr(), None], outs_=[None, outs[1].data_ptr(), None],
                    flags=hb.IQLHIP_GROUP_ACT_WAIT))
    assert [_counters(t) for t in members] == [before[0], (before[1][0], before[1][1] + 1), before[2]]
    assert bool((outs[0] == 7.0).all()) and bool((outs[2] == 7.0).all()) and not bool((outs[1][:2] == 7.0).any())
    # Python-level refusals: a wrong number of entries, a member with actor dropout in training mode
    with pytest.raises(ValueError):
        group.act([None] * (K - 1))
    _, _, build, _ = _hip()
    params = synth.synth_params(S, A, seed=1, gaussian=True)
    hyper = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    dm = [build(params, S, A, True, hyper, lrs, 1000, dropout=0.1) for _ in range(2)]
    for t in dm:
        t.actor.eval()
    gd = iql.ImplicitQLearningGroup(dm)
    dm[1].actor.train()
    with pytest.raises(NotImplementedError):
        gd.act([np.zeros(S, np.float32)] * 2)
    with pytest.raises(NotImplementedError):
        gd.actor_forward([x[:3], x[:3]])
    assert [_counters(t) for t in dm] == [(0, 0), (0, 0)]


def test_group_of_one_takes_the_solo_path(monkeypatch):
    iql, hb, _, _ = _hip()
    S, A = 29, 8
    m, t = _pair(0, S, A, True)
    group = iql.ImplicitQLearningGroup([m])
    m.actor.train()
    t.actor.train()
    counting = _CountingLib(hb.lib())
    monkeypatch.setattr(hb, "lib", lambda: counting)
    rng = np.random.default_rng(4)
    s = rng.standard_normal(S).astype(np.float32)
    x = torch.from_numpy(rng.standard_normal((50, S)).astype(np.float32)).cuda()
    got_a = group.act([s])
    got_none = group.act([None])
    got_f = group.actor_forward([x], sample=True)
    monkeypatch.undo()
    assert counting.calls.get("iqlhip_group_actor_forward", 0) == 0
    assert counting.calls.get("iqlhip_actor_sample", 0) == 2
    assert got_none == [None]
    _assert_acts(got_a, [t.actor.act(s, "cuda")], "K=1")
    assert torch.equal(got_f[0], t.actor_forward(x, sample=True))
    assert _counters(m) == _counters(t)
