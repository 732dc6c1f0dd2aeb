"""GPU tests of actor dropout inside policy inference (ImplicitQLearning.set_act_dropout / iqlhip_set_act_dropout):
the keep-bits every inference call draws are the CPU reference's (tests/act_dropout_ref.py) bit for bit, the actions
are the oracle's forward under those masks, eval mode and rate 0 are untouched, the training stream is not disturbed,
online_step(act_next=...) equals online_step + act, group calls equal the members' solo calls bit for bit, the
refusals of members that have not opted in keep their place, and a re-created context carries the stream on.

Bounds.  fp32 actions: the eval-mode bound of tests/test_hip_parity.py (2e-6 * max(1, max_action)) times
1 / (1 - p)^2 — the two scaled hidden layers enlarge the activations, and so their rounding, by at most that factor.
Sampling mode adds sigma * Z_TOL * max_action for the device's float32 Box-Muller (tests/test_hip_rng_streams.py).
bf16: 5e-3 on the actions (no injection path exists for the inference keep-bits)."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth
from act_dropout_ref import act_keep_words, keep_scale
from oracle import iql_oracle as O
from oracle import philox_ref as R

pytestmark = pytest.mark.gpu

HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
SEED_HI = 0xA5A5F00D00C0FFEE          # a key with high bits set
Z_TOL = 4 * 4.7e-7                    # tests/test_hip_rng_streams.py
EVAL_BOUND = 2e-6                     # tests/test_hip_parity.py::test_actor_forward_chunks_ragged_and_after_training
BF16_BOUND = 5e-3
DIMS = [(17, 6, True), (17, 6, False), (39, 28, True), (39, 28, False)]


def _hip():
    import iql
    import iqlhip_binding as hb
    from hip_helpers import build_hip_trainer, read_moments, read_params, to_torch_batch
    return iql, hb, build_hip_trainer, read_moments, read_params, to_torch_batch


def _build(S, A, gaussian, p, seed=SEED_HI, opt_in=True, max_action=1.0, idx=0, hyper=HYPER, lrs=LRS):
    build = _hip()[2]
    params = synth.synth_params(S, A, seed=300 + idx, gaussian=gaussian)
    t = build(params, S, A, gaussian, hyper, lrs, 1000, dropout=p, max_action=max_action)
    if seed is not None:
        t.set_dropout_seed(seed)
    if opt_in:
        t.set_act_dropout(True)
    return t


def _counters(t):
    """{training dropout step, act() noise call, inference keep-bit call}"""
    hb = _hip()[1]
    c = (C.c_uint64 * 2)()
    hb.check(hb.lib().iqlhip_get_counters(t._ctx, c))
    return int(c[0]), int(c[1]), t.act_dropout_calls()


def _set_position(t, n):
    hb = _hip()[1]
    hb.check(hb.lib().iqlhip_set_act_dropout_counter(t._ctx, n))


def _act_bits(t, rows=None):
    hb = _hip()[1]
    cap = max(t._max_batch, hb.IQLHIP_ACT_ROWS)
    w = t.debug_read("act_drop_bits").view(np.uint32).reshape(2, cap, 8)
    return w.copy() if rows is None else w[:, :rows].copy()


def _train_bits(t):
    return t.debug_read("drop_bits").view(np.uint32).copy()


def _ref_actions(pi, x, words, p, max_action, noise=None):
    """oracle.actor_act with the hidden activations under the reference masks x scale."""
    f = np.float32
    masks = None
    if words is not None:
        k0, k1 = R.keep_masks(words)
        masks = (k0.astype(f) * keep_scale(p), k1.astype(f) * keep_scale(p))
    pre, _, _ = O.mlp_forward({k: v.astype(f) for k, v in pi.items() if k != "log_std"}, x.astype(f), masks)
    a = np.tanh(pre)
    if noise is not None:
        std = np.exp(np.clip(pi["log_std"].astype(f), O.LOG_STD_MIN, O.LOG_STD_MAX))
        a = a + std * np.asarray(noise, dtype=f)
    return np.clip(a * f(max_action), -max_action, max_action).astype(f)


def _assert_same_state(a, b, what="", trained=True):
    """tests/test_hip_group.py's comparison (parameters and targets, Adam moments, step counts, learning rate; trainers
    that have taken no step have no moments yet: parameters and step count only) plus the three stream positions."""
    if trained:
        from test_hip_group import _assert_same_state as same
        same(a, b, what)
    else:
        read_params = _hip()[4]
        pa, pb = read_params(a), read_params(b)
        for n in pa:
            for k in pa[n]:
                assert np.array_equal(pa[n][k], pb[n][k]), (what, n, k)
        assert a.total_it == b.total_it == 0, what
    assert _counters(a) == _counters(b), (what, _counters(a), _counters(b))


def _tr(st, i):
    return (st["observations"][i], st["actions"][i], float(st["rewards"][i]), st["next_observations"][i],
            bool(st["terminals"][i]))


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("start", [0, (1 << 32) + 5])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("S,A,gaussian", [(17, 6, True), (39, 28, False)])
def test_keep_bits_equal_reference(S, A, gaussian, p, start):
    tr = _build(S, A, gaussian, p)
    rng = np.random.default_rng(5)
    a = tr.actor.act(rng.standard_normal(S).astype(np.float32), "cuda")       # (sends the rate, allocates the buffer)
    assert a.shape == (A,) and _counters(tr)[2] == 1
    _set_position(tr, start)
    n = start
    for rows in (1, 33, 700):
        x = torch.from_numpy(rng.standard_normal((rows, S)).astype(np.float32)).cuda()
        if rows == 1:
            tr.actor.act(x[0].cpu().numpy(), "cuda")
        else:
            tr.actor_forward(x, sample=(rows == 700))
        assert np.array_equal(_act_bits(tr, rows), act_keep_words(SEED_HI, n, p, rows)), (rows, n)
        n += 1
        assert _counters(tr)[2] == n
    if p == 0.1:
        # 4097 rows are two library calls (4096 + 1): the position moves by two and the rows restart at 0
        x = torch.from_numpy(rng.standard_normal((4097, S)).astype(np.float32)).cuda()
        tr.actor_forward(x)
        assert _counters(tr)[2] == n + 2
        bits = _act_bits(tr)
        first = act_keep_words(SEED_HI, n, p, 4096)
        assert np.array_equal(bits[:, :1], act_keep_words(SEED_HI, n + 1, p, 1))
        assert np.array_equal(bits[:, 1:4096], first[:, 1:])


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("S,A,gaussian", DIMS)
def test_actions_equal_oracle_under_reference_masks(S, A, gaussian, p):
    read_params = _hip()[4]
    max_action = 2.5 if S == 39 else 1.0
    tr = _build(S, A, gaussian, p, max_action=max_action)
    pi = read_params(tr)["pi"]
    bound = EVAL_BOUND * max(1.0, max_action) / (1.0 - p) ** 2
    rng = np.random.default_rng(11)
    worst = worst_eval = worst_smp = 0.0
    for rows in (1, 33, 700):
        x = rng.standard_normal((rows, S)).astype(np.float32)
        xd = torch.from_numpy(x).cuda()
        n = _counters(tr)[2]
        got = tr.actor_forward(xd).cpu().numpy()
        words = act_keep_words(SEED_HI, n, p, rows)
        assert np.array_equal(_act_bits(tr, rows), words)
        want = _ref_actions(pi, x, words, p, max_action)
        assert got.shape == want.shape
        worst = max(worst, float(np.abs(got - want).max()))
        # dropout is on: the masked forward is not the eval-mode one
        if rows > 1:
            assert float(np.abs(want - O.actor_act(pi, x, max_action)).max()) > 1e-3
        if gaussian:
            _, call, n = _counters(tr)
            got = tr.actor_forward(xd, sample=True).cpu().numpy()
            words = act_keep_words(SEED_HI, n, p, rows)
            noise = R.act_noise(tr._act_seed(), call, rows, A)
            want = _ref_actions(pi, x, words, p, max_action, noise=noise)
            sigma = float(np.exp(np.clip(pi["log_std"], O.LOG_STD_MIN, O.LOG_STD_MAX)).max())
            err = float(np.abs(got - want).max())
            worst_smp = max(worst_smp, err)
            assert err <= bound + sigma * Z_TOL * max_action, (rows, err)
            assert _counters(tr)[1:] == (call + 1, n + 1)
        tr.actor.eval()
        ev = tr.actor_forward(xd).cpu().numpy()
        tr.actor.train()
        worst_eval = max(worst_eval, float(np.abs(ev - O.actor_act(pi, x, max_action)).max()))
    print(f"MARGIN act_dropout S={S} A={A} gaussian={gaussian} p={p} max_action={max_action}: "
          f"dropout err {worst:.3e} (bound {bound:.3e}), sampling err {worst_smp:.3e}, eval-mode err {worst_eval:.3e} "
          f"(bound {EVAL_BOUND * max(1.0, max_action):.3e})")
    assert worst <= bound, (worst, bound)


# ---------------------------------------------------------------------------------------------------------------- 3
def test_bf16_actions_and_exact_keep_bits():
    read_params = _hip()[4]
    S, A, p, rows = 39, 28, 0.1, 33
    tr = _build(S, A, True, p)
    tr.set_precision("bf16")
    pi = read_params(tr)["pi"]
    x = np.random.default_rng(12).standard_normal((rows, S)).astype(np.float32)
    n = _counters(tr)[2]
    got = tr.actor_forward(torch.from_numpy(x).cuda()).cpu().numpy()
    words = act_keep_words(SEED_HI, n, p, rows)
    assert np.array_equal(_act_bits(tr, rows), words)
    err = float(np.abs(got - _ref_actions(pi, x, words, p, 1.0)).max())
    print(f"MARGIN act_dropout bf16 S={S} A={A} p={p} rows={rows}: err {err:.3e} (bound {BF16_BOUND:.1e})")
    assert err <= BF16_BOUND, err
    assert _counters(tr)[2] == n + 1


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("S,A,gaussian", [(17, 6, True), (39, 28, False)])
def test_eval_mode_and_rate_zero_are_untouched(S, A, gaussian):
    rng = np.random.default_rng(13)
    x = torch.from_numpy(rng.standard_normal((33, S)).astype(np.float32)).cuda()
    s = rng.standard_normal(S).astype(np.float32)
    # eval mode: an opted-in trainer against a twin that never opted in
    a, b = _build(S, A, gaussian, 0.1), _build(S, A, gaussian, 0.1, opt_in=False)
    for t in (a, b):
        t.actor.eval()
    # rate 0 in training mode (a Gaussian policy samples: both noise streams are at the same position)
    c, d = _build(S, A, gaussian, 0.0), _build(S, A, gaussian, 0.0, opt_in=False)
    e, f = _build(S, A, gaussian, 0.1), _build(S, A, gaussian, 0.1, opt_in=False)
    for t in (e, f):
        for m in t.actor.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
    for u, v in ((a, b), (c, d), (e, f)):
        for _ in range(2):
            assert np.array_equal(u.actor.act(s, "cuda"), v.actor.act(s, "cuda"))
            assert torch.equal(u.actor_forward(x), v.actor_forward(x))
            assert torch.equal(u.actor_forward(x, sample=True), v.actor_forward(x, sample=True))
        assert _counters(u) == _counters(v) and _counters(u)[2] == 0


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("gaussian", [True, False])
def test_training_stream_is_not_disturbed(gaussian):
    iql, _, _, read_moments, read_params, _ = _hip()
    S, A, B, cap, iters = 17, 6, 256, 64, 4
    a, b = _build(S, A, gaussian, 0.1), _build(S, A, gaussian, 0.1, opt_in=False)
    bufs = [iql.ReplayBuffer(S, A, cap, "cuda") for _ in range(2)]
    st = synth.synth_transitions(iters, S, A, seed=701, antmaze_rewards=True)
    logs = [[], []]
    for j, t in enumerate((a, b)):
        np.random.seed(17)
        for it in range(iters):
            if j == 0:
                log, act = t.online_step(bufs[j], *_tr(st, it), B, act_next=_tr(st, it)[3])
                assert act.shape == (A,)
            else:
                log = t.online_step(bufs[j], *_tr(st, it), B)
            logs[j].append(log)
    assert logs[0] == logs[1]
    assert _counters(a)[2] == iters and _counters(b)[2] == 0 and _counters(a)[0] == _counters(b)[0] == iters

    def same_training_state():
        from test_hip_group import _assert_same_state as same
        same(a, b)                                                            # parameters, targets, moments, step counts
        assert np.array_equal(_train_bits(a), _train_bits(b))
        assert _counters(a)[0] == _counters(b)[0]
    same_training_state()
    # train_steps calls (chunk graphs pre-draw the next step's keep-bits) interleaved with opted-in act() calls
    from test_hip_group import _buffer
    buf = _buffer(3000, 31, S, A)
    s = np.random.default_rng(3).standard_normal(S).astype(np.float32)
    got = []
    for n in (6, 2, 5):
        got.append((a.train_steps(buf, n, B, seed=9), b.train_steps(buf, n, B, seed=9)))
        a.actor.act(s, "cuda")
        a.actor_forward(torch.from_numpy(np.tile(s, (40, 1))).cuda())
    for x, y in got:
        assert np.array_equal(x, y)
    same_training_state()
    assert _counters(a)[2] == iters + 6


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("S,A,gaussian", [(17, 6, True), (39, 28, False)])
def test_online_step_act_next_equals_online_step_then_act(S, A, gaussian):
    iql = _hip()[0]
    B, cap, iters = 256, 64, 3
    a, b = _build(S, A, gaussian, 0.1), _build(S, A, gaussian, 0.1)
    bufs = [iql.ReplayBuffer(S, A, cap, "cuda") for _ in range(2)]
    st = synth.synth_transitions(iters, S, A, seed=702, antmaze_rewards=True)
    out = [[], []]
    for j, t in enumerate((a, b)):
        np.random.seed(18)
        for it in range(iters):
            tr = _tr(st, it)
            if j == 0:
                log, act = t.online_step(bufs[j], *tr, B, act_next=tr[3])
            else:
                log = t.online_step(bufs[j], *tr, B)
                act = t.actor.act(tr[3], "cuda")
            out[j].append((log, act))
    for (la, aa), (lb, ab) in zip(*out):
        assert la == lb and aa.dtype == ab.dtype and np.array_equal(aa, ab)
    _assert_same_state(a, b)
    assert _counters(a)[2] == iters and _counters(a)[1] == (iters if gaussian else 0)
    assert np.array_equal(_act_bits(a, 1), act_keep_words(SEED_HI, iters - 1, 0.1, 1))


# ---------------------------------------------------------------------------------------------------------------- 7
def _group_pairs(gaussian, S=17, A=6):
    """Members 0..3 and their solo twins: p = 0.1; p = 0.1 in eval(); rate 0 on its dropout layers; p = 0.3."""
    pairs = []
    for i, p in enumerate((0.1, 0.1, 0.1, 0.3)):
        hyper = dict(HYPER, beta=2.0 + i)
        pairs.append([_build(S, A, gaussian, p, seed=SEED_HI + i, idx=i, hyper=hyper) for _ in range(2)])
    for t in pairs[1]:
        t.actor.eval()
    for t in pairs[2]:
        for m in t.actor.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
    return [p[0] for p in pairs], [p[1] for p in pairs]


@pytest.mark.parametrize("gaussian", [True, False])
def test_group_inference_equals_solo_bitwise(gaussian):
    iql = _hip()[0]
    S, A, K = 17, 6, 4
    members, twins = _group_pairs(gaussian)
    group = iql.ImplicitQLearningGroup(members, actor_dropout=True)
    rng = np.random.default_rng(21)
    for rnd in range(3):
        states = [rng.standard_normal(S).astype(np.float32) for _ in range(K)]
        if rnd == 1:
            states[3] = None
        got = group.act(states)
        for k in range(K):
            if states[k] is None:
                assert got[k] is None
                continue
            want = twins[k].actor.act(states[k], "cuda")
            assert np.array_equal(got[k], want), (rnd, k)
            if twins[k].acts_with_dropout():
                assert np.array_equal(_act_bits(members[k], 1), _act_bits(twins[k], 1)), (rnd, k)
    assert [_counters(t)[2] for t in members] == [3, 0, 0, 2]
    for sample in (False, True):
        xs = [torch.from_numpy(rng.standard_normal((n, S)).astype(np.float32)).cuda() for n in (1, 33, 0, 5)]
        outs = group.actor_forward(xs, sample=sample)
        for k in range(K):
            want = twins[k].actor_forward(xs[k], sample=sample)
            assert outs[k].shape == want.shape and torch.equal(outs[k], want), (sample, k)
    for k in range(K):
        _assert_same_state(members[k], twins[k], f"member {k}", trained=False)
    assert [_counters(t)[2] for t in members] == [5, 0, 0, 4]
    assert np.array_equal(_act_bits(members[3], 5), act_keep_words(SEED_HI + 3, 3, 0.3, 5))


@pytest.mark.parametrize("S,A,gaussian", [(17, 6, True), (39, 28, False)])
def test_group_online_step_act_next_equals_solo_bitwise(S, A, gaussian):
    iql = _hip()[0]
    K, iters, B, cap = 4, 3, 256, 64
    members, twins = _group_pairs(gaussian, S, A)
    bufs = [iql.ReplayBuffer(S, A, cap, "cuda") for _ in range(K)]
    tbufs = [iql.ReplayBuffer(S, A, cap, "cuda") for _ in range(K)]
    streams = [synth.synth_transitions(iters, S, A, seed=710 + k, antmaze_rewards=True) for k in range(K)]
    group = iql.ImplicitQLearningGroup(members, actor_dropout=True)
    rng_seeds = [91, 92, 93, 94]
    rngs = [np.random.RandomState(s) for s in rng_seeds]
    res = []
    for it in range(iters):
        trs = [_tr(streams[k], it) for k in range(K)]
        act_next = [trs[k][3] for k in range(K)]
        if it == 1:
            act_next[0] = None
        res.append((group.online_step(bufs, *[list(x) for x in zip(*trs)], B, act_next=act_next, rngs=rngs), act_next))
    for k in range(K):
        np.random.seed(rng_seeds[k])
        for it in range(iters):
            (logs, acts), act_next = res[it]
            if act_next[k] is None:
                want = twins[k].online_step(tbufs[k], *_tr(streams[k], it), B)
                assert acts[k] is None and logs[k] == want, (it, k)
            else:
                want, wa = twins[k].online_step(tbufs[k], *_tr(streams[k], it), B, act_next=act_next[k])
                assert logs[k] == want and np.array_equal(acts[k], wa), (it, k)
    for k in range(K):
        _assert_same_state(members[k], twins[k], f"member {k}")
        assert torch.equal(bufs[k]._rows, tbufs[k]._rows), k
    assert [_counters(t)[2] for t in members] == [2, 0, 0, 3]
    assert np.array_equal(_act_bits(members[3], 1), _act_bits(twins[3], 1))


# ---------------------------------------------------------------------------------------------------------------- 8
def test_refusals_keep_their_place():
    iql, _, _, _, read_params, _ = _hip()
    S, A, K, B, cap = 17, 6, 3, 256, 64
    members = [_build(S, A, True, 0.1, seed=50 + i, idx=i, opt_in=(i != 1)) for i in range(K)]
    group = iql.ImplicitQLearningGroup(members, actor_dropout=True)
    bufs = [iql.ReplayBuffer(S, A, cap, "cuda") for _ in range(K)]
    st = [synth.synth_transitions(2, S, A, seed=720 + k, antmaze_rewards=True) for k in range(K)]
    rngs = [np.random.RandomState(5 + k) for k in range(K)]
    trs = [_tr(st[k], 0) for k in range(K)]
    group.online_step(bufs, *[list(x) for x in zip(*trs)], B, rngs=rngs)      # (a call without actions runs)
    assert group.act([trs[0][3], None, trs[2][3]])[1] is None                 # (... and the opted-in members act)

    def snapshot():
        return ([_counters(t) for t in members], [t.total_it for t in members],
                [(b._pointer, b._size, b._writes, b._rows.clone()) for b in bufs], [read_params(t) for t in members],
                [_train_bits(t) for t in members], [_act_bits(t) for t in (members[0], members[2])])

    def assert_unchanged(before):
        torch.cuda.synchronize()
        after = snapshot()
        assert after[0] == before[0] and after[1] == before[1]
        for x, y in zip(before[2], after[2]):
            assert x[:3] == y[:3] and torch.equal(x[3], y[3])
        for x, y in zip(before[3], after[3]):
            for n in x:
                for key in x[n]:
                    assert np.array_equal(x[n][key], y[n][key]), (n, key)
        for x, y in zip(before[4] + before[5], after[4] + after[5]):
            assert np.array_equal(x, y)

    before = snapshot()
    trs = [_tr(st[k], 1) for k in range(K)]
    with pytest.raises(NotImplementedError):
        group.act([trs[k][3] for k in range(K)])
    with pytest.raises(NotImplementedError):
        group.online_step(bufs, *[list(x) for x in zip(*trs)], B, act_next=[trs[k][3] for k in range(K)], rngs=rngs)
    with pytest.raises(NotImplementedError):
        members[1].online_step(bufs[1], *trs[1], B, act_next=trs[1][3])
    assert_unchanged(before)
    # the member that has not opted in still acts through its PyTorch modules
    calls = []
    members[1].act_one = lambda *a, **k: calls.append(1)
    assert members[1].actor.act(trs[1][3], "cuda").shape == (A,) and not calls
    # a group built without actor_dropout=True refuses a training-mode dropout member, opted in or not
    with pytest.raises(NotImplementedError):
        iql.ImplicitQLearningGroup([members[0], members[2]])


# ---------------------------------------------------------------------------------------------------------------- 9
def test_context_recreation_carries_position_rate_and_key():
    _, _, _, _, _, to_tb = _hip()
    from helpers import step_batch
    S, A, p = 17, 6, 0.1
    tr = _build(S, A, True, p)
    rng = np.random.default_rng(31)
    for _ in range(3):
        tr.actor.act(rng.standard_normal(S).astype(np.float32), "cuda")
    before = _counters(tr)
    assert before[2] == 3 and tr._max_batch == 256
    ctx = tr._ctx.value
    tr.train(to_tb(step_batch(S, A, 600, seed=4)))                            # a batch past max_batch: a new context
    assert tr._ctx.value != ctx and tr._max_batch >= 600
    assert _counters(tr) == (before[0] + 1, before[1], 3)
    x = torch.from_numpy(rng.standard_normal((33, S)).astype(np.float32)).cuda()
    tr.actor_forward(x)
    assert np.array_equal(_act_bits(tr, 33), act_keep_words(SEED_HI, 3, p, 33))
    assert _counters(tr)[2] == 4
