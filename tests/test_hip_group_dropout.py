"""GPU tests of actor dropout in trainer groups (ImplicitQLearningGroup(..., actor_dropout=True) /
iqlhip_group_create_flags with IQLHIP_GROUP_DROPOUT): every member of such a group ends exactly — bit for bit — where
a twin (a trainer built identically, with the same dropout seed, that runs the same steps alone) ends: parameters, Adam
moments, targets, losses, step counts and the library's random-stream counters, and the keep-bits the steps read.
Members may mix rates (0 included) and train() / eval() modes; injected masks are kept; a member handed back to solo
training carries its stream position on; the inference forwards stay eval-mode.  Without the opt-in the refusals
stay (tests/test_hip_group.py, test_hip_group_online.py, test_hip_group_act.py pin them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth
from helpers import assert_losses, check_step_against_golden, load_golden, single_step_inputs, step_batch

pytestmark = pytest.mark.gpu

S, A = 17, 6


def _hip():
    import iql
    import iqlhip_binding as hb
    from hip_helpers import build_hip_trainer, read_moments, read_params, to_torch_batch, unflatten_grads
    return iql, hb, build_hip_trainer, read_moments, read_params, to_torch_batch, unflatten_grads


def _spec(i, gaussian, S_=S, A_=A):
    params = synth.synth_params(S_, A_, seed=300 + i, gaussian=gaussian)
    hyper = {"iql_tau": 0.6 + 0.1 * (i % 4), "beta": 2.0 + i, "discount": 0.99, "tau": 0.005 * (1 + i)}
    lrs = {"v": 3e-4 * (1 + i), "q": 2e-4 * (1 + i), "pi": 1e-4 * (1 + i)}
    return params, hyper, lrs


def _pair(i, gaussian, p=0.1, precision="f32", S_=S, A_=A, max_steps=1000, seed=None):
    """Member i and its twin: the same parameters, dropout rate and (seed is not None) dropout seed."""
    build = _hip()[2]
    params, hyper, lrs = _spec(i, gaussian, S_, A_)
    out = []
    for _ in range(2):
        t = build(params, S_, A_, gaussian, hyper, lrs, max_steps, dropout=p)
        if precision != "f32":
            t.set_precision(precision)
        if seed is not None:
            t.set_dropout_seed(seed)
        out.append(t)
    return out


def _counters(t):
    hb = _hip()[1]
    c = (C.c_uint64 * 2)()
    hb.check(hb.lib().iqlhip_get_counters(t._ctx, c))
    return int(c[0]), int(c[1])


def _keep_bits(t, B):
    """The keep-bit words a step on B rows reads: rows < B of both layers."""
    return t.debug_read("drop_bits").view(np.uint32).reshape(2, t._max_batch, 8)[:, :B].copy()


def _assert_same_state(a, b, what=""):
    """tests/test_hip_group.py's comparison (parameters and targets, Adam moments, step counts, learning rate) plus
    the library's random-stream counters {dropout step, act() call}."""
    from test_hip_group import _assert_same_state as same
    same(a, b, what)
    assert _counters(a) == _counters(b), (what, _counters(a), _counters(b))


def _buffer(N, seed, S_=S, A_=A):
    from test_hip_group import _buffer as make
    return make(N, seed, S_, A_)


def _pi_w1(t):
    return _hip()[4](t)["pi"]["w1"]


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("B", [256, 100, 512])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("gaussian", [True, False])
@pytest.mark.parametrize("K", [2, 4])
def test_eager_dropout_group_steps_equal_solo_steps_bitwise(K, gaussian, precision, B):
    iql, _, _, _, _, to_tb, _ = _hip()
    pairs = [_pair(i, gaussian, 0.1, precision, seed=100 + i) for i in range(K)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    group = iql.ImplicitQLearningGroup(members, actor_dropout=True)
    for step in range(3):
        batches = [to_tb(step_batch(S, A, B, seed=1000 * i + step)) for i in range(K)]
        logs = group.train(batches)
        for i in range(K):
            want = twins[i].train(batches[i])
            assert logs[i] == want, (step, i, logs[i], want)
            assert np.array_equal(_keep_bits(members[i], B), _keep_bits(twins[i], B)), (step, i)
    for i in range(K):
        _assert_same_state(members[i], twins[i], f"member {i}")
        assert _counters(members[i])[0] == 3, i
    # the members' streams differ (their own seeds) and dropout is on (about a tenth of the bits are zero)
    bits = [_keep_bits(t, B) for t in members]
    assert not np.array_equal(bits[0], bits[1])
    ones = np.unpackbits(bits[0].view(np.uint8)).mean()
    assert abs(ones - 0.9) < 0.02, ones


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("shared", [True, False])
def test_device_drawn_dropout_group_steps_equal_solo_train_steps_bitwise(shared):
    """25 steps with chunk=16: two library calls (16 + 9) across which every member's dropout stream carries on."""
    iql = _hip()[0]
    K, n, B = 3, 25, 256
    pairs = [_pair(0, True, 0.1, max_steps=None, seed=7), _pair(1, True, 0.1, max_steps=None, seed=8),
             _pair(2, True, 0.1, max_steps=40, seed=9)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    bufs = _buffer(5000, 22) if shared else [_buffer(3000, 23), _buffer(4100, 24), _buffer(5000, 25)]
    seeds = [77, 78, 79]
    group = iql.ImplicitQLearningGroup(members, actor_dropout=True)
    got = group.train_steps(bufs, n, B, seeds, chunk=16)
    assert got.shape == (K, n, 3) and np.all(np.isfinite(got))
    for i in range(K):
        want = twins[i].train_steps(bufs if shared else bufs[i], n, B, seed=seeds[i])
        assert np.array_equal(got[i], want), i
        _assert_same_state(members[i], twins[i], f"member {i}")
        assert _counters(members[i])[0] == n, i


# ---------------------------------------------------------------------------------------------------------------- 3
def test_mixed_rates_and_modes_each_equal_their_solo_twin():
    """Members with p = 0.1, p = 0 (dropout layers whose rate is set to 0), p = 0.3 and p = 0.1 in eval() mode; the
    p = 0 member's twin is a trainer built without dropout layers.  Different dropout seeds: the two members that share
    everything but the seed (4 and 5) end with different actor parameters."""
    iql, _, build, _, _, to_tb, _ = _hip()
    B = 256
    pairs = [_pair(0, True, 0.1, seed=11), _pair(1, True, 0.1, seed=12), _pair(2, True, 0.3, seed=13),
             _pair(3, True, 0.1, seed=14)]
    for m in pairs[1][0].actor.modules():            # member 1: rate 0 on its dropout layers ...
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    params, hyper, lrs = _spec(1, True)
    pairs[1][1] = build(params, S, A, True, hyper, lrs, 1000, dropout=0.0)      # ... its twin has none
    for t in pairs[3]:
        t.actor.eval()
    # members 4 and 5: one specification, two dropout seeds
    pairs += [_pair(4, True, 0.1, seed=21), _pair(4, True, 0.1, seed=22)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    K = len(members)
    bufs = [_buffer(3000 + 100 * i, 80 + i) for i in range(K - 1)]
    bufs.append(bufs[4])                              # (members 4 and 5 draw the same rows: same buffer and seed)
    seeds = [5, 6, 7, 8, 9, 9]
    group = iql.ImplicitQLearningGroup(members, actor_dropout=True)
    got = group.train_steps(bufs, 6, B, seeds)
    for i in range(K):
        assert np.array_equal(got[i], twins[i].train_steps(bufs[i], 6, B, seed=seeds[i])), i
    for step in range(2):
        batches = [to_tb(step_batch(S, A, B, seed=50 * i + step)) for i in range(K - 1)]
        batches.append(batches[4])
        logs = group.train(batches)
        for i in range(K):
            assert logs[i] == twins[i].train(batches[i]), (step, i)
    for i in range(K):
        _assert_same_state(members[i], twins[i], f"member {i}")
    assert not np.array_equal(_pi_w1(members[4]), _pi_w1(members[5]))
    # the eval-mode member is where a dropout-free trainer with its parameters is
    params, hyper, lrs = _spec(3, True)
    plain = build(params, S, A, True, hyper, lrs, 1000, dropout=0.0)
    plain.train_steps(bufs[3], 6, B, seed=seeds[3])
    for step in range(2):
        plain.train(to_tb(step_batch(S, A, B, seed=50 * 3 + step)))
    assert np.array_equal(_pi_w1(members[3]), _pi_w1(plain))


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", ["g9_dropout_S39A28_gauss", "g9_dropout_S17A6_det"])
def test_injected_masks_are_kept_next_to_a_device_drawn_member(name):
    """tests/test_hip_parity.py::test_dropout_step_with_injected_masks_matches_reference with the training step taken
    inside a group: the fixture's member (the masks the reference's nn.Dropout was given, injected) next to a member
    that draws its keep-bits on the device.  The same assertions and tolerances as there."""
    iql, _, build, read_moments, read_params, to_tb, unflat = _hip()
    z, meta = load_golden(name)
    params, batch, hyper = single_step_inputs(meta)
    p = meta["dropout"]
    tr = build(params, meta["S"], meta["A"], meta["gaussian"], hyper, meta["lrs"], meta["max_steps"], dropout=p)
    assert list(tr.actor.state_dict().keys()) == meta["actor_state_keys"]
    k0, k1 = synth.synth_dropout_keep(meta["B"], p, seed=meta["seed"])
    tr.inject_dropout_masks(k0, k1)
    tb = to_tb(batch)
    grads, lw = unflat(tr, tr.flat_gradient(tb))
    info = {"value_loss": lw[0], "q_loss": lw[1], "actor_loss": lw[2], "grads": grads}
    check_step_against_golden(z, meta, info, None, None, grad_rtol=1e-5, loss_rtol=1e-5)
    other, twin = _pair(1, meta["gaussian"], 0.1, S_=meta["S"], A_=meta["A"], seed=3)
    group = iql.ImplicitQLearningGroup([other, tr], actor_dropout=True)
    ob = to_tb(step_batch(meta["S"], meta["A"], meta["B"], seed=77))
    before = _counters(tr)
    logs = group.train([ob, tb])
    log = logs[1]
    assert_losses([log["value_loss"], log["q_loss"], log["actor_loss"]], z["losses"], 1e-5)
    check_step_against_golden(z, meta, None, read_params(tr), read_moments(tr), param_atol=2e-6, moment_rtol=1e-5,
                              target_atol=1e-7)
    assert _counters(tr) == before                   # (injected masks: no draw, the stream stays where it was)
    assert logs[0] == twin.train(ob)
    _assert_same_state(other, twin, "device-drawn member")


# ---------------------------------------------------------------------------------------------------------------- 5
def test_dropout_member_handed_back_to_solo_training_continues_exactly():
    """7 group steps, 9 solo steps, 4 group steps against a twin that runs the 20 steps in one solo call: the dropout
    stream position and the cleared continuation carry over in both directions."""
    iql = _hip()[0]
    B = 256
    m, twin = _pair(0, True, 0.1, seed=31)
    other = _pair(1, True, 0.1, seed=32)[0]
    buf = _buffer(5000, 31)
    group = iql.ImplicitQLearningGroup([m, other], actor_dropout=True)
    a = [group.train_steps(buf, 7, B, [5, 6])[0], m.train_steps(buf, 9, B, seed=5),
         group.train_steps(buf, 4, B, [5, 6])[0]]
    want = twin.train_steps(buf, 20, B, seed=5)
    assert np.array_equal(np.concatenate(a), want)
    _assert_same_state(m, twin)
    assert _counters(m)[0] == 20


# ---------------------------------------------------------------------------------------------------------------- 6
def _tr(st, i):
    return (st["observations"][i], st["actions"][i], float(st["rewards"][i]), st["next_observations"][i],
            bool(st["terminals"][i]))


def test_online_dropout_group_steps_equal_solo_online_steps_bitwise():
    iql, _, _, _, read_params, _, _ = _hip()
    K, iters, B, cap = 3, 5, 256, 64
    pairs = [_pair(i, True, 0.1, seed=40 + i) for i in range(K)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    bufs = [iql.ReplayBuffer(S, A, cap, "cuda") for _ in range(K)]
    tbufs = [iql.ReplayBuffer(S, A, cap, "cuda") for _ in range(K)]
    streams = [synth.synth_transitions(iters + 1, S, A, seed=700 + k, antmaze_rewards=True) for k in range(K)]
    group = iql.ImplicitQLearningGroup(members, actor_dropout=True)
    rng_seeds = [91, 92, 93]
    rngs = [np.random.RandomState(s) for s in rng_seeds]
    logs = []
    for it in range(iters):
        args = [list(x) for x in zip(*[_tr(streams[k], it) for k in range(K)])]
        logs.append(group.online_step(bufs, *args, B, rngs=rngs))
    for k in range(K):
        np.random.seed(rng_seeds[k])
        for it in range(iters):
            want = twins[k].online_step(tbufs[k], *_tr(streams[k], it), B)
            assert logs[it][k] == want, (it, k)
    for k in range(K):
        _assert_same_state(members[k], twins[k], f"member {k}")
        assert _counters(members[k])[0] == iters, k
        assert (bufs[k]._pointer, bufs[k]._size, bufs[k]._writes) == (tbufs[k]._pointer, tbufs[k]._size, tbufs[k]._writes)
        assert torch.equal(bufs[k]._rows, tbufs[k]._rows), k
    # act_next with a member in training mode and dropout > 0: refused before anything moves (as the solo call refuses)
    before_p = [read_params(t) for t in members]
    before_c = [_counters(t) for t in members]
    before_b = [(b._pointer, b._size, b._writes, b._rows.clone()) for b in bufs]
    before_it = [t.total_it for t in members]
    trs = [_tr(streams[k], iters) for k in range(K)]
    args = [list(x) for x in zip(*trs)]
    with pytest.raises(NotImplementedError):
        group.online_step(bufs, *args, B, act_next=[trs[k][3] for k in range(K)], rngs=rngs)
    with pytest.raises(NotImplementedError):
        twins[0].online_step(tbufs[0], *trs[0], B, act_next=trs[0][3])
    torch.cuda.synchronize()
    assert [_counters(t) for t in members] == before_c and [t.total_it for t in members] == before_it
    for k in range(K):
        assert (bufs[k]._pointer, bufs[k]._size, bufs[k]._writes) == before_b[k][:3], k
        assert torch.equal(bufs[k]._rows, before_b[k][3]), k
        after = read_params(members[k])
        for n in after:
            for key in after[n]:
                assert np.array_equal(before_p[k][n][key], after[n][key]), (k, n, key)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_group_act_after_dropout_training_equals_solo_act():
    """Members that trained with dropout and are then put in eval(): their contexts still carry the rate (a plain group
    is refused by the library for it), the opt-in group's act() runs and equals the solo act() calls."""
    iql, hb, _, _, _, _, _ = _hip()
    K, B = 3, 256
    pairs = [_pair(i, True, 0.1, seed=60 + i) for i in range(K)]
    members, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    buf = _buffer(4000, 61)
    group = iql.ImplicitQLearningGroup(members, actor_dropout=True)
    group.train_steps(buf, 3, B, [1, 2, 3])
    for i in range(K):
        twins[i].train_steps(buf, 3, B, seed=i + 1)
    for t in members + twins:
        t.actor.eval()
    plain = iql.ImplicitQLearningGroup(members)
    rng = np.random.default_rng(8)
    for rnd in range(3):
        states = [rng.standard_normal(S).astype(np.float32) for _ in range(K)]
        if rnd == 1:
            states[1] = None
        got = group.act(states)
        for k in range(K):
            if states[k] is None:
                assert got[k] is None
                continue
            want = twins[k].actor.act(states[k], "cuda")
            assert got[k].shape == want.shape and np.array_equal(got[k], want), (rnd, k)
    with pytest.raises(NotImplementedError):         # (the library's refusal: the contexts' rate is 0.1)
        plain.act([np.zeros(S, np.float32)] * K)
    for k in range(K):
        _assert_same_state(members[k], twins[k], f"member {k}")
    members[2].actor.train()                         # training-mode dropout inside act(): refused, nothing moves
    before = [_counters(t) for t in members]
    with pytest.raises(NotImplementedError):
        group.act([np.zeros(S, np.float32)] * K)
    assert [_counters(t) for t in members] == before


# ---------------------------------------------------------------------------------------------------------------- 8
def test_group_create_flags_at_the_c_level():
    iql, hb, _, _, _, _, _ = _hip()
    a, b = _pair(0, True, 0.1)
    for t in (a, b):
        t._prepare(256)                              # (sends the rate to the contexts)
    lib = hb.lib()
    arr = (C.c_void_p * 2)(a._ctx.value, b._ctx.value)
    out = C.c_void_p()
    assert lib.iqlhip_group_create(arr, 2, C.byref(out)) == hb.E_UNSUPPORTED
    assert "dropout" in hb.last_error() and out.value is None
    assert lib.iqlhip_group_create_flags(arr, 2, 0, C.byref(out)) == hb.E_UNSUPPORTED and out.value is None
    assert lib.iqlhip_group_create_flags(arr, 2, hb.IQLHIP_GROUP_DROPOUT | 2, C.byref(out)) == hb.E_INVAL
    assert "flags" in hb.last_error() and out.value is None
    hb.check(lib.iqlhip_group_create_flags(arr, 2, hb.IQLHIP_GROUP_DROPOUT, C.byref(out)))
    assert out.value is not None
    hb.check(lib.iqlhip_group_destroy(out))
    assert _counters(a) == (0, 0) and _counters(b) == (0, 0)
