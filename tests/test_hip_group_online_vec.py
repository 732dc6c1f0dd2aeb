"""GPU tests of ImplicitQLearningGroup.online_step_vec (DESIGN.md 6b "Group vector-environment online step"): E_k
transitions, U gradient steps and the actions of E2_k states for every member in one library call, against twins — solo
trainers from the same seeds that make the solo online_step_vec calls in member order under the same numpy seed (or,
with rngs, each under its own generator's seed).  Everything compared is compared bitwise: ring contents and counters,
parameters, targets, Adam state, the schedule, total_it, the random-stream counters, per-step logs and statistics, the
clip record and the actions.  (S, A) = (3, 2) and (17, 6): row strides of 12 and 44 floats, 3 and 11 float4 per row, so
rows straddle the gather's 256-thread blocks; E_k, B_k and E2_k differ between members, so grid.x is one member's and the
others' blocks past their work must store nothing."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu

DIMS = [(3, 2), (17, 6)]
CAP = 40
ES = (1, 5, 8)              # new rows per call, per member
STARTS = (37, 25, 16)       # rows in each 40-row ring before the first call: six calls take every write across the wrap
E2S = (3, None, 6)          # act states per call, per member (None: that member asks for no action)
SEED = 7                    # np.random.seed of every comparison (and the base of the per-member generators' seeds): in
                            # every test every member draws one of its own new rows in some iteration (asserted in _run;
                            # seeds 3 and 5 miss one for the one-row member)


def _hip():
    import hip_helpers as H
    import iql
    import iqlhip_binding as hb
    return iql, hb, H


@functools.lru_cache(maxsize=None)
def _params(k, S, A, gaussian):
    return synth.synth_params(S, A, seed=500 + k, gaussian=gaussian)


@functools.lru_cache(maxsize=None)
def _data(k, S, A, n=700):
    d = synth.synth_transitions(n, S, A, seed=32 + k)
    return (d["observations"], d["actions"], d["rewards"].astype(np.float32), d["next_observations"],
            d["terminals"].astype(np.float32))


def _block(k, S, A, lo, n):
    """Transitions lo .. lo + n - 1 of member k's stream, as online_step_vec takes them."""
    return tuple(x[lo: lo + n] for x in _data(k, S, A))


def _build(k, S, A, gaussian=True, bf16=False, stats=False, clip=None, train_mode=True, dropout=0.0, act_dropout=False):
    hyper = {"iql_tau": 0.6 + 0.05 * k, "beta": 2.0 + k, "discount": 0.99, "tau": 0.005 * (1 + k % 3), "deterministic": not gaussian}
    lrs = {"v": 3e-4 * (1 + k % 4), "q": 2e-4 * (1 + k % 4), "pi": 1e-4 * (1 + k % 4)}
    tr = _hip()[2].build_hip_trainer(_params(k, S, A, gaussian), S, A, gaussian, hyper, lrs, 1000, dropout=dropout)
    if dropout:
        tr.set_dropout_seed(40 + k)
    if bf16:
        tr.set_precision("bf16")
    tr.set_step_stats(stats)
    tr.set_grad_clip(clip)
    tr.set_act_dropout(act_dropout)
    tr.actor.train(train_mode)
    return tr


def _ring(k, S, A, cap, prefill):
    ring = _hip()[0].ReplayBuffer(S, A, cap, "cuda")
    for lo in range(0, prefill, 64):
        ring.add_transitions(*_block(k, S, A, 400 + lo, min(64, prefill - lo)))
    return ring


def _counters(tr):
    hb = _hip()[1]
    out = (C.c_uint64 * 2)()
    hb.check(hb.lib().iqlhip_get_counters(tr._ctx, out))
    return int(out[0]), int(out[1]), tr.act_dropout_calls()


def _same_ring(a, b):
    assert (a._pointer, a._size, a._writes) == (b._pointer, b._size, b._writes)
    assert torch.equal(a._rows, b._rows)


def _new_rows_drawn(caps, starts, Es, Bs, U, iters, seed, per_member):
    """From numpy alone: per member, whether in some iteration one of its U * B_k indices falls into its E_k new slots.
    The draws are the call's: member order inside an iteration on the global stream, or — per_member — member k's own
    generator, seeded seed + k."""
    K = len(Es)
    gens = [np.random.RandomState(seed + k) for k in range(K)] if per_member else [np.random.RandomState(seed)] * K
    size, pointer, hit = list(starts), [s % c for s, c in zip(starts, caps)], [False] * K
    for _ in range(iters):
        for k in range(K):
            size[k] = min(size[k] + Es[k], caps[k])
            idx = np.concatenate([gens[k].randint(0, size[k], size=Bs[k]) for _ in range(U)])
            hit[k] = hit[k] or bool((((idx - pointer[k]) % caps[k]) < Es[k]).any())
            pointer[k] = (pointer[k] + Es[k]) % caps[k]
    return hit


def _run(S, A, K, U, iters=6, Bs=24, cap=CAP, Es=ES, starts=STARTS, E2s=E2S, per_member=False, group_kw=None, **kw):
    """`iters` group calls against the twins' solo calls; returns (group, members, twins, rings, twin rings, results)."""
    iql, hb, H = _hip()
    Es, starts, E2s = Es[:K], starts[:K], E2s[:K]
    Bl = [Bs] * K if isinstance(Bs, int) else list(Bs)
    members, twins = [_build(k, S, A, **kw) for k in range(K)], [_build(k, S, A, **kw) for k in range(K)]
    rings, trings = [_ring(k, S, A, cap, starts[k]) for k in range(K)], [_ring(k, S, A, cap, starts[k]) for k in range(K)]
    group = iql.ImplicitQLearningGroup(members, **(group_kw or {}))
    if U:
        assert all(_new_rows_drawn([cap] * K, starts, Es, Bl, U, iters, SEED, per_member)), "no new row drawn: pick another seed"
    blocks = [[_block(k, S, A, Es[k] * it, Es[k]) for k in range(K)] for it in range(iters)]
    acts = [[None if E2s[k] is None else _block(k, S, A, 300 + 7 * it, E2s[k])[0] for k in range(K)] for it in range(iters)]
    with_act = any(e is not None for e in E2s)
    rngs = [np.random.RandomState(SEED + k) for k in range(K)] if per_member else None
    np.random.seed(SEED)
    got = [group.online_step_vec(rings, *([b[j] for b in blocks[it]] for j in range(5)), Bs, updates=U,
                                 act_next=acts[it] if with_act else None, rngs=rngs) for it in range(iters)]
    want = [[None] * K for _ in range(iters)]

    def solo(it, k):
        want[it][k] = twins[k].online_step_vec(trings[k], *blocks[it][k], Bl[k], updates=U, act_next=acts[it][k])

    if per_member:
        for k in range(K):
            np.random.seed(SEED + k)
            for it in range(iters):
                solo(it, k)
    else:
        np.random.seed(SEED)
        for it in range(iters):
            for k in range(K):
                solo(it, k)
    for it in range(iters):
        logs, actions = got[it] if with_act else (got[it], [None] * K)
        assert len(logs) == K and len(actions) == K
        for k in range(K):
            w_logs, w_act = want[it][k] if E2s[k] is not None else (want[it][k], None)
            assert isinstance(logs[k], list) and len(logs[k]) == U
            assert logs[k] == w_logs, (it, k, logs[k], w_logs)
            assert all(np.isfinite(v) for log in w_logs for v in log.values())
            if w_act is None:
                assert actions[k] is None
            else:
                assert actions[k].shape == (E2s[k], A) and actions[k].dtype == np.float32
                assert np.array_equal(actions[k], w_act), (it, k)
    for k in range(K):
        g, t = members[k], twins[k]
        if g.total_it:
            H.assert_same_trainer_state(g, t, f"member {k}: the group call vs its solo calls")
        else:          # (no step has run: the optimizers hold no state to read yet; the arenas are what was loaded)
            assert (g.total_it, g._adam_t) == (t.total_it, t._adam_t) and np.array_equal(H.arenas(g), H.arenas(t))
        assert g.total_it == iters * U and g._adam_t == t._adam_t
        assert g.actor_optimizer.param_groups[0]["lr"] == t.actor_optimizer.param_groups[0]["lr"]
        assert (g.actor_lr_schedule.last_epoch, g.actor_lr_schedule._step_count) == \
               (t.actor_lr_schedule.last_epoch, t.actor_lr_schedule._step_count)
        _same_ring(rings[k], trings[k])
        assert _counters(g) == _counters(t), k
    return group, members, twins, rings, trings, got


# ---- 1. six iterations across the wrap, unequal E_k and E2_k, one member without an action -----------------------------
@pytest.mark.parametrize("S,A", DIMS)
@pytest.mark.parametrize("U", [0, 1, 3])
def test_three_members_equal_their_solo_calls_across_the_wrap(S, A, U):
    _, members, _, rings, _, got = _run(S, A, 3, U)
    for k, ring in enumerate(rings):
        assert STARTS[k] < CAP < STARTS[k] + 6 * ES[k] == ring._writes          # every member's write has crossed the wrap
        assert ring._pointer == (STARTS[k] + 6 * ES[k]) % CAP and ring._size == CAP
    assert [_counters(m)[1] for m in members] == [6, 0, 6]          # the act() noise counter: once per call that samples
    if U == 0:
        assert all(logs == [[], [], []] for logs, _ in got)


@pytest.mark.parametrize("S,A", DIMS)
def test_eval_mode_members_act_with_the_mean(S, A):
    _, members, _, _, _, _ = _run(S, A, 2, 1, train_mode=False)
    assert [_counters(m)[1] for m in members] == [0, 0]


def test_deterministic_policy():
    _run(17, 6, 2, 3, iters=3, gaussian=False)


# ---- 2. 64-row batches on a larger ring, staging slices beyond the first; the members' own generators ------------------
@pytest.mark.parametrize("S,A", DIMS)
@pytest.mark.parametrize("per_member", [False, True], ids=["global", "rngs"])
def test_two_members_on_larger_rings(S, A, per_member):
    _run(S, A, 2, 2, iters=3, Bs=64, cap=300, Es=(8, 3), starts=(100, 120), E2s=(5, 2), per_member=per_member)


def test_generators_of_their_own_at_the_wrap():
    _run(3, 2, 3, 3, per_member=True)


# ---- 3. options --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,A", DIMS)
def test_mixed_batch_group(S, A):
    _run(S, A, 2, 3, iters=4, Bs=(16, 40), Es=(5, 8), starts=(25, 16), E2s=(None, 4), group_kw={"mixed_batch": True})


@pytest.mark.parametrize("S,A", DIMS)
def test_statistics_of_every_step_for_every_member(S, A):
    iql, hb, H = _hip()
    group, members, _, _, _, got = _run(S, A, 3, 3, iters=3, E2s=(None, None, None), stats=True)
    for logs in got:
        for member in logs:
            assert all(len(log) == 19 for log in member)
            assert member[0] != member[1] and member[1] != member[2]          # every dict carries its own step's numbers
    # ... and the ring the library keeps holds the last call's: step u of member k in slot u
    out = (C.c_float * (3 * 3 * hb.IQLHIP_N_STATS))()
    hb.check(hb.lib().iqlhip_group_read_step_stats(group._g, out, 3, members[0]._stream()))
    ring = np.frombuffer(out, dtype=np.float32).reshape(3, 3, hb.IQLHIP_N_STATS)
    for k in range(3):
        for u in range(3):
            assert [float(x) for x in ring[u, k]] == [got[-1][k][u]["stats/" + n] for n in hb.STAT_NAMES]


@pytest.mark.parametrize("S,A", DIMS)
def test_gradient_clipping(S, A):
    _, members, twins, _, _, _ = _run(S, A, 3, 3, iters=3, clip=1.0)
    for g, t in zip(members, twins):
        assert g.last_grad_clip() == t.last_grad_clip()


@pytest.mark.parametrize("S,A", DIMS)
def test_actor_dropout_in_the_steps_and_in_the_act(S, A):
    _, members, _, _, _, _ = _run(S, A, 3, 3, iters=3, dropout=0.1, act_dropout=True, group_kw={"actor_dropout": True})
    # keep-bit draws: one per step; noise and act keep-bits: one per call of a member that asked for actions
    assert [_counters(m) for m in members] == [(9, 3, 3), (9, 0, 0), (9, 3, 3)]


@pytest.mark.parametrize("S,A", DIMS)
def test_bf16_members(S, A):
    _run(S, A, 3, 3, iters=3, bf16=True)


# ---- 4. the members alone afterwards -----------------------------------------------------------------------------------
def test_members_remain_usable_alone():
    iql, hb, H = _hip()
    _, members, twins, rings, trings, _ = _run(17, 6, 2, 2, iters=2)
    for k in range(2):
        la, lb = members[k].train_steps(rings[k], 4, 16, seed=3), twins[k].train_steps(trings[k], 4, 16, seed=3)
        assert np.array_equal(la, lb)
        H.assert_same_trainer_state(members[k], twins[k], f"member {k}: train_steps behind the group call")
    blk = _block(0, 17, 6, 200, 2)
    np.random.seed(SEED)
    a = members[0].online_step_vec(rings[0], *blk, 16, updates=1)
    np.random.seed(SEED)
    assert a == twins[0].online_step_vec(trings[0], *blk, 16, updates=1)
    _same_ring(rings[0], trings[0])


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    iql, hb, H = _hip()
    S, A, B, K = 17, 6, 16, 2
    members = [_build(k, S, A, dropout=0.1) for k in range(K)]
    group = iql.ImplicitQLearningGroup(members, actor_dropout=True)
    rings = [_ring(k, S, A, 8, 4) for k in range(K)]
    blocks = [_block(k, S, A, 0, 3) for k in range(K)]
    ok = tuple([b[j] for b in blocks] for j in range(5))
    act = [_block(0, S, A, 100, 2)[0], None]

    def state():
        return ([t.total_it for t in members], [dict(t._adam_t) for t in members],
                [(r._pointer, r._size, r._writes) for r in rings], torch.stack([r._rows for r in rings]),
                np.stack([H.arenas(t) for t in members]), [_counters(t) for t in members], np.random.get_state()[1].copy(),
                np.random.get_state()[2])

    def same(a, b):
        return all(torch.equal(x, y) if isinstance(x, torch.Tensor) else np.array_equal(x, y) for x, y in zip(a, b))

    def refused(exc, bufs, args, batch=B, **kw):
        s0 = state()
        with pytest.raises(exc):
            group.online_step_vec(bufs, *args, batch, **kw)
        assert same(state(), s0)

    def with_block(k, blk):
        return tuple([blk[j] if i == k else b[j] for i, b in enumerate(blocks)] for j in range(5))

    np.random.seed(SEED)
    refused(ValueError, rings, with_block(1, _block(1, S, A, 0, 9)))                    # E > capacity
    refused(ValueError, rings, ok, updates=33)
    refused(ValueError, rings, ok, updates=-1)
    refused(ValueError, rings, ok, batch=513)
    refused(ValueError, rings, ok, batch=0)
    refused(ValueError, rings, ok, batch=[16, 24])                                      # not a mixed_batch group
    b1 = blocks[1]
    refused(ValueError, rings, with_block(1, (b1[0], b1[1][:2], b1[2], b1[3], b1[4])))  # shapes that disagree
    refused(ValueError, rings, ok, act_next=[None, np.zeros((65, S), dtype=np.float32)])
    refused(ValueError, rings, ok, act_next=[np.zeros((2, S + 1), dtype=np.float32), None])
    refused(ValueError, [rings[0], iql.ReplayBuffer(S, A, 8, "cpu")], ok)
    refused(ValueError, [rings[0], rings[0]], ok)                                       # one ring for two members
    refused(NotImplementedError, rings, ok, act_next=act)                               # a dropout actor without the opt-in
    tracked = _ring(1, S, A, 8, 4)
    tracked.set_sample_weights(torch.ones(4, device="cuda"), updatable=True, track_max=True)
    refused(NotImplementedError, [rings[0], tracked], ok)                               # a ring with a tracking table
    assert (tracked._pointer, tracked._size, tracked._writes) == (4, 4, 4)
    for t in members:
        t.set_precision("bf16")
    refused(NotImplementedError, rings, ok, batch=513)
    for t in members:
        t.set_precision("f32")
    # the library's own refusals: overlapping rings, an index outside a ring, the sizes
    lib, U = hb.lib(), 2
    g = group._group()
    rows = np.zeros((6, rings[0]._ld), dtype=np.float32)
    idx = np.zeros(K * U * B, dtype=np.int64)
    scs, out = (hb.StepScalars * (K * U))(), (C.c_float * (3 * K * U))()
    a_in, a_out = np.zeros((4, S), dtype=np.float32), np.zeros((4, A), dtype=np.float32)
    max_a, seeds = np.ones(K, dtype=np.float32), np.zeros(K, dtype=np.uint64)

    def call(ring_ptrs=None, n_rows=(3, 3), n_upd=U, rows_b=(B, B), a_rows=None, pointers=None):
        ptrs = ring_ptrs or [r._rows.data_ptr() for r in rings]
        ar = None if a_rows is None else np.array(a_rows, dtype=np.int32)
        return lib.iqlhip_group_online_step_vec(
            g, (C.c_void_p * K)(*ptrs), rings[0]._ld, (C.c_int64 * K)(8, 8), (C.c_int64 * K)(*(pointers or [r._pointer for r in rings])),
            rows.ctypes.data, (C.c_int32 * K)(*n_rows), idx.ctypes.data, (C.c_int32 * K)(*rows_b), n_upd, C.addressof(scs),
            C.addressof(out), None if ar is None else a_in.ctypes.data, None if ar is None else ar.ctypes.data,
            max_a.ctypes.data, seeds.ctypes.data, a_out.ctypes.data, torch.cuda.current_stream().cuda_stream)

    s0 = state()
    idx[U * B + 3] = 8                                   # member 1's fourth index
    assert call() == hb.E_INDEX
    idx[U * B + 3] = 0
    base = rings[0]._rows.data_ptr()
    assert call(ring_ptrs=[base, base + 4 * rings[0]._ld * 4]) == hb.E_INVAL and "share" in hb.last_error()
    for bad in (dict(n_rows=(3, 0)), dict(n_rows=(9, 3)), dict(n_upd=33), dict(n_upd=-1), dict(rows_b=(B, 0)),
                dict(rows_b=(513, B)), dict(a_rows=(2, 65)), dict(a_rows=(-1, 2)), dict(pointers=[0, 8]),
                dict(ring_ptrs=[base, rings[1]._rows.data_ptr() + 4])):
        assert call(**bad) == hb.E_INVAL, bad
    members[1].inject_dropout_masks(*(np.ones((B, 256), dtype=np.uint8),) * 2)
    refused(NotImplementedError, rings, ok)
    assert call() == hb.E_UNSUPPORTED
    assert same(state(), s0)
