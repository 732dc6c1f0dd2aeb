"""GPU tests of per-row loss weights, importance-sampling weights and prioritised replay in trainer groups
(ImplicitQLearningGroup.train(loss_weights=, return_td=), .train_steps_weighted(is_beta=), .train_steps_prioritized;
iqlhip_group_step_rw / _train_steps_weighted_is / _train_steps_prioritized; DESIGN.md 6j "trainer groups").

The yardstick is the solo implementation (held to the float64 oracle and to the reference's goldens by its own tests):
every member ends bit for bit where its solo call leaves a twin built identically — parameters, targets, Adam moments,
losses, statistics, TD errors, counters, and the tables' total, flags and leaves.  No tolerance is involved, except where
TD errors are compared with the scoring kernels' columns (tests/test_hip_score.py's 2e-5 for q1, q2 and target_q)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import synth
from burst_twins import fourth_power_weights

pytestmark = pytest.mark.gpu

S, A, N, STEPS = 17, 6, 4096, 5
MAX_WEIGHT = 64.0


def _hip():
    import hip_helpers as H
    import iql
    import iqlhip_binding as hb
    import iqlhip_weighted as wtd
    return iql, hb, H, wtd


def _pair(i, dropout=0.0, drop_seed=None, stats=False, clip=None, count=2):
    """Member i and its twin(s): the same parameters (seed 300 + i), hyper-parameters, learning rates and settings."""
    H = _hip()[2]
    params = synth.synth_params(S, A, seed=300 + i)
    hyper = {"iql_tau": 0.6 + 0.1 * (i % 4), "beta": 2.0 + i, "discount": 0.99, "tau": 0.005 * (1 + i)}
    lrs = {"v": 3e-4 * (1 + i), "q": 2e-4 * (1 + i), "pi": 1e-4 * (1 + i)}
    out = []
    for _ in range(count):
        t = H.build_hip_trainer(params, S, A, True, hyper, lrs, 40 if i == 2 else 1000, dropout=dropout)
        if drop_seed is not None:
            t.set_dropout_seed(drop_seed)
        t.set_step_stats(stats)
        t.set_grad_clip(clip)
        out.append(t)
    return out


def _pairs(K, **kw):
    pairs = [_pair(i, **kw) for i in range(K)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


@functools.lru_cache(maxsize=None)
def _data(n):
    return synth.synth_transitions(n, S, A, seed=22)


def _buffer(n=N):
    iql = _hip()[0]
    buf = iql.ReplayBuffer(S, A, n, "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in _data(n).items()})
    return buf


def _weights(i, n=N):
    return fourth_power_weights(n, seed=2 + i)


def _tables(K, n=N, updatable=True, count=2):
    """count sets of K tables, member i's over _weights(i): [set][member]."""
    wtd = _hip()[3]
    kw = {"updatable": True, "max_weight": MAX_WEIGHT} if updatable else {}
    return [[wtd.SampleWeights(_weights(i, n), **kw) for i in range(K)] for _ in range(count)]


def _state(tab):
    return tab.leaves(), tab.total(), tab.flags()


def _counters(t):
    hb = _hip()[1]
    c = (C.c_uint64 * 2)()
    hb.check(hb.lib().iqlhip_get_counters(t._ctx, c))
    return int(c[0]), int(c[1])


def _assert_same(a, b, what=""):
    H = _hip()[2]
    H.assert_same_trainer_state(a, b, what)
    assert np.array_equal(H.arenas(a), H.arenas(b)), what
    assert a.total_it == b.total_it, what
    assert _counters(a) == _counters(b), (what, _counters(a), _counters(b))


def _assert_tables(a, b, what=""):
    (qa, ta, fa), (qb, tb, fb) = _state(a), _state(b)
    assert np.array_equal(qa, qb), (what, int(np.sum(qa != qb)))
    assert ta == tb == int(np.sum(qa.astype(object))) and fa == fb, (what, ta, tb, fa, fb)
    assert a.version == b.version, (what, a.version, b.version)


def _assert_losses(got, want, what=""):
    assert got.shape == want.shape and np.all(np.isfinite(got)), what
    assert np.array_equal(got, want), (what, got[:2], want[:2])


@functools.lru_cache(maxsize=None)
def _data_batch(B, seed):
    return synth.synth_transitions(B, S, A, seed=seed)


def _batches(Bs, seed=40):
    H = _hip()[2]
    out = []
    for i, B in enumerate(Bs):
        d = _data_batch(B, seed + i)
        out.append(H.to_torch_batch({"s": d["observations"], "a": d["actions"], "r": d["rewards"],
                                     "ns": d["next_observations"], "d": d["terminals"]}))
    return out


def _row_weights(Bs, seed=7):
    rng = np.random.RandomState(seed)
    return [torch.from_numpy(rng.rand(B).astype(np.float32) ** 2 + np.float32(0.05)).cuda() for B in Bs]


def _logs_equal(a, b):
    return list(a) == list(b) and all(a[k] == b[k] for k in a)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("Bs", [(64, 64, 64), (64, 300, 256)])
def test_eager_row_weights_equal_solo_steps_bitwise(Bs):
    """(64, 300, 256): a mixed_batch group; 300 rows are a partial tile and two Q1 loss blocks."""
    from helpers import rel_err
    import score_ref
    iql = _hip()[0]
    col = {name: i for i, name in enumerate(score_ref.SCORE_NAMES)}
    K = len(Bs)
    mixed = len(set(Bs)) > 1
    batches, cs = _batches(Bs), _row_weights(Bs)
    members, twins = _pairs(K)
    group = iql.ImplicitQLearningGroup(members, mixed_batch=mixed)
    if mixed:       # (group.score takes batches of one length: the twins' solo scores are bit for bit the group's)
        scores = [t.score(b, summary=False)[0] for t, b in zip(twins, batches)]
    else:
        scores = group.score(batches, summary=False)[0]
    logs = group.train(batches, loss_weights=cs, return_td=True)
    tds = group.last_td_errors()
    for i in range(K):
        want = twins[i].train(batches[i], loss_weights=cs[i], return_td=True)
        assert _logs_equal(logs[i], want), (i, logs[i], want)
        _assert_same(members[i], twins[i], f"member {i}")
        td = tds[i]
        assert tuple(td.shape) == (Bs[i], 2) and td.dtype == torch.float32 and td.is_cuda
        assert torch.equal(td, twins[i].last_td_errors()), i
        # (q1 - y, q2 - y), y = r + (1 - d) * discount * next_v, of the scores taken before the step: the q and next_v
        # columns are each within 2e-5 of their own largest value (tests/test_hip_score.py), r and d are exact
        sc = scores[i].cpu().numpy().astype(np.float64)
        d = _data_batch(Bs[i], 40 + i)
        r, done = d["rewards"].reshape(-1).astype(np.float64), d["terminals"].reshape(-1).astype(np.float64)
        y = r + (1.0 - done) * 0.99 * sc[:, col["next_v"]]
        for j, name in enumerate(("q1", "q2")):
            want = sc[:, col[name]] - y
            e = rel_err(td[:, j].cpu().numpy(), want)
            tol = 2e-5 * (np.max(np.abs(sc[:, col[name]])) + 0.99 * np.max(np.abs(sc[:, col["next_v"]]))) / np.max(np.abs(want))
            print(f"MARGIN td vs score member {i} {name} {e / tol:.3f}")
            assert e <= tol, (i, name, e, tol)
    assert not _logs_equal(logs[0], logs[1])
    # weights of one, and None entries, are the plain group step; return_td alone changes nothing else
    trios = [_pair(i, count=3) for i in range(K)]
    ones, nones, plain = ([p[j] for p in trios] for j in range(3))
    lo = iql.ImplicitQLearningGroup(ones, mixed_batch=mixed).train(
        batches, loss_weights=[torch.ones(B, dtype=torch.float32, device="cuda") for B in Bs])
    gn = iql.ImplicitQLearningGroup(nones, mixed_batch=mixed)
    ln = gn.train(batches, loss_weights=[None] * K, return_td=True)
    lp = iql.ImplicitQLearningGroup(plain, mixed_batch=mixed).train(batches)
    for i in range(K):
        assert _logs_equal(lo[i], lp[i]) and _logs_equal(ln[i], lp[i]), i
        _assert_same(ones[i], plain[i], f"ones, member {i}")
        _assert_same(nones[i], plain[i], f"None, member {i}")
    assert len(gn.last_td_errors()) == K
    gn.train(batches)
    with pytest.raises(RuntimeError, match="no TD errors"):
        gn.last_td_errors()


# ---------------------------------------------------------------------------------------------------------------- 2
def test_is_burst_equals_solo_calls_at_both_chunkings():
    iql = _hip()[0]
    K, B, seeds, betas = 2, 64, [11, 12], [0.4, 1.0]
    buf = _buffer()
    tabs = _tables(K, updatable=False, count=1)[0]
    for chunk in (2, 64):
        members, twins = _pairs(K)
        got = iql.ImplicitQLearningGroup(members).train_steps_weighted(buf, STEPS, B, seeds, weights=tabs, is_beta=betas,
                                                                       chunk=chunk)
        assert got.shape == (K, STEPS, 3)
        for i in range(K):
            want = twins[i].train_steps_weighted(buf, STEPS, B, seed=seeds[i], weights=tabs[i], is_beta=betas[i], chunk=chunk)
            _assert_losses(got[i], want, f"chunk {chunk}, member {i}")
            _assert_same(members[i], twins[i], f"chunk {chunk}, member {i}")
    # is_beta = 0 is the group call without is_beta; a scalar is_beta serves every member
    a, b = _pairs(K)
    la = iql.ImplicitQLearningGroup(a).train_steps_weighted(buf, STEPS, B, seeds, weights=tabs, is_beta=0.0)
    lb = iql.ImplicitQLearningGroup(b).train_steps_weighted(buf, STEPS, B, seeds, weights=tabs)
    _assert_losses(la, lb, "is_beta = 0")
    for i in range(K):
        _assert_same(a[i], b[i], f"is_beta = 0, member {i}")
    assert not np.array_equal(la, got)                      # (is_beta > 0 did weight the losses)
    # a member without a table draws uniformly with c = 1: its solo train_steps
    members, twins = _pairs(K)
    got = iql.ImplicitQLearningGroup(members).train_steps_weighted(buf, STEPS, B, seeds, weights=[tabs[0], None],
                                                                   is_beta=[0.4, 1.0], chunk=2)
    want = [twins[0].train_steps_weighted(buf, STEPS, B, seed=seeds[0], weights=tabs[0], is_beta=0.4, chunk=2),
            twins[1].train_steps(buf, STEPS, B, seed=seeds[1], chunk=2)]
    for i in range(K):
        _assert_losses(got[i], want[i], f"None member, member {i}")
        _assert_same(members[i], twins[i], f"None member, member {i}")


# ---------------------------------------------------------------------------------------------------------------- 3
ALPHAS, EPSS, BETAS = [0.6, 0.9, 0.3], [1e-3, 1e-2, 0.0], [0.5, 1.0, 0.0]


@pytest.mark.parametrize("K", [2, 3])
def test_prioritised_burst_equals_solo_calls_and_is_not_vacuous(K):
    iql = _hip()[0]
    B, seeds = 64, [21, 22, 23][:K]
    al, ep, be = ALPHAS[:K], EPSS[:K], BETAS[:K]
    buf = _buffer()
    results = {}
    for chunk in (2, 64):
        gt, st = _tables(K)
        q0 = [_state(t)[0] for t in gt]
        members, twins = _pairs(K)
        got = iql.ImplicitQLearningGroup(members).train_steps_prioritized(buf, STEPS, B, seeds, alpha=al, eps=ep,
                                                                          is_beta=be, weights=gt, chunk=chunk)
        assert got.shape == (K, STEPS, 3)
        for i in range(K):
            want = twins[i].train_steps_prioritized(buf, STEPS, B, seed=seeds[i], alpha=al[i], eps=ep[i], is_beta=be[i],
                                                    weights=st[i], chunk=chunk)
            _assert_losses(got[i], want, f"chunk {chunk}, member {i}")
            _assert_same(members[i], twins[i], f"chunk {chunk}, member {i}")
            _assert_tables(gt[i], st[i], f"chunk {chunk}, member {i}")
            assert gt[i].flags() == 0
            assert np.any(_state(gt[i])[0] != q0[i]), i                       # priorities were written
        for i in range(1, K):                                                 # ... and each member wrote its own
            d0, di = _state(gt[0])[0] != q0[0], _state(gt[i])[0] != q0[i]
            assert not np.array_equal(d0, di), i
        results[chunk] = (got, members, gt)
    # even B: the pieces go on with the lag-1 chain, so the two chunkings agree
    _assert_losses(results[2][0], results[64][0], "chunk 2 vs chunk 64")
    for i in range(K):
        _assert_same(results[2][1][i], results[64][1][i], f"chunkings, member {i}")
        assert np.array_equal(_state(results[2][2][i])[0], _state(results[64][2][i])[0]), i
    # from step 2 on the draws have seen updated priorities: the losses leave those of the IS burst on untouched tables
    frozen = _tables(K, count=1)[0]
    others = _pairs(K)[0]
    lw = iql.ImplicitQLearningGroup(others).train_steps_weighted(buf, STEPS, B, seeds, weights=frozen, is_beta=be)
    got = results[64][0]
    for i in range(K):
        assert np.array_equal(got[i, :2], lw[i, :2]), i                       # steps 0 and 1: drawn before any update landed
        assert not np.array_equal(got[i, 2:], lw[i, 2:]), i


# ---------------------------------------------------------------------------------------------------------------- 4
def test_odd_and_unequal_batch_sizes_redraw_per_piece():
    iql = _hip()[0]
    Bs, seeds, al, ep, be = [64, 75], [31, 32], [0.6, 0.8], [1e-3, 1e-3], [0.5, 0.7]
    buf = _buffer()
    gt, st = _tables(2)
    members, twins = _pairs(2)
    got = iql.ImplicitQLearningGroup(members, mixed_batch=True).train_steps_prioritized(
        buf, STEPS, Bs, seeds, alpha=al, eps=ep, is_beta=be, weights=gt, chunk=2)
    for i in range(2):
        want = twins[i].train_steps_prioritized(buf, STEPS, Bs[i], seed=seeds[i], alpha=al[i], eps=ep[i], is_beta=be[i],
                                                weights=st[i], chunk=2)
        _assert_losses(got[i], want, f"member {i}")
        _assert_same(members[i], twins[i], f"member {i}")
        _assert_tables(gt[i], st[i], f"member {i}")
    # the odd member's pieces each start on a fresh draw: one piece of five steps ends elsewhere
    one, tab1 = _pair(1, count=1)[0], _tables(2, count=1)[0][1]
    one.train_steps_prioritized(buf, STEPS, 75, seed=32, alpha=0.8, eps=1e-3, is_beta=0.7, weights=tab1, chunk=64)
    assert not np.array_equal(_state(tab1)[0], _state(gt[1])[0])


# ---------------------------------------------------------------------------------------------------------------- 5
def test_duplicate_rows_last_one_wins_as_solo():
    iql = _hip()[0]
    n, B, seeds = 48, 64, [41, 42]                   # 64 draws over 48 rows: every batch holds duplicates
    buf = _buffer(n)
    gt, st = _tables(2, n=n)
    members, twins = _pairs(2)
    got = iql.ImplicitQLearningGroup(members).train_steps_prioritized(buf, STEPS, B, seeds, alpha=[0.6, 1.0], eps=1e-3,
                                                                      is_beta=0.5, weights=gt)
    for i in range(2):
        idx = gt[i].draw_indices(B, seeds[i], 0).cpu().numpy()
        assert len(set(idx.tolist())) < B
        want = twins[i].train_steps_prioritized(buf, STEPS, B, seed=seeds[i], alpha=[0.6, 1.0][i], eps=1e-3, is_beta=0.5,
                                                weights=st[i])
        _assert_losses(got[i], want, f"member {i}")
        _assert_same(members[i], twins[i], f"member {i}")
        _assert_tables(gt[i], st[i], f"member {i}")
        assert gt[i].flags() == st[i].flags() == 0


# ---------------------------------------------------------------------------------------------------------------- 6
def test_everything_on_dropout_statistics_and_clipping():
    iql = _hip()[0]
    B, seeds = 64, [51, 52]
    buf = _buffer()
    gt, st = _tables(2)
    p0 = _pair(0, dropout=0.1, drop_seed=900, stats=True, clip=0.5)
    p1 = _pair(1, dropout=0.0, drop_seed=901)
    members, twins = [p0[0], p1[0]], [p0[1], p1[1]]
    for t in members + twins:
        t.actor.train()
    stats = iql.ImplicitQLearningGroup(members, actor_dropout=True).train_steps_prioritized(
        buf, STEPS, B, seeds, alpha=[0.6, 0.9], eps=[1e-3, 1e-2], is_beta=[0.5, 1.0], weights=gt, chunk=2,
        return_stats=True)
    assert stats.shape == (STEPS, 2, 16)
    _, want_stats = twins[0].train_steps_prioritized(buf, STEPS, B, seed=seeds[0], alpha=0.6, eps=1e-3, is_beta=0.5,
                                                     weights=st[0], chunk=2, return_stats=True)
    twins[1].train_steps_prioritized(buf, STEPS, B, seed=seeds[1], alpha=0.9, eps=1e-2, is_beta=1.0, weights=st[1], chunk=2)
    assert np.array_equal(stats[:, 0], want_stats) and np.all(np.isnan(stats[:, 1]))
    for i in range(2):
        _assert_same(members[i], twins[i], f"member {i}")
        _assert_tables(gt[i], st[i], f"member {i}")


# ---------------------------------------------------------------------------------------------------------------- 7
def test_two_python_calls_in_a_row_and_nothing_stale_afterwards():
    iql = _hip()[0]
    B, seeds = 64, [61, 62]
    buf = _buffer()
    gt, st = _tables(2)
    members, twins = _pairs(2)
    group = iql.ImplicitQLearningGroup(members)
    kw = dict(alpha=[0.6, 0.9], eps=1e-3, is_beta=[0.5, 1.0])
    got = [group.train_steps_prioritized(buf, k, B, seeds, weights=gt, chunk=2, **kw) for k in (3, 2)]
    for i in range(2):
        want = [twins[i].train_steps_prioritized(buf, k, B, seed=seeds[i], alpha=kw["alpha"][i], eps=1e-3,
                                                 is_beta=kw["is_beta"][i], weights=st[i], chunk=2) for k in (3, 2)]
        for j in range(2):
            _assert_losses(got[j][i], want[j], f"call {j}, member {i}")
        _assert_same(members[i], twins[i], f"member {i}")
        _assert_tables(gt[i], st[i], f"member {i}")
    # 3 + 2 steps are not 5: the second call's step 0 was a fresh draw, not a row set staged one update earlier
    gt5 = _tables(2, count=1)[0]
    five = _pairs(2)[0]
    iql.ImplicitQLearningGroup(five).train_steps_prioritized(buf, 5, B, seeds, weights=gt5, chunk=2, **kw)
    assert any(not np.array_equal(_state(gt5[i])[0], _state(gt[i])[0]) for i in range(2))
    # a solo weighted call on a member afterwards: nothing the group staged is continued
    for i in range(2):
        a = members[i].train_steps_weighted(buf, 4, B, seed=seeds[i], weights=gt[i], is_beta=0.5)
        b = twins[i].train_steps_weighted(buf, 4, B, seed=seeds[i], weights=st[i], is_beta=0.5)
        _assert_losses(a, b, f"solo afterwards, member {i}")
        _assert_same(members[i], twins[i], f"solo afterwards, member {i}")


def test_plain_and_row_weighted_calls_interleaved_on_one_group():
    """step, step_rw, step, then a 2-step train_steps_weighted_is on ONE group: the plain and the row-weighted calls run
    from two stagings through the same host code, each with its own upload event — every call equals the members' solo
    calls in the same order, bit for bit."""
    iql = _hip()[0]
    K, B, seeds, betas = 2, 10, [71, 72], [0.4, 1.0]
    buf = _buffer()
    tabs = _tables(K, updatable=False, count=1)[0]
    members, twins = _pairs(K)
    group = iql.ImplicitQLearningGroup(members)
    calls = [(_batches((B,) * K, seed=80), None), (_batches((B,) * K, seed=84), _row_weights((B,) * K)),
             (_batches((B,) * K, seed=88), None)]
    for n, (batches, cs) in enumerate(calls):
        kw = [{} if cs is None else {"loss_weights": cs[i], "return_td": True} for i in range(K)]
        logs = group.train(batches) if cs is None else group.train(batches, loss_weights=cs, return_td=True)
        for i in range(K):
            want = twins[i].train(batches[i], **kw[i])
            assert _logs_equal(logs[i], want), (n, i, logs[i], want)
            _assert_same(members[i], twins[i], f"call {n}, member {i}")
            if cs is not None:
                assert torch.equal(group.last_td_errors()[i], twins[i].last_td_errors()), (n, i)
    got = group.train_steps_weighted(buf, 2, B, seeds, weights=tabs, is_beta=betas, chunk=2)
    assert got.shape == (K, 2, 3)
    for i in range(K):
        want = twins[i].train_steps_weighted(buf, 2, B, seed=seeds[i], weights=tabs[i], is_beta=betas[i], chunk=2)
        _assert_losses(got[i], want, f"burst, member {i}")
        _assert_same(members[i], twins[i], f"burst, member {i}")
    assert not np.array_equal(got[0], got[1])


# ---------------------------------------------------------------------------------------------------------------- 8
def _snapshot(members, tables):
    H = _hip()[2]
    return ([H.arenas(t).copy() for t in members], [t.total_it for t in members], [_counters(t) for t in members],
            [t.version for t in tables], [_state(t)[1] for t in tables])


def _assert_untouched(members, tables, snap, what):
    now = _snapshot(members, tables)
    for a, b in zip(now[0], snap[0]):
        assert np.array_equal(a, b), what
    assert now[1:] == snap[1:], (what, now[1:], snap[1:])


def test_refusals_leave_everything_where_it_was():
    iql, hb, _, wtd = _hip()
    B, seeds = 64, [71, 72]
    buf = _buffer()
    tabs = _tables(2, count=1)[0]
    static = wtd.SampleWeights(_weights(0))
    short = wtd.SampleWeights(_weights(0, 100), updatable=True, max_weight=MAX_WEIGHT)
    members = _pairs(2, dropout=0.1, drop_seed=5)[0]
    for t in members:
        t.actor.train()
    group = iql.ImplicitQLearningGroup(members, actor_dropout=True)
    group.train_steps_prioritized(buf, 2, B, seeds, weights=tabs)            # (a first call: every lazy buffer exists)
    snap = _snapshot(members, tabs)
    cases = [("a static table", dict(weights=[tabs[0], static]), ValueError, "updatable"),
             ("a None entry", dict(weights=[tabs[0], None]), ValueError, "member 1"),
             ("one table twice", dict(weights=[tabs[0], tabs[0]]), ValueError, "member 1"),
             ("alpha = eps = 0", dict(weights=tabs, alpha=[0.6, 0.0], eps=[1e-3, 0.0]), ValueError, "member 1"),
             ("a negative is_beta", dict(weights=tabs, is_beta=[0.5, -0.1]), ValueError, "member 1"),
             ("another n", dict(weights=[tabs[0], short]), ValueError, "member 1")]
    for what, kw, exc, match in cases:
        with pytest.raises(exc, match=match):
            group.train_steps_prioritized(buf, 2, B, seeds, **kw)
        _assert_untouched(members, tabs, snap, what)
    with pytest.raises(ValueError, match="member 1"):
        group.train_steps_weighted(buf, 2, B, seeds, weights=tabs, is_beta=[0.5, float("nan")])
    _assert_untouched(members, tabs, snap, "a NaN is_beta")
    # the library's own refusals, the Python checks bypassed: the C entry point names the member and moves nothing
    lib, g, K = hb.lib(), group._group(), 2
    rows = (C.c_void_p * K)(*[buf._rows.data_ptr()] * K)
    sizes, Bs = (C.c_int64 * K)(N, N), (C.c_int32 * K)(B, B)
    tabs_sc = [np.ascontiguousarray(np.zeros((2, 12), dtype=np.float32)) for _ in range(K)]
    tab_ptrs = (C.c_void_p * K)(*[t.ctypes.data for t in tabs_sc])
    u64 = (C.c_uint64 * K)(1, 2)
    f = lambda *v: (C.c_float * K)(*v)
    wt = lambda *t: (C.c_void_p * K)(*[None if x is None else x._table for x in t])
    stream = members[0]._stream()
    base = [g, rows, buf._ld, sizes, Bs, tab_ptrs, 2, u64, u64, 0, stream]
    prio = lib.iqlhip_group_train_steps_prioritized
    for what, tail, code in [("static", [wt(tabs[0], static), f(0, 0), f(.6, .6), f(.1, .1)], hb.E_INVAL),
                             ("NULL entry", [wt(tabs[0], None), f(0, 0), f(.6, .6), f(.1, .1)], hb.E_INVAL),
                             ("twice", [wt(tabs[0], tabs[0]), f(0, 0), f(.6, .6), f(.1, .1)], hb.E_INVAL),
                             ("both zero", [wt(*tabs), f(0, 0), f(.6, 0), f(.1, 0)], hb.E_INVAL),
                             ("beta", [wt(*tabs), f(0, -1), f(.6, .6), f(.1, .1)], hb.E_INVAL),
                             ("n", [wt(tabs[0], short), f(0, 0), f(.6, .6), f(.1, .1)], hb.E_INVAL)]:
        assert prio(*base, *tail) == code, what
        assert "member 1" in hb.last_error(), (what, hb.last_error())
        _assert_untouched(members, tabs, snap, "C: " + what)
    bad_flags = list(base)
    bad_flags[9] = 2
    assert prio(*bad_flags, wt(*tabs), f(0, 0), f(.6, .6), f(.1, .1)) == hb.E_INVAL
    # NULL arrays
    full = base + [wt(*tabs), f(0, 0), f(.6, .6), f(.1, .1)]
    for hole in (1, 3, 4, 5, 7, 8, 11, 12, 13, 14):
        args = list(full)
        args[hole] = None
        assert prio(*args) == hb.E_INVAL, hole
    for hole in (11, 12):
        args = list(full[:13])
        args[hole] = None
        assert lib.iqlhip_group_train_steps_weighted_is(*args) == hb.E_INVAL, hole
    batches = _batches([B, B])
    structs = (hb.Batch * K)(*[members[i]._batch_struct(batches[i])[0] for i in range(K)])
    scs = (hb.StepScalars * K)()
    nulls = (C.c_void_p * K)(None, None)
    assert lib.iqlhip_group_step_rw(g, structs, scs, None, nulls, None, stream) == hb.E_INVAL
    assert lib.iqlhip_group_step_rw(g, structs, scs, nulls, None, None, stream) == hb.E_INVAL
    _assert_untouched(members, tabs, snap, "NULL arrays")
    # a bf16 member: per-row loss weights are an fp32 kernel
    members[1].set_precision("bf16")
    for call in (lambda: group.train_steps_prioritized(buf, 2, B, seeds, weights=tabs),
                 lambda: group.train_steps_weighted(buf, 2, B, seeds, weights=tabs, is_beta=0.5),
                 lambda: group.train(batches, loss_weights=[None, None], return_td=True)):
        with pytest.raises((NotImplementedError, ValueError)):
            call()
    members[1].set_precision("f32")
    _assert_untouched(members, tabs, snap, "bf16")
    # ... and after all of it the group still steps
    group.train_steps_prioritized(buf, 2, B, seeds, weights=tabs)
    assert [t.version for t in tabs] == [v + 1 for v in snap[3]]
