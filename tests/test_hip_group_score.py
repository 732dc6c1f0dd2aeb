"""GPU tests of group scoring (ImplicitQLearningGroup.score_buffer / score / evaluate; DESIGN.md 6h "group scoring"):
every member's scores and summary bit for bit its solo call's, the across-member spread (reproducible, equal to the
stated fp32 arithmetic, and within a derived bound of the float64 value), parity with the numpy oracle under the solo
tests' bounds, bytewise absence of side effects, refusals, scratch.  Buffers hold at most a few thousand rows."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch

import score_ref
import synth

pytestmark = pytest.mark.gpu

LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
N_ROWS = 700
COL = {name: i for i, name in enumerate(score_ref.SCORE_NAMES)}
PLAIN = ("v", "next_v", "q1", "q2", "target_q", "adv")


def _hip():
    import hip_helpers as H
    import iql
    import iqlhip_binding as hb
    return iql, hb, H


def _hyper(i):
    return {"iql_tau": 0.6 + 0.05 * (i % 4), "beta": 2.0 + (i % 5), "discount": 0.99 - 0.01 * (i % 3), "tau": 0.005}


@functools.lru_cache(maxsize=None)
def _params(S, A, gaussian, i):
    return synth.synth_params(S, A, seed=900 + i, gaussian=gaussian)


@functools.lru_cache(maxsize=None)
def _data(S, A, which=0, n=N_ROWS):
    return synth.synth_transitions(n + 37 * which, S, A, seed=60 + which)


@functools.lru_cache(maxsize=None)
def _buffer(S, A, which=0, n=N_ROWS):
    """Replay buffers: never written by a test.  which = 0 is the shared one; the others differ in size and content."""
    iql = _hip()[0]
    data = _data(S, A, which, n)
    buf = iql.ReplayBuffer(S, A, data["observations"].shape[0], "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in data.items()})
    return buf


def _member(S, A, gaussian, i, bf16=False, dropout=0.0, stats=False, clip=None):
    tr = _hip()[2].build_hip_trainer(_params(S, A, gaussian, i), S, A, gaussian, _hyper(i), LRS, 1000, dropout=dropout)
    if dropout:
        tr.set_dropout_seed(40 + i)
    if bf16:
        tr.set_precision("bf16")
    tr.set_step_stats(stats)
    tr.set_grad_clip(clip)
    return tr


def _group(K, S=17, A=6, gaussian=True, group_kw=None, **kw):
    members = [_member(S, A, gaussian, i, **kw) for i in range(K)]
    return _hip()[0].ImplicitQLearningGroup(members, **(group_kw or {})), members


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _batch_of(data, sl=slice(None)):
    return {"s": data["observations"][sl], "a": data["actions"][sl], "r": data["rewards"][sl],
            "ns": data["next_observations"][sl], "d": data["terminals"][sl]}


def _index_list(n, size, seed):
    """n indices into `size` rows with repeats and a descending run."""
    idx = np.random.RandomState(seed).randint(0, size, size=n).astype(np.int64)
    run = min(n, 9)
    idx[:run] = np.arange(size - 1, size - 1 - run, -1)
    if n > 12:
        idx[10:12] = idx[9]
    return idx


def _assert_equals_solo(group, members, bufs, what, **kw):
    """A group call against the members' solo calls with the same arguments: scores and summaries bit for bit."""
    K = len(members)
    per_buf = bufs if isinstance(bufs, list) else [bufs] * K
    indices = kw.pop("indices", None)
    per_idx = indices if isinstance(indices, list) else [indices] * K
    scores, summaries, _ = group.score_buffer(bufs, indices=indices, **kw)
    for k, t in enumerate(members):
        s, m = t.score_buffer(per_buf[k], indices=per_idx[k], **kw)
        assert np.array_equal(_bits(scores[k]), _bits(s)), (what, k)
        assert summaries[k] == m, (what, k, summaries[k], m)
    return scores, summaries


# ---- 1. bitwise against solo ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("gaussian", [True, False])
@pytest.mark.parametrize("S,A", [(11, 3), (17, 6), (39, 28)])
@pytest.mark.parametrize("K", [2, 3])
def test_scores_and_summaries_equal_the_solo_calls_bitwise(K, S, A, gaussian):
    group, members = _group(K, S, A, gaussian)
    shared = _buffer(S, A)
    own = [_buffer(S, A, 1 + k) for k in range(K)]
    for n in (1, 31, 33, 600):
        _assert_equals_solo(group, members, shared, ("range shared", n), start=7, n=n)
        _assert_equals_solo(group, members, own, ("range own", n), start=3, n=n)
        idx = _index_list(n, N_ROWS, seed=n)
        _assert_equals_solo(group, members, shared, ("index shared", n), indices=torch.from_numpy(idx).cuda())
        lists = [_index_list(n, N_ROWS + 37 * (1 + k), seed=100 * k + n) for k in range(K)]
        _assert_equals_solo(group, members, own, ("index own", n), indices=lists)


def test_chunked_calls_equal_the_solo_calls_cut_the_same_way():
    group, members = _group(2)
    buf = _buffer(17, 6)
    cut, cut_sum = _assert_equals_solo(group, members, buf, "chunk 64", n=600, chunk_rows=64)
    whole, whole_sum = _assert_equals_solo(group, members, buf, "one chunk", n=600)
    assert np.array_equal(_bits(cut), _bits(whole))
    for a, b in zip(cut_sum, whole_sum):
        for key in a:
            assert abs(a[key] - b[key]) <= 1e-6 * abs(b[key]), (key, a[key], b[key])


def test_sixteen_members_at_and_across_the_scratch_cap():
    """K = 16: the record tables at their longest and the smallest chunk cap, 4 096 rows; 4 097 rows cross it."""
    S, A = 17, 6
    group, members = _group(16, S, A)
    _assert_equals_solo(group, members, _buffer(S, A), "K16 n33", start=5, n=33)
    big = _buffer(S, A, 0, 4200)
    scores, summaries, spread = group.score_buffer(big, n=4097, spread=True)
    for k, t in enumerate(members):
        assert np.array_equal(_bits(scores[k]), _bits(t.score_buffer(big, n=4097, summary=False)[0])), k
    _check_spread(scores, spread, "K16 n4097")


@pytest.mark.parametrize("K", [2, 5])
def test_a_forward_cut_into_several_launches_equals_solo(K):
    """From a few thousand rows on, the chunk's forward goes as several launches over some of the members each (so that
    every launch fills the device): 6 400 rows are past that point for K = 2 and K = 5 on a device of 256 CUs (200 tiles:
    2 x (23 + 3) < 50 + 3 tile times).  Scores and summaries stay the solo calls' bits."""
    S, A = 17, 6
    group, members = _group(K, S, A)
    big = _buffer(S, A, 0, 6500)
    scores, summaries, _ = group.score_buffer(big, start=7, n=6400)
    for k, t in enumerate(members):
        s, m = t.score_buffer(big, start=7, n=6400)
        assert np.array_equal(_bits(scores[k]), _bits(s)) and summaries[k] == m, k


@pytest.mark.parametrize("kind", ["dropout", "bf16", "mixed_batch"])
def test_every_kind_of_group_scores_like_its_members(kind):
    kw = {"dropout": dict(dropout=0.1, group_kw={"actor_dropout": True}), "bf16": dict(bf16=True),
          "mixed_batch": dict(group_kw={"mixed_batch": True})}[kind]
    group, members = _group(3, **kw)
    for t in members:
        t.actor.train(True)
    _assert_equals_solo(group, members, _buffer(17, 6), kind, start=1, n=333)
    if kind == "bf16":          # ... which are the fp32 masters' scores
        plain = _member(17, 6, True, 1)
        assert np.array_equal(_bits(group.score_buffer(_buffer(17, 6), n=333)[0][1]),
                              _bits(plain.score_buffer(_buffer(17, 6), n=333)[0]))


def test_score_and_evaluate_of_batches_equal_the_solo_calls():
    H = _hip()[2]
    S, A, K = 17, 6, 3
    group, members = _group(K, S, A)
    shared = H.to_torch_batch(_batch_of(_data(S, A), slice(10, 343)))
    own = [H.to_torch_batch(_batch_of(_data(S, A, 1 + k), slice(k, k + 333))) for k in range(K)]
    for batches, per in ((shared, [shared] * K), (own, own)):
        scores, summaries, _ = group.score(batches)
        ev = group.evaluate(batches)
        for k, t in enumerate(members):
            s, m = t.score(per[k])
            assert np.array_equal(_bits(scores[k]), _bits(s)) and summaries[k] == m, k
            assert ev[k] == t.evaluate(per[k]), k


def test_two_queued_summaryless_calls_each_use_their_own_arguments():
    group, members = _group(2)
    buf = _buffer(17, 6)
    a = torch.zeros((2, 100, 8), device="cuda")
    b = torch.zeros((2, 77, 8), device="cuda")
    torch.cuda.synchronize()
    group.score_buffer(buf, start=0, n=100, out=a, summary=False)
    group.score_buffer(buf, start=300, n=77, out=b, summary=False)
    torch.cuda.synchronize()
    for k, t in enumerate(members):
        assert np.array_equal(_bits(a[k]), _bits(t.score_buffer(buf, start=0, n=100, summary=False)[0])), k
        assert np.array_equal(_bits(b[k]), _bits(t.score_buffer(buf, start=300, n=77, summary=False)[0])), k


# ---- 2. spread ------------------------------------------------------------------------------------------------------
def _check_spread(scores, spread, what):
    """spread against (a) the stated arithmetic in numpy float32, bit for bit, and (b) numpy float64 mean and population
    std within |err| <= 4 (K + 2) 2^-24 max_k |x_k| per element (the issue's derivation: K u M on the mean, (K + 2) u M
    on each deviation, the norm 1-Lipschitz in them, (K + 4) u M for squares, division and root; (2 K + 6) u M, doubled)."""
    x = scores.cpu().numpy()
    got = spread.cpu().numpy()
    K, n = x.shape[0], x.shape[1]
    assert got.shape == (n, 16) and got.dtype == np.float32
    mean = x[0].copy()
    for k in range(1, K):
        mean = mean + x[k]
    mean = mean / np.float32(K)
    dev = np.zeros_like(mean)
    for k in range(K):
        d = x[k] - mean
        dev = dev + d * d
    dev = np.sqrt(dev / np.float32(K))
    assert mean.dtype == np.float32 and dev.dtype == np.float32
    assert np.array_equal(got[:, :8].view(np.uint32), mean.view(np.uint32)), what
    assert np.array_equal(got[:, 8:].view(np.uint32), dev.view(np.uint32)), what
    x64 = x.astype(np.float64)
    bound = 4 * (K + 2) * 2.0 ** -24 * np.max(np.abs(x64), axis=0)
    e_mean = np.abs(got[:, :8] - x64.mean(axis=0))
    e_std = np.abs(got[:, 8:] - x64.std(axis=0))
    print(f"MARGIN spread {what} mean {np.max(e_mean / np.maximum(bound, 1e-300)):.3f} std {np.max(e_std / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(e_mean <= bound) and np.all(e_std <= bound), what


@pytest.mark.parametrize("K", [1, 2, 3, 16])
def test_spread_is_reproducible_exact_and_within_its_bound(K):
    group, members = _group(K)
    buf = _buffer(17, 6)
    for n in (33, 600):
        idx = torch.from_numpy(_index_list(n, N_ROWS, seed=n)).cuda()
        scores, _, spread = group.score_buffer(buf, indices=idx, spread=True)
        _check_spread(scores, spread, (K, n))
        again = torch.empty((n, 16), device="cuda")
        none, summaries, same = group.score_buffer(buf, indices=idx, out=False, spread=again)      # no per-row store at all
        assert none is None and same is again and np.array_equal(_bits(again), _bits(spread)), (K, n)
        assert summaries == group.score_buffer(buf, indices=idx, out=False)[1]
        only = group.score_buffer(buf, indices=idx, out=False, summary=False, spread=True)[2]
        assert np.array_equal(_bits(only), _bits(spread)), (K, n)
        if K == 1:
            assert np.array_equal(_bits(spread[:, :8]), _bits(scores[0])) and np.all(spread[:, 8:].cpu().numpy() == 0.0)


# ---- 3. parity with the oracle, under the solo tests' bounds (tests/test_hip_score.py) -------------------------------
@pytest.mark.parametrize("gaussian", [True, False])
def test_columns_and_losses_against_the_oracle(gaussian):
    """Bounds: exactly test_hip_score._check_against_oracle's — 2e-5 for the six plain columns (helpers' number),
    max(2e-5, 4 x rel_err(oracle fp32, oracle fp64)) for exp_adv, bc and the three losses, a mean held to its column's."""
    from helpers import rel_err
    S, A, K, n = 17, 6, 3, 600
    group, members = _group(K, S, A, gaussian)
    batch = _batch_of(_data(S, A), slice(0, n))
    scores, summaries, _ = group.score(_hip()[2].to_torch_batch(batch))
    for k in range(K):
        hyper = dict(_hyper(k), deterministic=not gaussian)
        r32 = score_ref.reference(_params(S, A, gaussian, k), batch, hyper, np.float32)
        r64 = score_ref.reference(_params(S, A, gaussian, k), batch, hyper, np.float64)
        got = scores[k].cpu().numpy()
        for name, i in COL.items():
            tol = 2e-5 if name in PLAIN else max(2e-5, 4 * rel_err(r32["cols"][:, i], r64["cols"][:, i]))
            e = rel_err(got[:, i], r64["cols"][:, i])
            assert e <= tol, (k, name, e, tol)
            scale = float(np.max(np.abs(r64["cols"][:, i])))
            em = abs(summaries[k]["mean_" + name] - float(r64["means"][i])) / max(scale, 1e-30)
            assert em <= tol, (k, "mean_" + name, em, tol)
        for j, name in enumerate(score_ref.LOSS_NAMES):
            want32, want64 = float(r32["losses"][j]), float(r64["losses"][j])
            tol = max(2e-5, 4 * abs(want32 - want64) / abs(want64))
            e = abs(summaries[k][name] - want64) / abs(want64)
            assert e <= tol, (k, name, e, tol)


# ---- 4. nothing else changes ------------------------------------------------------------------------------------------
def _counters(t):
    hb = _hip()[1]
    c = (C.c_uint64 * 2)()
    hb.check(hb.lib().iqlhip_get_counters(t._ctx, c))
    return int(c[0]), int(c[1]), t.act_dropout_calls()


@pytest.mark.parametrize("mode", ["f32", "bf16", "replay_mix"])
def test_group_scoring_between_training_calls_changes_nothing(mode):
    iql, hb, H = _hip()
    S, A, K, B = 17, 6, 3, 64
    buf = _buffer(S, A)
    held_out = H.to_torch_batch(_batch_of(_data(S, A, 1), slice(0, 333)))
    stream = _data(S, A, 2)
    runs = []
    for with_scoring in (False, True):
        members = [_member(S, A, True, i, bf16=mode == "bf16", dropout=0.0 if mode == "bf16" else 0.1,
                           stats=i == 1, clip=0.5 if i == 1 else None) for i in range(K)]
        group = iql.ImplicitQLearningGroup(members, actor_dropout=mode != "bf16")
        rings = [iql.ReplayBuffer(S, A, 128, "cuda") for _ in range(K)]
        for k, ring in enumerate(rings):
            for i in range(70):
                j = 70 * k + i
                ring.add_transition(stream["observations"][j], stream["actions"][j], float(stream["rewards"][j]),
                                    stream["next_observations"][j], bool(stream["terminals"][j]))
        seeds = [5 + k for k in range(K)]
        out = []

        def steps(n):
            if mode == "replay_mix":
                out.append(group.train_steps_replay_mix(buf, rings, n, B, seeds, 0.5))
                out.append(group.train_steps_replay_mix(buf, rings, n, B, seeds, 0.5, return_stats=True))
            else:
                out.append(group.train_steps(buf, n, B, seeds))
                out.append(group.train_steps(buf, n, B, seeds, return_stats=True))

        def scoring():
            if with_scoring:
                s, m, sp = group.score_buffer(buf, start=5, n=600, spread=True)
                assert np.all(np.isfinite(s.cpu().numpy())) and np.all(np.isfinite(sp.cpu().numpy()))
                group.evaluate(held_out)
                group.score_buffer(buf, indices=torch.tensor([3, 650, 77], device="cuda"), out=False, spread=True)

        steps(5)
        scoring()
        j = 500
        tr = [(stream["observations"][j + k], stream["actions"][j + k], float(stream["rewards"][j + k]),
               stream["next_observations"][j + k], bool(stream["terminals"][j + k])) for k in range(K)]
        rngs = [np.random.RandomState(s) for s in seeds]
        out.append(group.online_step(rings, *[list(x) for x in zip(*tr)], B, rngs=rngs))
        scoring()
        steps(4)
        runs.append((members, out))
    (ma, oa), (mb, ob) = runs
    for a, b in zip(oa, ob):
        if isinstance(a, np.ndarray):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), mode
        else:
            assert a == b, mode
    for k, (a, b) in enumerate(zip(ma, mb)):
        assert np.array_equal(H.arenas(a).view(np.uint32), H.arenas(b).view(np.uint32)), (mode, k)
        assert _counters(a) == _counters(b) and a.total_it == b.total_it and a._adam_t == b._adam_t, (mode, k)
        assert a.last_grad_clip() == b.last_grad_clip() if a._grad_clip is not None else True, (mode, k)


def test_a_members_own_scoring_scratch_is_untouched():
    group, members = _group(3)
    buf, other = _buffer(17, 6), _buffer(17, 6, 1)
    before = [t.score_buffer(buf, n=500) for t in members]
    group.score_buffer(other, start=9, n=650, spread=True)
    for t, (s, m) in zip(members, before):
        s2, m2 = t.score_buffer(buf, n=500)
        assert np.array_equal(_bits(s), _bits(s2)) and m == m2


# ---- 5. refusals and scratch ------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_the_next_call_is_correct():
    iql, hb, H = _hip()
    S, A, K = 17, 6, 3
    group, members = _group(K, S, A)
    buf, small = _buffer(S, A), _buffer(S, A, 0, 200)
    good = _bits(group.score_buffer(buf, n=64, summary=False)[0])
    out = torch.full((K, 64, 8), 7.0, device="cuda")
    spread = torch.full((64, 16), 7.0, device="cuda")
    bad = torch.arange(64, device="cuda")
    bad_1 = bad.clone()
    bad_1[40] = N_ROWS
    with pytest.raises(IndexError, match=f"member 1: index {N_ROWS} is out of bounds"):
        group.score_buffer(buf, indices=[bad, bad_1, bad], out=out)
    # the C entry point itself
    lib, g, st = hb.lib(), group._g, members[0]._stream()
    rows = (C.c_void_p * K)(*[buf._rows.data_ptr()] * K)
    rows_small = (C.c_void_p * K)(buf._rows.data_ptr(), small._rows.data_ptr(), buf._rows.data_ptr())
    sizes, sizes_small = (C.c_int64 * K)(*[N_ROWS] * K), (C.c_int64 * K)(N_ROWS, 200, N_ROWS)
    outs = (C.c_void_p * K)(*[out[k].data_ptr() for k in range(K)])
    outs_odd = (C.c_void_p * K)(out[0].data_ptr(), out[1].data_ptr() + 4, out[2].data_ptr())
    nulls = (C.c_void_p * K)(None, None, None)
    idx = (C.c_void_p * K)(bad.data_ptr(), bad_1.data_ptr(), bad.data_ptr())
    words = (C.c_float * (11 * K))()
    ld, sp = buf._ld, spread.data_ptr()
    assert lib.iqlhip_group_score_rows(g, rows, ld, sizes, 0, 64, idx, outs, sp, 0, words, st) == hb.E_INDEX
    assert "member 1" in hb.last_error() and str(N_ROWS) in hb.last_error()
    c_calls = {
        "misaligned out": (rows, ld, sizes, 0, 64, None, outs_odd, sp, 0, words, st),
        "misaligned spread": (rows, ld, sizes, 0, 64, None, outs, sp + 4, 0, words, st),
        "chunk_rows": (rows, ld, sizes, 0, 64, None, outs, sp, 48, words, st),
        "negative chunk_rows": (rows, ld, sizes, 0, 64, None, outs, sp, -32, words, st),
        "range beyond the smaller buffer": (rows_small, ld, sizes_small, 150, 64, None, outs, sp, 0, words, st),
        "negative row0": (rows, ld, sizes, -1, 64, None, outs, sp, 0, words, st),
        "n < 1": (rows, ld, sizes, 0, 0, None, outs, sp, 0, words, st),
        "stride": (rows, ld - 4, sizes, 0, 64, None, outs, sp, 0, words, st),
        "nothing to write": (rows, ld, sizes, 0, 64, None, nulls, None, 0, None, st),
        "nothing to write (no table)": (rows, ld, sizes, 0, 64, None, None, None, 0, None, st),
    }
    for what, args in c_calls.items():
        assert lib.iqlhip_group_score_rows(g, *args) == hb.E_INVAL, what
    with pytest.raises(ValueError):
        group.score_buffer([buf, small, buf], start=150, n=64, out=out)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 7.0) and np.all(spread.cpu().numpy() == 7.0)
    again, _, sp2 = group.score_buffer(buf, indices=bad, out=out, spread=spread)      # the next valid call is correct
    assert again is out and sp2 is spread and np.array_equal(_bits(out), good)
    _check_spread(out, spread, "after refusals")


def _live():
    gc.collect()
    return int(_hip()[1].lib().iqlhip_debug_live_buffers())


def _free_bytes():
    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info()[0])


def test_scratch_is_taken_by_the_first_group_scoring_call_only_and_returned():
    """Counts of owned buffers (exact integers) and the device's free memory around the first scoring call: creating a
    group — and training with it — takes no scoring scratch; the first scoring call takes it, later ones nothing; a
    group of 8 takes no more than a group of 2; destroying the group returns everything.
    The byte bound: the cap per member is 65 536 / K rows, so the row-sized regions are equal; only the record tables
    and the [K][16] running sums grow with K (well inside 64 KiB), and each of the six device allocations may round up
    by one 2 MiB granule of the device allocator."""
    S, A = 17, 6
    buf = _buffer(S, A)
    buf.sample(8)                                 # (the library's process-wide index staging ring, taken by the first sample)
    taken = {}
    for K in (2, 8):
        members = [_member(S, A, True, i) for i in range(K)]
        for t in members:
            t.score_buffer(buf, n=40)                 # (the members' own scratch: not the group's)
        base = _live()
        group = _hip()[0].ImplicitQLearningGroup(members)
        group.train_steps(buf, 2, 64, list(range(K)))
        out = torch.empty((K, 40, 8), dtype=torch.float32, device="cuda")   # (no torch allocation inside the window)
        held = _live()
        assert held > base
        free = _free_bytes()
        group.score_buffer(buf, n=40, out=out, summary=False)
        taken[K] = free - _free_bytes()
        first = _live() - held
        print(f"K={K}: first scoring call took {first} buffers, {taken[K]} device bytes")
        assert first > 0 and taken[K] > 0
        group.score_buffer(buf, chunk_rows=64, spread=True)
        group.evaluate(buf.sample(100))
        group.score_buffer(buf, indices=np.arange(5), out=False)
        group.train_steps(buf, 2, 64, list(range(K)))
        assert _live() - held == first
        taken[("count", K)] = first
        group._release()
        assert _live() == base
        del group, members, t
    assert taken[("count", 8)] == taken[("count", 2)]
    assert taken[8] <= taken[2] + 6 * (2 << 20) + 64 * 1024, taken


def test_spread_through_the_groups_scratch_rows_across_chunks():
    """out=False with spread=True over more than one chunk: the members' rows go through the group's chunk-sized
    scratch (restarted at every chunk) — the spread must be bit for bit the unchunked call's, and that of a call that
    was given an out."""
    group, members = _group(3)
    buf = _buffer(17, 6)
    _, _, whole = group.score_buffer(buf, n=600, out=False, summary=False, spread=True)
    _, _, cut = group.score_buffer(buf, n=600, out=False, summary=False, spread=True, chunk_rows=64)
    scores, _, with_out = group.score_buffer(buf, n=600, summary=False, spread=True, chunk_rows=64)
    assert np.array_equal(_bits(cut), _bits(whole)) and np.array_equal(_bits(cut), _bits(with_out))
    _check_spread(scores, cut, "chunked, no out")
