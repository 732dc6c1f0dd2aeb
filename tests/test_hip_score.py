"""GPU tests of scoring without a step (ImplicitQLearning.score_buffer / score / evaluate): against the
reference's recorded intermediates, against the numpy oracle (tests/score_ref.py) on all eight columns and the summary,
bitwise independence of a row from everything but itself, bytewise absence of side effects, 64-bit row addressing,
refusals, scratch.

Tolerances.  v, next_v, q1, q2, target_q, adv: helpers' 2e-5 (rel_err: max abs error over max abs value).  exp_adv, bc
and the three losses have no project number: per case the test derives max(2e-5, 4 x rel_err(oracle fp32, oracle fp64))
for that quantity on those inputs, on the CPU — the device and numpy are two fp32 roundings of the same quantity in
different summation orders, each about that far from the fp64 value; 2x covers the pair, 2x more the tail.  A column
mean is held to its column's bound (a mean moves by at most the largest row error).  Observed margins (error / bound,
worst over the cases of the test) are printed as MARGIN lines; profiles/score_parity_margins.txt is that output."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import synth
import score_ref
from helpers import SINGLE_STEP_CASES, assert_losses, load_golden, rel_err, single_step_inputs

pytestmark = pytest.mark.gpu

HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
COL = {name: i for i, name in enumerate(score_ref.SCORE_NAMES)}


def _hip():
    import iql
    import iqlhip_binding as hb
    import hip_helpers
    return iql, hb, hip_helpers


def _trainer(S, A, gaussian=True, seed=3, params=None, hyper=HYPER, **kw):
    params = synth.synth_params(S, A, seed=seed, gaussian=gaussian) if params is None else params
    return _hip()[2].build_hip_trainer(params, S, A, gaussian, hyper, LRS, 1000, **kw), params


def _batch_of(data, sl=slice(None)):
    return {"s": data["observations"][sl], "a": data["actions"][sl], "r": data["rewards"][sl],
            "ns": data["next_observations"][sl], "d": data["terminals"][sl]}


def _buffer(data, S, A, capacity=None):
    iql = _hip()[0]
    n = data["observations"].shape[0]
    buf = iql.ReplayBuffer(S, A, capacity or n, "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in data.items()})
    return buf


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ---- 1. the reference's goldens ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SINGLE_STEP_CASES)
def test_scores_meet_the_recorded_intermediates_and_evaluate_the_recorded_losses(name):
    _, _, hh = _hip()
    z, meta = load_golden(name)
    params, batch, hyper = single_step_inputs(meta)
    tr = hh.build_hip_trainer(params, meta["S"], meta["A"], meta["gaussian"], hyper, meta["lrs"], meta["max_steps"])
    tb = hh.to_torch_batch(batch)
    scores, summary = tr.score(tb)
    got = scores.cpu().numpy()
    assert got.shape == (meta["B"], 8)
    for k in ("next_v", "target_q", "adv"):
        e = rel_err(got[:, COL[k]], z[f"inter.{k}"])
        print(f"MARGIN golden {name} {k} {e / 2e-5:.3f}")
        assert e <= 2e-5, (name, k, e)
    ev = tr.evaluate(tb)
    assert list(ev) == ["value_loss", "q_loss", "actor_loss"]
    assert [ev[k] for k in ev] == [summary[k] for k in ev]
    assert_losses([ev[k] for k in ev], z["losses"], 1e-5, what=name + " evaluate")
    log = tr.train(tb)              # evaluate changed nothing the step depends on
    assert_losses([log["value_loss"], log["q_loss"], log["actor_loss"]], z["losses"], 1e-5, what=name + " train")


# ---- 2. the oracle: all eight columns and the summary -------------------------------------------------------------
SIZES = (1, 31, 32, 33, 257, 600)
PLAIN = ("v", "next_v", "q1", "q2", "target_q", "adv")


def _check_against_oracle(tag, tr, params, data, hyper, sizes):
    _, hb, hh = _hip()
    worst = {}
    for n in sizes:
        batch = _batch_of(data, slice(0, n))
        r32 = score_ref.reference(params, batch, hyper, np.float32)
        r64 = score_ref.reference(params, batch, hyper, np.float64)
        scores, summary = tr.score(hh.to_torch_batch(batch))
        got = scores.cpu().numpy()
        assert got.shape == (n, 8) and got.dtype == np.float32 and np.all(np.isfinite(got))
        for name, i in COL.items():
            tol = 2e-5 if name in PLAIN else max(2e-5, 4 * rel_err(r32["cols"][:, i], r64["cols"][:, i]))
            e = rel_err(got[:, i], r64["cols"][:, i])
            worst[name] = max(worst.get(name, 0.0), e / tol)
            assert e <= tol, (tag, n, name, e, tol)
            scale = float(np.max(np.abs(r64["cols"][:, i])))
            em = abs(summary["mean_" + name] - float(r64["means"][i])) / max(scale, 1e-30)
            worst["mean_" + name] = max(worst.get("mean_" + name, 0.0), em / tol)
            assert em <= tol, (tag, n, "mean_" + name, em, tol)
        for j, name in enumerate(score_ref.LOSS_NAMES):
            want32, want64 = float(r32["losses"][j]), float(r64["losses"][j])
            tol = max(2e-5, 4 * abs(want32 - want64) / abs(want64))
            e = abs(summary[name] - want64) / abs(want64)
            worst[name] = max(worst.get(name, 0.0), e / tol)
            assert e <= tol, (tag, n, name, e, tol)
    print(f"MARGIN oracle {tag} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("gaussian", [True, False])
@pytest.mark.parametrize("S,A", [(11, 3), (17, 6), (39, 28), (100, 28), (20, 32),
                                 (72, 28),      # layer-0 staging split inside the LDS-DMA kernel: V and pi staged, critics not
                                 (127, 1)])     # the widest packed row (65 float4), one action dim
def test_eight_columns_and_summary_against_the_oracle(S, A, gaussian):
    tr, params = _trainer(S, A, gaussian, seed=5)
    data = synth.synth_transitions(max(SIZES), S, A, seed=77)
    hyper = dict(HYPER, deterministic=not gaussian)
    _check_against_oracle(f"S{S}A{A}{'gauss' if gaussian else 'det'}", tr, params, data, hyper, SIZES)


def test_oracle_with_the_weight_clamp_crossed_and_log_std_outside_its_clamp():
    S, A = 17, 6
    params = synth.synth_params(S, A, seed=9, gaussian=True)
    data = synth.synth_transitions(257, S, A, seed=78)
    batch = _batch_of(data)
    adv = score_ref.reference(params, batch, dict(HYPER, deterministic=False), np.float64)["cols"][:, COL["adv"]]
    # beta * adv crosses log(100) inside the batch: the clamp holds for some rows and not for others
    beta = float(np.log(100.0) / np.quantile(adv[adv > 0], 0.5))
    hyper = dict(HYPER, beta=beta, deterministic=False)
    clamped = np.exp(beta * adv) >= 100.0
    assert 0 < clamped.sum() < clamped.size and (adv < 0).any()
    tr, _ = _trainer(S, A, True, params=params, hyper=hyper)
    _check_against_oracle("clamp_crossed", tr, params, data, hyper, (257,))
    got = tr.score(_hip()[2].to_torch_batch(batch))[0].cpu().numpy()[:, COL["exp_adv"]]
    far = np.abs(beta * adv - np.log(100.0)) > 1e-3
    assert np.array_equal((got == 100.0)[far], clamped[far])
    # log_std outside [-20, 2] on both sides (helpers.apply_edge's values)
    params["pi"]["log_std"] = np.array([3.0, -25.0, 0.5, 2.0, -20.0, -1.0], dtype=np.float32)
    hyper = dict(HYPER, deterministic=False)
    tr, _ = _trainer(S, A, True, params=params, hyper=hyper)
    _check_against_oracle("log_std_clamped", tr, params, data, hyper, (257,))


# ---- 3. a row's eight numbers depend on the row alone, bitwise ----------------------------------------------------
def test_row_independence_bitwise():
    S, A, N = 17, 6, 1000
    tr, _ = _trainer(S, A, True, seed=4)
    data = synth.synth_transitions(N, S, A, seed=31)
    buf = _buffer(data, S, A)
    full = _bits(tr.score_buffer(buf, summary=False)[0])
    assert full.shape == (N, 8)
    rng_ = _bits(tr.score_buffer(buf, start=100, n=200, summary=False)[0])
    assert np.array_equal(rng_, full[100:300])
    idx = np.arange(100, 300, dtype=np.int64)
    assert np.array_equal(_bits(tr.score_buffer(buf, indices=idx, summary=False)[0]), rng_)              # host indices
    assert np.array_equal(_bits(tr.score_buffer(buf, indices=torch.from_numpy(idx).cuda())[0]), rng_)    # device indices
    perm = np.random.RandomState(0).permutation(idx)
    assert np.array_equal(_bits(tr.score_buffer(buf, indices=perm, summary=False)[0]), full[perm])
    one = torch.empty((200, 8), dtype=torch.float32, device="cuda")
    for i in range(200):
        tr.score_buffer(buf, start=100 + i, n=1, out=one[i:i + 1], summary=False)
    assert np.array_equal(_bits(one), rng_)
    assert np.array_equal(_bits(tr.score_buffer(buf, start=100, n=200, chunk_rows=64, summary=False)[0]), rng_)
    assert np.array_equal(_bits(tr.score_buffer(buf, chunk_rows=32)[0]), full)
    gathered = buf.gather(torch.from_numpy(idx).cuda())
    assert np.array_equal(_bits(tr.score(gathered, summary=False)[0]), rng_)
    split = _hip()[2].to_torch_batch(_batch_of(data, slice(100, 300)))       # five separate tensors: packed by the call
    assert np.array_equal(_bits(tr.score(split, summary=False)[0]), rng_)
    dup = np.array([7, 7, 999, 0, 7, 999, 512, 512], dtype=np.int64)
    assert np.array_equal(_bits(tr.score_buffer(buf, indices=dup, summary=False)[0]), full[dup])
    # the summary of the same rows does not depend on how they are addressed either (same tiles, same order)
    s_rng = tr.score_buffer(buf, start=100, n=200, out=False)[1]
    s_idx = tr.score_buffer(buf, indices=idx, out=False)[1]
    assert s_rng == s_idx and tr.score_buffer(buf, start=100, n=200, out=False)[0] is None


# ---- 4. no side effects, bytewise ----------------------------------------------------------------------------------
def _counters(tr):
    hb = _hip()[1]
    c = (C.c_uint64 * 2)()
    hb.check(hb.lib().iqlhip_get_counters(tr._ctx, c))
    return int(c[0]), int(c[1])


def _state(tr):
    hh = _hip()[2]
    return hh.arenas(tr).view(np.uint32), _counters(tr), tr.actor_optimizer.param_groups[0]["lr"], tr.total_it, dict(tr._adam_t)


def _assert_same_state(a, b, what):
    sa, sb = _state(a), _state(b)
    assert np.array_equal(sa[0], sb[0]), (what, "arenas")
    assert sa[1:] == sb[1:], (what, sa[1:], sb[1:])


@pytest.mark.parametrize("mode", ["f32_stats_clip", "bf16", "mixed"])
def test_scoring_between_training_calls_changes_nothing(mode):
    S, A, B = 17, 6, 256
    data = synth.synth_transitions(2048, S, A, seed=41)
    buf = _buffer(data, S, A)
    online = _buffer(synth.synth_transitions(300, S, A, seed=42), S, A, capacity=512) if mode == "mixed" else None
    held_out = _hip()[2].to_torch_batch(_batch_of(synth.synth_transitions(333, S, A, seed=43)))
    runs = []
    for with_scoring in (False, True):
        tr, _ = _trainer(S, A, True, seed=6, dropout=0.1 if mode != "bf16" else 0.0)
        if mode == "f32_stats_clip":
            tr.set_step_stats(True)
            tr.set_grad_clip(0.5)
        if mode == "bf16":
            tr.set_precision("bf16")

        def steps(k):
            if mode == "mixed":
                return tr.train_steps_mixed(buf, online, k, B, 0.5, seed=3)
            if mode == "f32_stats_clip":
                return np.concatenate(tr.train_steps(buf, k, B, seed=3, return_stats=True), axis=1)
            return tr.train_steps(buf, k, B, seed=3)

        first = steps(7)
        if with_scoring:
            scores, summary = tr.score_buffer(buf, start=5, n=700)
            ev = tr.evaluate(held_out)
            assert np.all(np.isfinite(scores.cpu().numpy())) and all(np.isfinite(v) for v in ev.values())
            tr.score_buffer(buf, indices=torch.tensor([3, 2000, 77], device="cuda"), out=False)
        second = steps(9)
        runs.append((tr, first, second))
    (a, a1, a2), (b, b1, b2) = runs
    assert np.array_equal(a1.view(np.uint32), b1.view(np.uint32)) and np.array_equal(a2.view(np.uint32), b2.view(np.uint32)), mode
    _assert_same_state(a, b, mode)


def test_bf16_context_scores_with_the_fp32_masters():
    S, A = 17, 6
    data = synth.synth_transitions(300, S, A, seed=44)
    buf = _buffer(data, S, A)
    f32, params = _trainer(S, A, True, seed=8)
    b16, _ = _trainer(S, A, True, params=params)
    b16.set_precision("bf16")
    sa, ma = f32.score_buffer(buf)
    sb, mb = b16.score_buffer(buf)
    assert np.array_equal(_bits(sa), _bits(sb)) and ma == mb


# ---- 5. 64-bit row addressing ---------------------------------------------------------------------------------------
def test_rows_beyond_two_and_four_gib_score_like_their_copies():
    iql, hb, _ = _hip()
    S, A, N = 39, 28, 10_000_000
    ld = hb.row_stride(S, A)
    assert 4 * ld == 432 and N * 4 * ld > 2 ** 32
    buf = iql.ReplayBuffer(S, A, N, "cuda")
    buf.fill_synthetic(N, seed=17)
    tr, _ = _trainer(S, A, True, seed=12)
    for line in (2 ** 31, 2 ** 32):
        r0 = line // (4 * ld) - 32                   # 64 rows with the row that contains byte `line` in their middle
        assert r0 * 4 * ld < line < (r0 + 64) * 4 * ld <= N * 4 * ld
        small = iql.ReplayBuffer(S, A, 64, "cuda")
        small._rows.copy_(buf._rows[r0:r0 + 64])
        small._size = 64
        want = _bits(tr.score_buffer(small, summary=False)[0])
        assert np.any(want != 0)
        by_range, s_range = tr.score_buffer(buf, start=r0, n=64)
        by_index, s_index = tr.score_buffer(buf, indices=torch.arange(r0, r0 + 64, device="cuda"))
        assert np.array_equal(_bits(by_range), want) and np.array_equal(_bits(by_index), want), line
        assert s_range == s_index == tr.score_buffer(small)[1]
    del buf
    gc.collect()
    torch.cuda.empty_cache()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_leave_parameters_and_out_untouched_and_the_next_call_is_correct():
    iql, hb, hh = _hip()
    S, A, N = 17, 6, 400
    tr, _ = _trainer(S, A, True, seed=13)
    buf = _buffer(synth.synth_transitions(N, S, A, seed=45), S, A, capacity=512)      # 400 of 512 rows filled
    good = _bits(tr.score_buffer(buf, summary=False)[0])
    before = hh.arenas(tr).view(np.uint32)
    out = torch.full((64, 8), 7.0, device="cuda")
    lib, ptr, st = hb.lib(), buf._rows.data_ptr(), tr._stream()
    words = (C.c_float * 11)()
    idx_ok = torch.arange(64, device="cuda")
    c_calls = {                                       # section 2: the C entry point itself
        "n < 1": (ptr, buf._ld, N, 0, 0, None, out.data_ptr(), 0, words, st),
        "null rows": (None, buf._ld, N, 0, 64, None, out.data_ptr(), 0, words, st),
        "range beyond n_rows": (ptr, buf._ld, N, N - 63, 64, None, out.data_ptr(), 0, words, st),
        "negative row0": (ptr, buf._ld, N, -1, 64, None, out.data_ptr(), 0, words, st),
        "negative chunk": (ptr, buf._ld, N, 0, 64, None, out.data_ptr(), -32, words, st),
        "chunk not a multiple of 32": (ptr, buf._ld, N, 0, 64, None, out.data_ptr(), 48, words, st),
        "both outputs null": (ptr, buf._ld, N, 0, 64, None, None, 0, None, st),
        "stride": (ptr, buf._ld - 4, N, 0, 64, None, out.data_ptr(), 0, words, st),
    }
    for what, args in c_calls.items():
        assert lib.iqlhip_score_rows(tr._ctx, *args) == hb.E_INVAL, what
    bad_idx = torch.tensor([1, 2, N, 3], device="cuda")
    assert lib.iqlhip_score_rows(tr._ctx, ptr, buf._ld, N, 0, 4, bad_idx.data_ptr(), out.data_ptr(), 0, words, st) == hb.E_INDEX
    assert "out of bounds" in hb.last_error()
    # section 3: the Python surface (a device index list is checked by the library, before its forward)
    py_calls = [
        (ValueError, lambda: tr.score_buffer(iql.ReplayBuffer(S, A, 8, "cpu"))),
        (ValueError, lambda: tr.score_buffer(_buffer(synth.synth_transitions(8, 11, 3, seed=1), 11, 3))),
        (ValueError, lambda: tr.score_buffer(iql.ReplayBuffer(S, A, 8, "cuda"))),              # empty
        (ValueError, lambda: tr.score_buffer(buf, start=N)),
        (ValueError, lambda: tr.score_buffer(buf, start=N - 63, n=64, out=out)),                # start + n > len(buffer)
        (ValueError, lambda: tr.score_buffer(buf, n=64, out=out[:63])),
        (ValueError, lambda: tr.score_buffer(buf, n=64, out=out.double())),
        (ValueError, lambda: tr.score_buffer(buf, n=64, out=out.cpu())),
        (ValueError, lambda: tr.score_buffer(buf, start=1, indices=idx_ok, out=out)),
        (IndexError, lambda: tr.score_buffer(buf, indices=torch.tensor([0, N] + [1] * 62, device="cuda"), out=out)),
        (IndexError, lambda: tr.score_buffer(buf, indices=torch.tensor([-1] + [1] * 63, device="cuda"), out=out)),
        (IndexError, lambda: tr.score_buffer(buf, indices=np.array([450] + [1] * 63), out=out)),    # an unfilled row
    ]
    for exc, call in py_calls:
        with pytest.raises(exc):
            call()
    torch.cuda.synchronize()
    assert np.array_equal(hh.arenas(tr).view(np.uint32), before)
    assert np.all(out.cpu().numpy() == 7.0)
    again, _ = tr.score_buffer(buf, indices=idx_ok, out=out)          # the next valid call is correct
    assert again is out and np.array_equal(_bits(out), good[:64])


# ---- 7. scratch -----------------------------------------------------------------------------------------------------
def _live():
    gc.collect()
    return int(_hip()[1].lib().iqlhip_debug_live_buffers())


def test_scratch_is_taken_by_the_first_scoring_call_only_and_returned():
    """Counts of owned buffers (exact integers).  The scoring scratch is not part of what a context takes when it is
    created or when it trains: the first scoring call of a context that has done both takes exactly the scratch's six
    buffers (were they taken any earlier, that call would take none), later scoring calls take nothing, and a context
    that never scores never holds them."""
    S, A = 17, 6
    buf = _buffer(synth.synth_transitions(600, S, A, seed=46), S, A)
    buf.sample(256)                               # (the library's process-wide index staging ring, taken by the first sample)
    base = _live()
    tr, _ = _trainer(S, A, True, seed=14)
    tr.train_steps(buf, 3, 256, seed=1)
    tr.train(buf.sample(256))
    tr.actor_forward(buf.sample(8)[0])
    held = _live()
    tr.score_buffer(buf)
    assert _live() - held == 6                    # head partials (2), tile partials, running sums, two host-mapped blocks
    tr.score_buffer(buf, chunk_rows=64)
    tr.evaluate(buf.sample(100))
    tr.score_buffer(buf, indices=np.arange(5))
    tr.train_steps(buf, 3, 256, seed=1)
    assert _live() - held == 6                    # ... once, whatever is scored afterwards
    other, _ = _trainer(S, A, True, seed=15)      # the same calls without scoring: nothing is taken once it has trained
    before_other = _live()
    other.train_steps(buf, 3, 256, seed=1)
    other.train(buf.sample(256))
    other.actor_forward(buf.sample(8)[0])
    settled = _live()
    other.train_steps(buf, 3, 256, seed=1)
    other.train(buf.sample(256))
    assert _live() == settled and settled >= before_other
    del tr, other
    assert _live() == base


def test_more_than_one_default_chunk_equals_two_calls():
    S, A, N = 11, 3, 70_000
    iql = _hip()[0]
    buf = iql.ReplayBuffer(S, A, N, "cuda")
    buf.fill_synthetic(N, seed=23)
    tr, _ = _trainer(S, A, True, seed=16)
    whole, s_whole = tr.score_buffer(buf)
    cut = 40_000
    a, s_a = tr.score_buffer(buf, start=0, n=cut)
    b, s_b = tr.score_buffer(buf, start=cut)
    assert np.array_equal(_bits(whole), np.concatenate([_bits(a), _bits(b)]))
    for k in s_whole:
        two = (s_a[k] * cut + s_b[k] * (N - cut)) / N
        assert abs(two - s_whole[k]) <= 1e-6 * abs(s_whole[k]), (k, two, s_whole[k])
