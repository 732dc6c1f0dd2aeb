"""GPU tests of the n-step rows (iqlhip_rows_nstep, iqlhip_rows_nstep_ring, iqlhip_online_step_nstep; NStepReplay,
ImplicitQLearning.online_step_nstep).  Derived rows and step counts are compared bit for bit with the CPU
restatement tests/nstep_ref.py; the fused online call bit for bit with the eager sequence it replaces.

The parity test.  score_buffer's `target_q` column is the target critics' minimum, not the TD target; the kernel's TD
target y = r + ((1.f - d) * discount) * next_v is no column.  The test therefore forms y in fp32 from the derived rows'
r and d and score_buffer's `next_v` column — the kernel's own expression on the kernel's own V(s') — and holds it to the
bound tests/test_hip_score.py holds next_v and target_q to (helpers.rel_err <= 2e-5) against the float64 brute-force
target built from the RAW rows and the float64 torch ValueFunction.  MARGIN lines: profiles/nstep_parity_margins.txt."""
import copy

import numpy as np
import pytest
import torch

import nstep_ref as R
import synth
from helpers import rel_err
from nstep_cases import pack, packed_rows, ring_transitions

pytestmark = pytest.mark.gpu

HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
DIMS = [(3, 2), (17, 6)]


def _hip():
    import iql
    import iqlhip_binding as hb
    import hip_helpers
    return iql, hb, hip_helpers


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _raw_buffer(rows, S, A, capacity=None):
    """A GPU ReplayBuffer holding the packed host rows as they are (pad columns included)."""
    iql = _hip()[0]
    n = rows.shape[0]
    buf = iql.ReplayBuffer(S, A, capacity or n, "cuda")
    assert buf._ld == rows.shape[1]
    buf._rows[:n].copy_(torch.from_numpy(rows))
    buf._size, buf._pointer = n, min(n, buf._buffer_size)
    return buf


def _trainer(S, A, seed=3):
    params = synth.synth_params(S, A, seed=seed, gaussian=True)
    return _hip()[2].build_hip_trainer(params, S, A, True, HYPER, LRS, 1000), params


def _check_build(rows, S, A, N, what, episodes_kw=None):
    raw = _raw_buffer(rows, S, A)
    episodes = None if episodes_kw is None else raw.episode_returns(1000, 0.99, **episodes_kw)
    ns = raw.nstep(N, 0.99, episodes=episodes)
    ep_last = None if episodes is None else episodes.ep_last.cpu().numpy()
    want, want_steps = R.build(rows, S, A, N, 0.99, ep_last)
    n = rows.shape[0]
    assert ns.buffer._size == n and ns.buffer._pointer == raw._pointer and ns.n == N and ns.discount == 0.99
    assert np.array_equal(_bits(ns.buffer._rows.cpu().numpy()), _bits(want)), what
    assert ns.steps.dtype == torch.uint8 and np.array_equal(ns.steps.cpu().numpy(), want_steps), what
    assert np.array_equal(_bits(raw._rows.cpu().numpy()), _bits(rows)), what          # the source rows are only read
    return ns, ep_last, want_steps


# ---- build ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,A", DIMS)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 600])
def test_build_matches_the_restatement(S, A, n):
    """16 rows per block of 256 lanes: 255 / 256 / 257 rows end in a partial block, a full one and one row of the next;
    episodes of 1, 2, N - 1, N and N + 1 rows; done on the first and the last row; with and without the episode table
    (keep_tail off: the tail rows carry -1 and fall back to the end of the range)."""
    N = 5
    rng = np.random.default_rng(1000 * S + n)
    rows, ends = packed_rows(rng, n, S, A, N, first_done=n > 1, last_done=n > 2)
    _check_build(rows, S, A, N, "no table")
    _, ep_last, steps = _check_build(rows, S, A, N, "table, tail off", dict(state_break_tol=1e-6, keep_tail=False))
    rows2, ends2 = packed_rows(rng, n, S, A, N)
    _, ep_last2, _ = _check_build(rows2, S, A, N, "table, tail off, open end", dict(state_break_tol=1e-6, keep_tail=False))
    if n >= 255:
        assert (ep_last2 == -1).any() or ends2[-1]                 # a tail that belongs to no episode (or none was cut)
        assert set(np.unique(steps)) == set(range(1, N + 1))       # every chain length occurs
    _check_build(rows2, S, A, N, "table, tail kept", dict(state_break_tol=1e-6, keep_tail=True))


@pytest.mark.parametrize("N", [1, 2, 16, 17, 33, 64])
def test_build_at_other_horizons(N):
    """N = 1: the identity, bit for bit.  16 / 17, 33, 64: one, two, three and four rounds of 16 chain rows per group."""
    S, A, n = 17, 6, 300
    rng = np.random.default_rng(N)
    rows, _ = packed_rows(rng, n, S, A, N)
    rows[:, 2 * S + A + 1] *= (rng.random(n) < 0.3)                  # long chains too: most episode ends are time limits
    ns, _, steps = _check_build(rows, S, A, N, f"N={N}")
    _check_build(rows, S, A, N, f"N={N}, table", dict(state_break_tol=1e-6, keep_tail=True))
    assert steps.max() == N                                          # (a chain of every round count exists)
    if N == 1:
        assert np.array_equal(_bits(ns.buffer._rows.cpu().numpy()), _bits(rows)) and np.all(steps == 1)


def test_rebuild_follows_the_raw_rows():
    S, A, N = 17, 6, 3
    rows, _ = packed_rows(np.random.default_rng(4), 300, S, A, N)
    raw = _raw_buffer(rows, S, A)
    ns = raw.nstep(N, 0.99)
    writes = ns.buffer._writes
    raw.modify_reward_("antmaze-umaze-v2")
    ns.rebuild()
    assert ns.buffer._writes > writes
    want, _ = R.build(raw._rows.cpu().numpy(), S, A, N, 0.99)
    assert np.array_equal(_bits(ns.buffer._rows.cpu().numpy()), _bits(want))


def test_row_offsets_beyond_32_bits():
    """10 M rows of 432 bytes: the stores cross the 2^31 and the 2^32 byte lines.  The last 2 000 rows and 1 000 rows
    across each line match the restatement run on the downloaded rows."""
    iql = _hip()[0]
    S, A, N, n = 39, 28, 5, 10_000_000
    raw = iql.ReplayBuffer(S, A, n, "cuda")
    raw.fill_synthetic(n, seed=3, p_done=0.05)
    assert raw._ld * 4 * n > 2 ** 32
    ns = raw.nstep(N, 0.99)
    for lo in (n - 2000 - N, 2 ** 31 // (raw._ld * 4) - 500, 2 ** 32 // (raw._ld * 4) - 500):
        hi = min(lo + 1000 + N, n) if lo < n - 2000 - N else n
        src = raw._rows[lo:hi].cpu().numpy()
        want, want_steps = R.build(src, S, A, N, 0.99)
        keep = hi - lo if hi == n else 1000                          # (rows whose chains stay inside the download)
        assert np.array_equal(_bits(ns.buffer._rows[lo: lo + keep].cpu().numpy()), _bits(want[:keep])), lo
        assert np.array_equal(ns.steps[lo: lo + keep].cpu().numpy(), want_steps[:keep]), lo
        assert want_steps.max() == N and want_steps.min() == 1


# ---- ring ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,A", DIMS)
@pytest.mark.parametrize("capacity", [3, 7, 16])
def test_incremental_ring_equals_rebuild_on_the_device(S, A, capacity):
    iql = _hip()[0]
    N, disc = 5, 0.99
    rng = np.random.default_rng(capacity)
    raw = iql.ReplayBuffer(S, A, capacity, "cuda")
    ns = raw.nstep(N, disc)
    ld = raw._ld
    h_raw = np.zeros((capacity, ld), dtype=np.float32)
    h_der = np.zeros((capacity, ld), dtype=np.float32)
    h_ends, h_steps = np.zeros(capacity, dtype=np.uint8), np.zeros(capacity, dtype=np.uint8)
    size = pointer = 0
    for it, t in enumerate(ring_transitions(rng, 40, S, A, N)):
        writes = ns.buffer._writes
        ns.add_transition(*t[:5], episode_end=t[5])
        h_raw[pointer], h_ends[pointer] = pack(S, A, ld, t), t[5]
        newest, pointer, size = pointer, (pointer + 1) % capacity, min(size + 1, capacity)
        R.ring_refresh(h_raw, h_der, h_ends, capacity, size, newest, N, disc, S, A, h_steps)
        assert (ns.buffer._size, ns.buffer._pointer) == (raw._size, raw._pointer) == (size, pointer)
        assert ns.buffer._writes > writes
        assert np.array_equal(_bits(raw._rows.cpu().numpy()), _bits(h_raw)), it
        assert np.array_equal(ns.ends.cpu().numpy(), h_ends), it
        order = R.unroll(capacity, size, newest)
        got, got_steps = ns.buffer._rows.cpu().numpy()[order], ns.steps.cpu().numpy()[order]
        assert np.array_equal(_bits(got), _bits(h_der[order])) and np.array_equal(got_steps, h_steps[order]), it
        want, want_steps = R.build(h_raw[order], S, A, N, disc, R.ep_last_from_ends(h_ends[order]))
        assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(got_steps, want_steps), it


def test_add_transition_enters_the_new_row_into_a_tracking_table():
    iql = _hip()[0]
    S, A = 3, 2
    raw = iql.ReplayBuffer(S, A, 8, "cuda")
    ns = raw.nstep(3, 0.99)
    stream = ring_transitions(np.random.default_rng(0), 6, S, A, 3)
    for t in stream[:4]:
        ns.add_transition(*t[:5], episode_end=t[5])
    ns.buffer.set_sample_weights(np.full(4, 0.5, dtype=np.float32), updatable=True, max_weight=4.0, track_max=True,
                                 new_row_weight=2.0)
    version = ns.buffer._weights_version
    ns.add_transition(*stream[4][:5], episode_end=stream[4][5])
    assert ns.buffer._weights_version == version + 1
    idx = ns.buffer.draw_weighted_indices(4096, 1, 0).cpu().numpy()
    assert 0.4 < np.mean(idx == 4) < 0.6                             # weight 2 of 0.5 * 4 + 2


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_train_steps_on_a_horizon_one_buffer_equals_the_raw_buffer():
    H = _hip()[2]
    S, A, n = 17, 6, 600
    rows, _ = packed_rows(np.random.default_rng(8), n, S, A, 5)
    raw = _raw_buffer(rows, S, A)
    ns = raw.nstep(1, 0.99)
    a, _ = _trainer(S, A)
    b, _ = _trainer(S, A)
    la = a.train_steps(raw, 8, 256, seed=5)
    lb = b.train_steps(ns.buffer, 8, 256, seed=5)
    assert np.array_equal(np.asarray(la), np.asarray(lb))
    H.assert_same_trainer_state(a, b, "N = 1 derived vs raw")


def test_three_step_targets_through_score_buffer():
    """See the module docstring: y from the derived rows and score_buffer's next_v against the float64 brute force."""
    iql, hb, _ = _hip()
    S, A, N, n = 17, 6, 3, 256
    rows, ends = packed_rows(np.random.default_rng(21), n, S, A, N, last_done=True)
    raw = _raw_buffer(rows, S, A)
    tr, _ = _trainer(S, A, seed=5)
    vf64 = copy.deepcopy(tr.vf).double()
    with torch.no_grad():
        v_raw = vf64(raw._next_states[:n].double()).cpu().numpy().reshape(-1)      # V of every raw row's own s'
    worst = 0.0
    for tag, kw in (("no table", None), ("table", dict(state_break_tol=1e-6, keep_tail=True))):
        episodes = None if kw is None else raw.episode_returns(1000, 0.99, **kw)
        ns = raw.nstep(N, HYPER["discount"], episodes=episodes)
        ep_last = None if episodes is None else episodes.ep_last.cpu().numpy()
        want = R.brute_force_target(rows, S, A, N, HYPER["discount"], v_raw, ep_last)
        scores, _ = tr.score_buffer(ns.buffer)
        next_v = scores[:, hb.SCORE_NAMES.index("next_v")].cpu().numpy()
        der = ns.buffer._rows.cpu().numpy()
        y = der[:, 2 * S + A] + ((np.float32(1) - der[:, 2 * S + A + 1]) * np.float32(HYPER["discount"])) * next_v
        assert y.dtype == np.float32
        e = rel_err(y, want)
        print(f"MARGIN nstep N={N} {tag} td_target {e / 2e-5:.3f}  (rel_err {e:.3e}, bound 2e-5, "
              f"steps {np.bincount(ns.steps.cpu().numpy(), minlength=N + 1)[1:].tolist()})")
        worst = max(worst, e)
        assert e <= 2e-5, (tag, e)
        # the one-step target of the same rows is a different number: the check can tell the two apart
        y1 = rows[:, 2 * S + A] + ((np.float32(1) - rows[:, 2 * S + A + 1]) * np.float32(HYPER["discount"])) * v_raw.astype(np.float32)
        assert rel_err(y1, want) > 1e-2
    assert worst > 0.0


def _fused_pair(S, A, capacity, N, B):
    iql = _hip()[0]
    out = []
    for _ in range(2):
        raw = iql.ReplayBuffer(S, A, capacity, "cuda")
        out.append((raw.nstep(N, HYPER["discount"]), _trainer(S, A)[0]))
    return out


@pytest.mark.parametrize("S,A", DIMS)
def test_fused_online_step_equals_the_eager_sequence(S, A):
    """12 iterations on a ring of 8 (it wraps), with act_next: parameters, Adam moments, losses, both rings, steps, end
    bytes and the returned actions.  A plain online_step on a third trainer alongside does not disturb either."""
    iql, _, H = _hip()
    N, B, cap = 3, 16, 8
    (ns_g, g), (ns_t, t) = _fused_pair(S, A, cap, N, B)
    other, ring_o = _trainer(S, A, seed=9)[0], iql.ReplayBuffer(S, A, cap, "cuda")
    other_twin, ring_ot = _trainer(S, A, seed=9)[0], iql.ReplayBuffer(S, A, cap, "cuda")
    stream = ring_transitions(np.random.default_rng(4), 12, S, A, N)
    np.random.seed(5)
    got, longest = [], 0
    for tr_ in stream:
        got.append(g.online_step_nstep(ns_g, *tr_[:5], B, episode_end=tr_[5], act_next=tr_[3]))
        other.online_step(ring_o, *tr_[:5], B)
    np.random.seed(5)
    for it, tr_ in enumerate(stream):
        ns_t.add_transition(*tr_[:5], episode_end=tr_[5])
        log = t.train(ns_t.buffer.sample(B))
        a = t.act_one(tr_[3], t.actor.max_action, sample=t.actor.training)
        other_twin.online_step(ring_ot, *tr_[:5], B)
        assert got[it][0] == log, (it, got[it][0], log)
        assert np.array_equal(got[it][1], a), it
        assert all(np.isfinite(v) for v in log.values())
        longest = max(longest, int(ns_t.steps.max()))
    H.assert_same_trainer_state(g, t, "one call vs the eager sequence")
    H.assert_same_trainer_state(other, other_twin, "the plain online step alongside")
    for name in ("raw", "buffer"):
        bg, bt = getattr(ns_g, name), getattr(ns_t, name)
        assert torch.equal(bg._rows.view(torch.int32), bt._rows.view(torch.int32)), name
        assert (bg._size, bg._pointer) == (bt._size, bt._pointer) == (cap, 12 % cap), name
    assert torch.equal(ns_g.steps, ns_t.steps) and torch.equal(ns_g.ends, ns_t.ends)
    assert torch.equal(ring_o._rows, ring_ot._rows)
    assert longest == N                                              # (chains of every length were refreshed)


def test_writes_invalidate_a_train_steps_continuation_on_the_derived_buffer():
    """Two even-length train_steps calls with one seed: the second is offered as a continuation of the first.  A ring
    refresh in between rewrites rows the first call staged ahead; the buffer's write count must withhold the flag.  The
    twin runs the same steps eagerly on the same device-drawn indices.  The ring is full (40 rows, the oldest at
    position 0), so the insert leaves its size — which a continuation also depends on — as it was."""
    iql, _, H = _hip()
    S, A, N, B, K = 17, 6, 3, 256, 6
    rows, _ = packed_rows(np.random.default_rng(12), 40, S, A, N)
    nss = []
    for _ in range(2):
        raw = _raw_buffer(rows, S, A)
        raw._pointer = 0
        nss.append(raw.nstep(N, 0.99))
    a, b = _trainer(S, A)[0], _trainer(S, A)[0]
    t = ring_transitions(np.random.default_rng(3), 1, S, A, N)[0]
    la = [a.train_steps(nss[0].buffer, K, B, seed=5)]
    lb = [H.eager_segment(b, nss[1].buffer, K, B, 5)]
    before = nss[0].buffer._rows.clone()
    for ns in nss:
        writes = ns.buffer._writes
        ns.add_transition(*t[:5], episode_end=t[5])
        assert ns.buffer._writes > writes
    assert not torch.equal(nss[0].buffer._rows, before)
    la.append(a.train_steps(nss[0].buffer, K, B, seed=5))
    lb.append(H.eager_segment(b, nss[1].buffer, K, B, 5))
    assert np.array_equal(np.asarray(la, dtype=np.float32).reshape(-1, 3), np.asarray(lb, dtype=np.float32).reshape(-1, 3))
    H.assert_same_trainer_state(a, b, "train_steps across a ring refresh")


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    iql, hb, _ = _hip()
    S, A = 3, 2
    rows, _ = packed_rows(np.random.default_rng(1), 20, S, A, 3)
    raw = _raw_buffer(rows, S, A)
    for n, disc, match in ((0, 0.99, "horizon"), (65, 0.99, "horizon"), (3, 0.0, "discount"), (3, 1.5, "discount"),
                           (3, float("nan"), "discount")):
        with pytest.raises(ValueError, match=match):
            raw.nstep(n, disc)
    episodes = _raw_buffer(rows[:10], S, A).episode_returns(1000, 0.99)
    with pytest.raises(ValueError, match="episodes table covers"):
        raw.nstep(3, 0.99, episodes=episodes)
    ns = raw.nstep(3, 0.99)
    before = ns.buffer._rows.clone()
    p = raw._rows.data_ptr()
    assert hb.lib().iqlhip_rows_nstep(p, raw._ld, p, raw._ld, S, A, 0, 20, 3, 0.99, None, None, raw._stream()) == hb.E_INVAL
    assert "in place" in hb.last_error()
    assert hb.lib().iqlhip_rows_nstep_ring(p, p, raw._ld, S, A, 20, 20, 19, ns.ends.data_ptr(), 3, 0.99, None,
                                           raw._stream()) == hb.E_INVAL
    tr, _ = _trainer(S, A)
    state = H_state(tr)
    tr._dp_exchange = "p2p"                                          # (what enable_data_parallel records)
    try:
        with pytest.raises(NotImplementedError, match="data parallelism"):
            tr.online_step_nstep(ns, rows[0, :S], rows[0, S:S + A], 0.5, rows[0, :S], False, 8)
    finally:
        tr._dp_exchange = None
    torch.cuda.synchronize()
    assert torch.equal(ns.buffer._rows, before) and np.array_equal(_bits(raw._rows.cpu().numpy()), _bits(rows))
    assert np.array_equal(H_state(tr), state) and tr.total_it == 0


def H_state(tr):
    return _hip()[2].arenas(tr)
