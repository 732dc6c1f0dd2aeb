"""GPU tests that pin the library's four device random streams — the replay-row index draw, the actor-dropout
keep-bits, the act() noise and the synthetic buffer fill — to the CPU Philox reference oracle/philox_ref.py (itself
pinned by tests/test_philox_ref_cpu.py), at every site that draws: the exposed draw kernel, the direct head and the chunk
graphs of train_steps, the eager and the group mask kernels, the forward's idle blocks, iqlhip_actor_sample / the group
actor forward and iqlhip_rows_fill_synth.  Integer streams and everything computed from them are compared for
equality; the Box-Muller normals within Z_TOL.

Z_TOL: the device evaluates sqrtf(-2 logf(u1)) * cosf(2 pi u2) in float32, the reference in float64.  Measured on an
MI355X over the 4096 x 28 act() case: max |z_device - z_reference| = 4.695e-7 (profiles/r05_rng_stream_tests.txt);
the tolerance is four times that.  A wrong word, counter or call number moves a draw by O(1)."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth
from helpers import batch_from, step_batch
from oracle import philox_ref as R

pytestmark = pytest.mark.gpu

Z_MEASURED = 4.695e-7
Z_TOL = 4 * Z_MEASURED
assert Z_TOL <= 1e-5

SEED_HI = 0xDEADBEEF00000001          # keys with a non-zero high word
DROP_SEED = 0xA5A5F00D00C0FFEE
ACT_SEED = 0x9E3779B97F4A7C15
HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}


def _hip():
    import iql
    import iqlhip_binding as hb
    from hip_helpers import build_hip_trainer, read_params, to_torch_batch
    return iql, hb, build_hip_trainer, read_params, to_torch_batch


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _counters(t):
    hb = _hip()[1]
    c = (C.c_uint64 * 2)()
    hb.check(hb.lib().iqlhip_get_counters(t._ctx, c))
    return int(c[0]), int(c[1])


def _set_counters(t, drop=None, act=None):
    hb = _hip()[1]
    cur = _counters(t)
    c = (C.c_uint64 * 2)(cur[0] if drop is None else drop, cur[1] if act is None else act)
    hb.check(hb.lib().iqlhip_set_counters(t._ctx, c))


def _keep_words(t, B):
    return t.debug_read("drop_bits").view(np.uint32).reshape(2, t._max_batch, 8)[:, :B].copy()


def _buffer(data, S, A):
    iql = _hip()[0]
    n = data["observations"].shape[0]
    buf = iql.ReplayBuffer(S, A, n, "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in data.items()})
    return buf


def _assert_same_params(a, b):
    read_params = _hip()[3]
    pa, pb = read_params(a), read_params(b)
    for n in pa:
        for k in pa[n]:
            assert np.array_equal(pa[n][k], pb[n][k]), (n, k)


def _losses(log):
    return [log["value_loss"], log["q_loss"], log["actor_loss"]]


# ------------------------------------------------------------------------------------------------ a. the index draw
@pytest.mark.parametrize("n", [1, 2, 33, 4097])
def test_draw_indices_equals_reference(n):
    """Every (size, seed, offset): with n = 4097 the offset 2^32 - 3 carries into the counter's second word, 2^63 + 5
    has the top bit set; an odd n leaves the element behind the last index alone."""
    hb = _hip()[1]
    idx = torch.empty(n + 3, dtype=torch.int64, device="cuda")
    for size in (1, 2, 1000, 10 ** 7, 2 ** 40 + 12345):
        for seed in (0, 123, SEED_HI):
            for offset in (0, 7, 2 ** 32 - 3, 2 ** 63 + 5):
                idx.fill_(-7)
                hb.check(hb.lib().iqlhip_draw_indices(idx.data_ptr(), n, size, seed, offset, _stream()))
                got = idx.cpu().numpy()
                want = R.draw_indices(n, size, seed, offset)
                assert np.array_equal(got[:n], want), (size, seed, offset, np.flatnonzero(got[:n] != want)[:4])
                assert np.all(got[n:] == -7), (size, seed, offset)


# ------------------------------------------------------------------------------------------------ b. train_steps' rows
@pytest.mark.parametrize("B,calls", [(256, (87,)), (33, (7, 5))])
def test_train_steps_trains_on_the_reference_rows(B, calls):
    """train_steps (direct head, then chunk graphs of 64 / 16 / 4 / 2 / 1 steps whose idle blocks draw the next step's
    rows) against eager train() on batches gathered on the host at the reference's indices: every parameter bitwise,
    the losses equal.  87 steps take the head and every chunk size; with 33 rows a step's first index alternates
    between a counter's first and second word pair, and the second call starts at counter total_it * ceil(B / 2)."""
    _, _, build, _, to_tb = _hip()
    S, A, N = 17, 6, 5000
    params = synth.synth_params(S, A, seed=21)
    data = synth.synth_transitions(N, S, A, seed=22)
    buf = _buffer(data, S, A)
    g = build(params, S, A, True, HYPER, LRS, 1000)
    e = build(params, S, A, True, HYPER, LRS, 1000)
    half, done = (B + 1) // 2, 0
    for K in calls:
        losses = g.train_steps(buf, K, B, seed=SEED_HI)
        idx = R.draw_indices(K * B, N, SEED_HI, done * half).reshape(K, B)
        for k in range(K):
            log = e.train(to_tb(batch_from(data, idx[k])))
            assert _losses(log) == [float(x) for x in losses[k]], (done, k)
        done += K
        assert g.total_it == done
        _assert_same_params(g, e)


# ------------------------------------------------------------------------------------------------ c. eager dropout masks
@pytest.mark.parametrize("p,B,step0", [(0.1, 256, 0), (0.5, 256, 0), (0.1, 100, 0), (0.5, 100, 0),
                                       (0.1, 256, 2 ** 32 - 1)])
def test_eager_dropout_masks_equal_reference(p, B, step0):
    """The keep-bit words three consecutive train() steps read (contexts of max_batch = 256; 100-row steps read the
    first rows of the same words).  From position 2^32 - 1 the second step's counter has a high word."""
    _, _, build, _, to_tb = _hip()
    S, A = 17, 6
    tr = build(synth.synth_params(S, A, seed=41), S, A, True, HYPER, LRS, 1000, dropout=p)
    tr.set_dropout_seed(DROP_SEED)
    assert tr._max_batch == 256
    if step0:
        _set_counters(tr, drop=step0)
    batch = to_tb(step_batch(S, A, B, seed=42))
    for s in range(3):
        tr.train(batch)
        want = R.dropout_keep_words(DROP_SEED, step0 + s, p, 256, B)
        assert np.array_equal(_keep_words(tr, B), want), (s, "keep-bit words differ from the reference")
        assert _counters(tr)[0] == step0 + s + 1


# ------------------------------------------------------------------------------------------------ d. dropout in the graphs
@pytest.mark.parametrize("S,A,B,K,bf16,s0", [(17, 6, 256, 23, False, 2 ** 32 - 7), (39, 28, 1024, 3, True, 5)])
def test_chunk_graph_dropout_equals_reference_masks(S, A, B, K, bf16, s0):
    """train_steps with actor dropout from stream position s0 (the masks of step k + 1 are drawn by the idle blocks of
    forward k; the chunk headers advance the position on the device) equals eager steps on the reference's indices
    with the reference's masks of step s0 + s injected before every step.  23 steps from 2^32 - 7 cross into the high
    word inside a chunk; 1 024 rows in bf16 run the large-batch forward."""
    _, hb, build, _, to_tb = _hip()
    N, p = 4000, 0.2
    params = synth.synth_params(S, A, seed=51)
    data = synth.synth_transitions(N, S, A, seed=52)
    buf = _buffer(data, S, A)
    trainers = []
    for _ in range(2):
        t = build(params, S, A, True, HYPER, LRS, 1000, dropout=p)
        t.reserve_batch(B)
        if bf16:
            t.set_precision("bf16")
        t.set_dropout_seed(DROP_SEED)
        trainers.append(t)
    g, e = trainers
    MB = g._max_batch
    assert MB == (B + 255) // 256 * 256
    _set_counters(g, drop=s0)
    losses = g.train_steps(buf, K, B, seed=SEED_HI)
    assert _counters(g)[0] == s0 + K
    idx = R.draw_indices(K * B, N, SEED_HI, 0).reshape(K, B)
    for s in range(K):
        words = R.dropout_keep_words(DROP_SEED, s0 + s, p, MB, B)
        k0, k1 = R.keep_masks(words)
        assert np.array_equal(synth.pack_keep_bits(k0), words[0]) and np.array_equal(synth.pack_keep_bits(k1), words[1])
        e.inject_dropout_masks(k0, k1)
        log = e.train(to_tb(batch_from(data, idx[s])))
        assert _losses(log) == [float(x) for x in losses[s]], s
    _assert_same_params(g, e)


# ------------------------------------------------------------------------------------------------ e. group masks
def test_group_step_masks_equal_reference():
    """One group step of three members with their own seeds, rates (one of them 0), stream positions and context
    sizes: each drawing member's keep-bit words, rows < B, are the reference's at that member's position."""
    iql, _, build, _, to_tb = _hip()
    S, A, B = 17, 6, 100
    spec = [(0.1, DROP_SEED, 3, 256), (0.0, 17, 0, 256), (0.3, 0x0000000700000009, 2 ** 32 + 4, 512)]
    members = []
    for i, (p, seed, pos, mb) in enumerate(spec):
        t = build(synth.synth_params(S, A, seed=300 + i), S, A, True, HYPER, LRS, 1000, dropout=max(p, 0.1))
        if p == 0.0:
            for m in t.actor.modules():
                if isinstance(m, torch.nn.Dropout):
                    m.p = 0.0
        t.reserve_batch(mb)
        assert t._max_batch == mb
        t.set_dropout_seed(seed)
        _set_counters(t, drop=pos)
        members.append(t)
    group = iql.ImplicitQLearningGroup(members, actor_dropout=True)
    logs = group.train([to_tb(step_batch(S, A, B, seed=60 + i)) for i in range(3)])
    assert all(np.isfinite(v) for log in logs for v in log.values())
    for i, (p, seed, pos, mb) in enumerate(spec):
        if p == 0.0:
            assert _counters(members[i])[0] == pos
            continue
        want = R.dropout_keep_words(seed, pos, p, mb, B)
        assert np.array_equal(_keep_words(members[i], B), want), i
        assert _counters(members[i])[0] == pos + 1


# ------------------------------------------------------------------------------------------------ f. act() noise
def _actor_forward(tr, states, noise, max_action):
    hb = _hip()[1]
    out = torch.full((states.shape[0], tr._A), 99.0, dtype=torch.float32, device="cuda")
    hb.check(hb.lib().iqlhip_actor_forward(tr._ctx, states.data_ptr(), states.stride(0), states.shape[0],
                                           noise.data_ptr(), noise.stride(0), max_action, out.data_ptr(), out.stride(0),
                                           _stream()))
    torch.cuda.synchronize()
    return out


def _noise_probe(S, A, seed=71):
    """A Gaussian policy that returns the device's z itself: last layer zero (the mean is tanh(0) = 0), max_action = 8
    and sigma = exp(log_std) = 1/8, so that action = clamp(8 * (0 + z / 8), -8, 8) = z exactly — both factors are
    powers of two — and never clamped, |z| <= 5.9.  (With log_std = 0 the action 8 z would be clamped at |z| > 1: the
    clamp is at max_action.)  log_std is the float32 next to -ln 8 whose device exp() is 1/8 exactly; that it is gets
    checked through iqlhip_actor_forward on noise = 1."""
    build = _hip()[2]
    x0 = np.float32(-np.log(8.0))
    cands = [x0]
    for k in (1, 2):
        lo = hi = x0
        for _ in range(k):
            lo, hi = np.nextafter(lo, np.float32(-3)), np.nextafter(hi, np.float32(0))
        cands += [lo, hi]
    states = torch.zeros((1, S), dtype=torch.float32, device="cuda")
    ones = torch.ones((1, A), dtype=torch.float32, device="cuda")
    for x in cands:
        params = synth.synth_params(S, A, seed=seed, gaussian=True)
        params["pi"]["w2"] = np.zeros_like(params["pi"]["w2"])
        params["pi"]["b2"] = np.zeros_like(params["pi"]["b2"])
        params["pi"]["log_std"] = np.full(A, x, dtype=np.float32)
        tr = build(params, S, A, True, HYPER, LRS, 1000, max_action=8.0)
        if bool((_actor_forward(tr, states, ones, 8.0) == 1.0).all()):
            return tr
    pytest.fail("no float32 log_std next to -ln 8 gives sigma = 1/8 on this device")


def _actor_sample(tr, states, seed, max_action):
    hb = _hip()[1]
    out = torch.full((states.shape[0], tr._A), 99.0, dtype=torch.float32, device="cuda")
    hb.check(hb.lib().iqlhip_actor_sample(tr._ctx, states.data_ptr(), states.stride(0), states.shape[0], seed,
                                          max_action, out.data_ptr(), out.stride(0), _stream()))
    torch.cuda.synchronize()
    return out


def _device_z(actions):
    z = actions.cpu().numpy()
    assert np.abs(z).max() < 8.0                       # nothing clamped
    return z


@pytest.mark.parametrize("S,A,call0", [(17, 6, 0), (39, 28, 2 ** 32 - 1)])
def test_act_noise_equals_reference(S, A, call0):
    """iqlhip_actor_sample on 1, 33 and 4 096 rows (three consecutive call numbers; from 2^32 - 1 the later two have a
    high word), then 5 000 rows through actor_forward(sample=True): two library calls, the element number restarting
    with the second."""
    tr = _noise_probe(S, A)
    _set_counters(tr, act=call0)
    rng = np.random.default_rng(5)
    call = call0
    for rows in (1, 33, 4096):
        states = torch.from_numpy(rng.standard_normal((rows, S)).astype(np.float32)).cuda()
        z = _device_z(_actor_sample(tr, states, ACT_SEED, 8.0))
        want = R.act_noise(ACT_SEED, call, rows, A)
        err = float(np.abs(z - want).max())
        print(f"act noise rows={rows} A={A} call={call}: max |z_device - z_reference| = {err:.3e}")
        assert err <= Z_TOL, (rows, call, err)
        call += 1
        assert _counters(tr)[1] == call
    states = torch.from_numpy(rng.standard_normal((5000, S)).astype(np.float32)).cuda()
    key = tr._act_seed()
    z = _device_z(tr.actor_forward(states, sample=True))
    want = np.concatenate([R.act_noise(key, call, 4096, A), R.act_noise(key, call + 1, 5000 - 4096, A)])
    err = float(np.abs(z - want).max())
    print(f"act noise 5000 rows A={A}: max |z_device - z_reference| = {err:.3e}")
    assert err <= Z_TOL, err
    assert _counters(tr)[1] == call + 2


def test_group_actor_forward_noise_equals_reference():
    """The group's sampling forward: each member's noise is the reference's under that member's key and call number."""
    iql = _hip()[0]
    S, A = 17, 6
    members = [_noise_probe(S, A, seed=71 + i) for i in range(2)]
    calls = (2 ** 32 + 3, 6)
    for t, c in zip(members, calls):
        _set_counters(t, act=c)
    members[1]._act_key = ACT_SEED
    rng = np.random.default_rng(6)
    rows = (33, 5)
    states = [torch.from_numpy(rng.standard_normal((n, S)).astype(np.float32)).cuda() for n in rows]
    outs = iql.ImplicitQLearningGroup(members).actor_forward(states, sample=True)
    torch.cuda.synchronize()
    for t, c, n, out in zip(members, calls, rows, outs):
        err = float(np.abs(_device_z(out) - R.act_noise(t._act_seed(), c, n, A)).max())
        assert err <= Z_TOL, (n, err)
        assert _counters(t)[1] == c + 1


def test_actor_sample_equals_actor_forward_on_the_same_noise():
    """With trained-like parameters and a log_std vector spanning both clamps, iqlhip_actor_sample is — bitwise —
    iqlhip_actor_forward given the device's own z (read through the zero-head probe) as noise_dev."""
    build = _hip()[2]
    S, A, rows, call = 17, 6, 333, 2 ** 32 + 9
    probe = _noise_probe(S, A)
    _set_counters(probe, act=call)
    states = torch.from_numpy(np.random.default_rng(7).standard_normal((rows, S)).astype(np.float32)).cuda()
    z = _device_z(_actor_sample(probe, states, ACT_SEED, 8.0))
    assert float(np.abs(z - R.act_noise(ACT_SEED, call, rows, A)).max()) <= Z_TOL
    params = synth.synth_params(S, A, seed=72, gaussian=True)
    params["pi"]["log_std"] = np.array([3.0, -25.0, 0.5, 2.0, -20.0, -1.0], dtype=np.float32)
    tr = build(params, S, A, True, HYPER, LRS, 1000, max_action=1.0)
    _set_counters(tr, act=call)
    sampled = _actor_sample(tr, states, ACT_SEED, 1.0).cpu().numpy()
    given = _actor_forward(tr, states, torch.from_numpy(z).cuda(), 1.0).cpu().numpy()
    assert sampled.tobytes() == given.tobytes()
    assert np.any(np.abs(sampled) == 1.0) and np.any(np.abs(sampled) < 1.0)          # clamped and unclamped actions


# ------------------------------------------------------------------------------------------------ g. the synthetic fill
SENTINEL = -777.25


def _fill(S, A, total, row0, n, seed, p_done, antmaze):
    hb = _hip()[1]
    ld = hb.row_stride(S, A)
    rows = torch.full((total, ld), SENTINEL, dtype=torch.float32, device="cuda")
    hb.check(hb.lib().iqlhip_rows_fill_synth(rows.data_ptr(), ld, S, A, row0, n, seed, p_done, int(antmaze), _stream()))
    torch.cuda.synchronize()
    return rows.cpu().numpy()


@pytest.mark.parametrize("S,A", [(17, 6), (3, 9)])
@pytest.mark.parametrize("p_done", [0.0, 0.01, 1.0])
def test_synthetic_fill_equals_reference(S, A, p_done):
    iql, hb, _, _, _ = _hip()
    W, ld, n, total = 2 * S + A + 2, hb.row_stride(S, A), 1000, 1100
    assert ld == (W + 3) // 4 * 4 and ld > W
    for antmaze in (False, True):
        got = _fill(S, A, total, 0, n, SEED_HI, p_done, antmaze)
        want, exact = R.fill_rows(SEED_HI, 0, n, S, A, p_done, antmaze)
        assert np.array_equal(got[:n, :W][:, exact], want[:, exact].astype(np.float32)), "action / done / antmaze columns"
        err = float(np.abs(got[:n, :W][:, ~exact] - want[:, ~exact]).max())
        assert err <= Z_TOL, err
        assert np.all(got[:n, W:] == np.float32(SENTINEL)) and np.all(got[n:] == np.float32(SENTINEL))
        assert set(np.unique(got[:n, W - 1])) <= ({0.0} if p_done == 0.0 else {1.0} if p_done == 1.0 else {0.0, 1.0})
        # rows are numbered absolutely: a fill of rows 300..349 is that slice of the full fill
        part = _fill(S, A, total, 300, 50, SEED_HI, p_done, antmaze)
        assert part[300:350, :W].tobytes() == got[300:350, :W].tobytes()
        assert np.all(part[:300] == np.float32(SENTINEL)) and np.all(part[350:] == np.float32(SENTINEL))
        assert np.all(part[300:350, W:] == np.float32(SENTINEL))
    # ReplayBuffer.fill_synthetic: the same rows, accounted like load_d4rl_dataset; the five views show them
    buf = iql.ReplayBuffer(S, A, total, "cuda")
    buf.fill_synthetic(n, seed=SEED_HI, p_done=p_done, antmaze_rewards=True)
    ref = iql.ReplayBuffer(S, A, total, "cuda")
    ref.load_d4rl_dataset(synth.synth_transitions(n, S, A, seed=1))
    assert (buf._size, buf._pointer) == (ref._size, ref._pointer) == (n, n)
    with pytest.raises(ValueError):
        buf.fill_synthetic(n, seed=SEED_HI)
    views = (buf._states, buf._actions, buf._next_states, buf._rewards, buf._dones)
    cols = (slice(0, S), slice(S, S + A), slice(S + A, 2 * S + A), slice(2 * S + A, W - 1), slice(W - 1, W))
    for v, c in zip(views, cols):
        assert v.shape == (total, c.stop - c.start)
        assert np.array_equal(v[:n].cpu().numpy(), got[:n, c]) and not v[n:].any()
