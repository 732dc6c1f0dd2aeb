"""GPU tests of iqlhip_rows_episode_returns / iqlhip_ingest.episode_returns_device / ReplayBuffer.episode_returns: per-row
episode spans, episode returns and discounted return-to-go on packed device rows.  Every comparison is exact against the
CPU restatement tests/returns_ref.py — float64 outputs as int64 bit patterns, spans and counts as integers — and for the
fixture against the reference's recorded get_return_to_go (tests/golden/g18_return_to_go.npz) as well."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth
from helpers import load_golden
from returns_ref import episode_table_ref, rows_episode_returns_ref, top_fraction_weights_ref

pytestmark = pytest.mark.gpu

TILE = 256                      # rows per scan tile (RR_TILE, csrc/iqlhip_kernels.h)
MAX_BLOCKS = 4096               # blocks per launch (RR_MAX_BLOCKS): more tiles than that are walked with a block stride


def _hb():
    import iqlhip_binding as hb
    return hb


def _wide(rng, n):
    """float32 rewards of mixed sign, log-uniform over 1e-6 .. 1e6: any reordered float64 sum differs in its last bits."""
    return (rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-6.0, 6.0, size=n)).astype(np.float32)


def _flags(n, at):
    d = np.zeros(n, np.float32)
    d[list(at)] = 1.0
    return d


def _rows(r, d, S=3, A=1, seed=0, continuous=False):
    """Host packed rows [n, ld]: r and d in their columns, random cells elsewhere (padding included); `continuous`:
    s[i+1] == s'[i] on every row."""
    n, ld = len(r), _hb().row_stride(S, A)
    rng = np.random.default_rng(seed + n)
    host = rng.standard_normal((n, ld)).astype(np.float32)
    if continuous:
        host[1:, :S] = host[:-1, S + A: 2 * S + A]
    host[:, 2 * S + A], host[:, 2 * S + A + 1] = r, d
    return host


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _device(host, S, A, T, discount, tol=None, keep_tail=False, sparse_value=None, row0=0, n=None):
    import iqlhip_ingest as ing
    dev = host if isinstance(host, torch.Tensor) else torch.from_numpy(host).cuda()
    n = dev.shape[0] - row0 if n is None else n
    return ing.episode_returns_device(dev, S, A, n, T, discount, tol, keep_tail, sparse_value, row0=row0)


def _assert_equal(got, want, what):
    ret, rtg, first, last, episodes = want
    assert got.episodes == episodes, (what, got.episodes, episodes)
    assert np.array_equal(got.ep_first.cpu().numpy(), first), what
    assert np.array_equal(got.ep_last.cpu().numpy(), last), what
    assert got.ep_return.dtype == torch.float64 and got.return_to_go.dtype == torch.float64
    assert np.array_equal(_bits(got.ep_return.cpu().numpy()), _bits(ret)), what
    assert np.array_equal(_bits(got.return_to_go.cpu().numpy()), _bits(rtg)), what


def _check(host, S, A, T, discount, what, **kw):
    want = rows_episode_returns_ref(host, S, A, T, discount, kw.get("tol"), kw.get("keep_tail", False), kw.get("sparse_value"))
    dev = torch.from_numpy(host).cuda()
    _assert_equal(_device(dev, S, A, T, discount, **kw), want, what)
    assert np.array_equal(dev.cpu().numpy(), host), what             # reads only
    return want


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513])
def test_sizes_around_a_tile(n):
    rng = np.random.default_rng(n)
    r = _wide(rng, n)
    for name, d in (("random", (rng.random(n) < 0.05).astype(np.float32)), ("none", _flags(n, [])), ("last", _flags(n, [n - 1]))):
        host = _rows(r, d)
        for T in (1, 7, 256, 1000, n + 1):
            for keep_tail in (False, True):
                _check(host, 3, 1, T, 0.99, (n, name, T, keep_tail), keep_tail=keep_tail)


def test_more_than_256_tiles():
    """n = 66 000: more tile partials than one pass of the one-block scan takes; an episode that spans many tiles."""
    rng = np.random.default_rng(66)
    n = 66_000
    d = (rng.random(n) < 0.002).astype(np.float32)
    d[20_000: 24_000] = 0.0                                            # one run of 4 000 rows without a terminal
    host = _rows(_wide(rng, n), d)
    _check(host, 3, 1, 5000, 0.99, "long T")
    _check(host, 3, 1, 1000, 1.0, "T 1000", keep_tail=True)


def test_more_tiles_than_blocks():
    """n above RR_MAX_BLOCKS tiles: every block walks more than one tile, the last tile is ragged."""
    rng = np.random.default_rng(67)
    n = TILE * MAX_BLOCKS + 300
    host = _rows(_wide(rng, n), (rng.random(n) < 0.001).astype(np.float32))
    want = _check(host, 3, 1, 1000, 0.99, "block stride")
    assert want[4] > 1000 and want[3][-1] == -1


@pytest.mark.parametrize("T", [1, 7, 256, 1000, 5000])
def test_terminals_around_a_tile_edge(T):
    rng = np.random.default_rng(T)
    n = 3 * TILE + 37
    r = _wide(rng, n)
    for at in ([255], [256], [257], [255, 256, 257], [100], [0, 1, 2, n - 2, n - 1], []):
        for discount in (1.0, 0.99, 0.0):
            _check(_rows(r, _flags(n, at)), 3, 1, T, discount, (T, at, discount), keep_tail=bool(len(at) & 1))


def test_no_complete_episode():
    host = _rows(_wide(np.random.default_rng(1), 300), _flags(300, []))
    got = _device(host, 3, 1, 1000, 0.99)
    assert got.episodes == 0
    assert torch.all(got.ep_first == -1) and torch.all(got.ep_last == -1)
    assert np.array_equal(_bits(got.ep_return.cpu().numpy()), np.zeros(300, np.int64))
    assert np.array_equal(_bits(got.return_to_go.cpu().numpy()), np.zeros(300, np.int64))
    with pytest.raises(ValueError):
        got.top_fraction_weights(0.5)
    assert all(t.numel() == 0 for t in got.episode_table())
    tail = _device(host, 3, 1, 1000, 0.99, keep_tail=True)
    assert tail.episodes == 1 and torch.all(tail.ep_first == 0) and torch.all(tail.ep_last == 299)


def test_row0_ignores_what_lies_before_it():
    rng = np.random.default_rng(5)
    total, row0, n = 700, 300, 380
    d = _flags(total, [row0 - 1, 310, 600])                             # a terminal just before row0
    host = _rows(_wide(rng, total), d)
    want = rows_episode_returns_ref(host[row0: row0 + n], 3, 1, 90, 0.99, None, True)
    _assert_equal(_device(host, 3, 1, 90, 0.99, keep_tail=True, row0=row0, n=n), want, "row0")
    host[row0 - 1, 2 * 3 + 1 + 1] = 0.0                                 # ... and without it: the same
    _assert_equal(_device(host, 3, 1, 90, 0.99, keep_tail=True, row0=row0, n=n), want, "row0, no terminal before")
    assert want[2][0] == 0 and want[3][0] == 10


def test_state_discontinuity_rule():
    S, A = 17, 6
    rng = np.random.default_rng(17)
    n = 600
    base = _rows(_wide(rng, n), _flags(n, [50, 400]), S, A, continuous=True)
    off = _check(base, S, A, 1000, 0.99, "continuous, rule on", tol=1e-6, keep_tail=True)
    assert off[4] == 3
    host = base.copy()
    host[101, 0] += np.float32(0.5)                                     # first column only: a break at row 100
    host[257, S - 1] += np.float32(0.5)                                 # last column only: a break at row 256
    on = _check(host, S, A, 1000, 0.99, "two jumps", tol=1e-6, keep_tail=True)
    assert on[4] == 5 and on[3][100] == 100 and on[2][101] == 101 and on[3][256] == 256
    _check(host, S, A, 1000, 0.99, "rule off on the same rows", keep_tail=True)
    _check(host, S, A, 1000, 0.99, "tol 0", tol=0.0)
    # ss just above / just below tol^2: two columns differ by 3 and 4 ulps-of-one steps, ss = 25 * 2^-40 exactly
    edge = base.copy()
    for row, col, k in ((300, 3, 3.0), (300, 9, 4.0)):
        edge[row, col] = edge[row - 1, S + A + col] = np.float32(1.0)
        edge[row, col] += np.float32(k * 2.0 ** -20)
    ss = 25.0 * 2.0 ** -40
    tol = float(np.sqrt(ss))
    assert tol * tol == ss
    below, above = float(np.nextafter(tol, 0.0)), float(np.nextafter(tol, 1.0))
    assert below * below < ss < above * above
    for t, is_break in ((tol, False), (above, False), (below, True)):
        want = _check(edge, S, A, 1000, 0.99, ("edge", t), tol=t, keep_tail=True)
        assert (want[3][299] == 299) == is_break, t
    # tol = 0 on continuous rows: no difference at all, no break
    assert _check(base, S, A, 1000, 0.99, "continuous, tol 0", tol=0.0)[4] == 2


def test_sparse_option():
    rng = np.random.default_rng(8)
    n = 700
    r = (rng.random(n) < 0.3).astype(np.float32) - 1.0                  # -1 or 0
    d = (rng.random(n) < 0.03).astype(np.float32)
    host = _rows(r, d)
    want = _check(host, 3, 1, 50, 0.99, "sparse", sparse_value=-1.0, keep_tail=True)
    plain = _check(host, 3, 1, 50, 0.99, "not sparse", keep_tail=True)
    f, l, _, _ = episode_table_ref(*want[:4])
    hit = r[l] == -1.0
    assert hit.any() and (~hit).any()
    assert all(np.all(want[1][a: b + 1] == -1.0 / (1.0 - 0.99)) for a, b in zip(f[hit], l[hit]))
    assert all(np.array_equal(want[1][a: b + 1], plain[1][a: b + 1]) for a, b in zip(f[~hit], l[~hit]))
    import iqlhip_ingest as ing
    with pytest.raises(ValueError):
        ing.episode_returns_device(torch.from_numpy(host).cuda(), 3, 1, n, 50, 1.0, sparse_value=-1.0)


def test_golden_return_to_go():
    z, _ = load_golden("g18_return_to_go")
    n, S, A = len(z["rewards"]), z["s"].shape[1], 2
    host = _rows(z["rewards"], z["terminals"], S, A)
    host[:, :S], host[:, S + A: 2 * S + A] = z["s"], z["ns"]
    got = _device(host, S, A, int(z["T"]), float(z["discount"]), tol=float(z["tol"]), keep_tail=True)
    assert np.array_equal(_bits(got.return_to_go.cpu().numpy()), _bits(z["return_to_go"]))
    _check(host, S, A, int(z["T"]), float(z["discount"]), "g18", tol=float(z["tol"]), keep_tail=True)
    keep = _rows(z["keep_rewards"], z["keep_terminals"], S, A)
    got = _device(keep, S, A, int(z["T"]), float(z["discount"]))
    for frac in (0.1, 0.34, 0.5, 1.0):
        assert np.array_equal(np.flatnonzero(got.top_fraction_weights(frac).cpu().numpy()), z[f"kept_{frac}"]), frac


def test_low_level_outputs_are_optional():
    hb = _hb()
    rng = np.random.default_rng(12)
    n = 900
    host = _rows(_wide(rng, n), (rng.random(n) < 0.02).astype(np.float32))
    want = rows_episode_returns_ref(host, 3, 1, 100, 0.99)
    dev = torch.from_numpy(host).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def call(ret, rtg, first, last, ep):
        ptr = [t.data_ptr() if t is not None else None for t in (ret, rtg, first, last)]
        hb.check(hb.lib().iqlhip_rows_episode_returns(dev.data_ptr(), dev.stride(0), 3, 1, 0, n, 100, 0.99, -1.0, 0, None,
                                                      *ptr, C.byref(ep) if ep is not None else None, stream))
        torch.cuda.synchronize()

    ep = C.c_int64(-1)
    call(None, None, None, None, ep)
    assert ep.value == want[4]
    f64 = lambda: torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    i64 = lambda: torch.full((n,), 7, dtype=torch.int64, device="cuda")
    ret, rtg, first, last = f64(), f64(), i64(), i64()
    call(ret, None, None, None, None)
    assert np.array_equal(_bits(ret.cpu().numpy()), _bits(want[0]))
    call(None, rtg, None, None, None)
    assert np.array_equal(_bits(rtg.cpu().numpy()), _bits(want[1]))
    call(None, None, first, None, None)
    call(None, None, None, last, None)
    assert np.array_equal(first.cpu().numpy(), want[2]) and np.array_equal(last.cpu().numpy(), want[3])
    # a refusal leaves the outputs alone
    ret = f64()
    assert hb.lib().iqlhip_rows_episode_returns(dev.data_ptr(), dev.stride(0), 3, 1, 0, n, 0, 0.99, -1.0, 0, None,
                                                ret.data_ptr(), None, None, None, C.byref(ep), stream) == hb.E_INVAL
    torch.cuda.synchronize()
    assert torch.all(ret == 7.0) and ep.value == want[4]


def test_window_beyond_4_gib():
    """The last 5 000 rows of a 10 M-row buffer of 432-byte rows (obs 39 / act 28): every byte offset is above 2^32."""
    import iql
    hb = _hb()
    S, A, N, n, T = 39, 28, 10_000_000, 5000, 64
    ld = hb.row_stride(S, A)
    buf = iql.ReplayBuffer(S, A, N, "cuda")
    buf.fill_synthetic(N, seed=7, p_done=0.01)
    row0 = N - n
    assert row0 * 4 * ld > 2 ** 32
    host = buf._rows[row0:].cpu().numpy()
    for tol in (None, 1e-6):
        want = rows_episode_returns_ref(host, S, A, T, 0.99, tol, True)
        _assert_equal(_device(buf._rows, S, A, T, 0.99, tol=tol, keep_tail=True, row0=row0, n=n), want, tol)
    assert want[4] > n // T
    assert np.array_equal(buf._rows[row0:].cpu().numpy(), host)


def test_buffer_method_meets_return_reward_range_and_weighted_sampling():
    import iql
    hb = _hb()
    S, A, n, T = 17, 6, 6000, 100
    data = synth.synth_transitions(n, S, A, seed=181, p_done=0.02)
    data["rewards"] = _wide(np.random.default_rng(2), n)
    for cls in (iql.ReplayBuffer, iql.OfflineReplayBuffer):
        buf = cls(S, A, n + 10, "cuda")
        buf.load_d4rl_dataset({k: v.copy() for k, v in data.items()})
        before, writes = buf._rows.cpu().numpy(), buf._writes
        er = buf.episode_returns(T, 0.99)
        assert buf._writes == writes and np.array_equal(buf._rows.cpu().numpy(), before)
        want = rows_episode_returns_ref(before[:n], S, A, T, 0.99)
        _assert_equal(er, want, cls.__name__)
        first, last, ret, g0 = er.episode_table()
        tf, tl, tr, tg = episode_table_ref(*want[:4])
        assert np.array_equal(first.cpu().numpy(), tf) and np.array_equal(last.cpu().numpy(), tl)
        assert np.array_equal(_bits(ret.cpu().numpy()), _bits(tr)) and np.array_equal(_bits(g0.cpu().numpy()), _bits(tg))
        assert (float(ret.min()), float(ret.max())) == buf.return_reward_range(T) and len(tl) == er.episodes
        for by in ("return_to_go", "ep_return"):
            for frac in (0.0, 0.1, 0.5, 1.0):
                w = er.top_fraction_weights(frac, by)
                assert w.dtype == torch.float32 and w.shape == (n,)
                assert np.array_equal(w.cpu().numpy(), top_fraction_weights_ref(*want[:4], frac, by)), (by, frac)
        # top_fraction_weights -> set_sample_weights -> draws: only rows of kept episodes, and every such row drawable
        w = er.top_fraction_weights(0.1)
        kept = w.cpu().numpy() != 0
        assert 0 < kept.sum() < n
        buf.set_sample_weights(w)
        idx = buf.draw_weighted_indices(4096, seed=3, offset=0).cpu().numpy()
        assert kept[idx].all()
        cum = np.empty(n, dtype=np.uint64)
        hb.check(hb.lib().iqlhip_weights_info(buf._weights, None, None, None, None, cum.ctypes.data))
        assert np.array_equal(np.diff(np.concatenate(([0], cum.astype(np.int64)))) != 0, kept)
        buf.set_sample_weights(None)
    empty = iql.ReplayBuffer(S, A, 16, "cuda")
    with pytest.raises(ValueError, match="empty"):
        empty.episode_returns()


def test_call_between_training_calls_changes_nothing():
    """8 steps with episode_returns in their middle end bytewise where 8 steps without it end: the call writes no row,
    leaves the buffer's write count alone (the second call continues on the rows the first staged ahead) and touches no
    trainer state."""
    import iql
    import hip_helpers as hh
    S, A, B = 17, 6, 256
    data = synth.synth_transitions(2048, S, A, seed=41)
    params = synth.synth_params(S, A, seed=6)
    hyper = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    runs = []
    for with_call in (False, True):
        buf = iql.ReplayBuffer(S, A, 2048, "cuda")
        buf.load_d4rl_dataset({k: v.copy() for k, v in data.items()})
        tr = hh.build_hip_trainer(params, S, A, True, hyper, lrs, 1000)
        first = tr.train_steps(buf, 4, B, seed=3)
        writes, token = buf._writes, tr._ts_token
        if with_call:
            er = buf.episode_returns(100, 0.99, state_break_tol=1e-6, keep_tail=True)
            assert er.episodes > 0 and buf._writes == writes
        second = tr.train_steps(buf, 4, B, seed=3)
        assert tr._ts_token == token
        runs.append((first, second, hh.arenas(tr).view(np.uint32).copy(), buf._rows.cpu().numpy()))
    a, b = runs
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
