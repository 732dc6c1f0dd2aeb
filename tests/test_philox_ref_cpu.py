"""CPU tests of oracle/philox_ref.py, the reference tests/test_hip_rng_streams.py holds the library's four device random
streams to: Random123's known answers of Philox4x32-10, the vectorised forms against plain Python integers, the
streams' own statistics at 2^20 draws (so that the GPU tests compare against a formula that is itself right), and the
host arithmetic by which the shim advances a train_steps call's counter offset."""
import weakref

import numpy as np
import pytest
import torch

from oracle import philox_ref as R

N = 1 << 20
SD = 5.0          # every statistical bound below is 5 standard deviations of the statistic under the null hypothesis


# ---------------------------------------------------------------------------------------------------- the generator
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert R.philox4x32_10_scalar(*ctr, *key) == want
    got = R.philox4x32_10(*[np.array([c], dtype=np.uint64) for c in ctr], *key)
    assert tuple(int(g[0]) for g in got) == want


def test_vectorised_philox_equals_scalar():
    rng = np.random.default_rng(1)
    c = rng.integers(0, 1 << 32, size=(4, 300), dtype=np.uint64)
    c[:, 0] = 0
    c[:, 1] = 0xFFFFFFFF
    for k0, k1 in ((0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0x00000001, 0xDEADBEEF)):
        got = R.philox4x32_10(c[0], c[1], c[2], c[3], k0, k1)
        assert all(g.dtype == np.uint64 for g in got)
        for i in range(c.shape[1]):
            want = R.philox4x32_10_scalar(*(int(x) for x in c[:, i]), k0, k1)
            assert tuple(int(g[i]) for g in got) == want, i
    # scalar counter words broadcast against array ones
    got = R.philox4x32_10(c[0], 7, R.TAG_INDEX, 0, 5, 6)
    assert tuple(int(g[3]) for g in got) == R.philox4x32_10_scalar(int(c[0, 3]), 7, R.TAG_INDEX, 0, 5, 6)


@pytest.mark.parametrize("size", [1, 2, 1000, 10 ** 7, 2 ** 40 + 12345])
def test_multiply_high_equals_python_integers(size):
    rng = np.random.default_rng(size % 1000)
    r = rng.integers(0, 1 << 64, size=2000, dtype=np.uint64)
    r[:6] = [0, 1, (1 << 64) - 1, (1 << 63), (1 << 32) - 1, (1 << 32)]
    got = R.mulhi64(r, size)
    want = [(int(x) * size) >> 64 for x in r]
    assert [int(g) for g in got] == want
    assert int(got.max()) < size


def test_index_counters_wrap_and_pair_words():
    """ctr = offset + j // 2 modulo 2^64, even j reads words (o1, o0), odd j words (o3, o2)."""
    seed, size = 0xDEADBEEF00000001, 2 ** 40 + 12345
    for offset in (0, 7, 2 ** 32 - 3, 2 ** 63 + 5, 2 ** 64 - 2):
        got = R.draw_indices(9, size, seed, offset)
        for j in range(9):
            ctr = (offset + j // 2) % (1 << 64)
            o = R.philox4x32_10_scalar(ctr & 0xFFFFFFFF, ctr >> 32, 0x49514C48, 0, seed & 0xFFFFFFFF, seed >> 32)
            r = (o[3] << 32 | o[2]) if j & 1 else (o[1] << 32 | o[0])
            assert int(got[j]) == (r * size) >> 64, (offset, j)
        assert np.array_equal(R.draw_indices(4, size, seed, offset, j0=3), got[3:7])


# ---------------------------------------------------------------------------------------------------- the streams
def test_reference_indices_are_uniform():
    size = 1000
    idx = R.draw_indices(N, size, 123, 0)
    assert idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < size
    c = np.bincount(idx, minlength=size).astype(np.float64)
    chi2 = float(((c - N / size) ** 2 / (N / size)).sum())
    print(f"index chi2 {chi2:.1f} (999 dof)")
    assert abs(chi2 - 999) <= SD * np.sqrt(2 * 999), chi2
    # the two word pairs are not the same numbers: adjacent indices (one counter) are uncorrelated
    x = idx.astype(np.float64) - (size - 1) / 2
    rho = float(np.mean(x[0::2] * x[1::2]) / np.mean(x * x))
    assert abs(rho) <= SD / np.sqrt(N / 2), rho


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_reference_keep_rate(p):
    rows, max_batch = 256, 256
    bits = []
    for step in range(N // (2 * rows * 256)):                    # 8 steps of 131072 bits
        w = R.dropout_keep_words(0x123456789, step, p, max_batch, rows)
        assert w.dtype == np.uint32 and w.shape == (2, rows, 8)
        bits.append(np.unpackbits(w.view(np.uint8)))
    bits = np.concatenate(bits)
    assert bits.size == N
    pf = float(np.float32(p))
    rate = bits.mean()
    print(f"p={p}: keep rate {rate:.6f}")
    assert abs(rate - (1 - pf)) <= SD * np.sqrt(pf * (1 - pf) / N), rate
    k0, k1 = R.keep_masks(w)
    assert k0.shape == (rows, 256) and bool(k1[3, 32 * 5 + 7]) == bool((int(w[1, 3, 5]) >> 7) & 1)


def test_dropout_threshold_and_word_layout():
    assert R.dropout_threshold(0.5) == 1 << 31
    assert R.dropout_threshold(0.0) == 0
    assert R.dropout_threshold(0.1) == int(float(np.float32(0.1)) * 2.0 ** 32)
    assert R.dropout_threshold(np.nextafter(np.float32(1), np.float32(0))) == 0xFFFFFF00
    # a smaller call of the same context reads the first rows of the same words; the layer-1 words move with max_batch
    a = R.dropout_keep_words(9, 2 ** 32 + 1, 0.3, 256, 256)
    b = R.dropout_keep_words(9, 2 ** 32 + 1, 0.3, 256, 100)
    c = R.dropout_keep_words(9, 2 ** 32 + 1, 0.3, 512, 100)
    assert np.array_equal(a[:, :100], b) and np.array_equal(c[0], b[0]) and not np.array_equal(c[1], b[1])
    assert not np.array_equal(a, R.dropout_keep_words(9, 1, 0.3, 256, 256))          # the step's high word counts
    # one word by hand
    seed, step, layer, row, q = 0xAB00000009, 2 ** 32 + 1, 1, 77, 3
    w = layer * 256 * 8 + row * 8 + q
    word = 0
    for j in range(8):
        o = R.philox4x32_10_scalar(w, j | 0x44524F50, step & 0xFFFFFFFF, step >> 32, seed & 0xFFFFFFFF, seed >> 32)
        for t in range(4):
            word |= int(o[t] >= R.dropout_threshold(0.3)) << (4 * j + t)
    assert int(R.dropout_keep_words(seed, step, 0.3, 256, 100)[layer, row, q]) == word


def _assert_standard_normal(z, what):
    n = z.size
    m1, m2, m3, m4 = (float(np.mean(z ** k)) for k in (1, 2, 3, 4))
    print(f"{what}: mean {m1:.5f} var {m2:.5f} third {m3:.5f} fourth {m4:.5f} max|z| {np.abs(z).max():.3f}")
    # variances of the raw sample moments of N(0,1): 1, 2, 15, 96 (over n)
    assert abs(m1) <= SD * np.sqrt(1 / n), (what, m1)
    assert abs(m2 - 1) <= SD * np.sqrt(2 / n), (what, m2)
    assert abs(m3) <= SD * np.sqrt(15 / n), (what, m3)
    assert abs(m4 - 3) <= SD * np.sqrt(96 / n), (what, m4)
    assert np.abs(z).max() <= 5.9            # sqrt(-2 ln 2^-25) = 5.887: the clamp-free bound the act() test relies on


def test_reference_act_noise_is_standard_normal():
    z = R.act_noise(0x9E3779B97F4A7C15, 3, N // 32, 32)
    assert z.shape == (N // 32, 32) and z.dtype == np.float64
    _assert_standard_normal(z.ravel(), "act noise")
    # another call number, or its high word, is another stream; e restarts with every call
    assert not np.array_equal(z[:4], R.act_noise(0x9E3779B97F4A7C15, 4, 4, 32))
    assert not np.array_equal(z[:4], R.act_noise(0x9E3779B97F4A7C15, 3 + 2 ** 32, 4, 32))
    assert np.array_equal(z[:4], R.act_noise(0x9E3779B97F4A7C15, 3, 4, 32))


def test_unit_interval_rounding():
    """u = (float32(o >> 8) + 0.5f) * 2^-24 in float32: exact below 2^23, rounded to even from there, 1.0 at the top."""
    o = np.array([0, 0xFF, 0x100, (1 << 31) - 1, 1 << 31, (1 << 31) + 0x100, 0xFFFFFFFF], dtype=np.uint64)
    u = R._unit24(o)
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0 ** -25) and u[1] == u[0] and u[2] == np.float32(1.5 * 2.0 ** -24)
    assert u[3] == np.float32((2 ** 23 - 0.5) * 2.0 ** -24)       # 2^23 - 1 + 0.5: still exact
    assert u[4] == np.float32(0.5) and u[5] == np.float32((2 ** 23 + 2) * 2.0 ** -24)     # ties to even
    assert u[6] == np.float32(1.0) and u.min() > 0


def test_reference_fill_distributions():
    S, A = 17, 6
    W = 2 * S + A + 2
    n = N // W + 1
    for antmaze, p_done in ((False, 0.01), (True, 0.25)):
        v, exact = R.fill_rows(77, 0, n, S, A, p_done, antmaze)
        assert v.shape == (n, W) and exact.sum() == A + 1 + int(antmaze)
        _assert_standard_normal(np.concatenate([v[:, :S].ravel(), v[:, S + A: 2 * S + A].ravel()]), "fill states")
        a = v[:, S: S + A]
        assert np.abs(a).max() <= float(np.float32(0.999)) and np.array_equal(a, a.astype(np.float32))
        assert abs(a.mean()) <= SD * 0.999 / np.sqrt(3 * a.size)
        assert abs(np.mean(a * a) - 0.999 ** 2 / 3) <= SD * 0.999 ** 2 * np.sqrt(4 / 45 / a.size)
        d = v[:, 2 * S + A + 1]
        pf = float(np.float32(p_done))
        assert set(np.unique(d)) <= {0.0, 1.0} and abs(d.mean() - pf) <= SD * np.sqrt(pf * (1 - pf) / n), d.mean()
        r = v[:, 2 * S + A]
        if antmaze:
            assert set(np.unique(r)) <= {-1.0, 0.0} and abs(-r.mean() - 0.98) <= SD * np.sqrt(0.98 * 0.02 / n), r.mean()
        else:
            assert abs(r.mean()) <= SD / np.sqrt(n) and abs(np.mean(r * r) - 1) <= SD * np.sqrt(2 / n)
    # rows are addressed by their absolute number; p_done = 0 and 1 are never / always
    part, _ = R.fill_rows(77, 300, 50, S, A, 0.25, True)
    assert np.array_equal(part, v[300:350])
    assert R.fill_rows(5, 0, 200, 3, 9, 0.0, False)[0][:, -1].max() == 0.0
    assert R.fill_rows(5, 0, 200, 3, 9, 1.0, False)[0][:, -1].min() == 1.0


# ---------------------------------------------------------------------------------------------------- host arithmetic
class _RecordingLib:
    """Stands in for the library under ImplicitQLearning.train_steps: records (n_steps, seed, stream_offset)."""

    def __init__(self):
        self.calls = []

    def iqlhip_train_steps(self, ctx, rows, ld, size, B, tab, k, seed, offset, flags, stream):
        self.calls.append((int(k), int(seed), int(offset)))
        return 0


class _Rows:
    _ld, _writes = 44, 0

    def __init__(self):
        self._rows = torch.zeros(4, 44)


@pytest.mark.parametrize("B", [1, 33, 255])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_consecutive_train_steps_calls_never_share_counters(B, n, monkeypatch):
    """The shim passes stream_offset = total_it * ceil(B / 2): a call of n steps draws n * B indices from
    ceil(n * B / 2) counters, which must end before the next call's offset — for odd batches too, where a step's
    indices start in the middle of a counter."""
    import iqlhip_binding as hb
    import iqlhip_trainer as T
    rec = _RecordingLib()
    monkeypatch.setattr(hb, "lib", lambda: rec)
    tr = object.__new__(T.ImplicitQLearning)
    tr._ctx, tr._dp_world, tr._dp_rank, tr._ts_token, tr.total_it = None, 1, 0, None, 0
    tr._train_steps_args = lambda buf, b: (5000, 1.0 / b)
    tr._scalar_table = lambda k, inv: np.zeros((k, 16), dtype=np.float32)
    tr._lookahead_table = lambda k, inv: None
    tr._stream = lambda: 0
    buf = _Rows()
    assert weakref.ref(buf)() is buf
    for _ in range(4):
        tr.train_steps(buf, n, B, seed=3, return_losses=False)
    tr.train_steps(buf, 2 * n + 1, B, seed=3, return_losses=False, chunk=n)         # split into calls of n, n, 1
    assert [c[0] for c in rec.calls] == [n] * 6 + [1] and tr.total_it == 6 * n + 1
    half, t, end_prev = (B + 1) // 2, 0, 0
    for k, seed, offset in rec.calls:
        assert seed == 3 and offset == t * half
        first, end = R.call_counter_range(offset, k * B)
        assert first >= end_prev, (rec.calls, "a counter is drawn from twice")
        assert end - first == (k * B + 1) // 2
        t, end_prev = t + k, end
