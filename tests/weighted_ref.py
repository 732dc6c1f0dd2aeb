"""The CPU statement of weighted replay sampling (include/iqlhip.h "weighted replay sampling"), in Python
integers and numpy uint64 — what the device table and the device draw are compared with, bit for bit.

  e = floor(log2(max w));  q[i] = floor(w[i] * 2^(38 - e));  cum = cumsum(q);  total = cum[-1]
  index j: r = the 64 random bits of the index stream (oracle.philox_ref);  t = mulhi64(r, total);
           the smallest i with cum[i] > t
"""
import numpy as np

from oracle import philox_ref as P


def _parts(w):
    """float32 array -> (significand m, exponent E) with value = m * 2^E exactly (int64 arrays)."""
    b = np.ascontiguousarray(w, dtype=np.float32).view(np.uint32).astype(np.int64) & 0x7FFFFFFF
    ex = b >> 23
    frac = b & 0x7FFFFF
    m = np.where(ex > 0, frac | 0x800000, frac)
    E = np.where(ex > 0, ex - 150, -149)
    return m, E


def check(w):
    """ValueError for what the library refuses."""
    w = np.asarray(w)
    if w.dtype != np.float32 or w.ndim != 1 or not 1 <= w.shape[0] <= 1 << 24:
        raise ValueError("weights: a float32 vector of 1 .. 2^24 entries")
    if not np.all(np.isfinite(w)) or np.any(w < 0) or not np.any(w > 0):
        raise ValueError("weights: finite, >= 0, at least one > 0")


def exponent(w):
    """e = floor(log2(max w)) from the bit pattern (denormals included)."""
    m, E = _parts(np.asarray([np.max(w)], dtype=np.float32))
    return int(E[0]) + int(m[0]).bit_length() - 1


def quantise(w):
    """q[i] = floor(w[i] * 2^(38 - e)) as uint64: integer shifts of the significand, no floating-point operation."""
    check(w)
    sh0 = 38 - exponent(w)
    m, E = _parts(w)
    s = E + sh0
    left = np.left_shift(m.astype(np.uint64), np.clip(s, 0, 39).astype(np.uint64))
    right = np.right_shift(m.astype(np.uint64), np.clip(-s, 0, 63).astype(np.uint64))
    return np.where(s >= 0, left, right).astype(np.uint64)


def table(w):
    """(cum uint64 [n], total int)."""
    cum = np.cumsum(quantise(w), dtype=np.uint64)
    return cum, int(cum[-1])


def random_bits(n, seed, offset, j0=0):
    """The 64 random bits of indices j0 .. j0 + n - 1 of the stream (seed, offset): what philox_ref.draw_indices maps."""
    j = np.uint64(int(j0)) + np.arange(int(n), dtype=np.uint64)
    ctr = P.index_counters(offset, j)
    k0, k1 = P._key(seed)
    o0, o1, o2, o3 = P.philox4x32_10(ctr & np.uint64(0xFFFFFFFF), ctr >> np.uint64(32), P.TAG_INDEX, 0, k0, k1)
    odd = (j & np.uint64(1)).astype(bool)
    return np.where(odd, (o3 << np.uint64(32)) | o2, (o1 << np.uint64(32)) | o0)


def draw_indices(n, w, seed, offset, j0=0):
    """Weighted indices j0 .. j0 + n - 1 of the stream (seed, offset): int64 [n]."""
    cum, total = table(w)
    t = P.mulhi64(random_bits(n, seed, offset, j0), total)
    return np.searchsorted(cum, t, side="right").astype(np.int64)       # the smallest i with cum[i] > t
