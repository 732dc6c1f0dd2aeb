"""CPU reference of the four device random streams (numpy only; nothing of the library is imported).

Written from the stream contract of DESIGN.md "random streams" / include/iqlhip.h, not from the kernels:

  index draw        counter (lo32 ctr, hi32 ctr, "IQLH", 0),    ctr = offset + j // 2
  dropout keep-bits counter (word, block | "DROP", lo32 step, hi32 step)
  act() noise       counter (element, lo32 call, hi32 call, 0xAC7)
  synthetic fill    counter (lo32 ctr, hi32 ctr, "FILL", 0),    ctr = row * W + column

The key is always (lo32 seed, hi32 seed); the generator is Philox4x32-10 (Salmon et al., SC'11).  tests/
test_philox_ref_cpu.py pins this file to Random123's known answers and to its own statistics; tests/
test_hip_rng_streams.py holds every drawing site of the library to it.
"""
from __future__ import annotations

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57      # round multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85      # key increments (golden ratio, sqrt(3) - 1)
TAG_INDEX, TAG_DROP, TAG_FILL, TAG_ACT = 0x49514C48, 0x44524F50, 0x46494C4C, 0xAC7
_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------------------------------------- the generator
def philox4x32_10_scalar(c0, c1, c2, c3, k0, k1):
    """Pure-Python Philox4x32-10 on ints: (o0, o1, o2, o3)."""
    c0, c1, c2, c3, k0, k1 = (int(x) & _M32 for x in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0 = PHILOX_M0 * c0
        p1 = PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + PHILOX_W0) & _M32
        k1 = (k1 + PHILOX_W1) & _M32
    return c0, c1, c2, c3


def _u64(x):
    """Anything holding 32-bit values (Python ints included) -> a uint64 array."""
    if isinstance(x, (int, np.integer)):
        return np.asarray(int(x) & _M32, dtype=np.uint64)
    return np.asarray(x).astype(np.uint64) & np.uint64(_M32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10: uint64 arrays holding 32-bit values in (broadcast against each other), four such
    arrays out.  A product of two 32-bit values fits a uint64, so no step overflows."""
    c0, c1, c2, c3 = np.broadcast_arrays(_u64(c0), _u64(c1), _u64(c2), _u64(c3))
    k0, k1 = _u64(k0), _u64(k1)
    m32, s32 = np.uint64(_M32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0 = (k0 + np.uint64(PHILOX_W0)) & m32
        k1 = (k1 + np.uint64(PHILOX_W1)) & m32
    return c0, c1, c2, c3


def _key(seed):
    seed = int(seed) & _M64
    return seed & _M32, seed >> 32


def mulhi64(r, size):
    """floor(r * size / 2^64) for a uint64 array r and 0 <= size < 2^64, from 32-bit halves (no 128-bit type)."""
    r = np.asarray(r, dtype=np.uint64)
    size = int(size)
    if not 0 <= size <= _M64:
        raise ValueError("size outside [0, 2^64)")
    m32, s32 = np.uint64(_M32), np.uint64(32)
    rl, rh = r & m32, r >> s32
    sl, sh = np.uint64(size & _M32), np.uint64(size >> 32)
    ll, lh, hl, hh = rl * sl, rl * sh, rh * sl, rh * sh
    mid = (ll >> s32) + (lh & m32) + (hl & m32)          # < 3 * 2^32
    return hh + (lh >> s32) + (hl >> s32) + (mid >> s32)


# ---------------------------------------------------------------------------------------------------- index draw
def index_counters(offset, j):
    """64-bit counters offset + j // 2 (modulo 2^64) of the indices j (array) of one call."""
    j = np.asarray(j, dtype=np.uint64)
    return np.uint64(int(offset) & _M64) + (j >> np.uint64(1))       # uint64 array arithmetic wraps


def draw_indices(n, size, seed, offset, j0=0):
    """Indices j0 .. j0 + n - 1 of a call that draws from [0, size) under (seed, offset): int64 [n]."""
    j = np.uint64(int(j0)) + np.arange(int(n), dtype=np.uint64)
    ctr = index_counters(offset, j)
    k0, k1 = _key(seed)
    o0, o1, o2, o3 = philox4x32_10(ctr & np.uint64(_M32), ctr >> np.uint64(32), TAG_INDEX, 0, k0, k1)
    odd = (j & np.uint64(1)).astype(bool)
    r = np.where(odd, (o3 << np.uint64(32)) | o2, (o1 << np.uint64(32)) | o0)
    return mulhi64(r, size).astype(np.int64)


def call_counter_range(offset, n_indices):
    """[first, last + 1) of the counters a call drawing n_indices indices from `offset` consumes (Python ints, not
    reduced modulo 2^64)."""
    return int(offset), int(offset) + (int(n_indices) + 1) // 2


# ---------------------------------------------------------------------------------------------------- dropout
def dropout_threshold(p):
    """Keep iff word >= thresh: thresh = min(floor(double(float32(p)) * 2^32), 2^32 - 1)."""
    return min(int(float(np.float32(p)) * 4294967296.0), _M32)


def dropout_keep_words(seed, step, p, max_batch, rows):
    """Keep-bit words of step `step`: uint32 [2 layers][rows][8]; bit b of word q of a row = hidden unit 32 q + b.
    Word number w = layer * max_batch * 8 + row * 8 + q (the layer-1 words depend on the context's max_batch)."""
    step = int(step) & _M64
    k0, k1 = _key(seed)
    thresh = np.uint64(dropout_threshold(p))
    layer = np.arange(2, dtype=np.uint64)[:, None, None, None]
    row = np.arange(int(rows), dtype=np.uint64)[None, :, None, None]
    q = np.arange(8, dtype=np.uint64)[None, None, :, None]
    blk = np.arange(8, dtype=np.uint64)[None, None, None, :]
    w = layer * np.uint64(int(max_batch) * 8) + row * np.uint64(8) + q
    o = philox4x32_10(w, blk | np.uint64(TAG_DROP), step & _M32, step >> 32, k0, k1)
    word = np.zeros(np.broadcast_shapes(w.shape, blk.shape)[:3], dtype=np.uint64)
    for t in range(4):
        keep = (o[t] >= thresh).astype(np.uint64)                  # [2][rows][8][block]
        word |= (keep << (np.uint64(4) * blk + np.uint64(t))).sum(axis=3, dtype=np.uint64)   # (disjoint bits)
    return word.astype(np.uint32)


def keep_masks(words):
    """uint32 [2][rows][8] -> two bool arrays [rows][256] (unit 32 q + b = bit b of word q)."""
    b = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")
    m = b.reshape(2, words.shape[1], 256).astype(bool)
    return m[0], m[1]


# ---------------------------------------------------------------------------------------------------- normals
def _unit24(o):
    """(float32(o >> 8) + 0.5f) * 2^-24, every step in float32: the sum rounds (to even) once o >> 8 >= 2^23, so the
    result lies in (0, 1] — 1.0 itself included."""
    f = (o >> np.uint64(8)).astype(np.float32)
    return (f + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def box_muller(u1, u2):
    """z = sqrt(-2 ln u1) * cos(float32(float32(2 pi) * u2)): the argument of cos rounded to float32 like the device's,
    the functions themselves in float64."""
    arg = (np.float32(6.283185307179586) * u2.astype(np.float32)).astype(np.float32)
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(arg.astype(np.float64))


def act_noise(seed, call, rows, A):
    """N(0,1) noise of ONE library call (call number `call`) on `rows` states: float64 [rows][A]; element
    e = row * A + d restarts at 0 with every call."""
    call = int(call) & _M64
    k0, k1 = _key(seed)
    e = np.arange(int(rows) * int(A), dtype=np.uint64)
    o0, o1, _, _ = philox4x32_10(e, call & _M32, call >> 32, TAG_ACT, k0, k1)
    return box_muller(_unit24(o0), _unit24(o1)).reshape(int(rows), int(A))


# ---------------------------------------------------------------------------------------------------- synthetic fill
def fill_rows(seed, row0, n, S, A, p_done, antmaze):
    """Rows row0 .. row0 + n - 1 of the synthetic fill, columns [s | a | s' | r | d] (W = 2 S + A + 2, no padding).
    Returns (values float64 [n][W], exact bool [W]): exact columns (actions, dones, antmaze rewards) are float32
    values the device must reproduce bit for bit, the others are normals (box_muller)."""
    S, A, n = int(S), int(A), int(n)
    W = 2 * S + A + 2
    k0, k1 = _key(seed)
    i = np.arange(n, dtype=np.uint64)[:, None]
    c = np.arange(W, dtype=np.uint64)[None, :]
    ctr = (np.uint64(int(row0)) + i) * np.uint64(W) + c
    o0, o1, _, _ = philox4x32_10(ctr & np.uint64(_M32), ctr >> np.uint64(32), TAG_FILL, 0, k0, k1)
    u1, u2 = _unit24(o0), _unit24(o1)
    out = box_muller(u1, u2)
    exact = np.zeros(W, dtype=bool)
    a = slice(S, S + A)
    out[:, a] = ((np.float32(2.0) * u1[:, a] - np.float32(1.0)) * np.float32(0.999)).astype(np.float64)
    exact[a] = True
    r, d = 2 * S + A, 2 * S + A + 1
    if antmaze:
        out[:, r] = np.where(u1[:, r] < np.float32(0.98), -1.0, 0.0)
        exact[r] = True
    out[:, d] = np.where(u1[:, d] < np.float32(p_done), 1.0, 0.0)
    exact[d] = True
    return out, exact
