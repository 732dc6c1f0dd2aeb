"""CPU reference of the fifth device random stream: the keep-bits of actor dropout inside policy inference
(iqlhip_set_act_dropout; DESIGN.md "Random streams").  Built from oracle/philox_ref.py's generator and threshold.

  inference keep-bits of act-dropout call n   counter (w, j | "ADRP", lo32 n, hi32 n), j = 0..7,
                                              w = row * 16 + layer * 8 + q; bit 4 j + t of the word = (o_t >= thresh)

The key is (lo32 seed, hi32 seed); rows restart at 0 with every library call; bit b of word q = hidden unit 32 q + b.
"""
from __future__ import annotations

import numpy as np

from oracle.philox_ref import dropout_threshold, philox4x32_10

TAG_ACT_DROP = 0x41445250      # "ADRP"
_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF


def act_keep_counters(n, rows):
    """The counter words (c0, c1, c2, c3) of call n on `rows` rows: uint64 arrays that broadcast to
    [2 layers][rows][8 words][8 blocks]."""
    n = int(n) & _M64
    layer = np.arange(2, dtype=np.uint64)[:, None, None, None]
    row = np.arange(int(rows), dtype=np.uint64)[None, :, None, None]
    q = np.arange(8, dtype=np.uint64)[None, None, :, None]
    blk = np.arange(8, dtype=np.uint64)[None, None, None, :]
    w = row * np.uint64(16) + layer * np.uint64(8) + q
    return w, blk | np.uint64(TAG_ACT_DROP), np.uint64(n & _M32), np.uint64(n >> 32)


def act_keep_words(seed, n, p, rows):
    """Keep-bit words of act-dropout call n: uint32 [2 layers][rows][8]."""
    seed = int(seed) & _M64
    thresh = np.uint64(dropout_threshold(p))
    c0, c1, c2, c3 = act_keep_counters(n, rows)
    o = philox4x32_10(c0, c1, c2, c3, seed & _M32, seed >> 32)
    blk = np.arange(8, dtype=np.uint64)[None, None, None, :]
    word = np.zeros((2, int(rows), 8), dtype=np.uint64)
    for t in range(4):
        keep = (o[t] >= thresh).astype(np.uint64)                  # [2][rows][8][block]
        word |= (keep << (np.uint64(4) * blk + np.uint64(t))).sum(axis=3, dtype=np.uint64)   # (disjoint bits)
    return word.astype(np.uint32)


def keep_scale(p):
    """The keep scale of the training step: 1.f / (1.f - p) in float32."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))
