"""The CPU statement of UPDATABLE weight tables (include/iqlhip.h "updatable tables"), next to
weighted_ref's statement of the static ones — Python integers and numpy uint64, what the device is compared with bit for
bit.

  scale:   e = floor(log2(max(max_weight, max w))), fixed for the table's life;  q = floor(w * 2^(38 - e));
           a weight whose bit pattern is >= that of 2^(e + 1) saturates to 2^39 - 1
  update:  entries (i, w) with a NaN, an infinity, a negative weight (-0.0 is zero) or i outside [0, bound) are skipped and
           flagged (1 non-finite, 2 negative, 4 index); of the valid entries for a row the last position wins
  tree:    levels of 64-entry nodes; a node holds the inclusive prefix sums of its own children's subtree totals
  descent: per level child = #(entries <= t), clamped to the node; t -= the entry before the child
"""
import numpy as np

import weighted_ref as WR
from oracle import philox_ref as P

Q_SATURATED = (1 << 39) - 1
FLAG_NONFINITE, FLAG_NEGATIVE, FLAG_INDEX = 1, 2, 4
MAX_LEVELS = 4


def scale_exponent(w, max_weight=0.0):
    """e of a table built over w with max_weight (0: the largest weight present)."""
    return WR.exponent(np.asarray([max(float(np.max(w)), float(np.float32(max_weight)))], dtype=np.float32))


def quantise_at(w, e):
    """q of float32 weights (finite, >= 0) at the fixed scale e, with saturation: uint64 array."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    m, E = WR._parts(w)
    s = E + (38 - e)
    left = np.left_shift(m.astype(np.uint64), np.clip(s, 0, 39).astype(np.uint64))
    right = np.right_shift(m.astype(np.uint64), np.clip(-s, 0, 63).astype(np.uint64))
    q = np.where(s >= 0, left, right).astype(np.uint64)
    if e + 1 <= 127:
        bits = w.view(np.uint32).astype(np.int64) & 0x7FFFFFFF
        sat_bits = int(np.float32(2.0 ** (e + 1)).view(np.uint32)) if e + 1 >= -149 else 0
        q = np.where(bits >= sat_bits, np.uint64(Q_SATURATED), q)
    return q


def level_sizes(n):
    """Entries of every level over n rows, bottom first, up to the level of <= 64 entries."""
    sizes = [int(n)]
    while sizes[-1] > 64:
        sizes.append((sizes[-1] + 63) // 64)
    assert len(sizes) <= MAX_LEVELS
    return sizes


def build_tree(q):
    """The node-local tree over the leaf values q: a list of levels, each a list of Python ints (entry c of node k at
    index 64 k + c).  The last level is one node; its last entry is the total."""
    levels = []
    vals = [int(x) for x in q]
    while True:
        lvl, totals = [], []
        for k in range(0, len(vals), 64):
            run = 0
            for v in vals[k:k + 64]:
                run += v
                lvl.append(run)
            totals.append(run)
        levels.append(lvl)
        if len(lvl) <= 64:
            return levels
        vals = totals


def build_tree_np(q):
    """build_tree with numpy (large n): a list of uint64 arrays."""
    levels = []
    vals = np.asarray(q, dtype=np.uint64)
    while True:
        n = vals.shape[0]
        pad = np.zeros((n + 63) // 64 * 64, dtype=np.uint64)
        pad[:n] = vals
        pre = np.cumsum(pad.reshape(-1, 64), axis=1, dtype=np.uint64)
        levels.append(pre.reshape(-1)[:n].copy())
        if n <= 64:
            return levels
        vals = pre[:, 63].copy()


def descend(levels, t):
    """The local-layout descent for one t (Python int): the leaf index."""
    node = 0
    for lvl in reversed(levels):
        first = 64 * node
        width = min(64, len(lvl) - first)
        seps = [int(x) for x in lvl[first:first + width]]
        child = min(sum(1 for s in seps if s <= t), width - 1)
        if child:
            t -= seps[child - 1]
        node = first + child
    return node


def descend_r(levels, r):
    """... for 64 random bits r: t = mulhi64(r, total)."""
    total = int(levels[-1][-1])
    return descend(levels, (int(r) * total) >> 64)


class Table:
    """An updatable table on the CPU: q (uint64 [capacity]), the fixed scale e, the sticky flags and the version."""

    def __init__(self, w, capacity=None, max_weight=0.0):
        w = np.ascontiguousarray(w, dtype=np.float32)
        WR.check(w)
        n = w.shape[0]
        self.n = n if capacity is None else int(capacity)
        assert n <= self.n <= 1 << 24
        self.e = scale_exponent(w, max_weight)
        self.q = np.zeros(self.n, dtype=np.uint64)
        self.q[:n] = quantise_at(w, self.e)
        self.flags = 0
        self.version = 0

    def update(self, idx, w, bound=None):
        """Apply one update call; the semantics of iqlhip_weights_update."""
        idx = np.asarray(idx, dtype=np.int64)
        w = np.ascontiguousarray(w, dtype=np.float32)
        assert idx.shape == w.shape and idx.ndim == 1
        bound = self.n if bound is None else int(bound)
        bits = w.view(np.uint32)
        nonfinite = (bits & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
        negative = ~nonfinite & ((bits >> np.uint32(31)) != 0) & ((bits << np.uint32(1)) != 0)
        bad_index = (idx < 0) | (idx >= bound)
        if nonfinite.any():
            self.flags |= FLAG_NONFINITE
        if negative.any():
            self.flags |= FLAG_NEGATIVE
        if bad_index.any():
            self.flags |= FLAG_INDEX
        ok = ~(nonfinite | negative | bad_index)
        if ok.any():
            q_new = quantise_at(np.abs(w[ok]), self.e)          # (-0.0 is zero)
            for i, qv in zip(idx[ok], q_new):                   # in order: the last position wins
                self.q[i] = qv
        self.version += 1

    @property
    def total(self):
        return int(np.sum(self.q.astype(object))) if self.n < 4096 else int(np.cumsum(self.q, dtype=np.uint64)[-1])

    def tree(self):
        return build_tree_np(self.q)

    def draw_indices(self, n, seed, offset, j0=0):
        """Weighted indices of the stream (seed, offset) by the global-cum search (what the descent must equal)."""
        cum = np.cumsum(self.q, dtype=np.uint64)
        t = P.mulhi64(WR.random_bits(n, seed, offset, j0), int(cum[-1]))
        return np.minimum(np.searchsorted(cum, t, side="right"), self.n - 1).astype(np.int64)
