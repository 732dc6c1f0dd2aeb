"""The CPU statement of TRACKING weight tables (include/iqlhip.h "tracking tables", DESIGN.md 6j "Online prioritised
replay") over weighted_update_ref.Table — Python integers and numpy uint64, what the device is compared with bit for bit.

  q_max:   one integer at the table's fixed scale; max(max_i q[i], q(new_row_weight)) after the build (new_row_weight
           saturates like any weight)
  update:  every entry that is APPLIED — valid, and the last position among its row's valid entries — raises q_max to
           max(q_max, q_new); an entry that lost to a later duplicate or was skipped raises nothing; q_max never falls
  insert:  q[row] = q_max, row in [0, bound), bound <= n; the version grows by 1
"""
import numpy as np

import weighted_update_ref as U


def w_of_q(q, e):
    """The weight a table integer stands for at scale e, as the library reports it: float32(q * 2^(e - 38))."""
    return float(np.float32(np.ldexp(float(int(q)), e - 38)))


class TrackingTable(U.Table):
    """weighted_update_ref.Table plus the maximum word."""

    def __init__(self, w, capacity=None, max_weight=0.0, new_row_weight=1.0):
        super().__init__(w, capacity, max_weight)
        nrw = np.float32(new_row_weight)
        assert np.isfinite(nrw) and nrw > 0
        q_new = int(U.quantise_at(np.array([nrw], dtype=np.float32), self.e)[0])
        self.q_max = max(int(self.q.max()), q_new)

    def update(self, idx, w, bound=None):
        """iqlhip_weights_update on a tracking table: Table.update, and the applied entries raise q_max."""
        idx = np.asarray(idx, dtype=np.int64)
        w = np.ascontiguousarray(w, dtype=np.float32)
        limit = self.n if bound is None else int(bound)
        bits = w.view(np.uint32)
        nonfinite = (bits & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
        negative = ~nonfinite & ((bits >> np.uint32(31)) != 0) & ((bits << np.uint32(1)) != 0)
        ok = ~(nonfinite | negative | (idx < 0) | (idx >= limit))
        winner = {}
        for j in np.nonzero(ok)[0]:          # in order: the last valid position of a row wins
            winner[int(idx[j])] = int(j)
        super().update(idx, w, bound)
        for i in winner:                     # (the row now holds its winner's q_new)
            self.q_max = max(self.q_max, int(self.q[i]))

    def insert_max(self, row, bound=None):
        limit = self.n if bound is None else int(bound)
        assert 0 <= limit <= self.n and 0 <= int(row) < limit
        self.q[int(row)] = np.uint64(self.q_max)
        self.version += 1

    @property
    def w_max(self):
        return w_of_q(self.q_max, self.e)
