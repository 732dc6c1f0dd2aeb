"""Plain numpy restatement of the n-step rows (include/iqlhip.h "n-step rows"), written from the header's
statement of the arithmetic, not from the kernel: `build` (iqlhip_rows_nstep), `ring_refresh` (iqlhip_rows_nstep_ring)
and, from the definition of an n-step return alone and sharing no code with the two, `brute_force_target`.

Packed rows [s | a | s' | r | d | pad], float32.  Python floats are IEEE doubles and Python never fuses a product into a
sum, so `r + discount * G` below rounds the product, then the sum, as the header demands."""
import numpy as np


def _derive(rows_at, i, limit, stop_at, discount):
    """Row i of a chain that may run to `limit`: (m, (float32)G, float32 done value).  rows_at(j) -> (r, d) of logical
    row j as float32 scalars; stop_at(j): the chain may not pass row j."""
    m = limit
    for j in range(i, limit + 1):
        if rows_at(j)[1] != 0 or stop_at(j):
            m = j
            break
    G = float(rows_at(m)[0])
    for j in range(m - 1, i - 1, -1):
        p = float(discount) * G
        G = float(rows_at(j)[0]) + p
    d_m = rows_at(m)[1]
    if d_m != 0:
        d_out = np.float32(d_m)
    else:
        c = 1.0
        for _ in range(m - i):
            c = c * float(discount)
        d_out = np.float32(1.0 - c)
    return m, np.float32(G), d_out


def build(rows, S, A, N, discount, ep_last=None):
    """(derived rows, steps uint8 [n]) of the n rows given, in storage order; ep_last: int64 [n] or None."""
    rows = np.asarray(rows, dtype=np.float32)
    n = rows.shape[0]
    rcol, dcol = 2 * S + A, 2 * S + A + 1
    out = rows.copy()
    steps = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        end = n - 1
        if ep_last is not None and ep_last[i] >= 0:
            end = min(max(int(ep_last[i]), i), n - 1)
        limit = min(i + N - 1, end)
        m, G, d_out = _derive(lambda j: (rows[j, rcol], rows[j, dcol]), i, limit, lambda j: False, discount)
        out[i, S + A: rcol] = rows[m, S + A: rcol]
        out[i, rcol], out[i, dcol] = G, d_out
        steps[i] = m - i + 1
    return out, steps


def ring_refresh(raw, derived, ends, capacity, size, newest, N, discount, S, A, steps=None):
    """What one iqlhip_rows_nstep_ring call does, in place on `derived` (and `steps`, indexed by position): the
    min(N, size) derived rows that end at position `newest` are recomputed from the raw ring and its end bytes.
    (S, A: a packed row's width alone does not say where its columns are.)"""
    rcol, dcol = 2 * S + A, 2 * S + A + 1
    base = (newest - (size - 1)) % capacity

    def pos(j):
        return (base + j) % capacity

    for i in range(size - min(N, size), size):
        limit = min(i + N - 1, size - 1)
        m, G, d_out = _derive(lambda j: (raw[pos(j), rcol], raw[pos(j), dcol]), i, limit, lambda j: ends[pos(j)] != 0,
                              discount)
        p = pos(i)
        derived[p] = raw[p]
        derived[p, S + A: rcol] = raw[pos(m), S + A: rcol]
        derived[p, rcol], derived[p, dcol] = G, d_out
        if steps is not None:
            steps[p] = m - i + 1


def unroll(capacity, size, newest):
    """Positions of a ring's rows in time order, oldest first."""
    return [(newest - (size - 1) + j) % capacity for j in range(size)]


def ep_last_from_ends(ends_in_order):
    """ep_last of rows in time order from their end flags: the first flagged row at or behind each row, -1 if none."""
    n = len(ends_in_order)
    out = np.full(n, -1, dtype=np.int64)
    nxt = -1
    for i in range(n - 1, -1, -1):
        if ends_in_order[i]:
            nxt = i
        out[i] = nxt
    return out


def brute_force_target(rows, S, A, N, discount, value_of_next, ep_last=None):
    """float64 [n]: sum_{t < k} discount^t r_{i+t} + discount^k (1 - d_{i+k-1}) V(s'_{i+k-1}), straight from the
    definition, k being the number of rows the return of row i may span.  value_of_next: float64 [n], V of every row's
    OWN s' (the raw rows')."""
    rows = np.asarray(rows, dtype=np.float64)
    v = np.asarray(value_of_next, dtype=np.float64)
    n = rows.shape[0]
    r, d = rows[:, 2 * S + A], rows[:, 2 * S + A + 1]
    out = np.zeros(n, dtype=np.float64)
    for i in range(n):
        last_allowed = n - 1 if ep_last is None or ep_last[i] < 0 else int(ep_last[i])
        k = 0
        total = 0.0
        while True:
            total += discount ** k * r[i + k]
            k += 1
            if d[i + k - 1] != 0 or k == N or i + k - 1 >= last_allowed:
                break
        out[i] = total + discount ** k * (1.0 - d[i + k - 1]) * v[i + k - 1]
    return out
