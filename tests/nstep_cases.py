"""Inputs the n-step tests share (tests/test_nstep_cpu.py, tests/test_hip_nstep.py): packed rows cut into episodes of
1, 2, N - 1, N and N + 1 rows, and the transitions of a ring sequence with random done / episode_end flags."""
import numpy as np


def row_stride(S, A):
    return (2 * S + A + 2 + 3) // 4 * 4


def episode_lengths(N):
    return [L for L in (1, 2, N - 1, N, N + 1) if L >= 1]


def packed_rows(rng, n, S, A, N, first_done=False, last_done=False):
    """float32 [n, ld] rows (pad columns random too: they must be copied) with rewards in [-1, 1]; episodes of the
    lengths above in random order, each ended by done = 1 with probability 1/2 (else it just runs into the next one: a
    time limit only ep_last can see, marked by a state jump); s[i + 1] == s'[i] inside an episode."""
    ld = row_stride(S, A)
    rows = rng.uniform(-1.0, 1.0, size=(n, ld)).astype(np.float32)
    dcol = 2 * S + A + 1
    rows[:, dcol] = 0.0
    lengths = episode_lengths(N)
    i = 0
    ends = np.zeros(n, dtype=bool)
    while i < n:
        L = lengths[rng.integers(len(lengths))]
        last = min(i + L, n) - 1
        rows[i + 1: last + 1, :S] = rows[i: last, S + A: 2 * S + A]
        if i + L <= n:
            ends[last] = True
            if rng.random() < 0.5:
                rows[last, dcol] = 1.0
        i += L
    if first_done:
        rows[0, dcol] = 1.0
    if last_done:
        rows[n - 1, dcol] = 1.0
    return rows, ends


def ring_transitions(rng, adds, S, A, N):
    """`adds` transitions (state, action, reward, next_state, done, episode_end) in episodes of the lengths above: the
    last row of an episode has episode_end = True and done at random; one episode in four also carries a done that is no
    episode end (done = True, episode_end = False)."""
    lengths = episode_lengths(N)
    out = []
    while len(out) < adds:
        L = lengths[rng.integers(len(lengths))]
        for t in range(L):
            last = t == L - 1
            done = bool(last and rng.random() < 0.5)
            end = last
            if not last and rng.random() < 0.05:
                done, end = True, False
            out.append((rng.standard_normal(S).astype(np.float32), rng.uniform(-1, 1, A).astype(np.float32),
                        float(np.float32(rng.uniform(-1, 1))), rng.standard_normal(S).astype(np.float32), done, end))
    return out[:adds]


def pack(S, A, ld, t):
    row = np.zeros(ld, dtype=np.float32)
    row[:S], row[S: S + A], row[S + A: 2 * S + A] = t[0], t[1], t[3]
    row[2 * S + A], row[2 * S + A + 1] = np.float32(t[2]), np.float32(t[4])
    return row
