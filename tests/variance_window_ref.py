"""Numpy restatement of the variance learner's replay-buffer windows (DESIGN.md 6l "From a replay buffer"), written from
include/iqlhip.h, not from the kernel: the packed block of B consecutive packed rows, and the start rows a burst draws
(oracle/philox_ref.py's index stream, counter offset 0, index offset + k for update k)."""
import numpy as np

from oracle import philox_ref as P


def row_stride(S, A):
    """iqlhip_row_stride: 2 S + A + 2 floats rounded up to 16 bytes."""
    return (2 * S + A + 2 + 3) // 4 * 4


def pack_window(rows, start, B, S, A):
    """rows: float32 [n][ld] packed [s | a | s' | r | d | pad].  The block of the window at `start`:
    [B][S] states | [S] last next-state | [B] rewards | [B] next-dones, float32 [B S + S + 2 B]."""
    rows = np.asarray(rows)
    if not 0 <= start <= rows.shape[0] - B:
        raise ValueError("the window leaves the buffer")
    w = rows[start:start + B]
    return np.concatenate([w[:, :S].reshape(-1), w[B - 1, S + A:2 * S + A], w[:, 2 * S + A], w[:, 2 * S + A + 1]]).astype(np.float32)


def window_tensors(rows, start, B, S, A):
    """The window as the host arguments of pack_block / _update_v: (observations, actions, rewards, dones,
    next_observations, next_dones)."""
    w = np.asarray(rows)[start:start + B]
    return (w[:, :S].copy(), [None] * B, w[:, 2 * S + A].copy(), [False] * B, w[:, S + A:2 * S + A].copy(),
            w[:, 2 * S + A + 1].copy())


def burst_starts(n, size, B, seed, offset=0, starts=None):
    """Start rows of updates 0 .. n - 1 of a burst: int64 [n]."""
    span = (size - B + 1) if starts is None else len(starts)
    i = P.draw_indices(n, span, seed, 0, j0=offset)
    return i if starts is None else np.asarray(starts, dtype=np.int64)[i]


def synthetic_rows(n, S, A, seed, ld=None, p_done=0.05):
    """float32 [n][ld] packed rows: normal states, uniform rewards, 0 / 1 dones, NaN in the pad columns (nothing may
    read them)."""
    ld = row_stride(S, A) if ld is None else ld
    r = np.random.RandomState(seed)
    rows = np.full((n, ld), np.nan, dtype=np.float32)
    rows[:, :2 * S + A] = r.standard_normal((n, 2 * S + A)).astype(np.float32)
    rows[:, 2 * S + A] = r.uniform(-1, 1, size=n).astype(np.float32)
    rows[:, 2 * S + A + 1] = (r.uniform(size=n) < p_done).astype(np.float32)
    return rows
