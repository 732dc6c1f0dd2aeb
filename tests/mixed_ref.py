"""CPU reference of the index draw of a train_steps_mixed call, built on oracle.philox_ref.draw_indices.

A call's index stream does not know about the two buffers: index j = k * B + r of the call (step k, batch row r) is 64
random bits of counter offset + j / 2.  Only the mapping does: rows r < n_off map the bits over the offline size, rows
r >= n_off over the online size.  So the whole call is drawn twice, once per size, and each batch row takes its column
from the draw of its own buffer."""
import numpy as np

from oracle import philox_ref as R


def mixed_indices(n_steps, B, n_off, size_off, size_on, seed, offset):
    """(idx_off int64 [n_steps, n_off], idx_on int64 [n_steps, B - n_off]) of one call."""
    n_steps, B, n_off = int(n_steps), int(B), int(n_off)
    assert 1 <= n_off <= B - 1
    over_off = R.draw_indices(n_steps * B, size_off, seed, offset).reshape(n_steps, B)
    over_on = R.draw_indices(n_steps * B, size_on, seed, offset).reshape(n_steps, B)
    return np.ascontiguousarray(over_off[:, :n_off]), np.ascontiguousarray(over_on[:, n_off:])


def call_offset(total_it, B):
    """The counter the Python shim starts a call on (train_steps and train_steps_mixed alike)."""
    return int(total_it) * ((int(B) + 1) // 2)
