"""The eager twins of the five train_steps kinds (not a test module): K eager steps on the rows a burst call draws at the
trainer's current total_it, each built from the public eager calls and a CPU or device reference of the draw.  None of
them uses a graph, rows staged ahead or a continuation, so each is independent of everything a burst keeps between steps.
Shared by the kinds' own test modules (which pin one shape) and tests/test_hip_chunk_kind_shapes.py (which runs them over
a table of shapes): every function takes its dimensions from the buffers and trainers it is given.

The plain kind's twin is hip_helpers.eager_segment."""
import numpy as np
import torch

import mixed_ref
import weighted_ref


def losses_of(log):
    return np.array([log["value_loss"], log["q_loss"], log["actor_loss"]], dtype=np.float32)


def _stats_of(log):
    return [v for name, v in log.items() if name.startswith("stats/")]


# ---------------------------------------------------------------- mixed: two buffers, the CPU Philox reference
def gather_into(buf, idx, block):
    """Rows idx of buf -> block (packed rows) through iqlhip_rows_gather_packed_h."""
    import iqlhip_binding as hb
    n = idx.shape[0]
    host = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).pin_memory()
    scratch = torch.empty(n, dtype=torch.int64, device="cuda")
    hb.check(hb.lib().iqlhip_rows_gather_packed_h(buf._rows.data_ptr(), buf._ld, buf._buffer_size, host.data_ptr(),
                                                  scratch.data_ptr(), n, block.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream))
    torch.cuda.current_stream().synchronize()        # (host / scratch are free again)


def eager_mixed_segment(tr, off, on, K, B, n_off, seed, with_stats=False):
    """K eager train() steps on the batches train_steps_mixed draws at the trainer's current total_it."""
    S, A = off._state_dim, off._action_dim
    idx_off, idx_on = mixed_ref.mixed_indices(K, B, n_off, off._size, on._size, seed, mixed_ref.call_offset(tr.total_it, B))
    ld = off._ld
    losses, stats = np.empty((K, 3), dtype=np.float32), []
    for k in range(K):
        block = torch.empty((B, ld), dtype=torch.float32, device="cuda")
        gather_into(off, idx_off[k], block[:n_off])
        gather_into(on, idx_on[k], block[n_off:])
        log = tr.train([block[:, :S], block[:, S: S + A], block[:, 2 * S + A: 2 * S + A + 1], block[:, S + A: 2 * S + A],
                        block[:, 2 * S + A + 1: 2 * S + A + 2]])
        losses[k] = losses_of(log)
        stats.append(_stats_of(log))
    return (losses, np.array(stats, dtype=np.float32)) if with_stats else losses


def mixing_ratio(B, n_off):
    """A ratio train_steps_mixed turns into exactly n_off offline rows of B."""
    r = (n_off + 0.5) / B
    assert int(B * r) == n_off
    return r


# ---------------------------------------------------------------- weighted: the integer reference of the draw
def skewed_weights(n, of=5000, seed=8):
    """The first n of `of` log-normal weights, a tenth of them zero (tests/test_hip_weighted.py draws over all 5 000)."""
    rng = np.random.RandomState(seed)
    w = np.exp(2.0 * rng.randn(of)).astype(np.float32)
    w[rng.rand(of) < 0.1] = 0.0
    w = np.ascontiguousarray(w[:n])
    w.setflags(write=False)
    return w


def eager_weighted_segment(tr, buf, w, K, B, seed, with_stats=False):
    """K eager train() steps on the rows train_steps_weighted(buf, K, B, seed) draws at the trainer's total_it."""
    idx = weighted_ref.draw_indices(K * B, w, seed, tr.total_it * ((B + 1) // 2))
    losses, stats = np.empty((K, 3), dtype=np.float32), []
    for k in range(K):
        log = tr.train(buf.gather(torch.from_numpy(idx[k * B:(k + 1) * B])))
        losses[k] = losses_of(log)
        stats.append(_stats_of(log))
    return (losses, np.array(stats, dtype=np.float32)) if with_stats else losses


# ---------------------------------------------------------------- weighted with importance-sampling weights
def fourth_power_weights(n, seed=2):
    """rand ** 4 + 1e-3 with every seventh weight zero: the table of the is_beta and prioritised burst tests."""
    w = np.random.RandomState(seed).rand(n).astype(np.float32) ** 4 + np.float32(1e-3)
    w[::7] = 0.0
    return w


def eager_is_segment(tr, buf, K, B, seed, beta):
    """K eager iterations on the rows train_steps_weighted(buf, K, B, seed, is_beta=beta) draws at the trainer's current
    total_it: draw with is_beta -> gather -> train(batch, loss_weights=c); losses float32 [K, 3]."""
    idx, c = buf.draw_weighted_indices(K * B, seed, tr.total_it * ((B + 1) // 2), is_beta=beta, batch_size=B)
    out = np.empty((K, 3), dtype=np.float32)
    for k in range(K):
        out[k] = losses_of(tr.train(buf.gather(idx[k * B:(k + 1) * B]), loss_weights=c[k * B:(k + 1) * B]))
    return out


# ---------------------------------------------------------------- prioritised: the eager lag-1 loop
def eager_prioritized_segment(tr, buf, K, B, seed, alpha, eps, beta, lag=True):
    """K iterations of the eager loop on the rows train_steps_prioritized(buf, K, B, seed) draws at the trainer's current
    total_it (B even: step t's indices are a draw of their own at offset + t B / 2).  lag=False: the update of step t
    comes BEFORE the draw of step t + 1 — the order the burst does not have."""
    assert B % 2 == 0
    off0 = tr.total_it * (B // 2)

    def draw(t):
        return buf.draw_weighted_indices(B, seed, off0 + t * (B // 2), is_beta=beta)
    out = np.empty((K, 3), dtype=np.float32)
    idx, c = draw(0)
    for t in range(K):
        nxt = draw(t + 1) if lag else None
        out[t] = losses_of(tr.train(buf.gather(idx), loss_weights=c, return_td=True))
        buf.update_sample_weights_td(idx, tr.last_td_errors(), alpha, eps)
        idx, c = nxt if lag else draw(t + 1)
    return out


def table_of(buf):
    """(leaves, total) of the buffer's weight table."""
    import iqlhip_weighted as wtd
    total, _, _, q = wtd.table_state(buf._weights, buf.sample_weights_n, leaves=True)
    return q, total
