"""GPU tests of the reward ingest (iqlhip_rows_return_range / _reward_scale / _reward_shift, ReplayBuffer.return_reward_range
/ modify_reward_): return_reward_range / modify_reward of algorithms/finetune/iql.py:262-289 on packed device rows.  Every
comparison is bit-exact against the CPU restatement tests/reward_ref.py, and for the fixture cases against the
reference's recorded results (tests/golden/g17_reward_range.npz) as well.  S = 17, A = 6: the row stride carries padding.
Every case runs on rows [0, n) and on rows [5, 5 + n) of a store whose other cells hold a sentinel pattern that must
survive."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth
from helpers import load_golden
from reward_ref import episode_returns_ref, modify_reward_ref, return_reward_range_ref

pytestmark = pytest.mark.gpu

S, A = 17, 6
RCOL, DCOL = 2 * S + A, 2 * S + A + 1
TILE = 256                      # rows per scan tile (RR_TILE, csrc/iqlhip_kernels.h)
MAX_BLOCKS = 4096               # blocks per launch (RR_MAX_BLOCKS): more tiles than that are walked with a block stride


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _wide(rng, n):
    """float32 rewards of mixed sign over 1e-6 .. 1e6: the order of a float64 sum shows in its last bits."""
    return (rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-6.0, 6.0, size=n)).astype(np.float32)


def _store(r, d, row0):
    """A packed row store of row0 + n + 3 rows: sentinel values everywhere (padding included), r and d in their columns
    of rows [row0, row0 + n).  Returns (device tensor, host copy)."""
    import iqlhip_binding as hb
    n, ld = len(r), hb.row_stride(S, A)
    assert ld > DCOL + 1
    host = np.random.default_rng(n + row0).standard_normal((row0 + n + 3, ld)).astype(np.float32)
    host[row0: row0 + n, RCOL] = r
    host[row0: row0 + n, DCOL] = d
    return torch.from_numpy(host).cuda(), host


def _return_range(rows, row0, n, T):
    import iqlhip_binding as hb
    out, ep = (C.c_double * 2)(), C.c_int64(-1)
    hb.check(hb.lib().iqlhip_rows_return_range(rows.data_ptr(), rows.stride(0), S, A, row0, n, T, out, C.byref(ep), _stream()))
    return out[0], out[1], ep.value


def _check(r, d, T, want_range=None):
    """Rows [row0, row0 + n) for row0 in (0, 5): the range, the episode count, the rescaled and the shifted reward
    column, and every other cell untouched."""
    import iqlhip_binding as hb
    r, d = np.asarray(r, np.float32), np.asarray(d, np.float32)
    n = len(r)
    returns = episode_returns_ref(r, d, T)
    for row0 in (0, 5):
        rows, host = _store(r, d, row0)
        if not returns:
            with pytest.raises(ValueError, match="no complete episode"):
                _return_range(rows, row0, n, T)
            assert np.array_equal(rows.cpu().numpy(), host)
            continue
        mn, mx, episodes = _return_range(rows, row0, n, T)
        assert (mn, mx) == (min(returns), max(returns)) and episodes == len(returns), (row0, n, T)
        if want_range is not None:
            assert (mn, mx) == want_range
        assert np.array_equal(rows.cpu().numpy(), host)                              # the scan writes no row
        if mx != mn:
            want, _ = modify_reward_ref(r, d, "hopper", T)
            hb.check(hb.lib().iqlhip_rows_reward_scale(rows.data_ptr(), rows.stride(0), S, A, row0, n, mx - mn, float(T), _stream()))
            got = rows.cpu().numpy()
            assert np.array_equal(got[row0: row0 + n, RCOL], want), (row0, n, T)
            got[row0: row0 + n, RCOL] = r
            assert np.array_equal(got, host)                                         # no other cell, no sentinel row
            rows.copy_(torch.from_numpy(host))
        hb.check(hb.lib().iqlhip_rows_reward_shift(rows.data_ptr(), rows.stride(0), S, A, row0, n, 1.0, _stream()))
        got = rows.cpu().numpy()
        assert np.array_equal(got[row0: row0 + n, RCOL], modify_reward_ref(r, d, "antmaze", T)[0])
        got[row0: row0 + n, RCOL] = r
        assert np.array_equal(got, host)


def _flags(n, at):
    d = np.zeros(n, np.float32)
    d[list(at)] = 1.0
    return d


_RNG = np.random.default_rng(17)
BOUNDARY = {
    "one_row_no_terminal": (_wide(_RNG, 1), _flags(1, []), 1000),                    # ValueError
    "one_row_terminal": (_wide(_RNG, 1), _flags(1, [0]), 1000),
    "T1_every_row": (_wide(_RNG, 300), _flags(300, [4, 5, 299]), 1),
    "T_above_n_no_terminal": (_wide(_RNG, 40), _flags(40, []), 41),                  # ValueError
    "n_equals_T": (_wide(_RNG, 40), _flags(40, []), 40),
    "timeouts_only_3T_plus_2": (_wide(_RNG, 3 * 90 + 2), _flags(3 * 90 + 2, []), 90),
    "terminal_first_last_consecutive": (_wide(_RNG, 200), _flags(200, [0, 70, 71, 72, 199]), 1000),
    "terminal_on_timeout_row": (_wide(_RNG, 100), _flags(100, [9, 19, 25]), 10),     # rows 9, 19: both at once; 25: restart
    "T7_across_tiles": (_wide(_RNG, 2 * TILE + 11), _flags(2 * TILE + 11, [3, 255, 300]), 7),
}
N_CARRY = 3 * TILE + 37
CARRY = {
    "only_terminal_in_tile_0": (_wide(_RNG, N_CARRY), _flags(N_CARRY, [100]), 7),
    "only_terminal_in_tile_0_long_T": (_wide(_RNG, N_CARRY), _flags(N_CARRY, [100]), 301),
    "terminals_on_both_sides_of_a_tile_edge": (_wide(_RNG, N_CARRY), _flags(N_CARRY, [2 * TILE - 1, 2 * TILE]), 300),
    "terminal_on_last_row_of_ragged_tail": (_wide(_RNG, N_CARRY), _flags(N_CARRY, [TILE, N_CARRY - 1]), 1000),
    "no_terminal": (_wide(_RNG, N_CARRY), _flags(N_CARRY, []), 64),
}


@pytest.mark.parametrize("name", list(BOUNDARY))
def test_episode_boundaries(name):
    _check(*BOUNDARY[name])


@pytest.mark.parametrize("name", list(CARRY))
def test_previous_terminal_carries_across_scan_tiles(name):
    _check(*CARRY[name])


def test_golden_cases():
    z, meta = load_golden("g17_reward_range")
    ranged = 0
    for name in meta["cases"]:
        r, d, T, env = z[name + "_rewards"], z[name + "_terminals"], int(z[name + "_T"]), str(z[name + "_env_name"])
        want = modify_reward_ref(r, d, env, T)[0]
        assert np.array_equal(want, z[name + "_modified"])
        if np.isnan(z[name + "_min_ret"]):
            _check(r, d, T)
        else:
            ranged += 1
            _check(r, d, T, want_range=(float(z[name + "_min_ret"]), float(z[name + "_max_ret"])))
    assert ranged >= 4


def _loaded(data, extra=10):
    import iql
    buf = iql.ReplayBuffer(S, A, len(data["rewards"]) + extra, "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in data.items()})
    return buf


@pytest.mark.parametrize("env", ["hopper-medium-v2", "walker2d-expert-v2", "halfcheetah-random-v2", "antmaze-umaze-v2",
                                 "pen-human-v1"])
def test_modify_reward_on_the_buffer(env):
    z, _ = load_golden("g17_reward_range")
    case = {"hopper-medium-v2": "wide_hopper", "walker2d-expert-v2": "timeouts_only", "halfcheetah-random-v2": "wide_short_T7",
            "antmaze-umaze-v2": "antmaze", "pen-human-v1": "other_env"}[env]
    n, T = len(z[case + "_rewards"]), int(z[case + "_T"])
    data = synth.synth_transitions(n, S, A, seed=171)
    data["rewards"], data["terminals"] = z[case + "_rewards"].copy(), z[case + "_terminals"].copy()
    buf = _loaded(data)
    before, writes = buf._rows.cpu().numpy(), buf._writes
    want, want_info = modify_reward_ref(data["rewards"], data["terminals"], env, T)
    if want_info:
        assert buf.return_reward_range(T) == (want_info["min_ret"], want_info["max_ret"])
        assert buf._writes == writes and np.array_equal(buf._rows.cpu().numpy(), before)
    info = buf.modify_reward_(env, T)
    assert info == want_info and all(type(v) is type(want_info[k]) for k, v in info.items())
    after = buf._rows.cpu().numpy()
    assert np.array_equal(after[:n, RCOL], want)
    if want_info or "antmaze" in env:
        assert np.array_equal(want, z[case + "_modified"]) and buf._writes > writes
        if want_info:
            assert (info["min_ret"], info["max_ret"]) == (float(z[case + "_min_ret"]), float(z[case + "_max_ret"]))
    else:
        assert buf._writes == writes
    after[:n, RCOL] = before[:n, RCOL]
    assert np.array_equal(after, before)                      # states, actions, next states, dones, padding, free rows
    # the dict feeds the reference's modify_reward_online unchanged
    import iql
    online = iql.modify_reward_online(1.5, env, **info)
    if want_info:
        assert online == 1.5 / (info["max_ret"] - info["min_ret"]) * T
    else:
        assert online == (0.5 if "antmaze" in env else 1.5)


def test_empty_buffer_and_default_steps():
    import iql
    buf = iql.ReplayBuffer(S, A, 16, "cuda")
    for env in ("hopper-medium-v2", "antmaze-umaze-v2"):
        with pytest.raises(ValueError, match="empty"):
            buf.modify_reward_(env)
    with pytest.raises(ValueError, match="empty"):
        buf.return_reward_range(1000)
    assert buf.modify_reward_("door-human-v1") == {} and buf._writes == 0
    data = synth.synth_transitions(12, S, A, seed=3, p_done=0.0)
    off = iql.OfflineReplayBuffer(S, A, 16, "cuda")
    off.load_d4rl_dataset(data)
    with pytest.raises(ValueError, match="no complete episode"):       # 12 rows, no terminal, max_episode_steps = 1000
        off.modify_reward_("hopper-medium-v2")
    assert np.array_equal(off._rows.cpu().numpy()[:12, RCOL], data["rewards"])
    data["terminals"][7] = 1.0
    off = iql.OfflineReplayBuffer(S, A, 16, "cuda")
    off.load_d4rl_dataset(data)
    one = return_reward_range_ref(data["rewards"], data["terminals"], 1000)
    assert one[0] == one[1]
    with pytest.raises(ValueError, match="divide_by"):                 # one episode: max_ret == min_ret
        off.modify_reward_("hopper-medium-v2")
    assert np.array_equal(off._rows.cpu().numpy()[:12, RCOL], data["rewards"])


def test_train_steps_sees_the_modified_rewards():
    from hip_helpers import build_hip_trainer
    n, T, B, K = 3000, 100, 256, 2
    data = synth.synth_transitions(n, S, A, seed=172)
    params = synth.synth_params(S, A, seed=173)
    hyper = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    dev_buf = _loaded(data)
    tr_dev = build_hip_trainer(params, S, A, True, hyper, lrs, 1000)
    raw = tr_dev.train_steps(dev_buf, K, B, seed=5)              # (also: a call on the unmodified rows came first)
    info = dev_buf.modify_reward_("hopper-medium-v2", T)
    host = {k: v.copy() for k, v in data.items()}
    host["rewards"], want_info = modify_reward_ref(data["rewards"], data["terminals"], "hopper-medium-v2", T)
    assert info == want_info
    host_buf = _loaded(host)
    assert torch.equal(dev_buf._rows, host_buf._rows)
    a = build_hip_trainer(params, S, A, True, hyper, lrs, 1000).train_steps(dev_buf, K, B, seed=5)
    b = build_hip_trainer(params, S, A, True, hyper, lrs, 1000).train_steps(host_buf, K, B, seed=5)
    assert np.array_equal(a, b) and not np.array_equal(a, raw)
    # the trainer that stepped on the old rewards continues on the new ones (the buffer's write count has moved)
    c = tr_dev.train_steps(dev_buf, K, B, seed=5)
    tr_host = build_hip_trainer(params, S, A, True, hyper, lrs, 1000)
    tr_host.train_steps(_loaded(data), K, B, seed=5)
    assert np.array_equal(c, tr_host.train_steps(host_buf, K, B, seed=5))


def test_more_tiles_than_blocks():
    """n above RR_MAX_BLOCKS tiles: every block walks more than one tile (block stride), a ragged last tile."""
    import iql
    n = TILE * MAX_BLOCKS + 300
    buf = iql.ReplayBuffer(S, A, n, "cuda")
    buf.fill_synthetic(n, seed=4, p_done=0.001)
    before = buf._rows[:, RCOL: DCOL + 1].cpu().numpy()
    r, d = before[:, 0].copy(), before[:, 1].copy()
    want, want_info = modify_reward_ref(r, d, "walker2d-medium-v2", 1000)
    assert buf.return_reward_range(1000) == (want_info["min_ret"], want_info["max_ret"])
    assert buf.modify_reward_("walker2d-medium-v2") == want_info
    after = buf._rows[:, RCOL: DCOL + 1].cpu().numpy()
    assert np.array_equal(after[:, 0], want) and np.array_equal(after[:, 1], d)


def test_window_across_the_4_gib_line():
    """About 20 000 rows straddling byte 2^32 of a 10 M-row buffer of 432-byte rows (obs 39 / act 28, the shape of
    tests/test_hip_bigbuffer.py): 64-bit row offsets in the scan, the episode sums and the reward map."""
    import iql
    import iqlhip_binding as hb
    S2, A2, N, T = 39, 28, 10_000_000, 64
    ld = hb.row_stride(S2, A2)
    rcol = 2 * S2 + A2
    buf = iql.ReplayBuffer(S2, A2, N, "cuda")
    assert N * 4 * ld > 2 ** 32
    buf.fill_synthetic(N, seed=7, p_done=0.01)
    mid = 2 ** 32 // (4 * ld)
    row0, n = mid - 10_000, 20_001
    assert row0 * 4 * ld < 2 ** 32 < (row0 + n) * 4 * ld
    lo, hi = row0 - 2, row0 + n + 2
    before = buf._rows[lo:hi].cpu().numpy()
    r, d = before[2:-2, rcol].copy(), before[2:-2, rcol + 1].copy()
    returns = episode_returns_ref(r, d, T)
    assert len(returns) > n // T and (d != 0).sum() > 50
    out, ep = (C.c_double * 2)(), C.c_int64(0)
    hb.check(hb.lib().iqlhip_rows_return_range(buf._rows.data_ptr(), ld, S2, A2, row0, n, T, out, C.byref(ep), _stream()))
    assert (out[0], out[1], ep.value) == (min(returns), max(returns), len(returns))
    scaled = modify_reward_ref(r, d, "hopper", T)[0]
    hb.check(hb.lib().iqlhip_rows_reward_scale(buf._rows.data_ptr(), ld, S2, A2, row0, n, out[1] - out[0], float(T), _stream()))
    after = buf._rows[lo:hi].cpu().numpy()
    assert np.array_equal(after[2:-2, rcol], scaled)
    hb.check(hb.lib().iqlhip_rows_reward_shift(buf._rows.data_ptr(), ld, S2, A2, row0, n, 1.0, _stream()))
    shifted = buf._rows[lo:hi].cpu().numpy()
    assert np.array_equal(shifted[2:-2, rcol], scaled - np.float32(1.0))
    for got in (after, shifted):                              # nothing but the window's reward column has changed
        got[2:-2, rcol] = r
        assert np.array_equal(got, before)


def test_bad_arguments_leave_the_rewards_alone():
    import iqlhip_binding as hb
    lib = hb.lib()
    rng = np.random.default_rng(5)
    n = 50
    rows, host = _store(_wide(rng, n), _flags(n, [20, 49]), 5)
    ld = rows.stride(0)
    out, ep = (C.c_double * 2)(7.0, 7.0), C.c_int64(-3)
    good = dict(rows=rows.data_ptr(), ld=ld, row0=5, n=n, T=10)
    for bad in ({"rows": None}, {"n": 0}, {"row0": -1}, {"T": 0}, {"ld": hb.row_stride(S, A) - 1}):
        a = dict(good, **bad)
        assert lib.iqlhip_rows_return_range(a["rows"], a["ld"], S, A, a["row0"], a["n"], a["T"], out, C.byref(ep), _stream()) == hb.E_INVAL, bad
        assert hb.last_error()
        if "T" not in bad:
            assert lib.iqlhip_rows_reward_scale(a["rows"], a["ld"], S, A, a["row0"], a["n"], 2.0, 3.0, _stream()) == hb.E_INVAL, bad
            assert lib.iqlhip_rows_reward_shift(a["rows"], a["ld"], S, A, a["row0"], a["n"], 1.0, _stream()) == hb.E_INVAL, bad
    assert lib.iqlhip_rows_return_range(rows.data_ptr(), ld, S, A, 5, n, 10, None, C.byref(ep), _stream()) == hb.E_INVAL
    assert lib.iqlhip_rows_return_range(rows.data_ptr(), ld, S, A, 5, n, 10, out, None, _stream()) == hb.E_INVAL
    assert lib.iqlhip_rows_reward_scale(rows.data_ptr(), ld, S, A, 5, n, 0.0, 3.0, _stream()) == hb.E_INVAL
    assert (out[0], out[1], ep.value) == (7.0, 7.0, -3)
    torch.cuda.synchronize()
    assert np.array_equal(rows.cpu().numpy(), host)
    want = episode_returns_ref(host[5: 5 + n, RCOL], host[5: 5 + n, DCOL], 10)          # ... and a good call still works
    assert _return_range(rows, 5, n, 10) == (min(want), max(want), len(want)) and len(want) == 6
