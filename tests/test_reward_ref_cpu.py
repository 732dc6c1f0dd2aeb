"""CPU-only tests of the reward ingest (iqlhip_rows_return_range / _reward_scale / _reward_shift,
ReplayBuffer.return_reward_range / modify_reward_): the numpy restatement tests/reward_ref.py reproduces the reference's
recorded results (tests/golden/g17_reward_range.npz) bit for bit, the new symbols are declared, exported and bound, their
argument checks answer without a GPU, and a CPU buffer refuses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import iql
import iqlhip_binding as hb
from helpers import load_golden
from reward_ref import episode_returns_ref, modify_reward_ref, return_reward_range_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"iqlhip_rows_return_range": 10, "iqlhip_rows_reward_scale": 9, "iqlhip_rows_reward_shift": 8}


def golden_cases():
    z, meta = load_golden("g17_reward_range")
    for name in meta["cases"]:
        yield name, {k: z[f"{name}_{k}"] for k in ("rewards", "terminals", "modified", "T", "env_name", "min_ret", "max_ret")}


def test_restatement_reproduces_the_reference_fixture_bit_for_bit():
    seen_range = seen_shift = seen_other = 0
    for name, c in golden_cases():
        T, env = int(c["T"]), str(c["env_name"])
        assert c["rewards"].dtype == np.float32 and c["modified"].dtype == np.float32
        got, info = modify_reward_ref(c["rewards"], c["terminals"], env, T)
        assert got.dtype == np.float32 and np.array_equal(got, c["modified"]), name
        if np.isnan(c["min_ret"]):
            assert info == {}, name
            if "antmaze" in env:
                seen_shift += 1
                assert np.array_equal(c["modified"], c["rewards"] - np.float32(1.0))
            else:
                seen_other += 1
                assert np.array_equal(c["modified"], c["rewards"])
        else:
            seen_range += 1
            assert info == {"min_ret": float(c["min_ret"]), "max_ret": float(c["max_ret"]), "max_episode_steps": T}, name
            assert return_reward_range_ref(c["rewards"], c["terminals"], T) == (float(c["min_ret"]), float(c["max_ret"]))
    assert seen_range >= 4 and seen_shift >= 1 and seen_other >= 1


def test_fixture_pins_the_order_of_the_sums():
    """In the wide-magnitude cases a stored extreme return changes when its episode is summed backwards: a sum in any
    other order than row after row does not reproduce the fixture."""
    _, c = next(x for x in golden_cases() if x[0] == "wide_hopper")
    r, d, T = c["rewards"], c["terminals"], int(c["T"])
    fwd = episode_returns_ref(r, d, T)
    # the episodes of the reversed columns that lie between two terminals are the same rows in the opposite order
    ends = np.flatnonzero(d != 0)
    changed = 0
    for lo, hi in zip(ends[:-1], ends[1:]):
        if hi - lo <= T:
            a = episode_returns_ref(r[lo + 1: hi + 1], d[lo + 1: hi + 1], T)
            b = 0.0
            for x in r[lo + 1: hi + 1][::-1].tolist():
                b += x
            assert len(a) == 1 and a[0] in fwd
            changed += int(a[0] != b and a[0] in (float(c["min_ret"]), float(c["max_ret"])))
    assert changed >= 1


def test_restatement_boundaries():
    one = np.ones(1, np.float32)
    with pytest.raises(ValueError):
        return_reward_range_ref(one, [0], 1000)
    assert return_reward_range_ref(one, [1], 1000) == (1.0, 1.0)
    r = np.arange(1, 12, dtype=np.float32)
    assert episode_returns_ref(r, np.zeros(11), 1) == r.tolist()                      # T = 1: every row
    with pytest.raises(ValueError):
        return_reward_range_ref(r, np.zeros(11), 12)                                  # T > n, no terminal
    assert episode_returns_ref(r, np.zeros(11), 11) == [66.0]                         # n == T
    assert episode_returns_ref(r, np.zeros(11), 3) == [6.0, 15.0, 24.0]               # 3 T + 2: the tail is dropped
    d = np.zeros(11)
    d[2] = 1                                                                          # a terminal on a timeout row: one boundary
    assert episode_returns_ref(r, d, 3) == [6.0, 15.0, 24.0]
    d[3] = 1                                                                          # ... the next episode restarts behind it
    assert episode_returns_ref(r, d, 3) == [6.0, 4.0, 18.0, 27.0]


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    bound = {name: (res, args) for name, res, args in hb.SYMBOLS}
    for name, nargs in NEW.items():
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == nargs, name
        fn = getattr(hb.lib(), name)                 # (AttributeError if the built library does not export it)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
    m = re.search(r"#define\s+IQLHIP_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == hb.lib().iqlhip_version() >= 310
    assert "NaN rewards are outside the contract" in re.sub(r"\s*\n \*\s*", " ", header)


def test_new_symbols_check_their_arguments_before_any_device_work():
    """Every refusal the header lists is answered on a machine without a GPU (nothing is launched), with a message."""
    lib = hb.lib()
    S, A = 17, 6
    ld = hb.row_stride(S, A)
    out, ep = (C.c_double * 2)(7.0, 7.0), C.c_int64(-3)
    rows = 4096          # never dereferenced: a non-NULL address
    good = dict(rows=rows, ld=ld, S=S, A=A, row0=0, n=10, T=1000)
    for bad in ({"rows": None}, {"n": 0}, {"n": -1}, {"row0": -1}, {"T": 0}, {"ld": ld - 1}):
        a = dict(good, **bad)
        assert lib.iqlhip_rows_return_range(a["rows"], a["ld"], a["S"], a["A"], a["row0"], a["n"], a["T"], out,
                                            C.byref(ep), None) == hb.E_INVAL, bad
        assert hb.last_error()
        if "T" not in bad:
            assert lib.iqlhip_rows_reward_scale(a["rows"], a["ld"], a["S"], a["A"], a["row0"], a["n"], 2.0, 3.0, None) == hb.E_INVAL, bad
            assert lib.iqlhip_rows_reward_shift(a["rows"], a["ld"], a["S"], a["A"], a["row0"], a["n"], 1.0, None) == hb.E_INVAL, bad
    assert lib.iqlhip_rows_return_range(rows, ld, S, A, 0, 10, 1000, None, C.byref(ep), None) == hb.E_INVAL
    assert lib.iqlhip_rows_return_range(rows, ld, S, A, 0, 10, 1000, out, None, None) == hb.E_INVAL
    assert lib.iqlhip_rows_reward_scale(rows, ld, S, A, 0, 10, 0.0, 3.0, None) == hb.E_INVAL and "divide_by" in hb.last_error()
    assert (out[0], out[1], ep.value) == (7.0, 7.0, -3)


def test_cpu_buffer_refuses():
    buf = iql.ReplayBuffer(3, 2, 8, "cpu")
    with pytest.raises(RuntimeError, match="runs in libiqlhip.so and needs a GPU buffer"):
        buf.modify_reward_("hopper-medium-v2", 1000)
    with pytest.raises(RuntimeError, match="runs in libiqlhip.so and needs a GPU buffer"):
        buf.return_reward_range(1000)
    assert buf._writes == 0
    assert hasattr(iql.OfflineReplayBuffer, "modify_reward_") and hasattr(iql.OfflineReplayBuffer, "return_reward_range")
