"""CPU-only tests of the n-step rows (iqlhip_rows_nstep, iqlhip_rows_nstep_ring, iqlhip_online_step_nstep;
jsrl-corl_amd/iqlhip_nstep.py): the restatement tests/nstep_ref.py gives hand-computed answers, is the
identity at N = 1, yields through the step's fp32 target expression the n-step return of the definition, and keeps a
ring equal to a rebuild of its unrolled rows; the Python layer refuses bad arguments before any library call, and the
three symbols are declared, bound and exported."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import iql
import iqlhip_binding as hb
import iqlhip_nstep as ns
import nstep_ref as R
from nstep_cases import pack, packed_rows, ring_transitions, row_stride

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _six_rows():
    """S = A = 1, row [s, a, s', r, d, pad x 3].  Two episodes: rows 0-2 end with done = 1, rows 3-5 run into the end
    of the data.  discount = 0.5 makes every value below exact."""
    rows = np.zeros((6, 8), dtype=np.float32)
    rows[:, 0] = [0, 1, 2, 3, 4, 5]                  # s
    rows[:, 1] = [10, 11, 12, 13, 14, 15]            # a
    rows[:, 2] = [100, 101, 102, 103, 104, 105]      # s'
    rows[:, 3] = [1, 2, 4, 8, 16, 32]                # r
    rows[:, 4] = [0, 0, 1, 0, 0, 0]                  # d
    rows[:, 5:] = 7.0                                # pad
    return rows


def test_known_answers_six_rows_two_episodes():
    rows = _six_rows()
    out, steps = R.build(rows, 1, 1, 3, 0.5)
    # row 0: 1 + .5 (2 + .5 * 4) = 3, ends at the done of row 2;  row 1: 2 + .5 * 4 = 4;  row 2: itself
    # row 3: 8 + .5 (16 + .5 * 32) = 24, d = 1 - .5^2;  row 4: 16 + .5 * 32 = 32, d = 1 - .5;  row 5: itself, d = 0
    assert steps.tolist() == [3, 2, 1, 3, 2, 1]
    assert out[:, 3].tolist() == [3, 4, 4, 24, 32, 32]
    assert out[:, 4].tolist() == [1, 1, 1, 0.75, 0.5, 0]
    assert out[:, 2].tolist() == [102, 102, 102, 105, 105, 105]
    assert np.array_equal(out[:, [0, 1, 5, 6, 7]], rows[:, [0, 1, 5, 6, 7]])
    # the step's expression on the derived rows: 3-step targets with V(s') = s'
    y = out[:, 3] + ((np.float32(1) - out[:, 4]) * np.float32(0.5)) * out[:, 2]
    assert y.tolist() == [3, 4, 4, 24 + 0.125 * 105, 32 + 0.25 * 105, 32 + 0.5 * 105]
    # a time limit behind row 4 that only the episode table knows: rows 3 and 4 stop there
    out, steps = R.build(rows, 1, 1, 3, 0.5, ep_last=np.array([2, 2, 2, 4, 4, 5]))
    assert steps.tolist() == [3, 2, 1, 2, 1, 1]
    assert out[:, 3].tolist() == [3, 4, 4, 16, 16, 32]
    assert out[:, 4].tolist() == [1, 1, 1, 0.5, 0, 0]
    assert out[:, 2].tolist() == [102, 102, 102, 104, 104, 105]
    # tail rows of a table without keep_tail (-1) fall back to the end of the range
    a = R.build(rows, 1, 1, 3, 0.5, ep_last=np.array([2, 2, 2, -1, -1, -1]))
    b = R.build(rows, 1, 1, 3, 0.5)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])
    # the brute-force target agrees on the exact example
    want = R.brute_force_target(rows, 1, 1, 3, 0.5, rows[:, 2].astype(np.float64))
    assert want.tolist() == [3, 4, 4, 24 + 0.125 * 105, 32 + 0.25 * 105, 32 + 0.5 * 105]


@pytest.mark.parametrize("S,A", [(3, 2), (17, 6)])
def test_horizon_one_is_the_identity(S, A):
    rng = np.random.default_rng(S)
    rows, ends = packed_rows(rng, 200, S, A, 5)
    for ep_last in (None, R.ep_last_from_ends(ends)):
        out, steps = R.build(rows, S, A, 1, 0.99, ep_last)
        assert np.array_equal(_bits(out), _bits(rows)) and np.all(steps == 1)


@pytest.mark.parametrize("N", [1, 2, 3, 5, 10])
def test_step_expression_on_derived_rows_is_the_n_step_target(N):
    """y32 = r + ((1.f - d) * discount_f32) * next_v on a derived row against the float64 target of the definition.
    With u = 2^-24, |r| <= 1, |V| <= 100, discount = 0.99, d in {0, 1} in the raw rows:
      r      (float)G, |G| <= sum_t 0.99^t <= N:                          |err| <= N u         (float64 terms ~1e-15)
      1 - d  the stored d errs by <= u d <= 0.1 u, the subtraction rounds once: 1 - d = 0.99^(k-1) (1 + e), |e| <= 1.3 u
             (exact 0 behind a terminal row)
      * discount_f32   (float)0.99 errs by <= u relative, the product rounds once: the coefficient c = 0.99^k (1 + e),
             |e| <= 3.4 u, c <= 1
      * next_v   one rounding: |c V| <= 100, |err| <= 100 * 4.4 u = 440 u
      r + ..     one rounding of |y| <= N + 100: <= (N + 100) u
    total <= (2 N + 540) u <= 560 u = 3.4e-5 for N <= 10."""
    rng = np.random.default_rng(100 + N)
    S, A, n, disc = 3, 2, 400, 0.99
    rows, ends = packed_rows(rng, n, S, A, N, first_done=True, last_done=True)
    v32 = rng.uniform(-100.0, 100.0, size=n).astype(np.float32)          # V of every raw row's own s'
    bound = (2 * N + 540) * 2.0 ** -24
    for ep_last in (None, R.ep_last_from_ends(ends)):
        out, steps = R.build(rows, S, A, N, disc, ep_last)
        m = np.arange(n) + steps.astype(np.int64) - 1
        r, d = out[:, 2 * S + A], out[:, 2 * S + A + 1]
        y32 = r + ((np.float32(1) - d) * np.float32(disc)) * v32[m]
        assert y32.dtype == np.float32
        want = R.brute_force_target(rows, S, A, N, disc, v32.astype(np.float64), ep_last)
        err = np.abs(y32.astype(np.float64) - want).max()
        print(f"N={N} ep_last={'yes' if ep_last is not None else 'no'}: max |y32 - y64| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        assert steps.max() <= N and (N == 1 or steps.max() > 1)


@pytest.mark.parametrize("capacity", [3, 7, 16])
def test_incremental_ring_equals_rebuild(capacity):
    S, A, N, disc = 3, 2, 5, 0.99
    ld = row_stride(S, A)
    rng = np.random.default_rng(capacity)
    raw = np.zeros((capacity, ld), dtype=np.float32)
    derived = rng.standard_normal((capacity, ld)).astype(np.float32)     # (garbage: every live row must be written)
    ends = np.zeros(capacity, dtype=np.uint8)
    steps = np.zeros(capacity, dtype=np.uint8)
    size = pointer = 0
    for t in ring_transitions(rng, 40, S, A, N):
        raw[pointer], ends[pointer] = pack(S, A, ld, t), t[5]
        newest, pointer, size = pointer, (pointer + 1) % capacity, min(size + 1, capacity)
        R.ring_refresh(raw, derived, ends, capacity, size, newest, N, disc, S, A, steps)
        order = R.unroll(capacity, size, newest)
        want, want_steps = R.build(raw[order], S, A, N, disc, R.ep_last_from_ends(ends[order]))
        assert np.array_equal(_bits(derived[order]), _bits(want))
        assert np.array_equal(steps[order], want_steps)


def test_python_refusals_name_the_cause_and_call_nothing(monkeypatch):
    monkeypatch.setattr(hb, "lib", lambda: pytest.fail("a refusal reached the library"))
    for bad in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError, match="horizon"):
            ns.check_args(bad, 0.99)
    for bad in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="discount"):
            ns.check_args(3, bad)
    assert ns.check_args(1, 1.0) == (1, 1.0) and ns.check_args(64, 0.5) == (64, 0.5)
    import torch
    table = types.SimpleNamespace(ep_last=torch.zeros(9, dtype=torch.int64))
    with pytest.raises(ValueError, match="episodes table covers"):
        ns.check_episodes(table, 10)
    assert ns.check_episodes(None, 10) is None and ns.check_episodes(table, 9).shape == (9,)
    # a CPU buffer: as the variance learner refuses one
    cpu = iql.ReplayBuffer(3, 2, 8, "cpu")
    with pytest.raises(NotImplementedError, match="GPU"):
        cpu.nstep(3, 0.99)
    with pytest.raises(NotImplementedError, match="GPU"):
        iql.NStepReplay(cpu, 3, 0.99)
    assert cpu._writes == 0
    # data parallelism on the fused call, before the trainer or the buffers are touched
    fake = object.__new__(ns.NStepReplay)
    for world, exchange in ((2, None), (1, "rccl"), (1, "torch")):
        tr = types.SimpleNamespace(_dp_world=world, _dp_exchange=exchange)
        with pytest.raises(NotImplementedError, match="data parallelism"):
            ns.online_step_nstep(tr, fake, None, None, 0.0, None, False, 4)
    with pytest.raises(ValueError, match="NStepReplay"):
        ns.online_step_nstep(types.SimpleNamespace(_dp_world=1, _dp_exchange=None), cpu, None, None, 0.0, None, False, 4)
    assert hasattr(iql.ImplicitQLearning, "online_step_nstep")


NARGS = {"iqlhip_rows_nstep": 13, "iqlhip_rows_nstep_ring": 13, "iqlhip_online_step_nstep": 22}


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    bound = {name: (res, args) for name, res, args in hb.SYMBOLS}
    for name, nargs in NARGS.items():
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert bound[name][0] is C.c_int and len(bound[name][1]) == nargs, name
        fn = getattr(hb.lib(), name)                 # (AttributeError if the built library does not export it)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
    m = re.search(r"#define\s+IQLHIP_NSTEP_MAX_HORIZON\s+(\d+)", header)
    assert m and int(m.group(1)) == hb.IQLHIP_NSTEP_MAX_HORIZON == ns.MAX_HORIZON == 64
    m = re.search(r"#define\s+IQLHIP_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == hb.lib().iqlhip_version() >= 410


def test_library_refuses_before_any_device_work():
    """Every refusal the header lists is answered on a machine without a GPU (nothing is launched), with a message."""
    lib = hb.lib()
    S, A = 17, 6
    ld = hb.row_stride(S, A)
    src, dst = 1 << 20, 1 << 30          # never dereferenced: aligned, far apart
    good = dict(src=src, src_ld=ld, dst=dst, dst_ld=ld, S=S, A=A, row0=0, n=10, N=3, discount=0.99, ep=None, steps=None)

    def build(**kw):
        a = dict(good, **kw)
        return lib.iqlhip_rows_nstep(a["src"], a["src_ld"], a["dst"], a["dst_ld"], a["S"], a["A"], a["row0"], a["n"], a["N"],
                                     a["discount"], a["ep"], a["steps"], None)

    nan, inf = float("nan"), float("inf")
    for bad in ({"src": None}, {"dst": None}, {"n": 0}, {"row0": -1}, {"S": 0}, {"A": 0}, {"src_ld": ld - 4}, {"dst_ld": ld - 4},
                {"src_ld": ld + 1}, {"dst_ld": ld + 2}, {"src": src + 4}, {"dst": dst + 8}, {"dst": src},
                {"dst": src + 4 * ld * 5}, {"N": 0}, {"N": 65}, {"N": -3}, {"discount": 0.0}, {"discount": -0.1},
                {"discount": 1.0000001}, {"discount": nan}, {"discount": inf}, {"ep": 4}):
        assert build(**bad) == hb.E_INVAL, bad
        assert hb.last_error(), bad
    assert build(dst=src) == hb.E_INVAL and "in place" in hb.last_error()

    ring_good = dict(src=src, dst=dst, ld=ld, S=S, A=A, cap=8, size=8, newest=3, ends=4096, N=3, discount=0.99)

    def ring(**kw):
        a = dict(ring_good, **kw)
        return lib.iqlhip_rows_nstep_ring(a["src"], a["dst"], a["ld"], a["S"], a["A"], a["cap"], a["size"], a["newest"],
                                          a["ends"], a["N"], a["discount"], None, None)

    for bad in ({"src": None}, {"dst": None}, {"ends": None}, {"dst": src}, {"ld": ld - 4}, {"cap": 0}, {"size": 0},
                {"size": 9}, {"newest": -1}, {"newest": 8}, {"size": 4, "newest": 4}, {"N": 0}, {"N": 65},
                {"discount": nan}, {"discount": 2.0}):
        assert ring(**bad) == hb.E_INVAL, bad
        assert hb.last_error(), bad
    # the fused call: its own NULL checks come first, without a context
    assert lib.iqlhip_online_step_nstep(None, src, dst, ld, 8, 0, None, None, 4, None, None, None, 1.0, 0, None, None,
                                        4096, 0, 1, 3, 0.99, None) == hb.E_INVAL
