"""CPU-only tests of the episode-returns ingest (iqlhip_rows_episode_returns, ReplayBuffer.episode_returns): the
restatement tests/returns_ref.py agrees with tests/reward_ref.py on the episodes they share and reproduces the
reference's recorded get_return_to_go / keep_best_trajectories results (tests/golden/g18_return_to_go.npz) bit for bit;
the new symbol is declared, exported and bound, and refuses bad arguments without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import iql
import iqlhip_binding as hb
from helpers import load_golden
from returns_ref import (breaks_ref, episode_returns_rows_ref, episode_table_ref, rows_episode_returns_ref,
                         top_fraction_weights_ref)
from reward_ref import episode_returns_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = 17


def _wide(rng, n):
    return (rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-6.0, 6.0, size=n)).astype(np.float32)


def _bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def _closed_form(brk, T, keep_tail):
    """The header's definition of ends and starts: p(i), o = i - p(i) - 1, (o + 1) % T, p(i) + 1 + (o / T) * T."""
    n = len(brk)
    idx = np.where(brk, np.arange(n), -1)
    prev = np.maximum.accumulate(idx)
    p = np.concatenate(([-1], prev[:-1]))
    o = np.arange(n) - p - 1
    ends = brk | ((o + 1) % T == 0)
    if keep_tail:
        ends[-1] = True
    return ends, p + 1 + (o // T) * T


@pytest.mark.parametrize("T", [1, 7, 64, 1000])
def test_rule_off_tail_off_are_the_reward_ingests_episodes(T):
    rng = np.random.default_rng(T)
    n = 1500
    r, d = _wide(rng, n), (rng.random(n) < 0.01).astype(np.float32)
    d[[40, 41]] = 1.0
    ret, rtg, first, last, episodes = episode_returns_rows_ref(r, breaks_ref(d), T, 1.0)
    want = episode_returns_ref(r, d, T)
    f, l, per_episode, g0 = episode_table_ref(ret, rtg, first, last)
    assert per_episode.tolist() == want and episodes == len(want) == len(l)
    # the spans are the closed form of the header, and tail rows belong to no episode
    ends, starts = _closed_form(d != 0, T, False)
    assert np.array_equal(np.flatnonzero(ends), l) and np.array_equal(starts[l], f)
    tail = np.arange(n) > (l[-1] if len(l) else -1)
    assert np.all(first[tail] == -1) and np.all(last[tail] == -1) and np.all(ret[tail] == 0.0) and np.all(rtg[tail] == 0.0)
    assert np.all(first[~tail] <= np.arange(n)[~tail]) and np.all(np.arange(n)[~tail] <= last[~tail])
    # discount 1: return-to-go at the first row is the same rewards added from the other end
    for a, b, x in zip(f, l, g0):
        acc = 0.0
        for v in r[a: b + 1][::-1].tolist():
            acc = v + acc
        assert acc == x


def test_keep_tail_and_closed_form_with_the_rule():
    rng = np.random.default_rng(3)
    n, S = 500, 4
    obs = rng.standard_normal((n + 1, S)).astype(np.float32)
    s, ns = obs[:-1].copy(), obs[1:].copy()
    s[[100, 101, 333]] += np.float32(1.0)
    d = np.zeros(n, np.float32)
    d[[10, 250]] = 1.0
    brk = breaks_ref(d, s, ns, 1e-6)
    assert np.flatnonzero(brk).tolist() == [10, 99, 100, 250, 332]
    r = _wide(rng, n)
    for keep_tail in (False, True):
        ret, rtg, first, last, episodes = episode_returns_rows_ref(r, brk, 90, 0.99, keep_tail)
        ends, starts = _closed_form(brk, 90, keep_tail)
        f, l, _, _ = episode_table_ref(ret, rtg, first, last)
        assert np.array_equal(np.flatnonzero(ends), l) and np.array_equal(starts[l], f) and episodes == len(l)
        assert (last[-1] == n - 1) == keep_tail
    assert np.array_equal(breaks_ref(d, s, ns, None), d != 0)


def test_restatement_reproduces_get_return_to_go_bit_for_bit():
    z, _ = load_golden("g18_return_to_go")
    T, discount, tol = int(z["T"]), float(z["discount"]), float(z["tol"])
    brk = breaks_ref(z["terminals"], z["s"], z["ns"], tol)
    assert brk.sum() == (z["terminals"] != 0).sum() + 1                   # the one discontinuity that is no terminal
    ret, rtg, first, last, episodes = episode_returns_rows_ref(z["rewards"], brk, T, discount, keep_tail=True)
    assert rtg.dtype == np.float64 and np.array_equal(_bits(rtg), _bits(z["return_to_go"]))
    lengths = (last - first + 1)[last == np.arange(len(last))]
    assert episodes == len(lengths) >= 9 and (lengths == T).sum() >= 3 and (lengths == 1).sum() >= 2 and first.min() == 0
    assert last[-1] == len(last) - 1 and lengths[-1] < T                  # the tail that only the end of the data ends
    # the fixture pins the order: the discounted sums taken from the episodes' first rows forward differ in some episode
    differs = 0
    for a, b in zip(first[last == np.arange(len(last))], np.flatnonzero(last == np.arange(len(last)))):
        acc = 0.0
        for k, v in enumerate(z["rewards"][a: b + 1].tolist()):
            acc += discount ** k * v
        differs += int(acc != rtg[a])
    assert differs >= 1


def test_restatement_keeps_the_trajectories_the_reference_keeps():
    z, meta = load_golden("g18_return_to_go")
    T, discount = int(z["T"]), float(z["discount"])
    out = episode_returns_rows_ref(z["keep_rewards"], breaks_ref(z["keep_terminals"]), T, discount)
    for frac in meta["fracs"]:
        w = top_fraction_weights_ref(*out[:4], frac)
        assert w.dtype == np.float32 and np.array_equal(np.flatnonzero(w), z[f"kept_{frac}"]), frac
        assert set(np.unique(w)) <= {0.0, 1.0}
    assert len(z["kept_0.1"]) < len(z["kept_0.5"]) < len(z["kept_1.0"])


def test_top_fraction_ties_and_errors():
    r = np.array([1, 1, 5, 1, 1, 2, 2], np.float32)
    d = np.array([0, 1, 1, 0, 1, 1, 0], np.float32)                       # returns 2, 5, 2, 2; one tail row
    out = episode_returns_rows_ref(r, breaks_ref(d), 1000, 1.0)
    assert out[4] == 4
    assert top_fraction_weights_ref(*out[:4], 0.5, "ep_return").tolist() == [1, 1, 1, 0, 0, 0, 0]      # the earlier of the ties
    assert top_fraction_weights_ref(*out[:4], 0.0).tolist() == [0, 0, 1, 0, 0, 0, 0]                   # at least one episode
    assert top_fraction_weights_ref(*out[:4], 1.0).tolist() == [1, 1, 1, 1, 1, 1, 0]                   # never the tail
    none = episode_returns_rows_ref(r[:1], breaks_ref(d[:1]), 1000, 1.0)
    assert none[4] == 0
    with pytest.raises(ValueError):
        top_fraction_weights_ref(*none[:4], 0.5)


def test_sparse_option():
    r = np.array([0, 0, -1, 0, 0, 3, -1], np.float32)
    d = np.array([0, 0, 1, 0, 0, 1, 1], np.float32)
    _, rtg, _, _, _ = episode_returns_rows_ref(r, breaks_ref(d), 1000, 0.9, sparse_value=-1.0)
    assert rtg[:3].tolist() == [-1.0 / (1.0 - 0.9)] * 3 and rtg[6] == -1.0 / (1.0 - 0.9)
    assert rtg[3:6].tolist() == [0.0 + 0.9 * (0.0 + 0.9 * 3.0), 0.0 + 0.9 * 3.0, 3.0]


def test_rows_form_reads_the_packed_columns():
    S, A = 3, 1
    ld = hb.row_stride(S, A)
    rng = np.random.default_rng(9)
    rows = rng.standard_normal((30, ld)).astype(np.float32)
    rows[:, 2 * S + A + 1] = 0.0
    rows[[7, 20], 2 * S + A + 1] = 1.0
    rows[1:, :S] = rows[:-1, S + A: 2 * S + A]
    rows[12, 0] += np.float32(0.25)
    a = rows_episode_returns_ref(rows, S, A, 1000, 0.99, tol=1e-6, keep_tail=True)
    assert a[4] == 4 and a[3].tolist() == [7] * 8 + [11] * 4 + [20] * 9 + [29] * 9
    b = rows_episode_returns_ref(rows, S, A, 1000, 0.99)
    assert b[4] == 2 and b[3].tolist() == [7] * 8 + [20] * 13 + [-1] * 9


def test_new_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    name = "iqlhip_rows_episode_returns"
    m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", header)
    assert m and len(m.group(1).split(",")) == NARGS
    bound = {n: (res, args) for n, res, args in hb.SYMBOLS}
    assert bound[name][0] is C.c_int and len(bound[name][1]) == NARGS
    fn = getattr(hb.lib(), name)                     # (AttributeError if the built library does not export it)
    assert fn.restype is C.c_int and len(fn.argtypes) == NARGS
    m = re.search(r"#define\s+IQLHIP_EP_KEEP_TAIL\s+(\d+)", header)
    assert m and int(m.group(1)) == hb.IQLHIP_EP_KEEP_TAIL == 1
    m = re.search(r"#define\s+IQLHIP_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == hb.lib().iqlhip_version() >= 390


def test_new_symbol_checks_its_arguments_before_any_device_work():
    """Every refusal the header lists is answered on a machine without a GPU (nothing is launched), with a message."""
    lib = hb.lib()
    S, A = 17, 6
    ld = hb.row_stride(S, A)
    ep = C.c_int64(-3)
    sparse = C.c_double(-1.0)
    ptr = 4096           # never dereferenced: a non-NULL address
    good = dict(rows=ptr, ld=ld, S=S, A=A, row0=0, n=10, T=1000, discount=0.99, tol=-1.0, flags=0, sparse=None,
                ret=ptr, rtg=ptr, first=ptr, last=ptr, ep=C.byref(ep))

    def call(**kw):
        a = dict(good, **kw)
        return lib.iqlhip_rows_episode_returns(a["rows"], a["ld"], a["S"], a["A"], a["row0"], a["n"], a["T"], a["discount"],
                                               a["tol"], a["flags"], a["sparse"], a["ret"], a["rtg"], a["first"], a["last"],
                                               a["ep"], None)

    inf, nan = float("inf"), float("nan")
    for bad in ({"rows": None}, {"n": 0}, {"n": -1}, {"row0": -1}, {"S": 0}, {"A": 0}, {"ld": ld - 1},       # reward_args_ok
                {"T": 0}, {"T": -5}, {"discount": nan}, {"discount": inf}, {"discount": -0.5}, {"tol": nan},
                {"flags": 2}, {"flags": -1}, {"flags": 3},
                {"ret": None, "rtg": None, "first": None, "last": None, "ep": None},
                {"sparse": C.byref(sparse), "discount": 1.0}):
        assert call(**bad) == hb.E_INVAL, bad
        assert hb.last_error(), bad
    assert ep.value == -3


def test_cpu_buffer_refuses():
    buf = iql.ReplayBuffer(3, 2, 8, "cpu")
    with pytest.raises(RuntimeError, match="runs in libiqlhip.so and needs a GPU buffer"):
        buf.episode_returns()
    assert buf._writes == 0
    assert hasattr(iql.OfflineReplayBuffer, "episode_returns")
