"""CPU tests of the generated variance-learner cases (tests/variance_cases.py; DESIGN.md 6l "Widths, row counts and
trained-like values"): every case tests/test_hip_variance_shapes.py runs is what it claims to be — the cleaning ended, no
row is near a clip bound, the float32 and the float64 restatement agree on every ReLU mask and every gate bit, the
constructed units are dead / exactly zero, the kind delivers its row classes — so that the GPU tests cannot pass over an
empty or degenerate case.  The resulting bounds are printed."""
import numpy as np
import pytest

import variance_cases as VC
import variance_ref as R


def _check_case(c, nets32=None, nets64=None):
    """The conditions of one case under the nets of each precision; returns the float64 values."""
    B = c["B"]
    n32 = (c["mf"], c["vf"]) if nets32 is None else nets32
    n64 = (c["mf"], c["vf"]) if nets64 is None else nets64
    assert c["rounds"] <= VC.ROUNDS and c["obs"].shape == (B, c["S"]) and c["last"].shape == (c["S"],)
    assert c["obs"].dtype == c["last"].dtype == c["rewards"].dtype == np.float32 and c["nd"].dtype == bool
    assert np.abs(c["rewards"]).max() <= 10.0 and (B < 4 or np.abs(c["rewards"]).max() > 2.0)
    with np.errstate(over="ignore"):
        f32 = R.values(n32[0], n32[1], c["obs"], c["last"], c["rewards"], c["nd"], np.float32, c["aligned"])
        f64 = R.values(n64[0], n64[1], c["obs"], c["last"], c["rewards"], c["nd"], np.float64, c["aligned"])
    # the clip condition, and the gate bits
    assert VC.clip_distance(np.log(f64["e"])).min() > 1e-3
    assert np.array_equal(f32["open"], f64["open"])
    # every ReLU mask; the constructed units
    for k, key in enumerate(("act_m", "act_v")):
        sets = c["sets"][k]
        for l in (0, 1):
            a32, a64 = f32[key][l], f64[key][l]
            assert np.array_equal(a32 > 0, a64 > 0), (key, l)
            dead = sets["dead0" if l == 0 else "dead1"]
            assert len(dead) == VC.N_DEAD and not a32[:, dead].any() and not a64[:, dead].any()
            live = np.setdiff1d(np.arange(256), np.concatenate([dead, sets["zero0"]]) if l == 0 else dead)
            share = (a64[:, live] > 0).mean()
            assert 0.2 < share < 0.8, (key, l, share)
            # ... and nothing else sits within tau of zero: a mask cannot depend on a summation's order
            pos = a64[:, live][a64[:, live] > 0]
            assert pos.min() > c["tau"][l] > 0.0
        assert len(sets["zero0"]) == VC.N_ZERO and not f32[key][0][:, sets["zero0"]].any() and not f64[key][0][:, sets["zero0"]].any()
        assert not n32[k]["w0"][sets["zero0"]].any() and not n32[k]["b0"][sets["zero0"]].any()
    for k in (0, 1):
        assert len(c["sets"][k]["w2zero"]) == VC.N_ZERO
    return f32, f64


def _counts(f32, f64):
    e = f64["e"]
    with np.errstate(over="ignore"):
        inf = int(np.isinf(f32["e"]).sum())
    return int((e < R.CLIP_LO).sum()), int((e > R.CLIP_HI).sum()), int(f64["open"].sum()), inf


@pytest.mark.parametrize("name", list(VC.CASES))
def test_case_is_clean_and_delivers_its_kind(name):
    S, B, _seed, kind, aligned, dones = VC.CASES[name]
    c = VC.case(name)
    assert (c["S"], c["B"], c["kind"], c["aligned"]) == (S, B, kind, aligned)
    f32, f64 = _check_case(c)
    for k in (0, 1):
        assert not (c["vf"] if k else c["mf"])["w2"][0, c["sets"][k]["w2zero"]].any()
    assert np.abs(f64["pred"]).max() > 10.0                  # mf's values are in the tens
    lo, hi, n_open, inf = _counts(f32, f64)
    assert lo + hi + n_open == B
    if kind == "mixed":
        assert lo > 0 and hi > 0 and n_open > 0 and (inf > 0 or B < 4), (lo, hi, n_open, inf)
    elif kind == "closed":
        assert n_open == 0 and lo > 0 and hi > 0 and inf > 0
    assert {"none": not c["nd"].any(), "all": c["nd"].all(), "random": True}[dones]
    if dones == "random" and B >= 63:
        assert 0 < c["nd"].sum() < B
    for which in (0, 1):
        s32, s64, bound = VC.reference(name, which)
        dev = R.deviations(s32, s64, full_w1=True)
        print(f"{name} net{which}: " + "  ".join(f"{k} {dev[k]:.2e} (bound {bound[k]:.2e})" for k in dev))
        assert all(np.isfinite(bound[k]) and bound[k] >= R.PROJECT[k] for k in R.PROJECT)
        if which == 1 and kind == "closed":      # every row clipped: dy = 0, the step leaves vf as it is
            assert all(not s64["grads"][k].any() and np.array_equal(s64["params"][k], c["vf"][k]) for k in R.KEYS)
        else:                                    # ... otherwise the gradient lives on most units, and on none of the constructed ones
            sets, g = c["sets"][which], s64["grads"]
            live0 = np.setdiff1d(np.arange(256), np.concatenate([sets["dead0"], sets["zero0"]]))
            live1 = np.setdiff1d(np.arange(256), sets["dead1"])
            assert (g["b0"][live0] != 0).mean() > 0.2 and (g["w2"][0, live1] != 0).mean() > 0.2
            assert not g["w0"][sets["dead0"]].any() and not g["w0"][sets["zero0"]].any() and not g["b0"][sets["zero0"]].any()
            assert not g["w1"][sets["dead1"]].any() and not g["b1"][sets["dead1"]].any() and not g["b1"][sets["w2zero"]].any()
            assert not g["w1"][:, sets["dead0"]].any() and not g["w1"][:, sets["zero0"]].any() and not g["w2"][0, sets["dead1"]].any()


def test_case_list_covers_the_widths_and_row_counts():
    shapes = {(v[0], v[1]) for v in VC.CASES.values()}
    assert {(S, 31) for S in (1, 2, 4, 15, 16, 31, 32, 33, 63, 64, 65, 126, 127)} <= shapes
    assert {(S, B) for S in (64, 127) for B in (3, 15, 16, 31, 63, 1023, 1024)} <= shapes
    assert {(64, 63), (16, 16), (17, 33), (64, 256)} <= shapes
    assert {S % 4 for S, _ in shapes} == {0, 1, 2, 3} and {(S + 16) >> 4 for S, B in shapes if B == 31} >= {1, 2, 4, 5, 8}


def test_the_open_kind_keeps_every_row_open():
    c = VC.make_case(17, 33, 5017, "open")
    f32, f64 = _check_case(c)
    assert _counts(f32, f64) == (0, 0, 33, 0)


def test_chain_cases_are_clean_under_the_evolved_parameters():
    P32 = P64 = None
    for k, ((c, s32, s64), which) in enumerate(zip(VC.chain(), VC.CHAIN["which"])):
        if P32 is None:
            P32 = P64 = (c["mf"], c["vf"])
        f32, f64 = _check_case(c, P32, P64)
        lo, hi, n_open, inf = _counts(f32, f64)
        assert lo > 0 and hi > 0 and n_open > 0 and inf > 0
        dev = R.deviations(s32, s64, full_w1=True)
        print(f"chain step {k} net{which}: " + "  ".join(f"{q} {dev[q]:.2e} (bound {R.bounds(dev)[q]:.2e})" for q in dev))
        P32 = tuple(s32["params"] if i == which else P32[i] for i in (0, 1))
        P64 = tuple(s64["params"] if i == which else P64[i] for i in (0, 1))
        if k:
            assert s64["m"]["w1"].any() and s64["v"]["w1"].any()
    assert all(not np.array_equal(VC.chain()[0][0]["obs"], VC.chain()[k][0]["obs"]) for k in range(1, 6))
