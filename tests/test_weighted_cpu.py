"""CPU tests of weighted replay sampling: the integer definition of the distribution (tests/weighted_ref.py)
and the checks that need no GPU (iqlhip_weighted.py, ReplayBuffer.set_sample_weights on a CPU buffer, the C ABI's
symbols)."""
import os
import re

import numpy as np
import pytest
import torch

import iql
import iqlhip_binding as hb
import iqlhip_weighted as wtd
import weighted_ref as W
from oracle import philox_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("iqlhip_weights_build", "iqlhip_weights_free", "iqlhip_weights_info", "iqlhip_draw_indices_weighted",
               "iqlhip_train_steps_weighted", "iqlhip_train_steps_weighted_prepare")


# ---------------------------------------------------------------- the distribution
@pytest.mark.parametrize("n,seed,offset,j0", [(1, 0, 0, 0), (7, 3, 11, 0), (4097, 5, 123456789, 3),
                                              (1000, 2 ** 63 + 9, 2 ** 64 - 1, 1), (262145, 7, 2 ** 40, 0),
                                              (3 * 2 ** 20, 1, 5, 7)])
@pytest.mark.parametrize("value", [1.0, 3.0, 2.0 ** -130, 1e30])
def test_equal_weights_are_the_plain_stream(n, seed, offset, j0, value):
    """All weights equal: total = n q, and floor(floor(r n q / 2^64) / q) = floor(r n / 2^64) — the plain draw, bit for
    bit (an odd j0, an offset one below 2^64; a denormal and a huge common weight)."""
    w = np.full(n, value, dtype=np.float32)
    got = W.draw_indices(513, w, seed, offset, j0)
    want = P.draw_indices(513, n, seed, offset, j0)
    assert np.array_equal(got, want)


def test_zero_weight_rows_are_never_drawn():
    rng = np.random.RandomState(0)
    w = rng.rand(300).astype(np.float32)
    zero = rng.rand(300) < 0.5
    zero[:5] = True
    zero[-5:] = True
    w[zero] = 0.0
    idx = W.draw_indices(20000, w, 9, 77)
    assert not np.any(zero[idx])
    assert set(np.unique(idx)) == set(np.nonzero(~zero)[0])          # ... and every other row is


@pytest.mark.parametrize("n", [1, 2, 65, 4097])
@pytest.mark.parametrize("last", [False, True])
def test_a_single_non_zero_weight(n, last):
    w = np.zeros(n, dtype=np.float32)
    row = n - 1 if last else 0
    w[row] = 0.37
    assert np.all(W.draw_indices(1000, w, 4, 2 ** 64 - 3) == row)


def test_a_weight_40_binades_below_the_largest_quantises_to_zero():
    for wmax in (1.0, 1.5, 2.0 ** -60, 3e20):
        wmax = np.float32(wmax)
        w = np.array([wmax, wmax * np.float32(2.0 ** -40), wmax * np.float32(2.0 ** -38)], dtype=np.float32)
        q = W.quantise(w)
        assert q[1] == 0 and q[2] >= 1
        assert np.all(W.draw_indices(5000, w[:2], 1, 0) == 0)


def test_the_largest_quantum_lies_in_2_38_to_2_39():
    for e in range(-100, 101):
        for mant in (1.0, 1.25, 1.9999999):
            wmax = np.float32(mant * 2.0 ** e)
            q = W.quantise(np.array([wmax, wmax / np.float32(3.0), 0.0], dtype=np.float32))
            assert 2 ** 38 <= int(q[0]) < 2 ** 39, (e, mant, int(q[0]))
            assert int(q[0]) == int(np.floor(float(wmax) * 2.0 ** (38 - W.exponent(np.array([wmax])))))
    # a denormal largest weight
    q = W.quantise(np.array([1e-45, 3e-45], dtype=np.float32))
    assert 2 ** 38 <= int(q[1]) < 2 ** 39 and 0 < int(q[0]) < int(q[1])


def test_quantisation_is_floor_of_the_scaled_weight():
    rng = np.random.RandomState(3)
    w = (rng.rand(5000) * np.exp(rng.randn(5000) * 6)).astype(np.float32)
    sh = 38 - W.exponent(w)
    # (float64 holds w * 2^sh exactly: the product has the weight's 24 significant bits)
    want = [int(float(x) * 2.0 ** sh) for x in w]
    assert [int(a) for a in W.quantise(w)] == want


def test_frequencies_follow_the_weights():
    """200 000 draws over 8 rows with weights 1..8: every row within 5 standard deviations of w / sum(w) (a fixed seed:
    deterministic)."""
    w = np.arange(1, 9, dtype=np.float32)
    N = 200000
    idx = W.draw_indices(N, w, 12345, 0)
    p = w.astype(np.float64) / w.sum()
    count = np.bincount(idx, minlength=8)
    sd = np.sqrt(N * p * (1 - p))
    assert np.all(np.abs(count - N * p) <= 5 * sd), (count, N * p, sd)


def test_reference_refuses_what_the_library_refuses():
    for bad in ([1.0, np.nan], [1.0, np.inf], [1.0, -1.0], [0.0, 0.0]):
        with pytest.raises(ValueError):
            W.table(np.array(bad, dtype=np.float32))


# ---------------------------------------------------------------- the checks that need no GPU
def test_check_vector():
    assert wtd.check_vector(np.ones(5, dtype=np.float32), 5) == "numpy"
    assert wtd.check_vector(torch.ones(5), 5) == "torch"
    for bad, n in ((np.ones(4, dtype=np.float32), 5), (np.ones(5, dtype=np.float64), 5), (np.ones((5, 1), dtype=np.float32), 5),
                   (torch.ones(5, dtype=torch.float64), 5), (torch.ones(5, 1), 5), ([1.0] * 5, 5),
                   (np.ones(0, dtype=np.float32), 0)):
        with pytest.raises(ValueError):
            wtd.check_vector(bad, n)
    with pytest.raises(ValueError, match="2\\^24"):
        wtd.check_vector(np.ones(1, dtype=np.float32), (1 << 24) + 1)


def test_check_host_values():
    wtd.check_host_values(np.array([0.0, 2.0], dtype=np.float32))
    for bad in ([1.0, np.nan], [np.inf, 1.0], [1.0, -1e-30], [0.0, 0.0]):
        with pytest.raises(ValueError):
            wtd.check_host_values(np.array(bad, dtype=np.float32))


def test_check_trainer():
    wtd.check_trainer(1, None, "f32", 4096, 512)
    wtd.check_trainer(1, None, "bf16", 512, 512)
    with pytest.raises(NotImplementedError):
        wtd.check_trainer(2, "p2p", "f32", 256, 512)
    with pytest.raises(NotImplementedError):
        wtd.check_trainer(1, "rccl", "f32", 256, 512)
    with pytest.raises(NotImplementedError):
        wtd.check_trainer(1, None, "bf16", 513, 512)


def test_a_cpu_buffer_takes_no_weights():
    buf = iql.ReplayBuffer(3, 2, 10, "cpu")
    assert buf.sample_weights_n is None
    buf.set_sample_weights(None)                                  # clearing nothing is fine
    with pytest.raises(ValueError, match="GPU"):
        buf.set_sample_weights(np.ones(10, dtype=np.float32))
    with pytest.raises(ValueError, match="GPU"):
        wtd.check_call(buf)
    assert buf.sample_weights_n is None


def test_check_call_sees_a_changed_index_bound():
    class Fake:
        _gpu = True
        sample_weights_n = None
        size = 7

        def _index_bound(self):
            return self.size
    f = Fake()
    with pytest.raises(ValueError, match="no sample weights"):
        wtd.check_call(f)
    f.sample_weights_n = 7
    assert wtd.check_call(f) == 7
    f.size = 8
    with pytest.raises(ValueError, match="set_sample_weights again"):
        wtd.check_call(f)


# ---------------------------------------------------------------- C ABI
def test_header_binding_and_library_agree_on_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    declared = set(re.findall(r"\b(iqlhip_[a-z_0-9]+)\s*\(", header))
    bound = {name for name, _, _ in hb.SYMBOLS}
    lib = hb.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in bound and hasattr(lib, name), name
