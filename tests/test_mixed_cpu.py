"""CPU tests of the mixed offline / online batch semantics (jsrl-corl_amd/iqlhip_mixed.py) and of its index reference
(tests/mixed_ref.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import iqlhip_binding as hb
import iqlhip_mixed as mixed
import mixed_ref
from oracle import philox_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"iqlhip_online_step_mixed": 19, "iqlhip_train_steps_mixed": 13, "iqlhip_train_steps_mixed_prepare": 8}


@pytest.mark.parametrize("B,ratio,n_off", [(8, 0.4, 3), (256, 0.5, 128), (7, 0.3, 2), (256, 0.999, 255)])
def test_split_is_cal_qls_expression(B, ratio, n_off):
    assert mixed.split(B, ratio) == (n_off, B - n_off)
    assert n_off == int(B * ratio)


@pytest.mark.parametrize("B,ratio", [(8, 0.0), (8, 0.1), (8, 1.0), (256, 0.001), (1, 0.5), (8, 1.5), (8, -0.5)])
def test_split_refuses_an_empty_part_and_names_the_plain_call(B, ratio):
    with pytest.raises(ValueError, match=r"online_step / train_steps"):
        mixed.split(B, ratio)


def test_host_draw_consumes_numpy_like_the_two_sample_calls_in_reference_order():
    for size_off, n_off, size_on, n_on in ((5000, 3, 1, 5), (1000, 128, 77, 128), (12, 2, 4, 5)):
        np.random.seed(123)
        want_off = np.random.randint(0, size_off, size=n_off)          # offline_buffer.sample(n_off)
        want_on = np.random.randint(0, size_on, size=n_on)             # online_buffer.sample(n_on), size after the insert
        after = np.random.randint(0, 1 << 30)
        np.random.seed(123)
        idx_off, idx_on = mixed.draw_host_indices(size_off, n_off, size_on, n_on)
        assert idx_off.dtype == np.int64 and idx_on.dtype == np.int64
        assert np.array_equal(idx_off, want_off) and np.array_equal(idx_on, want_on)
        assert np.random.randint(0, 1 << 30) == after                  # nothing else was consumed
    with pytest.raises(ValueError):
        mixed.draw_host_indices(0, 3, 10, 5)


@pytest.mark.parametrize("B,n_off", [(8, 3), (7, 2), (256, 128)])
def test_mixed_ref_is_two_draws_per_step_of_the_one_stream(B, n_off):
    K, size_off, size_on, seed = 9, 5000, 37, 5
    offset = mixed_ref.call_offset(11, B)
    idx_off, idx_on = mixed_ref.mixed_indices(K, B, n_off, size_off, size_on, seed, offset)
    assert idx_off.shape == (K, n_off) and idx_on.shape == (K, B - n_off)
    for k in range(K):
        assert np.array_equal(idx_off[k], R.draw_indices(n_off, size_off, seed, offset, j0=k * B)), k
        assert np.array_equal(idx_on[k], R.draw_indices(B - n_off, size_on, seed, offset, j0=k * B + n_off)), k
    assert idx_off.min() >= 0 and idx_off.max() < size_off and idx_on.min() >= 0 and idx_on.max() < size_on
    # the stream is the plain call's: the same counters, whatever the split
    assert R.call_counter_range(offset, K * B) == (offset, offset + (K * B + 1) // 2)


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "iqlhip.h")).read()
    bound = {name: (res, args) for name, res, args in hb.SYMBOLS}
    for name, nargs in NEW.items():
        m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == nargs, name
        fn = getattr(hb.lib(), name)                 # (AttributeError if the built library does not export it)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
    m = re.search(r"#define\s+IQLHIP_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == hb.lib().iqlhip_version() >= 340


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = hb.lib()
    fake = 4096       # never dereferenced: every rejection below comes before a context is looked at
    out = (C.c_float * 3)()
    sc = hb.StepScalars()
    idx = (C.c_int64 * 4)()
    assert lib.iqlhip_online_step_mixed(None, fake, 44, 8, 0, fake, idx, 4, C.byref(sc), out, None, 1.0, 0, None, None,
                                        fake + 64, 8, idx, 4) == hb.E_INVAL
    assert lib.iqlhip_online_step_mixed(fake, fake, 44, 8, 0, fake, idx, 4, C.byref(sc), out, None, 1.0, 0, None, None,
                                        None, 8, idx, 4) == hb.E_INVAL                    # no offline rows
    assert lib.iqlhip_online_step_mixed(fake, fake, 44, 8, 0, fake, idx, 4, C.byref(sc), out, None, 1.0, 0, None, None,
                                        fake + 64, 8, idx, 0) == hb.E_INVAL                # n_off = 0
    assert "iqlhip_online_step" in hb.last_error()
    assert lib.iqlhip_online_step_mixed(fake, fake, 44, 8, 0, fake, idx, 4, C.byref(sc), out, None, 1.0, 0, None, None,
                                        fake, 8, idx, 4) == hb.E_INVAL                     # the same rows twice
    assert lib.iqlhip_train_steps_mixed(None, fake, 8, fake + 64, 8, 44, 8, 3, C.byref(sc), 1, 0, 0, None) == hb.E_INVAL
    assert lib.iqlhip_train_steps_mixed(fake, fake, 8, fake + 64, 8, 44, 8, 3, None, 1, 0, 0, None) == hb.E_INVAL
    assert lib.iqlhip_train_steps_mixed_prepare(None, fake, fake + 64, 44, 8, 3, 0.125, None) == hb.E_INVAL
