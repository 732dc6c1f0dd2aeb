"""CPU-only tests of actor dropout inside policy inference (ImplicitQLearning.set_act_dropout / iqlhip_set_act_dropout):
the new symbols are declared, exported and bound; the opt-in changes nothing for a CPU trainer; and the numpy
reference of the inference keep-bit stream (tests/act_dropout_ref.py) has distinct counters, differs from the training
stream and keeps the right fraction of units."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import iql
import iqlhip_binding as hb
from act_dropout_ref import TAG_ACT_DROP, act_keep_counters, act_keep_words, keep_scale
from oracle import philox_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"iqlhip_set_act_dropout": 3, "iqlhip_get_act_dropout_counter": 2, "iqlhip_set_act_dropout_counter": 2}


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
    # the binding's constants still match the header; the feature adds no group-creation flag
    for const in ("IQLHIP_ACT_ROWS", "IQLHIP_MAX_GROUP", "IQLHIP_GROUP_DROPOUT", "IQLHIP_GROUP_ACT_WAIT",
                  "IQLHIP_GROUP_MAX_STEPS", "IQLHIP_HIDDEN"):
        m = re.search(r"#define\s+" + const + r"\s+(\d+)", header)
        assert m and int(m.group(1)) == getattr(hb, const), const
    assert re.findall(r"#define\s+(IQLHIP_GROUP_[A-Z]+)\s+\d+\s", header).count("IQLHIP_GROUP_DROPOUT") == 1
    assert "0x41445250" in header and TAG_ACT_DROP == 0x41445250 == int.from_bytes(b"ADRP", "big")
    assert '"act_drop_bits"' in header


def test_new_symbols_reject_null_and_bad_rates_without_a_gpu():
    lib = hb.lib()
    n = C.c_uint64(7)
    assert lib.iqlhip_set_act_dropout(None, 0.1, 1) == hb.E_INVAL
    assert lib.iqlhip_get_act_dropout_counter(None, C.byref(n)) == hb.E_INVAL
    assert lib.iqlhip_set_act_dropout_counter(None, 3) == hb.E_INVAL
    assert n.value == 7


def _cpu_trainer(S=17, A=6, dropout=0.1):
    actor = iql.GaussianPolicy(S, A, 1.0, dropout=dropout)
    qf, vf = iql.TwinQ(S, A), iql.ValueFunction(S)
    return iql.ImplicitQLearning(max_action=1.0, actor=actor,
                                 actor_optimizer=torch.optim.Adam(actor.parameters(), lr=3e-4),
                                 q_network=qf, q_optimizer=torch.optim.Adam(qf.parameters(), lr=3e-4),
                                 v_network=vf, v_optimizer=torch.optim.Adam(vf.parameters(), lr=3e-4),
                                 max_steps=1000, device="cpu")


def test_set_act_dropout_on_a_cpu_trainer_leaves_act_on_the_pytorch_path():
    from iqlhip_networks import _hip_owner
    tr = _cpu_trainer()
    tr.set_act_dropout(True)
    assert tr._act_dropout is True and tr.acts_with_dropout()
    assert _hip_owner(tr.actor, "cpu") is None
    state = np.linspace(-1.0, 1.0, 17).astype(np.float32)
    torch.manual_seed(3)
    a = tr.actor.act(state, "cpu")
    torch.manual_seed(3)
    b = tr.actor.act(state, "cpu")                   # the PyTorch modules: torch's generator decides the masks
    assert a.shape == (6,) and np.array_equal(a, b)
    tr.actor.eval()
    assert not tr.acts_with_dropout()
    with pytest.raises(RuntimeError, match="GPU"):
        tr.actor_forward(torch.zeros(2, 17))
    with pytest.raises(RuntimeError, match="GPU"):
        tr.act_dropout_calls()
    tr.set_act_dropout(False)
    assert tr._act_dropout is False


# ---------------------------------------------------------------------------------------------------- the reference
def test_reference_counters_are_distinct():
    """Distinct (n, row, layer, q, block) give distinct counter words; distinct seeds are distinct keys."""
    seen = set()
    for n in (0, 1, (1 << 32) + 5, (1 << 32)):
        c0, c1, c2, c3 = np.broadcast_arrays(*act_keep_counters(n, 40))
        tup = np.stack([c0, c1, c2, c3], axis=-1).reshape(-1, 4)
        rows = {tuple(int(x) for x in r) for r in tup}
        assert len(rows) == tup.shape[0] == 2 * 40 * 8 * 8
        assert not (rows & seen)
        seen |= rows
    assert all(c[0] < 40 * 16 and (c[1] & ~7) == TAG_ACT_DROP for c in seen)
    a = act_keep_words(0x8000000100000002, 3, 0.5, 4)
    assert not np.array_equal(a, act_keep_words(0x8000000100000003, 3, 0.5, 4))       # low key word
    assert not np.array_equal(a, act_keep_words(0x8000000000000002, 3, 0.5, 4))       # high key word
    assert not np.array_equal(a, act_keep_words(0x8000000100000002, 3 + (1 << 32), 0.5, 4))   # high position word
    # the word number does not depend on how many rows the call has
    assert np.array_equal(act_keep_words(9, 2, 0.1, 50)[:, :7], act_keep_words(9, 2, 0.1, 7))


def test_reference_words_match_the_scalar_generator():
    seed, n, p = 0xF00DFACE12345678, (1 << 32) + 5, 0.1
    words = act_keep_words(seed, n, p, 3)
    thresh = R.dropout_threshold(p)
    for layer, row, q in ((0, 0, 0), (1, 2, 7), (1, 0, 3), (0, 2, 5)):
        word = 0
        for j in range(8):
            o = R.philox4x32_10_scalar(row * 16 + layer * 8 + q, j | TAG_ACT_DROP, n & 0xFFFFFFFF, n >> 32,
                                       seed & 0xFFFFFFFF, seed >> 32)
            for t in range(4):
                word |= int(o[t] >= thresh) << (4 * j + t)
        assert int(words[layer, row, q]) == word, (layer, row, q)


def test_reference_differs_from_the_training_stream():
    for seed, pos in ((5, 0), (0xF00DFACE12345678, 11)):
        a = act_keep_words(seed, pos, 0.5, 64)
        for mb in (64, 256):
            t = R.dropout_keep_words(seed, pos, 0.5, mb, 64)
            assert a.shape == t.shape and not np.array_equal(a, t)
            assert (a != t).mean() > 0.99            # (32-bit words of independent fair bits)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_reference_kept_fraction(p):
    """4096 rows x 2 layers x 256 units Bernoulli(1 - float32(p)) bits: the kept fraction within 5 binomial standard
    deviations."""
    words = act_keep_words(1234, 7, p, 4096)
    k0, k1 = R.keep_masks(words)
    n = k0.size + k1.size
    keep = 1.0 - float(np.float32(p))
    got = (k0.sum() + k1.sum()) / n
    sd = np.sqrt(keep * (1.0 - keep) / n)
    assert abs(got - keep) <= 5 * sd, (got, keep, sd)
    assert keep_scale(p).dtype == np.float32 and keep_scale(p) == np.float32(1.0) / (np.float32(1.0) - np.float32(p))
