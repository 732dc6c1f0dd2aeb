"""GPU tests of the five chunk-graph kinds of train_steps — plain, mixed, weighted, weighted with importance-sampling
weights, prioritised — over the shape table tests/chunk_kind_shapes.py: every instantiation of every kind's training
forward (layer-0 staging by LDS-DMA or not, one or several column slices per block, fp32 or bf16) and every row stride at
which a gather's loop over a row or the forward's row-tile registers change ("Chunk-graph kinds x shapes").

Each case builds two trainers from the same parameters.  One makes the burst calls; the other runs the kind's eager twin
(tests/burst_twins.py; hip_helpers.eager_segment for the plain kind): eager train() steps on the same rows, drawn by a CPU
or device reference, with no graph, no rows staged ahead and no continuation.  Everything is compared bitwise — the loss
triple of every step, parameters, targets, Adam moments and counters, for the prioritised kind the table's leaves and
total — so there is no tolerance here; what ties the eager step to the float64 oracle at these shapes are the edge lists
of tests/test_hip_parity.py, tests/test_hip_bf16_edges.py and tests/test_hip_score.py.

Calls of 7, 3, 2 and 2 steps (chunk_kind_shapes.CALLS): a direct head and two chunk graphs, so that the set-up kernel's
gather and the idle blocks' gathers both feed steps; a second call; and a call behind an even one, which starts on the
rows that one's last forward staged."""
import functools

import numpy as np
import pytest
import torch

import burst_twins as TW
import chunk_kind_shapes as T
import synth
from helpers import fwd_instantiation

pytestmark = pytest.mark.gpu

HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
SEED = 9
IS_BETA = 0.4
PRIO = {"alpha": 0.6, "eps": 1e-3, "is_beta": 0.5}
MAX_WEIGHT = 64.0


def _cases(kind):
    return pytest.mark.parametrize("case", [c for c in T.CASES if c[0] == kind], ids=T.case_id)


@functools.lru_cache(maxsize=None)
def _params(S, A, gaussian):
    return synth.synth_params(S, A, seed=21, gaussian=gaussian)


@functools.lru_cache(maxsize=None)
def _rows(S, A, n, seed):
    return synth.synth_transitions(n, S, A, seed=seed)


def _buffer(S, A, n=T.N_ROWS, seed=22, capacity=None):
    import iql
    buf = iql.ReplayBuffer(S, A, capacity or n, "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in _rows(S, A, n, seed).items()})
    return buf


def _pair(case):
    """The burst trainer and its eager twin; asserts the forward the table says this case runs, on this device."""
    from hip_helpers import build_hip_trainer
    kind, S, A, gaussian, B, precision = case
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert fwd_instantiation(kind, S, A, B, precision, n_cus) == T.instantiation(case), \
        f"{n_cus} CUs: this device takes {fwd_instantiation(kind, S, A, B, precision, n_cus)}, the table counts on {T.instantiation(case)}"
    out = []
    for _ in range(2):
        tr = build_hip_trainer(_params(S, A, gaussian), S, A, gaussian, dict(HYPER), dict(LRS), 1000)
        if precision == "bf16":
            tr.set_precision("bf16")
        out.append(tr)
    return out


def _run(case, burst_call, eager_call, after_each=None):
    """The calls of T.CALLS on both trainers.  burst_call(tr, K) / eager_call(tr, K) -> losses [K, 3]."""
    from hip_helpers import assert_same_trainer_state
    what = f"{T.case_id(case)} [{T.instantiation(case)}]"
    g, e = _pair(case)
    seen = []
    for n, K in enumerate(T.CALLS):
        lg = burst_call(g, K)
        le = eager_call(e, K)
        assert lg.dtype == np.float32 and lg.shape == le.shape == (K, 3) and np.all(np.isfinite(lg)), (what, n)
        bad = np.nonzero(np.any(lg != le, axis=1))[0]
        assert bad.size == 0, f"{what}: call {n} ({K} steps): steps {bad.tolist()} differ from the eager twin: " \
                              f"{lg[bad[0]]} vs {le[bad[0]]}"
        assert_same_trainer_state(g, e, f"{what}: after call {n}")
        if after_each:
            after_each(f"{what}: after call {n}")
        seen += [tuple(r) for r in lg]
    assert g.total_it == e.total_it == sum(T.CALLS)
    assert len(set(seen)) == len(seen), what                   # every step trained on another batch


@_cases("plain")
def test_plain(case):
    from hip_helpers import eager_segment
    _, S, A, _, B, _ = case
    buf = _buffer(S, A)
    _run(case, lambda tr, K: tr.train_steps(buf, K, B, seed=SEED), lambda tr, K: eager_segment(tr, buf, K, B, SEED))


@_cases("mixed")
def test_mixed(case):
    _, S, A, _, B, _ = case
    off, on = _buffer(S, A), _buffer(S, A, n=T.N_ONLINE, seed=24, capacity=T.ONLINE_CAPACITY)
    n_off = T.n_off_of(B)
    ratio = TW.mixing_ratio(B, n_off)
    _run(case, lambda tr, K: tr.train_steps_mixed(off, on, K, B, ratio, seed=SEED),
         lambda tr, K: TW.eager_mixed_segment(tr, off, on, K, B, n_off, SEED))


@_cases("weighted")
def test_weighted(case):
    _, S, A, _, B, _ = case
    buf, w = _buffer(S, A), TW.skewed_weights(T.N_ROWS)
    assert np.sum(w == 0) > 100
    buf.set_sample_weights(w)
    _run(case, lambda tr, K: tr.train_steps_weighted(buf, K, B, seed=SEED),
         lambda tr, K: TW.eager_weighted_segment(tr, buf, w, K, B, SEED))


@_cases("weighted_is")
def test_weighted_is(case):
    _, S, A, _, B, _ = case
    buf = _buffer(S, A)
    buf.set_sample_weights(TW.fourth_power_weights(T.N_ROWS))
    _run(case, lambda tr, K: tr.train_steps_weighted(buf, K, B, seed=SEED, is_beta=IS_BETA),
         lambda tr, K: TW.eager_is_segment(tr, buf, K, B, SEED, IS_BETA))


@_cases("prioritized")
def test_prioritized(case):
    """Every call's step 0 is a fresh draw from the table as the call before left it, in the burst and in the eager lag
    loop alike; the two tables (one per trainer: both are written) are compared after every call."""
    _, S, A, _, B, _ = case
    bufs = [_buffer(S, A) for _ in range(2)]
    for b in bufs:
        b.set_sample_weights(TW.fourth_power_weights(T.N_ROWS), updatable=True, max_weight=MAX_WEIGHT)
    q0, _ = TW.table_of(bufs[0])

    def same_table(what):
        (qb, tb), (qe, te) = TW.table_of(bufs[0]), TW.table_of(bufs[1])
        assert np.array_equal(qb, qe), (what, int(np.sum(qb != qe)))
        assert tb == te == int(np.sum(qb.astype(object))), what
        assert bufs[0].sample_weights_flags() == 0 and bufs[1].sample_weights_flags() == 0, what
        assert np.any(qb != q0), what                          # (priorities were written)

    _run(case, lambda tr, K: tr.train_steps_prioritized(bufs[0], K, B, seed=SEED, **PRIO),
         lambda tr, K: TW.eager_prioritized_segment(tr, bufs[1], K, B, SEED, PRIO["alpha"], PRIO["eps"], PRIO["is_beta"]),
         after_each=same_table)
