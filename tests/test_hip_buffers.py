"""GPU tests of buffer ownership in the host library (DESIGN.md "Buffer ownership"): every device buffer, pinned buffer
and event of a context or a trainer group belongs to its one owner, and iqlhip_debug_live_buffers() counts what the
owners of this process hold.  All assertions are on differences of that count — exact integers, no tolerance: a
destroy gives back everything its create and its opt-in features took, enabling a feature twice or toggling it takes
nothing more, a context re-created for a larger batch leaves nothing of the old one behind, and a group's calls
allocate once.

The smallest golden shape (S = 17, A = 6, deterministic policy), max_batch 256, batches of 10 rows.  Nothing here calls
ReplayBuffer.sample(), whose process-wide index staging is counted too."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import synth
from helpers import step_batch

pytestmark = pytest.mark.gpu

S, A, B = 17, 6, 10
HYPER = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
LRS = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
P_DROP = 0.1


def _hip():
    import hip_helpers as hh
    import iql
    import iqlhip_binding as hb
    return iql, hb, hh


def _live():
    """Buffers and events held right now (trainers an earlier test dropped are collected first)."""
    gc.collect()
    return int(_hip()[1].lib().iqlhip_debug_live_buffers())


def _trainer(seed=0, features=True):
    """A trainer (context of 256 rows); features: bf16, step statistics, gradient clipping, training and inference
    dropout — each reaches the library with the first call that uses it."""
    _, _, hh = _hip()
    tr = hh.build_hip_trainer(synth.synth_params(S, A, seed=40 + seed, gaussian=False), S, A, False, HYPER, LRS, 1000,
                              dropout=P_DROP)
    tr.set_dropout_seed(5 + seed)
    if features:
        tr.set_precision("bf16")
        tr.set_step_stats(True)
        tr.set_grad_clip(1.0)
        tr.set_act_dropout(True)
    return tr


def _batch(rows, seed=0):
    return _hip()[2].to_torch_batch(step_batch(S, A, rows, seed=900 + seed))


def _buffer(n=64, seed=3):
    iql = _hip()[0]
    buf = iql.ReplayBuffer(S, A, n, "cuda")
    buf.load_d4rl_dataset({k: v.copy() for k, v in synth.synth_transitions(n, S, A, seed=seed).items()})
    return buf


def _infer(tr):
    states = torch.from_numpy(synth.synth_transitions(4, S, A, seed=8)["observations"]).to("cuda")
    return tr.actor_forward(states)


def test_destroy_returns_what_create_and_every_feature_took():
    buf, tb = _buffer(), _batch(B)
    base = _live()
    tr = _trainer()
    created = _live()
    assert created > base
    log = tr.train(tb)
    assert len(log) == 19 and tr.last_grad_clip()["coef_vf"] <= 1.0          # statistics and clipping did run
    losses = tr.train_steps(buf, 3, B, seed=1)
    assert losses.shape == (3, 3) and np.all(np.isfinite(losses))
    assert _infer(tr).shape == (4, A) and tr.act_dropout_calls() == 1        # inference with keep-bits drawn
    used = _live()
    print("buffers and events: context", created - base, "with every feature and train_steps' arena copy", used - base)
    assert used > created                                                    # the features allocated on first use
    tr._release()
    assert _live() == base


def test_enabling_twice_and_toggling_allocates_nothing():
    _, hb, _ = _hip()
    lib = hb.lib()
    base = _live()
    tr = _trainer()
    tr.train(_batch(B))
    _infer(tr)
    ctx, on = tr._ctx, _live()
    lim, none = (C.c_float * 3)(1.0, 1.0, 1.0), (C.c_float * 3)(0.0, 0.0, 0.0)

    def enable():
        hb.check(lib.iqlhip_set_precision(ctx, 1))
        hb.check(lib.iqlhip_set_step_stats(ctx, 1))
        hb.check(lib.iqlhip_set_grad_clip(ctx, lim))
        hb.check(lib.iqlhip_set_dropout(ctx, P_DROP, 7))
        hb.check(lib.iqlhip_set_act_dropout(ctx, P_DROP, 7))

    enable()                                       # a second time
    assert _live() == on
    hb.check(lib.iqlhip_set_precision(ctx, 0))     # off ...
    hb.check(lib.iqlhip_set_step_stats(ctx, 0))
    hb.check(lib.iqlhip_set_grad_clip(ctx, none))
    hb.check(lib.iqlhip_set_dropout(ctx, 0.0, 7))
    hb.check(lib.iqlhip_set_act_dropout(ctx, 0.0, 7))
    assert _live() == on
    enable()                                       # ... and on again
    assert _live() == on
    tr._release()
    assert _live() == base


def test_a_context_recreated_for_a_larger_batch_leaves_nothing_behind():
    base = _live()
    grown = _trainer(1)
    grown.train(_batch(B))
    _infer(grown)
    assert grown._max_batch == 256
    old_ctx = grown._ctx.value
    grown.train(_batch(512, 1))                    # 256 -> 512 rows: the shim destroys the context and creates another
    assert grown._max_batch == 512 and grown._ctx.value != old_ctx
    _infer(grown)
    held_grown = _live() - base
    grown._release()
    assert _live() == base
    fresh = _trainer(1)
    fresh.reserve_batch(512)
    fresh.train(_batch(512, 1))
    _infer(fresh)
    held_fresh = _live() - base
    print("buffers and events at 512 rows: grown", held_grown, "fresh", held_fresh)
    assert held_grown == held_fresh
    fresh._release()
    assert _live() == base


def test_a_groups_calls_allocate_once_and_its_destroy_returns_it_all():
    iql, _, _ = _hip()
    members = [_trainer(10 + i, features=False) for i in range(2)]
    members[0].set_step_stats(True)
    members[0].set_grad_clip(1.0)
    for i, t in enumerate(members):                # the members' own lazy allocations happen here, not in the group calls
        t.train(_batch(B, 20 + i))
    buf = _buffer()
    rings = [iql.ReplayBuffer(S, A, 32, "cuda") for _ in range(2)]
    stream = synth.synth_transitions(4, S, A, seed=70, antmaze_rewards=True)
    base = _live()
    group = iql.ImplicitQLearningGroup(members, actor_dropout=True)

    def round_of_calls(it):
        logs = group.train([_batch(B, 30 + i) for i in range(2)])
        assert [len(x) for x in logs] == [19, 3]   # statistics for member 0 only
        group.train_steps(buf, 2, B, [7, 8])
        tr_ = (stream["observations"][it], stream["actions"][it], float(stream["rewards"][it]),
               stream["next_observations"][it], bool(stream["terminals"][it]))
        np.random.seed(it)
        logs = group.online_step(rings, *[[x, x] for x in tr_], B)
        assert [len(x) for x in logs] == [19, 3]

    round_of_calls(0)
    held = _live()
    assert held > base
    round_of_calls(1)
    assert _live() == held
    group._release()
    assert _live() == base
    for t in members:
        t._release()
