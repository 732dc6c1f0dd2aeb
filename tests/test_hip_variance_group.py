"""GPU tests of variance-learner groups (iqlhip_var_group; VarianceLearnerGroup; DESIGN.md 6l "Groups of learners").
No tolerance anywhere: the solo learner is pinned to the reference by tests/test_hip_variance*.py, and every assertion
here is bit for bit against solo twins — learners built from the same seeds and stepped by the solo calls on the same
data.  Shapes are the smallest at which the record indexing can go wrong: K = 1, 2, 3 and 16 (more than one label group),
B on both sides of a 32-row tile on both nets (mf runs on B + 1 rows), S = 3, 17, 65."""
import os

import numpy as np
import pytest
import torch

import variance_cases as VC
import variance_ref as R
import variance_window_ref as W

pytestmark = pytest.mark.gpu

_NAMES = {f"{k}{i}": f"v.net.{2 * i}.{n}" for i in range(3) for n, k in (("weight", "w"), ("bias", "b"))}
CFG = type("Cfg", (), {"device": "cuda", "variance_learn_frac": 0.5})()


def _load(L, mf, vf):
    for net, P in ((L.mf, mf), (L.vf, vf)):
        net.load_state_dict({n: torch.from_numpy(P[k].copy()) for k, n in _NAMES.items()})
    return L


def _learner(S, A, B, seed=1, aligned=False, config=None):
    import variance_learner as VL
    L = VL.VarianceLearner(S, A, config, None, batch_size=B, device="cuda", aligned_rewards=aligned)
    return _load(L, R.synth_net(S, 2 * seed + 1), R.synth_net(S, 2 * seed + 2))


def _pair(K, S, A, B, **kw):
    """K group members and their K solo twins: member i from seed i + 1."""
    return [_learner(S, A, B, seed=i + 1, **kw) for i in range(K)], [_learner(S, A, B, seed=i + 1, **kw) for i in range(K)]


def _buffer(rows, S, A):
    import iql
    buf = iql.ReplayBuffer(S, A, 4, "cuda")
    t = torch.from_numpy(rows).cuda()
    buf._rows, buf._rows_ptr, buf._ld = t, t.data_ptr(), t.shape[1]
    buf._buffer_size = buf._size = t.shape[0]
    buf._pointer = 0
    return buf


def _make(S, A, n, seed=0):
    rows = W.synthetic_rows(n, S, A, seed)
    return rows, _buffer(rows, S, A)


def _state(L):
    torch.cuda.synchronize()
    return [a.cpu().numpy().view(np.uint32).copy() for a in (L._params_arena, L._m_arena, L._v_arena)], list(L._adam_t)


def _same(a, b):
    return a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))


def _segment(state, L, k):
    lo, hi = int(L._layout[k].seg_begin), int(L._layout[k].seg_end)
    return [x[lo:hi] for x in state[0]]


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x).view(np.uint32)


def _same_log(a, b):
    assert set(a) == set(b) and np.float32(a["value_loss"]).view(np.uint32) == np.float32(b["value_loss"]).view(np.uint32)
    for key in ("values_samp_vec", "values_pred_vec", "variance_pred_vec"):
        assert np.array_equal(_bits(a[key]), _bits(b[key])), key


def _opt_steps(L):
    return [sorted(float(st["step"]) for st in opt.state.values()) for opt in (L.m_optimizer, L.mv_optimizer)]


# ------------------------------------------------------------------------------------------------ 1. the eager step
@pytest.mark.parametrize("S", [3, 17, 65])
@pytest.mark.parametrize("B", [1, 31, 33, 257])
@pytest.mark.parametrize("K", [1, 2, 3, 16])
def test_group_update_is_update_v_of_every_member(K, B, S):
    import variance_learner as VL
    A = 2
    members, twins = _pair(K, S, A, B)
    group = VL.VarianceLearnerGroup(members)
    rows = W.synthetic_rows(B + 2 * K + 2, S, A, seed=100 * K + B + S)
    for step, uv in enumerate((False, True, False)):             # mf, vf, mf again: moments and step counts carry over
        batches = [W.window_tensors(rows, 2 * i + step, B, S, A) for i in range(K)]      # every member its own rollout
        before = [_state(L) for L in members]
        logs = group.update(batches, uv)
        assert len(logs) == K
        for i in range(K):
            _same_log(logs[i], twins[i]._update_v(batches[i], uv))
            after = _state(members[i])
            assert _same(after, _state(twins[i])), (i, uv)
            other = 0 if uv else 1
            for x, y in zip(_segment(after, members[i], other), _segment(before[i], members[i], other)):
                assert np.array_equal(x, y), "the net that was not stepped changed"
            assert not np.array_equal(_segment(after, members[i], 1 - other)[0], _segment(before[i], members[i], 1 - other)[0])
            assert _opt_steps(members[i]) == _opt_steps(twins[i])
    assert all(L._adam_t == [2, 1] for L in members)
    if K > 1:      # different parameters and data: the members' results differ
        assert not np.array_equal(_state(members[0])[0][0], _state(members[1])[0][0])
    # get_values, for every member at once
    batches = [W.window_tensors(rows, 2 * i + 1, B, S, A) for i in range(K)]
    got = group.get_values([(b[0], b[2], b[4], b[3], b[5]) for b in batches])
    for i in range(K):
        want = twins[i].get_values(batches[i][0], batches[i][2], batches[i][4], None, batches[i][5])
        assert all(np.array_equal(_bits(x), _bits(y)) and x.shape == (B,) for x, y in zip(got[i], want))


# ------------------------------------------------------------------------------------------------ 2. no leakage
def _case_batch(c):
    B, S = c["B"], c["S"]
    nxt = np.zeros((B, S), np.float32)
    nxt[B - 1] = c["last"]
    return (c["obs"], [None] * B, c["rewards"], [False] * B, nxt, c["nd"].astype(np.float32))


@pytest.mark.parametrize("uv", [False, True])
def test_members_do_not_leak_into_each_other(uv):
    """Member 1's rollout is all-terminal, member 2's vf is clipped low and high (tests/variance_cases.py, with its
    trained-like nets); member 0 is an ordinary one.  Each equals its twin; swapping two members swaps the results."""
    import variance_learner as VL
    S, A, B = 16, 2, 16
    cases = [None, VC.case("S16_B16_mixed_alldone"), VC.make_case(S, B, 3016, "closed")]
    assert cases[1]["nd"].all() and set(cases[2]["targets"].tolist()) == {VC.LO, VC.HI, VC.INF}
    rows = W.synthetic_rows(B + 4, S, A, seed=41)
    batches = [W.window_tensors(rows, 1, B, S, A)] + [_case_batch(c) for c in cases[1:]]

    def build():
        Ls = [_learner(S, A, B, seed=1)]
        Ls += [_load(_learner(S, A, B), c["mf"], c["vf"]) for c in cases[1:]]
        return Ls

    members, twins, swapped = build(), build(), build()
    logs = VL.VarianceLearnerGroup(members).update(batches, uv)
    want = [t._update_v(b, uv) for t, b in zip(twins, batches)]
    for i in range(3):
        _same_log(logs[i], want[i])
        assert _same(_state(members[i]), _state(twins[i])), i
    # the clipped member's variances sit on the clip bounds, the terminal member's samples are its rewards
    var = logs[2]["variance_pred_vec"].numpy()
    assert set(np.unique(var).tolist()) <= {np.float32(1e-4), np.float32(1e8)}
    assert np.array_equal(logs[1]["values_samp_vec"].numpy(), np.roll(cases[1]["rewards"], 1)[:5])
    # positions 0 and 2 exchanged: the same learners and data in another order
    order = [2, 1, 0]
    logs2 = VL.VarianceLearnerGroup([swapped[j] for j in order]).update([batches[j] for j in order], uv)
    for pos, j in enumerate(order):
        _same_log(logs2[pos], want[j])
        assert _same(_state(swapped[j]), _state(twins[j])), j


# ------------------------------------------------------------------------------------------------ 3. windows
@pytest.mark.parametrize("shared", [True, False])
def test_window_calls_equal_the_solo_calls(shared):
    import variance_learner as VL
    K, S, A, B = 3, 17, 6, 33
    members, twins = _pair(K, S, A, B)
    group = VL.VarianceLearnerGroup(members)
    if shared:
        bufs = [_make(S, A, 200, seed=5)[1]] * K
        arg = bufs[0]
    else:
        bufs = [_make(S, A, n, seed=6 + i)[1] for i, n in enumerate((B, 150, 90))]      # (a buffer of exactly B rows)
        arg = bufs
    # every member at row 0, at its buffer's last window (size - B), and somewhere in between
    sets =[[0] * K, [b._size - B for b in bufs], [min(7 + i, b._size - B) for i, b in enumerate(bufs)]]
    for step, starts in enumerate(sets):
        uv = bool(step & 1)
        got = group.get_values_window(arg, starts)
        logs = group.update_from_buffer(arg, starts, uv)
        for i in range(K):
            want = twins[i].get_values_window(bufs[i], starts[i])
            assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(got[i], want)), (i, starts)
            _same_log(logs[i], twins[i].update_from_buffer(bufs[i], starts[i], uv))
            assert _same(_state(members[i]), _state(twins[i])), (i, starts)
    # one start for all members
    logs = group.update_from_buffer(arg, 0, True)
    for i in range(K):
        _same_log(logs[i], twins[i].update_from_buffer(bufs[i], 0, True))
        assert _same(_state(members[i]), _state(twins[i]))


# ------------------------------------------------------------------------------------------------ 4. bursts
def _burst_setup():
    import iql
    S, A, B, ep, E = 17, 3, 8, 40, 12
    rows = W.synthetic_rows(ep * E, S, A, seed=8, p_done=0.0)
    data = {"observations": rows[:, :S], "actions": rows[:, S:S + A], "next_observations": rows[:, S + A:2 * S + A],
            "rewards": rows[:, 2 * S + A], "terminals": (np.arange(ep * E) % ep == ep - 1).astype(np.float32)}
    buf = iql.ReplayBuffer(S, A, ep * E + 7, "cuda")
    buf.load_d4rl_dataset(data)
    first = buf.episode_returns(max_episode_steps=1000).episode_table()[0]
    other = _make(S, A, 300, seed=9)[1]
    return S, A, B, [buf, other, buf], [first, None, np.array([5, 400, 17], dtype=np.int64)]


def _solo_bursts(twins, bufs, n, seeds, offsets, uv, lists):
    return [t.train_on_buffer(b, n, s, o, uv, st) for t, b, s, o, st in zip(twins, bufs, seeds, offsets, lists)]


def _same_burst(out, want):
    K = len(want)
    assert out["losses"].dtype == np.float32 and out["starts"].dtype == np.int64 and out["losses"].shape[0] == K
    for i in range(K):
        assert np.array_equal(out["starts"][i], want[i]["starts"]), i
        assert np.array_equal(out["losses"][i].view(np.uint32), want[i]["losses"].view(np.uint32)), i


@pytest.mark.parametrize("uv", [False, True])
def test_group_burst_equals_the_solo_bursts(uv):
    import variance_learner as VL
    S, A, B, bufs, lists = _burst_setup()
    K, seeds, offsets = 3, [11, 12, 11], [0, 5, 2]                       # (an odd offset; two members share a seed)
    members, twins = _pair(K, S, A, B)
    split, _ = _pair(K, S, A, B)
    out = VL.VarianceLearnerGroup(members).train_on_buffer(bufs, 7, seeds, offsets, uv, lists)
    want = _solo_bursts(twins, bufs, 7, seeds, offsets, uv, lists)
    _same_burst(out, want)
    assert out["losses"].shape == (K, 7) and np.isfinite(out["losses"]).all()
    assert (out["starts"][0] % 40 == 0).all() and set(out["starts"][2].tolist()) <= {5, 400, 17}
    assert np.array_equal(out["starts"][1], W.burst_starts(7, 300, B, 12, offset=5))
    for i in range(K):
        assert _same(_state(members[i]), _state(twins[i])) and members[i]._adam_t == ([0, 7] if uv else [7, 0])
        assert _opt_steps(members[i]) == _opt_steps(twins[i])
    # 3 + 4 updates are the 7
    g2 = VL.VarianceLearnerGroup(split)
    parts = [g2.train_on_buffer(bufs, 3, seeds, offsets, uv, lists),
             g2.train_on_buffer(bufs, 4, seeds, [o + 3 for o in offsets], uv, lists)]
    for key in ("losses", "starts"):
        assert np.array_equal(np.concatenate([p[key] for p in parts], axis=1), out[key]), key
    assert all(_same(_state(a), _state(b)) for a, b in zip(split, members))


def test_scalar_seed_offset_and_one_list_for_all():
    import variance_learner as VL
    S, A, B, bufs, lists = _burst_setup()
    members, twins = _pair(2, S, A, B)
    lst = lists[2]
    out = VL.VarianceLearnerGroup(members).train_on_buffer(bufs[0], 5, 21, 3, False, lst)
    _same_burst(out, _solo_bursts(twins, [bufs[0]] * 2, 5, [21] * 2, [3] * 2, False, [lst] * 2))
    assert np.array_equal(out["starts"][0], out["starts"][1]) and not np.array_equal(out["losses"][0], out["losses"][1])
    assert all(_same(_state(a), _state(b)) for a, b in zip(members, twins))


def test_burst_longer_than_the_ring_is_split():
    import variance_learner as VL
    S, A, B, bufs, lists = _burst_setup()
    K, n, seeds, offsets = 3, VL.TRAIN_MAX_STEPS + 6, [3, 4, 5], [1, 0, 7]
    assert n == 1030
    members, twins = _pair(K, S, A, B)
    out = VL.VarianceLearnerGroup(members).train_on_buffer(bufs, n, seeds, offsets, False, lists)
    _same_burst(out, _solo_bursts(twins, bufs, n, seeds, offsets, False, lists))
    assert out["losses"].shape == (K, n) and np.isfinite(out["losses"]).all()
    for a, b in zip(members, twins):
        assert _same(_state(a), _state(b)) and a._adam_t == [n, 0]


# ------------------------------------------------------------------------------------------------ 5. interleaving
def test_solo_and_group_calls_interleave():
    import variance_learner as VL
    S, A, B, bufs, lists = _burst_setup()
    K = 3
    members, twins = _pair(K, S, A, B)
    group = VL.VarianceLearnerGroup(members)
    starts = [3, 100, 50]
    a1 = group.update_from_buffer(bufs, starts, False)
    solo = members[0].update_from_buffer(bufs[0], 9, False)                     # member 0 alone, between two group calls
    solo_burst = members[2].train_on_buffer(bufs[2], 2, 77)
    a2 = group.update_from_buffer(bufs, starts, False)
    a3 = group.train_on_buffer(bufs, 3, [1, 2, 3])
    for i in range(K):
        _same_log(a1[i], twins[i].update_from_buffer(bufs[i], starts[i], False))
    _same_log(solo, twins[0].update_from_buffer(bufs[0], 9, False))
    want_burst = twins[2].train_on_buffer(bufs[2], 2, 77)
    assert np.array_equal(solo_burst["losses"].view(np.uint32), want_burst["losses"].view(np.uint32))
    for i in range(K):
        _same_log(a2[i], twins[i].update_from_buffer(bufs[i], starts[i], False))
    _same_burst(a3, _solo_bursts(twins, bufs, 3, [1, 2, 3], [0] * K, False, [None] * K))
    assert [L._adam_t for L in members] == [[6, 0], [5, 0], [7, 0]]
    assert all(_same(_state(a), _state(b)) for a, b in zip(members, twins))
    # a member that re-attaches (new arenas, a new library handle): the group rebuilds its records
    handle = group._members[1]
    members[1]._release()
    members[1]._attach()
    twins[1]._release()
    twins[1]._attach()
    a4 = group.update_from_buffer(bufs, starts, True)
    assert group._members[1] != handle or group._members[1] == int(members[1]._h.value)
    for i in range(K):
        _same_log(a4[i], twins[i].update_from_buffer(bufs[i], starts[i], True))
        assert _same(_state(members[i]), _state(twins[i]))


# ------------------------------------------------------------------------------------------------ 6. the training loop
def test_run_training_on_buffer_and_gates(tmp_path):
    import iql
    import synth
    import variance_learner as VL
    from hip_helpers import build_hip_trainer
    S, A, B = 5, 2, 16
    _, buf = _make(S, A, 300, seed=9)
    members, twins = _pair(2, S, A, B, config=CFG)
    group = VL.VarianceLearnerGroup(members)
    gdir, sdir = tmp_path / "group", tmp_path / "solo"
    vfs = group.run_training_on_buffer(buf, n_updates=6, seeds=[13, 14], env_names=["EnvA", "EnvB"], save_dir=str(gdir))
    want = [t.run_training_on_buffer(buf, n_updates=6, seed=s, save_dir=str(sdir), env_name=n)
            for t, s, n in zip(twins, (13, 14), ("EnvA", "EnvB"))]
    assert sorted(os.listdir(gdir)) == sorted(os.listdir(sdir)) == sorted(
        f"{n}_None_6_0-5_{k}.pt" for n in ("EnvA", "EnvB") for k in ("vf", "mf"))
    for i in range(2):
        assert vfs[i] is members[i].vf and not vfs[i].training and not hasattr(members[i], "mf")
        assert members[i]._adam_t == [4, 2] and _same(_state(members[i]), _state(twins[i]))
        for key in ("losses", "starts"):
            assert np.array_equal(members[i].buffer_log[key], twins[i].buffer_log[key])
        assert np.array_equal(members[i].buffer_log["starts"], W.burst_starts(6, 300, B, 13 + i))
    for name in os.listdir(gdir):
        a, b = torch.load(str(gdir / name)), torch.load(str(sdir / name))
        f = VL.StateDepFunction(S)
        f.load_state_dict(a)                                            # the reference's module shape
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) and a[k].device.type == "cpu" for k in a), name
    # the gates, in member order, in front of K (learner, guide) pairs
    hyper = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    learners = [build_hip_trainer(synth.synth_params(S, A, seed=1 + i), S, A, False, hyper, lrs, 1000) for i in range(2)]
    guides = [build_hip_trainer(synth.synth_params(S, A, seed=5 + i), S, A, False, hyper, lrs, 1000) for i in range(2)]
    x = [np.random.RandomState(9 + i).standard_normal((9, S)).astype(np.float32) for i in range(2)]
    gates = group.gates()
    assert len(gates) == 2 and all(isinstance(g, iql.GateHolder) for g in gates)
    got = iql.JsrlActors(learners, guides, gates).act(x, [2, 2], gate_max=[0.0, 0.0])
    ref = iql.JsrlActors(learners, guides, [t.gate() for t in twins]).act(x, [2, 2], gate_max=[0.0, 0.0])
    for g, r in zip(got, ref):
        assert all(np.array_equal(_bits(np.asarray(a)), _bits(np.asarray(b))) for a, b in zip(g, r))
    assert not np.array_equal(got[0][2], got[1][2][:len(got[0][2])])      # (two gates, not one twice)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_change_nothing():
    import iqlhip_binding as hb
    import variance_learner as VL
    S, A, B = 5, 2, 16
    _, buf = _make(S, A, 100, seed=14)
    _, short = _make(S, A, B - 1, seed=15)
    members, twins = _pair(3, S, A, B)
    group = VL.VarianceLearnerGroup(members)
    group.train_on_buffer(buf, 2, seeds=[1, 2, 3])                     # (scratch and records exist, counters are not zero)
    for t, s in zip(twins, (1, 2, 3)):
        t.train_on_buffer(buf, 2, seed=s)
    before = [_state(L) for L in members]
    unchanged = lambda: all(_same(_state(L), b) for L, b in zip(members, before))
    # at construction
    with pytest.raises(ValueError, match="member 2: the learner is member 0 too"):
        VL.VarianceLearnerGroup([members[0], members[1], members[0]])
    with pytest.raises(ValueError, match="member 1: state_dim = 6"):
        VL.VarianceLearnerGroup([members[0], _learner(S + 1, A, B)])
    with pytest.raises(ValueError, match="got 17"):
        VL.VarianceLearnerGroup(members + [_learner(S, A, B) for _ in range(14)])
    # calls: a window that leaves member 1's buffer, a buffer shorter than a window for member 2, no updates, empty lists
    empty = np.array([], dtype=np.int64)
    rows = W.synthetic_rows(B + 3, S, A, seed=1)
    batch, longer = W.window_tensors(rows, 0, B, S, A), W.window_tensors(rows, 0, B + 1, S, A)
    calls = [
        (lambda: group.update_from_buffer(buf, [0, 85, 0], False), "member 1"),
        (lambda: group.update_from_buffer(buf, [0, 0, -1], True), "member 2"),
        (lambda: group.get_values_window(buf, [85, 0, 0]), "member 0"),
        (lambda: group.update_from_buffer([buf, buf, short], 0, False), "member 2"),
        (lambda: group.train_on_buffer([buf, buf, short], 2, seeds=1), "member 2"),
        (lambda: group.train_on_buffer(buf, 0, seeds=1), "n_updates"),
        (lambda: group.train_on_buffer(buf, 2, seeds=1, starts=empty), "member 0"),
        (lambda: group.train_on_buffer(buf, 2, seeds=1, starts=[None, empty, None]), "member 1"),
        (lambda: group.train_on_buffer(buf, 2, seeds=1, starts=[]), "member 0"),
        (lambda: group.train_on_buffer(buf, 2, seeds=1, starts=[None, None, np.array([0, 85])]), "member 2"),
        (lambda: group.update([batch, longer, batch], False), "member 1"),
        (lambda: group.update([batch, batch], False), "one entry per member"),
        (lambda: group.run_training_on_buffer([buf, short, buf], 6, seeds=1, save_dir=None), "member 1"),
    ]
    for i, (call, names) in enumerate(calls):
        with pytest.raises(ValueError, match=names):
            call()
        assert unchanged(), i
    assert all(hasattr(L, "mf") for L in members)
    # the C ABI's own checks: B = 0, size < B, n_steps = 0, a list without entries, K = 17, a member twice
    lib, g, st, K = hb.lib(), group._group(), group._stream(), 3
    ptrs = lambda v: (hb.C.c_void_p * len(v))(*v)
    i64 = lambda v: (hb.C.c_int64 * len(v))(*v)
    rows_p, ld, A_ = ptrs([buf._rows.data_ptr()] * K), i64([buf._ld] * K), (hb.C.c_int32 * K)(*[A] * K)
    from iqlhip_variance import adam_scalars
    sc = (hb.VarScalars * (2 * K))(*[adam_scalars(1e-4, (0.9, 0.999), 1e-8, 3 + i) for i in range(2) for _ in range(K)])
    seeds, offs = (hb.C.c_uint64 * K)(1, 2, 3), (hb.C.c_uint64 * K)(0, 0, 0)
    lst = torch.tensor([0, 84], dtype=torch.int64, device="cuda")
    none, zero = ptrs([None] * K), i64([0] * K)

    def train(size=(100,) * K, B_=B, steps=2, lists=none, n_lists=zero):
        return lib.iqlhip_var_group_train_steps(g, rows_p, ld, i64(list(size)), A_, B_, steps, 0, sc, seeds, offs, lists, n_lists, st)

    def step_windows(size=(100,) * K, B_=B, start=(0,) * K):
        return lib.iqlhip_var_group_step_windows(g, rows_p, ld, i64(list(size)), A_, i64(list(start)), B_, 0, sc, st)

    for call, who in ((lambda: train(B_=0), "member 0"), (lambda: train(B_=1025), "member 0"), (lambda: train(size=(100, B - 1, 100)), "member 1"),
                      (lambda: train(steps=0), "n_steps"), (lambda: train(steps=hb.IQLHIP_VAR_TRAIN_MAX_STEPS + 1), "n_steps"),
                      (lambda: train(lists=ptrs([None, None, lst.data_ptr()])), "member 2"),
                      (lambda: step_windows(B_=0), "member 0"), (lambda: step_windows(size=(100, 100, B - 1)), "member 2"),
                      (lambda: step_windows(start=(0, 85, 0)), "member 1"), (lambda: step_windows(start=(-1, 0, 0)), "member 0")):
        assert call() == hb.E_INVAL
        assert who in hb.last_error(), (who, hb.last_error())
    handles = [int(L._h.value) for L in members]
    out = hb.C.c_void_p()
    assert lib.iqlhip_var_group_create(ptrs(handles + [handles[0]]), 4, hb.C.byref(out)) == hb.E_INVAL and "member 3" in hb.last_error()
    assert lib.iqlhip_var_group_create(ptrs(handles * 6), 17, hb.C.byref(out)) == hb.E_INVAL and not out.value
    assert lib.iqlhip_var_group_create(ptrs(handles), 0, hb.C.byref(out)) == hb.E_INVAL
    assert lib.iqlhip_var_group_create(None, 3, hb.C.byref(out)) == hb.E_INVAL
    assert lib.iqlhip_var_group_create(ptrs([handles[0], None]), 2, hb.C.byref(out)) == hb.E_INVAL and "member 1" in hb.last_error()
    assert unchanged()
    # ... and the accepted forms still run, from the state the refusals left alone
    out = group.train_on_buffer(buf, 3, seeds=[4, 5, 6])
    _same_burst(out, _solo_bursts(twins, [buf] * 3, 3, [4, 5, 6], [0] * 3, False, [None] * 3))
    assert all(_same(_state(a), _state(b)) for a, b in zip(members, twins))
