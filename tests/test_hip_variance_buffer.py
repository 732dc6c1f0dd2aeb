"""GPU tests of the variance learner trained from a replay buffer (iqlhip_var_pack_window, iqlhip_var_train_steps,
iqlhip_var_values_window; VarianceLearner.pack_window / update_from_buffer / train_on_buffer / run_training_on_buffer;
DESIGN.md 6l "From a replay buffer").  Everything the device packs or draws is compared bit for bit: the packed block
against pack_block of the downloaded rows, a window update against _update_v on the downloaded tensors, a burst against
the eager loop over iqlhip_draw_indices' starts, the starts against oracle/philox_ref.py.  The one bounded comparison
(against the float64 restatement, tests/variance_ref.py) uses DESIGN.md 6l's rule: the larger of the project's fp32 bound
and four times the fp32 restatement's own deviation from float64."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import synth
import variance_ref as R
import variance_window_ref as W

pytestmark = pytest.mark.gpu

_NAMES = {f"{k}{i}": f"v.net.{2 * i}.{n}" for i in range(3) for n, k in (("weight", "w"), ("bias", "b"))}
CFG = type("Cfg", (), {"device": "cuda", "variance_learn_frac": 0.5})()


def _learner(S, A, B, aligned=False, seed=1, config=None):
    import variance_learner as VL
    L = VL.VarianceLearner(S, A, config, None, batch_size=B, device="cuda", aligned_rewards=aligned)
    for net, P in ((L.mf, R.synth_net(S, 2 * seed + 1)), (L.vf, R.synth_net(S, 2 * seed + 2))):
        net.load_state_dict({n: torch.from_numpy(P[k].copy()) for k, n in _NAMES.items()})
    return L


def _buffer(rows, S, A):
    """A GPU ReplayBuffer whose row store is exactly `rows` ([n][ld] float32 numpy or a device tensor), all rows held."""
    import iql
    buf = iql.ReplayBuffer(S, A, 4, "cuda")
    t = rows if isinstance(rows, torch.Tensor) else torch.from_numpy(rows).cuda()
    buf._rows, buf._rows_ptr, buf._ld = t, t.data_ptr(), t.shape[1]
    buf._buffer_size = buf._size = t.shape[0]
    buf._pointer = 0
    return buf


def _make(S, A, n, seed=0, pad=0):
    rows = W.synthetic_rows(n, S, A, seed, ld=W.row_stride(S, A) + pad)
    return rows, _buffer(rows, S, A)


def _state(L):
    """Every word the learner owns on the device, as bits, and its host counters."""
    torch.cuda.synchronize()
    return [a.cpu().numpy().view(np.uint32).copy() for a in (L._params_arena, L._m_arena, L._v_arena)], list(L._adam_t)


def _same(a, b):
    return a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))


def _segment(L, k):
    lo, hi = int(L._layout[k].seg_begin), int(L._layout[k].seg_end)
    return [x[lo:hi] for x in _state(L)[0]]


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x).view(np.uint32)


def _drawn(n, span, seed, offset=0):
    """iqlhip_draw_indices on the device: indices offset .. offset + n - 1 of the stream at counter offset 0."""
    import iqlhip_binding as hb
    ix = torch.empty(offset + n, dtype=torch.int64, device="cuda")
    hb.check(hb.lib().iqlhip_draw_indices(ix.data_ptr(), offset + n, span, seed, 0, torch.cuda.current_stream().cuda_stream))
    return ix.cpu().numpy()[offset:]


# ------------------------------------------------------------------------------------------------ 1. the packed block
@pytest.mark.parametrize("S,A,B", [(17, 6, 256), (3, 1, 1), (17, 6, 257), (127, 2, 33), (5, 28, 64)])
def test_pack_window_is_pack_block_of_the_downloaded_rows(S, A, B):
    from iqlhip_variance import pack_block
    L = _learner(S, A, B)
    n = B + 300
    for rows, buf in (_make(S, A, n, seed=B), _make(S, A, B, seed=B + 1), _make(S, A, n, seed=B + 2, pad=8)):
        size = rows.shape[0]
        down = buf._rows.cpu().numpy()
        for start in sorted({0, size - B, (size - B) // 3}):
            want, _ = pack_block(S, *[W.window_tensors(down, start, B, S, A)[i] for i in (0, 2, 4, 5)])
            got = L.pack_window(buf, start)
            assert got.device.type == "cuda" and got.shape == (B * S + S + 2 * B,)
            assert np.array_equal(_bits(got), want.view(np.uint32)), (size, start)
            assert np.array_equal(want.view(np.uint32), W.pack_window(rows, start, B, S, A).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 2. far rows
@pytest.mark.parametrize("line", [2 ** 31, 2 ** 32])
def test_pack_window_beyond_the_line(line):
    S, A, B = 17, 6, 256
    ld = W.row_stride(S, A)
    n = line // (4 * ld) + 1 + B // 2                # the last B rows lie on both sides of byte `line`
    assert n * ld * 4 > line > (n - B) * ld * 4
    store = torch.empty((n, ld), dtype=torch.float32, device="cuda")
    last = W.synthetic_rows(B, S, A, seed=3)
    store[n - B:] = torch.from_numpy(last).cuda()
    buf = _buffer(store, S, A)
    L = _learner(S, A, B)
    got = L.pack_window(buf, n - B)
    assert np.array_equal(_bits(got), W.pack_window(last, 0, B, S, A).view(np.uint32))
    s, p, v = L.get_values_window(buf, n - B)
    obs, _a, rew, _d, nxt, nd = W.window_tensors(last, 0, B, S, A)
    for a, b in zip((s, p, v), L.get_values(obs, rew, nxt, None, nd)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 3. one window update
@pytest.mark.parametrize("uv", [False, True])
@pytest.mark.parametrize("aligned", [False, True])
def test_update_from_buffer_is_update_v_on_the_downloaded_window(uv, aligned):
    S, A, B, start = 17, 6, 257, 5
    rows, buf = _make(S, A, 400, seed=11)
    a, b = _learner(S, A, B, aligned), _learner(S, A, B, aligned)
    for step in range(2):
        la = a.update_from_buffer(buf, start + step, uv)
        lb = b._update_v(W.window_tensors(buf._rows.cpu().numpy(), start + step, B, S, A), uv)
        assert set(la) == set(lb) and la["value_loss"] == lb["value_loss"]
        for key in ("values_samp_vec", "values_pred_vec", "variance_pred_vec"):
            assert np.array_equal(_bits(la[key]), _bits(lb[key])), key
    assert _same(_state(a), _state(b)) and a._adam_t == ([0, 2] if uv else [2, 0])
    opt = a.mv_optimizer if uv else a.m_optimizer
    assert all(float(st["step"]) == 2.0 for st in opt.state.values()) and len(opt.state) == 6
    # the alignment matters for these rows: the two settings give other values
    assert not torch.equal(a.get_values_window(buf, start)[0], _learner(S, A, B, not aligned).get_values_window(buf, start)[0])


# ------------------------------------------------------------------------------------------------ 4. the burst
def _eager(L, buf, starts, uv):
    return np.array([L.update_from_buffer(buf, int(s), uv)["value_loss"] for s in starts], dtype=np.float32)


@pytest.mark.parametrize("n", [1, 3, 7])
@pytest.mark.parametrize("uv", [False, True])
def test_train_on_buffer_equals_the_eager_loop(n, uv):
    S, A, B, seed = 17, 6, 33, 77
    rows, buf = _make(S, A, 1000, seed=5)
    a, b, fresh = _learner(S, A, B), _learner(S, A, B), _learner(S, A, B)
    out = a.train_on_buffer(buf, n, seed, update_vf=uv)
    starts = _drawn(n, 1000 - B + 1, seed)
    losses = _eager(b, buf, starts, uv)
    assert out["starts"].dtype == np.int64 and np.array_equal(out["starts"], starts)
    assert np.array_equal(out["starts"], W.burst_starts(n, 1000, B, seed))
    assert out["losses"].dtype == np.float32 and np.array_equal(out["losses"].view(np.uint32), losses.view(np.uint32))
    assert _same(_state(a), _state(b)) and a._adam_t == ([0, n] if uv else [n, 0])
    for x, y in zip(_segment(a, 0 if uv else 1), _segment(fresh, 0 if uv else 1)):
        assert np.array_equal(x, y), "the other net's parameters or moments changed"
    opt, other = (a.mv_optimizer, a.m_optimizer) if uv else (a.m_optimizer, a.mv_optimizer)
    assert all(float(st["step"]) == float(n) for st in opt.state.values()) and len(opt.state) == 6 and len(other.state) == 0
    for p, st in opt.state.items():
        assert st["exp_avg"].data_ptr() != 0 and st["exp_avg"].shape == p.shape and st["exp_avg"].abs().sum() > 0


def test_bursts_split_anywhere_give_the_same_result():
    S, A, B, seed = 5, 2, 8, 9
    rows, buf = _make(S, A, 600, seed=6)
    one, two = _learner(S, A, B), _learner(S, A, B)
    o = one.train_on_buffer(buf, 7, seed)
    t = [two.train_on_buffer(buf, 3, seed, offset=0), two.train_on_buffer(buf, 4, seed, offset=3)]
    assert np.array_equal(o["starts"], np.concatenate([x["starts"] for x in t]))
    assert np.array_equal(o["losses"].view(np.uint32), np.concatenate([x["losses"] for x in t]).view(np.uint32))
    assert _same(_state(one), _state(two))
    # a call longer than the ring: split inside train_on_buffer, against the same updates run in pieces
    import variance_learner as VL
    n = VL.TRAIN_MAX_STEPS + 6
    one, two = _learner(S, A, B), _learner(S, A, B)
    o = one.train_on_buffer(buf, n, seed, offset=1)
    t = [two.train_on_buffer(buf, 501, seed, offset=1), two.train_on_buffer(buf, n - 501, seed, offset=502)]
    assert np.array_equal(o["starts"], np.concatenate([x["starts"] for x in t]))
    assert np.array_equal(o["starts"], W.burst_starts(n, 600, B, seed, offset=1))
    assert np.array_equal(o["losses"].view(np.uint32), np.concatenate([x["losses"] for x in t]).view(np.uint32))
    assert _same(_state(one), _state(two)) and one._adam_t == [n, 0]
    assert np.isfinite(o["losses"]).all()


# ------------------------------------------------------------------------------------------------ 5. starts=
def test_starts_list_is_indexed_by_the_stream():
    S, A, B, seed, n = 5, 2, 16, 21, 40
    rows, buf = _make(S, A, 500, seed=7)
    lst = np.array([480, 3, 3, 250, 0, 484, 17], dtype=np.int64)
    a, b = _learner(S, A, B), _learner(S, A, B)
    out = a.train_on_buffer(buf, n, seed, offset=5, starts=lst)
    assert set(out["starts"].tolist()) <= set(lst.tolist()) and len(set(out["starts"].tolist())) > 3
    assert np.array_equal(out["starts"], W.burst_starts(n, 500, B, seed, offset=5, starts=lst))
    assert np.array_equal(out["starts"], lst[_drawn(n, len(lst), seed, offset=5)])
    losses = _eager(b, buf, out["starts"], False)
    assert np.array_equal(out["losses"].view(np.uint32), losses.view(np.uint32)) and _same(_state(a), _state(b))
    # a device tensor is taken as it is
    c = _learner(S, A, B)
    again = c.train_on_buffer(buf, n, seed, offset=5, starts=torch.from_numpy(lst).cuda())
    assert np.array_equal(again["starts"], out["starts"]) and _same(_state(a), _state(c))


def test_starts_from_the_episode_table_begin_at_episode_starts():
    import iql
    S, A, B, ep, E = 5, 2, 16, 40, 10
    rows = W.synthetic_rows(ep * E, S, A, seed=8, p_done=0.0)
    data = {"observations": rows[:, :S], "actions": rows[:, S:S + A], "next_observations": rows[:, S + A:2 * S + A],
            "rewards": rows[:, 2 * S + A], "terminals": (np.arange(ep * E) % ep == ep - 1).astype(np.float32)}
    buf = iql.ReplayBuffer(S, A, ep * E + 7, "cuda")
    buf.load_d4rl_dataset(data)
    first = buf.episode_returns(max_episode_steps=1000).episode_table()[0]
    assert first.dtype == torch.int64 and first.cpu().tolist() == list(range(0, ep * E, ep))
    L = _learner(S, A, B)
    out = L.train_on_buffer(buf, 30, seed=4, starts=first)
    assert (out["starts"] % ep == 0).all() and len(set(out["starts"].tolist())) > 3
    assert np.array_equal(out["starts"], W.burst_starts(30, ep * E, B, 4, starts=first.cpu().numpy()))
    # the window at an episode's first row carries the buffer's done flags as next_dones
    blk = L.pack_window(buf, int(out["starts"][0])).cpu().numpy()
    assert blk[(B + 1) * S + B:].sum() == 0.0
    assert L.pack_window(buf, ep - B).cpu().numpy()[(B + 1) * S + B:].tolist() == [0.0] * (B - 1) + [1.0]


# ------------------------------------------------------------------------------------------------ 6. the training loop
def test_run_training_on_buffer_splits_the_phases_and_saves(tmp_path):
    import iql
    import variance_learner as VL
    S, A, B = 5, 2, 16
    rows, buf = _make(S, A, 300, seed=9)
    a, b = _learner(S, A, B, config=CFG), _learner(S, A, B, config=CFG)
    vf = a.run_training_on_buffer(buf, n_updates=6, seed=13, save_dir=str(tmp_path), env_name="FakeEnv")
    m = b.train_on_buffer(buf, 4, 13, offset=0, update_vf=False)
    v = b.train_on_buffer(buf, 2, 13, offset=4, update_vf=True)
    assert vf is a.vf and not vf.training and not hasattr(a, "mf")
    assert a._adam_t == b._adam_t == [4, 2] and _same(_state(a), _state(b))
    assert np.array_equal(a.buffer_log["starts"], np.concatenate([m["starts"], v["starts"]]))
    assert np.array_equal(a.buffer_log["starts"], W.burst_starts(6, 300, B, 13))
    assert np.array_equal(a.buffer_log["losses"], np.concatenate([m["losses"], v["losses"]]))
    stem = tmp_path / "FakeEnv_None_6_0-5"
    sd = torch.load(str(stem) + "_vf.pt")
    assert os.path.exists(str(stem) + "_mf.pt") and all(t.device.type == "cpu" for t in sd.values())
    f = VL.StateDepFunction(S)
    f.load_state_dict(sd)
    assert all(torch.equal(x, y.cpu()) for x, y in zip(f.state_dict().values(), vf.state_dict().values()))
    g = VL.StateDepFunction(S)
    g.load_state_dict(torch.load(str(stem) + "_mf.pt"))
    assert all(torch.equal(x, y.cpu()) for x, y in zip(g.state_dict().values(), b.mf.state_dict().values()))
    assert iql.load_gate(sd, action_dim=A) is not None
    # save_dir=None writes nothing
    c = _learner(S, A, B, config=CFG)
    before = sorted(os.listdir(tmp_path))
    c.run_training_on_buffer(buf, n_updates=6, seed=13, save_dir=None)
    assert sorted(os.listdir(tmp_path)) == before and _same(_state(c), _state(b))


# ------------------------------------------------------------------------------------------------ 7. values
@pytest.mark.parametrize("S,A,B,aligned", [(17, 6, 256, False), (29, 8, 33, True), (3, 1, 1, False)])
def test_get_values_window_is_get_values_on_the_downloaded_window(S, A, B, aligned):
    rows, buf = _make(S, A, B + 50, seed=10)
    L = _learner(S, A, B, aligned)
    for start in (0, 50):
        obs, _a, rew, _d, nxt, nd = W.window_tensors(buf._rows.cpu().numpy(), start, B, S, A)
        want = L.get_values(obs, rew, nxt, None, nd)
        got = L.get_values_window(buf, start)
        for x, y in zip(got, want):
            assert x.device.type == "cpu" and x.shape == (B,) and np.array_equal(_bits(x), _bits(y))


# ------------------------------------------------------------------------------------------------ 8. parity
def test_burst_against_the_float64_restatement():
    S, A, B, n = 17, 6, 256, 3
    rows, buf = _make(S, A, 2000, seed=12)
    L = _learner(S, A, B, seed=1)
    out = L.train_on_buffer(buf, n, seed=31)
    chains = {}
    for dt in (np.float32, np.float64):
        mf, vf, m, v, steps = R.synth_net(S, 3), R.synth_net(S, 4), None, None, []
        for k, start in enumerate(out["starts"]):
            obs, _a, rew, _d, nxt, nd = W.window_tensors(rows, int(start), B, S, A)
            st = R.step(mf, vf, obs, nxt[B - 1], rew, nd > 0, 0, dt, t_adam=k + 1, m=m, v=v)
            mf, m, v = st["params"], st["m"], st["v"]
            steps.append(st)
        chains[dt] = steps
    bound = R.bounds(R.deviations(chains[np.float32][-1], chains[np.float64][-1]))
    want = chains[np.float64]
    dev_loss = max(R.rel(out["losses"][k], want[k]["loss"]) for k in range(n))
    ref_loss = max(R.rel(chains[np.float32][k]["loss"], want[k]["loss"]) for k in range(n))
    got = {grp: {} for grp in ("params", "m", "v")}
    for grp, arena in (("params", L._params_arena), ("m", L._m_arena), ("v", L._v_arena)):
        flat = arena.cpu().numpy()
        for key in R.KEYS:
            off, shape = int(getattr(L._layout[0], key)), want[-1]["params"][key].shape
            got[grp][key] = flat[off: off + int(np.prod(shape))].reshape(shape)
    dev_param = max(R.absmax(got["params"][k], want[-1]["params"][k]) for k in R.KEYS)
    dev_moment = max(R.rel(got[g][k], want[-1][g][k]) for g in ("m", "v") for k in R.KEYS)
    print(f"burst parity: loss {dev_loss:.2e} (bound {max(bound['loss'], 4 * ref_loss):.2e})  param {dev_param:.2e} "
          f"(bound {bound['param']:.2e})  moment {dev_moment:.2e} (bound {bound['moment']:.2e})")
    assert dev_loss <= max(bound["loss"], 4 * ref_loss)
    assert dev_param <= bound["param"] and dev_moment <= bound["moment"]


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_change_nothing():
    import iql
    import iqlhip_binding as hb
    S, A, B = 5, 2, 16
    rows, buf = _make(S, A, 100, seed=14)
    L = _learner(S, A, B)
    L.train_on_buffer(buf, 2, seed=1)                       # (the scratch exists, counters are not zero)
    before = _state(L)
    _, short = _make(S, A, B - 1, seed=15)
    _, other_dim = _make(S + 1, A, 100, seed=16)
    cpu_buf = iql.ReplayBuffer(S, A, 100, "cpu")
    cpu_buf._size = 100
    good = np.array([0, 84], dtype=np.int64)
    py_calls = [
        lambda: L.pack_window(buf, -1), lambda: L.pack_window(buf, 100 - B + 1), lambda: L.pack_window(short, 0),
        lambda: L.update_from_buffer(buf, -1, False), lambda: L.update_from_buffer(buf, 85, True),
        lambda: L.get_values_window(buf, 85), lambda: L.get_values_window(buf, -3),
        lambda: L.train_on_buffer(short, 2, seed=1), lambda: L.train_on_buffer(buf, 0, seed=1),
        lambda: L.train_on_buffer(other_dim, 2, seed=1), lambda: L.pack_window(other_dim, 0),
        lambda: L.train_on_buffer(cpu_buf, 2, seed=1), lambda: L.update_from_buffer(cpu_buf, 0, False),
        lambda: L.train_on_buffer(buf, 2, seed=1, starts=np.array([0, 85], dtype=np.int64)),
        lambda: L.train_on_buffer(buf, 2, seed=1, starts=np.array([-1], dtype=np.int64)),
        lambda: L.train_on_buffer(buf, 2, seed=1, starts=np.array([], dtype=np.int64)),
        lambda: L.train_on_buffer(buf, 2, seed=1, starts=np.array([1.0])),
        lambda: L.run_training_on_buffer(short, 6, save_dir=None),
    ]
    for i, call in enumerate(py_calls):
        with pytest.raises((ValueError, NotImplementedError)):
            call()
        assert _same(_state(L), before), i
    assert hasattr(L, "mf")
    # the C ABI's own checks
    lib, h, st = hb.lib(), L._h, L._stream()
    ptr, ld = buf._rows.data_ptr(), buf._ld
    out = torch.empty(B * S + S + 2 * B + 3 * B, dtype=torch.float32, device="cuda")
    lst = torch.from_numpy(good).cuda()
    sc = (hb.VarScalars * 2)(*[__import__("iqlhip_variance").adam_scalars(1e-4, (0.9, 0.999), 1e-8, t) for t in (3, 4)])
    pack = lambda **kw: lib.iqlhip_var_pack_window(*[{**dict(h=h, rows=ptr, ld=ld, n=100, S=S, A=A, start=0, B=B, out=out.data_ptr(), st=st), **kw}[k]
                                                    for k in ("h", "rows", "ld", "n", "S", "A", "start", "B", "out", "st")])
    vals = lambda **kw: lib.iqlhip_var_values_window(*[{**dict(h=h, rows=ptr, ld=ld, n=100, S=S, A=A, start=0, B=B, al=0, out=out.data_ptr(), st=st), **kw}[k]
                                                      for k in ("h", "rows", "ld", "n", "S", "A", "start", "B", "al", "out", "st")])
    train = lambda **kw: lib.iqlhip_var_train_steps(*[{**dict(h=h, rows=ptr, ld=ld, n=100, A=A, B=B, steps=2, net=0, sc=sc, seed=1, off=0, lst=None, nl=0, st=st), **kw}[k]
                                                     for k in ("h", "rows", "ld", "n", "A", "B", "steps", "net", "sc", "seed", "off", "lst", "nl", "st")])
    for fn in (pack, vals):
        for kw in (dict(h=None), dict(rows=None), dict(out=None), dict(S=S + 1), dict(B=0), dict(B=1025), dict(n=B - 1),
                   dict(start=-1), dict(start=85), dict(ld=ld - 4)):
            assert fn(**kw) == hb.E_INVAL, kw
    for kw in (dict(h=None), dict(rows=None), dict(sc=None), dict(B=0), dict(B=1025), dict(n=B - 1), dict(ld=ld - 4),
               dict(steps=0), dict(steps=hb.IQLHIP_VAR_TRAIN_MAX_STEPS + 1), dict(lst=lst.data_ptr(), nl=0), dict(net=2)):
        assert train(**kw) == hb.E_INVAL, kw
    lo, so = (C.c_float * 4)(), (C.c_int64 * 4)()
    for args in ((None, lo, so, 2, st), (h, None, so, 2, st), (h, lo, None, 2, st), (h, lo, so, 0, st),
                 (h, lo, so, hb.IQLHIP_VAR_TRAIN_MAX_STEPS + 1, st)):
        assert lib.iqlhip_var_read_train_ring(*args) == hb.E_INVAL
    assert _same(_state(L), before)
    # ... and the accepted forms still run, from the state the refusals left alone
    twin = _learner(S, A, B)
    twin.train_on_buffer(buf, 2, seed=1)
    assert pack() == 0 and vals() == 0
    a, b = L.train_on_buffer(buf, 3, seed=2, starts=good), twin.train_on_buffer(buf, 3, seed=2, starts=good)
    assert np.array_equal(a["losses"].view(np.uint32), b["losses"].view(np.uint32)) and _same(_state(L), _state(twin))


def test_learner_does_not_disturb_a_trainer_on_the_same_buffer():
    import iql
    from hip_helpers import build_hip_trainer
    S, A, B = 17, 6, 64
    hyper = {"iql_tau": 0.7, "beta": 3.0, "discount": 0.99, "tau": 0.005, "deterministic": False}
    lrs = {"v": 3e-4, "q": 3e-4, "pi": 3e-4}
    buf = iql.ReplayBuffer(S, A, 4096, "cuda")
    buf.fill_synthetic(4096, seed=3)

    def run(with_learner):
        tr = build_hip_trainer(synth.synth_params(S, A, seed=20), S, A, True, hyper, lrs, 1000, device="cuda:0")
        L = _learner(S, A, B) if with_learner else None
        losses = [np.asarray(tr.train_steps(buf, 5, B, seed=11))]
        burst = L.train_on_buffer(buf, 4, seed=6) if L is not None else None
        losses.append(np.asarray(tr.train_steps(buf, 5, B, seed=12)))
        torch.cuda.synchronize()
        arenas = [a.cpu().numpy().view(np.uint32).copy() for a in (tr._params_arena, tr._target_arena, tr._m_arena, tr._v_arena)]
        return losses, arenas, burst

    a, b = run(True), run(False)
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert np.array_equal(x, y)
    alone = _learner(S, A, B).train_on_buffer(buf, 4, seed=6)
    assert np.array_equal(a[2]["losses"].view(np.uint32), alone["losses"].view(np.uint32))
    assert np.array_equal(a[2]["starts"], alone["starts"])
