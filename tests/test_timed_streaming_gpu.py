"""StreamingPipeline(timed=True), driven by tick_keypoints: per-tick stamps, absent cameras and
keypoint masks through the rings self.win["dt"] / self.win["mask"].

  * one tick against the oracle chain (advance including both rings, factors, GN step, retract);
  * the 40-tick jitter / gap / drop-out stream of tests/test_timed_ref.py tracks the truth;
  * graph replay == eager, bit for bit, with five different stamp sets;
  * split tick == fused tick; marginalize=True runs; timed=False is the parent's tick;
  * the ValueError cases and the rings after a reset.
"""
import numpy as np
import pytest
import torch

import timed_ref as TR
from oracle import gn_ref as G
from perseus_amd.streaming import StreamingPipeline

from test_streaming_pose_gpu import LW, SIG, _device_lin, _init, _keypoints, _model, _pipe, _truth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module")
def case():
    return TR.stream_case()


def _tick(p, case, k, y=None):
    return p.tick_keypoints(case["y"][k] if y is None else y, stamps=case["stamps"][k], present=case["present"][k],
                            kp_mask=case["mask"][k])


def _np_win(st):
    w = {k: st[k] for k in ("y", "pose", "angvel", "vel", "dt")}
    w["mask"] = st["mask"].astype(np.int64) & 0xFFFFFFFF
    return w


def test_timed_tick_chain_vs_oracle(model, case):
    """_check_tick's form on a timed tick: a full window of jittered frames with single corners
    masked, then one more tick with a 2.2-period dt, one camera absent and one mask."""
    n, nk = 3, 8
    p = _pipe(model, True, init=(TR.init_pose(case["truth"][0]), np.zeros((n, 3)), np.zeros((n, 3))), timed=True)
    for k in range(LW + 1):
        _tick(p, case, k)
    before = p.window_state()
    k = LW + 1  # tick 7: camera 1 is absent
    assert not case["present"][k].all()
    stamps = case["stamps"][k - 1] + np.array([2.2, 0.8, 1.1]) * TR.DT
    mask = np.array([0b11011111, 0xFF, 0b00000001])
    pose, info = p.tick_keypoints(case["y"][k], stamps=stamps, present=case["present"][k], kp_mask=mask)
    after = p.window_state()
    dt_new = stamps - case["stamps"][k - 1]
    mask_new = np.where(case["present"][k], mask, 0)
    adv = TR.window_advance_t(_np_win(before), case["y"][k], dt_new, mask_new)
    np.testing.assert_array_equal(adv["y"], after["y"])
    np.testing.assert_array_equal(adv["dt"], after["dt"])  # the rings are only moved
    np.testing.assert_array_equal(adv["mask"], after["mask"].astype(np.int64) & 0xFFFFFFFF)
    ref = TR.window_factors(adv, np.full(n, LW), sigmas=TR.TICK_SIG)
    lin = _device_lin(p)
    np.testing.assert_array_equal(lin["status"], ref["status"])
    off = ref["status"] == 2
    assert off.sum() == 8 + 1 + 7 + sum(8 - bin(int(m) & 0xFF).count("1") for m in adv["mask"][:, :-1].reshape(-1))
    np.testing.assert_array_equal(lin["r_proj"][off], 0.0)
    np.testing.assert_array_equal(lin["j_proj"][off], 0.0)
    for key in ("r_proj", "j_proj", "r_dyn", "j_dyn0", "j_dyn1", "j_dyn2", "j_dyn3", "r_cv"):
        np.testing.assert_allclose(lin[key], ref[key], atol=1e-9, rtol=1e-12, err_msg=key)
    H, g, d = G.gn_step(lin, n, LW, nk, SIG["lam"])
    dd = p.gn.out["delta"].cpu().numpy().reshape(n, -1)
    eps = np.finfo(np.float64).eps
    for t in range(n):
        M = H[t] + SIG["lam"] * np.eye(H.shape[1])
        cond = np.linalg.cond(M)
        assert cond < 1e10 and info[t] == 0, (t, cond, info)
        np.testing.assert_allclose(dd[t], d[t], rtol=0, atol=max(10 * cond * eps, 1e-9) * np.abs(d[t]).max())
    from oracle import factors_ref as F

    ret = F.window_retract({key: adv[key] for key in ("y", "pose", "angvel", "vel")}, dd, info)
    for key in ("pose", "vel", "angvel"):
        np.testing.assert_allclose(after[key], ret[key], rtol=0, atol=1e-12, err_msg=key)
    np.testing.assert_array_equal(pose, after["pose"][:, -1])
    p.close()


@pytest.mark.parametrize("split", [True, False], ids=["split", "fused"])
def test_timed_stream_tracks_the_truth(model, case, split):
    """+-30 % jitter, a 3-period gap, a camera absent every 7th tick (its slot holds stale
    keypoints, which are run and ignored), single corners missing: 1e-4 rad / 1e-5 m over the last
    10 ticks, info == 0 on every tick."""
    n = 3
    p = _pipe(model, True, init=(TR.init_pose(case["truth"][0]), np.zeros((n, 3)), np.zeros((n, 3))), timed=True,
              split_pose=split)
    er, et = [], []
    last = case["y"][0].copy()
    for k in range(len(case["y"])):
        y = case["y"][k].copy()
        y[~case["present"][k]] = last[~case["present"][k]]
        last = y
        pose, info = _tick(p, case, k, y)
        assert (info == 0).all(), (k, info)
        r, t = TR.newest_errors(pose, case["truth"][k])
        er.append(r)
        et.append(t)
    print("rot", " ".join(f"{e:.1e}" for e in er))
    print("tra", " ".join(f"{e:.1e}" for e in et))
    assert er[0] > 1e-3 and max(er[-10:]) < TR.ROT_TOL and max(et[-10:]) < TR.TRA_TOL, (max(er[-10:]), max(et[-10:]))
    p.close()


def test_timed_graph_replay_equals_eager(model, case):
    g, e = _pipe(model, True, timed=True), _pipe(model, False, timed=True)
    assert g.graph is not None and e.graph is None
    for k in range(5):  # five different stamp sets through one captured graph
        for x, y_ in zip(_tick(g, case, k + 5), _tick(e, case, k + 5)):
            np.testing.assert_array_equal(x, y_)
        sg, se = g.window_state(), e.window_state()
        for key in sg:
            np.testing.assert_array_equal(sg[key], se[key], err_msg=key)
    assert len({tuple(r) for r in sg["dt"].reshape(-1, 1).tolist()}) > 5
    g.close()
    e.close()


def test_timed_split_tick_matches_fused(model, case):
    """test_streaming_pose_gpu.test_split_pose_tick_matches_fused's bar (delta within 1e-9 of its
    largest entry) on its kind of input, keypoints with 0.5 px noise, now with the stream's stamps,
    absent camera and masks.  (On exact keypoints the converged step is ~1e-5 and the two
    elimination orders' f64 rounding, ~2e-14 absolute, is not small against 1e-9 of that.)"""
    sp, fu = _pipe(model, True, timed=True), _pipe(model, True, timed=True, split_pose=False)
    assert sp.split_pose and not fu.split_pose
    rng = np.random.default_rng(11)
    for k in range(LW + 3):
        y = _keypoints(case["truth"][k], 0.5, rng)
        qs, ins = _tick(sp, case, k, y)
        qf, inf_ = _tick(fu, case, k, y)
        np.testing.assert_array_equal(ins, inf_)
        np.testing.assert_allclose(qs, qf, rtol=0, atol=1e-12)
        ds, df = sp.gn.out["delta"], fu.gn.out["delta"]
        assert (ds - df).abs().max().item() <= 1e-9 * df.abs().max().item(), k
        assert torch.equal(sp.lin["status"], fu.lin["status"])
    ws, wf = sp.window_state(), fu.window_state()
    for key in ("y", "dt", "mask"):
        np.testing.assert_array_equal(ws[key], wf[key], err_msg=key)
    sp.close()
    fu.close()


@pytest.mark.parametrize("graph", [True, False])
def test_timed_four_launch_tick_matches_fused(model, case, graph):
    """The four-launch pose stage (pa_window_advance_t, linearize, GN step, retract: what windows
    above 24 frames run) against the fused tick on the timed stream, bit for bit: poses, info, the
    window with both rings, every factor output and delta."""
    f, s = _pipe(model, graph, timed=True, split_pose=False), _pipe(model, graph, timed=True, split_pose=False)
    assert f.fused_pose and not f.split_pose
    s.fused_pose = False
    for k in range(LW + 3):
        qf, inf_ = _tick(f, case, k)
        qs, ins = _tick(s, case, k)
        np.testing.assert_array_equal(qf, qs)
        np.testing.assert_array_equal(inf_, ins)
        sf, ss = f.window_state(), s.window_state()
        assert set(sf) == {"y", "pose", "vel", "angvel", "dt", "mask"}
        for key in sf:
            np.testing.assert_array_equal(sf[key], ss[key], err_msg=key)
        for key, v in f.lin.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(v, s.lin[key]), key
        assert torch.equal(f.gn.out["delta"], s.gn.out["delta"])
    f.close()
    s.close()


def test_timed_long_window_runs_the_four_launch_tick(model, case):
    """A 30-frame timed window (above the fused tick's range) solves and carries its rings."""
    n = 3
    p = StreamingPipeline(model, graph=True, pose_window=30, timed=True, init_pose=TR.init_pose(case["truth"][0]),
                          init_vel=np.zeros((n, 3)), init_angvel=np.zeros((n, 3)), **SIG)
    assert not p.fused_pose and not p.split_pose
    for k in range(4):
        _, info = _tick(p, case, k)
        assert (info == 0).all(), (k, info)
    st = p.window_state()
    np.testing.assert_array_equal(st["dt"][:, -3:], np.diff(case["stamps"][:4], axis=0).T)
    np.testing.assert_array_equal(st["dt"][:, :-4], p.dt)
    np.testing.assert_array_equal(st["mask"][:, -4:].astype(np.int64) & 0xFF, case["mask"][:4].T)
    p.close()


@pytest.mark.parametrize("split", [True, False], ids=["split", "fused"])
def test_timed_zero_copy_reads_the_pinned_block(model, case, split):
    """zero_copy=True: the advance reads dt_new / mask_new from the pinned block in place
    (pa_host_device_pointer), no copy node.  Bit for bit the copying tick, graph replay."""
    a, b = _pipe(model, True, timed=True, zero_copy=True, split_pose=split), _pipe(model, True, timed=True,
                                                                                   zero_copy=False, split_pose=split)
    assert a.zero_copy and not b.zero_copy
    for k in range(LW + 3):
        for x, y_ in zip(_tick(a, case, k), _tick(b, case, k)):
            np.testing.assert_array_equal(x, y_)
    sa, sb = a.window_state(), b.window_state()
    for key in sa:
        np.testing.assert_array_equal(sa[key], sb[key], err_msg=key)
    assert len(np.unique(sa["dt"])) > 5
    a.close()
    b.close()


def test_direct_call_on_a_timed_pipeline_takes_the_nominal_timing(model):
    """pipe(rgb, depth) without tick(): not the previous tick's dt_new / mask_new again, but the
    nominal dt and all measured, and the last stamps move on by dt."""
    from test_streaming_gpu import _frames

    p = _pipe(model, True, timed=True)
    y = _keypoints(_truth(3, 1)[0][0])
    p.tick_keypoints(y, stamps=np.array([1.0, 1.0, 1.0]))
    p.tick_keypoints(y, stamps=np.array([1.09, 1.08, 1.07]), kp_mask=[1, 2, 4])
    p(*_frames(1))
    st = p.window_state()
    np.testing.assert_array_equal(st["dt"][:, -1], p.dt)
    np.testing.assert_array_equal(st["mask"][:, -1], -1)
    np.testing.assert_array_equal(st["mask"][:, -2], [1, 2, 4])
    p.tick_keypoints(y, stamps=np.array([1.09, 1.08, 1.07]) + p.dt + 0.05)
    np.testing.assert_allclose(p.window_state()["dt"][:, -1], 0.05, rtol=0, atol=1e-15)
    p.close()


def test_timed_marginalize_runs(model, case):
    p = _pipe(model, True, timed=True, marginalize=True)
    seen = []
    for k in range(10):
        _, info = _tick(p, case, k)
        assert (info == 0).all(), (k, info)
        seen.append(p.prior.minfo.cpu().numpy().copy())
    assert (seen[0] == 2).all() and (seen[-1] == 0).all(), seen  # 2 until the window has filled, then 0
    p.close()


def test_untimed_pipeline_is_the_parents(model):
    """timed=False (spelled out) against the pipeline built without the keyword, and a timed one fed
    nominal stamps: the same keypoints, bit for bit."""
    a, b, c = _pipe(model, True), _pipe(model, True, timed=False), _pipe(model, True, timed=True)
    truth, _, _ = _truth(3, LW + 2)
    for k in range(LW + 2):
        y = _keypoints(truth[k])
        qa, ia = a.tick_keypoints(y)
        qb, ib = b.tick_keypoints(y)
        qc, ic = c.tick_keypoints(y)
        for x, y_ in ((qa, qb), (ia, ib), (qa, qc), (ia, ic)):
            np.testing.assert_array_equal(x, y_)
    sa, sb, sc = a.window_state(), b.window_state(), c.window_state()
    assert set(sa) == set(sb) == {"y", "pose", "vel", "angvel"}
    for key in sa:
        np.testing.assert_array_equal(sa[key], sb[key], err_msg=key)
        np.testing.assert_array_equal(sa[key], sc[key], err_msg=key)
    for p in (a, b, c):
        p.close()


def test_value_errors_and_reset(model):
    with pytest.raises(ValueError, match="pre_ahead"):
        StreamingPipeline(model, pose_window=LW, timed=True, pre_ahead=True, **SIG)
    u = _pipe(model, False)
    y = _keypoints(_truth(3, 1)[0][0])
    for kw in (dict(stamps=np.zeros(3)), dict(present=np.ones(3, bool)), dict(kp_mask=np.full(3, 255))):
        with pytest.raises(ValueError, match="timed=True"):
            u.tick_keypoints(y, **kw)
    u.close()
    p = _pipe(model, False, timed=True)
    p.tick_keypoints(y, stamps=np.array([1.0, 1.0, 1.0]))
    p.tick_keypoints(y, stamps=np.array([1.04, 1.05, 1.06]), present=[True, False, True], kp_mask=[0x0F, 0xFF, 0xFF])
    before = p.window_state()
    for bad in (np.array([1.1, 1.05, 1.2]), np.array([1.1, np.nan, 1.2]), np.array([1.1, np.inf, 1.2]),
                np.array([1.1, 0.9, 1.2])):
        with pytest.raises(ValueError, match="stamps"):
            p.tick_keypoints(y, stamps=bad)
    after = p.window_state()
    for key in before:  # nothing was staged or enqueued: the window is untouched
        np.testing.assert_array_equal(before[key], after[key], err_msg=key)
    np.testing.assert_allclose(after["dt"][:, -1], [0.04, 0.05, 0.06], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(after["mask"][:, -1].astype(np.int64) & 0xFFFFFFFF, [0x0F, 0, 0xFF])
    p.reset_window()
    st = p.window_state()
    np.testing.assert_array_equal(st["dt"], np.full((3, LW - 1), p.dt))
    np.testing.assert_array_equal(st["mask"], np.full((3, LW), -1, np.int32))
    p.tick_keypoints(y, stamps=np.array([0.5, 0.5, 0.5]))  # the stamps were forgotten: the nominal dt
    np.testing.assert_array_equal(p.window_state()["dt"][:, -1], p.dt)
    p.close()
