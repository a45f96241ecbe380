"""StreamingPipeline(gate_chi2=...), driven by tick_keypoints on the occlusion scenario of
tests/gate_ref.py (timed_ref.stream_case() with single corners displaced 60 px on half of the frames
from tick 12 on; test_gate_ref.py asserts the scenario's margins on the reference chain):

  * split and fused ticks: the effective masks equal each other on every tick and the reference
    chain's from the first corrupted tick on, ginfo 0 there, and the stream tracks the truth;
  * graph replay == eager, bit for bit; gate_chi2=None is the pipeline without the keyword;
  * gate_chi2 without timed=True raises; predict() against the reference.
"""
import numpy as np
import pytest

import gate_ref as GR
import marginals_ref as MR
import timed_ref as TR
from perseus_amd.streaming import StreamingPipeline

from test_streaming_pose_gpu import LW, SIG, _device_lin, _model, _pipe

pytestmark = pytest.mark.gpu

OCC = GR.OCC
OCC_SIG = dict(proj_sigma=OCC["sigmas"]["proj"], dyn_sigma=OCC["sigmas"]["dyn"], cv_sigma=OCC["sigmas"]["cv"],
               lam=OCC["lam"])
GATE = dict(gate_chi2=OCC["chi2"], gate_min_pass=OCC["min_pass"], gate_min_frames=OCC["min_frames"])
assert OCC["L"] == LW


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module")
def occ():
    case = GR.occlusion_case()
    return case, GR.gated_chain(case)


def _gated(model, graph, case, **kw):
    n = case["y"].shape[1]
    return _pipe(model, graph, init=(TR.init_pose(case["truth"][0]), np.zeros((n, 3)), np.zeros((n, 3))), timed=True,
                 **{**OCC_SIG, **GATE, **kw})


def _ticks(case):
    """Per tick the keypoints as the chains feed them (an absent camera's slot holds its last seen
    keypoints) with the tick's keywords."""
    last = case["y"][0].copy()
    for k in range(len(case["y"])):
        y = case["y"][k].copy()
        y[~case["present"][k]] = last[~case["present"][k]]
        last = y
        yield k, y, dict(stamps=case["stamps"][k], present=case["present"][k], kp_mask=case["mask"][k])


def test_occlusion_stream_split_and_fused(model, occ):
    case, ref = occ
    first = OCC["first_tick"]
    sp, fu = _gated(model, True, case), _gated(model, True, case, split_pose=False)
    assert sp.split_pose and fu.fused_pose and not fu.split_pose
    er, et = {"split": [], "fused": []}, {"split": [], "fused": []}
    for k, y, kw in _ticks(case):
        states = {}
        for name, p in (("split", sp), ("fused", fu)):
            pose, info = p.tick_keypoints(y, **kw)
            assert (info == 0).all(), (name, k, info)
            st = p.gate_state()
            states[name] = st
            r, t = TR.newest_errors(pose, case["truth"][k])
            er[name].append(r)
            et[name].append(t)
            np.testing.assert_array_equal(st["mask"], p.window_state()["mask"][:, -1])
        ms, mf = (states[nm]["mask"].astype(np.int64) & 0xFF for nm in ("split", "fused"))
        np.testing.assert_array_equal(ms, mf, err_msg=f"tick {k}")
        np.testing.assert_array_equal(states["split"]["ginfo"], states["fused"]["ginfo"], err_msg=f"tick {k}")
        if k < OCC["min_frames"]:
            assert (states["split"]["ginfo"] == GR.YOUNG).all(), k
        if k >= first:
            np.testing.assert_array_equal(ms, ref["mask"][k] & 0xFF, err_msg=f"tick {k}")
            assert (states["split"]["ginfo"] == 0).all() and (states["fused"]["ginfo"] == 0).all(), k
            hit = case["bad"][k] >= 0
            d2 = states["split"]["d2"]
            assert (d2[hit, case["bad"][k][hit]] > OCC["chi2"]).all(), (k, d2)
    for name in ("split", "fused"):
        print(name, "rot", max(er[name][-10:]), "tra", max(et[name][-10:]))
        assert max(er[name][-10:]) < TR.ROT_TOL and max(et[name][-10:]) < TR.TRA_TOL, name
    sp.close()
    fu.close()


@pytest.mark.parametrize("split", [True, False], ids=["split", "fused"])
def test_gated_graph_replay_equals_eager(model, occ, split):
    """The captured tick with the gate's three launches against the eager one, bit for bit, over the
    five ticks around the first corrupted one (and every tick before them)."""
    case, _ = occ
    g, e = _gated(model, True, case, split_pose=split), _gated(model, False, case, split_pose=split)
    assert g.graph is not None and e.graph is None
    cleared = 0
    for k, y, kw in _ticks(case):
        if k >= OCC["first_tick"] + 4:
            break
        for a, b in zip(g.tick_keypoints(y, **kw), e.tick_keypoints(y, **kw)):
            np.testing.assert_array_equal(a, b)
        if k < OCC["first_tick"] - 1:
            continue
        sg, se = g.window_state(), e.window_state()
        for key in sg:
            np.testing.assert_array_equal(sg[key], se[key], err_msg=key)
        gg, ge = g.gate_state(), e.gate_state()
        for key in gg:
            np.testing.assert_array_equal(gg[key], ge[key], err_msg=key)
        cleared += int((case["bad"][k] >= 0).sum())
    assert cleared >= 3
    g.close()
    e.close()


def test_gate_off_is_the_pipeline_without_the_keyword(model, occ):
    case, _ = occ
    a = _pipe(model, True, timed=True, **OCC_SIG)
    b = _pipe(model, True, timed=True, gate_chi2=None, **OCC_SIG)
    assert a._gate is None and b._gate is None
    for k, y, kw in _ticks(case):
        if k >= LW + 3:
            break
        for x, y_ in zip(a.tick_keypoints(y, **kw), b.tick_keypoints(y, **kw)):
            np.testing.assert_array_equal(x, y_)
    sa, sb = a.window_state(), b.window_state()
    for key in sa:
        np.testing.assert_array_equal(sa[key], sb[key], err_msg=key)
    with pytest.raises(RuntimeError, match="gate_chi2"):
        a.gate_state()
    a.close()
    b.close()


def test_gate_needs_timed(model):
    with pytest.raises(ValueError, match="timed=True"):
        StreamingPipeline(model, pose_window=LW, gate_chi2=13.816, **SIG)
    with pytest.raises(ValueError, match="gate_chi2"):
        StreamingPipeline(model, pose_window=LW, timed=True, gate_chi2=-1.0, **SIG)


def test_predict_after_a_tick(model, occ):
    """predict([0, dt]): the newest pose itself at tau = 0, and covariances that match the
    reference computed from window_state() and the device's factor outputs."""
    case, _ = occ
    n, nk = case["y"].shape[1], case["y"].shape[2] // 2
    p = _gated(model, True, case)
    for k, y, kw in _ticks(case):
        if k > LW + 2:
            break
        p.tick_keypoints(y, **kw)
    taus = np.array([0.0, TR.DT])
    pose, cov = p.predict(taus)
    st = p.window_state()
    assert pose.shape == (n, 2, 12) and cov.shape == (n, 2, 12, 12)
    np.testing.assert_array_equal(pose[:, 0], st["pose"][:, -1])
    win = {key: st[key] for key in ("pose", "angvel", "vel")}
    rc, rx = MR.dense(_device_lin(p), n, LW, nk, OCC["lam"])
    q = GR.process_noise(OCC["sigmas"])
    rp, rcov = GR.predict(win, np.tile(taus, (n, 1)), rc, rx, q_diag=q)
    np.testing.assert_allclose(pose, rp, atol=1e-9, rtol=1e-12)
    sd = np.sqrt(np.einsum("...ii->...i", rcov))
    err = float((np.abs(cov - rcov) / (sd[..., :, None] * sd[..., None, :])).max())
    print("scaled covariance error", err)
    assert err <= 1e-9
    np.testing.assert_array_equal(cov, cov.transpose(0, 1, 3, 2))
    pose0, cov0 = p.predict(taus, process_noise=False)
    np.testing.assert_array_equal(pose0, pose)
    rcov0 = GR.predict(win, np.tile(taus, (n, 1)), rc, rx)[1]
    assert float((np.abs(cov0 - rcov0) / (sd[..., :, None] * sd[..., None, :])).max()) <= 1e-9
    # the window's own marginals at tau = 0 (F = I): window_covariance()'s newest pose block
    wc = p.window_covariance()["cov"]
    s6 = np.sqrt(np.einsum("tii->ti", wc[:, -1, :6, :6]))
    assert (np.abs(cov0[:, 0, :6, :6] - wc[:, -1, :6, :6]) / (s6[:, :, None] * s6[:, None, :])).max() <= 1e-9
    b = _pipe(model, False, pre_ahead=True)
    with pytest.raises(ValueError, match="pre_ahead"):
        b.predict(taus)
    b.close()
    p.close()
