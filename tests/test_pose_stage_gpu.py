"""PoseStage, the fixed-lag smoother without a detector, against StreamingPipeline's pose stage.

n = 3 windows of L = 6 frames and 8 keypoints (LW, SIG and _init of test_streaming_pose_gpu.py), fed
the first 12 ticks of timed_ref.stream_case() (keypoints, stamps, absent cameras and masks, all made
on the CPU): the window fills, and with marginalize=True prior.minfo goes from 2 to 0.

  * a stand-alone PoseStage and a StreamingPipeline built with the same keywords, both driven by
    tick_keypoints, agree after every tick in everything the tick writes, in every tick form and
    with every feature on, and after the ticks in window_covariance(), predict() and solve_window();
  * the stand-alone stage's graph replay == its eager ticks;
  * the constructor errors of the stage are the pipeline's.

Both sides run the same kernels in the same order on the same inputs: every comparison is exact.
"""
import numpy as np
import pytest
import torch

import timed_ref as TR
from perseus_amd import pipeline
from perseus_amd.pose_stage import PoseStage
from perseus_amd.streaming import StreamingPipeline

from test_gate_streaming_gpu import GATE, _ticks
from test_streaming_pose_gpu import LW, SIG, _init, _model

pytestmark = pytest.mark.gpu

N, NK, TICKS = 3, 8, 12
PLAIN = {}
FULL = dict(timed=True, marginalize=True, angvel_sigma=0.05, proj_robust=("cauchy", 1.0), **GATE)
FORMS = {"split": {}, "fused": dict(split_pose=False), "four": dict(split_pose=False)}
CASES = [(form, feat) for form in FORMS for feat in ("plain", "full")] + [("ahead", "plain")]


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module")
def case():
    c = TR.stream_case()
    assert c["y"].shape[1:] == (N, 2 * NK)
    return {k: (v[:TICKS] if k in ("y", "stamps", "present", "mask") else v) for k, v in c.items()}


def _kw(form, feat):
    p0, v0, w0 = _init()
    kw = dict(init_pose=p0, init_vel=v0, init_angvel=w0, **SIG, **(FULL if feat == "full" else PLAIN))
    return dict(kw, pre_ahead=True) if form == "ahead" else dict(kw, **FORMS[form])


def _pair(model, form, feat, graph=True):
    """(stand-alone stage, pipeline) in one tick form with one feature set."""
    kw = _kw(form, feat)
    s, p = PoseStage(N, LW, NK, graph=graph, **kw), StreamingPipeline(model, graph=graph, pose_window=LW, **kw)
    if form == "four":  # (both capture the keypoint tick's graph on first use)
        s.fused_pose = False
        p.fused_pose = False
    assert (s.split_pose, s.fused_pose, s.pre_ahead) == (p.split_pose, p.fused_pose, p.pre_ahead) \
        == (form in ("split", "ahead"), form != "four", form == "ahead")
    return s, p


def _feed(case, feat):
    for k, y, kw in _ticks(case):
        yield k, y, (kw if feat == "full" else {})


def _same_tensors(a: dict, b: dict, what):
    assert a.keys() == b.keys(), what
    for key, v in a.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, b[key]), (what, key)


def _same_arrays(a: dict, b: dict, what):
    assert a.keys() == b.keys(), what
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=f"{what} {key}")


def _tick_ws_written(p):
    """The part of the split tick's workspace that the pre half writes (csrc/gn_cr_dev.h, GN_TICK_WSD): per
    window 24 frame slots of 144 + 12 doubles (B_l | a_l), of which a window of L frames fills the first L,
    then the root's S | b (144 + 12) and the failure word, an int32 at the start of the last two doubles.
    The rest of the buffer is never written and holds whatever the allocation held."""
    fd, lmax = 144 + 12, pipeline.TICK_MAX_L
    w = p.tick_ws.view(torch.float64).view(N, -1)
    assert w.shape[1] == lmax * fd + fd + 2
    return w[:, :LW * fd], w[:, lmax * fd:lmax * fd + fd], w[:, lmax * fd + fd:].contiguous().view(torch.int32)[:, 0]


def _same_state(s, p, what, ahead=False):
    """Everything a tick writes: s a PoseStage, p a PoseStage or a StreamingPipeline."""
    _same_arrays(s.window_state(), p.window_state(), what)
    _same_tensors(s.lin, p.lin, what)
    assert torch.equal(s.gn.out["delta"], p.gn.out["delta"]), what
    if s.prior is not None:
        _same_tensors(s.prior.cur, p.prior.cur, (what, "prior.cur"))
        _same_tensors(s.prior.nxt, p.prior.nxt, (what, "prior.nxt"))
        assert torch.equal(s.prior.minfo, p.prior.minfo), what
    if s.gate_chi2 is not None:
        _same_arrays(s.gate_state(), p.gate_state(), what)
    if ahead:
        for a, b in zip(_tick_ws_written(s), _tick_ws_written(p)):
            assert torch.equal(a, b), what


@pytest.mark.parametrize("form,feat", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_stage_alone_equals_the_pipelines(model, case, form, feat):
    s, p = _pair(model, form, feat)
    assert s.graph is None and p.pose_graph is None
    for k, y, kw in _feed(case, feat):
        for a, b in zip(s.tick_keypoints(y, **kw), p.tick_keypoints(y, **kw)):
            np.testing.assert_array_equal(a, b, err_msg=f"tick {k}")
        _same_state(s, p, f"tick {k}", ahead=form == "ahead")
        if feat == "full":
            minfo = s.prior.minfo.cpu().numpy()
            assert (minfo == (2 if k + 1 < LW else 0)).all(), (k, minfo)
    assert s.graph is not None and p.pose_graph is not None
    if feat == "full":
        assert s.prior.nxt["info"].abs().max().item() > 0.0
        assert (s.gate_state()["ginfo"] == 0).all()  # (the gate is past its young ticks and applied)
    # the host API on the window the ticks left
    _same_arrays(s.window_covariance(), p.window_covariance(), "window_covariance")
    if form != "ahead":  # (pre_ahead: predict() raises, the window is already the next tick's)
        for a, b in zip(s.predict([0.0, TR.DT]), p.predict([0.0, TR.DT])):
            assert np.isfinite(a).all()
            np.testing.assert_array_equal(a, b)
    lm = dict(with_prior=True) if feat == "full" else {}
    rs, rp = s.solve_window(**lm), p.solve_window(**lm)
    assert (rs["iters"] >= 1).all()
    _same_arrays(rs, rp, "solve_window")
    _same_state(s, p, "after solve_window", ahead=form == "ahead")
    s.close()
    p.close()


def test_stage_alone_graph_replay_equals_eager(case):
    kw = _kw("split", "full")
    g, e = PoseStage(N, LW, NK, graph=True, **kw), PoseStage(N, LW, NK, graph=False, **kw)
    assert g.split_pose and e.split_pose
    for k, y, tk in _feed(case, "full"):
        for a, b in zip(g.tick_keypoints(y, **tk), e.tick_keypoints(y, **tk)):
            np.testing.assert_array_equal(a, b, err_msg=f"tick {k}")
        _same_state(g, e, f"tick {k}")
    assert g.graph is not None and e.graph is None
    g.close()
    e.close()


TIMED = dict(timed=True)
ERRORS = [(LW, dict(gate_chi2=13.816), ValueError, "timed=True"),
          (LW, dict(gate_chi2=-1.0, **TIMED), ValueError, "gate_chi2"),
          (2, dict(gate_chi2=13.816, **TIMED), ValueError, "pose_window >= 3"),
          (LW, dict(pre_ahead=True, **TIMED), ValueError, "pre_ahead"),
          (LW, dict(pre_ahead=True, marginalize=True), ValueError, "pre_ahead"),
          (1, {}, ValueError, "pose_window must be >= 2"),
          (4, dict(vel_frame="camera"), AssertionError, "vel_frame")]


@pytest.mark.parametrize("L,kw,exc,match", ERRORS, ids=[f"L{e[0]}-{'-'.join(e[1]) or 'plain'}" for e in ERRORS])
def test_constructor_errors_are_the_pipelines(model, L, kw, exc, match):
    with pytest.raises(exc, match=match) as es:
        PoseStage(N, L, NK, **kw)
    with pytest.raises(exc, match=match) as ep:
        StreamingPipeline(model, pose_window=L, **kw)
    assert str(es.value) == str(ep.value)


def test_pre_ahead_downgrade_warns_alike(model):
    msgs = []
    kw = dict(graph=False, split_pose=False, pre_ahead=True, **SIG)
    for build in (lambda: PoseStage(N, 4, NK, **kw), lambda: StreamingPipeline(model, pose_window=4, **kw)):
        with pytest.warns(RuntimeWarning, match="pre_ahead") as rec:
            q = build()
        assert not q.pre_ahead and not q.split_pose
        msgs.append(str(rec[0].message))
        q.close()
    assert msgs[0] == msgs[1]


def test_stage_alone_rejects_timing_when_untimed():
    s = PoseStage(N, LW, NK, graph=False, **SIG)
    with pytest.raises(ValueError, match="stamps"):
        s.tick_keypoints(np.zeros((N, 2 * NK), np.float32), stamps=np.zeros(N))
    with pytest.raises(RuntimeError, match="gate_chi2"):
        s.gate_state()
    s.close()
