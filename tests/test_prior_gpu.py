"""Fixed-lag marginalization on the device (csrc/prior.hip: pa_window_marginalize,
pa_window_prior_linearize; the prior on frame 0 in pa_trajectory_gn_step_prior,
pa_trajectory_marginals_prior and the streaming ticks) against tests/prior_ref.py, the dense
f64 Schur complement of the device's own whitened factors.

Bars: rtol 1e-9 on assembled blocks (atol scaled by the block's largest entry), 1e-7
on delta, the marginals tests' scaled deviation 1e-9 on covariances.  Windows: test_gn_gpu's
constructed ones.  Shapes: T in {1, 3} runs the cyclic-reduction step, T = 70 the two-ended one
(L = 25 is above the cyclic reduction's range at any T); n_kp 0 / 8 / 16 cover the null projection
arrays and both RP instantiations."""
import functools

import numpy as np
import pytest
import torch

import marginals_ref as MR  # tests/ is on sys.path (rootdir conftest)
import prior_ref as PR
from oracle import factors_ref as F
from perseus_amd import _lib, pipeline

from test_pipeline_gpu import CORNERS, KCAL, _problem

pytestmark = pytest.mark.gpu
RTOL = 1e-9
NV = 12
JAC = ("j_proj", "j_dyn0", "j_dyn1", "j_dyn2", "j_dyn3", "j_cv0", "j_cv1")
KEYS = ("r_proj", "j_proj", "status", "r_dyn", "j_dyn0", "j_dyn1", "j_dyn2", "j_dyn3", "r_cv", "j_cv0", "j_cv1")
CORNERS16 = np.concatenate([CORNERS, 0.6 * CORNERS[:, [1, 2, 0]]])
# name -> (T, L, K, lam, trajectories whose frame-0 keypoint 2 carries a cheirality status (1, r = J = NaN))
# (A frame 0 with NO usable keypoint and no input prior is held by lambda alone: Lambda' is then at
# the lambda level by cancellation from |F| ~ 1e3.  The n_kp = 0 windows without a prior are such
# windows and are asserted at the operand-scaled bar, see test_marginalize_matches_reference.)
CASES = {"t1_l3_k8": (1, 3, 8, 1e-3, ()), "t3_l24_k16": (3, 24, 16, 1e-3, (0,)), "t3_l3_k0": (3, 3, 0, 1e-2, ()),
         "t70_l24_k8": (70, 24, 8, 1e-3, (2,)), "t70_l25_k0": (70, 25, 0, 1e-2, ()), "t70_l3_k16": (70, 3, 16, 1e-4, ())}


def _dev(a, dtype=torch.float64):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


@functools.lru_cache(maxsize=None)
def _case(name):
    """A named window, built once and never modified: f (numpy factors, Jacobians (n, rows,
    cols)), raw (device tensors in the C layout, Jacobians column-major), the state, a random SPD
    prior with its gradient."""
    T, L, K, lam, cheir = CASES[name]
    poses, vels, angvels, _ = _problem(T, L, 100 + T + L + K)
    kk = K or 8
    y = np.random.default_rng(T * L + K).uniform(-1, 1, (T * L, 2 * kk)).astype(np.float32)
    lin = pipeline.linearize_trajectories(torch.as_tensor(y, device="cuda"), poses, vels, angvels,
                                          CORNERS16 if K == 16 else CORNERS, KCAL, T=T, L=L, dt=0.1,
                                          proj_sigmas=np.array([2.0, 2.0]), dyn_sigmas=np.full(6, 0.05),
                                          cv_sigmas=np.full(3, 0.5))
    f = {k: lin[k].cpu().numpy().copy() for k in KEYS}
    for t in cheir:
        u = t * L * K + 2
        f["status"][u], f["r_proj"][u], f["j_proj"][u] = 1, np.nan, np.nan
    if K == 0:  # null projection arrays
        f["r_proj"], f["j_proj"], f["status"] = np.zeros((0, 2)), np.zeros((0, 2, 6)), np.zeros(0, np.int32)
    pinfo, pgrad = PR.random_spd(np.random.default_rng(7 + T), T, 3.0)
    return dict(T=T, L=L, K=K, lam=lam, f=f, raw=_raw(f, K), pose=poses, vel=vels, angvel=angvels, pinfo=pinfo,
                pgrad=pgrad)


def _raw(f, K):
    """numpy factors -> device tensors in the C layout (None for the projection arrays at K = 0)."""
    out = {}
    for k in KEYS:
        if K == 0 and k in ("r_proj", "j_proj", "status"):
            out[k] = None
        elif k in JAC:
            out[k] = _dev(f[k].transpose(0, 2, 1))
        else:
            out[k] = _dev(f[k], torch.int32 if k == "status" else torch.float64)
    return out


def _fptrs(raw):
    return [_lib.ptr(raw[k]) for k in KEYS]


def _gn(raw, T, L, K, lam, pinfo=None, pgrad=None, parent=False):
    """(delta (T, L, 12), info (T,)) of pa_trajectory_gn_step_prior (parent: pa_trajectory_gn_step)."""
    L_, p = _lib.lib(), _lib.ptr
    delta = torch.full((T * L, NV), 7.0, dtype=torch.float64, device="cuda")
    info = torch.full((T,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(int(L_.pa_trajectory_gn_workspace(T, L)), 8), dtype=torch.uint8, device="cuda")
    head = (T, L, K, *_fptrs(raw), lam, None, None, None, p(delta), p(info), p(ws), ws.numel())
    pi, pg = _dev(pinfo), _dev(pgrad)
    if parent:
        _lib.check(L_.pa_trajectory_gn_step(*head, None), "gn")
    else:
        _lib.check(L_.pa_trajectory_gn_step_prior(*head, p(pi), p(pg), None), "gn prior")
    torch.cuda.synchronize()
    return delta.cpu().numpy().reshape(T, L, NV), info.cpu().numpy()


def _marginals(raw, T, L, K, lam, pinfo=None, pgrad=None, parent=False):
    L_, p = _lib.lib(), _lib.ptr
    cov = torch.full((T * L, NV, NV), 7.0, dtype=torch.float64, device="cuda")
    info = torch.full((T,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(int(L_.pa_trajectory_marginals_workspace(T, L)), 8), dtype=torch.uint8, device="cuda")
    head = (T, L, K, *_fptrs(raw), lam, p(cov), None, None, p(info), p(ws), ws.numel())
    pi, pg = _dev(pinfo), _dev(pgrad)
    if parent:
        _lib.check(L_.pa_trajectory_marginals(*head, None), "marginals")
    else:
        _lib.check(L_.pa_trajectory_marginals_prior(*head, p(pi), p(pg), None), "marginals prior")
    torch.cuda.synchronize()
    return cov.cpu().numpy().reshape(T, L, NV, NV), info.cpu().numpy()


def _marginalize(c, lam=None, pinfo=None, pgrad=None, delta=None, gn_info=None, nvalid=None, raw=None):
    """pa_window_marginalize on case c: dict of numpy outputs."""
    T, L, K = c["T"], c["L"], c["K"]
    p = _lib.ptr
    o = {"info": torch.full((T, NV, NV), 7.0, dtype=torch.float64, device="cuda"),
         "eta": torch.full((T, NV), 7.0, dtype=torch.float64, device="cuda"),
         "xbar_pose": torch.zeros((T, 12), dtype=torch.float64, device="cuda"),
         "xbar_angvel": torch.zeros((T, 3), dtype=torch.float64, device="cuda"),
         "xbar_vel": torch.zeros((T, 3), dtype=torch.float64, device="cuda"),
         "minfo": torch.full((T,), -1, dtype=torch.int32, device="cuda")}
    keep = [_dev(pinfo), _dev(pgrad), _dev(delta), _dev(gn_info, torch.int32), _dev(nvalid, torch.int32),
            _dev(c["pose"]), _dev(c["angvel"]), _dev(c["vel"])]
    _lib.check(_lib.lib().pa_window_marginalize(
        T, L, K, *_fptrs(c["raw"] if raw is None else raw), p(keep[0]), p(keep[1]), c["lam"] if lam is None else lam,
        *[p(k) for k in keep[2:]], *[p(o[k]) for k in ("info", "eta", "xbar_pose", "xbar_angvel", "xbar_vel", "minfo")],
        None), "marginalize")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _close_blocks(got, ref, what, scales=None):
    """rtol 1e-9, atol 1e-9 x the largest entry of each trajectory's reference block (or x
    scales[t] where the block is nonzero)."""
    for t in range(len(ref)):
        scale = np.abs(ref[t]).max()
        if scales is not None and scale:
            scale = scales[t]
        err = np.abs(got[t] - ref[t]).max() / scale if scale else np.abs(got[t]).max()
        np.testing.assert_allclose(got[t], ref[t], rtol=RTOL, atol=RTOL * scale, err_msg=f"{what}[{t}]")
    return err


# ---------------------------------------------------------------- 1. marginalize against the reference
@pytest.mark.parametrize("name,prior", [(n, p) for p in (True, False) for n in CASES])
def test_marginalize_matches_reference(name, prior):
    """Bar: rtol 1e-9, atol 1e-9 x the reference block's own largest entry.  The exception, stated
    before the run: n_kp = 0 without an input prior.  Frame 0 is then held by lambda alone (H has
    three eigenvalues at lambda = 1e-2 under entries of 1e3), Lambda' = F - E^T H^-1 E and
    g' = h - E^T H^-1 g_0 come out at the lambda level by cancellation, and f64 carries them to
    eps x cond(H) x |F| (|h|), not to 1e-9 of themselves.  Those two windows are asserted with
    atol 1e-9 x the largest entry of the operands, H, E, F for Lambda' and g_0, h for eta
    (prior_ref.operand_scale: the scales test_gn_gpu's atol uses for assembled blocks and g).
    Measured: Lambda' 1e-13 of the operands, 5e-9 of its own largest entry; eta 6e-9 of its own."""
    c = _case(name)
    ill = not prior and c["K"] == 0
    scales, gscales = PR.operand_scale(c["f"], c["T"], c["L"], c["K"]) if ill else (None, None)
    T, L, K, lam = c["T"], c["L"], c["K"], c["lam"]
    pinfo, pgrad = (c["pinfo"], c["pgrad"]) if prior else (None, None)
    nvalid = np.full(T, L, np.int32)
    if T > 1:
        nvalid[1] = L - 1  # one window that has not filled
    ref_info, ref_eta, ref_minfo = PR.marginalize(c["f"], T, L, K, lam, pinfo, pgrad, nvalid=nvalid)
    out = _marginalize(c, pinfo=pinfo, pgrad=pgrad, nvalid=nvalid)
    np.testing.assert_array_equal(out["minfo"], ref_minfo)
    assert set(ref_minfo.tolist()) == ({0, 2} if T > 1 else {0})
    e_info = _close_blocks(out["info"], ref_info, "info", scales)
    e_eta = _close_blocks(out["eta"], ref_eta, "eta", gscales)
    print(f"{name} prior={prior}: last trajectory's scaled deviation info {e_info:.3g}, eta {e_eta:.3g}")
    assert _bits(out["info"], out["info"].transpose(0, 2, 1))
    if T > 1:
        assert not out["info"][1].any() and not out["eta"][1].any()  # (zeros, not the 7.0 fill)
    f1 = np.arange(T) * L + 1  # xbar = frame 1 as it stands, whatever minfo says
    assert _bits(out["xbar_pose"], c["pose"][f1]) and _bits(out["xbar_angvel"], c["angvel"][f1])
    assert _bits(out["xbar_vel"], c["vel"][f1])
    # nvalid NULL: every window counts as full, the other trajectories' bits unchanged
    full = _marginalize(c, pinfo=pinfo, pgrad=pgrad)
    assert (full["minfo"] == 0).all()
    keep = nvalid == L
    assert _bits(full["info"][keep], out["info"][keep]) and _bits(full["eta"][keep], out["eta"][keep])


def test_marginalize_reports_a_singular_frame():
    """H not positive definite, built honestly: no keypoints, no prior, lambda = 0 and zero
    dynamics Jacobians, so frame 0's pose and angular velocity are in no factor (H's leading
    pivots are exactly 0)."""
    c = dict(_case("t3_l3_k0"))
    f = {k: v.copy() for k, v in c["f"].items()}
    for k in ("j_dyn0", "j_dyn1", "j_dyn2"):
        f[k][:] = 0.0
    _, _, ref_minfo = PR.marginalize(f, c["T"], c["L"], 0, 0.0)
    out = _marginalize(c, lam=0.0, raw=_raw(f, 0))
    assert (ref_minfo == 1).all()
    np.testing.assert_array_equal(out["minfo"], ref_minfo)
    assert not out["info"].any() and not out["eta"].any()
    assert _bits(out["xbar_pose"], c["pose"][np.arange(c["T"]) * c["L"] + 1])


# ---------------------------------------------------------------- 2. / 3. the Schur identity on the device
@pytest.mark.parametrize("name", list(CASES))
def test_schur_identity_gn_step(name):
    """The step of the L-frame window with a random SPD prior on frame 0, and the step of frames
    1 .. L-1 alone with the prior pa_window_marginalize made of frame 0: the same delta."""
    c = _case(name)
    T, L, K, lam = c["T"], c["L"], c["K"], c["lam"]
    d_full, i_full = _gn(c["raw"], T, L, K, lam, c["pinfo"], c["pgrad"])
    m = _marginalize(c, pinfo=c["pinfo"], pgrad=c["pgrad"])
    assert (m["minfo"] == 0).all()
    sub = _raw(PR.drop_frame0(c["f"], T, L, K), K)
    d_red, i_red = _gn(sub, T, L - 1, K, lam, m["info"], -m["eta"])
    assert (i_full == 0).all() and (i_red == 0).all(), (i_full, i_red)
    ref = PR.dense_delta(c["f"], T, L, K, lam, c["pinfo"], c["pgrad"]).reshape(T, L, NV)
    scale = np.abs(ref).max()
    print(f"{name}: |delta| {scale:.3g}, full vs dense {np.abs(d_full - ref).max() / scale:.3g}, "
          f"reduced vs full {np.abs(d_red - d_full[:, 1:]).max() / scale:.3g}")
    np.testing.assert_allclose(d_full, ref, rtol=1e-7, atol=1e-9 * scale)
    np.testing.assert_allclose(d_red, d_full[:, 1:], rtol=1e-7, atol=1e-9 * scale)


@pytest.mark.parametrize("name", list(CASES))
def test_schur_identity_marginals(name):
    """The marginals tests' bar, scaled deviation 1e-9, on the windows with keypoints.  The two
    windows with none (n_kp = 0: every frame held by the prior on frame 0 and lam = 1e-2 alone under
    entries of H up to 1e3, cond ~ 1e5 per frame and growing along the chain) are asserted at
    1e-8: at t70_l25_k0 the parent step itself is 2.3e-10 off the dense solve
    (test_schur_identity_gn_step prints it) and the two covariances measured 2.7e-9 apart."""
    c = _case(name)
    T, L, K, lam = c["T"], c["L"], c["K"], c["lam"]
    cov_full, i_full = _marginals(c["raw"], T, L, K, lam, c["pinfo"], c["pgrad"])
    m = _marginalize(c, pinfo=c["pinfo"], pgrad=c["pgrad"])
    sub = _raw(PR.drop_frame0(c["f"], T, L, K), K)
    cov_red, i_red = _marginals(sub, T, L - 1, K, lam, m["info"], -m["eta"])
    assert (i_full == 0).all() and (i_red == 0).all()
    e, _ = MR.scaled_err(cov_red, None, cov_full[:, 1:], None)
    print(f"{name}: scaled deviation of the shared frames' covariance {e:.3g}")
    assert e <= (RTOL if K else 1e-8)


# ---------------------------------------------------------------- 4. no prior = the parent, bit for bit
@pytest.mark.parametrize("name", ["t3_l24_k16", "t70_l24_k8", "t70_l25_k0"])
def test_null_prior_is_the_parent_entry_point(name):
    c = _case(name)
    T, L, K, lam = c["T"], c["L"], c["K"], c["lam"]
    d0, i0 = _gn(c["raw"], T, L, K, lam, parent=True)
    d1, i1 = _gn(c["raw"], T, L, K, lam)
    assert _bits(d0, d1) and np.array_equal(i0, i1) and (i0 == 0).all()
    c0, j0 = _marginals(c["raw"], T, L, K, lam, parent=True)
    c1, j1 = _marginals(c["raw"], T, L, K, lam)
    assert _bits(c0, c1) and np.array_equal(j0, j1) and (j0 == 0).all()
    d2, _ = _gn(c["raw"], T, L, K, lam, c["pinfo"], c["pgrad"])
    assert not _bits(d0, d2)  # (and a prior does change the step)


# ---------------------------------------------------------------- 5. re-centring
def test_recentring():
    c = _case("t3_l24_k16")
    T, L = c["T"], c["L"]
    rng = np.random.default_rng(3)
    delta = rng.standard_normal((T * L, NV))
    gn_info = np.array([0, 5, 0], np.int32)
    base = _marginalize(c, pinfo=c["pinfo"], pgrad=c["pgrad"])
    rec = _marginalize(c, pinfo=c["pinfo"], pgrad=c["pgrad"], delta=delta, gn_info=gn_info)
    assert _bits(base["info"], rec["info"])
    d1 = delta.reshape(T, L, NV)[:, 1]
    for t in (0, 2):
        want = base["eta"][t] - base["info"][t] @ d1[t]
        np.testing.assert_allclose(rec["eta"][t], want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
        assert not _bits(rec["eta"][t], base["eta"][t])
    assert _bits(rec["eta"][1], base["eta"][1])  # its step failed: nothing was retracted
    noinfo = _marginalize(c, pinfo=c["pinfo"], pgrad=c["pgrad"], delta=delta)  # gn_info NULL: every step counts
    assert _bits(noinfo["eta"][[0, 2]], rec["eta"][[0, 2]]) and not _bits(noinfo["eta"][1], base["eta"][1])


# ---------------------------------------------------------------- pa_window_prior_linearize
@pytest.mark.parametrize("T,L,frame", [(1, 3, 0), (70, 24, 23), (3, 5, 1)])
def test_prior_linearize_matches_reference(T, L, frame):
    rng = np.random.default_rng(T + L)
    info, eta = PR.random_spd(rng, T)
    pose, vel, angvel, _ = _problem(T, L, 3)
    fr = np.arange(T) * L + frame
    xp = np.stack([F.pack(F.compose(F.unpack(pose[f]), F.pose_exp(0.05 * rng.standard_normal(6)))) for f in fr])
    xw, xv = angvel[fr] + 0.1 * rng.standard_normal((T, 3)), vel[fr] + 0.1 * rng.standard_normal((T, 3))
    xp[0], xw[0], xv[0] = pose[fr[0]], angvel[fr[0]], vel[fr[0]]  # trajectory 0 sits at xbar
    ref_xi, ref_grad, ref_err = PR.linearize(info, eta, xp, xw, xv, pose, angvel, vel, L, frame)
    plan = pipeline.PriorPlan(T=T, L=L, device="cuda")
    for k, v in (("info", info), ("eta", eta), ("xbar_pose", xp), ("xbar_angvel", xw), ("xbar_vel", xv)):
        plan.cur[k].copy_(_dev(v))
    plan.linearize(_dev(pose), _dev(angvel), _dev(vel), frame=frame)
    torch.cuda.synchronize()
    grad, err = plan.grad.cpu().numpy(), plan.err.cpu().numpy()
    np.testing.assert_allclose(grad, ref_grad, rtol=RTOL, atol=RTOL * np.abs(ref_grad).max())
    np.testing.assert_allclose(err, ref_err, rtol=RTOL, atol=RTOL * np.abs(ref_err).max())
    np.testing.assert_allclose(grad[0], -eta[0], rtol=0, atol=1e-12 * np.abs(eta[0]).max())
    assert abs(err[0]) <= 1e-12 and not ref_xi[0].any()


# ---------------------------------------------------------------- 4b. a zero prior through the three tick forms
from test_streaming_pose_gpu import LW, _init, _keypoints, _model, _pipe, _truth  # noqa: E402


@pytest.fixture(scope="module")
def model():
    return _model()


FORMS = {"split": {}, "fused": dict(split_pose=False), "four": dict(split_pose=False)}


def _form(model, form, graph=True, **kw):
    p = _pipe(model, graph, init=_init(3), **FORMS[form], **kw)
    if form == "four":  # (as test_fused_pose_tick_matches_four_launches: the pose graph is captured on first use)
        p.fused_pose = False
    return p


@pytest.mark.parametrize("form", list(FORMS))
def test_zero_prior_equals_no_prior_in_every_tick_form(model, form):
    """The default pipeline (NULL prior pointers: the parents' code path) against the same tick
    given an all-zero prior through the _prior entry points: poses, info and the window bit for
    bit (adding 0.0 to frame 0's blocks changes nothing)."""
    a, b = _form(model, form), _form(model, form)
    assert a.prior is None and a.gn.prior is None
    zero = pipeline.PriorPlan(T=3, L=LW, device=b.dev)
    b._enqueue_prior_in = b._enqueue_prior_out = lambda *args: None  # (the prior stays zero: no marginalization)
    b.prior = b.gn.prior = zero
    b.pose_graph = None
    truth, _, _ = _truth(3, LW + 2)
    rng = np.random.default_rng(4)
    for k in range(LW + 2):
        y = _keypoints(truth[k], 0.5, rng)
        qa, ia = a.tick_keypoints(y)
        qb, ib = b.tick_keypoints(y)
        assert _bits(qa, qb) and np.array_equal(ia, ib) and (ia == 0).all(), k
    for key, v in a.window_state().items():
        np.testing.assert_array_equal(v, b.window_state()[key], err_msg=key)
    a.close()
    b.close()


# ---------------------------------------------------------------- 6. streaming
def _pose_err(pose, truth_k):
    er, et = [], []
    for c, (Rt, tt) in enumerate(truth_k):
        R, t = F.unpack(pose[c])
        er.append(np.linalg.norm(F.rot_log(Rt.T @ R)))
        et.append(np.linalg.norm(t - tt))
    return max(er), max(et)


@pytest.mark.parametrize("form", list(FORMS))
def test_streaming_marginalize(model, form):
    """L + 16 ticks of exact keypoints of test_streaming_pose_gpu's known trajectory at L = 6,
    with marginalize=True (graph replay) beside marginalize=False and beside the eager
    marginalizing pipeline.  Measured on an MI355X (all three forms alike): newest pose within
    5e-7 rad / 2e-7 m from the fifth tick on (bars 1e-4 / 1e-5, asserted on every tick from the
    one that fills the window); variance ratio with / without the prior on the same factors at
    most 0.9987 (frame 0) .. 1.0 (newest frame); newest-frame variances against the
    marginalize=False run 0.72 .. 1 + 3e-8."""
    n, ticks = 3, LW + 16
    truth, _, _ = _truth(n, ticks)
    g, e, plain = _form(model, form, marginalize=True), _form(model, form, graph=False, marginalize=True), _form(model, form)
    assert g.prior is not None and plain.prior is None
    err_r, err_t = [], []
    for k in range(ticks):
        y = _keypoints(truth[k])
        pose, info = g.tick_keypoints(y)
        plain.tick_keypoints(y)
        assert (info == 0).all(), (k, info)
        minfo = g.prior.minfo.cpu().numpy()
        assert (minfo == (2 if k + 1 < LW else 0)).all(), (k, minfo)  # tick k + 1 holds min(k + 1, L) real frames
        pe, ie = e.tick_keypoints(y)
        assert _bits(pose, pe) and np.array_equal(info, ie), k
        r, t = _pose_err(pose, truth[k])
        err_r.append(r)
        err_t.append(t)
    print("rotation error (rad) per tick:", " ".join(f"{x:.1e}" for x in err_r))
    print("translation error (m) per tick:", " ".join(f"{x:.1e}" for x in err_t))
    assert max(err_r[LW - 1:]) < 1e-4 and max(err_t[LW - 1:]) < 1e-5  # 17 ticks: no drift under the prior
    for key, v in g.window_state().items():
        np.testing.assert_array_equal(v, e.window_state()[key], err_msg=key)
    for key in ("info", "eta", "xbar_pose"):
        assert torch.equal(g.prior.nxt[key], e.prior.nxt[key]), key
    assert g.prior.nxt["info"].abs().max().item() > 0.0
    # Added information cannot widen a marginal.  Exactly so at ONE linearization: the window's
    # factors with the prior against the same factors without it, every frame, slack 1e-9.
    cm = g.window_covariance()
    same = pipeline.MarginalsPlan(g.lin, T=n, L=LW, lam=g.gn.lam)
    with torch.cuda.stream(g.stream):
        same.launch()
    g.stream.synchronize()
    assert (cm["info"] == 0).all() and (same.out["info"] == 0).all()
    dm = np.einsum("nlii->nli", cm["cov"])
    ds = np.einsum("nlii->nli", same.out["cov"].view(n, LW, 12, 12).cpu().numpy())
    print("variance ratio (with / without the prior, same factors), worst per frame:", (dm / ds).max((0, 2)))
    assert (dm <= ds * (1.0 + 1e-9)).all(), (dm / ds).max()
    assert (dm[:, 0] < ds[:, 0]).any()
    # Against the run with marginalize=False, per entry and per camera.  That run is linearized
    # at other states (its older frames lack the history; both runs sit within the keypoints' f32
    # rounding, ~1e-7 relative, of the truth), so its covariance is that of slightly different
    # factors and the inequality cannot be exact: the issue's slack of 1e-9 is missed on one
    # rotation entry whose prior contribution is nil, measured 1 + 3e-8.  Asserted at 1e-7, the
    # size of the two runs' state difference (DESIGN 5.5e records the change of bar).
    cp = plain.window_covariance()
    assert (cp["info"] == 0).all()
    dn, dp = dm[:, -1], np.einsum("nii->ni", cp["cov"][:, -1])
    print("newest-frame variance ratio (marginalize run / plain run):", (dn / dp).min(), "..", (dn / dp).max())
    assert (dn <= dp * (1.0 + 1e-7)).all(), (dn / dp).max()
    assert (dn < dp * (1.0 - 1e-3)).any()
    with pytest.raises(ValueError, match="marginal"):
        g.solve_window()
    for p in (g, e, plain):
        p.close()


def test_marginalizing_tick_forms_agree(model):
    """A non-zero prior through every tick form, on noisy keypoints past a full window: the fused
    tick and the four launches bit for bit (poses, window, the next prior), the split tick within
    test_split_pose_tick_matches_fused's bars of the fused one (another elimination order: poses
    1e-12, blocks rtol 1e-9)."""
    ticks = LW + 4
    fu, fo, sp = (_form(model, f, marginalize=True) for f in ("fused", "four", "split"))
    assert fu.fused_pose and not fu.split_pose and not fo.fused_pose and sp.split_pose
    truth, _, _ = _truth(3, ticks)
    rng = np.random.default_rng(12)
    for k in range(ticks):
        y = _keypoints(truth[k], 0.5, rng)
        (qu, iu), (qo, io), (qs, is_) = fu.tick_keypoints(y), fo.tick_keypoints(y), sp.tick_keypoints(y)
        assert (iu == 0).all() and np.array_equal(iu, io) and np.array_equal(iu, is_), k
        assert _bits(qu, qo), k
        np.testing.assert_allclose(qs, qu, rtol=0, atol=1e-12, err_msg=str(k))
    wu, wo, ws = fu.window_state(), fo.window_state(), sp.window_state()
    for key in ("pose", "vel", "angvel"):
        np.testing.assert_array_equal(wu[key], wo[key], err_msg=key)
        np.testing.assert_allclose(ws[key], wu[key], rtol=0, atol=1e-12, err_msg=key)
    assert (fu.prior.minfo == 0).all() and fu.prior.nxt["info"].abs().max().item() > 1.0
    for key in ("info", "eta", "xbar_pose", "xbar_angvel", "xbar_vel"):
        u, o, s = (p.prior.nxt[key].cpu().numpy() for p in (fu, fo, sp))
        assert _bits(u, o), key
        np.testing.assert_allclose(s, u, rtol=RTOL, atol=RTOL * np.abs(u).max(), err_msg=key)
    # and the prior does move the estimate: the same ticks without it end elsewhere
    plain = _form(model, "fused")
    rng = np.random.default_rng(12)
    for k in range(ticks):
        qp, _ = plain.tick_keypoints(_keypoints(truth[k], 0.5, rng))
    assert np.abs(qp - qu).max() > 1e-9
    for p in (fu, fo, sp, plain):
        p.close()


def test_marginalize_rejects_pre_ahead_and_no_pose_stage(model):
    from perseus_amd.streaming import StreamingPipeline

    with pytest.raises(ValueError, match="pre_ahead"):
        StreamingPipeline(model, pose_window=LW, marginalize=True, pre_ahead=True)
    with pytest.raises(ValueError, match="pose_window"):
        StreamingPipeline(model, marginalize=True)
