"""Robust (Huber / Cauchy) keypoint noise models on the device (pa_traj_args.robust_proj,
pa_proj_linearize_robust; pipeline's / StreamingPipeline's proj_robust, smoother.noiseModel.Robust)
against the numpy restatement tests/robust_ref.py:

  * the linearize: sqrt(w)-scaled residuals and Jacobians and err = rho on both sides of n = k,
    cheirality and nvalid rows untouched, the batched entry point and the trajectory kernel
    bit-identical, kind 0 bit-identical to args that never heard of the fields;
  * Levenberg-Marquardt on the robust cost, decision for decision (test_lm_gpu._check_decisions'
    comparison), and to convergence with the reference's error figures;
  * marginal covariances of the robust-weighted system;
  * the streaming tick in its three forms on a sequence with one corner 40 px off every fourth
    tick, against the numpy tick chain;
  * the drop-in factor class with noiseModel.Robust.

LM deviation of the device from robust_ref over this file's compared cases, measured on an MI355X
(DESIGN.md 5.5d): state 5.03e-12 (absolute, on pose entries and velocities of magnitude <= 1),
cost_hist 9.15e-15 relative; the bounds are 10 x the measured values, as test_lm_gpu.py sets its
own (7.76e-12 -> 7.76e-11 and 1.9e-9 -> 1.9e-8 for the plain solve; both figures here are below
those).  Per case, state / cost_hist: Huber 1.345 after 3 iterations 5.03e-12 / 2.5e-15 (the
iterate is still moving, the cost falling by 3e-4 to 1e-2 per step: the one case above 1e-13), to
convergence 4.47e-14 / 2.5e-15; Cauchy 1.0 after 3 iterations 5.57e-14 / 9.15e-15, to convergence
2.39e-14 / 9.15e-15.  (The plain solve's cost figure sits at its noise floor, C ~ 1e-10; the
robust costs keep the outliers' rho and stay far above it, hence the smaller relative figure.)
"""
import numpy as np
import pytest
import torch

import lm_ref  # tests/ is on sys.path (rootdir conftest)
import marginals_ref as MR
import robust_ref
from oracle import factors_ref as F
from oracle import resnet_ref as R
from perseus_amd import _lib, pipeline, smoother, synth

pytestmark = pytest.mark.gpu

ATOL = 1e-9  # tests/test_factors_gpu.py
MARGIN = 1e-6  # tests/test_lm_gpu.py: decisions the reference takes with a smaller |C' - C| / C are not compared
STATE_MEASURED, HIST_MEASURED = 5.03e-12, 9.15e-15  # worst over the cases, MI355X (see the header)
STATE_ATOL, HIST_RTOL = 10 * STATE_MEASURED, 10 * HIST_MEASURED
MARG_RTOL = 1e-9  # tests/test_marginals_gpu.py RTOL, marginals_ref.scaled_err
ROBUST = [("huber", 1.345), ("cauchy", 1.0)]
IDS = ["huber", "cauchy"]
SIG = lm_ref.SIGMAS
PARITY = dict(lm_ref.PARAMS, rel_tol=0.0, abs_tol=0.0, max_iters=8)  # tests/test_lm_gpu.py PARITY
DT3 = 1.0 / 12.0
JAC = ("j_proj", "j_dyn0", "j_dyn1", "j_dyn2", "j_dyn3", "j_cv0", "j_cv1")


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _np(lin):
    """The device's factor outputs as numpy, Jacobians (n, rows, cols)."""
    return {k: v.cpu().numpy() for k, v in lin.items() if isinstance(v, torch.Tensor)}


# ---------------------------------------------------------------- 1. linearize
LIN_SIG = dict(proj=60.0, dyn=0.1, cv=0.1)


def _lin_dev(tr, T, L, robust, nvalid=None, poses=None):
    nv = None if nvalid is None else torch.as_tensor(np.asarray(nvalid, np.int32), device="cuda")
    out = pipeline.linearize_trajectories(
        torch.as_tensor(tr["y"], device="cuda"), tr["poses"] if poses is None else poses, tr["vels"], tr["angvels"],
        tr["corners"], tr["K"], T=T, L=L, dt=DT3, proj_sigmas=[LIN_SIG["proj"]] * 2, dyn_sigmas=[LIN_SIG["dyn"]] * 6,
        cv_sigmas=[LIN_SIG["cv"]] * 3, nvalid=nv, proj_robust=robust)
    torch.cuda.synchronize()
    return _np(out)


def _lin_ref(tr, T, L, robust, nvalid=None, poses=None):
    """robust_ref's factors per trajectory, stacked as the device returns them."""
    nk = len(tr["corners"])
    P = (tr["poses"] if poses is None else poses).reshape(T, L, 12)
    y, V, W = tr["y"].reshape(T, L, -1), tr["vels"].reshape(T, L, 3), tr["angvels"].reshape(T, L, 3)
    fs = [robust_ref.apply(lm_ref.factors(y[t], P[t], V[t], W[t], L, dt=DT3, sigmas=LIN_SIG, corners=tr["corners"],
                                          K=tr["K"], nvalid=None if nvalid is None else nvalid[t]),
                           *(robust if robust is not None else (None, 0.0))) for t in range(T)]
    return {k: np.concatenate([f[k] for f in fs]) for k in fs[0]}, nk


@pytest.mark.parametrize("robust", ROBUST, ids=IDS)
@pytest.mark.parametrize("T,L,K", [(3, 5, 8), (2, 3, 5)])
def test_linearize_matches_reference(T, L, K, robust):
    """Uniform keypoints against random poses, sigma = 60 px: the whitened norms straddle
    k = 1.345 (35 of 120 and 9 of 30 at or below it), so both Huber branches run."""
    tr = synth.synthetic_trajectories(3, T, L, K)
    plain, _ = _lin_ref(tr, T, L, None)
    assert (plain["status"] == 0).all()
    n = np.sqrt((plain["r_proj"] ** 2).sum(1))
    inl = int((n <= 1.345).sum())
    print(f"T={T} L={L} K={K}: {inl} of {n.size} projections with n <= 1.345")
    assert 0.2 * n.size <= inl <= 0.8 * n.size
    ref, _ = _lin_ref(tr, T, L, robust)
    dev = _lin_dev(tr, T, L, robust)
    np.testing.assert_array_equal(dev["status"], 0)
    for k in ("r_proj", "j_proj", "err_proj"):
        d = np.abs(dev[k] - ref[k]).max()
        print(f"  {robust[0]} {k}: max deviation {d:.3g}")
        np.testing.assert_allclose(dev[k], ref[k], rtol=0, atol=ATOL, err_msg=k)
    w = robust_ref.weight(*robust, n)
    assert (w < 0.9).any() and (dev["err_proj"] <= plain["err_proj"] * (1 + 1e-12)).all()
    # the other factors do not know about it
    off = _lin_dev(tr, T, L, None)
    for k in dev:
        if not k.endswith("_proj"):
            assert _bits(dev[k], off[k]), k


@pytest.mark.parametrize("robust", ROBUST, ids=IDS)
@pytest.mark.parametrize("T,L,K", [(3, 5, 8), (2, 3, 5)])
def test_linearize_keeps_cheirality_and_nvalid_rows(T, L, K, robust):
    """One frame behind the camera (t.z < 0): NaN and status 1, as without the robust model;
    frames outside nvalid: zeros and status 2."""
    tr = synth.synthetic_trajectories(3, T, L, K)
    poses = tr["poses"].copy()
    fb = 1 * L + (L - 1)  # trajectory 1's newest frame
    poses[fb, 11] = -poses[fb, 11]
    nvalid = [L - 1] + [L] * (T - 1)
    ref, nk = _lin_ref(tr, T, L, robust, nvalid=nvalid, poses=poses)
    dev = _lin_dev(tr, T, L, robust, nvalid=nvalid, poses=poses)
    st = ref["status"].reshape(T * L, nk)
    assert (st[fb] == 1).all() and (st[0] == 2).all() and (np.delete(st, [0, fb], 0) == 0).all()
    np.testing.assert_array_equal(dev["status"], ref["status"])
    behind, masked, ok = (ref["status"] == s for s in (1, 2, 0))
    for k in ("r_proj", "j_proj", "err_proj"):
        assert np.isnan(dev[k][behind]).all(), k
        assert (dev[k][masked] == 0).all(), k
        np.testing.assert_allclose(dev[k][ok], ref[k][ok], rtol=0, atol=ATOL, err_msg=k)


@pytest.mark.parametrize("robust", ROBUST, ids=IDS)
@pytest.mark.parametrize("T,L,K", [(3, 5, 8), (2, 3, 5)])
def test_batched_entry_point_is_the_trajectory_kernel_bit_for_bit(T, L, K, robust):
    tr = synth.synthetic_trajectories(3, T, L, K)
    poses = tr["poses"].copy()
    poses[L - 1, 11] = -poses[L - 1, 11]  # a cheirality frame on both paths
    dev = _lin_dev(tr, T, L, robust, poses=poses)
    z = R.denormalize_f32(tr["y"], 256, 256).astype(np.float64).reshape(-1, 2)
    out = smoother.linearize_projection(np.repeat(poses, K, axis=0), np.tile(tr["corners"], (T * L, 1)), z, tr["K"],
                                        inv_sigma=[1.0 / LIN_SIG["proj"]] * 2, robust=robust)
    torch.cuda.synchronize()
    assert _bits(out["r"].cpu().numpy(), dev["r_proj"])
    assert _bits(out["J"].cpu().numpy(), dev["j_proj"])
    assert _bits(out["err"].cpu().numpy(), dev["err_proj"])
    assert _bits(out["status"].cpu().numpy(), dev["status"])
    assert (dev["status"] == 1).sum() == K


@pytest.mark.parametrize("T,L,K", [(3, 5, 8), (2, 3, 5)])
def test_kind_zero_is_the_plain_linearize_bit_for_bit(T, L, K):
    """robust_proj = 0 with a stray k in the struct against args whose two fields were never
    touched (a caller compiled before they existed passes zeros)."""
    tr = synth.synthetic_trajectories(3, T, L, K)
    kw = dict(T=T, L=L, dt=DT3, proj_sigmas=[LIN_SIG["proj"]] * 2, dyn_sigmas=[LIN_SIG["dyn"]] * 6,
              cv_sigmas=[LIN_SIG["cv"]] * 3)
    y = torch.as_tensor(tr["y"], device="cuda")
    outs = []
    for k in (None, 1.345):
        a, out = pipeline.prepare_trajectories(y, tr["poses"], tr["vels"], tr["angvels"], tr["corners"], tr["K"], **kw)
        assert a.robust_proj == 0 and a.robust_proj_k == 0.0
        if k is not None:
            a.robust_proj_k = k
        pipeline.launch(a, y.device)
        torch.cuda.synchronize()
        outs.append(_np(out))
    for k in outs[0]:
        assert _bits(outs[0][k], outs[1][k]), k
    on = _lin_dev(tr, T, L, ("huber", 1.345))
    assert not _bits(np.swapaxes(on["j_proj"], 1, 2), outs[0]["j_proj"])  # (and the switch does something)


# ---------------------------------------------------------------- 2. Levenberg-Marquardt
def _lm_dev(pr, params, robust, **kw):
    T, L = robust_ref.LM_T, robust_ref.LM_L
    out = pipeline.lm_solve(torch.as_tensor(pr["y"], device="cuda"), pr["pose"], pr["vel"], pr["angvel"],
                            synth.CUBE_CORNERS, synth.CAMERA_K, T=T, L=L, dt=lm_ref.DT,
                            proj_sigmas=[SIG["proj"]] * 2, dyn_sigmas=[SIG["dyn"]] * 6, cv_sigmas=[SIG["cv"]] * 3,
                            proj_robust=robust, **kw, **params)
    torch.cuda.synchronize()
    res = {k: out[k].cpu().numpy() for k in ("pose", "vel", "angvel", "cost0", "cost", "iters", "status", "lambda",
                                             "cost_hist")}
    res["out"] = out
    return res


def _deviation(dev, ref):
    ds = max(np.abs(dev[k] - ref[k]).max() for k in ("pose", "vel", "angvel"))
    h, g = dev["cost_hist"], ref["cost_hist"]
    np.testing.assert_array_equal(np.isnan(h), np.isnan(g))
    ok = ~np.isnan(g)
    return ds, (np.abs(h[ok] - g[ok]) / g[ok]).max()


@pytest.fixture(scope="module")
def lm_pr():
    return robust_ref.lm_problem()


@pytest.mark.parametrize("robust", ROBUST, ids=IDS)
def test_lm_decisions_match_reference(lm_pr, robust):
    """The outlier problem, rel_tol = abs_tol = 0, 8 iterations: cost_hist per trajectory up to the
    first decision the reference takes with margin < 1e-6, then a second solve of as many
    iterations as every trajectory decides with that margin, compared in full."""
    T, L = robust_ref.LM_T, robust_ref.LM_L
    ref = robust_ref.solve(lm_pr, T, L, PARITY, robust)
    nok = []
    for t in range(T):
        m = [r["margin"] >= MARGIN for r in ref["log"][t]]
        nok.append(m.index(False) if False in m else len(m))
    dec = [[r["accept"] for r in log] for log in ref["log"]]
    print("reference decisions:", dec, "well defined:", nok)
    assert min(nok) >= 3
    dev = _lm_dev(lm_pr, PARITY, robust)
    worst_h = 0.0
    for t in range(T):
        n = nok[t]
        h, g = dev["cost_hist"][t, :n + 1], ref["cost_hist"][t, :n + 1]
        dh = (np.abs(h - g) / g).max()
        worst_h = max(worst_h, dh)
        print(f"{robust[0]} trajectory {t}: {n} iterations compared, cost_hist relative deviation {dh:.3g}")
        np.testing.assert_array_equal(np.diff(h) < 0, dec[t][:n])  # the same accepts and rejects
    m = min(nok)
    short = dict(PARITY, max_iters=m)
    ref_m = robust_ref.solve(lm_pr, T, L, short, robust)
    for t in range(T):
        assert all(r["margin"] >= MARGIN for r in ref_m["log"][t])
    dev_m = _lm_dev(lm_pr, short, robust)
    np.testing.assert_array_equal(dev_m["iters"], ref_m["iters"])
    np.testing.assert_array_equal(dev_m["status"], ref_m["status"])
    np.testing.assert_array_equal(dev_m["lambda"], ref_m["lambda"])
    ds, dh = _deviation(dev_m, ref_m)
    print(f"{robust[0]}, {m} iterations: state deviation {ds:.3g}, cost_hist relative deviation {dh:.3g}")
    assert worst_h <= HIST_RTOL, worst_h
    assert ds <= STATE_ATOL and dh <= HIST_RTOL, (ds, dh)
    for t in range(T):
        assert dev_m["cost0"][t] == dev_m["cost_hist"][t, 0] and dev_m["cost"][t] == dev_m["cost_hist"][t, m]


@pytest.mark.parametrize("robust", ROBUST, ids=IDS)
def test_lm_converges_with_the_reference_error_figures(lm_pr, robust):
    """60 iterations allowed: CONVERGED in the reference's number of steps; the worst rotation /
    translation error against the truth is the reference's (0.119 rad / 8.4e-3 m Huber, 5.5e-3 rad /
    3.3e-4 m Cauchy, where the plain solve is left 0.704 rad / 4.6e-2 m off).  A pose entry moves
    the rotation error by at most 3 x and the translation error by sqrt(3) x its own deviation:
    the figures agree within 10 x the state bound."""
    T, L = robust_ref.LM_T, robust_ref.LM_L
    ref = robust_ref.solve(lm_pr, T, L, robust_ref.LM_PARAMS, robust)
    assert (ref["status"] == lm_ref.CONVERGED).all()
    dev = _lm_dev(lm_pr, robust_ref.LM_PARAMS, robust)
    assert (dev["status"] == _lib.LM_CONVERGED).all(), dev["status"]
    np.testing.assert_array_equal(dev["iters"], ref["iters"])
    (rd, td), (rr, tr_) = lm_ref.pose_errors(dev["pose"], lm_pr["truth"]), lm_ref.pose_errors(ref["pose"], lm_pr["truth"])
    ds, dh = _deviation(dev, ref)
    print(f"{robust[0]}: iters {dev['iters']}, {rd.max():.3g} rad, {td.max():.3g} m (reference {rr.max():.3g}, "
          f"{tr_.max():.3g}); state deviation {ds:.3g}, cost_hist relative deviation {dh:.3g}")
    assert abs(rd.max() - rr.max()) <= 10 * STATE_ATOL and abs(td.max() - tr_.max()) <= 10 * STATE_ATOL
    assert ds <= STATE_ATOL and dh <= HIST_RTOL, (ds, dh)
    # the cost is the sum of rho: err_proj of the final linearization, summed as the device sums it
    lin = _np(dev["out"]["lin"])
    cost = lin["err_dyn"].reshape(T, -1).sum(1) + lin["err_cv"].reshape(T, -1).sum(1) + lin["err_proj"].reshape(T, -1).sum(1)
    np.testing.assert_allclose(cost, dev["cost"], rtol=1e-12)


# ---------------------------------------------------------------- 3. marginals
@pytest.mark.parametrize("robust", ROBUST, ids=IDS)
def test_marginals_of_the_robust_weighted_system(lm_pr, robust):
    """lm_solve(proj_robust, covariance=True): cov is the dense inverse of the robust-weighted
    reference factors (robust_ref at the state the solve returned) + lam I."""
    T, L, lam = robust_ref.LM_T, robust_ref.LM_L, 1e-6
    dev = _lm_dev(lm_pr, robust_ref.LM_PARAMS, robust, covariance=True, cov_lambda=lam)
    assert (dev["out"]["cov_info"].cpu().numpy() == 0).all()
    y = lm_pr["y"].reshape(T, L, -1)
    P, V, W = (dev[k].reshape(T, L, -1) for k in ("pose", "vel", "angvel"))
    fs = [robust_ref.factors(*robust)(y[t], P[t], V[t], W[t], L) for t in range(T)]
    ref = {k: np.concatenate([f[k] for f in fs]) for k in fs[0]}
    ref_cov, _ = MR.dense(ref, T, L, 8, lam)
    e_cov, _ = MR.scaled_err(dev["out"]["cov"].cpu().numpy(), None, ref_cov, None)
    plain = {k: np.concatenate([lm_ref.factors(y[t], P[t], V[t], W[t], L)[k] for t in range(T)]) for k in fs[0]}
    e_plain, _ = MR.scaled_err(dev["out"]["cov"].cpu().numpy(), None, MR.dense(plain, T, L, 8, lam)[0], None)
    print(f"{robust[0]}: scaled deviation {e_cov:.3g} (from the plain system's covariance: {e_plain:.3g})")
    assert e_cov <= MARG_RTOL, e_cov
    assert e_plain > 1e-3  # the down-weighted outliers widen it


# ---------------------------------------------------------------- 4. streaming
@pytest.fixture(scope="module")
def model():
    from perseus_amd.detector import KeypointCNN

    m = KeypointCNN(num_channels=4)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synthetic_state_dict(0).items()})
    return m


@pytest.fixture(scope="module")
def sequence():
    return robust_ref.stream_sequence()


@pytest.fixture(scope="module")
def chain_worst(sequence):
    truth, ys = sequence
    return robust_ref.stream_chain(truth, ys, ("cauchy", 1.0))[-12:].max()


def _pipe(model, graph=True, robust=("cauchy", 1.0), **kw):
    from perseus_amd.streaming import StreamingPipeline

    return StreamingPipeline(model, n_cams=robust_ref.ST_N, graph=graph, pose_window=robust_ref.ST_L,
                             proj_robust=robust, **kw)


def _drive(p, sequence):
    truth, ys = sequence
    errs = []
    for k, y in enumerate(ys):
        pose, info = p.tick_keypoints(y)
        assert (info == 0).all(), (k, info)
        errs.append(robust_ref.newest_rot_errors(pose, truth[k]))
    return np.array(errs)


def test_streaming_tick_forms_agree(model, sequence):
    """The split tick, the fused tick and the four-launch chain on the outlier sequence with
    Cauchy(1.0), graph replays: fused == four launches bit for bit
    (test_fused_pose_tick_matches_four_launches), split == fused to f64 rounding
    (test_split_pose_tick_matches_fused's tolerances), info == 0 on every tick."""
    sp, fu, fo = _pipe(model), _pipe(model, split_pose=False), _pipe(model, split_pose=False)
    assert sp.split_pose and fu.fused_pose and not fu.split_pose
    fo.fused_pose = False
    assert sp.traj_args.robust_proj == _lib.ROBUST_CAUCHY and sp.traj_args.robust_proj_k == 1.0
    _, ys = sequence
    for k, y in enumerate(ys):
        (qs, ins), (qf, inf_), (qo, ino) = (p.tick_keypoints(y) for p in (sp, fu, fo))
        assert (ins == 0).all() and (inf_ == 0).all() and (ino == 0).all(), k
        assert _bits(qf, qo), k
        wf, wo, ws = fu.window_state(), fo.window_state(), sp.window_state()
        for key in wf:
            assert _bits(wf[key], wo[key]), (k, key)
        for key, v in fu.lin.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(v, fo.lin[key]), (k, key)
        assert torch.equal(fu.gn.out["delta"], fo.gn.out["delta"])
        np.testing.assert_allclose(qs, qf, rtol=0, atol=1e-12)
        np.testing.assert_array_equal(ws["y"], wf["y"])
        for key in ("pose", "vel", "angvel"):
            np.testing.assert_allclose(ws[key], wf[key], rtol=0, atol=1e-12, err_msg=key)
        for key, v in sp.lin.items():
            if isinstance(v, torch.Tensor):
                if k == 0 or key == "status":
                    assert torch.equal(v, fu.lin[key]), (k, key)
                else:
                    torch.testing.assert_close(v, fu.lin[key], rtol=1e-9, atol=1e-12, msg=f"{k} {key}")
        ds, df = sp.gn.out["delta"], fu.gn.out["delta"]
        assert (ds - df).abs().max().item() <= 1e-9 * df.abs().max().item(), k
    for p in (sp, fu, fo):
        p.close()


@pytest.mark.parametrize("pre_ahead", [False, True])
def test_streaming_holds_the_pose_through_outliers(model, sequence, chain_worst, pre_ahead):
    """Worst newest-pose rotation error over the last 12 of the 40 ticks: within 10 % of the numpy
    chain's (5.5e-4 rad; the chains differ by rounding only)."""
    p = _pipe(model, pre_ahead=pre_ahead)
    assert p.split_pose and p.pre_ahead == pre_ahead and p.pose_graph is None
    worst = _drive(p, sequence)[-12:].max()
    assert p.pose_graph is not None  # (every tick after the capture was a replay)
    print(f"pre_ahead={pre_ahead}: worst rotation error {worst:.4g} rad, numpy chain {chain_worst:.4g} rad")
    assert abs(worst - chain_worst) <= 0.1 * chain_worst
    assert chain_worst <= 1.1e-3
    # the inherited consumers run on the robust window too
    res = p.solve_window(max_iters=10)
    assert set(res["status"].tolist()) <= {_lib.LM_CONVERGED, _lib.LM_MAX_ITERS, _lib.LM_STALLED}
    assert (res["cost"] <= res["cost0"]).all()
    assert (p.window_covariance()["info"] == 0).all()
    p.close()


def test_plain_streaming_is_dragged_by_the_outliers(model, sequence):
    p = _pipe(model, robust=None)
    assert p.traj_args.robust_proj == 0
    worst = _drive(p, sequence)[-12:].max()
    print(f"plain pipeline: worst rotation error {worst:.3g} rad")
    assert worst > 0.1
    p.close()


# ---------------------------------------------------------------- 5. drop-in classes
@pytest.mark.parametrize("robust", ROBUST, ids=IDS)
def test_dropin_factor_with_a_robust_noise_model(robust):
    """KeypointProjectionFactor with noiseModel.Robust: error(v) = rho and linearize(v) the
    sqrt(w)-scaled (A, b), an inlier and an outlier measurement."""
    kind, k = robust
    nm = smoother.noiseModel
    est = (nm.mEstimator.Huber if kind == "huber" else nm.mEstimator.Cauchy).Create(k)
    noise = nm.Robust.Create(est, nm.Isotropic.Sigma(2, 2.0))
    pose = F.pose_exp(np.array([0.2, -0.1, 0.3, 0.01, -0.02, 0.35]))
    v = smoother.Values()
    v.insert("x", smoother.Pose3(*pose))
    pb = synth.CUBE_CORNERS[2]
    r0, J0, st, _ = F.projection(pose, pb, np.zeros(2), synth.CAMERA_K)
    assert st == 0
    for off in (np.array([0.5, -1.0]), np.array([40.0, 3.0])):
        z = r0 - off  # the measurement that leaves the residual `off`
        f = smoother.KeypointProjectionFactor("x", noise, smoother.Cal3_S2(*synth.CAMERA_K), z, pb)
        rw = off / 2.0
        n = np.sqrt(rw @ rw)
        sw = np.sqrt(robust_ref.weight(kind, k, n))
        assert (n <= k) == (off[0] < 1)
        assert abs(f.error(v) - float(robust_ref.loss(kind, k, n))) <= ATOL
        A, b = f.linearize(v)
        np.testing.assert_allclose(b, -sw * rw, rtol=0, atol=ATOL)
        np.testing.assert_allclose(A[0], sw * J0 / 2.0, rtol=0, atol=ATOL)
        np.testing.assert_allclose(f.unwhitenedError(v), off, rtol=0, atol=ATOL)
        plain = smoother.KeypointProjectionFactor("x", nm.Isotropic.Sigma(2, 2.0), smoother.Cal3_S2(*synth.CAMERA_K),
                                                  z, pb)
        assert abs(plain.error(v) - 0.5 * n * n) <= ATOL
