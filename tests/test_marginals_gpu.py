"""pa_trajectory_marginals (pipeline.marginals / MarginalsPlan, lm_solve(covariance=True),
StreamingPipeline.window_covariance) on the device against the dense inverse
np.linalg.inv(H + lam I) built from the device's own whitened factors (tests/marginals_ref.py).

Metric: marginals_ref.scaled_err, per entry |delta_ij| / sqrt(ref_ii ref_jj); bound RTOL = 1e-9,
the GN tests' RTOL (the device inverts by the sweep operator with a Newton-refined reciprocal,
not by LAPACK; the numpy recursion itself agrees with the dense inverse to 1.2e-11 or better,
test_marginals_ref.py).
"""
import functools

import numpy as np
import pytest
import torch

import lm_ref  # tests/ is on sys.path (rootdir conftest)
import marginals_ref as MR
from perseus_amd import pipeline, synth

from test_gn_gpu import _lin, _np
from test_pipeline_gpu import CORNERS

pytestmark = pytest.mark.gpu
RTOL = 1e-9
SIG = lm_ref.SIGMAS
NK = len(CORNERS)
JAC = ("j_proj", "j_dyn0", "j_dyn1", "j_dyn2", "j_dyn3", "j_cv0", "j_cv1")


def _lm_lin(T, L, nvalid=None, pending=False, seed=5):
    """The device's factors of a lm_ref.problem window (0.1 rad off the truth); nvalid: that many
    measured frames per window; pending: the newest frame's projection factors carry status 3."""
    pr = lm_ref.problem(T, L, 0.1, seed=seed)
    nv = None if nvalid is None else torch.full((T,), nvalid, dtype=torch.int32, device="cuda")
    lin = pipeline.linearize_trajectories(torch.as_tensor(pr["y"], device="cuda"), pr["pose"], pr["vel"],
                                          pr["angvel"], synth.CUBE_CORNERS, synth.CAMERA_K, T=T, L=L, dt=lm_ref.DT,
                                          proj_sigmas=[SIG["proj"]] * 2, dyn_sigmas=[SIG["dyn"]] * 6,
                                          cv_sigmas=[SIG["cv"]] * 3, nvalid=nv)
    if pending:
        lin["status"].view(T, L, -1)[:, -1] = 3
    return lin


@functools.lru_cache(maxsize=None)
def _case(name):
    """(lin, T, L, lam) of a named window; built once and shared, never modified."""
    if name == "full2":
        return _lin(3, 2, 7), 3, 2, 1e-3
    if name == "full5":
        return _lin(3, 5, 10), 3, 5, 1e-9
    if name == "full24":
        return _lin(2, 24, 29, behind=(7,)), 2, 24, 1e-3
    if name == "nvalid3":
        return _lm_lin(2, 8, nvalid=3), 2, 8, 1e-2
    if name == "pending":
        return _lm_lin(2, 8, pending=True), 2, 8, 1e-2
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _dense(name):
    lin, T, L, lam = _case(name)
    return MR.dense(_np(lin), T, L, NK, lam)


def _run(lin, T, L, lam, **kw):
    plan = pipeline.MarginalsPlan(lin, T=T, L=L, lam=lam, **kw)
    plan.launch()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in plan.out.items()}


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("name", ["full2", "full5", "full24", "nvalid3", "pending"])
def test_cov_and_cross_match_dense_inverse(name):
    """Worst scaled deviation measured on an MI355X (cov / cross):
    full2 (3 x 2, lam 1e-3) 2.04e-13 / 2.45e-13, full5 (3 x 5, lam 1e-9) 1.41e-13 / 5.71e-13,
    full24 (2 x 24, lam 1e-3, frame 7 behind the camera) 2.17e-13 / 8.77e-13,
    nvalid3 (2 x 8, lam 1e-2) 1.48e-13 / 1.44e-13, pending (2 x 8, lam 1e-2) 5.43e-14 / 1.56e-13:
    worst 8.8e-13, three orders inside the bound."""
    lin, T, L, lam = _case(name)
    ref_cov, ref_cross = _dense(name)
    out = _run(lin, T, L, lam, cross=True)
    assert (out["info"] == 0).all(), out["info"]
    e_cov, e_cross = MR.scaled_err(out["cov"], out["cross"], ref_cov, ref_cross)
    print(f"{name}: T={T} L={L} lam={lam:g}: scaled deviation cov {e_cov:.3g}, cross {e_cross:.3g}")
    assert e_cov <= RTOL and e_cross <= RTOL, (name, e_cov, e_cross)


# ---------------------------------------------------------------- bit identity, symmetry
@pytest.mark.parametrize("name", ["full2", "full24", "nvalid3"])
def test_output_forms_are_bit_identical(name):
    """cov_newest alone is cov's last block, and cov does not depend on whether cross or
    cov_newest is written too."""
    lin, T, L, lam = _case(name)
    both = _run(lin, T, L, lam, cross=True)
    only = _run(lin, T, L, lam)
    newest = _run(lin, T, L, lam, full=False, newest=True)
    allof = _run(lin, T, L, lam, cross=True, newest=True)
    assert set(only) == {"cov", "info"} and set(newest) == {"cov_newest", "info"}
    assert _bits(only["cov"], both["cov"]) and _bits(allof["cov"], both["cov"]) and _bits(allof["cross"], both["cross"])
    last = both["cov"].reshape(T, L, 12, 12)[:, L - 1]
    assert _bits(newest["cov_newest"], last) and _bits(allof["cov_newest"], last)
    assert (newest["info"] == 0).all() and (only["info"] == 0).all()


@pytest.mark.parametrize("name", ["full5", "full24", "pending"])
def test_blocks_are_exactly_symmetric_with_positive_diagonal(name):
    lin, T, L, lam = _case(name)
    out = _run(lin, T, L, lam, newest=True)
    assert (out["info"] == 0).all()
    for key in ("cov", "cov_newest"):
        c = out[key]
        assert _bits(c, c.transpose(0, 2, 1)), key
        assert (np.einsum("nii->ni", c) > 0).all(), key


# ---------------------------------------------------------------- singular input
def test_lambda_zero_fails_at_the_last_frame():
    """lam = 0 on a full window: the last frame's angular velocity is in no factor (as
    test_gn_step_reports_singular_trajectories pins for the step)."""
    lin, T, L, _ = _case("full5")
    out = _run(lin, T, L, 0.0, cross=True, newest=True)
    assert (out["info"] == L).all(), out["info"]
    for key in ("cov", "cross", "cov_newest"):
        assert np.isnan(out[key]).all(), key
    newest = _run(lin, T, L, 0.0, full=False, newest=True)
    assert (newest["info"] == L).all() and np.isnan(newest["cov_newest"]).all()


def test_failed_trajectory_leaves_its_neighbour_untouched():
    """One launch with a failing trajectory 0 (its frame-1 dynamics Jacobian is NaN, so no pivot
    of frame 1 passes the positive-definite test) beside a good trajectory 1, and a second launch
    on the clean factors: trajectory 1's blocks are the same bits in both."""
    lin, T, L, lam = _case("full5")
    clean = _run(lin, T, L, lam, cross=True)
    bad = dict(lin)
    bad["j_dyn0"] = lin["j_dyn0"].transpose(1, 2).contiguous().clone()  # (the column-major buffer)
    bad["j_dyn0"][1] = float("nan")  # trajectory 0, pair (1, 2)
    out = _run(bad, T, L, lam, cross=True)
    assert out["info"][0] == 2 and (out["info"][1:] == 0).all(), out["info"]
    cov, cross = out["cov"].reshape(T, L, 12, 12), out["cross"].reshape(T, L - 1, 12, 12)
    assert np.isnan(cov[0]).all() and np.isnan(cross[0]).all()
    assert _bits(cov[1:], clean["cov"].reshape(T, L, 12, 12)[1:])
    assert _bits(cross[1:], clean["cross"].reshape(T, L - 1, 12, 12)[1:])


# ---------------------------------------------------------------- monotone in information
def test_more_measurements_never_raise_the_newest_pose_covariance():
    """The same window with every frame measured and with only the newest one (nvalid = 1), at
    lam = 1e-2: H_full = H_1 + (a positive semi-definite term), so the newest frame's pose block
    obeys Sigma_full <= Sigma_1 in the Loewner order.  Bound: eigenvalues of the difference
    >= -1e-12 x the largest eigenvalue of Sigma_1 (f64 rounding of blocks of that size)."""
    T, L, lam = 2, 8, 1e-2
    full = _run(_lm_lin(T, L), T, L, lam, full=False, newest=True)
    one = _run(_lm_lin(T, L, nvalid=1), T, L, lam, full=False, newest=True)
    assert (full["info"] == 0).all() and (one["info"] == 0).all()
    for t in range(T):
        a, b = full["cov_newest"][t, :6, :6], one["cov_newest"][t, :6, :6]
        ev = np.linalg.eigvalsh(b - a)
        scale = np.linalg.eigvalsh(b).max()
        print(f"trajectory {t}: eigenvalues of the difference / scale {ev / scale}")
        assert (ev >= -1e-12 * scale).all(), (t, ev, scale)
        assert ev.max() > 0.0  # (and the two windows are not the same one)


# ---------------------------------------------------------------- more trajectories than CUs
def _slice(lin, t, T):
    """Trajectory t's factors as views of the T-trajectory arrays."""
    out = {}
    for k, v in lin.items():
        if isinstance(v, torch.Tensor):
            per = v.shape[0] // T
            out[k] = v[t * per:(t + 1) * per]
    return out


def test_more_trajectories_than_cus():
    """T = CUs + 1, L = 4: every trajectory's blocks are bit for bit those of the launch of that
    trajectory alone (one workgroup per trajectory, no state shared between them)."""
    T, L, lam = torch.cuda.get_device_properties(0).multi_processor_count + 1, 4, 1e-3
    lin = _lm_lin(T, L)
    out = _run(lin, T, L, lam, cross=True)
    assert (out["info"] == 0).all()
    cov, cross = out["cov"].reshape(T, L, 12, 12), out["cross"].reshape(T, L - 1, 12, 12)
    assert not _bits(cov[0], cov[T - 1])
    plan = None
    for t in range(T):
        one = _slice(lin, t, T)
        if plan is None:
            plan = pipeline.MarginalsPlan(one, T=1, L=L, lam=lam, cross=True)
        plan.lin = one
        plan.launch()
        torch.cuda.synchronize()
        assert plan.out["info"].item() == 0
        assert _bits(plan.out["cov"].cpu().numpy(), cov[t]), t
        assert _bits(plan.out["cross"].cpu().numpy(), cross[t]), t


# ---------------------------------------------------------------- determinism, graph
def test_deterministic_and_graph_replay():
    lin, T, L, lam = _case("full24")
    plan = pipeline.MarginalsPlan(lin, T=T, L=L, lam=lam, cross=True, newest=True)
    runs = []
    for _ in range(2):
        for v in plan.out.values():
            v.zero_()
        plan.launch()
        torch.cuda.synchronize()
        runs.append({k: v.cpu().numpy() for k, v in plan.out.items()})
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.launch()
    for v in plan.out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    runs.append({k: v.cpu().numpy() for k, v in plan.out.items()})
    for other in runs[1:]:
        for k in ("cov", "cross", "cov_newest"):
            assert _bits(runs[0][k], other[k]), k
        assert np.array_equal(runs[0]["info"], other["info"])
    assert (runs[0]["info"] == 0).all() and np.isfinite(runs[0]["cov"]).all()


# ---------------------------------------------------------------- lm_solve(covariance=True)
def test_lm_solve_with_covariance():
    T, L = 3, 6
    pr = lm_ref.problem(T, L, 0.1)

    def solve(**kw):
        out = pipeline.lm_solve(torch.as_tensor(pr["y"], device="cuda"), pr["pose"], pr["vel"], pr["angvel"],
                                synth.CUBE_CORNERS, synth.CAMERA_K, T=T, L=L, dt=lm_ref.DT,
                                proj_sigmas=[SIG["proj"]] * 2, dyn_sigmas=[SIG["dyn"]] * 6,
                                cv_sigmas=[SIG["cv"]] * 3, **lm_ref.PARAMS, **kw)
        torch.cuda.synchronize()
        return out

    plain, withcov = solve(), solve(covariance=True, cov_lambda=1e-6)
    assert "cov" not in plain and "cov_info" not in plain
    for k in ("pose", "vel", "angvel", "cost0", "cost", "iters", "status", "lambda"):
        assert torch.equal(plain[k], withcov[k]), k
    assert torch.equal(plain["cost_hist"].nan_to_num(-1.0), withcov["cost_hist"].nan_to_num(-1.0))
    assert (withcov["cov_info"].cpu().numpy() == 0).all()
    m = pipeline.marginals(withcov["lin"], T=T, L=L, lam=1e-6)
    torch.cuda.synchronize()
    assert torch.equal(withcov["cov"], m["cov"]) and tuple(m["cov"].shape) == (T * L, 12, 12)
    dflt = solve(covariance=True)  # cov_lambda = 1e-9
    m9 = pipeline.marginals(dflt["lin"], T=T, L=L, lam=1e-9)
    torch.cuda.synchronize()
    assert torch.equal(dflt["cov"], m9["cov"]) and not torch.equal(dflt["cov"], withcov["cov"])
    assert (dflt["cov_info"].cpu().numpy() == 0).all()
    assert (dflt["cov"].diagonal(dim1=1, dim2=2) > 0).all()


# ---------------------------------------------------------------- streaming
@pytest.fixture(scope="module")
def model():
    from perseus_amd.detector import KeypointCNN

    m = KeypointCNN(num_channels=4)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synthetic_state_dict(0).items()})
    return m


@pytest.mark.parametrize("pre_ahead", [False, True])
def test_streaming_window_covariance(model, pre_ahead):
    """After a few ticks on exact keypoints: shapes, info = 0, parity with the dense inverse of
    the factors the pipeline holds (pipe.lin), and with pre_ahead the predicted newest frame
    (no keypoints yet) is less certain than the measured one before it."""
    from perseus_amd.streaming import StreamingPipeline

    n, Lw, ticks, lam = 3, 6, 4, 1e-2
    truth, _, _ = lm_ref.truth(n, ticks + 1)
    p = StreamingPipeline(model, graph=True, pose_window=Lw, init_pose=lm_ref.problem(n, 1, 0.05)["pose"],
                          init_vel=np.zeros((n, 3)), init_angvel=np.zeros((n, 3)), proj_sigma=SIG["proj"],
                          dyn_sigma=SIG["dyn"], cv_sigma=SIG["cv"], lam=lam, pre_ahead=pre_ahead)
    assert p.pre_ahead == pre_ahead
    p.reset_window()
    for k in range(ticks):
        _, info = p.tick_keypoints(lm_ref.keypoints(truth[k]))
        assert (info == 0).all()
    res = p.window_covariance()
    assert res["cov"].shape == (n, Lw, 12, 12) and res["info"].shape == (n,)
    assert (res["info"] == 0).all(), res["info"]
    f = {k: (p.lin[k].transpose(1, 2) if k in JAC else p.lin[k]).cpu().numpy()
         for k in ("r_proj", "status", "r_dyn", "r_cv", *JAC)}
    if pre_ahead:
        assert (f["status"].reshape(n, Lw, -1)[:, -1] == 3).all()
    ref_cov, ref_cross = MR.dense(f, n, Lw, model.n_keypoints, lam)
    e_cov, _ = MR.scaled_err(res["cov"], None, ref_cov, ref_cross)
    print(f"pre_ahead={pre_ahead}: scaled deviation {e_cov:.3g}")
    assert e_cov <= RTOL
    other = p.window_covariance(lam=1e-1)  # another prior: another answer, smaller everywhere on the diagonal
    d0, d1 = np.einsum("nlii->nli", res["cov"]), np.einsum("nlii->nli", other["cov"])
    assert (d1 < d0).all()
    if pre_ahead:  # summed variance of the rotation and of the translation part
        for part in (slice(0, 3), slice(3, 6)):
            new, prev = d0[:, Lw - 1, part].sum(1), d0[:, Lw - 2, part].sum(1)
            assert (new > prev).all(), (new, prev)
    _, info = p.tick_keypoints(lm_ref.keypoints(truth[ticks]))  # the tick goes on as before
    assert (info == 0).all()
    p.close()

    q = StreamingPipeline(model, graph=False)
    with pytest.raises(RuntimeError, match="pose stage"):
        q.window_covariance()
    q.close()
