"""The constant-velocity factor on the angular velocity ("cw") through the solvers built on the
factor kernels (tests/test_cw_gpu.py has the kernels themselves):

  4. the streaming ticks: fused = the four launches bit for bit, the split tick within the split
     rule, graph replay = eager, and angvel_sigma=None = today's tick in every form;
  5. the LM solve against tests/cw_ref.py: decisions where the margin is >= 1e-6, state and
     cost_hist within test_lm_gpu.py's named bounds, independence of trajectories, determinism,
     the prior sibling;
  6. what the factor is for: on noisy keypoints it halves the rotation error of a long window;
  7. StreamingPipeline(angvel_sigma=..., timed=True) on the jitter / gap / drop-out stream.
"""
import numpy as np
import pytest
import torch

import cw_ref
import lm_ref
import prior_ref as PR
import timed_ref as TR
from oracle import factors_ref as F
from perseus_amd import pipeline, synth

import test_lm_gpu as TL  # tests/ is on sys.path (rootdir conftest)
import test_prior_gpu as TP
from test_streaming_pose_gpu import LW, _keypoints, _model, _pipe, _truth

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIG = lm_ref.SIGMAS
CW_SIGMA = 0.05
ISIG = np.full(3, 1.0 / CW_SIGMA)


@pytest.fixture(scope="module")
def model():
    return _model()


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


# ---------------------------------------------------------------- 4. ticks
@pytest.mark.parametrize("extra", [{}, dict(marginalize=True), dict(timed=True)], ids=["plain", "marginalize", "timed"])
def test_tick_forms_agree_with_the_factor(model, extra):
    """Noisy keypoints past a full window: the fused tick and the four launches bit for bit, the
    split tick within test_split_pose_tick_matches_fused's bars (poses 1e-12), and the factor
    shows (the same ticks without it end elsewhere)."""
    ticks = LW + 4
    fu, fo, sp, plain = (TP._form(model, f, angvel_sigma=s, **extra)
                         for f, s in (("fused", CW_SIGMA), ("four", CW_SIGMA), ("split", CW_SIGMA), ("fused", None)))
    assert fu.fused_pose and not fu.split_pose and not fo.fused_pose and sp.split_pose
    assert fu.lin["r_cw"] is not None and plain.lin.get("r_cw") is None and not plain.traj_args.r_cw
    truth, _, _ = _truth(3, ticks)
    rng = np.random.default_rng(12)
    for k in range(ticks):
        y = _keypoints(truth[k], 0.5, rng)
        (qu, iu), (qo, io), (qs, is_) = fu.tick_keypoints(y), fo.tick_keypoints(y), sp.tick_keypoints(y)
        qp, _ = plain.tick_keypoints(y)
        assert (iu == 0).all() and np.array_equal(iu, io) and np.array_equal(iu, is_), k
        assert _bits(qu, qo), k
        np.testing.assert_allclose(qs, qu, rtol=0, atol=1e-12, err_msg=str(k))
    wu, wo, ws = fu.window_state(), fo.window_state(), sp.window_state()
    for key in ("pose", "vel", "angvel"):
        np.testing.assert_array_equal(wu[key], wo[key], err_msg=key)
        np.testing.assert_allclose(ws[key], wu[key], rtol=0, atol=1e-12, err_msg=key)
    for key in ("r_cw", "err_cw"):
        assert torch.equal(fu.lin[key], fo.lin[key]), key
    assert np.abs(qp - qu).max() > 1e-9
    if extra.get("marginalize"):
        for key in ("info", "eta"):
            assert _bits(fu.prior.nxt[key].cpu().numpy(), fo.prior.nxt[key].cpu().numpy()), key
    for p in (fu, fo, sp, plain):
        p.close()


@pytest.mark.parametrize("form", list(TP.FORMS))
def test_graph_replay_equals_eager_with_the_factor(model, form):
    g, e = TP._form(model, form, angvel_sigma=CW_SIGMA), TP._form(model, form, graph=False, angvel_sigma=CW_SIGMA)
    truth, _, _ = _truth(3, LW + 2)
    rng = np.random.default_rng(4)
    for k in range(LW + 2):
        y = _keypoints(truth[k], 0.5, rng)
        (qg, ig), (qe, ie) = g.tick_keypoints(y), e.tick_keypoints(y)
        assert _bits(qg, qe) and np.array_equal(ig, ie) and (ig == 0).all(), k
    for key, v in g.window_state().items():
        np.testing.assert_array_equal(v, e.window_state()[key], err_msg=key)
    g.close()
    e.close()


@pytest.mark.parametrize("extra", [{}, dict(marginalize=True), dict(timed=True)], ids=["plain", "marginalize", "timed"])
@pytest.mark.parametrize("form", ["fused", "split"])
def test_angvel_sigma_none_is_todays_tick(model, form, extra):
    """angvel_sigma=None against the pipeline built without the keyword: the same pa_traj_args
    (the three fields NULL), the same bits."""
    a, b = TP._form(model, form, **extra), TP._form(model, form, angvel_sigma=None, **extra)
    assert not b.traj_args.r_cw and not b.traj_args.err_cw and not b.traj_args.isig_cw
    truth, _, _ = _truth(3, LW + 1)
    rng = np.random.default_rng(5)
    for k in range(LW + 1):
        y = _keypoints(truth[k], 0.5, rng)
        (qa, ia), (qb, ib) = a.tick_keypoints(y), b.tick_keypoints(y)
        assert _bits(qa, qb) and np.array_equal(ia, ib), k
    a.close()
    b.close()


# ---------------------------------------------------------------- 5. LM
def _dev(pr, T, L, params, cw=True, prior=None):
    out = pipeline.lm_solve(torch.as_tensor(pr["y"], device=DEV), pr["pose"], pr["vel"], pr["angvel"],
                            synth.CUBE_CORNERS, synth.CAMERA_K, T=T, L=L, dt=lm_ref.DT, proj_sigmas=[SIG["proj"]] * 2,
                            dyn_sigmas=[SIG["dyn"]] * 6, cv_sigmas=[SIG["cv"]] * 3,
                            cw_sigmas=[CW_SIGMA] * 3 if cw else None, prior=prior, **params)
    torch.cuda.synchronize()
    res = {k: out[k].cpu().numpy() for k in ("pose", "vel", "angvel", "cost0", "cost", "iters", "status", "lambda",
                                             "cost_hist")}
    res["lin"] = out["lin"]
    return res


def _ref(pr, T, L, params):
    return cw_ref.solve(pr["y"], pr["pose"], pr["vel"], pr["angvel"], T, L, params, isig_cw=ISIG)


@pytest.mark.parametrize("T,L", [(3, 6), (2, 24)])
def test_lm_decisions_match_reference(T, L):
    """test_lm_gpu.test_decisions_match_reference with the factor: 0.8 rad off, 8 iterations,
    decisions compared where the reference's margin is >= 1e-6, cost_hist and the
    state within test_lm_gpu's named bounds (HIST_RTOL, STATE_ATOL)."""
    pr = lm_ref.problem(T, L, 0.8)
    ref = _ref(pr, T, L, TL.PARITY)
    nok = TL._well_defined(ref, T)
    dec = [[r["accept"] for r in log] for log in ref["log"]]
    print("reference decisions:", dec, "well defined:", nok)
    assert min(nok) >= 5  # (as test_lm_gpu: a change of the problem that lowers it needs another seed)
    assert any(not a for d, n in zip(dec, nok) for a in d[:n]), "no reject among the compared decisions"
    assert any(a for d, n in zip(dec, nok) for a in d[:n]), "no accept among the compared decisions"
    dev = _dev(pr, T, L, TL.PARITY)
    for t in range(T):
        n = nok[t]
        h, g = dev["cost_hist"][t, :n + 1], ref["cost_hist"][t, :n + 1]
        dh = (np.abs(h - g) / g).max()
        print(f"trajectory {t}: {n} iterations compared, cost_hist relative deviation {dh:.3g}")
        assert dh <= TL.HIST_RTOL, (t, dh)
        np.testing.assert_array_equal(np.diff(h) < 0, dec[t][:n])
    m = min(nok)
    short = dict(TL.PARITY, max_iters=m)
    ref_m = _ref(pr, T, L, short)
    TL._assert_matches(_dev(pr, T, L, short), ref_m, T, f"cw T={T} L={L}, {m} iterations")
    # the factor outputs the solve leaves are those of the final state: one subtract, one multiply
    want = cw_ref.residual(dev["angvel"], L, ISIG)
    assert _bits(dev["lin"]["r_cw"].cpu().numpy(), want)
    np.testing.assert_allclose(dev["lin"]["err_cw"].cpu().numpy(), 0.5 * (want ** 2).sum(1), atol=1e-9, rtol=1e-12)


def test_lm_is_independent_per_trajectory_and_deterministic():
    """T = CUs + 1: trajectory T-1 is bit for bit its own T = 1 solve; two runs are bit-identical."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    T, L = cus + 1, 6
    base = lm_ref.problem(3, L, 0.3)
    idx = np.arange(T) % 3
    pr = {k: base[k].reshape(3, L, -1)[idx].reshape(T * L, -1) for k in ("y", "pose", "vel", "angvel")}
    params = dict(lm_ref.PARAMS, max_iters=6)
    a, b = _dev(pr, T, L, params), _dev(pr, T, L, params)
    for k in ("pose", "vel", "angvel", "cost", "cost_hist", "lambda"):
        assert _bits(a[k], b[k]), k
    t = T - 1
    one = {k: pr[k].reshape(T, L, -1)[t] for k in pr}
    c = _dev(one, 1, L, params)
    for k in ("pose", "vel", "angvel"):
        assert _bits(a[k].reshape(T, L, -1)[t], c[k].reshape(L, -1)), k
    for k in ("cost", "cost0", "lambda", "cost_hist"):
        assert _bits(a[k][t:t + 1], c[k]), k
    np.testing.assert_array_equal(a["iters"][t:t + 1], c["iters"])
    assert (a["iters"] > 0).all()


def test_lm_prior_sibling_runs_with_the_factor():
    T, L = 3, 6
    pr = lm_ref.problem(T, L, 0.1)
    outs = []
    for cw in (True, False):
        prior = pipeline.PriorPlan(T=T, L=L, device=DEV)
        info, _ = PR.random_spd(np.random.default_rng(11), T, 3.0)
        prior.cur["info"].copy_(torch.as_tensor(info, device=DEV))
        prior.cur["xbar_pose"].copy_(torch.as_tensor(pr["pose"].reshape(T, L, 12)[:, 0], device=DEV))
        outs.append(_dev(pr, T, L, dict(lm_ref.PARAMS, max_iters=10), cw=cw, prior=prior))
    on, off = outs
    assert (on["iters"] > 0).all() and np.isfinite(on["cost"]).all() and (on["cost"] < on["cost0"]).all()
    assert not _bits(on["angvel"], off["angvel"])
    rot, tra = lm_ref.pose_errors(on["pose"], pr["truth"])
    assert rot.max() < 1e-2 and tra.max() < 1e-2


# ---------------------------------------------------------------- 6. what it is for
FOR_SIG = dict(proj=1.0, dyn=0.02, cv=0.05)


def _noisy_problem(T, L, seed):
    """lm_ref.truth with its linear velocity scaled by min(1, 24 / L) (it leaves the image after
    about 170 frames otherwise), every corner asserted in view; 0.5 px keypoint noise; the initial
    state 0.03 rad / 3 mm off the truth per frame, velocities at the truth's."""
    rng = np.random.default_rng(5)
    w = 0.3 * rng.standard_normal((T, 3))
    v = 0.01 * rng.standard_normal((T, 3)) * min(1.0, 24.0 / L)
    cur = []
    for c in range(T):
        R0, _ = F.pose_exp(np.concatenate([0.3 * rng.standard_normal(3), np.zeros(3)]))
        cur.append((R0, np.array([0.0, 0.0, 0.35]) + 0.005 * rng.standard_normal(3)))
    tr = []
    for _ in range(L):
        tr.append(list(cur))
        cur = [F.compose(P, F.pose_exp(np.concatenate([lm_ref.DT * w[c], lm_ref.DT * (P[0].T @ v[c])])))
               for c, P in enumerate(cur)]
    y = np.stack([lm_ref.keypoints(tr[l]) for l in range(L)], 1)  # (asserts every corner in view)
    nrng = np.random.default_rng(seed)
    y = (y + (0.5 / 127.5) * nrng.standard_normal(y.shape)).astype(np.float32).reshape(T * L, -1)
    pose = np.zeros((T, L, 12))
    for t in range(T):
        for l in range(L):
            Rm, tt = tr[l][t]
            d, e = nrng.standard_normal(3), nrng.standard_normal(3)
            Rp, _ = F.pose_exp(np.concatenate([0.03 * d / np.linalg.norm(d), np.zeros(3)]))
            pose[t, l] = F.pack((Rm @ Rp, tt + 0.003 * e / np.linalg.norm(e)))
    true = np.array([[F.pack(tr[l][t]) for l in range(L)] for t in range(T)]).reshape(T * L, 12)
    return dict(y=y, pose=pose.reshape(T * L, 12), vel=np.repeat(v, L, 0), angvel=np.repeat(w, L, 0), truth=true)


def _device_lm_any_length(pr, L, cw, params):
    """Steps 1-5 of pa_trajectory_lm_solve for ONE trajectory of any length, driven from the host
    over the device's kernels (pa_trajectory_lm_solve itself stops at L = 24): linearize, the
    damped step (pa_trajectory_gn_step_cw through GNPlan), retract, linearize, compare the costs."""
    p = dict(lm_ref.PARAMS, **params)
    y = torch.as_tensor(pr["y"], device=DEV)
    kw = dict(T=1, L=L, dt=lm_ref.DT, proj_sigmas=[FOR_SIG["proj"]] * 2, dyn_sigmas=[FOR_SIG["dyn"]] * 6,
              cv_sigmas=[FOR_SIG["cv"]] * 3, cw_sigmas=[CW_SIGMA] * 3 if cw else None)

    def lin_at(x):
        a, lin = pipeline.prepare_trajectories(y, x[0], x[1], x[2], synth.CUBE_CORNERS, synth.CAMERA_K, **kw)
        pipeline.launch(a, DEV)
        c = lin["err_dyn"].sum() + lin["err_cv"].sum() + (lin["err_proj"] * (lin["status"] == 0)).sum()
        if cw:
            c = c + lin["err_cw"].sum()
        return lin, float(c)

    x = tuple(torch.as_tensor(pr[k], device=DEV).clone() for k in ("pose", "vel", "angvel"))
    lin, C = lin_at(x)
    lam = p["lambda0"]
    for _ in range(p["max_iters"]):
        plan = pipeline.GNPlan(lin, T=1, L=L, lam=lam)
        plan.launch()
        ok = int(plan.out["info"][0]) == 0
        if ok:
            d = plan.out["delta"].cpu().numpy().reshape(L, 12)
            pn, vn, wn = lm_ref.retract(x[0].cpu().numpy(), x[1].cpu().numpy(), x[2].cpu().numpy(), d)
            xn = tuple(torch.as_tensor(a, device=DEV) for a in (pn, vn, wn))
            lin_n, Cn = lin_at(xn)
        if ok and Cn < C:
            done = C - Cn <= p["rel_tol"] * C + p["abs_tol"]
            x, lin, C = xn, lin_n, Cn
            lam = max(lam / p["lambda_down"], p["lambda_min"])
            if done:
                break
        else:
            lam *= p["lambda_up"]
            if lam > p["lambda_max"]:
                break
    return x[0].cpu().numpy()


@pytest.mark.parametrize("seed", [1, 2])
def test_the_factor_halves_the_rotation_error_of_a_noisy_window(seed):
    """T = 2, L = 48, 0.5 px noise, sigmas proj 1.0 px / dyn 0.02 / cv 0.05 (/ cw 0.05 rad/s): each
    device solution's rotation RMS over the 48 frames is within 1 % of the reference solve's on the
    same data, and the reference's own on / off ratio is below 0.6 (measured 0.46 .. 0.52)."""
    T, L = 2, 48
    pr = _noisy_problem(T, L, seed)
    params = dict(max_iters=40)
    rms = {}
    for cw in (False, True):
        ref = cw_ref.solve(pr["y"], pr["pose"], pr["vel"], pr["angvel"], T, L, dict(lm_ref.PARAMS, **params),
                           isig_cw=ISIG if cw else None, sigmas=FOR_SIG)
        rr, _ = lm_ref.pose_errors(ref["pose"], pr["truth"])
        dev_pose = np.concatenate([
            _device_lm_any_length({k: v.reshape(T, L, -1)[t] for k, v in pr.items()}, L, cw, params) for t in range(T)])
        dr, _ = lm_ref.pose_errors(dev_pose, pr["truth"])
        rms[cw] = (np.sqrt((rr ** 2).mean()), np.sqrt((dr ** 2).mean()))
        print(f"seed {seed} cw={cw}: rotation RMS reference {rms[cw][0]:.4g}, device {rms[cw][1]:.4g}")
        assert abs(rms[cw][1] - rms[cw][0]) <= 0.01 * rms[cw][0], rms[cw]
    ratio = rms[True][0] / rms[False][0]
    print(f"seed {seed}: reference on / off ratio {ratio:.3f}")
    assert ratio < 0.6, ratio


# ---------------------------------------------------------------- 7. streaming
@pytest.fixture(scope="module")
def case():
    return TR.stream_case()


@pytest.mark.parametrize("marginalize", [False, True], ids=["plain", "marginalize"])
def test_timed_stream_with_the_factor(model, case, marginalize):
    """test_timed_streaming_gpu's stream (+-30 % jitter, a 3-period gap, a camera absent every 7th
    tick, single corners missing) with angvel_sigma = 0.05: info == 0 on every tick, 1e-4 rad /
    1e-5 m over the last 10 of 40 ticks (the truth's angular velocity is constant, so the factor
    agrees with it)."""
    n = 3
    p = _pipe(model, True, init=(TR.init_pose(case["truth"][0]), np.zeros((n, 3)), np.zeros((n, 3))), timed=True,
              angvel_sigma=CW_SIGMA, marginalize=marginalize)
    er, et = [], []
    last = case["y"][0].copy()
    assert len(case["y"]) == 40
    for k in range(len(case["y"])):
        y = case["y"][k].copy()
        y[~case["present"][k]] = last[~case["present"][k]]
        last = y
        pose, info = p.tick_keypoints(y, stamps=case["stamps"][k], present=case["present"][k], kp_mask=case["mask"][k])
        assert (info == 0).all(), (k, info)
        r, t = TR.newest_errors(pose, case["truth"][k])
        er.append(r)
        et.append(t)
    print("rot", " ".join(f"{e:.1e}" for e in er))
    print("tra", " ".join(f"{e:.1e}" for e in et))
    assert max(er[-10:]) < 1e-4 and max(et[-10:]) < 1e-5, (max(er[-10:]), max(et[-10:]))
    cov = p.window_covariance()
    assert (cov["info"] == 0).all() and np.isfinite(cov["cov"]).all()
    # solve_window on that window: the factor travels in the pa_traj_args (err_cw in the cost)
    lm = p.solve_window(max_iters=5, with_prior=marginalize)
    assert (lm["iters"] > 0).all() and np.isfinite(lm["cost"]).all() and (lm["cost"] <= lm["cost0"]).all()
    r, t = TR.newest_errors(p.window_state()["pose"][:, -1], case["truth"][-1])
    assert r < 1e-4 and t < 1e-5, (r, t)
    p.close()
