"""The constant-velocity factor on the ANGULAR velocity ("cw": pa_traj_args.r_cw / err_cw /
isig_cw and the _cw siblings of the entry points with explicit pointer lists) on the device,
against tests/cw_ref.py (the numpy references with the factor's rows appended).

  1. linearize: r_cw bit-exact (one subtract, one multiply), err_cw at the factors' bar, every
     other output bit for bit the launch without the factor, canaries, NULL err_cw / isig_cw;
  2. the GN step against the dense reference at test_gn_gpu.py's bars, both solver forms,
     delta-only launches, r_cw NULL = the _prior parent, L = 1, and lambda = 0 on a full window;
  3. marginals and marginalization (the bars of test_marginals_gpu.py / test_prior_gpu.py), the
     Schur identity, and the frames without keypoints that the factor makes observable.
The ticks, the LM solve and the streaming pipeline: tests/test_cw_solve_gpu.py.
"""

import numpy as np
import pytest
import torch

import cw_ref
import marginals_ref as MR
import prior_ref as PR
from perseus_amd import _lib, pipeline

import test_prior_gpu as TP  # tests/ is on sys.path (rootdir conftest)
from test_pipeline_gpu import CORNERS, KCAL, _problem

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-9                      # test_gn_gpu.RTOL, test_marginals_gpu.RTOL, test_prior_gpu.RTOL
SIG_CW = np.array([0.05, 0.08, 0.03])
ISIG = 1.0 / SIG_CW
SIGKW = dict(proj_sigmas=np.array([2.0, 2.0]), dyn_sigmas=np.full(6, 0.05), cv_sigmas=np.full(3, 0.5))  # test_gn_gpu._lin
SHAPES = [(1, 2), (3, 4), (5, 14), (2, 24), (70, 25)]  # the timed tests' (T, L)
OUT = ("r_proj", "j_proj", "err_proj", "status", "r_dyn", "j_dyn0", "j_dyn1", "j_dyn2", "j_dyn3", "err_dyn", "r_cv",
       "j_cv0", "j_cv1", "err_cv")
PAD, CANARY = 64, -7.25


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _inputs(T, L, nk, seed):
    poses, vels, angvels, _ = _problem(T, L, seed)
    y = np.random.default_rng(seed + 1).uniform(-1, 1, (T * L, 2 * nk)).astype(np.float32)
    corners = TP.CORNERS16 if nk == 16 else CORNERS[:nk]
    return poses, vels, angvels, y, corners


# ---------------------------------------------------------------- 1. linearize
@pytest.mark.parametrize("vf", ["world", "body"])
@pytest.mark.parametrize("TL,nk", list(zip(SHAPES, (8, 16, 8, 16, 8))), ids=[f"{t}x{l}" for t, l in SHAPES])
def test_linearize(TL, nk, vf):
    """(5, 14): 65 pairs, one past the 64-factor unit; (70, 25): 1680 pairs, 27 units."""
    T, L = TL
    poses, vels, angvels, y, corners = _inputs(T, L, nk, 3 * T + L)
    yd = torch.as_tensor(y, device=DEV)
    kw = dict(T=T, L=L, dt=0.1, vel_frame=vf, **SIGKW)
    a0, off = pipeline.prepare_trajectories(yd, poses, vels, angvels, corners, KCAL, **kw)
    pipeline.launch(a0, DEV)
    a1, on = pipeline.prepare_trajectories(yd, poses, vels, angvels, corners, KCAL, cw_sigmas=SIG_CW, **kw)
    m = T * (L - 1)
    want_r = (angvels.reshape(T, L, 3)[:, 1:] - angvels.reshape(T, L, 3)[:, :-1]) * ISIG
    want_e = 0.5 * (want_r ** 2).sum(-1).reshape(-1)

    def run(err=True, whiten=True):
        """One launch with r_cw / err_cw inside canary-filled allocations."""
        rb = torch.full((PAD + m * 3 + PAD,), CANARY, dtype=torch.float64, device=DEV)
        eb = torch.full((PAD + m + PAD,), CANARY, dtype=torch.float64, device=DEV)
        for k in OUT:
            if on[k] is not None:
                on[k].fill_(7 if k == "status" else CANARY)
        a1.r_cw, a1.err_cw = rb.data_ptr() + 8 * PAD, (eb.data_ptr() + 8 * PAD) if err else None
        a1.isig_cw = on["isig_cw"].data_ptr() if whiten else None
        pipeline.launch(a1, DEV)
        torch.cuda.synchronize()
        rb, eb = rb.cpu().numpy(), eb.cpu().numpy()
        assert (rb[:PAD] == CANARY).all() and (rb[PAD + m * 3:] == CANARY).all(), "r_cw canaries"
        assert (eb[:PAD] == CANARY).all() and (eb[PAD + m:] == CANARY).all(), "err_cw canaries"
        for k in OUT:  # every other output: bit for bit the launch without the factor
            if off[k] is not None:
                assert torch.equal(on[k], off[k]), k
        return rb[PAD:PAD + m * 3].reshape(T, L - 1, 3), eb[PAD:PAD + m]

    r, e = run()
    assert _bits(r, want_r)
    np.testing.assert_allclose(e, want_e, atol=1e-9, rtol=1e-12)
    r2, e2 = run(err=False)
    assert _bits(r2, want_r) and (e2 == CANARY).all()  # err_cw NULL: not written
    r3, e3 = run(whiten=False)
    assert _bits(r3, angvels.reshape(T, L, 3)[:, 1:] - angvels.reshape(T, L, 3)[:, :-1])  # isig_cw NULL: unwhitened
    np.testing.assert_allclose(e3, 0.5 * (r3 ** 2).sum(-1).reshape(-1), atol=1e-9, rtol=1e-12)


def test_linearize_single_frame_has_no_pairs():
    """L = 1 with the switch on: nothing to write, the other outputs as ever."""
    T, L, nk = 3, 1, 8
    poses, vels, angvels, y, corners = _inputs(T, L, nk, 2)
    yd = torch.as_tensor(y, device=DEV)
    a0, off = pipeline.prepare_trajectories(yd, poses, vels, angvels, corners, KCAL, T=T, L=L, dt=0.1, **SIGKW)
    pipeline.launch(a0, DEV)
    a1, on = pipeline.prepare_trajectories(yd, poses, vels, angvels, corners, KCAL, T=T, L=L, dt=0.1, **SIGKW)
    guard = torch.full((PAD,), CANARY, dtype=torch.float64, device=DEV)
    a1.r_cw = a1.err_cw = guard.data_ptr() + 8 * (PAD // 2)
    a1.isig_cw = torch.as_tensor(ISIG, device=DEV).data_ptr()
    pipeline.launch(a1, DEV)
    torch.cuda.synchronize()
    assert (guard == CANARY).all()
    for k in ("r_proj", "j_proj", "err_proj", "status"):
        assert torch.equal(on[k], off[k]), k


# ---------------------------------------------------------------- 2. the GN step
def _lin(T, L, seed, behind=(), cw=True, nk=8):
    poses, vels, angvels, y = _problem(T, L, seed, behind)
    if nk != 8:
        y = np.random.default_rng(seed + 1).uniform(-1, 1, (T * L, 2 * nk)).astype(np.float32)
    corners = TP.CORNERS16 if nk == 16 else CORNERS[:nk]
    return pipeline.linearize_trajectories(torch.as_tensor(y, device=DEV), poses, vels, angvels, corners, KCAL, T=T, L=L,
                                           dt=0.1, cw_sigmas=SIG_CW if cw else None, **SIGKW)


def _np(lin):
    f = {k: lin[k].cpu().numpy() for k in TP.KEYS}
    if lin.get("r_cw") is not None:
        f["r_cw"] = lin["r_cw"].cpu().numpy()
    return f


def _check_step(lin, T, L, lam, nk=8):
    out = pipeline.gn_step(lin, T=T, L=L, lam=lam)
    H, g, d = cw_ref.gn_step(_np(lin), T, L, nk, lam, ISIG if L > 1 else None)
    assert (out["info"].cpu().numpy() == 0).all()
    Dd, Ed = out["D"].cpu().numpy(), out["E"].cpu().numpy()
    for t in range(T):
        D, E = cw_ref.G.blocks(H[t], L)
        scale = np.abs(H[t]).max()
        np.testing.assert_allclose(Dd[t * L:(t + 1) * L], D, rtol=RTOL, atol=RTOL * scale)
        if L > 1:
            np.testing.assert_allclose(Ed[t * (L - 1):(t + 1) * (L - 1)], E, rtol=RTOL, atol=RTOL * scale)
    np.testing.assert_allclose(out["g"].cpu().numpy().reshape(T, -1), g, rtol=RTOL, atol=RTOL * np.abs(g).max())
    np.testing.assert_allclose(out["delta"].cpu().numpy().reshape(T, -1), d, rtol=1e-7, atol=1e-9 * np.abs(d).max())
    return out


@pytest.mark.parametrize("T,L,lam,behind", [(3, 5, 1e-2, ()), (2, 24, 1e-4, (7,)), (4, 1, 1e-3, ())])
def test_gn_step_matches_dense_reference(T, L, lam, behind):
    """test_gn_gpu's cases and bars.  The factor must show: the same launch without it differs."""
    lin = _lin(T, L, 5 + L, behind)
    out = _check_step(lin, T, L, lam)
    plain = pipeline.gn_step(_lin(T, L, 5 + L, behind, cw=False), T=T, L=L, lam=lam)
    if L > 1:
        assert not torch.equal(out["D"], plain["D"]) and not torch.equal(out["delta"], plain["delta"])
    else:  # no pairs: the parent, bit for bit
        for k in ("D", "g", "delta", "info"):
            assert torch.equal(out[k], plain[k]), k


@pytest.mark.parametrize("L", [2, 3, 4, 5, 7, 13, 23, 24, 25])
@pytest.mark.parametrize("variant", [64, 128], ids=["cyclic", "two-ended"])
def test_gn_step_in_both_solver_forms(L, variant):
    """test_gn_step_cyclic_reduction_and_two_ended_forms with the factor (L = 25 is past the cyclic
    reduction's limit: both variants then run the two-ended elimination)."""
    lin = _lin(3, L, 50 + L)
    L_ = _lib.lib()
    try:
        _lib.check(L_.pa_debug_gn_set_assemblers(variant))
        _check_step(lin, 3, L, 1e-3)
    finally:
        _lib.check(L_.pa_debug_gn_set_assemblers(0))


@pytest.mark.parametrize("T,L,nk", [(5, 24, 8), (70, 25, 16), (3, 4, 16)])
def test_gn_step_delta_only_and_null_switch(T, L, nk):
    lin = _lin(T, L, 17, nk=nk)
    ref = pipeline.gn_step(lin, T=T, L=L, lam=1e-3)
    plan = pipeline.GNPlan(lin, T=T, L=L, lam=1e-3)  # D, E, g NULL
    plan.launch()
    assert torch.equal(plan.out["delta"], ref["delta"]) and torch.equal(plan.out["info"], ref["info"])
    assert (ref["info"] == 0).all()
    # r_cw NULL through the sibling = pa_trajectory_gn_step_prior, with and without a prior
    raw = {k: lin[k] if k not in TP.JAC else lin[k].transpose(1, 2) for k in TP.KEYS}
    pinfo, pgrad = PR.random_spd(np.random.default_rng(3), T, 3.0)
    for pi, pg in ((None, None), (pinfo, pgrad)):
        d0, i0 = TP._gn(raw, T, L, nk, 1e-3, pi, pg)
        d1, i1 = _gn_cw(raw, T, L, nk, 1e-3, None, None, pi, pg)
        assert _bits(d0, d1) and np.array_equal(i0, i1) and (i0 == 0).all()
    d2, _ = _gn_cw(raw, T, L, nk, 1e-3, lin["r_cw"], lin["isig_cw"])
    assert _bits(d2, ref["delta"].cpu().numpy().reshape(T, L, 12))


def _gn_cw(raw, T, L, K, lam, r_cw, isig_cw, pinfo=None, pgrad=None):
    L_, p = _lib.lib(), _lib.ptr
    delta = torch.full((T * L, 12), 7.0, dtype=torch.float64, device=DEV)
    info = torch.full((T,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(int(L_.pa_trajectory_gn_workspace(T, L)), 8), dtype=torch.uint8, device=DEV)
    pi, pg = TP._dev(pinfo), TP._dev(pgrad)
    _lib.check(L_.pa_trajectory_gn_step_cw(T, L, K, *TP._fptrs(raw), p(r_cw), p(isig_cw), lam, None, None, None,
                                           p(delta), p(info), p(ws), ws.numel(), p(pi), p(pg), None), "gn cw")
    torch.cuda.synchronize()
    return delta.cpu().numpy().reshape(T, L, 12), info.cpu().numpy()


@pytest.mark.parametrize("variant", [0, 64, 128], ids=["shipped", "cyclic", "two-ended"])
def test_lambda_zero_on_a_full_window_solves(variant):
    """New ground: without the factor the last frame's angular velocity is in no factor and
    lambda = 0 fails at frame L (test_gn_step_reports_singular_trajectories); with it info == 0
    and the step is the dense reference's."""
    T, L = 2, 6
    L_ = _lib.lib()
    try:
        _lib.check(L_.pa_debug_gn_set_assemblers(variant))
        plain = pipeline.gn_step(_lin(T, L, 9, cw=False), T=T, L=L, lam=0.0)
        assert (plain["info"].cpu().numpy() == L).all()
        lin = _lin(T, L, 9)
        out = pipeline.gn_step(lin, T=T, L=L, lam=0.0)
    finally:
        _lib.check(L_.pa_debug_gn_set_assemblers(0))
    assert (out["info"].cpu().numpy() == 0).all()
    _, _, d = cw_ref.gn_step(_np(lin), T, L, 8, 0.0, ISIG)
    assert np.isfinite(d).all()
    np.testing.assert_allclose(out["delta"].cpu().numpy().reshape(T, -1), d, rtol=1e-7, atol=1e-9 * np.abs(d).max())


# ---------------------------------------------------------------- 3. marginals and marginalization
def _cw_case(name):
    """test_prior_gpu's named window plus the factor's whitened residuals of its angular velocities."""
    c = dict(TP._case(name))
    T, L = c["T"], c["L"]
    c["f"] = dict(c["f"], r_cw=cw_ref.residual(c["angvel"], L, ISIG))
    c["r_cw"], c["isig"] = TP._dev(c["f"]["r_cw"]), TP._dev(ISIG)
    return c


def _marginals_cw(raw, T, L, K, lam, r_cw, isig, pinfo=None, pgrad=None, cross=False):
    L_, p = _lib.lib(), _lib.ptr
    cov = torch.full((T * L, 12, 12), 7.0, dtype=torch.float64, device=DEV)
    crs = torch.full((T * (L - 1), 12, 12), 7.0, dtype=torch.float64, device=DEV) if cross else None
    info = torch.full((T,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(int(L_.pa_trajectory_marginals_workspace(T, L)), 8), dtype=torch.uint8, device=DEV)
    pi, pg = TP._dev(pinfo), TP._dev(pgrad)
    _lib.check(L_.pa_trajectory_marginals_cw(T, L, K, *TP._fptrs(raw), p(r_cw), p(isig), lam, p(cov), p(crs), None,
                                             p(info), p(ws), ws.numel(), p(pi), p(pg), None), "marginals cw")
    torch.cuda.synchronize()
    return (cov.cpu().numpy().reshape(T, L, 12, 12), None if crs is None else crs.cpu().numpy().reshape(T, L - 1, 12, 12),
            info.cpu().numpy())


def _marginalize_cw(c, r_cw, isig, pinfo=None, pgrad=None, raw=None):
    T, L, K = c["T"], c["L"], c["K"]
    p = _lib.ptr
    o = {"info": torch.full((T, 12, 12), 7.0, dtype=torch.float64, device=DEV),
         "eta": torch.full((T, 12), 7.0, dtype=torch.float64, device=DEV),
         "xbar_pose": torch.zeros((T, 12), dtype=torch.float64, device=DEV),
         "xbar_angvel": torch.zeros((T, 3), dtype=torch.float64, device=DEV),
         "xbar_vel": torch.zeros((T, 3), dtype=torch.float64, device=DEV),
         "minfo": torch.full((T,), -1, dtype=torch.int32, device=DEV)}
    keep = [TP._dev(pinfo), TP._dev(pgrad), TP._dev(c["pose"]), TP._dev(c["angvel"]), TP._dev(c["vel"])]
    _lib.check(_lib.lib().pa_window_marginalize_cw(
        T, L, K, *TP._fptrs(c["raw"] if raw is None else raw), p(keep[0]), p(keep[1]), p(r_cw), p(isig), c["lam"],
        None, None, None, *[p(k) for k in keep[2:]],
        *[p(o[k]) for k in ("info", "eta", "xbar_pose", "xbar_angvel", "xbar_vel", "minfo")], None), "marginalize cw")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


MCASES = ["t1_l3_k8", "t3_l24_k16", "t70_l24_k8", "t70_l25_k0"]


@pytest.mark.parametrize("name", MCASES)
def test_marginals_match_dense_inverse(name):
    """test_marginals_gpu's bar: scaled deviation |d_ij| / sqrt(ref_ii ref_jj) <= 1e-9."""
    c = _cw_case(name)
    T, L, K, lam = c["T"], c["L"], c["K"], c["lam"]
    cov, cross, info = _marginals_cw(c["raw"], T, L, K, lam, c["r_cw"], c["isig"], cross=True)
    assert (info == 0).all()
    rc, rx = cw_ref.dense_cov(c["f"], T, L, K, lam, ISIG)
    e_cov, e_cross = MR.scaled_err(cov, cross, rc, rx)
    print(f"{name}: scaled deviation cov {e_cov:.3g}, cross {e_cross:.3g}")
    assert e_cov <= RTOL and e_cross <= RTOL
    # r_cw NULL = the _prior parent, bit for bit; and the factor does change the covariance
    c0, i0 = TP._marginals(c["raw"], T, L, K, lam)
    c1, _, i1 = _marginals_cw(c["raw"], T, L, K, lam, None, None)
    assert _bits(c0, c1) and np.array_equal(i0, i1)
    assert not _bits(c0, cov)


@pytest.mark.parametrize("prior", [True, False])
@pytest.mark.parametrize("name", MCASES)
def test_marginalize_matches_reference(name, prior):
    """test_prior_gpu's bar (rtol 1e-9, atol 1e-9 x the reference block's largest entry); the
    n_kp = 0 window without an input prior at the operand-scaled bar, as there."""
    c = _cw_case(name)
    T, L, K, lam = c["T"], c["L"], c["K"], c["lam"]
    pinfo, pgrad = (c["pinfo"], c["pgrad"]) if prior else (None, None)
    ill = not prior and K == 0
    scales, gscales = PR.operand_scale(c["f"], T, L, K) if ill else (None, None)
    ref_info, ref_eta, ref_minfo = cw_ref.marginalize(c["f"], T, L, K, lam, ISIG, pinfo, pgrad)
    out = _marginalize_cw(c, c["r_cw"], c["isig"], pinfo, pgrad)
    np.testing.assert_array_equal(out["minfo"], ref_minfo)
    assert (ref_minfo == 0).all()
    TP._close_blocks(out["info"], ref_info, "info", scales)
    TP._close_blocks(out["eta"], ref_eta, "eta", gscales)
    assert _bits(out["info"], out["info"].transpose(0, 2, 1))
    # r_cw NULL = the parent, bit for bit
    par = TP._marginalize(c, pinfo=pinfo, pgrad=pgrad)
    nul = _marginalize_cw(c, None, None, pinfo, pgrad)
    for k in par:
        assert _bits(par[k].astype(np.float64), nul[k].astype(np.float64)), k
    assert not _bits(par["info"], out["info"])
    # without the factor frame 1's angular velocity gets no information from frame 0 unless the prior
    # couples them; with it the marginal carries some
    if not prior:
        assert (np.abs(par["info"][:, 6:9, 6:9]).max((1, 2)) < 1e-6 * np.abs(out["info"][:, 6:9, 6:9]).max((1, 2))).all()


@pytest.mark.parametrize("name", MCASES)
def test_schur_identity(name):
    """pa_window_marginalize's header text with the factor: the step of the L-frame window with a
    prior on frame 0, and the step of frames 1 .. L-1 alone with the prior made of frame 0."""
    c = _cw_case(name)
    T, L, K, lam = c["T"], c["L"], c["K"], c["lam"]
    d_full, i_full = _gn_cw(c["raw"], T, L, K, lam, c["r_cw"], c["isig"], c["pinfo"], c["pgrad"])
    m = _marginalize_cw(c, c["r_cw"], c["isig"], c["pinfo"], c["pgrad"])
    assert (m["minfo"] == 0).all()
    sub = TP._raw(PR.drop_frame0(c["f"], T, L, K), K)
    r_sub = TP._dev(c["f"]["r_cw"].reshape(T, L - 1, 3)[:, 1:].reshape(-1, 3))
    d_red, i_red = _gn_cw(sub, T, L - 1, K, lam, r_sub if L > 2 else None, c["isig"] if L > 2 else None,
                          m["info"], -m["eta"])
    assert (i_full == 0).all() and (i_red == 0).all(), (i_full, i_red)
    ref = cw_ref.dense_delta(c["f"], T, L, K, lam, ISIG, c["pinfo"], c["pgrad"]).reshape(T, L, 12)
    scale = np.abs(ref).max()
    np.testing.assert_allclose(d_full, ref, rtol=1e-7, atol=1e-9 * scale)
    np.testing.assert_allclose(d_red, d_full[:, 1:], rtol=1e-7, atol=1e-9 * scale)


def test_frames_without_keypoints_are_observable():
    """Frames 20-23 of an L = 48 window masked out (kp_mask = 0), lambda = 1e-9: with the factor
    info == 0 and those frames' rotation variances are finite and below 1 rad^2, the dense
    reference's to the marginals bar; without it the same variances are of order 1 / lambda."""
    T, L, nk, lam = 2, 48, 8, 1e-9
    poses, vels, angvels, y, corners = _inputs(T, L, nk, 41)
    mask = np.full((T, L), 0xFF, np.int64)
    mask[:, 20:24] = 0
    kw = dict(T=T, L=L, dt=0.1, kp_mask=mask, **SIGKW)
    yd = torch.as_tensor(y, device=DEV)
    on = pipeline.linearize_trajectories(yd, poses, vels, angvels, corners, KCAL, cw_sigmas=SIG_CW, **kw)
    off = pipeline.linearize_trajectories(yd, poses, vels, angvels, corners, KCAL, **kw)
    assert (on["status"].view(T, L, nk)[:, 20:24] == 2).all()
    m_on, m_off = pipeline.marginals(on, T=T, L=L, lam=lam), pipeline.marginals(off, T=T, L=L, lam=lam)
    assert (m_on["info"].cpu().numpy() == 0).all()
    cov = m_on["cov"].cpu().numpy().reshape(T, L, 12, 12)
    var = np.einsum("tlii->tli", cov)[:, 20:24, :3]
    assert np.isfinite(var).all() and (var > 0).all() and (var < 1.0).all(), var.max()
    ref, _ = cw_ref.dense_cov(_np(on), T, L, nk, lam, ISIG)
    e, _ = MR.scaled_err(cov, None, ref, None)
    print(f"rotation variances of the masked frames {var.min():.3g} .. {var.max():.3g}, scaled deviation {e:.3g}")
    assert e <= RTOL
    if (m_off["info"].cpu().numpy() == 0).all():  # (a failed pivot there is the other way of saying it)
        voff = np.einsum("tlii->tli", m_off["cov"].cpu().numpy().reshape(T, L, 12, 12))[:, 20:24, :3]
        assert voff.max() > 1e-3 / lam, voff.max()
