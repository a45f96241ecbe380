"""Config 3: keypoint forward + per-frame factor linearize, fused on the GPU.

The reference chains these through the host: `KeypointCNN.forward` (models.py:34-40)
-> `.cpu()` -> kornia `denormalize_pixel_coordinates` (validate.py:144-153) -> one
GTSAM `KeypointProjectionFactor` per keypoint (factors.py:182-275) plus one
`PoseDynamicsFactor` (factors.py:8-142) and one `ConstantVelocityFactor`
(factors.py:145-171) per consecutive frame pair, each evaluated through a Python
callback.  Here the detector output never leaves HBM: `pa_trajectory_linearize`
reads it directly, denormalizes in-kernel and evaluates every factor of T
trajectories x L frames in ONE launch on the detector's stream.

Layout (all device, f64 unless noted):
  y        (T*L, 2K) f32   detector output, frame f = t*L + l
  poses    (T*L, 12)       body pose per frame (R row-major, t)
  vels     (T*L, 3)        linear velocity in `vel_frame`
  angvels  (T*L, 3)        body angular velocity
  corners  (K, 3)          keypoints in the body frame
Outputs (factor order: projection f*K + k; dynamics / const-vel t*(L-1) + l):
  proj: r (n,2), J (n,2,6), err (n,), status (n,) int32 (1 = cheirality)
  dyn:  r (m,6), J0 (m,6,6), J1 (m,6,3), J2 (m,6,3), J3 (m,6,6), err (m,)
  cv:   r (m,3), J0 (m,3,3), J1 (m,3,3), err (m,)
Jacobians are whitened (A = H / sigma) and residuals r / sigma when sigmas are given,
matching GTSAM's JacobianFactor (b = -r).
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib


def _f64(a, dev, shape=None):
    if a is None:
        return None
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, np.float64))
    t = t.to(device=dev, dtype=torch.float64).contiguous()
    if shape is not None:
        t = t.reshape(shape)
    return t


def _mask(a, dev, shape):
    """Keypoint masks (one bit per keypoint, bit k = keypoint k) as a contiguous int32 device
    tensor, the 32 bits of each word as given (values up to 2**32 - 1 are taken as unsigned)."""
    if isinstance(a, torch.Tensor) and a.dtype == torch.int32:
        return a.to(device=dev).contiguous().reshape(shape)
    m = np.asarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).astype(np.int64).astype(np.uint32)
    return torch.as_tensor(m.view(np.int32), device=dev).contiguous().reshape(shape)


def _isig(sigmas, dim, dev):
    if sigmas is None:
        return None
    s = np.broadcast_to(np.asarray(sigmas, np.float64).reshape(-1), (dim,))
    return torch.as_tensor(1.0 / s, device=dev).contiguous()


def _empty(dev):
    """e(*shape, dtype=f64): an uninitialised tensor on dev."""
    def e(*shape, dtype=torch.float64):
        return torch.empty(shape, dtype=dtype, device=dev)
    return e


def _vel_code(vel_frame: str) -> int:
    if vel_frame not in ("world", "body"):
        raise AssertionError("vel_frame must be 'world' or 'body'.")  # factors.py:41
    return _lib.VEL_WORLD if vel_frame == "world" else _lib.VEL_BODY


def _factor_args(lin: dict, T: int, L: int, n_kp: int) -> tuple:
    """(T, L, n_kp, then the 11 factor-output pointers) as pa_trajectory_gn_step_cw, pa_trajectory_marginals_cw
    and pa_window_marginalize_cw take them first (projection outputs may be absent with n_kp = 0)."""
    return (T, L, n_kp) + tuple(_lib.ptr(lin.get(k)) for k in (
        "r_proj", "j_proj", "status", "r_dyn", "j_dyn0", "j_dyn1", "j_dyn2", "j_dyn3", "r_cv", "j_cv0", "j_cv1"))


def _entry(base: str, lin: dict, prior) -> str:
    """The name of the narrowest C entry point that takes these arguments: what an error is reported
    under.  The call itself goes to the widest sibling, whose NULL arguments make it the narrower ones."""
    return base + ("_cw" if lin.get("r_cw") is not None else "_prior" if prior is not None else "")


def prepare_trajectories(y: torch.Tensor, poses, vels, angvels, corners, K, *, T: int, L: int, dt: float,
                         vel_frame: str = "world", camera_pose=None, H: int = 256, W: int = 256,
                         proj_sigmas=None, dyn_sigmas=None, cv_sigmas=None, jacobians: bool = True,
                         nvalid: torch.Tensor | None = None, proj_robust=None, dt_pair=None, kp_mask=None,
                         cw_sigmas=None):
    """Stage inputs on the device and allocate outputs: returns (args, out).  `args`
    (a pa_traj_args) can be launched repeatedly with `launch(args, device)`; `out`
    holds the output tensors (Jacobians as (n, cols, rows) column-major buffers) and
    keeps every staged input alive.  nvalid (optional, int32 (T,) on the device, read at
    every launch): frames with a measurement, counted from the window's end; the projection
    factors of the others get status 2 and zero residual / Jacobian (the GN step skips them).
    proj_robust: None, ("huber", k) or ("cauchy", k), k in whitened units: GTSAM's
    noiseModel.Robust on the projection factors (r_proj and j_proj sqrt(w)-scaled, err_proj the
    m-estimator's loss; pa_traj_args.robust_proj); every consumer of the outputs (gn_step,
    marginals, lm_solve, the streaming ticks) then does IRLS unchanged.
    dt_pair (optional, (T, L-1) seconds): the dynamics factor of frame pair (l, l+1) of trajectory
    t uses dt_pair[t, l] instead of dt (pa_traj_args.dt_pair).  kp_mask (optional, (T, L) ints):
    bit k set = keypoint k of that frame was measured; the projection factors of cleared bits get
    status 2 and zero residual / Jacobian, as nvalid's (pa_traj_args.kp_mask; K <= 32).  Arrays
    are staged; a device tensor of the right type (f64 / int32, contiguous) is used in place and
    read at every launch.  Both are in out["dt_pair"] / out["kp_mask"] and kept alive.
    cw_sigmas (optional, 3 or one value, rad/s): switches on the ConstantVelocityFactor on the
    ANGULAR velocity of every frame pair (pa_traj_args.r_cw): out["r_cw"] (T*(L-1), 3) and
    out["err_cw"] (T*(L-1),), whitened, and out["isig_cw"]; GNPlan, MarginalsPlan, PriorPlan.marginalize,
    LMPlan and the streaming ticks honour the factor when `out` / `args` carry it.  None: off."""
    if y.device.type != "cuda":
        raise RuntimeError("linearize_trajectories expects the detector output on the GPU (no CPU fallback)")
    vel_code = _vel_code(vel_frame)
    dev = y.device
    F = T * L
    y = y.to(torch.float32).contiguous()
    if y.dim() != 2 or y.shape[0] != F or y.shape[1] % 2:
        raise ValueError(f"y must be (T*L, 2K) = ({F}, 2K), got {tuple(y.shape)}")
    nk = y.shape[1] // 2
    P = _f64(poses, dev, (F, 12))
    V = _f64(vels, dev, (F, 3))
    Wv = _f64(angvels, dev, (F, 3))
    Cn = _f64(corners, dev, (nk, 3))
    Kt = _f64(K, dev, (5,))
    Tc = _f64(camera_pose, dev, (12,))
    isp, isd, isc = _isig(proj_sigmas, 2, dev), _isig(dyn_sigmas, 6, dev), _isig(cv_sigmas, 3, dev)
    isw = _isig(cw_sigmas, 3, dev)
    n, m = F * nk, T * max(L - 1, 0)
    e = _empty(dev)
    out = {"r_proj": e(n, 2), "status": e(n, dtype=torch.int32), "err_proj": e(n) if isp is not None or proj_robust is not None else None,
           "r_dyn": e(m, 6), "err_dyn": e(m) if isd is not None else None,
           "r_cv": e(m, 3), "err_cv": e(m) if isc is not None else None}
    for k, shp in _JAC.items():
        out[k] = e(*((n, m)[shp[0]],) + shp[1:]) if jacobians else None

    a = _lib.TrajArgs()
    a.T, a.L, a.n_kp, a.H, a.W = T, L, nk, H, W
    a.y, a.pose, a.vel, a.angvel, a.corners, a.K = (t.data_ptr() for t in (y, P, V, Wv, Cn, Kt))
    a.tcam = _lib.ptr(Tc)
    a.dt = float(dt)
    a.vel_frame = vel_code
    a.isig_proj, a.isig_dyn, a.isig_cv = _lib.ptr(isp), _lib.ptr(isd), _lib.ptr(isc)
    if isw is not None:  # the factor on the angular velocity: r_cw is its switch
        out["r_cw"], out["err_cw"], out["isig_cw"] = e(m, 3), e(m), isw
        a.isig_cw, a.r_cw, a.err_cw = isw.data_ptr(), out["r_cw"].data_ptr(), out["err_cw"].data_ptr()
    if nvalid is not None and (nvalid.device != dev or nvalid.dtype != torch.int32 or nvalid.numel() != T
                               or not nvalid.is_contiguous()):
        raise RuntimeError(f"nvalid must be a contiguous int32 ({T},) tensor on {dev}")
    a.nvalid = _lib.ptr(nvalid)
    a.robust_proj, a.robust_proj_k = _lib.robust_code(proj_robust)
    dtp = None if dt_pair is None else _f64(dt_pair, dev, (T, max(L - 1, 0)))
    msk = None if kp_mask is None else _mask(kp_mask, dev, (T, L))
    if msk is not None and nk > 32:
        raise ValueError(f"kp_mask holds one bit per keypoint: n_kp {nk} > 32")
    a.dt_pair, a.kp_mask = _lib.ptr(dtp), _lib.ptr(msk)
    out["dt_pair"], out["kp_mask"] = dtp, msk
    for k in ("r_proj", "err_proj", "status", "r_dyn", "err_dyn", "r_cv", "err_cv", *_JAC):
        setattr(a, k, _lib.ptr(out[k]))
    out["_keep"] = (y, P, V, Wv, Cn, Kt, Tc, isp, isd, isc, nvalid, dtp, msk, isw)  # inputs stay alive until the stream drains
    return a, out


# column-major per factor: (0 = proj rows / 1 = dyn,cv rows, cols, rows)
_JAC = {"j_proj": (0, 6, 2), "j_dyn0": (1, 6, 6), "j_dyn1": (1, 3, 6), "j_dyn2": (1, 3, 6), "j_dyn3": (1, 6, 6),
        "j_cv0": (1, 3, 3), "j_cv1": (1, 3, 3)}


def launch(args, device) -> None:
    """One pa_trajectory_linearize launch on `device`'s current stream."""
    with torch.cuda.device(device):
        _lib.check(_lib.lib().pa_trajectory_linearize(C.byref(args), _lib.stream_of(device)),
                   "pa_trajectory_linearize")


def linearize_trajectories(y: torch.Tensor, poses, vels, angvels, corners, K, *, T: int, L: int, dt: float,
                           **kw) -> dict:
    """All factors of T trajectories x L frames from the detector output `y` (device).
    Keywords as `prepare_trajectories`; Jacobians are returned as (n, rows, cols) views."""
    a, out = prepare_trajectories(y, poses, vels, angvels, corners, K, T=T, L=L, dt=dt, **kw)
    launch(a, y.device)
    for k in _JAC:
        if out[k] is not None:
            out[k] = out[k].transpose(1, 2)
    return out


def detect_and_linearize(model, x: torch.Tensor, poses, vels, angvels, corners, K, *, T: int, L: int, dt: float,
                         **kw) -> dict:
    """Config 3 end to end: `model(x)` then `linearize_trajectories` on the same stream;
    the keypoints stay in HBM between the two launches."""
    y = model(x)
    out = linearize_trajectories(y, poses, vels, angvels, corners, K, T=T, L=L, dt=dt, H=model.H, W=model.W, **kw)
    out["y"] = y
    return out


class GNPlan:
    """One damped Gauss-Newton / LM step per trajectory (SURVEY.md 8f.4,
    pa_trajectory_gn_step) over `lin` = the outputs of prepare_trajectories /
    linearize_trajectories run with whitening sigmas and Jacobians, with every output and
    the workspace allocated once, so `launch` can be captured in a HIP graph and replayed
    (the streaming pose stage).  out: delta (T*L,12), info (T,) int32 (0 = solved), and
    with blocks=True also the normal-matrix blocks D (T*L,12,12), E (T*(L-1),12,12) and
    g (T*L,12) (blocks=False: they stay on chip, the launch writes delta and info only).
    Variable block per frame: [pose (6) | angvel (3) | vel (3)].
    prior (optional, a PriorPlan): the marginalization prior on frame 0, its current Lambda and
    the gradient its last linearize() left (pa_trajectory_gn_step_prior)."""

    def __init__(self, lin: dict, *, T: int, L: int, lam: float = 0.0, blocks: bool = False, prior=None):
        if lin.get("j_proj") is None:
            raise RuntimeError("gn_step needs the Jacobians (linearize with jacobians=True)")
        dev = lin["r_proj"].device
        self.T, self.L, self.lam, self.lin, self.prior = T, L, float(lam), lin, prior
        self.n_kp = lin["r_proj"].shape[0] // (T * L) if T * L else 0
        m = T * max(L - 1, 0)
        self.m = m
        e = _empty(dev)
        self.out = {"delta": e(T * L, 12), "info": e(T, dtype=torch.int32)}
        if blocks:
            self.out.update(D=e(T * L, 12, 12), E=e(max(m, 1), 12, 12), g=e(T * L, 12))
        L_ = _lib.lib()
        self.ws = torch.empty(max(int(L_.pa_trajectory_gn_workspace(T, L)), 8), dtype=torch.uint8, device=dev)
        self.dev = dev

    def launch(self) -> None:
        """One pa_trajectory_gn_step on the device's current stream."""
        lin, out, p, pr = self.lin, self.out, _lib.ptr, self.prior
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().pa_trajectory_gn_step_cw(
                *_factor_args(lin, self.T, self.L, self.n_kp), p(lin.get("r_cw")), p(lin.get("isig_cw")), self.lam,
                p(out.get("D")), p(out.get("E")), p(out.get("g")), p(out["delta"]), p(out["info"]), p(self.ws),
                self.ws.numel(), p(pr.info) if pr else None, p(pr.grad) if pr else None, _lib.stream_of(self.dev)),
                _entry("pa_trajectory_gn_step", lin, pr))


def gn_step(lin: dict, *, T: int, L: int, lam: float = 0.0) -> dict:
    """One damped Gauss-Newton / LM step per trajectory on the device (SURVEY.md 8f.4,
    pa_trajectory_gn_step) from `linearize_trajectories(...)` run with whitening sigmas and
    Jacobians.  Returns D (T*L,12,12), E (T*(L-1),12,12), g (T*L,12), delta (T*L,12) and
    info (T,) int32 (0 = solved).  Variable block per frame: [pose (6) | angvel (3) | vel (3)]."""
    plan = GNPlan(lin, T=T, L=L, lam=lam, blocks=True)
    plan.launch()
    out = dict(plan.out)
    out["E"] = out["E"][:plan.m]
    out["_ws"] = plan.ws
    return out


class MarginalsPlan:
    """Marginal covariances of every trajectory (pa_trajectory_marginals: what
    gtsam.Marginals(graph, values).marginalCovariance(key) gives on the host) over `lin` = the
    whitened factor outputs GNPlan takes: Sigma = (J^T J + lam I)^-1 per trajectory.  Outputs
    and workspace are allocated once, so `launch` can be captured in a HIP graph and replayed.
    out: info (T,) int32 (0, or the 1-based frame of a failed pivot block: that trajectory's
    blocks are NaN); full=True: cov (T*L,12,12), the marginal covariance of each frame's
    [pose (6, right perturbation, [omega; v]) | angvel (3) | vel (3)]; cross=True (needs full):
    cross (T*(L-1),12,12) = Sigma_{l,l+1}, frame l on rows; newest=True: cov_newest (T,12,12),
    bit for bit cov's last block per trajectory (alone, only the forward elimination runs).
    lam = 0 fails on a full window (the last frame's angular velocity is in no factor): pass a
    small lam (1e-9) for the undamped covariance.
    prior (optional, a PriorPlan): the marginalization prior on frame 0; its current Lambda joins
    frame 0's block (pa_trajectory_marginals_prior)."""

    def __init__(self, lin: dict, *, T: int, L: int, lam: float, full: bool = True, cross: bool = False,
                 newest: bool = False, prior=None):
        if lin.get("j_proj") is None:
            raise RuntimeError("marginals needs the Jacobians (linearize with jacobians=True)")
        if not (full or newest):
            raise ValueError("MarginalsPlan: nothing to compute (full=False and newest=False)")
        if cross and not full:
            raise ValueError("MarginalsPlan: cross=True needs full=True")
        dev = lin["r_proj"].device
        self.T, self.L, self.lam, self.lin, self.dev, self.prior = T, L, float(lam), lin, dev, prior
        self.n_kp = lin["r_proj"].shape[0] // (T * L) if T * L else 0
        e = _empty(dev)
        self.out = {"info": e(T, dtype=torch.int32)}
        if full:
            self.out["cov"] = e(T * L, 12, 12)
        if cross:
            self.out["cross"] = e(T * max(L - 1, 0), 12, 12)
        if newest:
            self.out["cov_newest"] = e(T, 12, 12)
        n = int(_lib.lib().pa_trajectory_marginals_workspace(T, L))
        self.ws = torch.empty(max(n, 8), dtype=torch.uint8, device=dev)

    def launch(self) -> None:
        """One pa_trajectory_marginals on the device's current stream."""
        lin, out, p, pr = self.lin, self.out, _lib.ptr, self.prior
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().pa_trajectory_marginals_cw(
                *_factor_args(lin, self.T, self.L, self.n_kp), p(lin.get("r_cw")), p(lin.get("isig_cw")), self.lam,
                p(out.get("cov")), p(out.get("cross")), p(out.get("cov_newest")), p(out["info"]), p(self.ws),
                self.ws.numel(), p(pr.info) if pr else None, p(pr.grad) if pr else None, _lib.stream_of(self.dev)),
                _entry("pa_trajectory_marginals", lin, pr))


def marginals(lin: dict, *, T: int, L: int, lam: float, cross: bool = False) -> dict:
    """Marginal covariances on the device (pa_trajectory_marginals, MarginalsPlan): cov
    (T*L,12,12) = the diagonal blocks of (J^T J + lam I)^-1 over the whitened factors `lin`, info
    (T,) int32 (0 = computed) and, with cross=True, cross (T*(L-1),12,12) = Sigma_{l,l+1}."""
    plan = MarginalsPlan(lin, T=T, L=L, lam=lam, cross=cross)
    plan.launch()
    out = dict(plan.out)
    out["_ws"] = plan.ws
    return out


class PriorPlan:
    """The fixed-lag marginalization prior of T trajectory windows (include/perseus_amd.h "fixed-lag
    marginalization"): what GTSAM's BatchFixedLagSmoother keeps of the states that left the lag,
    a linear prior on the oldest frame, instead of the window forgetting them.  Buffers (device,
    f64, allocated once so both launches can be captured in a HIP graph): the CURRENT prior info
    (T,12,12), eta (T,12), xbar_pose (T,12), xbar_angvel / xbar_vel (T,3); the NEXT one (`nxt`,
    the same keys) that marginalize() writes; grad (T,12) and err (T,) of linearize(); minfo (T,)
    int32 of marginalize() (0 computed, 1 H not positive definite, 2 window not full: the next
    prior is then zero).  A new plan holds the zero prior (no information)."""

    def __init__(self, *, T: int, L: int, device):
        self.T, self.L, self.dev = T, L, torch.device(device)

        def z(*shape, dtype=torch.float64):
            return torch.zeros(shape, dtype=dtype, device=self.dev)

        def buf():  # one allocation per prior, so advance() is one copy
            flat = z(T * 174)
            b, o = {"_flat": flat}, 0
            for k, shape in (("info", (T, 12, 12)), ("eta", (T, 12)), ("xbar_pose", (T, 12)), ("xbar_angvel", (T, 3)),
                             ("xbar_vel", (T, 3))):
                n = int(np.prod(shape))
                b[k] = flat[o:o + n].view(shape)
                o += n
            b["xbar_pose"][:, (0, 4, 8)] = 1.0  # identity rotation
            return b

        self.cur, self.nxt = buf(), buf()
        self.grad, self.err, self.minfo = z(T, 12), z(T), z(T, dtype=torch.int32)

    @property
    def info(self):
        return self.cur["info"]

    def zero(self) -> None:
        """Back to the zero prior (current stream); xbar too goes back to the identity, so that
        whatever state an earlier marginalization copied there (a NaN would survive the product
        with a zero Lambda) is gone."""
        for b in (self.cur, self.nxt):
            b["_flat"].zero_()
            b["xbar_pose"][:, (0, 4, 8)] = 1.0
        self.grad.zero_()
        self.err.zero_()
        self.minfo.zero_()

    def linearize(self, pose, angvel, vel, *, frame: int) -> None:
        """pa_window_prior_linearize on the current stream: grad, err of the current prior at
        window frame `frame` of pose (T*L,12) / angvel / vel (T*L,3)."""
        p, c = _lib.ptr, self.cur
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().pa_window_prior_linearize(
                self.T, self.L, int(frame), p(c["info"]), p(c["eta"]), p(c["xbar_pose"]), p(c["xbar_angvel"]),
                p(c["xbar_vel"]), p(pose), p(angvel), p(vel), p(self.grad), p(self.err), _lib.stream_of(self.dev)),
                "pa_window_prior_linearize")

    def marginalize(self, lin: dict, pose, angvel, vel, *, lam: float, delta=None, gn_info=None, nvalid=None,
                    n_kp: int | None = None) -> None:
        """pa_window_marginalize on the current stream: frame 0 of the whitened factors `lin`,
        with the current prior and the gradient linearize() left, becomes the NEXT prior (on
        frame 1, xbar = frame 1 of pose / angvel / vel as they stand); delta (T*L,12) with gn_info:
        the step the window was retracted by since `lin` was linearized.  advance() then makes
        the next prior the current one."""
        p, c, n = _lib.ptr, self.cur, self.nxt
        if n_kp is None:
            n_kp = lin["r_proj"].shape[0] // (self.T * self.L) if self.T * self.L and lin.get("r_proj") is not None else 0
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().pa_window_marginalize_cw(
                *_factor_args(lin, self.T, self.L, n_kp), p(c["info"]), p(self.grad), p(lin.get("r_cw")),
                p(lin.get("isig_cw")), float(lam), p(delta), p(gn_info), p(nvalid), p(pose), p(angvel), p(vel),
                p(n["info"]), p(n["eta"]), p(n["xbar_pose"]), p(n["xbar_angvel"]), p(n["xbar_vel"]), p(self.minfo),
                _lib.stream_of(self.dev)), _entry("pa_window_marginalize", lin, None))

    def advance(self) -> None:
        """The next prior becomes the current one: one device copy on the current stream (capturable;
        the buffers keep their addresses, so a captured graph and pa_traj_args stay valid)."""
        self.cur["_flat"].copy_(self.nxt["_flat"])


LM_DEFAULTS = dict(max_iters=30, lambda0=1e-3, lambda_up=10.0, lambda_down=10.0, lambda_min=1e-12, lambda_max=1e12,
                   rel_tol=1e-6, abs_tol=1e-9)


class LMPlan:
    """Levenberg-Marquardt per trajectory on the device (pa_trajectory_lm_solve: what a GTSAM
    LevenbergMarquardtOptimizer.optimize() call does for the reference's users) over `args`, `lin`
    = prepare_trajectories(...) run with all three whitening sigmas and Jacobians.  Outputs and
    workspace are allocated once, so `launch` (1 + 2 max_iters kernel launches, no host
    synchronisation) can be captured in a HIP graph and replayed.  The state arrays `args`
    points at (pose, vel, angvel) are updated in place to the final accepted state and `lin`
    then holds the linearization there.  out: cost0, cost, lambda (T,) f64, iters, status (T,)
    int32 (_lib.LM_CONVERGED / LM_MAX_ITERS / LM_STALLED), cost_hist (T, max_iters + 1) f64 (NaN
    after a trajectory's stop).  Keywords: the fields of pa_lm_params (LM_DEFAULTS).
    newest_pending: the window is the one the split tick's pre half leaves between ticks (frame
    L-1 predicted, its keypoints not in yet): its projection factors stay out (pa_window_lm_solve).
    prior (optional, a PriorPlan): the marginalization prior on frame 0 (pa_trajectory_lm_prior_solve /
    pa_window_lm_prior_solve): its current Lambda, eta and xbar enter the cost and every step, and
    after launch() prior.grad / prior.err hold its gradient and cost at the solved frame 0, the
    prior_grad_in PriorPlan.marginalize consumes with `lin`."""

    def __init__(self, args, lin: dict, *, T: int, L: int, newest_pending: bool = False, prior=None, **params):
        unknown = set(params) - set(LM_DEFAULTS)
        if unknown:
            raise TypeError(f"LMPlan: unknown parameters {sorted(unknown)}")
        if lin.get("j_proj") is None:
            raise RuntimeError("lm_solve needs the Jacobians (prepare_trajectories with jacobians=True)")
        if any(lin.get(k) is None for k in ("err_proj", "err_dyn", "err_cv")):
            raise RuntimeError("lm_solve needs proj_sigmas, dyn_sigmas and cv_sigmas (the cost is whitened)")
        p = dict(LM_DEFAULTS, **params)
        self.params = _lib.LMParams(int(p["max_iters"]), *(float(p[k]) for k in (
            "lambda0", "lambda_up", "lambda_down", "lambda_min", "lambda_max", "rel_tol", "abs_tol")))
        dev = lin["r_proj"].device
        self.args, self.lin, self.T, self.L, self.dev = args, lin, T, L, dev
        self.max_iters = int(p["max_iters"])
        self.newest_pending = bool(newest_pending)
        self.prior = prior
        if prior is not None and (prior.T, prior.L) != (T, L):
            raise ValueError(f"LMPlan: the prior is for T {prior.T}, L {prior.L}, the solve for T {T}, L {L}")
        e = _empty(dev)
        self.out = {"cost0": e(T), "cost": e(T), "lambda": e(T), "iters": e(T, dtype=torch.int32),
                    "status": e(T, dtype=torch.int32), "cost_hist": e(T, max(self.max_iters, 0) + 1)}
        size = _lib.lib().pa_trajectory_lm_workspace if prior is None else _lib.lib().pa_trajectory_lm_prior_workspace
        n = int(size(T, L, int(args.n_kp), self.max_iters))
        self.ws = torch.empty(max(n, 16), dtype=torch.uint8, device=dev)

    def _prior_struct(self):
        """The pa_lm_prior of self.prior as its buffers stand (they keep their addresses)."""
        p, c = _lib.ptr, self.prior.cur
        return _lib.LMPrior(p(c["info"]), p(c["eta"]), p(c["xbar_pose"]), p(c["xbar_angvel"]), p(c["xbar_vel"]),
                            p(self.prior.grad), p(self.prior.err))

    def launch(self) -> None:
        """One pa_trajectory_lm_solve on the device's current stream."""
        o, p = self.out, _lib.ptr
        pr = None if self.prior is None else C.byref(self._prior_struct())
        what = f"pa_{'window' if self.newest_pending else 'trajectory'}_lm_{'' if pr is None else 'prior_'}solve"
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().pa_window_lm_prior_solve(
                C.byref(self.args), C.byref(self.params), int(self.newest_pending), pr, p(o["cost0"]), p(o["cost"]),
                p(o["iters"]), p(o["status"]), p(o["lambda"]), p(o["cost_hist"]), p(self.ws), self.ws.numel(),
                _lib.stream_of(self.dev)), what)


def lm_solve(y: torch.Tensor, poses, vels, angvels, corners, K, *, T: int, L: int, dt: float, proj_sigmas, dyn_sigmas,
             cv_sigmas, nvalid: torch.Tensor | None = None, vel_frame: str = "world", camera_pose=None, H: int = 256,
             W: int = 256, newest_pending: bool = False, covariance: bool = False, cov_lambda: float = 1e-9,
             proj_robust=None, prior=None, dt_pair=None, kp_mask=None, cw_sigmas=None, **params) -> dict:
    """Smoothed trajectories: Levenberg-Marquardt over all factors of T trajectories x L frames
    from the keypoints `y` (device) and the initial state, on the device (pa_trajectory_lm_solve;
    layouts as linearize_trajectories, the inputs are not modified).  Returns pose (T*L, 12),
    vel, angvel (T*L, 3) at the final accepted state, cost0, cost, iters, status, lambda (T,),
    cost_hist (T, max_iters + 1), and `lin`: the factor outputs at that state.  newest_pending: frame
    L-1 has no keypoints yet and its projection factors stay out (pa_window_lm_solve).  **params:
    max_iters, lambda0, lambda_up, lambda_down, lambda_min, lambda_max, rel_tol, abs_tol.
    covariance=True: also cov (T*L, 12, 12) and cov_info (T,), the marginal covariances
    (pipeline.marginals) of the linearization the solve leaves at the final state, with
    lam = cov_lambda (partly filled or pending windows need about 1e-2, see MarginalsPlan).
    proj_robust: as prepare_trajectories; the cost is then the sum of the m-estimator's losses and
    the covariance that of the sqrt(w)-weighted system at the final state.
    prior (a PriorPlan): the marginalization prior on frame 0 (LMPlan); its grad / err are updated, and
    the covariance then has its Lambda in frame 0's block.
    dt_pair, kp_mask: as prepare_trajectories (a frame without any measured keypoint is held by its
    dynamics factors alone; its rotation is then not observable unless cw_sigmas is given, see
    include/perseus_amd.h).  cw_sigmas: as prepare_trajectories, the ConstantVelocityFactor on the angular
    velocity; it enters the cost, every step and the covariance."""
    dev = y.device
    P, V, Wv = (_f64(a, dev).clone() for a in (poses, vels, angvels))  # updated in place: never the caller's
    a, lin = prepare_trajectories(y, P, V, Wv, corners, K, T=T, L=L, dt=dt, vel_frame=vel_frame,
                                  camera_pose=camera_pose, H=H, W=W, proj_sigmas=proj_sigmas, dyn_sigmas=dyn_sigmas,
                                  cv_sigmas=cv_sigmas, nvalid=nvalid, proj_robust=proj_robust, dt_pair=dt_pair,
                                  kp_mask=kp_mask, cw_sigmas=cw_sigmas)
    P, V, Wv = lin["_keep"][1:4]
    plan = LMPlan(a, lin, T=T, L=L, newest_pending=newest_pending, prior=prior, **params)
    plan.launch()
    out = dict(plan.out)
    out.update(pose=P, vel=V, angvel=Wv, lin=lin, _ws=plan.ws)
    if covariance:
        mp = MarginalsPlan(lin, T=T, L=L, lam=cov_lambda, prior=prior)
        mp.launch()
        out.update(cov=mp.out["cov"], cov_info=mp.out["info"], _cov_ws=mp.ws)
    return out


def window_advance(y_new: torch.Tensor, win: dict, *, dt: float, vel_frame: str = "world",
                   nvalid: torch.Tensor | None = None, dt_new=None, mask_new=None) -> None:
    """pa_window_advance on the device's current stream: every trajectory's window
    (win: y (T, L, 2K) f32, pose (T, L, 12), angvel / vel (T, L, 3) f64) moves one frame,
    y_new (T, 2K) becomes its last frame, whose pose is predicted by the
    PoseDynamicsFactor model (factors.py:100-105).  nvalid (optional, int32 (T,)): the
    window's count of real frames, += 1 up to L (pa_window_advance_n).
    dt_new (f64 (T,) device tensor or address): the window carries per-pair periods in win["dt"]
    (T, L-1) f64; they move with it, dt_new[t] becomes the new last pair's and predicts the new
    frame.  mask_new (int32 (T,) device tensor or address): the same for the keypoint masks
    win["mask"] (T, L) int32 (pa_window_advance_t; either ring alone is fine)."""
    T, L, ny = win["y"].shape
    dev = win["y"].device
    if dt_new is not None or mask_new is not None:
        if (dt_new is None) != (win.get("dt") is None) or (mask_new is None) != (win.get("mask") is None):
            raise ValueError("window_advance: dt_new goes with win['dt'] and mask_new with win['mask']")
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().pa_window_advance_t(
                T, L, ny // 2, y_new.data_ptr(), win["y"].data_ptr(), win["pose"].data_ptr(),
                win["angvel"].data_ptr(), win["vel"].data_ptr(), _lib.ptr(nvalid), _lib.ptr(win.get("dt")),
                _lib.ptr(win.get("mask")), _lib.ptr(dt_new), _lib.ptr(mask_new), float(dt),
                _vel_code(vel_frame), _lib.stream_of(dev)), "pa_window_advance_t")
        return
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pa_window_advance_n(
            T, L, ny // 2, y_new.data_ptr(), win["y"].data_ptr(), win["pose"].data_ptr(), win["angvel"].data_ptr(),
            win["vel"].data_ptr(), _lib.ptr(nvalid), float(dt), _vel_code(vel_frame),
            _lib.stream_of(dev)), "pa_window_advance")


TICK_MAX_L = 24  # pa_window_pose_tick: L <= 24 (the cyclic-reduction GN step), T <= the CU count


def _prior_ptrs(prior):
    """(prior_info, prior_grad) of a PriorPlan for the _prior entry points; (None, None) = the parent."""
    return (None, None) if prior is None else (prior.info.data_ptr(), prior.grad.data_ptr())


def window_pose_tick(args, y_new: torch.Tensor, *, lam: float, delta: torch.Tensor, info: torch.Tensor,
                     newest: torch.Tensor | None = None, prior=None) -> None:
    """pa_window_pose_tick on the device's current stream: window_advance(y_new) ->
    pa_trajectory_linearize(args) -> pa_trajectory_gn_step (delta, info) ->
    window_retract(newest) in two launches, bit for bit that sequence.  `args` comes from
    prepare_trajectories over the window arrays (with nvalid, whitening sigmas and Jacobians).
    prior (a PriorPlan): the marginalization prior on frame 0 in the GN step (pa_window_pose_tick_prior)."""
    dev = y_new.device
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pa_window_pose_tick_prior(C.byref(args), y_new.data_ptr(), float(lam), delta.data_ptr(),
                                                        info.data_ptr(), _lib.ptr(newest), *_prior_ptrs(prior),
                                                        _lib.stream_of(dev)), "pa_window_pose_tick")


def window_pose_tick_workspace(T: int, L: int, device) -> torch.Tensor:
    """The reduced system pa_window_pose_tick_pre leaves for _post (bytes as a u8 tensor)."""
    n = int(_lib.lib().pa_window_pose_tick_workspace(int(T), int(L)))
    return torch.empty(max(n, 1), dtype=torch.uint8, device=device)


def window_pose_tick_pre(args, ws: torch.Tensor, *, lam: float, prior=None) -> None:
    """pa_window_pose_tick_pre on the device's current stream: the window advances without the
    new keypoints, every factor but the newest frame's projections, the GN system reduced to
    the newest frame (into ws)."""
    dev = ws.device
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pa_window_pose_tick_pre_prior(C.byref(args), float(lam), ws.data_ptr(), ws.numel(),
                                                            *_prior_ptrs(prior), _lib.stream_of(dev)),
                   "pa_window_pose_tick_pre")


def window_pose_tick_reduce(args, ws: torch.Tensor, *, lam: float, prior=None) -> None:
    """pa_window_pose_tick_reduce on the device's current stream: the pre half's reduction alone,
    from the factor outputs as they stand (no advance, no linearize)."""
    dev = ws.device
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pa_window_pose_tick_reduce_prior(C.byref(args), float(lam), ws.data_ptr(), ws.numel(),
                                                               *_prior_ptrs(prior), _lib.stream_of(dev)),
                   "pa_window_pose_tick_reduce")


def window_pose_tick_post(args, y_new: torch.Tensor, ws: torch.Tensor, *, delta: torch.Tensor, info: torch.Tensor,
                          newest: torch.Tensor | None = None) -> None:
    """pa_window_pose_tick_post on the device's current stream: y_new lands, the newest frame's
    projection factors join the reduced system, solve (delta, info), retract (newest).  info /
    newest: tensors or device addresses (e.g. of mapped pinned host memory)."""
    dev = y_new.device
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pa_window_pose_tick_post(C.byref(args), y_new.data_ptr(), ws.data_ptr(), ws.numel(),
                                                       delta.data_ptr(), _lib.ptr(info), _lib.ptr(newest),
                                                       _lib.stream_of(dev)), "pa_window_pose_tick_post")


def window_retract(win: dict, delta: torch.Tensor, info: torch.Tensor | None = None,
                   newest: torch.Tensor | None = None) -> None:
    """pa_window_retract on the device's current stream: pose <- pose Exp(delta[:6]),
    angvel += delta[6:9], vel += delta[9:12]; trajectories with info != 0 unchanged.
    newest (optional, contiguous f64 (T, 12) on the device): each trajectory's last-frame
    pose after the update (pa_window_retract_newest)."""
    T, L = win["pose"].shape[:2]
    dev = win["pose"].device
    if newest is not None and (newest.device != dev or newest.dtype != torch.float64 or newest.numel() != T * 12
                               or not newest.is_contiguous()):
        raise RuntimeError(f"newest must be a contiguous float64 ({T}, 12) tensor on {dev}")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pa_window_retract_newest(T, L, delta.data_ptr(), _lib.ptr(info), win["pose"].data_ptr(),
                                                       win["angvel"].data_ptr(), win["vel"].data_ptr(),
                                                       _lib.ptr(newest), _lib.stream_of(dev)),
                   "pa_window_retract")


class PredictPlan:
    """The newest state of every window predicted Q horizons ahead, with its covariance
    (pa_window_predict): the PoseDynamicsFactor model pa_window_advance predicts the new frame with,
    from pose and velocity of frame L-1 and the angular velocity of frame L-2.  win: the window dict
    (pose (T, L, 12), angvel / vel (T, L, 3), device f64, read in place at every launch).  marg
    (optional): a MarginalsPlan(cross=True) over the same windows; its cov, cross and info feed the
    covariance cov_out = F Sigma* F^T + diag(q_diag) (include/perseus_amd.h), NaN for a trajectory
    whose marginals failed.  q_diag (optional, 12 variances: [pose 6 | angvel 3 | vel 3]).  Buffers
    are allocated once, so `launch` can be captured in a HIP graph and replayed.
    tau (T, Q) f64 device, seconds: fill it before a launch, or pass tau= (a device tensor or
    address of T*Q doubles read in place, e.g. a tick's dt_new with Q = 1).
    out: pose (T, Q, 12) and, with marg, cov (T, Q, 12, 12)."""

    def __init__(self, win: dict, *, Q: int = 1, marg=None, q_diag=None, vel_frame: str = "world", tau=None):
        T, L = win["pose"].shape[:2]
        dev = win["pose"].device
        if marg is not None and (marg.out.get("cov") is None or marg.out.get("cross") is None):
            raise ValueError("PredictPlan: the covariance needs a MarginalsPlan(full=True, cross=True)")
        self.T, self.L, self.Q, self.win, self.marg, self.dev = T, L, int(Q), win, marg, dev
        self.vel_frame = _vel_code(vel_frame)
        self.q_diag = _f64(q_diag, dev, (12,))
        self.tau = torch.zeros((T, self.Q), dtype=torch.float64, device=dev) if tau is None else tau
        self.out = {"pose": torch.empty((T, self.Q, 12), dtype=torch.float64, device=dev)}
        if marg is not None:
            self.out["cov"] = torch.empty((T, self.Q, 12, 12), dtype=torch.float64, device=dev)

    def launch(self) -> None:
        """One pa_window_predict on the device's current stream."""
        p, w, m = _lib.ptr, self.win, self.marg
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().pa_window_predict(
                self.T, self.L, self.Q, p(w["pose"]), p(w["angvel"]), p(w["vel"]),
                p(m.out["cov"]) if m else None, p(m.out["cross"]) if m else None, p(m.out["info"]) if m else None,
                p(self.q_diag), p(self.tau), self.vel_frame, p(self.out["pose"]), p(self.out.get("cov")),
                _lib.stream_of(self.dev)), "pa_window_predict")


class GatePlan:
    """The chi-square gate of the detector's keypoints against a predicted pose (pa_keypoint_gate):
    a corner whose innovation d2 exceeds chi2 under S = H P H^T + diag(sigma^2) loses its mask bit.
    y (T, 2K) f32 device keypoints; pose_pred / cov_pred: device tensors (or addresses) of the
    predicted poses (stride pose_stride doubles per trajectory) and covariances (T, 12, 12), e.g. a
    PredictPlan's outputs with Q = 1; corners (K, 3), K (5), isig_proj (2), tcam (12 or None): device
    f64 tensors, as prepare_trajectories stages them; mask: int32 device tensor or address of the
    words gated in place, word t at mask + t*mask_stride; nvalid (optional, int32 (T,)).  Outputs
    are allocated once, `launch` is capturable.  out: d2 (T, K), zhat (T, K, 2), ginfo (T,) int32
    (_lib.GATE_APPLIED / GATE_FEW / GATE_NOCOV / GATE_YOUNG: everything but APPLIED leaves the
    word as it came)."""

    def __init__(self, y: torch.Tensor, pose_pred, cov_pred, corners, K, isig_proj, mask, *, chi2: float,
                 min_pass: int = 4, min_frames: int = 3, nvalid=None, tcam=None, H: int = 256, W: int = 256,
                 pose_stride: int = 12, mask_stride: int = 1):
        T, ny = y.shape
        dev = y.device
        self.T, self.n_kp, self.H, self.W, self.dev = T, ny // 2, int(H), int(W), dev
        self.y, self.pose_pred, self.cov_pred, self.mask, self.nvalid = y, pose_pred, cov_pred, mask, nvalid
        self.corners, self.K, self.isig_proj, self.tcam = corners, K, isig_proj, tcam
        self.chi2, self.min_pass, self.min_frames = float(chi2), int(min_pass), int(min_frames)
        self.pose_stride, self.mask_stride = int(pose_stride), int(mask_stride)
        self.out = {"d2": torch.empty((T, self.n_kp), dtype=torch.float64, device=dev),
                    "zhat": torch.empty((T, self.n_kp, 2), dtype=torch.float64, device=dev),
                    "ginfo": torch.empty(T, dtype=torch.int32, device=dev)}

    def launch(self) -> None:
        """One pa_keypoint_gate on the device's current stream."""
        p, o = _lib.ptr, self.out
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().pa_keypoint_gate(
                self.T, self.n_kp, self.H, self.W, p(self.y), p(self.pose_pred), self.pose_stride, p(self.cov_pred),
                p(self.corners), p(self.K), p(self.tcam), p(self.isig_proj), self.chi2, self.min_pass,
                p(self.nvalid), self.min_frames, p(self.mask), self.mask_stride, p(o["d2"]), p(o["zhat"]),
                p(o["ginfo"]), _lib.stream_of(self.dev)), "pa_keypoint_gate")


def predict(win: dict, taus, *, cov=None, cross=None, cov_info=None, q_diag=None, vel_frame: str = "world") -> dict:
    """pa_window_predict, eagerly: the newest state of every window in `win` (pose (T, L, 12), angvel /
    vel (T, L, 3), device) at the horizons taus ((Q,) shared by every trajectory, or (T, Q), seconds).
    cov / cross (optional, together): pa_trajectory_marginals' outputs (`marginals(..., cross=True)`),
    with cov_info its info.  Returns pose (T, Q, 12) and, with cov, cov (T, Q, 12, 12)."""
    T, L = win["pose"].shape[:2]
    dev = win["pose"].device
    tau = torch.as_tensor(np.asarray(taus, np.float64), device=dev)
    tau = (tau.reshape(1, -1).expand(T, -1) if tau.dim() < 2 else tau.reshape(T, -1)).contiguous()
    if (cov is None) != (cross is None):
        raise ValueError("predict: cov and cross are given together")
    marg = None
    if cov is not None:
        class _Marg:  # (the three tensors a MarginalsPlan would hold)
            out = {"cov": _f64(cov, dev, (T * L, 12, 12)), "cross": _f64(cross, dev, (T * (L - 1), 12, 12)),
                   "info": None if cov_info is None else cov_info.to(device=dev, dtype=torch.int32).contiguous()}
        marg = _Marg
    w = {k: _f64(win[k], dev) for k in ("pose", "angvel", "vel")}
    plan = PredictPlan(w, Q=tau.shape[1], marg=marg, q_diag=q_diag, vel_frame=vel_frame, tau=tau)
    plan.launch()
    out = dict(plan.out)
    out["_keep"] = (w, tau, marg, plan.q_diag)
    return out


def gate_keypoints(y: torch.Tensor, pose_pred, cov_pred, corners, K, proj_sigmas, mask, *, chi2: float,
                   min_pass: int = 4, min_frames: int = 3, nvalid=None, camera_pose=None, H: int = 256,
                   W: int = 256) -> dict:
    """pa_keypoint_gate, eagerly: y (T, 2K) device keypoints against pose_pred (T, 12) with cov_pred
    (T, 12, 12); mask (T,) ints (one bit per keypoint) is staged, not modified.  Returns mask (T,)
    int32 (the gated words), d2 (T, K), zhat (T, K, 2) and ginfo (T,) int32."""
    if y.device.type != "cuda":
        raise RuntimeError("gate_keypoints expects the detector output on the GPU (no CPU fallback)")
    dev = y.device
    y = y.to(torch.float32).contiguous()
    T, nk = y.shape[0], y.shape[1] // 2
    m = _mask(mask, dev, (T,)).clone()
    keep = (_f64(pose_pred, dev, (T, 12)), _f64(cov_pred, dev, (T, 12, 12)), _f64(corners, dev, (nk, 3)),
            _f64(K, dev, (5,)), _isig(proj_sigmas, 2, dev), _f64(camera_pose, dev, (12,)))
    nv = None if nvalid is None else torch.as_tensor(np.asarray(nvalid, np.int32), device=dev) \
        if not isinstance(nvalid, torch.Tensor) else nvalid.to(device=dev, dtype=torch.int32).contiguous()
    plan = GatePlan(y, keep[0], keep[1], keep[2], keep[3], keep[4], m, chi2=chi2, min_pass=min_pass,
                    min_frames=min_frames, nvalid=nv, tcam=keep[5], H=H, W=W)
    plan.launch()
    out = dict(plan.out)
    out["mask"] = m
    out["_keep"] = (y, keep, nv)
    return out
