"""TEST HELPER (not a test): the Levenberg-Marquardt loop of pa_trajectory_lm_solve
(include/perseus_amd.h) restated in numpy, decision for decision, from the oracle's pieces:
oracle.factors_ref.projection_batch / dynamics_batch for the factors (wired as
test_pipeline_gpu._oracle, whitened as test_streaming_pose_gpu._whiten), the pose_exp retract of
oracle.factors_ref.window_retract, and oracle.gn_ref.gn_step for the damped step, called per
trajectory with that trajectory's own lambda.

`solve` records, per trajectory and iteration, the accept decision, what rejected a step
("cost", "cheirality" or "pivot") and the decision's margin |C' - C| / C, so that a device test
can restrict its comparison to decisions that f64 rounding cannot flip.
"""
from __future__ import annotations

import numpy as np

from oracle import factors_ref as F
from oracle import gn_ref as G
from oracle import resnet_ref as R
from perseus_amd import synth

CONVERGED, MAX_ITERS, STALLED = 1, 2, 3
DT = 1.0 / 30.0
SIGMAS = dict(proj=2.0, dyn=0.1, cv=0.5)
PARAMS = dict(max_iters=30, lambda0=1e-3, lambda_up=10.0, lambda_down=10.0, lambda_min=1e-12, lambda_max=1e12,
              rel_tol=1e-6, abs_tol=1e-9)


# ---------------------------------------------------------------- problems
def truth(n, ticks, seed=5, dt=DT):
    """test_streaming_pose_gpu._truth: per trajectory a cube trajectory that follows the
    PoseDynamicsFactor model exactly.  Returns poses (ticks, n) of (R, t), w (n, 3), v (n, 3)."""
    rng = np.random.default_rng(seed)
    w = 0.3 * rng.standard_normal((n, 3))
    v = 0.01 * rng.standard_normal((n, 3))
    poses, cur = [], []
    for c in range(n):
        R0, _ = F.pose_exp(np.concatenate([0.3 * rng.standard_normal(3), np.zeros(3)]))
        cur.append((R0, np.array([0.0, 0.0, 0.35]) + 0.005 * rng.standard_normal(3)))
    for _ in range(ticks):
        poses.append(list(cur))
        cur = [F.compose(T, F.pose_exp(np.concatenate([dt * w[c], dt * (T[0].T @ v[c])]))) for c, T in enumerate(cur)]
    return poses, w, v


def keypoints(poses_tick):
    """test_streaming_pose_gpu._keypoints without noise: normalized keypoints (n, 2K) f32 of the
    cube corners seen by the identity camera synth.CAMERA_K."""
    fx, fy, s, u0, v0 = synth.CAMERA_K
    out = []
    for Rm, t in poses_tick:
        pc = synth.CUBE_CORNERS @ Rm.T + t
        assert (pc[:, 2] > 0).all()
        u = fx * pc[:, 0] / pc[:, 2] + s * pc[:, 1] / pc[:, 2] + u0
        v = fy * pc[:, 1] / pc[:, 2] + v0
        px = np.stack([u, v], 1)
        assert (px > 0).all() and (px < 255).all()
        out.append((px / 127.5 - 1.0).reshape(-1))
    return np.array(out, np.float32)


def problem(T, L, rot, seed=5, trans=0.01):
    """Exact keypoints of T true trajectories over L frames, and the initial window: every frame
    at the first true pose rotated by `rot` rad and moved by `trans` m (random directions), at
    rest.  Returns dict(y (T*L, 2K) f32, pose (T*L, 12), vel, angvel (T*L, 3), truth (T*L, 12))."""
    tr, _, _ = truth(T, L, seed)
    y = np.stack([keypoints(tr[l]) for l in range(L)], 1).reshape(T * L, -1)  # frame f = t * L + l
    rng = np.random.default_rng(seed + 100)
    pose = np.zeros((T, L, 12))
    for t, (Rm, tt) in enumerate(tr[0]):
        d = rng.standard_normal(3)
        Rp, _ = F.pose_exp(np.concatenate([rot * d / np.linalg.norm(d), np.zeros(3)]))
        e = rng.standard_normal(3)
        pose[t, :] = F.pack((Rm @ Rp, tt + trans * e / np.linalg.norm(e)))
    true = np.array([[F.pack(tr[l][t]) for l in range(L)] for t in range(T)]).reshape(T * L, 12)
    return dict(y=y, pose=pose.reshape(T * L, 12), vel=np.zeros((T * L, 3)), angvel=np.zeros((T * L, 3)), truth=true)


def pose_errors(pose, true):
    """Per frame (rotation error rad, translation error m) of (n, 12) poses."""
    rot, tra = [], []
    for p, q in zip(np.asarray(pose).reshape(-1, 12), np.asarray(true).reshape(-1, 12)):
        (Ra, ta), (Rb, tb) = F.unpack(p), F.unpack(q)
        rot.append(np.linalg.norm(F.rot_log(Ra.T @ Rb)))
        tra.append(np.linalg.norm(ta - tb))
    return np.array(rot), np.array(tra)


# ---------------------------------------------------------------- the factors of one trajectory
def factors(y, pose, vel, angvel, L, *, dt=DT, vel_frame="world", sigmas=SIGMAS, nvalid=None, corners=None, K=None,
            Tc=None, pending=False):
    """One trajectory's whitened factors (gn_ref's dict) with err_* = 0.5 |r_w|^2 per factor;
    frames l < L - nvalid carry status 2 and zero projection rows.  pending (pa_window_lm_solve's
    newest_pending): frame L - 1's projection factors carry status 3 and stay out of everything."""
    corners = synth.CUBE_CORNERS if corners is None else np.asarray(corners, np.float64)
    K = synth.CAMERA_K if K is None else np.asarray(K, np.float64)
    nk = len(corners)
    z = R.denormalize_f32(np.asarray(y, np.float32).reshape(L, 2 * nk), 256, 256).astype(np.float64).reshape(-1, 2)
    rp, Jp, st = F.projection_batch(np.repeat(pose, nk, axis=0), np.tile(corners, (L, 1)), z, K, Tc)
    idx = np.arange(L - 1)
    rd, J0, J1, J2, J3 = F.dynamics_batch(pose[idx], angvel[idx], vel[idx], pose[idx + 1], dt, vel_frame)
    rc = vel[idx + 1] - vel[idx]
    sp, sd, sc = sigmas["proj"], sigmas["dyn"], sigmas["cv"]
    f = dict(r_proj=rp / sp, j_proj=Jp / sp, status=st.copy(), r_dyn=rd / sd, j_dyn0=J0 / sd, j_dyn1=J1 / sd,
             j_dyn2=J2 / sd, j_dyn3=J3 / sd, r_cv=rc / sc,
             j_cv0=np.broadcast_to(-np.eye(3) / sc, (L - 1, 3, 3)).copy(),
             j_cv1=np.broadcast_to(np.eye(3) / sc, (L - 1, 3, 3)).copy())
    if nvalid is not None:
        off = np.repeat(np.arange(L) < L - int(nvalid), nk)
        f["status"][off] = 2
        f["r_proj"][off] = 0.0
        f["j_proj"][off] = 0.0
    if pending:
        f["status"][(L - 1) * nk:] = 3
    f["err_proj"] = 0.5 * (f["r_proj"] ** 2).sum(1)
    f["err_dyn"] = 0.5 * (f["r_dyn"] ** 2).sum(1)
    f["err_cv"] = 0.5 * (f["r_cv"] ** 2).sum(1)
    return f


def cost(f):
    return float(f["err_dyn"].sum() + f["err_cv"].sum() + f["err_proj"][f["status"] == 0].sum())


def retract(pose, vel, angvel, delta):
    """oracle.factors_ref.window_retract for one trajectory: delta (L, 12)."""
    p = np.array([F.pack(F.compose(F.unpack(pose[l]), F.pose_exp(delta[l, :6]))) for l in range(len(pose))])
    return p, vel + delta[:, 9:12], angvel + delta[:, 6:9]


# ---------------------------------------------------------------- the loop
def solve_one(y, pose, vel, angvel, L, params=PARAMS, **kw):
    """pa_trajectory_lm_solve's algorithm on one trajectory.  Returns a dict: pose, vel, angvel
    (final), cost0, cost, iters, status, lambda, cost_hist (max_iters + 1, NaN after the stop),
    log: per iteration dict(accept, why, margin, lam) (lam: the damping the step was solved with)."""
    p = dict(PARAMS, **params)
    nk = np.asarray(y).reshape(L, -1).shape[1] // 2
    x = (np.array(pose, np.float64), np.array(vel, np.float64), np.array(angvel, np.float64))
    f = factors(y, *x, L, **kw)
    C = cost(f)
    lam = p["lambda0"]
    hist = np.full(p["max_iters"] + 1, np.nan)
    hist[0] = C
    cost0, status, iters, log = C, 0, 0, []
    for k in range(1, p["max_iters"] + 1):
        iters = k
        _, _, d = G.gn_step(f, 1, L, nk, lam)
        rec = dict(accept=False, why="pivot", margin=np.inf, lam=lam)
        if np.isfinite(d).all():
            xn = retract(*x, d.reshape(L, 12))
            fn = factors(y, *xn, L, **kw)
            Cn = cost(fn)
            rec["margin"] = abs(Cn - C) / C if C > 0 else np.inf
            rec["cost_lower"] = Cn < C  # what the cost test alone would have decided
            if ((f["status"] == 0) & (fn["status"] == 1)).any():
                rec["why"] = "cheirality"
            elif Cn < C:
                rec.update(accept=True, why="cost")
            else:
                rec["why"] = "cost"
        log.append(rec)
        if rec["accept"]:
            x, f = xn, fn
            lam = max(lam / p["lambda_down"], p["lambda_min"])
            if C - Cn <= p["rel_tol"] * C + p["abs_tol"]:
                status = CONVERGED
            C = Cn
        else:
            lam = lam * p["lambda_up"]
            if lam > p["lambda_max"]:
                status = STALLED
        hist[k] = C
        if status:
            break
    if not status:
        status = MAX_ITERS
    return dict(pose=x[0], vel=x[1], angvel=x[2], cost0=cost0, cost=C, iters=iters, status=status, cost_hist=hist,
                log=log, **{"lambda": lam})


def solve(y, pose, vel, angvel, T, L, params=PARAMS, nvalid=None, **kw):
    """Every trajectory independently; arrays stacked as the device returns them."""
    y = np.asarray(y).reshape(T, L, -1)
    P, V, W = (np.asarray(a, np.float64).reshape(T, L, -1) for a in (pose, vel, angvel))
    res = [solve_one(y[t], P[t], V[t], W[t], L, params, nvalid=None if nvalid is None else nvalid[t], **kw)
           for t in range(T)]
    out = {k: np.array([r[k] for r in res]) for k in ("cost0", "cost", "iters", "status", "lambda", "cost_hist")}
    for k in ("pose", "vel", "angvel"):
        out[k] = np.concatenate([r[k] for r in res], 0)
    out["log"] = [r["log"] for r in res]
    return out
