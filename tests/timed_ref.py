"""TEST HELPER (not a test): the smoother with real timestamps, restated in numpy from the
oracle's pieces.  Every PoseDynamicsFactor has its own dt (oracle.factors_ref.dynamics per frame
pair) and every frame a keypoint mask (bit k set: keypoint k was measured; a cleared bit gives
that projection factor status 2 and zero rows, exactly what `nvalid` gives a whole frame):

  factors            lm_ref.factors with dt_pair (L-1) and kp_mask (L)
  window_advance_t   oracle.factors_ref.window_advance with the two rings win["dt"] (T, L-1) and
                     win["mask"] (T, L): they shift with the window, dt_new / mask_new land at
                     the end and dt_new predicts the new frame
  tick / chain       one streaming tick (advance -> factors -> dense GN -> retract) and the
                     jitter / gap / drop-out stream the tests track
  solve_one / solve  lm_ref.solve_one's loop on these factors
"""
from __future__ import annotations

import numpy as np

import lm_ref
from oracle import factors_ref as F
from oracle import gn_ref as G
from perseus_amd import synth

DT = lm_ref.DT
SIGMAS = lm_ref.SIGMAS
TICK_SIG = dict(proj=2.0, dyn=0.1, cv=0.5)  # test_streaming_pose_gpu.SIG
TICK_LAM = 1e-2
ROT_TOL, TRA_TOL = 1e-4, 1e-5
_untimed_factors = lm_ref.factors  # (solve_one below puts `factors` in its place while it runs)


def mask_off(kp_mask, L, nk):
    """(L * nk,) bool: projection factor (frame l, keypoint k) is switched off by the mask."""
    m = np.asarray(kp_mask).astype(np.int64).reshape(L)
    return ((m[:, None] >> np.arange(nk)[None, :]) & 1).reshape(-1) == 0


def factors(y, pose, vel, angvel, L, *, dt=DT, dt_pair=None, kp_mask=None, vel_frame="world", sigmas=SIGMAS,
            nvalid=None, **kw):
    """lm_ref.factors with a per-pair dt (dt_pair (L-1), None: the scalar dt) and a per-frame
    keypoint mask (kp_mask (L) ints, None: all measured).  The mask combines with nvalid by OR of
    "off" and wins over cheirality (status 2, not 1)."""
    f = _untimed_factors(y, pose, vel, angvel, L, dt=dt, vel_frame=vel_frame, sigmas=sigmas, nvalid=nvalid, **kw)
    if dt_pair is not None:
        dtp = np.asarray(dt_pair, np.float64).reshape(L - 1)
        sd = sigmas["dyn"]
        for l in range(L - 1):
            r, H = F.dynamics(F.unpack(pose[l]), angvel[l], vel[l], F.unpack(pose[l + 1]), float(dtp[l]), vel_frame)
            f["r_dyn"][l] = r / sd
            for k in range(4):
                f[f"j_dyn{k}"][l] = H[k] / sd
        f["err_dyn"] = 0.5 * (f["r_dyn"] ** 2).sum(1)
    if kp_mask is not None:
        nk = f["r_proj"].shape[0] // L
        off = mask_off(kp_mask, L, nk)
        pend = f["status"] == 3
        f["status"][off & ~pend] = 2
        f["r_proj"][off] = 0.0
        f["j_proj"][off] = 0.0
        f["err_proj"] = 0.5 * (f["r_proj"] ** 2).sum(1)
    return f


def window_advance_t(win: dict, y_new, dt_new=None, mask_new=None, dt=DT, vel_frame="world") -> dict:
    """pa_window_advance_t: oracle.factors_ref.window_advance, the rings win["dt"] / win["mask"]
    (either may be absent) moving with the window; the new frame is predicted with dt_new."""
    T = win["pose"].shape[0]
    core = {k: win[k] for k in ("y", "pose", "angvel", "vel")}
    if dt_new is None:
        out = F.window_advance(core, y_new, dt, vel_frame)
    else:
        outs = [F.window_advance({k: v[t:t + 1] for k, v in core.items()}, np.asarray(y_new)[t:t + 1],
                                 float(np.asarray(dt_new)[t]), vel_frame) for t in range(T)]
        out = {k: np.concatenate([o[k] for o in outs], 0) for k in core}
    if dt_new is not None:
        out["dt"] = np.concatenate([win["dt"][:, 1:], np.asarray(dt_new, np.float64).reshape(T, 1)], 1)
    if mask_new is not None:
        out["mask"] = np.concatenate([win["mask"][:, 1:], np.asarray(mask_new).astype(win["mask"].dtype).reshape(T, 1)], 1)
    return out


def window_factors(win, nvalid, *, sigmas=TICK_SIG, dt=DT, vel_frame="world"):
    """The whitened factors of every trajectory of a window (stacked as the device lays them
    out), rings honoured when present."""
    T, L = win["pose"].shape[:2]
    fs = [factors(win["y"][t], win["pose"][t], win["vel"][t], win["angvel"][t], L, dt=dt,
                  dt_pair=win["dt"][t] if "dt" in win else None, kp_mask=win["mask"][t] if "mask" in win else None,
                  vel_frame=vel_frame, sigmas=sigmas, nvalid=None if nvalid is None else int(nvalid[t]))
          for t in range(T)]
    return {k: np.concatenate([f[k] for f in fs], 0) for k in fs[0]}


def init_window(T, L, nk, pose0, dt=DT, timed=True):
    win = dict(y=np.zeros((T, L, 2 * nk), np.float32), pose=np.repeat(np.asarray(pose0).reshape(T, 1, 12), L, 1),
               angvel=np.zeros((T, L, 3)), vel=np.zeros((T, L, 3)))
    if timed:
        win["dt"] = np.full((T, L - 1), dt)
        win["mask"] = np.full((T, L), 0xFFFFFFFF, np.int64)
    return win


def tick(win, nvalid, y_new, dt_new=None, mask_new=None, *, lam=TICK_LAM, sigmas=TICK_SIG, dt=DT):
    """One streaming tick on the oracle: returns (window, nvalid, info (T,), factors)."""
    T, L = win["pose"].shape[:2]
    nk = win["y"].shape[2] // 2
    adv = window_advance_t(win, y_new, dt_new, mask_new, dt)
    nvalid = np.minimum(np.asarray(nvalid) + 1, L)
    f = window_factors(adv, nvalid, sigmas=sigmas, dt=dt)
    _, _, d = G.gn_step(f, T, L, nk, lam)
    d = np.asarray(d).reshape(T, L * 12)
    info = (~np.isfinite(d).all(1)).astype(np.int32)
    core = F.window_retract({k: adv[k] for k in ("y", "pose", "angvel", "vel")}, np.nan_to_num(d).reshape(-1, 12), info)
    adv.update(core)
    return adv, nvalid, info, f


# ---------------------------------------------------------------- the jittered stream
def stream_case(n=3, ticks=40, seed=5, jitter=0.3, gap_tick=17, drop_every=7, dt=DT):
    """The case of the tracking tests: per camera stamps with +-`jitter` period jitter, one
    3-period gap (every camera, at `gap_tick`), camera (k // drop_every) % n absent on every
    drop_every-th tick, and single corners missing at random.  The cube follows the dynamics model
    exactly in continuous time, so its pose at a stamp s is T0 Exp(s [w; R0^T v]) ... composed
    stepwise with the true per-pair dt (the model is a one-parameter subgroup only for v = 0, so
    the truth is built by the same steps the factors describe).
    Returns dict(stamps (ticks, n), dt_new (ticks, n), present (ticks, n) bool, mask (ticks, n)
    int64, truth [ticks][n] (R, t), y (ticks, n, 2K) f32, w, v)."""
    rng = np.random.default_rng(seed)
    w = 0.3 * rng.standard_normal((n, 3))
    v = 0.01 * rng.standard_normal((n, 3))
    cur = []
    for c in range(n):
        R0, _ = F.pose_exp(np.concatenate([0.3 * rng.standard_normal(3), np.zeros(3)]))
        cur.append((R0, np.array([0.0, 0.0, 0.35]) + 0.005 * rng.standard_normal(3)))
    jr = np.random.default_rng(seed + 1000)
    dts = dt * (1.0 + jitter * jr.uniform(-1.0, 1.0, (ticks, n)))
    dts[gap_tick] = 3.0 * dt
    dts[0] = dt  # the first tick's dt is the nominal one (nothing came before)
    present = np.ones((ticks, n), bool)
    for k in range(drop_every, ticks, drop_every):  # (tick 35 is among the last 10, the ones judged)
        present[k, (k // drop_every) % n] = False
    mask = np.full((ticks, n), 0xFF, np.int64)
    for k in range(2, ticks):
        for c in range(n):
            if jr.uniform() < 0.25:
                mask[k, c] &= ~(1 << int(jr.integers(0, 8)))
    mask[~present] = 0
    truth, stamps, s = [], [], np.zeros(n)
    for k in range(ticks):
        if k > 0:
            cur = [F.compose(T, F.pose_exp(np.concatenate([dts[k, c] * w[c], dts[k, c] * (T[0].T @ v[c])])))
                   for c, T in enumerate(cur)]
            s = s + dts[k]
        truth.append(list(cur))
        stamps.append(s.copy())
    y = np.stack([lm_ref.keypoints(tk) for tk in truth])
    return dict(stamps=np.array(stamps), dt_new=dts, present=present, mask=mask, truth=truth, y=y, w=w, v=v)


def init_pose(truth0, seed=5):
    """test_streaming_pose_gpu._init: the first true pose, ~0.1 rad / ~1 cm off."""
    rng = np.random.default_rng(seed + 100)
    p = []
    for Rm, t in truth0:
        Rp, _ = F.pose_exp(np.concatenate([0.1 * rng.standard_normal(3) / np.sqrt(3), np.zeros(3)]))
        p.append(F.pack((Rm @ Rp, t + 0.01 * rng.standard_normal(3) / np.sqrt(3))))
    return np.array(p)


def newest_errors(pose, truth_tick):
    er, et = [], []
    for c, (Rt, tt) in enumerate(truth_tick):
        Rm, t = F.unpack(pose[c])
        er.append(np.linalg.norm(F.rot_log(Rt.T @ Rm)))
        et.append(np.linalg.norm(t - tt))
    return max(er), max(et)


def chain(case, L=6, timed=True, dt=DT):
    """The stream through the oracle tick.  timed=False: the scalar nominal dt and no masks (an
    absent camera's slot then holds its last seen keypoints).  Returns (rot err, tra err, info)
    per tick, worst over the cameras, and the final window."""
    ticks, n = case["dt_new"].shape
    nk = case["y"].shape[2] // 2
    win = init_window(n, L, nk, init_pose(case["truth"][0]), dt, timed)
    nvalid = np.zeros(n, int)
    er, et, infos = [], [], []
    last = case["y"][0].copy()
    for k in range(ticks):
        y = case["y"][k].copy()
        y[~case["present"][k]] = last[~case["present"][k]]
        last = y
        if timed:
            win, nvalid, info, _ = tick(win, nvalid, y, case["dt_new"][k], case["mask"][k], dt=dt)
        else:
            win, nvalid, info, _ = tick(win, nvalid, y, dt=dt)
        r, t = newest_errors(win["pose"][:, -1], case["truth"][k])
        er.append(r)
        et.append(t)
        infos.append(info)
    return np.array(er), np.array(et), np.array(infos), win


# ---------------------------------------------------------------- Levenberg-Marquardt
LM_DT_PAIR = np.array([1.0, 3.0, 0.5, 2.0, 1.25]) / 30.0
LM_MASKS = np.array([0xFF, 0xFF, 0b10110111, 0, 0xFF, 0xFF], np.int64)
LM_MEASURED = (0, 1, 2, 4, 5)


def lm_problem(T=3, L=6, rot=0.1, seed=5, dt_pair=LM_DT_PAIR):
    """lm_ref.problem with frames dt_pair apart: exact keypoints of T true trajectories, the
    initial window at the first true pose rotated by `rot` rad, at rest."""
    base = lm_ref.problem(T, L, rot, seed)
    rng = np.random.default_rng(seed)
    w = 0.3 * rng.standard_normal((T, 3))
    v = 0.01 * rng.standard_normal((T, 3))
    cur = [F.unpack(base["truth"].reshape(T, L, 12)[t, 0]) for t in range(T)]
    tr = [list(cur)]
    for l in range(L - 1):
        cur = [F.compose(X, F.pose_exp(np.concatenate([dt_pair[l] * w[c], dt_pair[l] * (X[0].T @ v[c])])))
               for c, X in enumerate(cur)]
        tr.append(list(cur))
    base["y"] = np.stack([lm_ref.keypoints(tr[l]) for l in range(L)], 1).reshape(T * L, -1)
    base["truth"] = np.array([[F.pack(tr[l][t]) for l in range(L)] for t in range(T)]).reshape(T * L, 12)
    return base


def solve_one(y, pose, vel, angvel, L, params=lm_ref.PARAMS, **kw):
    """lm_ref.solve_one's loop, decision for decision, on `factors` above (kw: dt_pair, kp_mask
    and lm_ref.factors' keywords)."""
    saved = lm_ref.factors
    lm_ref.factors = factors
    try:
        return lm_ref.solve_one(y, pose, vel, angvel, L, params, **kw)
    finally:
        lm_ref.factors = saved


def solve(y, pose, vel, angvel, T, L, params=lm_ref.PARAMS, dt_pair=None, kp_mask=None, **kw):
    """Every trajectory independently (dt_pair (T, L-1), kp_mask (T, L) or None), stacked as
    lm_ref.solve stacks them."""
    y = np.asarray(y).reshape(T, L, -1)
    P, V, W = (np.asarray(a, np.float64).reshape(T, L, -1) for a in (pose, vel, angvel))
    res = [solve_one(y[t], P[t], V[t], W[t], L, params, dt_pair=None if dt_pair is None else np.asarray(dt_pair)[t],
                     kp_mask=None if kp_mask is None else np.asarray(kp_mask)[t], **kw) for t in range(T)]
    out = {k: np.array([r[k] for r in res]) for k in ("cost0", "cost", "iters", "status", "lambda", "cost_hist")}
    for k in ("pose", "vel", "angvel"):
        out[k] = np.concatenate([r[k] for r in res], 0)
    out["log"] = [r["log"] for r in res]
    return out
