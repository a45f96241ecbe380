"""TEST HELPER (not a test): the constant-velocity factor on the ANGULAR velocity ("cw",
pa_traj_args.r_cw in include/perseus_amd.h) restated in numpy around the existing references.

For pair (l, l+1) of a trajectory: r = (angvel[l+1] - angvel[l]) * isig_cw, three rows, with
the constant Jacobians -diag(isig_cw) on frame l's angular velocity (variables 6..8 of its
12-block) and +diag(isig_cw) on frame l+1's.  `stack` appends those rows to oracle.gn_ref.stack's
dense (A, r); `cost` adds 0.5 |r|^2 to lm_ref.cost; `solve_one` restates steps 1-5 of
pa_trajectory_lm_solve around that system (lm_ref.solve_one is closed over the old factor set).
With isig_cw None every function here is the parent reference, value for value.
"""
from __future__ import annotations

import numpy as np

import lm_ref
from oracle import gn_ref as G

NV = G.NV


def residual(angvel, L, isig_cw):
    """(T*(L-1), 3) whitened residuals of angvel (T*L, 3): one subtract, one multiply."""
    w = np.asarray(angvel, np.float64).reshape(-1, L, 3)
    s = np.ones(3) if isig_cw is None else np.asarray(isig_cw, np.float64).reshape(3)
    return ((w[:, 1:] - w[:, :-1]) * s).reshape(-1, 3)


def rows(r_cw, isig_cw, T, L):
    """Per trajectory the factor's dense rows (A_cw (3 (L-1), 12 L), r (3 (L-1),))."""
    s = np.asarray(isig_cw, np.float64).reshape(3)
    r_cw = np.asarray(r_cw, np.float64).reshape(T, max(L - 1, 0), 3)
    out = []
    for t in range(T):
        A = np.zeros((3 * (L - 1), NV * L))
        for l in range(L - 1):
            for i in range(3):
                A[3 * l + i, l * NV + 6 + i] = -s[i]
                A[3 * l + i, (l + 1) * NV + 6 + i] = s[i]
        out.append((A, r_cw[t].reshape(-1)))
    return out


def stack(f: dict, T: int, L: int, K: int, isig_cw=None):
    """oracle.gn_ref.stack's (A, r) per trajectory with the factor's rows appended (f["r_cw"]:
    the whitened residuals); isig_cw None: gn_ref.stack itself."""
    base = G.stack(f, T, L, K)
    if isig_cw is None or L < 2:
        return base
    return [(np.concatenate([A, Aw], 0), np.concatenate([r, rw], 0))
            for (A, r), (Aw, rw) in zip(base, rows(f["r_cw"], isig_cw, T, L))]


def gn_step(f: dict, T: int, L: int, K: int, lam: float, isig_cw=None):
    """oracle.gn_ref.gn_step over `stack`: H (T, 12L, 12L), g (T, 12L), delta (T, 12L)."""
    Hs, gs, ds = [], [], []
    for A, r in stack(f, T, L, K, isig_cw):
        H = A.T @ A
        g = A.T @ r
        M = H + lam * np.eye(H.shape[0])
        try:
            np.linalg.cholesky(M)
            d = np.linalg.solve(M, -g)
        except np.linalg.LinAlgError:
            d = np.full_like(g, np.nan)
        Hs.append(H)
        gs.append(g)
        ds.append(d)
    return np.stack(Hs), np.stack(gs), np.stack(ds)


def factors(y, pose, vel, angvel, L, *, isig_cw=None, **kw):
    """lm_ref.factors of one trajectory plus r_cw / err_cw when isig_cw is given."""
    f = lm_ref.factors(y, pose, vel, angvel, L, **kw)
    if isig_cw is not None:
        f["r_cw"] = residual(angvel, L, isig_cw)
        f["err_cw"] = 0.5 * (f["r_cw"] ** 2).sum(1)
    return f


def cost(f):
    c = lm_ref.cost(f)
    return c + float(f["err_cw"].sum()) if "err_cw" in f else c


def solve_one(y, pose, vel, angvel, L, params=lm_ref.PARAMS, *, isig_cw=None, **kw):
    """Steps 1-5 of pa_trajectory_lm_solve (include/perseus_amd.h) on one trajectory, the cost and
    the step taken over the factor set with the cw rows.  Same returns as lm_ref.solve_one."""
    p = dict(lm_ref.PARAMS, **params)
    nk = np.asarray(y).reshape(L, -1).shape[1] // 2
    x = (np.array(pose, np.float64), np.array(vel, np.float64), np.array(angvel, np.float64))
    f = factors(y, *x, L, isig_cw=isig_cw, **kw)
    C = cost(f)
    lam = p["lambda0"]
    hist = np.full(p["max_iters"] + 1, np.nan)
    hist[0] = C
    cost0, status, iters, log = C, 0, 0, []
    for k in range(1, p["max_iters"] + 1):
        iters = k
        _, _, d = gn_step(f, 1, L, nk, lam, isig_cw)
        rec = dict(accept=False, why="pivot", margin=np.inf, lam=lam)
        if np.isfinite(d).all():
            xn = lm_ref.retract(*x, d.reshape(L, 12))
            fn = factors(y, *xn, L, isig_cw=isig_cw, **kw)
            Cn = cost(fn)
            rec["margin"] = abs(Cn - C) / C if C > 0 else np.inf
            rec["cost_lower"] = Cn < C
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
                status = lm_ref.CONVERGED
            C = Cn
        else:
            lam = lam * p["lambda_up"]
            if lam > p["lambda_max"]:
                status = lm_ref.STALLED
        hist[k] = C
        if status:
            break
    if not status:
        status = lm_ref.MAX_ITERS
    return dict(pose=x[0], vel=x[1], angvel=x[2], cost0=cost0, cost=C, iters=iters, status=status, cost_hist=hist,
                log=log, **{"lambda": lam})


def solve(y, pose, vel, angvel, T, L, params=lm_ref.PARAMS, nvalid=None, *, isig_cw=None, **kw):
    """Every trajectory independently; arrays stacked as the device returns them (lm_ref.solve)."""
    y = np.asarray(y).reshape(T, L, -1)
    P, V, W = (np.asarray(a, np.float64).reshape(T, L, -1) for a in (pose, vel, angvel))
    res = [solve_one(y[t], P[t], V[t], W[t], L, params, isig_cw=isig_cw,
                     nvalid=None if nvalid is None else nvalid[t], **kw) for t in range(T)]
    out = {k: np.array([r[k] for r in res]) for k in ("cost0", "cost", "iters", "status", "lambda", "cost_hist")}
    for k in ("pose", "vel", "angvel"):
        out[k] = np.concatenate([r[k] for r in res], 0)
    out["log"] = [r["log"] for r in res]
    return out


# ---------------------------------------------------------------- marginals / marginalization with the rows appended
def dense_cov(f: dict, T: int, L: int, K: int, lam: float, isig_cw=None):
    """marginals_ref.dense over `stack`: (cov (T, L, 12, 12), cross (T, L-1, 12, 12))."""
    cov, cross = [], []
    for A, _ in stack(f, T, L, K, isig_cw):
        H = A.T @ A
        S = np.linalg.inv(H + lam * np.eye(H.shape[0]))
        D, E = G.blocks(S, L)
        cov.append(D)
        cross.append(E)
    return np.stack(cov), np.stack(cross)


def dense_delta(f: dict, T: int, L: int, K: int, lam: float, isig_cw=None, prior_info=None, prior_grad=None):
    """prior_ref.dense_delta over `stack`: delta (T, 12 L) with the prior on frame 0."""
    out = []
    for t, (A, r) in enumerate(stack(f, T, L, K, isig_cw)):
        H = A.T @ A + lam * np.eye(A.shape[1])
        g = A.T @ r
        if prior_info is not None:
            H[:NV, :NV] += prior_info[t]
            g[:NV] += prior_grad[t]
        out.append(np.linalg.solve(H, -g))
    return np.stack(out)


def marginalize(f: dict, T: int, L: int, K: int, lam: float, isig_cw=None, prior_info=None, prior_grad=None):
    """prior_ref.marginalize (every window full, no re-centring) with the pair (0, 1)'s cw rows
    appended to the rows that touch x_0: (info (T, 12, 12), eta (T, 12), minfo (T,))."""
    import prior_ref as PR

    info, eta, minfo = np.zeros((T, NV, NV)), np.zeros((T, NV)), np.zeros(T, np.int32)
    for t in range(T):
        A, r = PR._pair01(f, t, L, K)
        if isig_cw is not None:
            (Aw, rw), = rows(np.asarray(f["r_cw"]).reshape(T, L - 1, 3)[t, :1], isig_cw, 1, 2)
            A, r = np.concatenate([A, Aw], 0), np.concatenate([r, rw], 0)
        A0, B = A[:, :NV], A[:, NV:]
        H = A0.T @ A0 + lam * np.eye(NV)
        g0 = A0.T @ r
        if prior_info is not None:
            H = H + prior_info[t]
            g0 = g0 + prior_grad[t]
        try:
            np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            minfo[t] = 1
            continue
        E = A0.T @ B
        X = np.linalg.solve(H, np.concatenate([E, g0[:, None]], 1))
        lp = B.T @ B - E.T @ X[:, :NV]
        info[t], eta[t] = 0.5 * (lp + lp.T), -(B.T @ r - E.T @ X[:, NV])
    return info, eta, minfo
