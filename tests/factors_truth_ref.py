"""60-digit reference of the smoother factors (CPU only, mpmath; no GPU test imports it).

oracle/factors_ref.py restates the GTSAM 4.2 closed forms branch for branch, so it shares
every series branch, threshold and cancellation with the kernels.  This module shares none
of them: exp is `mpmath.expm` of the 4x4 twist, log is atan2 plus the exact V^-1, and the
Jacobians are central differences over right perturbations at h = 1e-25, all at
`mp.dps = 60` (truncation ~1e-50, rounding ~1e-35).  Inputs are the f64 values exactly.

Tangent order [omega; v], right perturbations, poses 12 f64 = R row-major then t
(oracle/factors_ref.py's encoding).
"""
from __future__ import annotations

import functools

import mpmath as mp
import numpy as np

DPS = 60
H_FD = "1e-25"


def _at_dps(fn):
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        with mp.workdps(DPS):
            return fn(*a, **kw)
    return wrapped


def _mpv(x):
    return [mp.mpf(float(t)) for t in np.asarray(x, np.float64).reshape(-1)]


def _mat(p12):
    """12 f64 -> 4x4 mp matrix."""
    p = _mpv(p12)
    M = mp.eye(4)
    for r in range(3):
        for c in range(3):
            M[r, c] = p[3 * r + c]
        M[r, 3] = p[9 + r]
    return M


def _inv(T):
    M = mp.eye(4)
    for r in range(3):
        for c in range(3):
            M[r, c] = T[c, r]
    for r in range(3):
        M[r, 3] = -sum(T[k, r] * T[k, 3] for k in range(3))
    return M


def se3_exp(xi):
    """Exp of the twist [omega; v] (6 mpf) as a 4x4 matrix, by mpmath.expm."""
    w0, w1, w2, v0, v1, v2 = xi
    if not any(xi):
        return mp.eye(4)
    return mp.expm(mp.matrix([[0, -w2, w1, v0], [w2, 0, -w0, v1], [-w1, w0, 0, v2], [0, 0, 0, 0]]))


def se3_log(T):
    """[omega; u] of a 4x4 pose: theta = atan2(sin, cos) from the antisymmetric part and the
    trace, omega = theta / (2 sin theta) vee, u = V^-1 t with the exact
    V^-1 = I - W/2 + (1/theta^2 - (1 + cos theta) / (2 theta sin theta)) W^2."""
    vee = [T[2, 1] - T[1, 2], T[0, 2] - T[2, 0], T[1, 0] - T[0, 1]]
    s = mp.sqrt(sum(x * x for x in vee)) / 2
    c = (T[0, 0] + T[1, 1] + T[2, 2] - 1) / 2
    th = mp.atan2(s, c)
    k = th / (2 * s) if s != 0 else mp.mpf(1) / 2
    w = [k * x for x in vee]
    if th < mp.mpf("1e-15"):  # 1/th^2 - ... loses 2 log10(1/th) digits; its series is exact to th^6 here
        b = mp.mpf(1) / 12 + th * th / 720 + th ** 4 / 30240
    else:
        b = 1 / (th * th) - (1 + mp.cos(th)) / (2 * th * mp.sin(th))
    t = [T[0, 3], T[1, 3], T[2, 3]]

    def cross(a, x):
        return [a[1] * x[2] - a[2] * x[1], a[2] * x[0] - a[0] * x[2], a[0] * x[1] - a[1] * x[0]]

    wt = cross(w, t)
    wwt = cross(w, wt)
    u = [t[i] - wt[i] / 2 + b * wwt[i] for i in range(3)]
    return w + u


def _dyn_residual(x0, w, v, x1, dt, vel_frame, d0=None, dw=None, dv=None, d3=None):
    if d0 is not None:
        x0 = x0 * se3_exp(d0)
    if d3 is not None:
        x1 = x1 * se3_exp(d3)
    if dw is not None:
        w = [a + b for a, b in zip(w, dw)]
    if dv is not None:
        v = [a + b for a, b in zip(v, dv)]
    if vel_frame == "world":
        vb = [sum(x0[k, i] * v[k] for k in range(3)) for i in range(3)]  # R0^T v
    else:
        vb = v
    pred = x0 * se3_exp([dt * a for a in w] + [dt * a for a in vb])
    return se3_log(_inv(pred) * x1)


def _fd(fn, dim):
    """Central differences of fn(delta) (a list of mpf) over `dim` unit directions."""
    h = mp.mpf(H_FD)
    cols = []
    for k in range(dim):
        d = [mp.mpf(0)] * dim
        d[k] = h
        fp = fn(d)
        d[k] = -h
        fm = fn(d)
        cols.append([(a - b) / (2 * h) for a, b in zip(fp, fm)])
    return np.array([[float(cols[c][r]) for c in range(dim)] for r in range(len(cols[0]))])


@_at_dps
def dynamics(T1, w, v, T2, dt, vel_frame="world", jac=True):
    """PoseDynamicsFactor: r (6,) and [J0 6x6, J1 6x3, J2 6x3, J3 6x6] (or None), rounded
    to f64 from the 60-digit values.  T1 / T2 are 12-vectors, dt a float."""
    x0, x1 = _mat(T1), _mat(T2)
    w, v = _mpv(w), _mpv(v)
    dt = mp.mpf(float(dt))
    f = functools.partial(_dyn_residual, x0, w, v, x1, dt, vel_frame)
    r = np.array([float(x) for x in f()])
    if not jac:
        return r, None
    return r, [_fd(lambda d: f(d0=d), 6), _fd(lambda d: f(dw=d), 3), _fd(lambda d: f(dv=d), 3),
               _fd(lambda d: f(d3=d), 6)]


def _proj_residual(xb, pb, z, K, xc, d=None):
    if d is not None:
        xb = xb * se3_exp(d)
    pw = [sum(xb[r, k] * pb[k] for k in range(3)) + xb[r, 3] for r in range(3)]
    q = [pw[r] - xc[r, 3] for r in range(3)]
    pc = [sum(xc[k, i] * q[k] for k in range(3)) for i in range(3)]  # Rc^T (pw - tc)
    if pc[2] <= 0:
        return None
    x, y = pc[0] / pc[2], pc[1] / pc[2]
    fx, fy, s, u0, v0 = K
    return [fx * x + s * y + u0 - z[0], fy * y + v0 - z[1]]


@_at_dps
def projection(Tb, p_b, z, K, Tc=None):
    """KeypointProjectionFactor with Cal3_S2 K = (fx, fy, s, u0, v0) and a camera pose (12 or
    None = identity): (r (2,), J (2, 6), status); status 1 = pc.z <= 0, r and J NaN."""
    xb = _mat(Tb)
    xc = mp.eye(4) if Tc is None else _mat(Tc)
    pb, z, K = _mpv(p_b), _mpv(z), _mpv(K)
    f = functools.partial(_proj_residual, xb, pb, z, K, xc)
    r = f()
    if r is None:
        return np.full(2, np.nan), np.full((2, 6), np.nan), 1
    return np.array([float(x) for x in r]), _fd(lambda d: f(d=d), 6), 0


# --------------------------------------------------------------------------------------
# input construction in 60 digits, rounded once to f64 (independent of the host's libm)
@_at_dps
def pose_exp12(xi):
    """12-vector of Exp(xi), xi 6 f64."""
    return _pack(se3_exp(_mpv(xi)))


def _pack(M):
    return np.array([float(M[r, c]) for r in range(3) for c in range(3)] + [float(M[r, 3]) for r in range(3)])


@_at_dps
def predict_then_offset(T1, w, v, dt, vel_frame, e):
    """T2 = T1 Exp(dt [w; v_b]) Exp(e) as a 12-vector (e 6 f64): the second pose of a dynamics
    case whose residual is e up to the f64 rounding of T2."""
    x0 = _mat(T1)
    w, v = _mpv(w), _mpv(v)
    dt = mp.mpf(float(dt))
    vb = [sum(x0[k, i] * v[k] for k in range(3)) for i in range(3)] if vel_frame == "world" else v
    return _pack(x0 * se3_exp([dt * a for a in w] + [dt * a for a in vb]) * se3_exp(_mpv(e)))
