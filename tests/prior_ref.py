"""TEST HELPER (not a test): numpy f64 references for the fixed-lag marginalization prior
(include/perseus_amd.h "fixed-lag marginalization"; csrc/prior.hip).

The prior on a window's oldest frame is (Lambda (12, 12), eta (12), xbar): with
    xi = [Logmap(xbar_pose^-1 pose); angvel - xbar_angvel; vel - xbar_vel]
(oracle.factors_ref's Logmap) its cost is 0.5 xi^T Lambda xi - eta^T xi and, the chart's Jacobian
taken as the identity, it adds Lambda to D_0 and grad = Lambda xi - eta to g_0.

`linearize`: xi, grad, err of pa_window_prior_linearize.

`marginalize`: the dense Schur complement of frame 0.  The rows of the stacked whitened Jacobian
that touch x_0 (oracle.gn_ref.stack's row stacking on the two-frame sub-problem of frames 0 and 1
with frame 1's own projection rows left out: frame 0's projection factors and the dynamics and
constant-velocity factors of the pair (0, 1)) give A = [A_0 | B] and r, and with
    H = A_0^T A_0 + Lambda_in + lam I,  E = A_0^T B,  F = B^T B,  g_0 = A_0^T r,  h = B^T r:
    Lambda' = F - E^T H^-1 E,   g' = h - E^T H^-1 (g_0 + grad_in),   eta' = -g'
(+ Lambda' delta_1 on g' when the window was retracted by delta after the linearization).
minfo: 0 computed, 1 H not positive definite (Cholesky fails), 2 nvalid < L; the prior is zero in
both non-zero cases.

`dense_delta`: (A^T A + lam I + prior on frame 0) delta = -(A^T r + grad on frame 0), dense.
`drop_frame0`: the factors of frames 1 .. L-1 of every trajectory (numpy arrays or torch tensors).
"""
from __future__ import annotations

import numpy as np

from oracle import factors_ref as F
from oracle import gn_ref as G

NV = G.NV
PROJ = ("r_proj", "j_proj", "status", "err_proj")
PAIR = ("r_dyn", "j_dyn0", "j_dyn1", "j_dyn2", "j_dyn3", "err_dyn", "r_cv", "j_cv0", "j_cv1", "err_cv")


def xi(xbar_pose, xbar_angvel, xbar_vel, pose, angvel, vel):
    """(12,) of one frame: pose arrays are the 12-double encoding (R row-major, t)."""
    d = F.pose_log(F.between(F.unpack(np.asarray(xbar_pose)), F.unpack(np.asarray(pose))))
    return np.concatenate([d, np.asarray(angvel) - np.asarray(xbar_angvel), np.asarray(vel) - np.asarray(xbar_vel)])


def linearize(info, eta, xbar_pose, xbar_angvel, xbar_vel, pose, angvel, vel, L: int, frame: int):
    """(xi (T, 12), grad (T, 12), err (T,)) of window frame `frame`; pose (T*L, 12), angvel / vel (T*L, 3)."""
    T = len(info)
    x = np.stack([xi(xbar_pose[t], xbar_angvel[t], xbar_vel[t], pose[t * L + frame], angvel[t * L + frame],
                     vel[t * L + frame]) for t in range(T)])
    lx = np.einsum("tij,tj->ti", info, x)
    return x, lx - eta, 0.5 * np.einsum("ti,ti->t", x, lx) - np.einsum("ti,ti->t", eta, x)


def _pair01(f: dict, t: int, L: int, K: int):
    """(A (rows, 24), r) of the factor rows that touch x_0 of trajectory t."""
    p0 = (t * L) * K
    u = t * (L - 1)
    sub = {k: f[k][u:u + 1] for k in PAIR if f.get(k) is not None}
    st = f.get("status")
    st0 = np.zeros(K, np.int32) if st is None else np.asarray(st[p0:p0 + K])
    sub["status"] = np.concatenate([st0, np.ones(K, np.int32)])  # frame 1's own projections stay out
    if K:
        sub["r_proj"], sub["j_proj"] = f["r_proj"][p0:p0 + 2 * K], f["j_proj"][p0:p0 + 2 * K]
    return G.stack(sub, 1, 2, K)[0]


def operand_scale(f: dict, T: int, L: int, K: int):
    """Per trajectory ((T,), (T,)): the largest entry of [A_0 | B]^T [A_0 | B], the blocks H, E, F
    that Lambda' is the Schur complement of, and of [A_0 | B]^T r, the g_0 and h that g' is made
    of (the scales test_gn_gpu's atol uses for assembled blocks and for g)."""
    sm, sg = [], []
    for t in range(T):
        A, r = _pair01(f, t, L, K)
        sm.append(np.abs(A.T @ A).max())
        sg.append(np.abs(A.T @ r).max())
    return np.array(sm), np.array(sg)


def marginalize(f: dict, T: int, L: int, K: int, lam: float, prior_info=None, prior_grad=None, delta=None,
                gn_info=None, nvalid=None):
    """(info (T, 12, 12), eta (T, 12), minfo (T,)); delta (T*L, 12) or None."""
    info, eta, minfo = np.zeros((T, NV, NV)), np.zeros((T, NV)), np.zeros(T, np.int32)
    for t in range(T):
        if nvalid is not None and nvalid[t] < L:
            minfo[t] = 2
            continue
        A, r = _pair01(f, t, L, K)
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
        lp = 0.5 * (lp + lp.T)
        gp = B.T @ r - E.T @ X[:, NV]
        if delta is not None and (gn_info is None or gn_info[t] == 0):
            gp = gp + lp @ np.asarray(delta).reshape(T, L, NV)[t, 1]
        info[t], eta[t] = lp, -gp
    return info, eta, minfo


def dense_delta(f: dict, T: int, L: int, K: int, lam: float, prior_info=None, prior_grad=None):
    """delta (T, 12 L) of the dense solve with the prior on frame 0."""
    out = []
    for t, (A, r) in enumerate(G.stack(f, T, L, K)):
        H = A.T @ A + lam * np.eye(A.shape[1])
        g = A.T @ r
        if prior_info is not None:
            H[:NV, :NV] += prior_info[t]
            g[:NV] += prior_grad[t]
        out.append(np.linalg.solve(H, -g))
    return np.stack(out)


def drop_frame0(f: dict, T: int, L: int, K: int) -> dict:
    """The factor arrays of frames 1 .. L-1 (an (L-1)-frame window per trajectory)."""
    pi = [(t * L + l) * K + k for t in range(T) for l in range(1, L) for k in range(K)]
    qi = [t * (L - 1) + l for t in range(T) for l in range(1, L - 1)]
    out = {}
    for k, v in f.items():
        if v is None or not (k in PROJ or k in PAIR):
            continue
        idx = np.asarray(pi if k in PROJ else qi, np.int64)
        if not isinstance(v, np.ndarray):  # a torch tensor: index on its device
            import torch

            idx = torch.as_tensor(idx, device=v.device)
        out[k] = v[idx]
    return out


def random_spd(rng, T: int, scale: float = 1.0):
    """(T, 12, 12) symmetric positive definite, and a (T, 12) gradient."""
    m = rng.standard_normal((T, NV, NV))
    return scale * (np.einsum("tij,tkj->tik", m, m) + NV * np.eye(NV)), scale * rng.standard_normal((T, NV))
