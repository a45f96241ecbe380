"""TEST HELPER (not a test): GTSAM's noiseModel::Robust on the projection factors, in numpy.

`apply` takes one trajectory's whitened factors (lm_ref.factors' dict) and, on every projection
row with status 0, with n = |r_w|_2 and k > 0 (include/perseus_amd.h, "Robust noise models"):

    Huber   w = 1 (n <= k), k / n (n > k);   rho = n^2 / 2 (n <= k), k (n - k / 2) (n > k)
    Cauchy  w = 1 / (1 + n^2 / k^2);         rho = (k^2 / 2) log1p(n^2 / k^2)

    r_proj <- sqrt(w) r_proj,   j_proj <- sqrt(w) j_proj,   err_proj <- rho

Rows with another status (cheirality NaN, frames outside nvalid, a pending newest frame) stay as
they are.  `substituted` puts the wrapped factors in lm_ref.factors' place for the length of a
`with` block, so lm_ref.solve_one / solve run the device's IRLS decision for decision: the step
is Gauss-Newton on the sqrt(w)-scaled rows, the accept test compares sums of rho.

Also the two outlier problems the robust tests share (numpy only): the batch LM problem and the
streaming tick chain with one corner 40 px off on every fourth tick.
"""
from __future__ import annotations

import contextlib

import numpy as np

import lm_ref
from oracle import factors_ref as F
from oracle import gn_ref as G

KINDS = {"huber": 1, "cauchy": 2}  # PA_ROBUST_HUBER, PA_ROBUST_CAUCHY
PX = 1.0 / 127.5  # one pixel of a 256-wide image in normalized keypoint coordinates


def weight(kind, k, n):
    n = np.asarray(n, np.float64)
    if kind == "huber":
        return np.where(n <= k, 1.0, k / np.maximum(n, k))
    if kind == "cauchy":
        return 1.0 / (1.0 + n * n / (k * k))
    raise ValueError(kind)


def loss(kind, k, n):
    n = np.asarray(n, np.float64)
    if kind == "huber":
        with np.errstate(over="ignore"):  # (the branch not taken, at a huge k)
            return np.where(n <= k, 0.5 * n * n, k * (n - 0.5 * k))
    if kind == "cauchy":
        return 0.5 * k * k * np.log1p(n * n / (k * k))
    raise ValueError(kind)


def apply(f, kind, k):
    """The robust-weighted copy of one trajectory's factors; kind None: f itself."""
    if kind is None:
        return f
    f = dict(f)
    ok = f["status"] == 0
    n = np.sqrt((f["r_proj"][ok] ** 2).sum(1))
    sw = np.sqrt(weight(kind, k, n))
    for key in ("r_proj", "j_proj", "err_proj"):
        f[key] = f[key].copy()
    f["r_proj"][ok] *= sw[:, None]
    f["j_proj"][ok] *= sw[:, None, None]
    rho = loss(kind, k, n)
    if kind == "huber":  # n <= k: the plain factor, to the bit
        rho = np.where(n <= k, f["err_proj"][ok], rho)
    f["err_proj"][ok] = rho
    return f


_plain_factors = lm_ref.factors


def factors(kind, k):
    """lm_ref.factors with the robust projection rows."""
    def wrapped(*a, **kw):
        return apply(_plain_factors(*a, **kw), kind, k)
    return wrapped


@contextlib.contextmanager
def substituted(robust):
    """robust: None or (kind, k).  lm_ref.factors is the robust one inside the block."""
    if robust is None:
        yield
        return
    lm_ref.factors = factors(*robust)
    try:
        yield
    finally:
        lm_ref.factors = _plain_factors


def solve(pr, T, L, params, robust=None, **kw):
    with substituted(robust):
        return lm_ref.solve(pr["y"], pr["pose"], pr["vel"], pr["angvel"], T, L, params, **kw)


# ---------------------------------------------------------------- the batch LM outlier problem
LM_T, LM_L = 3, 6
LM_PARAMS = dict(lm_ref.PARAMS, max_iters=60)


def lm_problem():
    """lm_ref.problem(3, 6, 0.3) with corner 2 +40 px in x in frames 1-4 and corner 5 -30 px in y
    in frames 2-3, in every trajectory."""
    pr = lm_ref.problem(LM_T, LM_L, 0.3)
    y = pr["y"].reshape(LM_T, LM_L, 8, 2).copy()
    y[:, 1:5, 2, 0] += np.float32(40 * PX)
    y[:, 2:4, 5, 1] -= np.float32(30 * PX)
    pr["y"] = y.reshape(LM_T * LM_L, 16)
    return pr


# ---------------------------------------------------------------- the streaming outlier chain
ST_N, ST_L, ST_TICKS, ST_LAM = 2, 8, 40, 1e-2
ST_SIGMAS = dict(proj=1.0, dyn=0.1, cv=0.1)  # StreamingPipeline's defaults
ST_INIT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0.4], np.float64)  # and its default init_pose


def stream_sequence():
    """(truth, ys): lm_ref.truth(2, 40) and its keypoints per tick, corner 2 +40 px in x on every
    tick with tick % 4 == 1."""
    truth, _, _ = lm_ref.truth(ST_N, ST_TICKS)
    ys = []
    for k in range(ST_TICKS):
        y = lm_ref.keypoints(truth[k]).reshape(ST_N, 8, 2).copy()
        if k % 4 == 1:
            y[:, 2, 0] += np.float32(40 * PX)
        ys.append(y.reshape(ST_N, 16))
    return truth, ys


def newest_rot_errors(poses, truth_tick):
    return lm_ref.pose_errors(poses, [F.pack(T) for T in truth_tick])[0]


def stream_chain(truth, ys, robust=None):
    """The streaming tick in numpy: advance -> linearize -> one GN step (lambda 1e-2) -> retract
    per tick, from the reset window.  Returns the newest pose's rotation error (ticks, n)."""
    n, L = ST_N, ST_L
    win = {"y": np.zeros((n, L, 16), np.float32), "pose": np.tile(ST_INIT, (n, L, 1)),
           "angvel": np.zeros((n, L, 3)), "vel": np.zeros((n, L, 3))}
    kind, k = robust if robust is not None else (None, 0.0)
    errs = []
    for tick, y_new in enumerate(ys):
        win = F.window_advance(win, y_new, lm_ref.DT, "world")
        nv = min(tick + 1, L)
        delta = np.zeros((n, L, 12))
        info = np.zeros(n, np.int32)
        for c in range(n):
            f = apply(_plain_factors(win["y"][c], win["pose"][c], win["vel"][c], win["angvel"][c], L,
                                     sigmas=ST_SIGMAS, nvalid=nv), kind, k)
            _, _, d = G.gn_step(f, 1, L, 8, ST_LAM)
            if np.isfinite(d).all():
                delta[c] = d.reshape(L, 12)
            else:
                info[c] = 1
        win = F.window_retract(win, delta.reshape(n * L, 12), info)
        errs.append(newest_rot_errors(win["pose"][:, -1], truth[tick]))
    return np.array(errs)
