"""TEST HELPER (not a test): the Levenberg-Marquardt loop of pa_trajectory_lm_prior_solve
(include/perseus_amd.h) in numpy: lm_ref.solve_one's loop with the marginalization prior on frame 0,

  cost   C = lm_ref.cost(factors) + e_prior, e_prior = 0.5 xi^T Lambda xi - eta^T xi with xi at frame 0
         of the state being evaluated (prior_ref.linearize(frame=0));
  step   (A^T A + lam I + Lambda on frame 0) delta = -(A^T r + (Lambda xi - eta) on frame 0), xi at the
         current state (prior_ref.dense_delta; a system that is not positive definite is a failed
         pivot, as oracle.gn_ref.gn_step has it);
  sign   C may be negative: CONVERGED iff C - C' <= rel_tol |C| + abs_tol, margin = |C' - C| / |C|.

A prior is a dict of ONE trajectory's info (12, 12), eta (12), xbar_pose (12), xbar_angvel (3),
xbar_vel (3); None is lm_ref.solve_one, decision for decision and bit for bit (the same calls).
The factors come from lm_ref.factors looked up at call time, so robust_ref.substituted works here
as it does for lm_ref.solve.  `solve_one` also returns grad (12) and err of the prior at the final state.
"""
from __future__ import annotations

import numpy as np

import lm_ref
import prior_ref
from oracle import gn_ref as G

CONVERGED, MAX_ITERS, STALLED = lm_ref.CONVERGED, lm_ref.MAX_ITERS, lm_ref.STALLED
PRIOR_KEYS = ("info", "eta", "xbar_pose", "xbar_angvel", "xbar_vel")


def zero_prior():
    """No information, xbar = the identity at rest (pipeline.PriorPlan's initial prior)."""
    return dict(info=np.zeros((12, 12)), eta=np.zeros(12), xbar_pose=np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]),
                xbar_angvel=np.zeros(3), xbar_vel=np.zeros(3))


def prior_at(prior, x, L):
    """(grad (12), err) of `prior` at frame 0 of the state x = (pose, vel, angvel); (None, 0.0) without one."""
    if prior is None:
        return None, 0.0
    _, g, e = prior_ref.linearize(prior["info"][None], prior["eta"][None], prior["xbar_pose"][None],
                                  prior["xbar_angvel"][None], prior["xbar_vel"][None], x[0], x[2], x[1], L, 0)
    return g[0], float(e[0])


def step(f, L, nk, lam, prior, grad, reverse=False):
    """delta (12 L) of the damped step with the prior on frame 0; NaN where the system is not
    positive definite.  reverse: the same system solved with its unknowns in reverse order, which
    changes nothing but the rounding (own_error)."""
    if prior is None:
        return G.gn_step(f, 1, L, nk, lam)[2][0]
    A, r = G.stack(f, 1, L, nk)[0]
    H = A.T @ A + lam * np.eye(A.shape[1])
    H[:12, :12] += prior["info"]
    try:
        np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return np.full(12 * L, np.nan)
    if reverse:
        g = A.T @ r
        g[:12] += grad
        return np.linalg.solve(H[::-1, ::-1], -g[::-1])[::-1]
    return prior_ref.dense_delta(f, 1, L, nk, lam, prior["info"][None], grad[None])[0]


def solve_one(y, pose, vel, angvel, L, params=lm_ref.PARAMS, prior=None, abs_in_tol=True, reverse=False, **kw):
    """lm_ref.solve_one's dict plus grad, err (the prior at the final state; None / 0.0 without a
    prior).  log: per iteration dict(accept, why, margin, lam, cost_lower).  abs_in_tol=False: the
    parent's rel_tol * C in the convergence test (for showing what the sign rule changes)."""
    p = dict(lm_ref.PARAMS, **params)
    nk = np.asarray(y).reshape(L, -1).shape[1] // 2
    x = (np.array(pose, np.float64), np.array(vel, np.float64), np.array(angvel, np.float64))
    f = lm_ref.factors(y, *x, L, **kw)
    g, e = prior_at(prior, x, L)
    C = lm_ref.cost(f) + e
    lam = p["lambda0"]
    hist = np.full(p["max_iters"] + 1, np.nan)
    hist[0] = C
    cost0, status, iters, log = C, 0, 0, []
    for k in range(1, p["max_iters"] + 1):
        iters = k
        d = step(f, L, nk, lam, prior, g, reverse)
        rec = dict(accept=False, why="pivot", margin=np.inf, lam=lam)
        if np.isfinite(d).all():
            xn = lm_ref.retract(*x, d.reshape(L, 12))
            fn = lm_ref.factors(y, *xn, L, **kw)
            gn, en = prior_at(prior, xn, L)
            Cn = lm_ref.cost(fn) + en
            rec["margin"] = abs(Cn - C) / abs(C) if C != 0 else np.inf
            rec["cost_lower"] = Cn < C
            if ((f["status"] == 0) & (fn["status"] == 1)).any():
                rec["why"] = "cheirality"
            elif Cn < C:
                rec.update(accept=True, why="cost")
            else:
                rec["why"] = "cost"
        log.append(rec)
        if rec["accept"]:
            x, f, g, e = xn, fn, gn, en
            lam = max(lam / p["lambda_down"], p["lambda_min"])
            if C - Cn <= p["rel_tol"] * (abs(C) if abs_in_tol else C) + p["abs_tol"]:
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
                log=log, grad=g, err=e, **{"lambda": lam})


def own_error(ref, *args, **kw):
    """The reference's own rounding error on a problem, per entry: dict(pose, vel, angvel) of
    |difference| between `ref` = solve(*args, **kw) and the same solve with every step's linear
    system solved in reverse variable order (decisions asserted equal).  Where directions of the
    state are held by the damping alone (the angular velocities of a partly filled window's
    unmeasured frames) this is orders above eps, and no implementation can be asked to match the
    reference closer than it matches itself."""
    other = solve(*args, reverse=True, **kw)
    np.testing.assert_array_equal(other["iters"], ref["iters"])
    np.testing.assert_array_equal(other["status"], ref["status"])
    return {k: np.abs(other[k] - ref[k]) for k in ("pose", "vel", "angvel")}


def solve(y, pose, vel, angvel, T, L, params=lm_ref.PARAMS, priors=None, nvalid=None, **kw):
    """Every trajectory independently (priors: a list of T priors or None); stacked as the device
    returns them."""
    y = np.asarray(y).reshape(T, L, -1)
    P, V, W = (np.asarray(a, np.float64).reshape(T, L, -1) for a in (pose, vel, angvel))
    res = [solve_one(y[t], P[t], V[t], W[t], L, params, prior=None if priors is None else priors[t],
                     nvalid=None if nvalid is None else nvalid[t], **kw) for t in range(T)]
    out = {k: np.array([r[k] for r in res]) for k in ("cost0", "cost", "iters", "status", "lambda", "cost_hist")}
    for k in ("pose", "vel", "angvel"):
        out[k] = np.concatenate([r[k] for r in res], 0)
    if priors is not None:
        out["grad"] = np.array([r["grad"] for r in res])
        out["err"] = np.array([r["err"] for r in res])
    out["log"] = [r["log"] for r in res]
    return out


def stack_priors(priors):
    """A list of T priors as the (T, ...) arrays the device takes."""
    return {k: np.stack([np.asarray(p[k], np.float64) for p in priors]) for k in PRIOR_KEYS}


# ---------------------------------------------------------------- the problems the tests share
SEEDS = (5, 6, 7)
PX = 1.0 / 127.5  # one pixel in normalized keypoint coordinates
PARITY = dict(lm_ref.PARAMS, rel_tol=0.0, abs_tol=0.0, max_iters=8)  # tests/test_lm_gpu.py PARITY
TIGHT = dict(lm_ref.PARAMS, rel_tol=1e-12, abs_tol=1e-14, max_iters=40)


def noisy(pr, seed, px=0.5):
    """(pr with y + px pixels of Gaussian noise from default_rng(seed), cast to f32; the generator,
    for the draws that follow)."""
    rng = np.random.default_rng(seed)
    pr = dict(pr)
    pr["y"] = (pr["y"] + px * PX * rng.standard_normal(pr["y"].shape)).astype(np.float32)
    return pr, rng


def case(which, seed, L=6, rot=0.8):
    """Case A (a strong prior at the truth: rejects and accepts under a prior) or B (a prior whose
    eta makes the cost negative) for one seed: (problem, prior)."""
    pr, rng = noisy(lm_ref.problem(1, L, rot, seed), seed + 2000)
    info, _ = prior_ref.random_spd(rng, 1, 10.0)
    prior = dict(zero_prior(), info=info[0], xbar_pose=pr["truth"][0].copy())
    if which == "B":
        xs = 0.05 * rng.standard_normal(12)
        prior.update(info=100.0 * info[0], eta=100.0 * info[0] @ xs)
    return pr, prior


def stacked(cases):
    """[(problem, prior)] of single trajectories -> (problem of T trajectories, list of priors)."""
    pr = {k: np.concatenate([c[0][k] for c in cases]) for k in cases[0][0]}
    return pr, [c[1] for c in cases]


def fixed_lag(seed):
    """The 'fixed lag reproduces batch' construction for one seed: dict(batch: the 7-frame solve,
    prior: the marginal of frame 0 at it (on frame 1), sub: the 6-frame problem of frames 1..6
    started 0.3 rad off, pr7: the 7-frame problem)."""
    L = 7
    pr7, _ = noisy(lm_ref.problem(1, L, 0.1, seed), seed + 1000)
    batch = solve_one(pr7["y"], pr7["pose"], pr7["vel"], pr7["angvel"], L, TIGHT)
    f = lm_ref.factors(pr7["y"], batch["pose"], batch["vel"], batch["angvel"], L)
    info, eta, minfo = prior_ref.marginalize(f, 1, L, 8, 0.0)
    assert minfo[0] == 0
    prior = dict(info=info[0], eta=eta[0], xbar_pose=batch["pose"][1].copy(), xbar_angvel=batch["angvel"][1].copy(),
                 xbar_vel=batch["vel"][1].copy())
    far = lm_ref.problem(1, L, 0.3, seed)
    sub = dict(y=pr7["y"][1:], pose=far["pose"][1:], vel=far["vel"][1:], angvel=far["angvel"][1:])
    return dict(batch=batch, prior=prior, sub=sub, pr7=pr7)


def distance(sol, batch):
    """max over pose entries, vel and angvel of |sol - batch's frames 1..|."""
    return max(np.abs(np.asarray(sol[k]) - np.asarray(batch[k])[1:]).max() for k in ("pose", "vel", "angvel"))
