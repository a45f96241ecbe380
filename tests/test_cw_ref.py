"""The numpy reference of the constant-velocity factor on the angular velocity (tests/cw_ref.py),
checked on the CPU: its dense rows against finite differences of its residual, and with the
factor absent it is lm_ref / gn_ref exactly."""
import numpy as np

import cw_ref
import lm_ref
from oracle import gn_ref as G

ISIG = np.array([20.0, 10.0, 40.0])


def _factors(T, L, rot=0.3, seed=5, isig_cw=None):
    pr = lm_ref.problem(T, L, rot, seed)
    rng = np.random.default_rng(seed + 1)
    pr["angvel"] = 0.3 * rng.standard_normal((T * L, 3))
    pr["vel"] = 0.01 * rng.standard_normal((T * L, 3))
    y, P, V, W = (pr[k].reshape(T, L, -1) for k in ("y", "pose", "vel", "angvel"))
    fs = [cw_ref.factors(y[t], P[t], V[t], W[t], L, isig_cw=isig_cw) for t in range(T)]
    return pr, fs


def test_rows_match_finite_differences():
    """d r / d angvel by central differences (the residual is linear: exact up to rounding)."""
    T, L, h = 2, 5, 1e-3
    rng = np.random.default_rng(0)
    w = rng.standard_normal((T * L, 3))
    r0 = cw_ref.residual(w, L, ISIG)
    assert r0.shape == (T * (L - 1), 3)
    np.testing.assert_array_equal(r0.reshape(T, L - 1, 3), (w.reshape(T, L, 3)[:, 1:] - w.reshape(T, L, 3)[:, :-1]) * ISIG)
    dense = cw_ref.rows(r0, ISIG, T, L)
    for t in range(T):
        A, r = dense[t]
        np.testing.assert_array_equal(r, r0.reshape(T, -1)[t])
        assert A.shape == (3 * (L - 1), 12 * L)
        fd = np.zeros_like(A)
        for l in range(L):
            for i in range(3):
                wp, wm = w.copy(), w.copy()
                wp[t * L + l, i] += h
                wm[t * L + l, i] -= h
                d = (cw_ref.residual(wp, L, ISIG) - cw_ref.residual(wm, L, ISIG)) / (2 * h)
                fd[:, l * 12 + 6 + i] = d.reshape(T, -1)[t]
        np.testing.assert_allclose(A, fd, rtol=1e-10, atol=1e-10)
        # only angular-velocity columns, -s on frame l and +s on frame l + 1
        mask = np.zeros(12 * L, bool)
        for l in range(L):
            mask[l * 12 + 6:l * 12 + 9] = True
        assert not A[:, ~mask].any()


def test_normal_equations_closed_form():
    """What the device folds in (include/perseus_amd.h): D_l[6+i][6+i] += s_i^2 per pair touching l,
    E_l[6+i][6+i] -= s_i^2, g_l[6+i] += s_i (r_{l-1,i} - r_{l,i})."""
    T, L = 1, 4
    rng = np.random.default_rng(1)
    r = rng.standard_normal((L - 1, 3))
    (A, rr), = cw_ref.rows(r, ISIG, T, L)
    D, E = G.blocks(A.T @ A, L)
    g = (A.T @ rr).reshape(L, 12)
    for l in range(L):
        want = np.zeros((12, 12))
        want[6:9, 6:9] = np.diag(ISIG ** 2) * ((l > 0) + (l + 1 < L))
        np.testing.assert_allclose(D[l], want, rtol=1e-15)
        gw = np.zeros(12)
        gw[6:9] = ISIG * ((r[l - 1] if l > 0 else 0.0) - (r[l] if l + 1 < L else 0.0))
        # (s (a - b) against s a - s b: a few ulps of the larger term)
        np.testing.assert_allclose(g[l], gw, rtol=1e-13, atol=1e-13 * np.abs(ISIG * r).max())
    for l in range(L - 1):
        want = np.zeros((12, 12))
        want[6:9, 6:9] = -np.diag(ISIG ** 2)
        np.testing.assert_allclose(E[l], want, rtol=1e-15)


def test_absent_factor_is_the_parent_reference_exactly():
    T, L = 2, 6
    pr, fs = _factors(T, L)
    for t, f in enumerate(fs):
        assert "r_cw" not in f and cw_ref.cost(f) == lm_ref.cost(f)
        (A, r), = cw_ref.stack(f, 1, L, 8)
        (A0, r0), = G.stack(f, 1, L, 8)
        np.testing.assert_array_equal(A, A0)
        np.testing.assert_array_equal(r, r0)
        for a, b in zip(cw_ref.gn_step(f, 1, L, 8, 1e-3), G.gn_step(f, 1, L, 8, 1e-3)):
            np.testing.assert_array_equal(a, b)
    params = dict(lm_ref.PARAMS, max_iters=4)
    a = cw_ref.solve(pr["y"], pr["pose"], pr["vel"], pr["angvel"], T, L, params)
    b = lm_ref.solve(pr["y"], pr["pose"], pr["vel"], pr["angvel"], T, L, params)
    for k in ("pose", "vel", "angvel", "cost0", "cost", "iters", "status", "lambda", "cost_hist"):
        np.testing.assert_array_equal(a[k], b[k])


def test_factor_adds_its_cost_and_rows():
    T, L = 1, 5
    _, (f,) = _factors(T, L, isig_cw=ISIG)
    assert f["r_cw"].shape == (L - 1, 3) and f["err_cw"].shape == (L - 1,)
    assert cw_ref.cost(f) == lm_ref.cost(f) + float(f["err_cw"].sum())
    (A, r), = cw_ref.stack(f, 1, L, 8, ISIG)
    (A0, r0), = G.stack(f, 1, L, 8)
    assert A.shape[0] == A0.shape[0] + 3 * (L - 1)
    np.testing.assert_array_equal(A[:A0.shape[0]], A0)
    np.testing.assert_array_equal(r[A0.shape[0]:], f["r_cw"].reshape(-1))
    # lambda = 0 on a full window: singular without the factor (the last frame's angular velocity
    # is in no factor), solvable with it
    assert np.isnan(G.gn_step(f, 1, L, 8, 0.0)[2]).all()
    assert np.isfinite(cw_ref.gn_step(f, 1, L, 8, 0.0, ISIG)[2]).all()
