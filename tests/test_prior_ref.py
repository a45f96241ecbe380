"""CPU self-checks of the marginalization reference (tests/prior_ref.py): the Schur complement
identity its `marginalize` must obey, and the prior's xi / grad / err."""
import numpy as np
import pytest

import prior_ref as PR  # tests/ is on sys.path (rootdir conftest)
from oracle import factors_ref as F

from test_oracle_gn import _factors

NV = PR.NV


@pytest.mark.parametrize("with_prior,lam", [(True, 1e-6), (False, 1e-6), (True, 1e-2), (False, 1e-2)])
def test_schur_identity(with_prior, lam):
    """delta of frames 1 .. 3 from the dense solve of all 4 frames (with a random SPD prior on
    frame 0, or none) = the dense solve of frames 1 .. 3 alone with `marginalize`'s prior.
    (lam > 0 throughout: at lam = 0 the newest frame's angular velocity is in no factor and the
    window is singular whatever the prior, test_oracle_gn.py.)"""
    T, L, K = 2, 4, 8
    f = _factors(T, L, K, 3)
    rng = np.random.default_rng(11)
    pinfo, pgrad = PR.random_spd(rng, T) if with_prior else (None, None)
    full = PR.dense_delta(f, T, L, K, lam, pinfo, pgrad).reshape(T, L, NV)
    info, eta, minfo = PR.marginalize(f, T, L, K, lam, pinfo, pgrad)
    assert (minfo == 0).all()
    np.testing.assert_array_equal(info, info.transpose(0, 2, 1))
    red = PR.dense_delta(PR.drop_frame0(f, T, L, K), T, L - 1, K, lam, info, -eta).reshape(T, L - 1, NV)
    err = np.abs(red - full[:, 1:]).max() / np.abs(full).max()
    print(f"with_prior={with_prior} lam={lam:g}: relative deviation {err:.3g}")
    assert err <= 1e-10


def test_recentring_moves_the_gradient_only():
    T, L, K, lam = 2, 4, 8, 1e-3
    f = _factors(T, L, K, 5)
    rng = np.random.default_rng(2)
    delta = 1e-2 * rng.standard_normal((T * L, NV))
    i0, e0, _ = PR.marginalize(f, T, L, K, lam)
    i1, e1, _ = PR.marginalize(f, T, L, K, lam, delta=delta, gn_info=np.array([0, 3]))
    np.testing.assert_array_equal(i0, i1)
    np.testing.assert_allclose(e1[0], e0[0] - i0[0] @ delta.reshape(T, L, NV)[0, 1], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(e1[1], e0[1])  # gn_info != 0: nothing was retracted


def test_minfo():
    T, L, K = 3, 4, 8
    f = _factors(T, L, K, 7)
    f["status"][:] = 0
    f["status"][:K] = 1  # trajectory 0: frame 0's projections fail cheirality, and with zero dynamics
    for k in ("j_dyn0", "j_dyn1", "j_dyn2"):  # Jacobians its pose and angular velocity are in no factor
        f[k][0] = 0.0
    info, eta, minfo = PR.marginalize(f, T, L, K, 0.0, nvalid=np.array([L, L - 1, L]))
    assert minfo.tolist() == [1, 2, 0]
    assert not info[:2].any() and not eta[:2].any() and info[2].any()


def _state(rng, T):
    pose = np.stack([F.pack(F.pose_exp(np.concatenate([0.5 * rng.standard_normal(3), 0.2 * rng.standard_normal(3)])))
                     for _ in range(T)])
    return pose, rng.standard_normal((T, 3)), rng.standard_normal((T, 3))


def test_xi_and_grad():
    """xi = 0 and grad = -eta at x = xbar; at xbar (+) d, xi = d to first order (exactly for the
    velocities, and exactly for the pose too: Logmap inverts the retraction's Expmap), so
    grad = Lambda d - eta."""
    T, L = 3, 4
    rng = np.random.default_rng(4)
    info, eta = PR.random_spd(rng, T)
    xp, xw, xv = _state(rng, T)
    pose, w, v = (np.repeat(a, L, axis=0) for a in (xp, xw, xv))
    x, grad, err = PR.linearize(info, eta, xp, xw, xv, pose, w, v, L, 2)
    assert np.abs(x).max() <= 1e-15
    np.testing.assert_allclose(grad, -eta, rtol=0, atol=1e-13)
    assert np.abs(err).max() <= 1e-13
    d = 1e-3 * rng.standard_normal((T, NV))
    for t in range(T):
        f = t * L + 2
        pose[f] = F.pack(F.compose(F.unpack(xp[t]), F.pose_exp(d[t, :6])))
        w[f] = xw[t] + d[t, 6:9]
        v[f] = xv[t] + d[t, 9:]
    x, grad, err = PR.linearize(info, eta, xp, xw, xv, pose, w, v, L, 2)
    np.testing.assert_allclose(x, d, rtol=0, atol=1e-12)
    want = np.einsum("tij,tj->ti", info, d) - eta
    np.testing.assert_allclose(grad, want, rtol=0, atol=1e-9 * np.abs(want).max())
    np.testing.assert_allclose(err, 0.5 * np.einsum("ti,tij,tj->t", d, info, d) - np.einsum("ti,ti->t", eta, d),
                               rtol=1e-6, atol=1e-12)
    # the other frames still sit at xbar
    x0, _, _ = PR.linearize(info, eta, xp, xw, xv, pose, w, v, L, 1)
    assert np.abs(x0).max() <= 1e-15
