"""The numpy restatement of pa_trajectory_marginals' block recursion (tests/marginals_ref.py)
against the dense inverse np.linalg.inv(H + lam I), on lm_ref.problem windows (0.1 rad off the
truth, at rest) linearized by lm_ref.factors.  No GPU.

Metric: marginals_ref.scaled_err, |delta_ij| / sqrt(ref_ii ref_jj).  Bound 1e-10: a tenth of
the device test's 1e-9 (test_marginals_gpu.py), so that the two references' own disagreement
takes at most a tenth of what the device is allowed.

Measured here (worst of cov and cross, numpy / LAPACK f64):
    full windows, L = 2, 5, 24, lam = 1e-9 and 1e-3      <= 1.1e-13
    nvalid = 3 of 8, lam = 1e-3                             1.2e-11
    nvalid = 1 of 24, lam = 1e-2                            1.3e-12
    pending newest frame, L = 24, lam = 1e-2                8.0e-14
(lam <= 1e-3 with nvalid = 1, or lam = 1e-6 on any partly filled window, is left out on purpose:
there the dense inverse itself is only good to 1e-10 .. 1e-4 and is no reference.)
"""
import numpy as np
import pytest

import lm_ref  # tests/ is on sys.path (rootdir conftest)
import marginals_ref as MR

BOUND = 1e-10
NK = 8


def _factors(L, seed=5, nvalid=None, pending=False):
    pr = lm_ref.problem(1, L, 0.1, seed=seed)
    return lm_ref.factors(pr["y"], pr["pose"], pr["vel"], pr["angvel"], L, nvalid=nvalid, pending=pending)


CASES = [(2, 1e-9, None, False), (2, 1e-3, None, False), (5, 1e-9, None, False), (5, 1e-3, None, False),
         (24, 1e-9, None, False), (24, 1e-3, None, False), (8, 1e-3, 3, False), (24, 1e-2, 1, False),
         (24, 1e-2, None, True)]


@pytest.mark.parametrize("L,lam,nvalid,pending", CASES)
def test_recursion_matches_dense_inverse(L, lam, nvalid, pending):
    f = _factors(L, nvalid=nvalid, pending=pending)
    ref_cov, ref_cross = MR.dense(f, 1, L, NK, lam)
    cov, cross = MR.recursion(f, 1, L, NK, lam)
    e_cov, e_cross = MR.scaled_err(cov, cross, ref_cov, ref_cross)
    print(f"L={L} lam={lam:g} nvalid={nvalid} pending={pending}: cov {e_cov:.3g}, cross {e_cross:.3g}")
    assert e_cov <= BOUND and e_cross <= BOUND
    for l in range(L):
        assert np.array_equal(cov[0, l], cov[0, l].T) and (np.diag(cov[0, l]) > 0).all()


def test_unconstrained_angular_velocity_sits_at_one_over_lambda():
    """Full window: the last frame's angular velocity is in no factor, so its marginal is the
    prior's alone, 1 / lam, decoupled from everything else."""
    L, lam = 5, 1e-9
    cov, _ = MR.recursion(_factors(L), 1, L, NK, lam)
    blk = cov[0, L - 1]
    np.testing.assert_allclose(blk[6:9, 6:9], np.eye(3) / lam, rtol=1e-12, atol=0)
    assert (blk[6:9, :6] == 0).all() and (blk[6:9, 9:] == 0).all()


def test_dense_blocks_are_the_inverse_blocks():
    """`dense` cuts the blocks where the kernel's outputs are defined: cov_l = Sigma[l, l],
    cross_l = Sigma[l, l+1] (frame l on rows)."""
    L, lam = 3, 1e-3
    f = _factors(L)
    H = MR.normal_matrices(f, 1, L, NK)[0]
    S = np.linalg.inv(H + lam * np.eye(12 * L))
    cov, cross = MR.dense(f, 1, L, NK, lam)
    assert np.array_equal(cov[0, 1], S[12:24, 12:24]) and np.array_equal(cross[0, 1], S[12:24, 24:36])
