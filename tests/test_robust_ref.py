"""tests/robust_ref.py alone (numpy, no GPU): the m-estimators' weight / loss pair is consistent,
the wrapper leaves inliers alone, and the two claims the robust noise models were added for hold
on the numpy chains, with margin (the measured figures halved or doubled):

  batch LM (robust_ref.lm_problem), worst error against the truth, measured
      plain 0.704 rad / 4.6e-2 m, Huber 1.345 0.119 rad / 8.4e-3 m, Cauchy 1.0 5.5e-3 rad / 3.3e-4 m
  streaming chain (robust_ref.stream_chain), worst newest-pose rotation error over the last 12 ticks
      plain 0.449 rad, Huber 1.345 0.028 rad, Cauchy 1.0 5.5e-4 rad
"""
import numpy as np
import pytest

import lm_ref
import robust_ref

KS = {"huber": (0.5, 1.345, 3.0), "cauchy": (0.5, 1.0, 3.0)}


@pytest.mark.parametrize("kind", ["huber", "cauchy"])
def test_loss_derivative_is_weight_times_n(kind):
    """rho'(n) = w(n) n: IRLS on sqrt(w)-scaled rows descends rho.  Central differences, h = 1e-6:
    truncation h^2 rho''' / 6 <= 1e-12, rounding eps rho / h <= 1e-8 at rho <= 50."""
    for k in KS[kind]:
        n = np.concatenate([np.linspace(0.01, 0.99, 23) * k, np.linspace(1.01, 30.0, 41) * k])
        h = 1e-6
        d = (robust_ref.loss(kind, k, n + h) - robust_ref.loss(kind, k, n - h)) / (2 * h)
        np.testing.assert_allclose(d, robust_ref.weight(kind, k, n) * n, rtol=0, atol=1e-7)


@pytest.mark.parametrize("kind", ["huber", "cauchy"])
def test_continuous_at_k(kind):
    for k in KS[kind]:
        for f in (robust_ref.weight, robust_ref.loss):
            lo, at, hi = (f(kind, k, k * s) for s in (1 - 1e-12, 1.0, 1 + 1e-12))
            assert abs(lo - at) <= 1e-11 * max(1.0, k * k) and abs(hi - at) <= 1e-11 * max(1.0, k * k)
    assert robust_ref.weight("huber", 1.345, 1.345) == 1.0
    assert robust_ref.loss("huber", 1.345, 1.345) == 0.5 * 1.345 ** 2
    assert robust_ref.weight("cauchy", 2.0, 2.0) == 0.5


def test_huber_with_a_huge_k_is_the_plain_factor():
    pr = robust_ref.lm_problem()
    L = robust_ref.LM_L
    plain = lm_ref.factors(pr["y"][:L], pr["pose"][:L], pr["vel"][:L], pr["angvel"][:L], L)
    rob = robust_ref.factors("huber", 1e300)(pr["y"][:L], pr["pose"][:L], pr["vel"][:L], pr["angvel"][:L], L)
    assert set(plain) == set(rob)
    for key, v in plain.items():
        np.testing.assert_array_equal(rob[key], v, err_msg=key)


def test_other_statuses_are_left_alone():
    pr = robust_ref.lm_problem()
    L = robust_ref.LM_L
    a = (pr["y"][:L], pr["pose"][:L], pr["vel"][:L], pr["angvel"][:L], L)
    plain = lm_ref.factors(*a, nvalid=4, pending=True)
    rob = robust_ref.factors("cauchy", 1.0)(*a, nvalid=4, pending=True)
    out = plain["status"] != 0
    assert out.any() and (~out).any()
    for key in ("r_proj", "j_proj", "err_proj", "status"):
        np.testing.assert_array_equal(rob[key][out], plain[key][out], err_msg=key)
    assert (rob["err_proj"][~out] < plain["err_proj"][~out]).any()
    for key in plain:
        if not key.endswith("proj") and key != "status":
            np.testing.assert_array_equal(rob[key], plain[key], err_msg=key)


@pytest.fixture(scope="module")
def lm_errors():
    pr = robust_ref.lm_problem()
    out = {}
    for name, robust in (("plain", None), ("huber", ("huber", 1.345)), ("cauchy", ("cauchy", 1.0))):
        ref = robust_ref.solve(pr, robust_ref.LM_T, robust_ref.LM_L, robust_ref.LM_PARAMS, robust)
        rot, tra = lm_ref.pose_errors(ref["pose"], pr["truth"])
        out[name] = (ref, rot.max(), tra.max())
        print(f"LM {name}: status {ref['status']}, iters {ref['iters']}, {rot.max():.3g} rad, {tra.max():.3g} m")
    return out


def test_batch_lm_robust_kernels_hold_the_pose(lm_errors):
    for name, (ref, _, _) in lm_errors.items():
        assert (ref["status"] == lm_ref.CONVERGED).all(), name
        assert ref["iters"].max() <= 7, (name, ref["iters"])
    (_, rp, tp), (_, rh, th), (_, rc, _) = (lm_errors[k] for k in ("plain", "huber", "cauchy"))
    assert rp >= 4 * rh and tp >= 4 * th
    assert rc <= 1e-2


def test_streaming_chain_robust_kernels_hold_the_pose():
    truth, ys = robust_ref.stream_sequence()
    worst = {}
    for name, robust in (("plain", None), ("huber", ("huber", 1.345)), ("cauchy", ("cauchy", 1.0))):
        worst[name] = robust_ref.stream_chain(truth, ys, robust)[-12:].max()
        print(f"streaming chain {name}: worst rotation error over the last 12 ticks {worst[name]:.3g} rad")
    assert worst["huber"] <= worst["plain"] / 8
    assert worst["cauchy"] <= 1.1e-3
