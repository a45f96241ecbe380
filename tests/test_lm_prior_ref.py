"""tests/lm_prior_ref.py (the numpy Levenberg-Marquardt solve with a marginalization prior) on its
own: the conditions the device tests (tests/test_lm_prior_gpu.py) rely on hold on the reference.

  1. fixed lag reproduces batch: the 6-frame solve with the marginal prior of the dropped frame
     lands on the 7-frame solve; without the prior it does not;
  2. case A: under a strong prior every one of the 8 decisions is taken with a margin f64 rounding
     cannot flip, rejects and accepts among them;
  3. case B: the cost goes negative, and the convergence test on |C| stops where the parent's
     rel_tol * C would not;
  4. no prior, and the zero prior, are lm_ref.solve_one exactly.
"""
import numpy as np
import pytest

import lm_prior_ref as R
import lm_ref

MARGIN = 1e-6
KEYS = ("pose", "vel", "angvel", "cost0", "cost", "iters", "status", "lambda", "cost_hist")


def _solve(pr, L, params, prior=None, **kw):
    return R.solve_one(pr["y"], pr["pose"], pr["vel"], pr["angvel"], L, params, prior=prior, **kw)


@pytest.mark.parametrize("seed", R.SEEDS)
def test_fixed_lag_reproduces_batch(seed):
    c = R.fixed_lag(seed)
    assert c["batch"]["status"] == R.CONVERGED
    with_prior = _solve(c["sub"], 6, R.TIGHT, c["prior"])
    without = _solve(c["sub"], 6, R.TIGHT)
    dw, do = R.distance(with_prior, c["batch"]), R.distance(without, c["batch"])
    print(f"seed {seed}: distance from the 7-frame solve {dw:.3g} with the prior, {do:.3g} without")
    assert dw <= 1e-7  # measured <= 7.9e-9
    assert do >= 1e-3  # measured >= 1.56e-2


@pytest.mark.parametrize("seed", R.SEEDS)
def test_case_a_rejects_under_a_prior(seed):
    pr, prior = R.case("A", seed)
    ref = _solve(pr, 6, R.PARITY, prior)
    margins = [r["margin"] for r in ref["log"]]
    acc = [r["accept"] for r in ref["log"]]
    print(f"seed {seed}: accepts {acc}, smallest margin {min(margins):.3g}")
    assert len(margins) == 8 and min(margins) >= MARGIN  # measured >= 6.7e-3
    assert any(acc) and not all(acc)  # measured 4 / 6 / 5 rejects


@pytest.mark.parametrize("seed", R.SEEDS)
def test_case_b_cost_goes_negative(seed):
    pr, prior = R.case("B", seed)
    ref = _solve(pr, 6, R.PARITY, prior)
    print(f"seed {seed}: cost_hist {ref['cost_hist']}, margins {[r['margin'] for r in ref['log']]}")
    assert all(r["margin"] >= MARGIN for r in ref["log"][:4])  # the fourth: 2.9e-3 / 5.1e-5 / 1.2e-3
    assert ref["cost_hist"][0] > 0 and ref["cost"] < 0


def test_case_b_converges_on_the_magnitude_of_a_negative_cost():
    """Seed 6, rel_tol 1e-3: CONVERGED at iteration 4 with C < 0.  With the parent's rel_tol * C the
    tolerance is negative there and the accepted step's decrease C - C' > 0 can never meet it."""
    pr, prior = R.case("B", 6)
    params = dict(R.PARITY, rel_tol=1e-3)
    ref = _solve(pr, 6, params, prior)
    assert ref["status"] == R.CONVERGED and ref["iters"] == 4 and ref["cost"] < 0, (ref["status"], ref["iters"])
    assert ref["cost_hist"][3] < 0  # the C the test was taken on
    assert all(r["margin"] >= MARGIN for r in ref["log"])
    signed = _solve(pr, 6, params, prior, abs_in_tol=False)
    assert not (signed["status"] == R.CONVERGED and signed["iters"] == 4)


@pytest.mark.parametrize("rot,params", [(0.8, R.PARITY), (0.1, lm_ref.PARAMS)])
def test_no_prior_and_zero_prior_are_the_parent(rot, params):
    pr = lm_ref.problem(1, 6, rot)
    want = lm_ref.solve_one(pr["y"], pr["pose"], pr["vel"], pr["angvel"], 6, params)
    for prior in (None, R.zero_prior()):
        got = _solve(pr, 6, params, prior)
        for k in KEYS:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        assert [r["accept"] for r in got["log"]] == [r["accept"] for r in want["log"]]
