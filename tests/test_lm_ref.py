"""The numpy Levenberg-Marquardt reference (tests/lm_ref.py, the restatement the device solve
pa_trajectory_lm_solve is checked against) pinned on its own: from a window 0.1 rad / 1 cm off
and from one 0.8 rad off it converges to the true trajectories within the project's bounds
(test_streaming_pose_gpu.test_pose_tracks_known_trajectory: 1e-4 rad, 1e-5 m), its cost never
increases, and the far start needs rejected steps on the way."""
import numpy as np
import pytest

import lm_ref  # tests/ is on sys.path (rootdir conftest)

T, L = 3, 6
ROT_TOL, TRA_TOL = 1e-4, 1e-5


@pytest.fixture(scope="module", params=[0.1, 0.8])
def run(request):
    pr = lm_ref.problem(T, L, request.param)
    return request.param, pr, lm_ref.solve(pr["y"], pr["pose"], pr["vel"], pr["angvel"], T, L, lm_ref.PARAMS)


def test_reference_converges_to_truth(run):
    rot0, pr, out = run
    assert (out["status"] == lm_ref.CONVERGED).all(), out["status"]
    rot, tra = lm_ref.pose_errors(out["pose"], pr["truth"])
    print(f"start {rot0} rad: iters {out['iters']}, rot err {rot.max():.3g} rad, trans err {tra.max():.3g} m")
    assert rot.max() < ROT_TOL and tra.max() < TRA_TOL
    assert (out["iters"] >= 1).all() and (out["iters"] <= lm_ref.PARAMS["max_iters"]).all()


def test_reference_cost_never_increases(run):
    _, _, out = run
    for t in range(T):
        h = out["cost_hist"][t]
        k = out["iters"][t]
        assert np.isfinite(h[:k + 1]).all() and np.isnan(h[k + 1:]).all()
        assert (np.diff(h[:k + 1]) <= 0).all()
        assert h[0] == out["cost0"][t] and h[k] == out["cost"][t]
        # a plateau is a rejected step, a drop an accepted one
        acc = np.array([r["accept"] for r in out["log"][t]])
        np.testing.assert_array_equal(np.diff(h[:k + 1]) < 0, acc)


def test_far_start_rejects_steps(run):
    rot0, _, out = run
    rejects = sum(not r["accept"] for log in out["log"] for r in log)
    print(f"start {rot0} rad: {rejects} rejected steps")
    if rot0 == 0.8:
        assert rejects >= 1
    # the damping follows the decisions: / 10 per accept (floored), * 10 per reject
    for t in range(T):
        lam = lm_ref.PARAMS["lambda0"]
        for r in out["log"][t]:
            assert r["lam"] == lam
            lam = max(lam / 10.0, lm_ref.PARAMS["lambda_min"]) if r["accept"] else lam * 10.0
        assert out["lambda"][t] == lam
