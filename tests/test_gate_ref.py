"""The numpy reference of pa_window_predict / pa_keypoint_gate (tests/gate_ref.py) checked on its
own, without a GPU: the first-order map F against central differences of the prediction map, the
predicted pose against the advance's new frame, Sigma* positive semi-definite, and the occlusion
scenario's margins on the reference chain (the device tests then compare against that chain)."""
import numpy as np
import pytest

import gate_ref as GR
import marginals_ref as MR
import timed_ref as TR
from oracle import factors_ref as F


def _local(Ta, Tb):
    return F.pose_log(F.between(Ta, Tb))


def _map(T1, w, v, tau, vel_frame, d):
    """The prediction map in local coordinates: the state perturbed by d (12), the predicted state's
    offset from the unperturbed prediction (12)."""
    Tp = F.compose(T1, F.pose_exp(d[:6]))
    base = GR.predict_pose(T1, w, v, tau, vel_frame)
    out = GR.predict_pose(Tp, w + d[6:9], v + d[9:12], tau, vel_frame)
    return np.concatenate([_local(base, out), d[6:9], d[9:12]])


def _axis(rng):
    a = rng.standard_normal(3)
    return a / np.linalg.norm(a)


# kind -> (angular velocity, scale of the linear velocity in m/s)
CASES = {"generic": (lambda rng: 0.7 * rng.standard_normal(3), 0.3), "zero": (lambda rng: np.zeros(3), 1e-3),
         "rest": (lambda rng: np.zeros(3), 0.0), "near_pi": (lambda rng: (np.pi - 1e-3) / 0.05 * _axis(rng), 0.3)}


@pytest.mark.parametrize("vel_frame", ["world", "body"])
@pytest.mark.parametrize("kind", list(CASES))
def test_F_matches_central_differences(vel_frame, kind):
    """Step 1e-6, agreement 1e-7.  At w = 0 the differences step to |tau w| = 5e-8, where
    Pose3::Expmap's translation (wxv - R wxv + w (w.v)) / theta^2 cancels to a few eps * tau |v| / h
    of f64 rounding, so the difference QUOTIENT carries about 3 eps tau |v| / h^2 there: 1e-5 at
    |v| = 0.3 m/s (measured 1.3e-5), 3e-7 at 0.01 m/s (measured), against F's own exactness at w = 0.
    That is the quotient's noise, not an error of F, so w = 0 is checked with a slow cube (1e-3 m/s:
    3e-8) and with the cube at rest (v = 0, the pipeline's initial state: no cancellation at all);
    the generic and near-pi cases move at 0.3 m/s."""
    rng = np.random.default_rng(3)
    tau = 0.05
    R0, _ = F.pose_exp(np.concatenate([0.8 * rng.standard_normal(3), np.zeros(3)]))
    T1 = (R0, np.array([0.02, -0.01, 0.4]))
    w, v = CASES[kind][0](rng), CASES[kind][1] * rng.standard_normal(3)
    if kind == "near_pi":
        assert abs(np.linalg.norm(tau * w) - np.pi) < 2e-3
    Fm = GR.predict_F(T1, w, v, tau, vel_frame)
    h = 1e-6
    num = np.zeros((12, 12))
    for j in range(12):
        d = np.zeros(12)
        d[j] = h
        num[:, j] = (_map(T1, w, v, tau, vel_frame, d) - _map(T1, w, v, tau, vel_frame, -d)) / (2 * h)
    assert np.abs(Fm - num).max() < 1e-7, np.abs(Fm - num).max()
    np.testing.assert_array_equal(Fm[6:], np.eye(12)[6:])


def _head(case, ticks):
    return {k: (v[:ticks] if k in ("stamps", "dt_new", "present", "mask", "truth", "y") else v) for k, v in case.items()}


@pytest.fixture(scope="module")
def stream():
    return TR.stream_case()


def test_predicted_pose_is_the_advances_new_frame(stream):
    case = _head(stream, 9)
    g = GR.gated_chain(case, gate_on=False)
    win = g["win"]
    n = win["pose"].shape[0]
    dt_new = np.array([0.031, 0.07, 0.0123])
    adv = TR.window_advance_t(win, case["y"][0], dt_new, np.full(n, 0xFF))
    pose, cov = GR.predict(win, dt_new.reshape(n, 1))
    assert cov is None
    np.testing.assert_array_equal(pose[:, 0], adv["pose"][:, -1])
    np.testing.assert_array_equal(GR.predict(win, np.zeros((n, 1)))[0][:, 0], win["pose"][:, -1])
    for vf in ("world", "body"):  # L = 2 takes frame 1's angular velocity, as the advance does
        w2 = {k: v[:, -2:].copy() for k, v in win.items()}
        w2["angvel"][:, 1] += 0.1
        a2 = TR.window_advance_t(w2, case["y"][0], dt_new, np.full(n, 0xFF), vel_frame=vf)
        np.testing.assert_array_equal(GR.predict(w2, dt_new.reshape(n, 1), vel_frame=vf)[0][:, 0], a2["pose"][:, -1])


def test_sigma_star_is_symmetric_positive_semidefinite(stream):
    case = stream
    n, L, nk = 3, 6, 8
    win = TR.init_window(n, L, nk, TR.init_pose(case["truth"][0]))
    nvalid = np.zeros(n, int)
    for k in range(9):
        win, nvalid, _, f = TR.tick(win, nvalid, case["y"][k], case["dt_new"][k], case["mask"][k])
    cov, cross = MR.dense(f, n, L, nk, TR.TICK_LAM)
    for t in range(n):
        S = GR.sigma_star(cov[t], cross[t])
        np.testing.assert_array_equal(S, S.T)
        ev = np.linalg.eigvalsh(S)
        assert ev.min() > -1e-12 * ev.max(), ev
        # the predicted covariance too, and it carries the process noise on its diagonal
        q = GR.process_noise(TR.TICK_SIG)
        _, C = GR.predict(win, np.full((n, 1), TR.DT), cov, cross, q_diag=q)
        _, C0 = GR.predict(win, np.full((n, 1), TR.DT), cov, cross)
        np.testing.assert_array_equal(C[t, 0], C[t, 0].T)
        np.testing.assert_allclose(np.diag(C[t, 0]) - np.diag(C0[t, 0]), q, rtol=1e-9, atol=1e-15)
        assert np.linalg.eigvalsh(C0[t, 0]).min() > -1e-12 * np.linalg.eigvalsh(C0[t, 0]).max()
    # tau = 0: F = I
    _, Cz = GR.predict(win, np.zeros((n, 1)), cov, cross)
    for t in range(n):
        np.testing.assert_allclose(Cz[t, 0], GR.sigma_star(cov[t], cross[t]), rtol=0, atol=1e-15 * np.abs(Cz[t, 0]).max())


def test_gate_abstains_in_order(stream):
    """YOUNG before NOCOV before FEW; an abstaining gate leaves the word as it came."""
    case = stream
    n = 3
    pose = np.array([F.pack(T) for T in case["truth"][1]])
    P = np.tile(1e-6 * np.eye(12), (n, 1, 1))
    y = case["y"][1].copy()
    y[:, :10] += 0.5  # five corners 64 px off
    kw = dict(chi2=GR.CHI2_999, min_pass=4, min_frames=3)
    m, d2, _, gi = GR.gate(y, pose, P, np.full(n, 0xFF), nvalid=np.array([3, 2, 3]), **kw)
    np.testing.assert_array_equal(gi, [GR.FEW, GR.YOUNG, GR.FEW])
    np.testing.assert_array_equal(m, 0xFF)
    assert np.isfinite(d2[0]).all() and np.isnan(d2[1]).all()
    Pn = P.copy()
    Pn[0, 2, 3] = np.nan
    Pn[1, 7, 7] = np.nan  # outside the pose block: ignored
    m, d2, _, gi = GR.gate(case["y"][1], pose, Pn, np.array([0xFF, 0x1FF, 0]), nvalid=np.array([3, 3, 3]), **kw)
    np.testing.assert_array_equal(gi, [GR.NOCOV, GR.APPLIED, GR.APPLIED])
    np.testing.assert_array_equal(m, [0xFF, 0x1FF, 0])


@pytest.fixture(scope="module")
def occlusion():
    case = GR.occlusion_case()
    return case, GR.gated_chain(case), GR.gated_chain(case, gate_on=False)


def test_occlusion_scenario_margins(occlusion):
    """The scenario the device tests replay (gate_ref.OCC): on the reference chain alone, from the
    first corrupted tick on, every displaced corner is at least a factor 2 above chi2 and every other
    measured corner a factor 2 below, the gate applies on every tick, the gated chain tracks the
    truth and the ungated one is driven away."""
    case, g, u = occlusion
    first, chi2 = GR.OCC["first_tick"], GR.OCC["chi2"]
    bad = case["bad"]
    ticks, n = bad.shape
    assert (bad[:first] < 0).all() and (bad[first:] >= 0).sum() >= 20
    assert (bad[first] >= 0).any()  # the first corrupted tick is first_tick itself
    hit = np.zeros(g["d2"].shape, bool)
    for k, c in zip(*np.nonzero(bad >= 0)):
        assert case["present"][k, c] and case["present"][k - 1, c] and case["dt_new"][k, c] <= 2 * TR.DT
        hit[k, c, bad[k, c]] = True
    d2 = g["d2"]
    assert np.isfinite(d2[hit]).all()
    print("corrupted d2 min", d2[hit].min(), "clean d2 max", np.nanmax(d2[first:][~hit[first:]]))
    assert d2[hit].min() >= 2 * chi2
    assert np.nanmax(d2[first:][~hit[first:]]) <= chi2 / 2
    assert (g["ginfo"][first:] == GR.APPLIED).all() and (g["info"] == 0).all()
    want = case["mask"].copy()
    for k, c in zip(*np.nonzero(bad >= 0)):
        want[k, c] &= ~(1 << bad[k, c])
    np.testing.assert_array_equal(g["mask"][first:], want[first:])
    print("gated", g["er"][-10:].max(), g["et"][-10:].max(), "ungated", u["er"][-10:].max(), u["et"][-10:].max())
    assert g["er"][-10:].max() < TR.ROT_TOL and g["et"][-10:].max() < TR.TRA_TOL
    assert u["er"][-10:].max() > 100 * TR.ROT_TOL and u["et"][-10:].max() > 100 * TR.TRA_TOL
    assert (bad[-10:] >= 0).any()  # corrupted frames among the ticks judged
