"""pa_window_predict and pa_keypoint_gate on the device against tests/gate_ref.py.

Predict: every branch of Pose3::Expmap (w exactly 0, |tau w| ~ 1e-9, generic, |tau w| near pi), both
velocity frames, tau in {0, dt, 2.5 dt, -dt}; the tau = dt pose against the device's own
pa_window_advance_t, the tau = 0 pose against the input; covariances at test_marginals_gpu.py's
scaled bound; NaN for a failed marginal; the pose-only form at L = 2; a launch of several blocks.
Gate: the seven cases of the header's table, n_kp = 1 and 32, and the strided in-place form.
"""
import numpy as np
import pytest
import torch

import gate_ref as GR
from oracle import factors_ref as F
from perseus_amd import _lib, pipeline, synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = 1.0 / 30.0
ATOL, RTOL = 1e-9, 1e-12  # the factor tests' bounds
COV_RTOL = 1e-9           # test_marginals_gpu.RTOL, on marginals_ref.scaled_err's scale


def _axis(rng):
    a = rng.standard_normal(3)
    return a / np.linalg.norm(a)


def _window(T, L, seed, branches=True):
    rng = np.random.default_rng(seed)
    pose = np.zeros((T, L, 12))
    for t in range(T):
        for l in range(L):
            R0, _ = F.pose_exp(np.concatenate([0.8 * rng.standard_normal(3), np.zeros(3)]))
            pose[t, l] = F.pack((R0, np.array([0.0, 0.0, 0.4]) + 0.05 * rng.standard_normal(3)))
    win = dict(pose=pose, angvel=0.3 * rng.standard_normal((T, L, 3)), vel=0.1 * rng.standard_normal((T, L, 3)))
    if branches:  # the frame a prediction takes the angular velocity from
        fw = L - 2 if L >= 3 else L - 1
        win["angvel"][0, fw] = 0.0
        win["angvel"][1, fw] = 1e-9 / DT * _axis(rng)
        if T > 3:
            win["angvel"][3, fw] = (np.pi - 1e-3) / DT * _axis(rng)
    return win


def _marginals(T, L, seed):
    """cov (T, L, 12, 12) and cross (T, L-1, 12, 12) cut from a random SPD matrix per trajectory
    (exactly symmetric, as the marginals kernel writes its blocks)."""
    rng = np.random.default_rng(seed)
    cov, cross = np.zeros((T, L, 12, 12)), np.zeros((T, L - 1, 12, 12))
    for t in range(T):
        A = rng.standard_normal((12 * L, 12 * L + 5)) * np.exp(rng.uniform(-4, 0, (12 * L, 1)))
        S = A @ A.T
        S = 0.5 * (S + S.T)
        for l in range(L):
            cov[t, l] = S[12 * l:12 * l + 12, 12 * l:12 * l + 12]
            if l + 1 < L:
                cross[t, l] = S[12 * l:12 * l + 12, 12 * l + 12:12 * l + 24]
    return cov, cross


def _dev(win):
    return {k: torch.as_tensor(v, device=DEV) for k, v in win.items()}


def _scaled(got, ref):
    sd = np.sqrt(np.einsum("...ii->...i", ref))
    return float((np.abs(got - ref) / (sd[..., :, None] * sd[..., None, :])).max())


TAUS = np.array([0.0, DT, 2.5 * DT, -DT])


@pytest.mark.parametrize("vel_frame", ["world", "body"])
def test_predict_matches_the_reference(vel_frame):
    T, L = 4, 4
    win = _window(T, L, 1)
    cov, cross = _marginals(T, L, 2)
    q = np.random.default_rng(3).uniform(1e-6, 1e-2, 12)
    taus = np.tile(TAUS, (T, 1))
    fw = L - 2
    thw = np.linalg.norm(win["angvel"][:, fw], axis=1) * DT
    assert thw[0] == 0 and 0 < thw[1] ** 2 < F.EPS and thw[2] ** 2 > 1e-6 and abs(thw[3] - np.pi) < 2e-3
    info = torch.zeros(T, dtype=torch.int32, device=DEV)
    out = pipeline.predict(_dev(win), taus, cov=cov, cross=cross, cov_info=info, q_diag=q, vel_frame=vel_frame)
    rp, rc = GR.predict(win, taus, cov, cross, q_diag=q, vel_frame=vel_frame)
    pose, C = out["pose"].cpu().numpy(), out["cov"].cpu().numpy()
    np.testing.assert_allclose(pose, rp, atol=ATOL, rtol=RTOL)
    np.testing.assert_array_equal(pose[:, 0], win["pose"][:, -1])  # tau = 0: the input pose, bit for bit
    err = _scaled(C, rc)
    print("scaled covariance error", err)
    assert err <= COV_RTOL
    np.testing.assert_array_equal(C, C.transpose(0, 1, 3, 2))  # exactly symmetric
    # without q_diag the diagonal is smaller by exactly what was added (to rounding), the rest equal
    out0 = pipeline.predict(_dev(win), taus, cov=cov, cross=cross, vel_frame=vel_frame)
    C0 = out0["cov"].cpu().numpy()
    off = ~np.eye(12, dtype=bool)
    np.testing.assert_array_equal(C0[..., off], C[..., off])
    np.testing.assert_array_equal(out0["pose"].cpu().numpy(), pose)


@pytest.mark.parametrize("vel_frame", ["world", "body"])
@pytest.mark.parametrize("L", [2, 4])
def test_predict_at_dt_is_the_advances_frame(vel_frame, L):
    """tau = the dt of an advance: bit for bit the frame pa_window_advance_t predicts (per-trajectory
    dt_new, so four different horizons at once)."""
    T, nk = 4, 8
    win = _window(T, L, 4)
    dt_new = DT * np.array([1.0, 0.7, 2.2, 3.0])
    out = pipeline.predict(_dev(win), dt_new.reshape(T, 1), vel_frame=vel_frame)
    assert "cov" not in out
    w = _dev(win)
    w["y"] = torch.zeros((T, L, 2 * nk), dtype=torch.float32, device=DEV)
    w["dt"] = torch.full((T, L - 1), DT, dtype=torch.float64, device=DEV)
    pipeline.window_advance(torch.zeros((T, 2 * nk), dtype=torch.float32, device=DEV), w, dt=123.0, vel_frame=vel_frame,
                            dt_new=torch.as_tensor(dt_new, device=DEV))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out["pose"].cpu().numpy()[:, 0], w["pose"].cpu().numpy()[:, -1])
    rp, _ = GR.predict(win, dt_new.reshape(T, 1), vel_frame=vel_frame)
    np.testing.assert_allclose(out["pose"].cpu().numpy(), rp, atol=ATOL, rtol=RTOL)


def test_predict_failed_marginals_give_nan():
    T, L = 3, 4
    win = _window(T, L, 5)
    cov, cross = _marginals(T, L, 6)
    info = torch.tensor([0, 2, 0], dtype=torch.int32, device=DEV)
    out = pipeline.predict(_dev(win), TAUS, cov=cov, cross=cross, cov_info=info)
    C, pose = out["cov"].cpu().numpy(), out["pose"].cpu().numpy()
    assert np.isnan(C[1]).all() and np.isfinite(C[[0, 2]]).all() and np.isfinite(pose).all()
    rp, rc = GR.predict(win, np.tile(TAUS, (T, 1)), cov, cross, cov_info=[0, 2, 0])
    np.testing.assert_allclose(pose, rp, atol=ATOL, rtol=RTOL)
    assert _scaled(C[[0, 2]], rc[[0, 2]]) <= COV_RTOL


def test_predict_many_blocks():
    """T * Q = 390: seven blocks of 64 lanes, the last one partly filled."""
    T, L, Q = 130, 3, 3
    win = _window(T, L, 7, branches=False)
    cov, cross = _marginals(T, L, 8)
    taus = DT * np.random.default_rng(9).uniform(-1.0, 3.0, (T, Q))
    out = pipeline.predict(_dev(win), taus, cov=cov, cross=cross)
    rp, rc = GR.predict(win, taus, cov, cross)
    np.testing.assert_allclose(out["pose"].cpu().numpy(), rp, atol=ATOL, rtol=RTOL)
    assert _scaled(out["cov"].cpu().numpy(), rc) <= COV_RTOL


# ---------------------------------------------------------------------------------- the gate
SIG_PX = (2.0, 1.5)
CHI2 = GR.CHI2_999


def _kp(pose12, corners, offsets=None):
    """Normalized f32 keypoints (2K,) of the corners at a pose, seen by the identity camera, plus
    pixel offsets (K, 2)."""
    px = np.array([F.projection(F.unpack(pose12), c, np.zeros(2), synth.CAMERA_K)[3] for c in corners])
    if offsets is not None:
        px = px + offsets
    return (np.nan_to_num(px) / 127.5 - 1.0).reshape(-1).astype(np.float32)


def _gate_inputs(T, corners, seed):
    rng = np.random.default_rng(seed)
    nk = len(corners)
    pose = np.zeros((T, 12))
    for t in range(T):
        R0, _ = F.pose_exp(np.concatenate([0.4 * rng.standard_normal(3), np.zeros(3)]))
        pose[t] = F.pack((R0, np.array([0.0, 0.0, 0.35]) + 0.01 * rng.standard_normal(3)))
    P = np.zeros((T, 12, 12))
    for t in range(T):
        A = rng.standard_normal((12, 14)) * np.array([2e-3] * 3 + [1e-3] * 3 + [0.1] * 6)[:, None]
        P[t] = 0.5 * (A @ A.T + (A @ A.T).T)
    off = rng.uniform(-0.7, 0.7, (T, nk, 2))  # sub-pixel detector noise: d2 well below chi2 / 2
    return pose, P, off


def _run_gate(y, pose, P, corners, mask, **kw):
    out = pipeline.gate_keypoints(torch.as_tensor(y, device=DEV), pose, P, corners, synth.CAMERA_K, SIG_PX, mask,
                                  chi2=CHI2, **kw)
    torch.cuda.synchronize()
    return (out["mask"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF, out["d2"].cpu().numpy(), out["zhat"].cpu().numpy(),
            out["ginfo"].cpu().numpy())


def _compare(got, ref, chi2=CHI2):
    (m, d2, zh, gi), (rm, rd2, rzh, rgi) = got, ref
    fin = np.isfinite(rd2)
    assert (np.minimum(rd2[fin] / chi2, chi2 / np.maximum(rd2[fin], 1e-300)) <= 0.5).all(), rd2  # a factor 2 from chi2
    np.testing.assert_array_equal(gi, rgi)
    np.testing.assert_array_equal(m, rm)
    np.testing.assert_array_equal(np.isnan(d2), np.isnan(rd2))
    np.testing.assert_allclose(d2[fin], rd2[fin], atol=ATOL, rtol=RTOL)
    np.testing.assert_array_equal(np.isnan(zh), np.isnan(rzh))
    np.testing.assert_allclose(zh[np.isfinite(rzh)], rzh[np.isfinite(rzh)], atol=ATOL, rtol=RTOL)


def test_gate_cases():
    T, nk = 7, 8
    corners = synth.CUBE_CORNERS
    pose, P, off = _gate_inputs(T, corners, 11)
    mask = np.full(T, 0xFF, np.int64)
    nvalid = np.full(T, 3, np.int32)
    # 0: all pass.  1: one corner 40 px off.  2: five corners off -> the gate abstains (FEW).
    off[1, 3] += [40.0, 0.0]
    off[2, :5] += [[40.0, 0], [0, -40.0], [30.0, 30.0], [-40.0, 0], [0, 40.0]]
    # 3: corner 0 behind the camera at the predicted pose (the cube's diagonal along the optical
    # axis, its centre a third of the half diagonal in front of the camera); the three corners next
    # to it are in front
    a = corners[0] / np.linalg.norm(corners[0])
    v = np.cross(a, [0, 0, -1.0])
    s, c = np.linalg.norm(v), -a[2]
    R3, _ = F.pose_exp(np.concatenate([v / s * np.arctan2(s, c), np.zeros(3)]))
    d = np.linalg.norm(corners[0])
    pose[3] = F.pack((R3, np.array([0.0, 0.0, 2.0 * d / 3.0])))
    z3 = (corners @ R3.T)[:, 2] + 2.0 * d / 3.0
    assert z3[0] < 0 and (z3[1:] > 0).all()
    # 4: an incoming mask with cleared bits (one of them on a corner that is 40 px off)
    mask[4] = 0b10110101
    off[4, 1] += [40.0, 0.0]
    # 5: a NaN in the pose block of the covariance.  6: a young window.
    P[5, 1, 4] = P[5, 4, 1] = np.nan
    nvalid[6] = 2
    y = np.stack([_kp(pose[t], corners, off[t]) for t in range(T)])
    ref = GR.gate(y, pose, P, mask, chi2=CHI2, nvalid=nvalid, proj_sigmas=SIG_PX)
    got = _run_gate(y, pose, P, corners, mask, nvalid=nvalid)
    _compare(got, ref)
    m, d2, zh, gi = got
    np.testing.assert_array_equal(gi, [0, 0, GR.FEW, 0, 0, GR.NOCOV, GR.YOUNG])
    np.testing.assert_array_equal(m, [0xFF, 0xFF & ~(1 << 3), 0xFF, 0xFE, 0b10110101, 0xFF, 0xFF])
    assert np.isfinite(d2[2]).all() and (d2[2, :5] > 2 * CHI2).all()
    assert np.isnan(d2[3, 0]) and np.isnan(zh[3, 0]).all() and np.isfinite(d2[3, 1:]).all()
    assert np.isnan(d2[4, [1, 3, 6]]).all() and np.isfinite(d2[4, [0, 2, 4, 5, 7]]).all()
    assert np.isnan(d2[5]).all() and np.isnan(d2[6]).all()
    # min_pass above what passes: the one bad corner of trajectory 1 now makes the gate abstain
    got8 = _run_gate(y, pose, P, corners, mask, nvalid=nvalid, min_pass=8)
    _compare(got8, GR.gate(y, pose, P, mask, chi2=CHI2, nvalid=nvalid, proj_sigmas=SIG_PX, min_pass=8))
    assert got8[3][1] == GR.FEW and got8[0][1] == 0xFF and got8[3][0] == 0
    # nvalid NULL: never young
    gotn = _run_gate(y, pose, P, corners, mask)
    assert gotn[3][6] == 0


@pytest.mark.parametrize("nk", [1, 32])
def test_gate_other_keypoint_counts(nk):
    T = 11  # (two workgroups of eight trajectories)
    rng = np.random.default_rng(12)
    corners = rng.uniform(-0.02, 0.02, (nk, 3))
    pose, P, off = _gate_inputs(T, corners, 13)
    mask = np.full(T, 0xFFFFFFFF, np.int64)
    off[2, 0] += [0.0, 50.0]
    if nk == 32:
        off[5, [7, 31]] += [45.0, -20.0]
        mask[7] = 0x7FFF00FF
        off[7, 30] += [45.0, 0.0]
        off[7, 9] += [45.0, 0.0]  # (masked on the way in: stays out)
    y = np.stack([_kp(pose[t], corners, off[t]) for t in range(T)])
    ref = GR.gate(y, pose, P, mask, chi2=CHI2, proj_sigmas=SIG_PX, corners=corners)
    got = _run_gate(y, pose, P, corners, mask)
    _compare(got, ref)
    low = (1 << nk) - 1
    if nk == 1:
        # the only corner fails: fewer than min(min_pass, 1) pass, the gate abstains
        assert got[3][2] == GR.FEW and got[0][2] == 0xFFFFFFFF
        assert (got[0] == 0xFFFFFFFF).all()  # bits at and above n_kp are copied through
    else:
        assert got[0][5] == 0xFFFFFFFF & ~((1 << 7) | (1 << 31)) and got[0][7] == 0x3FFF00FF and (got[3] == 0).all()


def test_gate_strided_in_place_matches_stride_one():
    """The split tick's form: the mask word is the ring entry kp_mask[t*L + L-1] (stride L) and the
    pose the window's frame L-1 (stride 12 L), gated in place; the neighbours stay untouched."""
    T, nk, L = 7, 8, 6
    corners = synth.CUBE_CORNERS
    pose, P, off = _gate_inputs(T, corners, 14)
    mask = np.array([0xFF, 0xFF, 0x7F, 0xFF, 0xF0FF, 0xFF, 0xFF], np.int64)
    for t, k in ((0, 2), (2, 5), (4, 0), (6, 7)):
        off[t, k] += [35.0, -35.0]
    y = np.stack([_kp(pose[t], corners, off[t]) for t in range(T)])
    want = _run_gate(y, pose, P, corners, mask)
    ring = torch.full((T, L), 0x55, dtype=torch.int32, device=DEV)
    ring[:, -1] = torch.as_tensor(mask.astype(np.int32), device=DEV)
    wpose = torch.full((T, L, 12), float("nan"), dtype=torch.float64, device=DEV)
    wpose[:, -1] = torch.as_tensor(pose, device=DEV)
    keep = [torch.as_tensor(a, device=DEV) for a in (y, P, corners, synth.CAMERA_K, 1.0 / np.array(SIG_PX))]
    plan = pipeline.GatePlan(keep[0], wpose.data_ptr() + (L - 1) * 12 * 8, keep[1], keep[2], keep[3], keep[4],
                             ring.data_ptr() + (L - 1) * 4, chi2=CHI2, pose_stride=12 * L, mask_stride=L)
    plan.launch()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ring[:, -1].cpu().numpy().astype(np.int64) & 0xFFFFFFFF, want[0])
    assert (ring[:, :-1] == 0x55).all()
    np.testing.assert_array_equal(plan.out["d2"].cpu().numpy(), want[1])
    np.testing.assert_array_equal(plan.out["ginfo"].cpu().numpy(), want[3])
    assert want[0][0] == 0xFF & ~(1 << 2) and want[0][4] == 0xF0FE
