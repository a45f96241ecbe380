"""The timed smoother's reference (tests/timed_ref.py) against the references it extends, and
the case for real timestamps on the oracle alone (no GPU):

  * constant dt and full masks: timed_ref.factors is lm_ref.factors, bit for bit;
  * a mask that clears the leading frames is `nvalid`;
  * a 40-tick stream with +-30 % period jitter, one 3-period gap, a camera absent every 7th tick
    and single corners missing tracks the truth to 1e-4 rad / 1e-5 m with per-pair dt and masks,
    and misses 1e-3 rad with the scalar nominal dt: the case is sensitive to what it tests;
  * Levenberg-Marquardt on a window with five different periods and a frame without keypoints.
"""
import numpy as np
import pytest

import lm_ref
import timed_ref as TR


def test_constant_dt_and_full_masks_are_the_untimed_factors():
    L = 5
    pr = lm_ref.problem(2, L, 0.05)
    for t in range(2):
        s = slice(t * L, (t + 1) * L)
        a = lm_ref.factors(pr["y"][s], pr["pose"][s], pr["vel"][s] + 0.01, pr["angvel"][s] + 0.2, L)
        b = TR.factors(pr["y"][s], pr["pose"][s], pr["vel"][s] + 0.01, pr["angvel"][s] + 0.2, L,
                       dt_pair=np.full(L - 1, lm_ref.DT), kp_mask=np.full(L, 0xFF))
        assert a.keys() == b.keys()
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("nvalid", [0, 1, 3, 5])
def test_mask_on_leading_frames_is_nvalid(nvalid):
    L = 5
    pr = lm_ref.problem(1, L, 0.05)
    a = lm_ref.factors(pr["y"], pr["pose"], pr["vel"], pr["angvel"], L, nvalid=nvalid)
    mask = np.where(np.arange(L) < L - nvalid, 0, 0xFFFFFFFF)
    b = TR.factors(pr["y"], pr["pose"], pr["vel"], pr["angvel"], L, kp_mask=mask)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # and on top of nvalid: OR of "off"
    c = TR.factors(pr["y"], pr["pose"], pr["vel"], pr["angvel"], L, kp_mask=np.full(L, 0b01010101), nvalid=nvalid)
    off = TR.mask_off(np.full(L, 0b01010101), L, 8) | np.repeat(np.arange(L) < L - nvalid, 8)
    np.testing.assert_array_equal(c["status"] == 2, off)
    np.testing.assert_array_equal(c["r_proj"][off], 0.0)
    np.testing.assert_array_equal(c["j_proj"][~off], a["j_proj"][~off])


def test_masked_factor_behind_the_camera_has_status_2():
    L = 3
    pr = lm_ref.problem(1, L, 0.0)
    pose = pr["pose"].copy()
    pose[1, 11] = -0.4  # frame 1 behind the camera
    a = TR.factors(pr["y"], pose, pr["vel"], pr["angvel"], L)
    assert (a["status"][8:16] == 1).all()
    b = TR.factors(pr["y"], pose, pr["vel"], pr["angvel"], L, kp_mask=[0xFF, 0b11110000, 0xFF])
    np.testing.assert_array_equal(b["status"][8:16], [2, 2, 2, 2, 1, 1, 1, 1])
    np.testing.assert_array_equal(b["r_proj"][8:12], 0.0)
    np.testing.assert_array_equal(b["j_proj"][8:12], 0.0)


def test_window_advance_moves_both_rings():
    T, L, nk = 2, 4, 8
    rng = np.random.default_rng(0)
    pr = lm_ref.problem(T, L, 0.05)
    win = dict(y=pr["y"].reshape(T, L, -1), pose=pr["pose"].reshape(T, L, 12), vel=rng.standard_normal((T, L, 3)) * 0.01,
               angvel=rng.standard_normal((T, L, 3)) * 0.3, dt=rng.uniform(0.01, 0.1, (T, L - 1)),
               mask=rng.integers(0, 256, (T, L)))
    y_new = rng.uniform(-0.5, 0.5, (T, 2 * nk)).astype(np.float32)
    dt_new, mask_new = np.array([0.02, 0.09]), np.array([5, 250])
    out = TR.window_advance_t(win, y_new, dt_new, mask_new)
    np.testing.assert_array_equal(out["dt"], np.concatenate([win["dt"][:, 1:], dt_new[:, None]], 1))
    np.testing.assert_array_equal(out["mask"], np.concatenate([win["mask"][:, 1:], mask_new[:, None]], 1))
    from oracle import factors_ref as F

    core = {k: win[k] for k in ("y", "pose", "angvel", "vel")}
    for t in range(T):  # the prediction uses that trajectory's dt_new
        ref = F.window_advance({k: v[t:t + 1] for k, v in core.items()}, y_new[t:t + 1], dt_new[t])
        for k in core:
            np.testing.assert_array_equal(out[k][t], ref[k][0], err_msg=k)
    # either ring alone
    w2 = {k: v for k, v in win.items() if k != "mask"}
    assert "mask" not in TR.window_advance_t(w2, y_new, dt_new, None)


@pytest.fixture(scope="module")
def case():
    return TR.stream_case()


def test_stream_case_is_what_it_says(case):
    dts, present, mask = case["dt_new"], case["present"], case["mask"]
    r = dts / TR.DT
    assert r.min() >= 0.7 and r[np.arange(len(r)) != 17].max() <= 1.3 and (r[17] == 3.0).all()
    assert (~present).sum() == 5 and (~present[-10:]).sum() == 1 and (mask[~present] == 0).all()
    single = [bin(int(m)).count("1") for m in mask[present]]
    assert single.count(7) >= 5  # single corners missing
    np.testing.assert_allclose(np.diff(case["stamps"], axis=0), dts[1:], rtol=0, atol=1e-12)


def test_timed_chain_tracks_and_the_scalar_dt_does_not(case):
    er, et, info, _ = TR.chain(case, timed=True)
    print("timed   rot", " ".join(f"{e:.1e}" for e in er))
    print("timed   tra", " ".join(f"{e:.1e}" for e in et))
    assert (info == 0).all()  # every tick solves
    assert er[-10:].max() < TR.ROT_TOL and et[-10:].max() < TR.TRA_TOL, (er[-10:].max(), et[-10:].max())
    er0, et0, _, _ = TR.chain(case, timed=False)
    print("untimed rot", " ".join(f"{e:.1e}" for e in er0))
    assert er0[-10:].max() > 1e-3, er0[-10:].max()  # the case is sensitive to dt


@pytest.fixture(scope="module")
def lm_case():
    T, L = 3, 6
    pr = TR.lm_problem(T, L, 0.1)
    dtp, msk = np.tile(TR.LM_DT_PAIR, (T, 1)), np.tile(TR.LM_MASKS, (T, 1))
    ref = TR.solve(pr["y"], pr["pose"], pr["vel"], pr["angvel"], T, L, dt_pair=dtp, kp_mask=msk)
    return pr, dtp, msk, ref


def test_lm_with_per_pair_dt_and_masks(lm_case):
    T, L = 3, 6
    pr, dtp, msk, ref = lm_case
    assert (ref["status"] == lm_ref.CONVERGED).all(), ref["status"]
    rot, tra = lm_ref.pose_errors(ref["pose"], pr["truth"])
    rot, tra = rot.reshape(T, L), tra.reshape(T, L)
    m = list(TR.LM_MEASURED)  # frame 3 has no keypoints: its rotation is not observable, not asserted
    print("rot", rot.max(0), "tra", tra.max(0))
    assert rot[:, m].max() < TR.ROT_TOL and tra[:, m].max() < TR.TRA_TOL, (rot[:, m].max(), tra[:, m].max())
    # the same solve with the mean scalar dt: the cost stays at least 1e3 x higher
    sc = TR.solve(pr["y"], pr["pose"], pr["vel"], pr["angvel"], T, L, dt=float(TR.LM_DT_PAIR.mean()), kp_mask=msk)
    print("cost timed", ref["cost"], "scalar", sc["cost"])
    assert (sc["cost"] >= 1e3 * ref["cost"]).all(), (sc["cost"], ref["cost"])
