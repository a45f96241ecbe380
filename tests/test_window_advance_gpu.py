"""pa_window_advance and pa_window_retract on their own (they otherwise run only inside streaming
ticks at T = 3, K = 8, world frame), against oracle/factors_ref.window_advance / window_retract:
the L = 2 carry-over, the body frame, windows that take several rounds of the shift loop
((L - 1)(2K + 18) > 1024 elements with 256 threads x 4), and a retract over two 64-frame blocks
with an unsolved trajectory and deltas on both sides of Expmap's th^2 <= eps."""
import numpy as np
import pytest
import torch

from oracle import factors_ref as F
from perseus_amd import pipeline

pytestmark = pytest.mark.gpu
DT = 1.0 / 12.0
# (T, L, K, frame): elements to shift per trajectory = (L - 1)(2K + 18)
CASES = [(1, 2, 1, "world"),    # 20: the L = 2 carry-over (frame 1's angular velocity is carried)
         (3, 3, 8, "body"),     # 68
         (2, 24, 16, "world"),  # 1150: two rounds
         (2, 64, 32, "body")]   # 5166: six rounds, 64 keypoint floats


def _window(T, L, K, seed):
    rng = np.random.default_rng(seed)
    pose = np.zeros((T, L, 12))
    for t in range(T):
        for l in range(L):
            pose[t, l] = F.pack(F.pose_exp(np.concatenate([0.5 * rng.standard_normal(3), rng.standard_normal(3)])))
    return {"y": rng.uniform(-1, 1, (T, L, 2 * K)).astype(np.float32), "pose": pose,
            "vel": rng.standard_normal((T, L, 3)), "angvel": rng.standard_normal((T, L, 3))}


def _to_dev(win):
    return {k: torch.as_tensor(np.ascontiguousarray(v), device="cuda") for k, v in win.items()}


def _to_host(dwin):
    return {k: v.cpu().numpy() for k, v in dwin.items()}


@pytest.mark.parametrize("T,L,K,vf", CASES)
def test_window_advance_alone(T, L, K, vf):
    assert ((L - 1) * (2 * K + 18) > 1024) == (L >= 24)
    rng = np.random.default_rng(L)
    win = _window(T, L, K, seed=10 * L + K)
    dwin = _to_dev(win)
    nvalid = torch.full((T,), L - 1, dtype=torch.int32, device="cuda")
    for step in range(2):
        y_new = rng.uniform(-1, 1, (T, 2 * K)).astype(np.float32)
        ref = F.window_advance(win, y_new, DT, vf)
        pipeline.window_advance(torch.as_tensor(y_new, device="cuda"), dwin, dt=DT, vel_frame=vf, nvalid=nvalid)
        got = _to_host(dwin)
        assert nvalid.cpu().tolist() == [L] * T, step  # L - 1 -> L -> L
        # moved, not recomputed: every keypoint and every shifted / carried state element is exact
        np.testing.assert_array_equal(got["y"], ref["y"])
        np.testing.assert_array_equal(got["pose"][:, :-1], ref["pose"][:, :-1])
        np.testing.assert_array_equal(got["vel"], ref["vel"])
        np.testing.assert_array_equal(got["angvel"], ref["angvel"])
        np.testing.assert_array_equal(got["pose"][:, :-1], win["pose"][:, 1:])
        np.testing.assert_array_equal(got["angvel"][:, -1], win["angvel"][:, L - 2 if L >= 3 else L - 1])
        # the predicted pose: pose[L-2] Exp(dt [w; v_b]) (the retract test's bound)
        np.testing.assert_allclose(got["pose"][:, -1], ref["pose"][:, -1], rtol=0, atol=1e-12)
        assert np.abs(got["pose"][:, -1] - got["pose"][:, -2]).max() > 1e-3
        win = got  # the second advance starts from the device's own window


def test_window_retract_two_blocks():
    T, L = 5, 13  # 65 frames: a full 64-thread block and a tail of 1
    win = _window(T, L, 1, seed=65)
    del win["y"]
    rng = np.random.default_rng(66)
    delta = 0.05 * rng.standard_normal((T * L, 12))
    delta[7] = 0.0
    eps = np.finfo(np.float64).eps
    for f, s in ((20, 0.9), (21, 1.1), (64, 0.9)):  # |d omega|^2 on both sides of eps; the tail block's frame too
        n = rng.standard_normal(3)
        delta[f, :3] = n / np.linalg.norm(n) * np.sqrt(s * eps)
        assert (delta[f, :3] @ delta[f, :3] <= eps) == (s < 1)
    info = np.array([0, 0, 3, 0, 0], dtype=np.int32)
    dwin = _to_dev(win)
    newest = torch.full((T, 12), float("nan"), dtype=torch.float64, device="cuda")
    pipeline.window_retract(dwin, torch.as_tensor(delta, device="cuda"), torch.as_tensor(info, device="cuda"),
                            newest=newest)
    ref = F.window_retract(win, delta, info)
    got = _to_host(dwin)
    for k in ("pose", "vel", "angvel"):
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=1e-12, err_msg=k)
        np.testing.assert_array_equal(got[k][2], win[k][2], err_msg=k)  # info != 0: untouched
        assert np.abs(got[k][0] - win[k][0]).max() > 1e-3
    np.testing.assert_array_equal(got["pose"].reshape(T * L, 12)[7], win["pose"].reshape(T * L, 12)[7])  # zero delta
    np.testing.assert_array_equal(newest.cpu().numpy(), got["pose"][:, -1])
