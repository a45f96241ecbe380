"""The factor kernels against the 60-digit truth at every branch point of the GTSAM closed
forms (tests/golden/factors_truth.npz: cases, truth, the f64 oracle's output and the per-class
tolerances; oracle/gen_factors_truth.py documents the layout).  Away from pi the kernels are
pinned to the truth; in the trace ~ -1 branch of Rot3::Logmap, a first-order formula that is
off by O((pi - theta)^2) by design, to the oracle's output."""
import os

import numpy as np
import pytest
import torch

from perseus_amd import pipeline, smoother

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "factors_truth.npz")
DT = 1.0 / 12.0
OUTS = (("r", 0, 6),("J0", 6, 36), ("J1", 42, 18), ("J2", 60, 18), ("J3", 78, 36))  # name, offset, size
NEAR_PI_R, NEAR_PI_J = 1e-8, 1e-6  # test_factors_gpu.test_branches_small_and_near_pi's bounds vs the oracle


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def _flat(r, J):
    """(n, 114) in the golden's layout from r (n, 6) and four (n, 6, cols) Jacobians."""
    return np.concatenate([r.cpu().numpy()] + [j.cpu().numpy().reshape(len(r), -1) for j in J], axis=1)


def _check_dynamics(g, got, vf, what):
    """got (n, 114) for all cases; the frame's stored cases against truth (tol) or oracle (near pi)."""
    idx = np.arange(len(g["dyn/cls"])) if vf == "world" else g["dyn/body/idx"]
    ref, cls, tol, gap = g[f"dyn/{vf}/out"], g["dyn/cls"], g["dyn/tol"], g["dyn/gap"]
    worst_pi, worst_rel, bad = {}, 0.0, []
    for row, i in enumerate(idx):
        c = cls[i]
        for k, (name, off, size) in enumerate(OUTS):
            sl = slice(off, off + size)
            if np.isnan(gap[c]):
                err = np.abs(got[i, sl] - ref[row, sl, 0]).max()
                bound = tol[c, k]
                worst_rel = max(worst_rel, err / bound)
            else:
                err = np.abs(got[i, sl] - ref[row, sl, 1]).max()
                bound = NEAR_PI_R if name == "r" else NEAR_PI_J
                key = (float(gap[c]), "r" if name == "r" else "J")
                worst_pi[key] = max(worst_pi.get(key, 0.0), err)
            if not err <= bound:
                bad.append((str(g["dyn/class_names"][c]), int(i), name, float(err), float(bound)))
    print(f"{what} {vf}: worst |gpu - truth| / tol away from pi {worst_rel:.3f}; near pi |gpu - oracle| "
          + ", ".join(f"g={k[0]:g} {k[1]} {v:.1e}" for k, v in sorted(worst_pi.items())))
    assert not bad, bad


@pytest.mark.parametrize("vf", ["world", "body"])
def test_dyn_kernel_vs_truth(g, vf):
    out = smoother.linearize_dynamics(g["dyn/T1"], g["dyn/w"], g["dyn/v"], g["dyn/T2"], DT, vf)
    _check_dynamics(g, _flat(out["r"], [out[f"J{k}"] for k in range(4)]), vf, "dyn_kernel")


@pytest.mark.parametrize("vf", ["world", "body"])
def test_traj_all_kernel_vs_truth(g, vf):
    """The same cases as trajectories of two frames: pose[2i] = T1, pose[2i + 1] = T2."""
    n = len(g["dyn/cls"])
    poses = np.stack([g["dyn/T1"], g["dyn/T2"]], axis=1).reshape(2 * n, 12)
    vels, angvels = np.zeros((2 * n, 3)), np.zeros((2 * n, 3))
    vels[0::2], angvels[0::2] = g["dyn/v"], g["dyn/w"]
    y = torch.zeros((2 * n, 2), dtype=torch.float32, device="cuda")
    out = pipeline.linearize_trajectories(y, poses, vels, angvels, np.zeros((1, 3)),
                                          np.array([280.0, 280.0, 0.0, 128.0, 128.0]), T=n, L=2, dt=DT, vel_frame=vf)
    _check_dynamics(g, _flat(out["r_dyn"], [out[f"j_dyn{k}"] for k in range(4)]), vf, "traj_all_kernel")


@pytest.mark.parametrize("vf", ["world", "body"])
def test_dyn_kernel_error_only_is_bit_identical(g, vf):
    isig = np.array([10.0, 20.0, 5.0, 3.0, 7.0, 0.5])
    full = smoother.linearize_dynamics(g["dyn/T1"], g["dyn/w"], g["dyn/v"], g["dyn/T2"], DT, vf, inv_sigma=isig)
    eo = smoother.linearize_dynamics(g["dyn/T1"], g["dyn/w"], g["dyn/v"], g["dyn/T2"], DT, vf, inv_sigma=isig,
                                     jacobians=False)
    assert "J0" not in eo
    for k in ("r", "err"):
        assert torch.equal(full[k].view(torch.int64), eo[k].view(torch.int64)), k
    torch.testing.assert_close(full["err"], 0.5 * (full["r"] ** 2).sum(1), rtol=1e-14, atol=0)


@pytest.mark.parametrize("group", range(6))
def test_proj_kernel_vs_truth(g, group):
    """One launch per (K shared / per factor) x (camera pose none / shared / per factor), its
    cases repeated to n = 130: two full waves and a tail."""
    kmode, cmode = divmod(group, 3)
    idx = np.resize(np.nonzero(g["proj/group"] == group)[0], 130)
    K = g["proj/K"][idx] if kmode else g["proj/K"][idx[0]]
    Tc = [None, g["proj/Tc"][idx[0]], g["proj/Tc"][idx]][cmode]
    assert kmode or (g["proj/K"][idx] == K).all()
    assert cmode != 1 or (g["proj/Tc"][idx] == Tc).all()
    assert np.isnan(g["proj/Tc"][idx]).all() == (cmode == 0)
    out = smoother.linearize_projection(g["proj/T"][idx], g["proj/pb"][idx], g["proj/z"][idx], K, Tc)
    st = out["status"].cpu().numpy()
    np.testing.assert_array_equal(st, g["proj/status"][idx])
    r, J = out["r"].cpu().numpy(), out["J"].cpu().numpy().reshape(130, 12)
    assert (st == 1).any() and np.isnan(r[st == 1]).all() and np.isnan(J[st == 1]).all()
    ref, cls, tol = g["proj/out"][idx, :, 0], g["proj/cls"][idx], g["proj/tol"]
    worst = 0.0
    for c in (0, 1):
        m = cls == c
        assert m.any() and (st[m] == 0).all()
        er, ej = np.abs(r[m] - ref[m, :2]).max(), np.abs(J[m] - ref[m, 2:]).max()
        worst = max(worst, er / tol[c, 0], ej / tol[c, 1])
        assert er <= tol[c, 0] and ej <= tol[c, 1], (c, er, ej, tol[c])
    print(f"proj_kernel group {group}: worst |gpu - truth| / tol {worst:.3f}")
