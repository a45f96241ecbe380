"""The 60-digit factor reference (tests/factors_truth_ref.py) and its golden file
(tests/golden/factors_truth.npz, oracle/gen_factors_truth.py), on the CPU: the file regenerates
bit for bit, the finite-difference Jacobians agree with autodiff, the f64 oracle sits inside
the stored tolerances away from pi and inside the derived O((pi - theta)^2) bound next to it."""
import os

import numpy as np
import pytest

pytest.importorskip("mpmath")

import factors_truth_ref as R  # noqa: E402  (tests/ is on sys.path, rootdir conftest)

from oracle import factors_ref as F  # noqa: E402
from oracle import gen_factors_truth as G  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden", "factors_truth.npz")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_golden_regenerates_bit_for_bit(g):
    """A seeded subset of the cases (one per kind of class and projection group), rebuilt from
    the generator, and every derived array rebuilt from the stored ones."""
    specs, names, gaps = G.dyn_specs()
    assert list(g["dyn/class_names"]) == names and _same(g["dyn/gap"], gaps)
    assert _same(g["dyn/cls"], np.array([s[0] for s in specs], np.int32))
    assert _same(g["dyn/body/idx"], G.body_subset(specs))
    pick = [0, 13, len(specs) - 1]  # a = 0; (a, 1) at 1.4e-8; pi - 1e-6 on R11, negative sign
    assert specs[13][1:3] == (1.4e-8, 1.0) and specs[-1][3:] == (0, -1.0)
    for i in pick:
        inp = G.dyn_inputs(i, specs[i])
        for k, name in enumerate(("T1", "w", "v", "T2")):
            assert _same(inp[k], g[f"dyn/{name}"][i]), (i, name)
        assert _same(G.dyn_outputs(inp, "world"), g["dyn/world/out"][i]), i
    j = 4  # a body-frame case: (a, a) at 1.4e-8
    i = int(g["dyn/body/idx"][j])
    assert specs[i][1:3] == (1.4e-8, 1.4e-8)
    assert _same(G.dyn_outputs(G.dyn_inputs(i, specs[i]), "body"), g["dyn/body/out"][j])
    cls = g["dyn/cls"]
    tol = G.tolerances(np.concatenate([g["dyn/world/out"], g["dyn/body/out"]]),
                       np.concatenate([cls, cls[g["dyn/body/idx"]]]), len(names), ~np.isnan(gaps))
    assert _same(tol, g["dyn/tol"])

    ps = G.proj_specs()
    assert _same(g["proj/group"], np.array([s[0] for s in ps], np.int32))
    assert _same(g["proj/cls"], np.array([s[1] for s in ps], np.int32))
    for i in (1, 3, len(ps) - 1):  # pc.z = 1e-3 without a camera pose; exact 0; -1e-3, per-factor K and pose
        inp = G.proj_inputs(i, ps[i])
        for k, name in enumerate(("T", "pb", "z", "K", "Tc")):
            assert _same(inp[k], g[f"proj/{name}"][i]), (i, name)
        out, st = G.proj_outputs(inp)
        assert _same(out, g["proj/out"][i]) and st == g["proj/status"][i], i
    assert ps[3][2] is None and g["proj/status"][3] == 1
    ptol, pmag = G.proj_tolerances(g["proj/out"], g["proj/cls"])
    assert _same(ptol, g["proj/tol"]) and _same(pmag, g["proj/mag"])


@pytest.mark.parametrize("vf", ["world", "body"])
def test_finite_differences_match_autodiff_dynamics(vf):
    rng = np.random.default_rng(7)
    T1 = R.pose_exp12(rng.standard_normal(6))
    w, v = rng.standard_normal(3), rng.standard_normal(3)
    T2 = R.predict_then_offset(T1, w, v, G.DT, "world", np.concatenate([0.7 * rng.standard_normal(3),
                                                                        0.05 * rng.standard_normal(3)]))
    r, J = R.dynamics(T1, w, v, T2, G.DT, vf)
    ra, Ja = F.autodiff_dynamics(F.unpack(T1), w, v, F.unpack(T2), G.DT, vf)
    np.testing.assert_allclose(r, ra, rtol=0, atol=1e-9)
    for k in range(4):
        np.testing.assert_allclose(J[k], Ja[k], rtol=0, atol=1e-9, err_msg=f"J{k}")


def test_finite_differences_match_autodiff_projection():
    rng = np.random.default_rng(8)
    Tb = R.pose_exp12(np.concatenate([rng.standard_normal(3), [0.02, -0.03, 0.4]]))
    Tc = R.pose_exp12(np.array([0.02, -0.01, 0.03, 0.01, -0.02, -0.05]))
    pb, z = np.array([0.0175, -0.0175, 0.0175]), np.array([100.0, 120.0])
    r, J, st = R.projection(Tb, pb, z, G.KCAL, Tc)
    ra, Ja = F.autodiff_projection(F.unpack(Tb), pb, z, G.KCAL, F.unpack(Tc))
    assert st == 0
    np.testing.assert_allclose(r, ra, rtol=0, atol=1e-9)
    np.testing.assert_allclose(J, Ja, rtol=0, atol=1e-9)


def _oracle114(g, i, vf):
    return G.flat114(*F.dynamics(F.unpack(g["dyn/T1"][i]), g["dyn/w"][i], g["dyn/v"][i], F.unpack(g["dyn/T2"][i]),
                                 G.DT, vf))


def _frames(g):
    """(frame, case indices, truth (m, 114))."""
    return (("world", np.arange(len(g["dyn/cls"])), g["dyn/world/out"][..., 0]),
            ("body", g["dyn/body/idx"], g["dyn/body/out"][..., 0]))


def test_oracle_within_quarter_tol_away_from_pi(g):
    """The oracle as it is now (not its stored output) against the truth, per class and output;
    and the tolerances stay under the cap the cases were chosen for (1e-8; tol_caps for the one
    exception, projection relative to the output's magnitude)."""
    tol, cls, near_pi = g["dyn/tol"], g["dyn/cls"], ~np.isnan(g["dyn/gap"])
    assert np.isnan(tol[near_pi]).all() and not np.isnan(tol[~near_pi]).any()
    caps = G.tol_caps()
    assert (tol[~near_pi] <= caps[~near_pi]).all()
    assert (caps <= 1e-8).sum() == caps.size - 2 and caps.max() <= 2.9e-8
    for vf, idx, truth in _frames(g):
        for row, i in enumerate(idx):
            c = cls[i]
            if near_pi[c]:
                continue
            o = _oracle114(g, i, vf)
            for k, (name, off, rows, cols) in enumerate(G.OUTS):
                sl = slice(off, off + rows * cols)
                err = np.abs(o[sl] - truth[row, sl]).max()
                assert err <= tol[c, k] / 4, (vf, g["dyn/class_names"][c], name, err, tol[c, k])
    assert (g["proj/tol"] <= 1e-8 * g["proj/mag"]).all()
    for i in np.nonzero(g["proj/status"] == 0)[0]:
        Tc = g["proj/Tc"][i]
        r, J, st, _ = F.projection(F.unpack(g["proj/T"][i]), g["proj/pb"][i], g["proj/z"][i], g["proj/K"][i],
                                   None if np.isnan(Tc[0]) else F.unpack(Tc))
        c = g["proj/cls"][i]
        assert st == 0
        assert np.abs(r - g["proj/out"][i, :2, 0]).max() <= g["proj/tol"][c, 0] / 4
        assert np.abs(J.reshape(-1) - g["proj/out"][i, 2:, 0]).max() <= g["proj/tol"][c, 1] / 4


def test_oracle_near_pi_deviation_is_second_order(g):
    """GTSAM 4.2's trace ~ -1 branch of Rot3::Logmap returns 0.5 mag / sqrt(Q1) * vec.  With
    R = cos th I + sin th [n]x + (1 - cos th) n n^T and k the dominant axis,
    vec = 4 n_k n + 2 (1 + cos th) (e_k - n_k n): the second term (its e_k part is the extra
    2 (1 + cos th) of Q1 = 2 + 2 R_kk) is not along n.  With g = pi - th, 1 + cos th ~ g^2 / 2,
    sqrt(Q1) ~ 2 |n_k| and mag ~ pi, so the rotation vector is off by
    ~ pi g^2 (e_k - n_k n) / (4 |n_k|): for n_k >= 1 / sqrt(3) at most
    pi sqrt(3) / 4 * 2 / 3 = 0.91 g^2 in the max norm (measured here 0.03 - 0.6 g^2).  Bound:
    |oracle r - truth r| <= g^2 + 1e-9; and the deviation is real: above 1e-6 where the branch
    starts (g = 0.0315)."""
    cls, gap = g["dyn/cls"], g["dyn/gap"]
    worst = {}
    for vf, idx, truth in _frames(g):
        for row, i in enumerate(idx):
            gg = gap[cls[i]]
            if np.isnan(gg):
                continue
            err = np.abs(_oracle114(g, i, vf)[:6] - truth[row, :6]).max()
            assert err <= gg * gg + 1e-9, (vf, i, gg, err)
            worst[gg] = max(worst.get(gg, 0.0), err)
    print({k: f"{v:.2e}" for k, v in worst.items()})
    assert sorted(worst) == sorted(G.NEAR_PI_G)
    assert worst[0.0315] > 1e-6
