"""ORACLE fixture generator: the factor kernels' cases at every branch point, with their
60-digit truth (tests/factors_truth_ref.py, mpmath) and the f64 oracle's output.

    python -m oracle.gen_factors_truth            # writes tests/golden/factors_truth.npz
    python -m oracle.gen_factors_truth --table    # also prints the DESIGN.md accuracy table

Seeded and deterministic: every case draws from its own generator (SEED, case index), its
poses are built in 60 digits and rounded once to f64, so a subset regenerates bit for bit
(tests/test_factors_truth_ref.py).

Dynamics cases (dt = 1/12, world-frame |v| ~ N(0, 1), T1 = Exp(N(0, 1)^6)): w = a_w / dt
along a random axis, T2 = T1 Exp(dt [w; R1^T v]) Exp([e_w; N(0, 0.05)]).  The rotation part
of the residual is e_w in both velocity frames (the increment's rotation is Exp(dt w) in
both), so the body frame runs on the same inputs.
  * small angles: one class per a in SMALL_A with (|dt w|, |e_w|) = (a, a), (a, 1), (1, a)
    (a > 1: (1, a) only): both sides of th^2 <= eps, th < 1e-10, phi > 1e-5, tr - 3 < -1e-6
    and the last point of the acos branch (tr + 1 >= 1e-3).
  * near pi: one class per g in NEAR_PI_G, |e_w| = pi - g, for each dominant axis of the
    trace ~ -1 branch (largest diagonal R11 / R22 / R33) and both signs of the antisymmetric
    part.
Projection cases: Cal3_S2 with skew, K shared / per factor, camera pose none / shared / per
factor (six launch groups), depth pc.z in {0.3, 1e-3, -1e-3} and an exact 0.

Layout of the .npz (all f64 unless noted):
  dyn/T1, dyn/T2 (n, 12); dyn/w, dyn/v (n, 3); dyn/cls (n,) int32 class of each case;
  dyn/class_names (c,) str; dyn/gap (c,) g of a near-pi class, NaN otherwise
  dyn/world/out (n, 114, 2): [.., 0] truth, [.., 1] oracle; 114 = r 6 | J0 36 | J1 18 |
      J2 18 | J3 36, Jacobians row-major
  dyn/body/idx (m,) int32 cases that carry body-frame outputs, dyn/body/out (m, 114, 2)
  dyn/tol (c, 5) per class and output (r, J0..J3), over the class's cases in both frames;
      NaN in the near-pi classes
  proj/T, proj/Tc (n, 12; Tc NaN without a camera pose), proj/pb (n, 3), proj/z (n, 2),
  proj/K (n, 5), proj/group (n,) int32 = 3 * (K per factor) + (0 none, 1 shared, 2 per
      factor camera pose), proj/cls (n,) int32 (0: pc.z = 0.3, 1: pc.z = 1e-3, 2: cheirality),
  proj/status (n,) int32, proj/out (n, 14, 2) (r 2 | J 12 row-major; NaN where status = 1),
  proj/tol (2, 2), proj/mag (2, 2) = max |truth| per class and output (r, J)
tol = max(4 max_class |oracle - truth|, 1e-13 max(1, max_class |truth|)): the device's
rounding (1-2 ulp sincos / divide, FMA contraction) is a perturbation of the host's order
through the same condition number; 2 for the ulp ratio, 2 slack.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import factors_truth_ref as R  # noqa: E402  (tests/factors_truth_ref.py)

from oracle import factors_ref as F  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "factors_truth.npz")
SEED = 60
DT = 1.0 / 12.0
SMALL_A = [0.0, 1e-12, 0.9e-10, 1.1e-10, 1.4e-8, 1.6e-8, 1e-6, 0.9e-5, 1.1e-5, 1e-4, 0.9e-3, 1.1e-3, 1e-2, 1.0,
           3.0, math.pi - 0.1, math.pi - 0.0317]
NEAR_PI_G = [0.0315, 1e-2, 1e-3, 1e-4, 1e-6]
SNAP = 1e-30   # |truth| below this is a structural zero of the Jacobian (finite-difference noise ~1e-35)
TOL_CAP = 1e-8
OUTS = (("r", 0, 6, 1), ("J0", 6, 6, 6), ("J1", 42, 6, 3), ("J2", 60, 6, 3), ("J3", 78, 6, 6))


def dyn_specs():
    """[(class index, (|dt w|, |e_w|), axis or None, sign)] in case order, and the class names / gaps."""
    specs, names, gaps = [], [], []
    for a in SMALL_A:
        c = len(names)
        names.append(f"a={a:.6g}")
        gaps.append(np.nan)
        for aw, ae in ([(a, a), (a, 1.0), (1.0, a)] if a < 1.0 else [(1.0, a)]):
            specs.append((c, aw, ae, None, 1.0))
    for g in NEAR_PI_G:
        c = len(names)
        names.append(f"pi-{g:.6g}")
        gaps.append(g)
        for axis in (2, 1, 0):
            for sign in (1.0, -1.0):
                specs.append((c, 1.0, math.pi - g, axis, sign))
    return specs, names, np.array(gaps)


def _unit(rng):
    x = rng.standard_normal(3)
    return x / np.linalg.norm(x)


def dyn_inputs(i, spec):
    """(T1, w, v, T2) of case i."""
    _, aw, ae, axis, sign = spec
    rng = np.random.default_rng([SEED, 0, i])
    T1 = R.pose_exp12(rng.standard_normal(6))
    v = rng.standard_normal(3)
    w = (aw / DT) * _unit(rng)
    if axis is None:
        n = _unit(rng)
    else:  # component `axis` dominant (>= 1 / sqrt(1 + 2 * 0.7^2)), its sign the antisymmetric part's
        n = 0.35 * np.clip(rng.standard_normal(3), -2.0, 2.0)
        n[axis] = 1.0
        n *= sign / np.linalg.norm(n)
    e = np.concatenate([ae * n, 0.05 * rng.standard_normal(3)])
    T2 = R.predict_then_offset(T1, w, v, DT, "world", e)
    return T1, w, v, T2


def flat114(r, J):
    return np.concatenate([r] + [np.asarray(j).reshape(-1) for j in J])


def dyn_outputs(inp, vf):
    """(114, 2): truth | oracle of one case in one velocity frame."""
    T1, w, v, T2 = inp
    t = flat114(*R.dynamics(T1, w, v, T2, DT, vf))
    t[np.abs(t) < SNAP] = 0.0
    o = flat114(*F.dynamics(F.unpack(T1), w, v, F.unpack(T2), DT, vf))
    return np.stack([t, o], axis=1)


def check_branch(inp, spec):
    """The case lands on the side of each threshold its class names."""
    T1, w, v, T2 = inp
    _, aw, ae, axis, sign = spec
    P1 = F.unpack(T1)
    rel = F.between(F.compose(P1, F.pose_exp(np.concatenate([DT * w, DT * (P1[0].T @ v)]))), F.unpack(T2))[0]
    tr = np.trace(rel)
    th = np.linalg.norm(F.rot_log(rel))
    if axis is not None:
        assert tr + 1.0 < 1e-3, (spec, tr)
        assert int(np.argmax(np.diag(rel))) == axis
        wv = (rel[2, 1] - rel[1, 2], rel[0, 2] - rel[2, 0], rel[1, 0] - rel[0, 1])[axis]
        assert np.sign(wv) == sign
        return
    assert tr + 1.0 >= 1e-3
    assert (tr - 3.0 < -1e-6) == (ae > 1e-3), (spec, tr - 3)
    assert (th < 1e-10) == (ae < 1e-10), (spec, th)
    assert (th * th <= F.EPS) == (ae * ae <= F.EPS) and (th > 1e-5) == (ae > 1e-5), (spec, th)
    xw = DT * w
    assert (xw @ xw <= F.EPS) == (aw * aw <= F.EPS) and (np.linalg.norm(xw) > 1e-5) == (aw > 1e-5), (spec, xw)


def tolerances(out, cls, ncls, skip):
    """(ncls, 5): tol per class and output from out (n, 114, 2); NaN where skip[c] or no case."""
    tol = np.full((ncls, len(OUTS)), np.nan)
    for c in range(ncls):
        m = cls == c
        if skip[c] or not m.any():
            continue
        for k, (_, o, rows, cols) in enumerate(OUTS):
            t, orc = out[m, o:o + rows * cols, 0], out[m, o:o + rows * cols, 1]
            tol[c, k] = max(4.0 * np.abs(orc - t).max(), 1e-13 * max(1.0, np.abs(t).max()))
    return tol


def tol_caps():
    """(ncls, 5): what each tol may reach.  TOL_CAP everywhere but J0 / J3 of the class just under
    th^2 <= eps: there SO3 LogmapDerivative returns I, dropping W / 2 = |e_w| / 2 times a unit
    vector whose largest component is >= 1 / sqrt(3), so the oracle is off by >= 4.0e-9 at
    |e_w| = 1.4e-8 whatever the inputs, and 4 x that passes TOL_CAP; the cap there is
    4 (|e_w| / 2) + 1e-9 (the 1e-9: the class's rounding, as in its other outputs)."""
    caps = np.full((len(SMALL_A) + len(NEAR_PI_G), len(OUTS)), TOL_CAP)
    for c, a in enumerate(SMALL_A):
        if a * a <= F.EPS and 2.0 * a + 1e-9 > TOL_CAP:
            caps[c, 1] = caps[c, 4] = 2.0 * a + 1e-9
    return caps


# ----------------------------------------------------------------------------- projection
PROJ_Z = (0.3, 1e-3, -1e-3)
PROJ_DRAWS = 1
KCAL = np.array([280.0, 275.0, 1.5, 128.0, 126.0])


def proj_specs():
    """[(group, class, pc.z or None for the exact-zero case)] in case order."""
    specs = []
    for kmode in (0, 1):
        for cmode in (0, 1, 2):
            g = 3 * kmode + cmode
            for zc, pz in enumerate(PROJ_Z):
                specs += [(g, zc, pz)] * PROJ_DRAWS
            if cmode == 0:
                specs.append((g, 2, None))
    return specs


def proj_inputs(i, spec):
    """(T, pb, z, K, Tc (NaN: none)) of case i.  Shared K / camera pose: drawn from the group's
    generator, so every case of the group carries the same one."""
    import mpmath as mp

    g, _, pz = spec
    kmode, cmode = divmod(g, 3)
    rng = np.random.default_rng([SEED, 1, i])
    grng = np.random.default_rng([SEED, 2, g])
    Kg = KCAL * (1.0 + 0.02 * grng.standard_normal(5))
    Tcg = R.pose_exp12(np.concatenate([0.05 * grng.standard_normal(3), 0.03 * grng.standard_normal(3)]))
    K = KCAL * (1.0 + 0.02 * rng.standard_normal(5)) if kmode else Kg
    Tc = [np.full(12, np.nan), Tcg,
          R.pose_exp12(np.concatenate([0.05 * rng.standard_normal(3), 0.03 * rng.standard_normal(3)]))][cmode]
    if pz is None:  # pc.z exactly 0
        T = F.pack((np.eye(3), np.array([0.0, 0.0, 0.5])))
        return T, np.array([0.0, 0.0, -0.5]), np.array([128.0, 126.0]), K, Tc
    pb = 0.0175 * rng.choice([-1.0, 1.0], 3)
    Rb = R.pose_exp12(np.concatenate([rng.standard_normal(3), np.zeros(3)]))[:9].reshape(3, 3)
    pc = np.array([0.2 * abs(pz) * rng.standard_normal(), 0.2 * abs(pz) * rng.standard_normal(), pz])
    with mp.workdps(R.DPS):  # t = Rc pc + tc - R pb in 60 digits, rounded once
        Rc, tc = (np.eye(3), np.zeros(3)) if cmode == 0 else F.unpack(Tc)
        t = np.array([float(sum(mp.mpf(Rc[r, k]) * mp.mpf(pc[k]) for k in range(3)) + mp.mpf(tc[r])
                            - sum(mp.mpf(Rb[r, k]) * mp.mpf(pb[k]) for k in range(3))) for r in range(3)])
    T = np.concatenate([Rb.reshape(-1), t])
    if pz > 0:
        pix = np.array([K[0] * pc[0] / pz + K[2] * pc[1] / pz + K[3], K[1] * pc[1] / pz + K[4]])
    else:
        pix = np.array([128.0, 126.0])
    return T, pb, pix + 2.0 * rng.standard_normal(2), K, Tc


def proj_outputs(inp):
    """((14, 2) truth | oracle, status) of one case."""
    T, pb, z, K, Tc = inp
    tc = None if np.isnan(Tc[0]) else Tc
    r, J, st = R.projection(T, pb, z, K, tc)
    ro, Jo, sto, _ = F.projection(F.unpack(T), pb, z, K, None if tc is None else F.unpack(tc))
    assert st == sto
    return np.stack([np.concatenate([r, J.reshape(-1)]), np.concatenate([ro, Jo.reshape(-1)])], axis=1), st


def proj_tolerances(out, cls):
    tol, mag = np.zeros((2, 2)), np.zeros((2, 2))
    for c in range(2):
        for k, sl in enumerate((slice(0, 2), slice(2, 14))):
            t, o = out[cls == c, sl, 0], out[cls == c, sl, 1]
            mag[c, k] = np.abs(t).max()
            tol[c, k] = max(4.0 * np.abs(o - t).max(), 1e-13 * max(1.0, mag[c, k]))
    return tol, mag


def body_subset(specs):
    """Cases that carry body-frame outputs: the first of each small-angle class's (a, a) / (1, a)
    cases and one case per near-pi class (the file stays under the size of factors_golden.npz)."""
    seen, idx = set(), []
    for i, s in enumerate(specs):
        if s[0] not in seen:
            seen.add(s[0])
            idx.append(i)
    return np.array(idx, np.int32)


def generate():
    specs, names, gaps = dyn_specs()
    n, ncls = len(specs), len(names)
    cls = np.array([s[0] for s in specs], np.int32)
    inp = [dyn_inputs(i, s) for i, s in enumerate(specs)]
    for i, s in enumerate(specs):
        check_branch(inp[i], s)
    g = {"dyn/T1": np.stack([x[0] for x in inp]), "dyn/w": np.stack([x[1] for x in inp]),
         "dyn/v": np.stack([x[2] for x in inp]), "dyn/T2": np.stack([x[3] for x in inp]), "dyn/cls": cls,
         "dyn/class_names": np.array(names), "dyn/gap": gaps}
    near_pi = ~np.isnan(gaps)
    g["dyn/world/out"] = np.stack([dyn_outputs(x, "world") for x in inp])
    bi = body_subset(specs)
    g["dyn/body/idx"] = bi
    g["dyn/body/out"] = np.stack([dyn_outputs(inp[i], "body") for i in bi])
    g["dyn/tol"] = tolerances(np.concatenate([g["dyn/world/out"], g["dyn/body/out"]]),
                              np.concatenate([cls, cls[bi]]), ncls, near_pi)
    assert (np.nan_to_num(g["dyn/tol"]) <= tol_caps()).all(), g["dyn/tol"]

    ps = proj_specs()
    pin = [proj_inputs(i, s) for i, s in enumerate(ps)]
    pout = [proj_outputs(x) for x in pin]
    for k, name in enumerate(("T", "pb", "z", "K", "Tc")):
        g[f"proj/{name}"] = np.stack([x[k] for x in pin])
    g["proj/group"] = np.array([s[0] for s in ps], np.int32)
    g["proj/cls"] = np.array([s[1] for s in ps], np.int32)
    g["proj/status"] = np.array([o[1] for o in pout], np.int32)
    g["proj/out"] = np.stack([o[0] for o in pout])
    assert ((g["proj/status"] == 1) == (g["proj/cls"] == 2)).all()
    g["proj/tol"], g["proj/mag"] = proj_tolerances(g["proj/out"], g["proj/cls"])
    assert (g["proj/tol"] <= TOL_CAP * g["proj/mag"]).all(), (g["proj/tol"], g["proj/mag"])
    return g


def table(g):
    """The per-class table of DESIGN.md ("Factor accuracy at the branch points")."""
    out = np.concatenate([g["dyn/world/out"], g["dyn/body/out"]])
    cls = np.concatenate([g["dyn/cls"], g["dyn/cls"][g["dyn/body/idx"]]])
    tol = g["dyn/tol"]
    lines = ["dynamics, worst |f64 oracle - truth| over the class's cases in both frames (tol):", "",
             "| class | cases | r | J0 | J1 | J2 | J3 |", "|---|---|---|---|---|---|---|"]
    for c, name in enumerate(g["dyn/class_names"]):
        m = cls == c
        cells = []
        for k, (_, o, rows, cols) in enumerate(OUTS):
            e = np.abs(out[m, o:o + rows * cols, 1] - out[m, o:o + rows * cols, 0]).max()
            cells.append(f"{e:.1e}" + ("" if np.isnan(tol[c, k]) else f" ({tol[c, k]:.1e})"))
        lines.append(f"| {name} | {int(m.sum())} | " + " | ".join(cells) + " |")
    lines.append("")
    lines += ["projection, worst |f64 oracle - truth| (tol; max |truth|):", "", "| pc.z | cases | r | J |",
              "|---|---|---|---|"]
    for c, z in enumerate(PROJ_Z[:2]):
        m = g["proj/cls"] == c
        cells = []
        for k, sl in enumerate((slice(0, 2), slice(2, 14))):
            e = np.abs(g["proj/out"][m, sl, 1] - g["proj/out"][m, sl, 0]).max()
            cells.append(f"{e:.1e} ({g['proj/tol'][c, k]:.1e}; {g['proj/mag'][c, k]:.1e})")
        lines.append(f"| {z:g} | {int(m.sum())} | " + " | ".join(cells) + " |")
    return "\n".join(lines)


if __name__ == "__main__":
    gold = generate()
    np.savez_compressed(OUT, **gold)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(gold['dyn/cls'])} dynamics / {len(gold['proj/cls'])} "
          "projection cases")
    if "--table" in sys.argv:
        print(table(gold))
