"""Real timestamps on the device: pa_traj_args.dt_pair / kp_mask (and dt_new / mask_new in the
entry points that advance the window), pa_window_advance_t and pa_dyn_linearize_dt.

  1. legacy identity: dt_pair = dt everywhere and all-ones masks give, bit for bit, what the
     launch without them gives (linearize, the LM solve, the fused and the split tick);
  2. per-pair dt against the f64 oracle, every element, status bit-exact, canaries untouched;
  3. masks: status 2 and exact zeros, everything else bit for bit the unmasked launch, a leading
     mask is nvalid, a masked factor behind the camera has status 2, and the GN step on those
     factors is the dense oracle's (pa_window_advance_t: tests/test_timed_advance_gpu.py);
  4. pa_dyn_linearize_dt against the 60-digit truth, and n = 8 with eight dt = eight n = 1;
  5. the LM solve of tests/test_timed_ref.py's case;
  6. marginalization of a window with variable dt and a partly masked frame 0.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import lm_ref
import prior_ref as PR
import timed_ref as TR
from oracle import factors_ref as F
from oracle import gn_ref as G
from perseus_amd import _lib, pipeline, smoother, synth

import test_prior_gpu as TP  # tests/ is on sys.path (rootdir conftest)
import test_trajectory_shapes_gpu as TS

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIG = lm_ref.SIGMAS
SIGKW = dict(proj_sigmas=[SIG["proj"]] * 2, dyn_sigmas=[SIG["dyn"]] * 6, cv_sigmas=[SIG["cv"]] * 3)
ALL = 0xFFFFFFFF
MARGIN = 1e-6  # test_lm_gpu.MARGIN


def _bits_equal(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    ia = a.contiguous().view(torch.int64 if a.element_size() == 8 else torch.int32)
    ib = b.contiguous().view(torch.int64 if b.element_size() == 8 else torch.int32)
    assert torch.equal(ia, ib), what


def _same_outputs(a, b, what):
    for k in TS.WIDTH:
        if a.get(k) is not None or b.get(k) is not None:
            _bits_equal(a[k], b[k], f"{what}: {k}")


def _dt_pairs(T, L, seed):
    """log-uniform in [1/240, 0.5]"""
    rng = np.random.default_rng(seed)
    return np.exp(rng.uniform(np.log(1.0 / 240.0), np.log(0.5), (T, L - 1)))


# ---------------------------------------------------------------- 1. legacy identity
ID_T, ID_L, ID_K = 3, 4, 8


@pytest.fixture(scope="module")
def id_problem():
    pr = lm_ref.problem(ID_T, ID_L, 0.05)
    rng = np.random.default_rng(3)
    pr["vel"] = 0.01 * rng.standard_normal(pr["vel"].shape)
    pr["angvel"] = 0.3 * rng.standard_normal(pr["angvel"].shape)
    return pr


def _id_extra():
    return dict(dt_pair=np.full((ID_T, ID_L - 1), lm_ref.DT), kp_mask=np.full((ID_T, ID_L), ALL, np.int64))


def test_identity_linearize(id_problem):
    pr = id_problem
    y = torch.as_tensor(pr["y"], device=DEV)
    for sig in ({}, SIGKW):
        a = pipeline.linearize_trajectories(y, pr["pose"], pr["vel"], pr["angvel"], synth.CUBE_CORNERS, synth.CAMERA_K,
                                            T=ID_T, L=ID_L, dt=lm_ref.DT, **sig)
        for extra in (_id_extra(), dict(dt_pair=_id_extra()["dt_pair"]), dict(kp_mask=_id_extra()["kp_mask"])):
            b = pipeline.linearize_trajectories(y, pr["pose"], pr["vel"], pr["angvel"], synth.CUBE_CORNERS,
                                                synth.CAMERA_K, T=ID_T, L=ID_L, dt=lm_ref.DT, **sig, **extra)
            _same_outputs(a, b, f"linearize {sorted(extra)}")


def test_identity_lm_solve(id_problem):
    pr = id_problem
    y = torch.as_tensor(pr["y"], device=DEV)
    kw = dict(T=ID_T, L=ID_L, dt=lm_ref.DT, **SIGKW, **lm_ref.PARAMS)
    a = pipeline.lm_solve(y, pr["pose"], pr["vel"], pr["angvel"], synth.CUBE_CORNERS, synth.CAMERA_K, **kw)
    b = pipeline.lm_solve(y, pr["pose"], pr["vel"], pr["angvel"], synth.CUBE_CORNERS, synth.CAMERA_K, **kw, **_id_extra())
    for k in ("pose", "vel", "angvel", "cost0", "cost", "iters", "status", "lambda"):
        _bits_equal(a[k], b[k], f"lm {k}")
    assert (a["iters"] > 0).all()
    _same_outputs(a["lin"], b["lin"], "lm lin")
    # with the marginalization prior (pa_trajectory_lm_prior_solve accepts the fields)
    outs = []
    for extra in ({}, _id_extra()):
        prior = pipeline.PriorPlan(T=ID_T, L=ID_L, device=DEV)
        info, _ = PR.random_spd(np.random.default_rng(11), ID_T, 3.0)
        prior.cur["info"].copy_(torch.as_tensor(info, device=DEV))
        prior.cur["xbar_pose"].copy_(torch.as_tensor(pr["pose"].reshape(ID_T, ID_L, 12)[:, 0], device=DEV))
        outs.append(pipeline.lm_solve(y, pr["pose"], pr["vel"], pr["angvel"], synth.CUBE_CORNERS, synth.CAMERA_K,
                                      prior=prior, newest_pending=True, **kw, **extra))  # pa_window_lm_prior_solve
        outs[-1]["pgrad"] = prior.grad.clone()
    for k in ("pose", "vel", "angvel", "cost0", "cost", "iters", "status", "lambda", "pgrad"):
        _bits_equal(outs[0][k], outs[1][k], f"lm prior {k}")


class Window:
    """A streaming window on the device and its pa_traj_args, with or without the rings."""

    def __init__(self, pose0, L, nk, timed, dt=lm_ref.DT):
        T = len(pose0)
        f64 = dict(dtype=torch.float64, device=DEV)
        self.T, self.L, self.nk, self.timed = T, L, nk, timed
        self.win = {"y": torch.zeros((T, L, 2 * nk), dtype=torch.float32, device=DEV),
                    "pose": torch.as_tensor(np.repeat(np.asarray(pose0).reshape(T, 1, 12), L, 1), **f64).contiguous(),
                    "angvel": torch.zeros((T, L, 3), **f64), "vel": torch.zeros((T, L, 3), **f64)}
        self.nvalid = torch.zeros(T, dtype=torch.int32, device=DEV)
        extra = {}
        if timed:
            self.win["dt"] = torch.full((T, L - 1), dt, **f64)
            self.win["mask"] = torch.full((T, L), -1, dtype=torch.int32, device=DEV)
            extra = dict(dt_pair=self.win["dt"], kp_mask=self.win["mask"])
            self.dt_new = torch.full((T,), dt, **f64)
            self.mask_new = torch.full((T,), -1, dtype=torch.int32, device=DEV)
        self.args, self.lin = pipeline.prepare_trajectories(
            self.win["y"].view(T * L, 2 * nk), self.win["pose"].view(T * L, 12), self.win["vel"].view(T * L, 3),
            self.win["angvel"].view(T * L, 3), synth.CUBE_CORNERS[:nk], synth.CAMERA_K, T=T, L=L, dt=dt,
            proj_sigmas=[TR.TICK_SIG["proj"]] * 2, dyn_sigmas=[TR.TICK_SIG["dyn"]] * 6,
            cv_sigmas=[TR.TICK_SIG["cv"]] * 3, nvalid=self.nvalid, **extra)
        if timed:
            assert self.args.dt_pair == self.win["dt"].data_ptr() and self.args.kp_mask == self.win["mask"].data_ptr()
            self.args.dt_new, self.args.mask_new = self.dt_new.data_ptr(), self.mask_new.data_ptr()
        self.delta = torch.zeros((T * L, 12), **f64)
        self.info = torch.zeros(T, dtype=torch.int32, device=DEV)
        self.newest = torch.zeros((T, 12), **f64)
        self.ws = pipeline.window_pose_tick_workspace(T, L, DEV)

    def tick(self, y, split, dt_new=None, mask_new=None):
        y = torch.as_tensor(np.asarray(y, np.float32), device=DEV).contiguous()
        if self.timed:
            if dt_new is not None:
                self.dt_new.copy_(torch.as_tensor(np.asarray(dt_new, np.float64), device=DEV))
            if mask_new is not None:
                self.mask_new.copy_(torch.as_tensor(np.asarray(mask_new).astype(np.int64).astype(np.uint32).view(np.int32),
                                                    device=DEV))
        if split:
            pipeline.window_pose_tick_pre(self.args, self.ws, lam=TR.TICK_LAM)
            pipeline.window_pose_tick_post(self.args, y, self.ws, delta=self.delta, info=self.info, newest=self.newest)
        else:
            pipeline.window_pose_tick(self.args, y, lam=TR.TICK_LAM, delta=self.delta, info=self.info, newest=self.newest)
        torch.cuda.synchronize()

    def state(self):
        out = {k: v.clone() for k, v in self.win.items()}
        out.update(delta=self.delta.clone(), info=self.info.clone(), newest=self.newest.clone(),
                   **{k: self.lin[k].clone() for k in TS.WIDTH if self.lin.get(k) is not None})
        return out


@pytest.mark.parametrize("split", [False, True], ids=["fused", "split"])
def test_identity_ticks(split):
    truth, _, _ = lm_ref.truth(ID_T, 3)
    pose0 = TR.init_pose(truth[0])
    a, b = Window(pose0, ID_L, ID_K, False), Window(pose0, ID_L, ID_K, True)
    for k in range(3):
        y = lm_ref.keypoints(truth[k])
        a.tick(y, split)
        b.tick(y, split)
        sa, sb = a.state(), b.state()
        for key in sa:
            _bits_equal(sa[key], sb[key], f"tick {k} {key}")
        assert (sa["info"] == 0).all()
        assert torch.equal(sb["dt"], torch.full_like(sb["dt"], lm_ref.DT)) and (sb["mask"] == -1).all()


# ---------------------------------------------------------------- 2. per-pair dt against the oracle
def _launch(P, whiten, **extra):
    """TS.Problem.launch (sentinel-filled allocations, canaries checked) with dt_pair / kp_mask."""
    p = P.p
    sig = dict(proj_sigmas=TS.SP, dyn_sigmas=TS.SD, cv_sigmas=TS.SC) if whiten else {}
    args, keep = pipeline.prepare_trajectories(torch.as_tensor(p["y"], device=DEV), p["poses"], p["vels"], p["angvels"],
                                               p["corners"], TS.KCAL, T=P.T, L=P.L, dt=TS.DT, vel_frame=P.vf, **sig,
                                               **extra)
    saved, P.staged = P.staged, {(whiten, None): (args, keep)}
    try:
        return P.launch(whiten)
    finally:
        P.staged = saved


_PROBS = {}


def _prob(shape):
    if shape not in _PROBS:
        T, L, nk, vf = shape
        P = TS.Problem(T, L, nk, vf)
        P.dtp = _dt_pairs(T, L, 7 * T + L)
        idx = np.array([t * L + l for t in range(T) for l in range(L - 1)], dtype=np.int64)
        for j, f in enumerate(idx):  # the dynamics factors again, each with its own dt
            r, H = F.dynamics(F.unpack(P.p["poses"][f]), P.p["angvels"][f], P.p["vels"][f], F.unpack(P.p["poses"][f + 1]),
                              float(P.dtp.reshape(-1)[j]), vf)
            P.ref["r_dyn"][j] = r
            for k in range(4):
                P.ref[f"j_dyn{k}"][j] = H[k].T  # (column-major per factor, as TS._oracle lays them out)
        _PROBS[shape] = P
    return _PROBS[shape]


@pytest.mark.parametrize("vf", ["world", "body"])
@pytest.mark.parametrize("nk", [1, 8, 16])
@pytest.mark.parametrize("TL", [(1, 2), (3, 4), (5, 14)], ids=["1x2", "3x4", "5x14"])
def test_per_pair_dt_vs_oracle(TL, nk, vf):
    """(5, 14): 65 dynamics pairs, one past the 64-factor block.  The "factors" bar."""
    P = _prob((*TL, nk, vf))
    out = _launch(P, False, dt_pair=P.dtp)
    st = out["status"].cpu().numpy()
    np.testing.assert_array_equal(st, P.ref["status"])
    ok = st == 0
    for name, (kind, per) in TS.WIDTH.items():
        if name == "status" or name.startswith("err"):
            continue
        got = TS._f64(out[name]).reshape(P.count[kind], -1)
        ref = np.asarray(P.ref[name], np.float64).reshape(P.count[kind], -1)
        if kind == 0:
            assert np.isnan(got[~ok]).all()
            got, ref = got[ok], ref[ok]
        np.testing.assert_allclose(got, ref, atol=1e-9, rtol=1e-12, err_msg=name)
    # the projection and constant-velocity factors do not know about dt: bit for bit the plain launch
    plain = P.launch(False)
    for name in ("r_proj", "j_proj", "status", "r_cv", "j_cv0", "j_cv1"):
        assert torch.equal(out[name], plain[name]), name
    assert not torch.equal(out["r_dyn"], plain["r_dyn"])


# ---------------------------------------------------------------- 3. masks
def _masks(T, L, nk, seed):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 1 << nk, (T, L)).astype(np.int64)
    m[0, 0] = 0                      # an all-zero frame
    m[-1, -1] = 1 << (nk - 1)        # a single set bit, the highest keypoint's (bit 15 at n_kp = 16)
    m |= rng.integers(0, 1 << 16, (T, L)).astype(np.int64) << 16 if nk <= 16 else 0  # bits above n_kp: ignored
    return m


@pytest.mark.parametrize("shape", [(3, 4, 16, "world"), (5, 14, 8, "body"), (1, 2, 1, "world")],
                         ids=["3x4x16", "5x14x8", "1x2x1"])
def test_masks(shape):
    T, L, nk, vf = shape
    P = _prob(shape)
    m = _masks(T, L, nk, 5)
    b = P.p["behind"]
    m.reshape(-1)[b] &= ~1  # keypoint 0 of the frame behind the camera: masked
    if nk > 1:
        m.reshape(-1)[b] |= 2  # and keypoint 1 measured: still cheirality
    off = TR.mask_off(m.reshape(-1) & ((1 << nk) - 1), T * L, nk)
    for whiten in (False, True):
        plain, out = P.launch(whiten), _launch(P, whiten, kp_mask=m)
        st, st0 = out["status"].cpu().numpy(), plain["status"].cpu().numpy()
        np.testing.assert_array_equal(st[off], 2)
        np.testing.assert_array_equal(st[~off], st0[~off])
        assert st[b * nk] == 2 and st0[b * nk] == 1  # masked wins over cheirality
        if nk > 1:
            assert st[b * nk + 1] == 1
        for name, (kind, per) in TS.WIDTH.items():
            got, ref = out[name].view(-1, per), plain[name].view(-1, per)
            if kind == 0:
                if name != "status":
                    assert not bool(got[torch.as_tensor(off, device=DEV)].any()), name  # exact zeros (0 bits)
                sel = torch.as_tensor(~off, device=DEV)
                assert torch.equal(got[sel], ref[sel]), name
            else:
                assert torch.equal(got, ref), name
    # a mask clearing exactly the leading L - nvalid frames is the nvalid launch
    nvalid = np.random.default_rng(1).integers(0, L + 1, T).astype(np.int32)
    lead = np.where(np.arange(L)[None, :] < (L - nvalid)[:, None], 0, ALL)
    a = P.launch(True, nvalid=torch.as_tensor(nvalid, device=DEV))
    c = _launch(P, True, kp_mask=lead)
    for name in TS.WIDTH:
        assert torch.equal(a[name], c[name]), name


def test_masked_gn_step_vs_oracle():
    T, L, nk, lam = 3, 6, 8, 1e-2
    pr = TR.lm_problem(T, L, 0.02)
    dtp, msk = np.tile(TR.LM_DT_PAIR, (T, 1)), np.tile(TR.LM_MASKS, (T, 1))
    msk[1] = _masks(1, L, nk, 9)[0] & 0xFF
    lin = pipeline.linearize_trajectories(torch.as_tensor(pr["y"], device=DEV), pr["pose"], pr["vel"], pr["angvel"],
                                          synth.CUBE_CORNERS, synth.CAMERA_K, T=T, L=L, dt=lm_ref.DT, **SIGKW,
                                          dt_pair=dtp, kp_mask=msk)
    g = pipeline.gn_step(lin, T=T, L=L, lam=lam)
    keys = ("r_proj", "j_proj", "status", "r_dyn", "j_dyn0", "j_dyn1", "j_dyn2", "j_dyn3", "r_cv", "j_cv0", "j_cv1",
            "err_proj", "err_dyn", "err_cv")  # (err_*: 0.5 |r_w|^2 per factor, err_dyn under its pair's dt)
    dev = {k: lin[k].cpu().numpy() for k in keys}
    _, _, d = G.gn_step(dev, T, L, nk, lam)
    assert (g["info"].cpu().numpy() == 0).all()
    np.testing.assert_allclose(g["delta"].cpu().numpy().reshape(T, -1), d, rtol=1e-7, atol=1e-9 * np.abs(d).max())
    # and the device's factors are the reference's
    for t in range(T):
        s = slice(t * L, (t + 1) * L)
        ref = TR.factors(pr["y"][s], pr["pose"][s], pr["vel"][s], pr["angvel"][s], L, dt_pair=dtp[t], kp_mask=msk[t])
        np.testing.assert_array_equal(dev["status"][t * L * nk:(t + 1) * L * nk], ref["status"])
        for k in keys:
            if k != "status":
                n = len(ref[k])
                np.testing.assert_allclose(dev[k][t * n:(t + 1) * n], ref[k], atol=1e-9, rtol=1e-12, err_msg=k)


# ---------------------------------------------------------------- 4. pa_dyn_linearize_dt against the truth
@pytest.fixture(scope="module")
def truth_cases():
    import factors_truth_ref as FT

    rng = np.random.default_rng(21)
    cases = []
    for vf in ("world", "body"):
        for dt in (1.0 / 240.0, 1.0 / 30.0, 0.1, 0.5):  # rotations 0.2 .. 1.3 rad: away from every branch point
            T1 = FT.pose_exp12(np.concatenate([0.5 * rng.standard_normal(3), 0.2 * rng.standard_normal(3)]))
            w, v = 0.8 * rng.standard_normal(3), 0.3 * rng.standard_normal(3)
            T2 = FT.predict_then_offset(T1, w, v, dt, vf, np.concatenate([0.3 * rng.standard_normal(3),
                                                                          0.05 * rng.standard_normal(3)]))
            r, J = FT.dynamics(T1, w, v, T2, dt, vf)
            ro, Jo = F.dynamics(F.unpack(T1), w, v, F.unpack(T2), dt, vf)
            cases.append(dict(vf=vf, dt=dt, T1=T1, w=w, v=v, T2=T2, truth=[r, *J], oracle=[ro, *Jo]))
    return cases


def test_dyn_linearize_dt_vs_truth(truth_cases):
    """DESIGN 3.1's rule per output: tol = max(4 max|oracle - truth|, 1e-13 max(1, max|truth|)),
    from the oracle on these same cases."""
    names = ("r", "J0", "J1", "J2", "J3")
    for vf in ("world", "body"):
        cs = [c for c in truth_cases if c["vf"] == vf]
        stack = lambda k: np.stack([c[k] for c in cs])
        dts = np.array([c["dt"] for c in cs])
        out = smoother.linearize_dynamics(stack("T1"), stack("w"), stack("v"), stack("T2"), dts, vf)
        for k, name in enumerate(names):
            tr = np.stack([c["truth"][k] for c in cs])
            orc = np.stack([c["oracle"][k] for c in cs])
            tol = max(4.0 * np.abs(orc - tr).max(), 1e-13 * max(1.0, np.abs(tr).max()))
            err = np.abs(out[name].cpu().numpy() - tr).max()
            print(f"{vf} {name}: |gpu - truth| {err:.2e}, tol {tol:.2e}")
            assert err <= tol, (vf, name, err, tol)
        # one launch with four dt = four launches of one factor, bit for bit
        for i, c in enumerate(cs):
            one = smoother.linearize_dynamics(c["T1"][None], c["w"][None], c["v"][None], c["T2"][None],
                                              np.array([c["dt"]]), vf)
            for name in names:
                _bits_equal(one[name].contiguous(), out[name][i:i + 1].contiguous(), f"{vf} {i} {name}")


def test_dyn_linearize_dt_eight_at_once(truth_cases):
    """n = 8 with eight different dt (both frames' inputs, one frame per launch) = eight n = 1 launches."""
    cs = truth_cases
    stack = lambda k: np.stack([c[k] for c in cs])
    dts = np.array([c["dt"] * (1.0 + 0.1 * i) for i, c in enumerate(cs)])
    assert len(set(dts.tolist())) == 8
    for vf in ("world", "body"):
        out = smoother.linearize_dynamics(stack("T1"), stack("w"), stack("v"), stack("T2"), dts, vf,
                                          inv_sigma=np.full(6, 10.0))
        for i, c in enumerate(cs):
            one = smoother.linearize_dynamics(c["T1"][None], c["w"][None], c["v"][None], c["T2"][None], dts[i:i + 1], vf,
                                              inv_sigma=np.full(6, 10.0))
            for name in ("r", "J0", "J1", "J2", "J3", "err"):
                _bits_equal(one[name].contiguous(), out[name][i:i + 1].contiguous(), f"{vf} {i} {name}")


# ---------------------------------------------------------------- 5. Levenberg-Marquardt
def test_lm_case_on_the_device():
    T, L = 3, 6
    pr = TR.lm_problem(T, L, 0.1)
    dtp, msk = np.tile(TR.LM_DT_PAIR, (T, 1)), np.tile(TR.LM_MASKS, (T, 1))
    ref = TR.solve(pr["y"], pr["pose"], pr["vel"], pr["angvel"], T, L, dt_pair=dtp, kp_mask=msk)
    out = pipeline.lm_solve(torch.as_tensor(pr["y"], device=DEV), pr["pose"], pr["vel"], pr["angvel"], synth.CUBE_CORNERS,
                            synth.CAMERA_K, T=T, L=L, dt=lm_ref.DT, **SIGKW, dt_pair=dtp, kp_mask=msk, **lm_ref.PARAMS)
    st, it = out["status"].cpu().numpy(), out["iters"].cpu().numpy()
    print("status", st, ref["status"], "iters", it, ref["iters"], "cost", out["cost"].cpu().numpy(), ref["cost"])
    decided = [t for t in range(T) if all(r["margin"] >= MARGIN for r in ref["log"][t])]
    print("trajectories decided with the margin throughout:", decided)
    assert decided == [0, 1, 2]  # (on the reference alone: every decision of this case has the margin)
    for t in decided:  # every decision of the reference is one f64 rounding cannot flip
        assert st[t] == ref["status"][t] == _lib.LM_CONVERGED and it[t] == ref["iters"][t], (t, st, it)
    rot, tra = lm_ref.pose_errors(out["pose"].cpu().numpy(), pr["truth"])
    rot, tra = rot.reshape(T, L), tra.reshape(T, L)
    m = list(TR.LM_MEASURED)
    print("rot", rot.max(0), "tra", tra.max(0))
    assert rot[:, m].max() < TR.ROT_TOL and tra[:, m].max() < TR.TRA_TOL


# ---------------------------------------------------------------- 6. marginalization
def test_marginalize_with_variable_dt_and_a_masked_frame_0():
    T, L, K, lam = 3, 6, 8, 1e-3
    pr = TR.lm_problem(T, L, 0.02)
    rng = np.random.default_rng(4)
    pr["vel"] = 0.01 * rng.standard_normal(pr["vel"].shape)
    pr["angvel"] = 0.3 * rng.standard_normal(pr["angvel"].shape)
    dtp = _dt_pairs(T, L, 12)
    msk = np.full((T, L), 0xFF, np.int64)
    msk[:, 0] = [0b00101101, 0b11110000, 0b10000001]  # frame 0 partly masked
    sig = dict(proj=2.0, dyn=0.05, cv=0.5)
    lin = pipeline.linearize_trajectories(torch.as_tensor(pr["y"], device=DEV), pr["pose"], pr["vel"], pr["angvel"],
                                          synth.CUBE_CORNERS, synth.CAMERA_K, T=T, L=L, dt=lm_ref.DT,
                                          proj_sigmas=[2.0, 2.0], dyn_sigmas=[0.05] * 6, cv_sigmas=[0.5] * 3,
                                          dt_pair=dtp, kp_mask=msk)
    fs = [TR.factors(pr["y"][t * L:(t + 1) * L], pr["pose"][t * L:(t + 1) * L], pr["vel"][t * L:(t + 1) * L],
                     pr["angvel"][t * L:(t + 1) * L], L, dt_pair=dtp[t], kp_mask=msk[t], sigmas=sig) for t in range(T)]
    f = {k: np.concatenate([x[k] for x in fs], 0) for k in TP.KEYS}
    pinfo, pgrad = PR.random_spd(np.random.default_rng(8), T, 3.0)
    ref_info, ref_eta, ref_minfo = PR.marginalize(f, T, L, K, lam, pinfo, pgrad, nvalid=np.full(T, L, np.int32))
    raw = {k: (lin[k].transpose(1, 2).contiguous() if k in TP.JAC else lin[k]) for k in TP.KEYS}
    c = dict(T=T, L=L, K=K, lam=lam, raw=raw, pose=pr["pose"], vel=pr["vel"], angvel=pr["angvel"])
    out = TP._marginalize(c, pinfo=pinfo, pgrad=pgrad, nvalid=np.full(T, L, np.int32))
    np.testing.assert_array_equal(out["minfo"], ref_minfo)
    assert (ref_minfo == 0).all()
    TP._close_blocks(out["info"], ref_info, "info")
    TP._close_blocks(out["eta"], ref_eta, "eta")
