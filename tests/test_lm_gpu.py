"""pa_trajectory_lm_solve (pipeline.lm_solve / LMPlan, StreamingPipeline.solve_window) on the
device against the numpy restatement tests/lm_ref.py:

  * decision-for-decision parity from a start 0.8 rad off (rejected steps on the way), over the
    iterations whose accept / reject decision the reference takes with a margin f64 rounding
    cannot flip (|C' - C| / C >= 1e-6, asserted on the reference alone);
  * convergence to the true trajectories within the project's bounds, in the reference's
    number of iterations; real rejects (cost plateaus) and the reference's final damping;
  * the cheirality guard, nvalid windows, per-trajectory independence and early exit, more
    trajectories than CUs, determinism, graph replay, a window whose newest frame is pending,
    and the streaming pipeline's method with and without pre_ahead, every following tick checked.
"""
import numpy as np
import pytest
import torch

import lm_ref  # tests/ is on sys.path (rootdir conftest)
from oracle import factors_ref as F
from perseus_amd import _lib, pipeline, synth

pytestmark = pytest.mark.gpu

MARGIN = 1e-6  # decisions the reference takes with a smaller |C' - C| / C are not compared
# Worst deviation of the device from lm_ref measured on an MI355X over this file's compared cases
# (both parity shapes, the 0.8 rad solve to convergence, the 0.1 rad, guard, nvalid and pending
# cases; DESIGN.md "Levenberg-Marquardt on the device"): state 7.76e-12 (absolute, on pose entries
# and velocities of magnitude <= 1), cost_hist 1.9e-9 relative.  The reduction and elimination
# orders differ and the error compounds over iterations; the bounds are 10 x the measured values.
# (The state figure is the pending case's, whose newest frame only its dynamics factor and the
# damping, down to 1e-7, hold; every other case stays below 4.1e-13.  The cost figure is set at
# the noise floor, C ~ 1e-10: its residuals of ~1e-5 px are differences of ~128 px quantities,
# eps * 128 / 1e-5 = 2.8e-9 relative each; above the floor the measured deviation is 1e-16 .. 1e-11.)
# The n_kp = 5 parity case (lm_step_kernel's general instantiation), measured the same way: state
# 4.82e-13, cost_hist 1.72e-9 relative (at the same floor), inside the bounds above.
STATE_ATOL = 7.76e-11
HIST_RTOL = 1.9e-8
ROT_TOL, TRA_TOL = 1e-4, 1e-5  # test_streaming_pose_gpu.test_pose_tracks_known_trajectory
SIG = lm_ref.SIGMAS


def _dev(pr, T, L, params, nvalid=None, pending=False, corners=None):
    """pipeline.lm_solve on a lm_ref problem; numpy outputs."""
    nv = None if nvalid is None else torch.as_tensor(np.asarray(nvalid, np.int32), device="cuda")
    out = pipeline.lm_solve(torch.as_tensor(pr["y"], device="cuda"), pr["pose"], pr["vel"], pr["angvel"],
                            synth.CUBE_CORNERS if corners is None else corners, synth.CAMERA_K, T=T, L=L, dt=lm_ref.DT,
                            proj_sigmas=[SIG["proj"]] * 2, dyn_sigmas=[SIG["dyn"]] * 6, cv_sigmas=[SIG["cv"]] * 3,
                            nvalid=nv, newest_pending=pending, **params)
    torch.cuda.synchronize()
    res = {k: out[k].cpu().numpy() for k in ("pose", "vel", "angvel", "cost0", "cost", "iters", "status", "lambda",
                                             "cost_hist")}
    res["lin"] = out["lin"]
    return res


def _ref(pr, T, L, params, nvalid=None, pending=False, corners=None):
    return lm_ref.solve(pr["y"], pr["pose"], pr["vel"], pr["angvel"], T, L, params, nvalid=nvalid, pending=pending,
                        corners=corners)


def _deviation(dev, ref):
    """(state deviation, relative cost_hist deviation) over every compared entry."""
    ds = max(np.abs(dev[k] - ref[k]).max() for k in ("pose", "vel", "angvel"))
    h, g = dev["cost_hist"], ref["cost_hist"]
    np.testing.assert_array_equal(np.isnan(h), np.isnan(g))
    ok = ~np.isnan(g)
    dh = (np.abs(h[ok] - g[ok]) / g[ok]).max()
    return ds, dh


def _assert_matches(dev, ref, T, what):
    np.testing.assert_array_equal(dev["iters"], ref["iters"], err_msg=what)
    np.testing.assert_array_equal(dev["status"], ref["status"], err_msg=what)
    np.testing.assert_array_equal(dev["lambda"], ref["lambda"], err_msg=what)  # powers of 10, the same operations
    ds, dh = _deviation(dev, ref)
    print(f"{what}: state deviation {ds:.3g}, cost_hist relative deviation {dh:.3g}")
    assert ds <= STATE_ATOL and dh <= HIST_RTOL, (what, ds, dh)
    for t in range(T):
        k = ref["iters"][t]
        assert dev["cost0"][t] == dev["cost_hist"][t, 0] and dev["cost"][t] == dev["cost_hist"][t, k]


def _well_defined(ref, T):
    """Per trajectory the number of leading iterations whose decision has margin >= MARGIN."""
    n = []
    for t in range(T):
        m = [r["margin"] >= MARGIN for r in ref["log"][t]]
        n.append(m.index(False) if False in m else len(m))
    return n


# ---------------------------------------------------------------- parity
PARITY = dict(lm_ref.PARAMS, rel_tol=0.0, abs_tol=0.0, max_iters=8)


@pytest.mark.parametrize("T,L", [(3, 6), (2, 24)])
def test_decisions_match_reference(T, L):
    """0.8 rad off, rel_tol = abs_tol = 0, 8 iterations: cost_hist is compared per trajectory up to
    the first decision the reference takes with margin < 1e-6 (a trajectory that reaches the noise
    floor of its f32 keypoints early then improves by 1e-8 relative steps), and a second solve of
    as many iterations as EVERY trajectory decides with that margin is compared in full: iters,
    status, lambda, cost_hist and the final state."""
    _check_decisions(lm_ref.problem(T, L, 0.8), T, L)


def test_decisions_match_reference_five_keypoints():
    """n_kp = 5 (the first five cube corners): lm_step_kernel's general instantiation, which every
    other case of this file (8 corners) leaves out.  The comparison of test_decisions_match_reference;
    the reference decides 8 and 6 leading iterations with the margin, trajectory 0 rejecting its first
    five steps and trajectory 1 accepting its first seven."""
    T, L = 2, 6
    pr = lm_ref.problem(T, L, 0.8)
    pr["y"] = np.ascontiguousarray(pr["y"][:, :10])
    _check_decisions(pr, T, L, corners=synth.CUBE_CORNERS[:5])


def _check_decisions(pr, T, L, corners=None):
    ref = _ref(pr, T, L, PARITY, corners=corners)
    nok = _well_defined(ref, T)
    dec = [[r["accept"] for r in log] for log in ref["log"]]
    print("reference decisions:", dec, "well defined:", nok)
    assert min(nok) >= 5  # (the seeds' figure; a change of the problem that lowers it needs another seed)
    assert any(not a for d, n in zip(dec, nok) for a in d[:n]), "no reject among the compared decisions"
    assert any(a for d, n in zip(dec, nok) for a in d[:n]), "no accept among the compared decisions"
    dev = _dev(pr, T, L, PARITY, corners=corners)
    for t in range(T):
        n = nok[t]
        h, g = dev["cost_hist"][t, :n + 1], ref["cost_hist"][t, :n + 1]
        dh = (np.abs(h - g) / g).max()
        print(f"trajectory {t}: {n} iterations compared, cost_hist relative deviation {dh:.3g}")
        assert dh <= HIST_RTOL, (t, dh)
        np.testing.assert_array_equal(np.diff(h) < 0, dec[t][:n])  # the same accepts and rejects
    m = min(nok)
    short = dict(PARITY, max_iters=m)
    ref_m = _ref(pr, T, L, short, corners=corners)
    for t in range(T):
        assert all(r["margin"] >= MARGIN for r in ref_m["log"][t])  # every compared decision, on the reference alone
    _assert_matches(_dev(pr, T, L, short, corners=corners), ref_m, T, f"T={T} L={L}, {m} iterations")
    for t in range(T):  # trajectories decided with the margin throughout: the 8-iteration solve in full
        if nok[t] == PARITY["max_iters"]:
            one = {k: (v[t * L:(t + 1) * L] if k in ("pose", "vel", "angvel") else v[t:t + 1])
                   for k, v in dev.items() if k != "lin"}
            ref1 = {k: (v[t * L:(t + 1) * L] if k in ("pose", "vel", "angvel") else v[t:t + 1])
                    for k, v in ref.items() if k != "log"}
            _assert_matches(one, ref1, 1, f"T={T} L={L}, trajectory {t}, 8 iterations")


# ---------------------------------------------------------------- convergence, accept / reject
def test_converges_to_truth_like_reference():
    """test_lm_ref.py's 0.1 rad case on the device: CONVERGED within the bounds, in the
    reference's number of iterations."""
    T, L = 3, 6
    pr = lm_ref.problem(T, L, 0.1)
    ref = _ref(pr, T, L, lm_ref.PARAMS)
    dev = _dev(pr, T, L, lm_ref.PARAMS)
    assert (ref["status"] == lm_ref.CONVERGED).all()
    assert (dev["status"] == _lib.LM_CONVERGED).all(), dev["status"]
    np.testing.assert_array_equal(dev["iters"], ref["iters"])
    rot, tra = lm_ref.pose_errors(dev["pose"], pr["truth"])
    print(f"iters {dev['iters']}, rot err {rot.max():.3g} rad, trans err {tra.max():.3g} m")
    assert rot.max() < ROT_TOL and tra.max() < TRA_TOL
    # on return the factor outputs hold the linearization at the final state
    lin = pipeline.linearize_trajectories(torch.as_tensor(pr["y"], device="cuda"), dev["pose"], dev["vel"],
                                          dev["angvel"], synth.CUBE_CORNERS, synth.CAMERA_K, T=T, L=L, dt=lm_ref.DT,
                                          proj_sigmas=[SIG["proj"]] * 2, dyn_sigmas=[SIG["dyn"]] * 6,
                                          cv_sigmas=[SIG["cv"]] * 3)
    for k, v in lin.items():
        if isinstance(v, torch.Tensor):
            got = dev["lin"][k].transpose(1, 2) if k.startswith("j_") else dev["lin"][k]
            assert torch.equal(got, v), k


def test_rejects_are_real():
    """From 0.8 rad: at least one cost plateau (a rejected step: the present fixed-lambda chain
    would have applied it), cost_hist never increases, the final lambda is the reference's.
    (Seed 4: the reference takes every decision up to convergence with margin >= 1e-6; with the
    other tests' seed 5 one trajectory's last accept has 1e-8.)"""
    T, L = 3, 6
    pr = lm_ref.problem(T, L, 0.8, seed=4)
    ref = _ref(pr, T, L, lm_ref.PARAMS)
    assert all(r["margin"] >= MARGIN for log in ref["log"] for r in log)
    assert sum(not r["accept"] for log in ref["log"] for r in log) >= 1
    dev = _dev(pr, T, L, lm_ref.PARAMS)
    plateaus = 0
    for t in range(T):
        k = dev["iters"][t]
        h = dev["cost_hist"][t]
        assert np.isfinite(h[:k + 1]).all() and np.isnan(h[k + 1:]).all()
        assert (np.diff(h[:k + 1]) <= 0).all(), (t, h)
        plateaus += int((np.diff(h[:k + 1]) == 0).sum())
    print("iters", dev["iters"], "reference", ref["iters"], "plateaus", plateaus)
    assert plateaus >= 1
    np.testing.assert_array_equal(dev["lambda"], ref["lambda"])
    assert (dev["status"] == _lib.LM_CONVERGED).all()
    _assert_matches(dev, ref, T, "0.8 rad to convergence")
    rot, tra = lm_ref.pose_errors(dev["pose"], pr["truth"])
    assert rot.max() < ROT_TOL and tra.max() < TRA_TOL


# ---------------------------------------------------------------- cheirality guard
def _guard_problem(L=6):
    """Trajectory 0: a 0.8 rad problem's.  Trajectory 1: a static cube 0.12 m from the camera
    whose window starts 0.6 m away: the image is 5 x larger than predicted, and the linearized
    depth correction (-4 x the depth) puts every corner behind the camera."""
    pr = lm_ref.problem(1, L, 0.8)
    R0, _ = F.pose_exp(np.array([0.2, -0.1, 0.3, 0.0, 0.0, 0.0]))
    true = (R0, np.array([0.005, -0.003, 0.12]))
    y = np.repeat(lm_ref.keypoints([true]), L, 0)
    pose = np.tile(F.pack((R0, np.array([0.005, -0.003, 0.6]))), (L, 1))
    z = np.zeros((L, 3))
    return dict(y=np.concatenate([pr["y"], y]), pose=np.concatenate([pr["pose"], pose]),
                vel=np.concatenate([pr["vel"], z]), angvel=np.concatenate([pr["angvel"], z]))


def test_cheirality_guard_rejects_a_step_that_loses_measurements():
    T, L = 2, 6
    pr = _guard_problem(L)
    params = dict(lm_ref.PARAMS, rel_tol=0.0, abs_tol=0.0, max_iters=8)
    ref = _ref(pr, T, L, params)
    first = ref["log"][1][0]
    # the guard, not the cost test: the trial's cost (its lost measurements skipped) is LOWER
    assert not first["accept"] and first["why"] == "cheirality" and first["cost_lower"]
    assert all(r["margin"] >= MARGIN or r["why"] == "cheirality" for log in ref["log"] for r in log)
    assert any(r["accept"] for r in ref["log"][1])  # damped enough, the step stays in front and is taken
    dev = _dev(pr, T, L, params)
    for k in ("pose", "vel", "angvel", "cost", "lambda"):
        assert np.isfinite(dev[k]).all(), k
    assert dev["cost_hist"][1, 1] == dev["cost_hist"][1, 0]  # rejected on the device too
    _assert_matches(dev, ref, T, "cheirality guard")
    assert (dev["lin"]["status"].cpu().numpy() == 0).all()


# ---------------------------------------------------------------- nvalid
def test_partly_filled_window_matches_reference():
    """Only the last 2 of 6 frames measured (the streaming window before it has filled)."""
    T, L = 3, 6
    pr = lm_ref.problem(T, L, 0.1)
    nv = [2, 2, 2]
    ref = _ref(pr, T, L, lm_ref.PARAMS, nvalid=nv)
    assert (ref["status"] == lm_ref.CONVERGED).all()
    assert all(r["margin"] >= MARGIN for log in ref["log"] for r in log)
    dev = _dev(pr, T, L, lm_ref.PARAMS, nvalid=nv)
    _assert_matches(dev, ref, T, "nvalid = 2")
    st = dev["lin"]["status"].cpu().numpy().reshape(T, L, -1)
    assert (st[:, :L - 2] == 2).all() and (st[:, L - 2:] == 0).all()
    rot, tra = lm_ref.pose_errors(dev["pose"].reshape(T, L, 12)[:, -2:], pr["truth"].reshape(T, L, 12)[:, -2:])
    assert rot.max() < ROT_TOL and tra.max() < TRA_TOL  # the measured frames


# ---------------------------------------------------------------- independence, early exit, large T
def _slice(pr, t, L):
    return {k: v[t * L:(t + 1) * L] for k, v in pr.items()}


def _assert_same_bits(a, b, ta, tb, L, what):
    for k in ("pose", "vel", "angvel"):
        np.testing.assert_array_equal(a[k][ta * L:(ta + 1) * L], b[k][tb * L:(tb + 1) * L], err_msg=f"{what} {k}")
    for k in ("cost0", "cost", "iters", "status", "lambda", "cost_hist"):
        np.testing.assert_array_equal(a[k][ta], b[k][tb], err_msg=f"{what} {k}")


def test_trajectories_are_independent_and_exit_early():
    """T = 5: trajectories 0-3 start at the truth (they stop after a step or two and their
    workgroups return at once from then on), trajectory 4 starts 0.8 rad off; its outputs are
    bit for bit those of the T = 1 solve of it alone."""
    T, L = 5, 6
    pr = lm_ref.problem(T, L, 0.8)
    _, w, v = lm_ref.truth(T, L)
    for k in ("pose", "vel", "angvel"):
        pr[k] = pr[k].reshape(T, L, -1).copy()
    pr["pose"][:4] = pr["truth"].reshape(T, L, 12)[:4]
    pr["vel"][:4] = v[:4, None]
    pr["angvel"][:4] = w[:4, None]
    for k in ("pose", "vel", "angvel"):
        pr[k] = pr[k].reshape(T * L, -1)
    dev = _dev(pr, T, L, lm_ref.PARAMS)
    print("iters", dev["iters"], "status", dev["status"])
    assert (dev["iters"][:4] <= 2).all() and (dev["status"][:4] == _lib.LM_CONVERGED).all()
    assert dev["iters"][4] > 2 and dev["status"][4] == _lib.LM_CONVERGED
    one = _dev(_slice(pr, 4, L), 1, L, lm_ref.PARAMS)
    _assert_same_bits(dev, one, 4, 0, L, "trajectory 4")


def test_more_trajectories_than_cus():
    """T = CUs + 1, L = 2: one workgroup per trajectory whatever the CU count."""
    T, L = torch.cuda.get_device_properties(0).multi_processor_count + 1, 2
    pr = lm_ref.problem(T, L, 0.1)
    dev = _dev(pr, T, L, lm_ref.PARAMS)
    assert (dev["status"] == _lib.LM_CONVERGED).all(), np.unique(dev["status"], return_counts=True)
    rot, tra = lm_ref.pose_errors(dev["pose"], pr["truth"])
    assert rot.max() < ROT_TOL and tra.max() < TRA_TOL
    one = _dev(_slice(pr, T - 1, L), 1, L, lm_ref.PARAMS)
    _assert_same_bits(dev, one, T - 1, 0, L, f"trajectory {T - 1}")


# ---------------------------------------------------------------- determinism, graph
def test_deterministic_and_graph_replay():
    T, L = 3, 6
    pa, pb = lm_ref.problem(T, L, 0.8), lm_ref.problem(T, L, 0.8, seed=9)
    a1, a2 = _dev(pa, T, L, lm_ref.PARAMS), _dev(pa, T, L, lm_ref.PARAMS)
    for t in range(T):
        _assert_same_bits(a1, a2, t, t, L, "two eager runs")
    eager_b = _dev(pb, T, L, lm_ref.PARAMS)
    # a plan over persistent tensors, captured once, replayed on re-seeded inputs
    dev = torch.device("cuda")
    y = torch.as_tensor(pa["y"], device=dev)
    P, V, W = (torch.as_tensor(pa[k], device=dev) for k in ("pose", "vel", "angvel"))
    args, lin = pipeline.prepare_trajectories(y, P, V, W, synth.CUBE_CORNERS, synth.CAMERA_K, T=T, L=L, dt=lm_ref.DT,
                                              proj_sigmas=[SIG["proj"]] * 2, dyn_sigmas=[SIG["dyn"]] * 6,
                                              cv_sigmas=[SIG["cv"]] * 3)
    assert lin["_keep"][1].data_ptr() == P.data_ptr()  # solved in place
    plan = pipeline.LMPlan(args, lin, T=T, L=L, **lm_ref.PARAMS)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.launch()
    for src in (pa, pb):
        y.copy_(torch.as_tensor(src["y"]))
        for t_, k in ((P, "pose"), (V, "vel"), (W, "angvel")):
            t_.copy_(torch.as_tensor(src[k]))
        g.replay()
        torch.cuda.synchronize()
        got = {k: plan.out[k].cpu().numpy() for k in plan.out}
        got.update(pose=P.cpu().numpy(), vel=V.cpu().numpy(), angvel=W.cpu().numpy())
        want = a1 if src is pa else eager_b
        for t in range(T):
            _assert_same_bits(got, want, t, t, L, "graph replay")


# ---------------------------------------------------------------- the newest frame pending
def test_pending_newest_frame_matches_reference():
    """pa_window_lm_solve(newest_pending): the window the split tick's pre half leaves, whose
    newest slot holds stale keypoints.  Frame L-1's projection factors carry status 3 and stay
    out of the cost and the step (lm_ref with the same mask), whatever the slot holds."""
    T, L = 3, 6
    pr = lm_ref.problem(T, L, 0.1)
    y = pr["y"].reshape(T, L, -1).copy()
    y[:, -1] = y[:, 0]  # stale: the oldest frame's keypoints
    pr["y"] = y.reshape(T * L, -1)
    ref = _ref(pr, T, L, lm_ref.PARAMS, pending=True)
    assert (ref["status"] == lm_ref.CONVERGED).all()
    assert all(r["margin"] >= MARGIN for log in ref["log"] for r in log)
    dev = _dev(pr, T, L, lm_ref.PARAMS, pending=True)
    _assert_matches(dev, ref, T, "newest frame pending")
    st = dev["lin"]["status"].cpu().numpy().reshape(T, L, -1)
    assert (st[:, -1] == 3).all() and (st[:, :-1] == 0).all()
    rot, tra = lm_ref.pose_errors(dev["pose"].reshape(T, L, 12)[:, :-1], pr["truth"].reshape(T, L, 12)[:, :-1])
    assert rot.max() < ROT_TOL and tra.max() < TRA_TOL  # the measured frames
    y[:, -1] = 0.0  # other stale values: the same bits
    pr["y"] = y.reshape(T * L, -1)
    other = _dev(pr, T, L, lm_ref.PARAMS, pending=True)
    for t in range(T):
        _assert_same_bits(dev, other, t, t, L, "stale keypoints")


# ---------------------------------------------------------------- streaming
@pytest.fixture(scope="module")
def model():
    from perseus_amd.detector import KeypointCNN

    m = KeypointCNN(num_channels=4)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synthetic_state_dict(0).items()})
    return m


@pytest.mark.parametrize("pre_ahead", [False, True])
def test_streaming_solve_window(model, pre_ahead):
    """A camera window reset to a pose 0.8 rad off: after the first tick solve_window reports
    CONVERGED on every camera and the window's measured frame is at the truth; then EVERY
    following (unchanged, one fixed-lambda step) tick is checked.

    From the second tick on: the issue's bounds, 1e-4 rad / 1e-5 m.  The first tick after the
    solve cannot meet them, with or without this change: one measured frame leaves vel and angvel
    unobservable (they stay zero), so that tick linearizes at a prediction one frame of true
    motion off (theta = dt |w| = 1.2e-2 .. 1.6e-2 rad, d = dt |v| = 6e-4 .. 7e-4 m for these
    trajectories) and takes ONE Gauss-Newton step, whose error is second order in theta.  Its
    bound here is that prediction error itself, per camera: the step must not leave the pose
    farther from the truth than where it started.  Measured on an MI355X (max over cameras), ticks
    1, 2, 3, 4: 2.9e-4, 3.5e-5, 3.6e-6, 3.8e-7 rad and 3.0e-5, 9.9e-7, 1.4e-7, 6.4e-8 m, then
    <= 4.2e-7 rad / 1.2e-7 m on every tick (the f32 keypoints' floor); pre_ahead: 2.7e-4, 3.3e-5,
    3.4e-6, 3.6e-7 rad and 2.8e-5, 1.1e-6, 1.5e-7, 6.5e-8 m, then the same floor.

    pre_ahead: the window between ticks is the next tick's (frame L-1 predicted, no keypoints):
    the solve leaves that frame's projections out and the pre half's reduction is redone, which
    on an unchanged window rewrites the tick workspace bit for bit."""
    from perseus_amd.streaming import StreamingPipeline

    n, Lw, ticks = 3, 6, 40
    truth, w, v = lm_ref.truth(n, ticks)
    init = lm_ref.problem(n, 1, 0.8)["pose"]
    p = StreamingPipeline(model, graph=True, pose_window=Lw, init_pose=init, init_vel=np.zeros((n, 3)),
                          init_angvel=np.zeros((n, 3)), proj_sigma=SIG["proj"], dyn_sigma=SIG["dyn"],
                          cv_sigma=SIG["cv"], lam=1e-2, pre_ahead=pre_ahead)
    assert p.pre_ahead == pre_ahead
    p.reset_window()
    p.tick_keypoints(lm_ref.keypoints(truth[0]))
    if pre_ahead:
        p.stream.synchronize()
        before = p.tick_ws.clone()
        with torch.cuda.stream(p.stream):
            pipeline.window_pose_tick_reduce(p.traj_args, p.tick_ws, lam=p.gn.lam)
        p.stream.synchronize()
        assert torch.equal(before, p.tick_ws)
    res = p.solve_window(max_iters=30)
    print("solve_window:", res)
    assert (res["status"] == _lib.LM_CONVERGED).all(), res
    assert (res["cost"] < res["cost0"]).all()
    measured = -2 if pre_ahead else -1  # (pre_ahead: the window is already advanced for the next tick)
    rot, tra = lm_ref.pose_errors(p.window_state()["pose"][:, measured], [F.pack(T) for T in truth[0]])
    print(f"after solve_window: measured frame {rot.max():.3g} rad, {tra.max():.3g} m")
    assert rot.max() < ROT_TOL and tra.max() < TRA_TOL
    theta, d = lm_ref.DT * np.linalg.norm(w, axis=1), lm_ref.DT * np.linalg.norm(v, axis=1)
    err_r, err_t = [], []
    for k in range(1, ticks):
        pose, info = p.tick_keypoints(lm_ref.keypoints(truth[k]))
        assert (info == 0).all(), (k, info)
        rot, tra = lm_ref.pose_errors(pose, [F.pack(T) for T in truth[k]])
        err_r.append(rot.max())
        err_t.append(tra.max())
        if k == 1:
            assert (rot <= theta).all() and (tra <= d).all(), (rot, theta, tra, d)
        else:
            assert rot.max() < ROT_TOL and tra.max() < TRA_TOL, (k, rot, tra)
    print("rotation error (rad) per tick:", " ".join(f"{e:.1e}" for e in err_r))
    print("translation error (m) per tick:", " ".join(f"{e:.1e}" for e in err_t))
    p.close()


def test_solve_window_limits(model):
    """Windows above the cyclic-reduction range run the four-launch tick but have no LM solve."""
    from perseus_amd.streaming import StreamingPipeline

    p = StreamingPipeline(model, graph=False, pose_window=pipeline.TICK_MAX_L + 1)
    with pytest.raises(ValueError, match="pose_window 25"):
        p.solve_window()
    p.close()
    q = StreamingPipeline(model, graph=False)
    with pytest.raises(RuntimeError, match="pose stage"):
        q.solve_window()
    q.close()


