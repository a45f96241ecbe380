"""pa_window_pose_tick_pre + _post (the split streaming tick, csrc/pose_tick.hip) against
pa_window_pose_tick (the fused tick, itself bit-identical to the four separate calls) at every
level structure of the ROOT-order cyclic reduction: L = 2 .. 24 (even and odd level counts,
the n = 3 -> 2 -> 1 tail), n_kp = 8 (the RP = 34 instance) and 16 (the general one), windows
whose first frames are unmeasured (nvalid = L - 2: status-2 rows).  Same inputs, three ticks
each: info equal, the split delta solves the damped normal equations of its factors (the dense
oracle's backward error, oracle/gn_ref.py) and agrees with the fused delta within
max(1e-9, 100 cond eps) (another elimination order in f64; the random windows are not all well
conditioned), statuses and the window's keypoints equal."""
import numpy as np
import pytest
import torch

from oracle import gn_ref as G
from perseus_amd import pipeline, synth

pytestmark = pytest.mark.gpu


def _setup(L, nk, seed):
    T = 3
    dev = torch.device("cuda", 0)
    tr = synth.synthetic_trajectories(seed, T, L, n_kp=nk)
    nvalid = torch.full((T,), max(L - 2, 1), dtype=torch.int32, device=dev)
    y = torch.as_tensor(tr["y"], device=dev)
    corners = np.asarray(tr["corners"])
    if len(corners) < nk:  # (the synthetic set has the 8 cube corners: 8 more inside the cube)
        corners = np.concatenate([corners, 0.5 * corners])[:nk]
    a, lin = pipeline.prepare_trajectories(y, tr["poses"], tr["vels"], tr["angvels"], corners, tr["K"], T=T,
                                           L=L, dt=1 / 30, proj_sigmas=[2.0, 2.0], dyn_sigmas=[0.1] * 6,
                                           cv_sigmas=[0.5] * 3, nvalid=nvalid)
    out = dict(delta=torch.zeros((T * L, 12), dtype=torch.float64, device=dev),
               info=torch.zeros(T, dtype=torch.int32, device=dev),
               newest=torch.zeros((T, 12), dtype=torch.float64, device=dev))
    return a, lin, out, tr


@pytest.mark.parametrize("nk", [8, 16])
@pytest.mark.parametrize("L", [2, 3, 4, 5, 7, 12, 13, 23, 24])
def test_split_tick_matches_fused(L, nk):
    fa, flin, fout, tr = _setup(L, nk, 100 + L)
    sa, slin, sout, _ = _setup(L, nk, 100 + L)
    ws = pipeline.window_pose_tick_workspace(3, L, torch.device("cuda", 0))
    rng = np.random.default_rng(L)
    for k in range(3):
        y_new = torch.as_tensor((tr["y"][:3] + 0.01 * rng.standard_normal(tr["y"][:3].shape)).astype(np.float32),
                                device="cuda").contiguous()
        pipeline.window_pose_tick(fa, y_new, lam=1e-2, **fout)
        pipeline.window_pose_tick_pre(sa, ws, lam=1e-2)
        pipeline.window_pose_tick_post(sa, y_new, ws, **sout)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(sout["info"].cpu().numpy(), fout["info"].cpu().numpy())
        assert (fout["info"] == 0).all()
        # the split step solves the damped normal equations of its own factors (dense oracle,
        # backward error), and agrees with the fused step (a wrong elimination order or a lost
        # factor shows as O(delta))
        lin = {kk: (v.transpose(1, 2) if kk.startswith("j_") else v).cpu().numpy() for kk, v in slin.items()
               if isinstance(v, torch.Tensor)}
        H, g, _ = G.gn_step(lin, 3, L, nk, 1e-2)
        ds = sout["delta"].cpu().numpy().reshape(3, -1)
        df = fout["delta"].cpu().numpy().reshape(3, -1)
        for t in range(3):
            M = H[t] + 1e-2 * np.eye(H.shape[1])
            res = M @ ds[t] + g[t]
            assert np.abs(res).max() <= 1e-10 * (np.abs(M).max() * np.abs(ds[t]).max() + np.abs(g[t]).max()), (k, t)
            # forward agreement within the f64 bound for the conditioning of this system
            tol = max(1e-9, 100 * np.linalg.cond(M) * np.finfo(np.float64).eps)
            assert np.abs(ds[t] - df[t]).max() <= tol * np.abs(df[t]).max(), (k, t)
        assert torch.equal(slin["status"], flin["status"]), (k, L)
        assert torch.equal(slin["_keep"][0], flin["_keep"][0])  # the window's keypoints
        # the fused tick ran on its own window, which has drifted by the earlier ticks' rounding:
        # from here on the split tick continues from the fused tick's state
        for i in (1, 2, 3):  # pose, vel, angvel of the window
            slin["_keep"][i].copy_(flin["_keep"][i])


def _setup_rows(tr, t0, t1, L, nk):
    """prepare_trajectories over trajectories t0 .. t1 - 1 of `tr` (one set of synthetic
    windows sliced, so a small launch sees exactly the bytes a large one does)."""
    dev = torch.device("cuda", 0)
    T = t1 - t0
    r = slice(t0 * L, t1 * L)
    nvalid = torch.full((T,), L - 2, dtype=torch.int32, device=dev)
    y = torch.as_tensor(tr["y"][r], device=dev)
    a, lin = pipeline.prepare_trajectories(y, tr["poses"][r], tr["vels"][r], tr["angvels"][r], tr["corners"],
                                           tr["K"], T=T, L=L, dt=1 / 30, proj_sigmas=[2.0, 2.0],
                                           dyn_sigmas=[0.1] * 6, cv_sigmas=[0.5] * 3, nvalid=nvalid)
    out = dict(delta=torch.zeros((T * L, 12), dtype=torch.float64, device=dev),
               info=torch.zeros(T, dtype=torch.int32, device=dev),
               newest=torch.zeros((T, 12), dtype=torch.float64, device=dev))
    return a, lin, out


def test_ticks_with_more_trajectories_than_cus():
    """the tick entry points take any T (one workgroup per trajectory, no grid-level
    sync).  At T = CUs + 1, over three ticks: the fused tick (pa_window_pose_tick) and the split
    tick (pre + post) give the first and the last three trajectories exactly the bits the same
    windows get in T = 3 launches (no trajectory depends on how many others run, or on which CU
    round it lands in), and the fused tick agrees with the four separate launches (cyclic
    reduction forced: pa_debug_gn_set_assemblers(64), the fused tick's GN form) on every
    trajectory -- info equal, delta to f64 rounding at the first tick (later ticks: see below).  (On these random windows the fused
    tick's projection factors differ from pa_trajectory_linearize's in the last bits on a few
    trajectories -- two kernels, two FMA contractions -- so delta is compared to 1e-10 of its
    scale, not bit for bit; on the streaming windows the two are bit-identical,
    tests/test_streaming_pose_gpu.py.)"""
    from perseus_amd import _lib

    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    T, L, nk = ncu + 1, 24, 8
    tr = synth.synthetic_trajectories(31, T, L, n_kp=nk)
    fa, flin, fout = _setup_rows(tr, 0, T, L, nk)
    qa, qlin, qout = _setup_rows(tr, 0, T, L, nk)
    sa, slin, sout = _setup_rows(tr, 0, T, L, nk)
    fsubs = [(t0, _setup_rows(tr, t0, t0 + 3, L, nk)) for t0 in (0, T - 3)]
    ssubs = [(t0, _setup_rows(tr, t0, t0 + 3, L, nk)) for t0 in (0, T - 3)]
    keep = qlin["_keep"]
    win = {"y": keep[0].view(T, L, 2 * nk), "pose": keep[1].view(T, L, 12), "vel": keep[2].view(T, L, 3),
           "angvel": keep[3].view(T, L, 3)}
    plan = pipeline.GNPlan(qlin, T=T, L=L, lam=1e-2)
    plan.out["delta"], plan.out["info"] = qout["delta"], qout["info"]
    ws = pipeline.window_pose_tick_workspace(T, L, torch.device("cuda", 0))
    ws3 = pipeline.window_pose_tick_workspace(3, L, torch.device("cuda", 0))
    rng = np.random.default_rng(5)
    L_ = _lib.lib()
    for k in range(3):
        y_new = torch.as_tensor((tr["y"].reshape(T, L, -1)[:, -1] + 0.01 * rng.standard_normal((T, 2 * nk)))
                                .astype(np.float32), device="cuda").contiguous()
        pipeline.window_pose_tick(fa, y_new, lam=1e-2, **fout)
        for t0, (a3, _, o3) in fsubs:
            pipeline.window_pose_tick(a3, y_new[t0:t0 + 3].contiguous(), lam=1e-2, **o3)
        _lib.check(L_.pa_debug_gn_set_assemblers(64), "force cyclic reduction")
        try:
            pipeline.window_advance(y_new, win, dt=1 / 30, nvalid=keep[10])
            pipeline.launch(qa, torch.device("cuda", 0))
            plan.launch()
            pipeline.window_retract(win, qout["delta"], qout["info"], newest=qout["newest"])
            torch.cuda.synchronize()
        finally:
            L_.pa_debug_gn_set_assemblers(0)
        pipeline.window_pose_tick_pre(sa, ws, lam=1e-2)
        pipeline.window_pose_tick_post(sa, y_new, ws, **sout)
        for t0, (a3, _, o3) in ssubs:
            pipeline.window_pose_tick_pre(a3, ws3, lam=1e-2)
            pipeline.window_pose_tick_post(a3, y_new[t0:t0 + 3].contiguous(), ws3, **o3)
        torch.cuda.synchronize()

        def same(a, b):  # bit for bit, an unsolved trajectory's NaN delta equal to itself
            return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))

        for big, subs in ((fout, fsubs), (sout, ssubs)):
            for t0, (_, _, o3) in subs:
                assert same(big["delta"][t0 * L:(t0 + 3) * L], o3["delta"]), (k, t0)
                assert torch.equal(big["info"][t0:t0 + 3], o3["info"]), (k, t0)
                assert same(big["newest"][t0:t0 + 3], o3["newest"]), (k, t0)
        # tick 0 starts the fused and the four-launch chains from the same windows: info equal and
        # delta to f64 rounding; later ticks start from windows that carry the last-bit differences
        # of the two factor kernels through the retract, and these random (not conditioned) windows'
        # solves amplify them (8.8e-8 of the scale at tick 1, r06b) or, rarely, fail a pivot in one
        # chain only: 1e-6 of the scale there, on the trajectories both chains solved
        fi, qi = fout["info"], qout["info"]
        if k == 0:
            assert torch.equal(fi, qi)
        else:
            assert int((fi != qi).sum()) <= max(2, T // 100), k
        assert int((fi == 0).sum()) >= T // 2
        ok = (fi == 0) & (qi == 0)  # (an unsolved trajectory's delta is NaN)
        df, dq = fout["delta"].view(T, -1)[ok], qout["delta"].view(T, -1)[ok]
        tol = 1e-10 if k == 0 else 1e-6
        assert (df - dq).abs().max().item() <= tol * df.abs().max().item(), k
        # the split tick (another elimination order) on its own window: the same solvability at
        # tick 0; after that its window evolves on its own (these random windows are not
        # conditioned: an unsolved tick leaves a window unretracted in one form only -- 1 to 7 of
        # 257 differ by tick 2, r06c / r06e), and the split-vs-fused equivalence is
        # test_split_tick_matches_fused's, on conditioned windows
        if k == 0:
            np.testing.assert_array_equal(sout["info"].cpu().numpy(), fout["info"].cpu().numpy())
        # the four-launch window continues from the fused tick's (they drift by rounding)
        for i in (1, 2, 3):
            qlin["_keep"][i].copy_(flin["_keep"][i])
