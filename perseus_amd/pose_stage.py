"""The streaming pose stage: a fixed-lag smoother over the last L frames of each of n cameras,
driven by normalized keypoints (the detector's output convention), with no model anywhere.

The window is built from the reference's own factors (perseus/smoother/factors.py:
KeypointProjectionFactor :182-275 per keypoint, PoseDynamicsFactor :8-142 and ConstantVelocityFactor
:145-171 per frame pair); the reference stops at pixels, so this build defines the loop: one damped
Gauss-Newton step per tick.  A tick is the sequence pa_window_advance_n (the window shifts one frame,
the new keypoints appended, the new pose predicted by the dynamics model, the count of real frames
+ 1) -> pa_trajectory_linearize (whitened factors of every camera's window; frames not yet filled by
a real tick carry no projection factors) -> pa_trajectory_gn_step (delta and info only) ->
pa_window_retract_newest (pose Exp(delta), velocities += delta, newest poses out), in one of three
forms: the split tick for windows <= 24 frames (pa_window_pose_tick_pre: all of it that does not
need the new keypoints; pa_window_pose_tick_post once they are there), the fused tick
(pa_window_pose_tick's two launches) and the four separate launches (bit for bit the fused form;
windows above 24 frames).  PoseStage.enqueue_pre / enqueue_post / enqueue put a tick on the current
stream and are the one place that fixes the order of its optional pieces; StreamingPipeline calls
them beside the detector's forward, PoseStage.tick_keypoints drives the stage alone.  Every buffer
is allocated at construction, so the ticks can be captured in a HIP graph.
"""

from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import torch

from . import _lib, pipeline, synth


def capture(stream, enqueue) -> torch.cuda.CUDAGraph:
    """What enqueue() puts on `stream`, captured as one HIP graph."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        enqueue()
    return g


def mapped_address(pinned: torch.Tensor) -> int:
    """The device address of a pinned host tensor (zero-copy reads and writes over PCIe)."""
    dp = C.c_void_p()
    _lib.check(_lib.lib().pa_host_device_pointer(C.c_void_p(pinned.data_ptr()), C.byref(dp)), "host_device_pointer")
    return dp.value


class PoseStage:
    """The fixed-lag smoother of n windows of L frames and n_kp keypoints (module docstring).  Its
    parameters: K (fx, fy, s, u0, v0) of the H x W image and the body-frame corners (defaults: the
    datagen camera and cube, synth.CAMERA_K / CUBE_CORNERS); dt = the camera period;
    sigmas of the diagonal noise models (pixels, dynamics tangent, velocity); lam = the
    LM damping; init_pose (n, 12) / init_vel / init_angvel fill every frame of the
    initial window (default: the cube 0.4 m in front of each camera, at rest);
    proj_robust = None, ("huber", k) or ("cauchy", k): GTSAM's noiseModel.Robust on the keypoint
    factors (pipeline.prepare_trajectories), so that a keypoint tens of pixels off, an occluded
    corner, is down-weighted in every tick form, solve_window() and window_covariance().
    marginalize=True: the fixed-lag smoother proper (GTSAM's BatchFixedLagSmoother): the frame a
    tick drops is not forgotten but marginalized, its factors' Schur complement carried as a
    linear prior on the oldest frame (pipeline.PriorPlan, self.prior).  Each tick then runs, inside
    the same graph: the last tick's new prior becomes the current one (one device copy),
    pa_window_prior_linearize at frame 1 of the un-advanced window (the frame about to become
    the oldest), the tick in whatever form it uses with the prior on frame 0, and
    pa_window_marginalize with the tick's delta and info.  self.prior.minfo (device, int32) is 2
    until the window has filled, then 0.  Not with pre_ahead (between ticks the factor outputs
    already belong to the next tick): ValueError.  solve_window(with_prior=True) is the
    Levenberg-Marquardt solve of such a window with its prior; without the keyword it raises.
    timed=True: real timestamps (cameras skip frames, so consecutive frames are 1, 2 or 3 periods
    apart; one of the batched cameras has no frame; a hand hides single corners).  The window
    carries two rings beside its frames, self.win["dt"] (n, L-1) f64, the period of every frame
    pair (initially dt), and self.win["mask"] (n, L) int32, one bit per keypoint (initially all
    ones); pa_traj_args.dt_pair / kp_mask point at them, so every factor, solve_window() and
    window_covariance() use them.  tick_keypoints() (and StreamingPipeline.tick()) take stamps=,
    present= and kp_mask=; the new pair's dt and the new frame's mask go through one small pinned
    block [dt_new (n) f64 | mask_new (n) u32] that the graph copies to the device on the stream that
    runs the advance (timed_zero_copy: read in place), so one captured graph serves every tick.  Not
    with pre_ahead.
    angvel_sigma (rad/s; None = off): the ConstantVelocityFactor on the ANGULAR velocity of every
    frame pair (pipeline.prepare_trajectories cw_sigmas, pa_traj_args.r_cw), as GTSAM users put the
    reference's factor on the angular-velocity keys: successive angular velocities are coupled, so a
    frame without keypoints keeps an observable rotation.  It travels in the window's pa_traj_args
    and factor outputs: every tick form, solve_window(), window_covariance(), marginalize=True and
    timed=True honour it.
    gate_chi2 (None = off; needs timed=True, else ValueError): the chi-square gate that fills in
    kp_mask.  Every tick, inside the captured graph: the window's marginals with their cross blocks
    (pipeline.MarginalsPlan over the factor outputs as they stand when the tick starts: the last
    tick's linearization, the one window_covariance() reports, with the tick's lam, the prior and the
    factor on the angular velocity where they are on), pa_window_predict to this tick's dt_new with one
    factor's worth of process noise (dyn_sigma^2 on the pose, angvel_sigma^2 or 0, cv_sigma^2), and
    pa_keypoint_gate on the tick's keypoints: a corner whose innovation exceeds gate_chi2 (13.816
    = the 0.999 quantile at 2 degrees of freedom) loses its bit.  The effective mask, the staged one
    AND the gate, is what the tick sees and what lands in win["mask"][:, -1].  The gate abstains while
    the window holds fewer than gate_min_frames real frames, while the covariance is not finite, and
    when fewer than gate_min_pass corners pass (a lost track must be able to recover); gate_state()
    reports d2, ginfo and the effective mask.  With the gate on, dt_new / mask_new are copied to the
    device every tick (not read zero-copy), because the fused tick's gate writes the copy.  The
    covariance is taken at the last tick's linearization point while the state is the retracted one,
    as window_covariance()'s is.  The gate is only as sharp as the model's own noise: with dyn_sigma =
    0.1 the prediction is uncertain by about 0.1 m and a corner 40 px off passes; gating such corners
    needs a dyn_sigma of a few mm / mrad.  That is a property of the model, not a defect of the gate.
    predict(taus): the newest pose with its covariance at horizons after the newest frame.
    split_pose: the split tick where the window allows it (self.split_pose): everything but the newest
    frame's projection factors can run beside whatever produces the keypoints.  pre_ahead: the pre half
    of tick k + 1 runs right after tick k's results are on the host (in the gap before the next camera
    frames), so a tick's latency path is the post half alone (self.pre_ahead; without the split tick
    a RuntimeWarning, and the full-latency tick).

    Where a tick's info (n,) int32 and newest poses (n, 12) f64 land: a block laid out [info | pad to
    8 B | poses], pinned (out_h, what the host reads: self.info_h / self.pose_h) and on the device
    (out_d, what the fused and four-launch forms write).  out_mapped = the device address of out_h:
    the split tick's post half then writes the pinned block in place (None: it writes out_d too);
    flush() enqueues whatever copy brings out_d's results to out_h.  StreamingPipeline passes the
    tail of its own output block and its own copy.  out_h=None is the stand-alone stage: it
    allocates the block, a stream (unless given) and the pinned keypoint block, runs one warm-up
    tick and resets; tick_keypoints() (graph=True: captured on first use) then drives it."""

    def __init__(self, n: int, L: int, n_kp: int, *, device=None, H: int = 256, W: int = 256, K=None, corners=None,
                 dt: float = 1.0 / 30.0, vel_frame: str = "world", proj_sigma: float = 1.0, dyn_sigma: float = 0.1,
                 cv_sigma: float = 0.1, lam: float = 1e-2, init_pose=None, init_vel=None, init_angvel=None,
                 proj_robust=None, marginalize: bool = False, timed: bool = False, angvel_sigma: float | None = None,
                 gate_chi2: float | None = None, gate_min_pass: int = 4, gate_min_frames: int = 3,
                 split_pose: bool = True, pre_ahead: bool = False, graph: bool = True, stream=None, out_h=None,
                 out_d=None, out_mapped: int | None = None, flush=None, timed_zero_copy: bool = False):
        self.check_args(L, timed=timed, marginalize=marginalize, pre_ahead=pre_ahead, gate_chi2=gate_chi2,
                        gate_min_pass=gate_min_pass)
        n, Lw, nk = int(n), int(L), int(n_kp)
        if Lw < 2:
            raise ValueError("pose_window must be >= 2 frames (the dynamics factors couple frame pairs)")
        pipeline._vel_code(vel_frame)  # (AssertionError, as factors.py:41)
        dev = torch.device(device or torch.device("cuda", torch.cuda.current_device()))
        self.n, self.L, self.n_kp, self.dev, self.H, self.W = n, Lw, nk, dev, int(H), int(W)
        self.dt, self.vel_frame = float(dt), vel_frame
        self.angvel_sigma = None if angvel_sigma is None else float(angvel_sigma)
        self.gate_chi2 = None if gate_chi2 is None else float(gate_chi2)
        self.timed, self.marginalize = bool(timed), bool(marginalize)
        alone = out_h is None
        self.stream = torch.cuda.Stream(dev) if stream is None else stream
        po = (n * 4 + 7) // 8 * 8
        if alone:  # its own block, and the copy the fused and four-launch forms need
            out_h = torch.zeros(po + n * 12 * 8, dtype=torch.uint8).pin_memory()
            out_d = torch.zeros(po + n * 12 * 8, dtype=torch.uint8, device=dev)
            out_mapped = mapped_address(out_h)
            flush = lambda: None if self.split_pose else out_h.copy_(out_d, non_blocking=True)  # noqa: E731
        self._flush = flush
        self.info_h, self.pose_h = out_h[:n * 4].view(torch.int32), out_h[po:].view(torch.float64).view(n, 12)
        self.info_d, self.pose_d = out_d[:n * 4].view(torch.int32), out_d[po:].view(torch.float64).view(n, 12)
        self.y = torch.empty((n, 2 * nk), dtype=torch.float32, device=dev)
        self.y_h = torch.zeros((n, 2 * nk), dtype=torch.float32).pin_memory()  # tick_keypoints' input
        K = synth.CAMERA_K if K is None else np.asarray(K, np.float64)
        corners = synth.CUBE_CORNERS[:nk] if corners is None else np.asarray(corners, np.float64)
        if init_pose is None:
            init_pose = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0.4], np.float64), (n, 1))
        zeros = np.zeros((n, 3))
        self._init = {"pose": np.asarray(init_pose, np.float64).reshape(n, 12),
                      "vel": np.asarray(zeros if init_vel is None else init_vel, np.float64).reshape(n, 3),
                      "angvel": np.asarray(zeros if init_angvel is None else init_angvel, np.float64).reshape(n, 3)}
        f64 = dict(dtype=torch.float64, device=dev)
        self.win = {"y": torch.zeros((n, Lw, 2 * nk), dtype=torch.float32, device=dev),
                    "pose": torch.empty((n, Lw, 12), **f64), "angvel": torch.empty((n, Lw, 3), **f64),
                    "vel": torch.empty((n, Lw, 3), **f64)}
        # real frames per window (from its end): the others are the initial state, with no projection factor
        self.nvalid = torch.zeros(n, dtype=torch.int32, device=dev)
        rings = {}
        if self.timed:
            # the rings, and the tick's [dt_new (n) f64 | mask_new (n) u32] block, pinned, with its device copy
            self.win["dt"] = torch.full((n, Lw - 1), self.dt, **f64)
            self.win["mask"] = torch.full((n, Lw), -1, dtype=torch.int32, device=dev)
            rings = dict(dt_pair=self.win["dt"], kp_mask=self.win["mask"])
            self.tm_h = torch.zeros(n * 12, dtype=torch.uint8).pin_memory()
            self.tm_d = torch.zeros(n * 12, dtype=torch.uint8, device=dev)
            self.dt_new_h = self.tm_h[:n * 8].view(torch.float64)
            self.mask_new_h = self.tm_h[n * 8:].view(torch.int32)
            self.dt_new_h.fill_(self.dt)
            self.mask_new_h.fill_(-1)
            self._stamps = None  # the last tick's stamps (None: the next tick uses the nominal dt)
        self.traj_args, self.lin = pipeline.prepare_trajectories(
            self.win["y"].view(n * Lw, 2 * nk), self.win["pose"].view(n * Lw, 12), self.win["vel"].view(n * Lw, 3),
            self.win["angvel"].view(n * Lw, 3), corners, K, T=n, L=Lw, dt=self.dt, vel_frame=vel_frame, H=self.H,
            W=self.W, proj_sigmas=[proj_sigma] * 2, dyn_sigmas=[dyn_sigma] * 6, cv_sigmas=[cv_sigma] * 3,
            nvalid=self.nvalid, proj_robust=proj_robust,
            cw_sigmas=None if self.angvel_sigma is None else [self.angvel_sigma] * 3, **rings)
        for k in ("y", "pose", "vel", "angvel"):  # linearize reads the window in place, no staging copy
            assert self.lin["_keep"][("y", "pose", "vel", "angvel").index(k)].data_ptr() == self.win[k].data_ptr()
        self._tm_copy = self.timed and not (timed_zero_copy and self.gate_chi2 is None)
        if self.timed:
            assert self.traj_args.dt_pair == self.win["dt"].data_ptr()
            assert self.traj_args.kp_mask == self.win["mask"].data_ptr()
            # (the gate writes the device copy's masks, so with it the block is never read in place)
            base = self.tm_d.data_ptr() if self._tm_copy else mapped_address(self.tm_h)
            self._tm_ptrs = (base, base + n * 8)
            self.traj_args.dt_new, self.traj_args.mask_new = self._tm_ptrs
        # (the fused / split ticks get the prior beside the pa_traj_args, the four-launch path's GN step from its plan)
        self.prior = pipeline.PriorPlan(T=n, L=Lw, device=dev) if self.marginalize else None
        self.gn = pipeline.GNPlan(self.lin, T=n, L=Lw, lam=lam, prior=self.prior)
        self.gn.out["info"] = self.info_d  # the GN step writes info into the output block
        # pa_window_pose_tick: one workgroup per camera of up to 24 frames, at most one per CU
        self.fused_pose = (Lw <= pipeline.TICK_MAX_L
                           and n <= torch.cuda.get_device_properties(dev).multi_processor_count)
        # the split tick (pa_window_pose_tick_pre / _post): the same limits
        self.split_pose = self.fused_pose and bool(split_pose)
        # pre_ahead: the window and factor outputs between ticks already hold the next tick's advance
        self.pre_ahead = self.split_pose and bool(pre_ahead)
        if pre_ahead and not self.pre_ahead:  # never drop the request silently
            why = ("split_pose=False" if not split_pose else
                   f"pose_window {Lw} > {pipeline.TICK_MAX_L}" if Lw > pipeline.TICK_MAX_L else
                   f"{n} cameras > the device's CUs")
            warnings.warn(f"StreamingPipeline: pre_ahead needs the split pose tick ({why}); running the full-latency "
                          f"tick (self.pre_ahead is False)", RuntimeWarning, stacklevel=3)
        self._post_out = (self.info_d, self.pose_d)
        if self.split_pose and out_mapped is not None:
            # the post half writes info and the newest poses straight into the pinned output block
            # (self.info_h / self.pose_h); nothing writes a device copy, so none is exposed
            self._post_out = (out_mapped, out_mapped + po)
            self.gn.out["info"] = None
        self.tick_ws = pipeline.window_pose_tick_workspace(n, Lw, dev)
        # one factor's worth of process noise, [dyn_sigma^2 x 6 | angvel_sigma^2 or 0 x 3 | cv_sigma^2 x 3]:
        # the graph's dynamics noise is per frame pair, not per second
        sd, sw, sc = float(dyn_sigma), self.angvel_sigma or 0.0, float(cv_sigma)
        self._q_diag = torch.tensor([sd * sd] * 6 + [sw * sw] * 3 + [sc * sc] * 3, dtype=torch.float64, device=dev)
        self._pred = None  # predict()'s plans, built on first use
        self._gate = None
        if self.gate_chi2 is not None:
            # the gate's three launches.  Marginals and prediction read the window and the factor
            # outputs as the tick finds them; the gate itself acts on the new frame's mask word: the
            # ring entry the pre half has landed (split tick: strides L and 12 L, the predicted pose is
            # the advanced window's newest frame), or the device copy of mask_new (fused / four-launch)
            marg = pipeline.MarginalsPlan(self.lin, T=n, L=Lw, lam=lam, cross=True, prior=self.prior)
            self._gate_nvalid = torch.zeros(n, dtype=torch.int32, device=dev)  # nvalid as the tick starts
            pred = pipeline.PredictPlan(self.win, Q=1, marg=marg, q_diag=self._q_diag, vel_frame=vel_frame,
                                        tau=self._tm_ptrs[0])
            _, _, _, _, Cn, Kt, Tc, isp = self.lin["_keep"][:8]
            if self.split_pose:
                tgt = dict(pose_pred=self.win["pose"].data_ptr() + (Lw - 1) * 12 * 8, pose_stride=12 * Lw,
                           mask=self.win["mask"].data_ptr() + (Lw - 1) * 4, mask_stride=Lw)
            else:
                tgt = dict(pose_pred=pred.out["pose"], pose_stride=12, mask=self._tm_ptrs[1], mask_stride=1)
            gate = pipeline.GatePlan(self.y, tgt.pop("pose_pred"), pred.out["cov"], Cn, Kt, isp, tgt.pop("mask"),
                                     chi2=self.gate_chi2, min_pass=int(gate_min_pass),
                                     min_frames=int(gate_min_frames), nvalid=self._gate_nvalid, tcam=Tc, H=self.H,
                                     W=self.W, **tgt)
            self._gate = (marg, pred, gate)
        self._graph_req = bool(graph)
        self.graph = self.pre_graph = None  # tick_keypoints' tick, captured on first use; the pre half's (pre_ahead)
        self._done = torch.cuda.Event()
        if alone:
            with torch.cuda.stream(self.stream):  # eager warm-up (also builds the kernels' first-launch state)
                if self.pre_ahead:
                    self.enqueue_pre()
                self._enqueue_keypoints()
            self.stream.synchronize()
            self.reset()  # the warm-up tick advanced the window (pre_ahead: and prepares the next tick)
            if self._graph_req and self.pre_ahead:
                self.pre_graph = capture(self.stream, self.enqueue_pre)

    @staticmethod
    def check_args(L, *, timed, marginalize, pre_ahead, gate_chi2, gate_min_pass) -> None:
        """The checks between the stage's keywords (L = 0: no window-size check; StreamingPipeline
        runs them before anything else, whatever its pose_window)."""
        if gate_chi2 is not None:
            if not timed:
                raise ValueError("StreamingPipeline: gate_chi2 needs timed=True (the gate writes the keypoint masks)")
            if not (np.isfinite(float(gate_chi2)) and float(gate_chi2) > 0) or int(gate_min_pass) < 0:
                raise ValueError(f"StreamingPipeline: gate_chi2 must be a positive finite number and gate_min_pass "
                                 f">= 0, got {gate_chi2}, {gate_min_pass}")
            if 0 < L < 3:
                raise ValueError("StreamingPipeline: gate_chi2 needs pose_window >= 3 (the prediction's covariance "
                                 "takes frame L-2's angular velocity)")
        if timed and pre_ahead:
            raise ValueError("StreamingPipeline: timed=True cannot run with pre_ahead=True (the next tick's dt is "
                             "not known when its pre half runs)")
        if marginalize and pre_ahead:
            raise ValueError("StreamingPipeline: marginalize=True cannot run with pre_ahead=True (between ticks the "
                             "factor outputs already belong to the next tick)")

    def _enqueue_head(self, gate_y=None):
        """What every tick form starts with, in the order the bit-for-bit tests pin.
        timed: this tick's [dt_new | mask_new] to the device, on the stream that runs the advance and
        before it (one 12 n byte copy; read in place: nothing).
        gate: nvalid before the advance, the marginals of the window as the tick finds it (the last
        tick's linearization and prior, so before the prior moves on and before the tick overwrites
        the factor outputs) and the prediction to this tick's dt_new (after the copy); gate_y (fused /
        four-launch): the gate itself, on the device copy of mask_new, before the advance reads it.
        marginalize: the last tick's new prior becomes the current one, and its gradient at frame 1
        of the un-advanced window, the frame the tick's advance makes the oldest."""
        if self._tm_copy:
            self.tm_d.copy_(self.tm_h, non_blocking=True)
        if self._gate is not None:
            marg, pred, _ = self._gate
            self._gate_nvalid.copy_(self.nvalid)
            marg.launch()
            pred.launch()
            if gate_y is not None:
                self._enqueue_gate(gate_y)
        if self.marginalize:
            self.prior.advance()
            self.prior.linearize(self.win["pose"], self.win["angvel"], self.win["vel"], frame=1)

    def _enqueue_gate(self, y):
        """gate: the keypoints y against the prediction; clears bits of the new frame's mask word
        before the launch that reads it."""
        self._gate[2].y = y
        self._gate[2].launch()

    def _enqueue_prior_out(self, info):
        """marginalize: frame 0 of the tick's linearization becomes the next prior, re-centred at
        the retracted window."""
        if self.marginalize:
            self.prior.marginalize(self.lin, self.win["pose"], self.win["angvel"], self.win["vel"], lam=self.gn.lam,
                                   delta=self.gn.out["delta"], gn_info=info, nvalid=self.nvalid, n_kp=self.n_kp)

    def enqueue_pre(self) -> None:
        """The split tick's pre half: everything that does not need the new keypoints."""
        self._enqueue_head()
        pipeline.window_pose_tick_pre(self.traj_args, self.tick_ws, lam=self.gn.lam, prior=self.prior)

    def enqueue_post(self, y: torch.Tensor) -> None:
        """The split tick's post half, from the keypoints y (n, 2 n_kp) f32 on the device."""
        if self._gate is not None:
            self._enqueue_gate(y)  # (on the ring entry the pre half landed)
        info, newest = self._post_out
        pipeline.window_pose_tick_post(self.traj_args, y, self.tick_ws, delta=self.gn.out["delta"], info=info,
                                       newest=newest)
        self._enqueue_prior_out(info)

    def enqueue(self, y: torch.Tensor) -> None:
        """One tick from the keypoints y (HBM-resident window): advance -> linearize -> GN step ->
        retract, as pa_window_pose_tick_pre + _post (split; pre_ahead: the post half alone),
        pa_window_pose_tick's two launches (fused) or the four separate ones (bit-identical to
        the fused form; windows above 24 frames)."""
        if self.split_pose:
            if not self.pre_ahead:
                self.enqueue_pre()
            self.enqueue_post(y)
            return
        self._enqueue_head(gate_y=y)
        if self.fused_pose:
            pipeline.window_pose_tick(self.traj_args, y, lam=self.gn.lam, delta=self.gn.out["delta"],
                                      info=self.gn.out["info"], newest=self.pose_d, prior=self.prior)
        else:
            tm = dict(dt_new=self._tm_ptrs[0], mask_new=self._tm_ptrs[1]) if self.timed else {}
            pipeline.window_advance(y, self.win, dt=self.dt, vel_frame=self.vel_frame, nvalid=self.nvalid, **tm)
            pipeline.launch(self.traj_args, self.dev)
            self.gn.launch()  # delta, and info straight into the output block
            pipeline.window_retract(self.win, self.gn.out["delta"], self.gn.out["info"], newest=self.pose_d)
        self._enqueue_prior_out(self.gn.out["info"])

    def pre(self) -> None:
        """pre_ahead: the next tick's pre half on the current stream (its graph, once captured)."""
        if self.pre_graph is not None:
            self.pre_graph.replay()
        else:
            self.enqueue_pre()

    def _enqueue_keypoints(self):
        self.y.copy_(self.y_h, non_blocking=True)
        self.enqueue(self.y)
        self._flush()

    def reset(self) -> None:
        """Every frame of every camera's window back to the initial state (keypoints 0, no
        real frame: the next tick's window holds one measured frame)."""
        with torch.cuda.stream(self.stream):
            self.win["y"].zero_()
            self.nvalid.zero_()
            if self.timed:  # the rings back to the nominal dt and all measured; the last stamps forgotten
                self.win["dt"].fill_(self.dt)
                self.win["mask"].fill_(-1)
                self._stamps = None
            if self.prior is not None:
                self.prior.zero()
            for k in ("pose", "vel", "angvel"):
                self.win[k].copy_(torch.as_tensor(self._init[k], device=self.dev)[:, None, :]
                                  .expand_as(self.win[k]))
            if self.pre_ahead:  # the next tick's pre half, from the reset window
                self.enqueue_pre()
        self.stream.synchronize()

    def solve_window(self, max_iters: int = 20, *, with_prior: bool = False, **params) -> dict:
        """Levenberg-Marquardt on the current window of every camera (pipeline.LMPlan,
        pa_trajectory_lm_solve): the tick takes ONE fixed-lambda step per frame, which nothing
        protects when the window is far from the truth (start-up from the guessed init_pose);
        this iterates with accept / reject and adaptive damping until each camera's window has
        converged.  Runs eagerly on the pipeline's stream, outside the captured tick graph (the
        tick itself is unchanged), and updates the window in place.  Returns per camera: status
        (_lib.LM_CONVERGED / LM_MAX_ITERS / LM_STALLED), cost0, cost, iters (numpy).  **params:
        the other fields of pa_lm_params (pipeline.LM_DEFAULTS).
        With pre_ahead the window between ticks is already the next tick's: advanced, its newest
        frame predicted and without keypoints.  That frame's projection factors stay out of the
        solve (pa_window_lm_solve, newest_pending: its dynamics factor alone holds it), and the
        pre half's reduction is then redone on the solved window (pa_window_pose_tick_reduce:
        the whole pre half would advance the window a second time).
        Windows above 24 frames (pipeline.TICK_MAX_L, the cyclic-reduction solver's range) run
        the four-launch tick but have no LM solve: ValueError.
        marginalize=True: the window's factors alone are not the problem the ticks solve, so the
        plain solve raises ValueError; with_prior=True runs the solve with the current prior on
        frame 0 (pa_trajectory_lm_prior_solve: BatchFixedLagSmoother's optimize) and then
        re-derives the NEXT prior from the linearization at the solved window (pa_window_marginalize
        with the gradient the solve leaves, no damping step to re-centre by), as that smoother
        marginalizes at its optimized point.  No buffer moves: the captured tick graph stays valid.
        with_prior=True on a pipeline without marginalize=True: ValueError."""
        if self.L > pipeline.TICK_MAX_L:
            raise ValueError(f"solve_window(): pose_window {self.L} > {pipeline.TICK_MAX_L}, the range of the "
                             "device Levenberg-Marquardt solve (pa_trajectory_lm_solve)")
        if self.marginalize and not with_prior:
            raise ValueError("solve_window(): marginalize=True, and the plain Levenberg-Marquardt solve would leave the "
                             "marginalization prior out of its cost and steps; solve_window(with_prior=True) runs the "
                             "solve with the prior on frame 0")
        if with_prior and not self.marginalize:
            raise ValueError("solve_window(with_prior=True) needs a pipeline built with marginalize=True (there is no "
                             "prior to solve with)")
        key = (int(max_iters), tuple(sorted(params.items())))
        if getattr(self, "_lm_key", None) != key:
            self._lm = pipeline.LMPlan(self.traj_args, self.lin, T=self.n, L=self.L, max_iters=max_iters,
                                       newest_pending=self.pre_ahead, prior=self.prior if with_prior else None,
                                       **params)
            self._lm_key = key
        with torch.cuda.stream(self.stream):
            self._lm.launch()
            if with_prior:  # the next prior from the linearization at the solved window
                self.prior.marginalize(self.lin, self.win["pose"], self.win["angvel"], self.win["vel"],
                                       lam=self.gn.lam, delta=None, gn_info=None, nvalid=self.nvalid,
                                       n_kp=self.n_kp)
            if self.pre_ahead:
                pipeline.window_pose_tick_reduce(self.traj_args, self.tick_ws, lam=self.gn.lam)
        self.stream.synchronize()
        return {k: self._lm.out[k].cpu().numpy() for k in ("status", "cost0", "cost", "iters")}

    def window_state(self) -> dict:
        """Host copies of the window (y, pose, vel, angvel) after the last tick (pre_ahead: after
        the next tick's advance, whose newest keypoints are not in yet)."""
        self.stream.synchronize()
        return {k: v.cpu().numpy().copy() for k, v in self.win.items()}

    def window_covariance(self, lam: float | None = None) -> dict:
        """Marginal covariance of every frame of every camera's window (pipeline.MarginalsPlan,
        pa_trajectory_marginals): cov (n, L, 12, 12), Sigma = (J^T J + lam I)^-1 restricted to
        each frame's [pose (6, right perturbation, [omega; v]) | angvel (3) | vel (3)], and info
        (n,) int32 (0 = computed), as numpy.  Reads the factor outputs (self.lin) as they stand:
        the last tick's linearization (pre_ahead: the next tick's pre half's, so between ticks
        frame L-1 is the predicted one, its projection factors are out (status 3) and its
        covariance is the prediction's, as window_state()).  marginalize=True: with the prior the
        last tick's step had on frame 0.  lam defaults to the tick's; a window
        that has not filled yet needs a lam of that order.  Runs eagerly on the pipeline's
        stream, outside the captured tick graph."""
        lam = self.gn.lam if lam is None else float(lam)
        if getattr(self, "_marg", None) is None:
            self._marg = pipeline.MarginalsPlan(self.lin, T=self.n, L=self.L, lam=lam, prior=self.prior)
        self._marg.lam = lam
        with torch.cuda.stream(self.stream):
            self._marg.launch()
        self.stream.synchronize()
        return {"cov": self._marg.out["cov"].view(self.n, self.L, 12, 12).cpu().numpy().copy(),
                "info": self._marg.out["info"].cpu().numpy().copy()}

    def gate_state(self) -> dict:
        """The last tick's gate (gate_chi2), per camera, as numpy: d2 (n, K) the innovations' squared
        Mahalanobis distances (NaN for a corner that came in masked, that could not be tested, or
        when the gate was too young or had no covariance), ginfo (n,) int32 (_lib.GATE_APPLIED = 0,
        GATE_FEW = 1, GATE_NOCOV = 2, GATE_YOUNG = 3; non-zero: the staged mask went through as it
        came) and mask (n,) int32, the effective mask the tick used (win["mask"][:, -1]).
        Synchronises the pipeline's stream."""
        if self._gate is None:
            raise RuntimeError("gate_state() needs a pipeline built with gate_chi2")
        self.stream.synchronize()
        out = self._gate[2].out
        return {"d2": out["d2"].cpu().numpy().copy(), "ginfo": out["ginfo"].cpu().numpy().copy(),
                "mask": self.win["mask"][:, -1].cpu().numpy().copy()}

    def predict(self, taus, process_noise: bool = True) -> tuple:
        """The latency-compensated output: every camera's newest pose predicted to the horizons taus
        ((Q,) seconds after the newest frame's stamp) with the PoseDynamicsFactor model, and its
        covariance (pipeline.PredictPlan, pa_window_predict): poses (n, Q, 12) and covariances
        (n, Q, 12, 12) of [pose (6, right perturbation, [omega; v]) | angvel (3) | vel (3)], numpy.
        The covariance propagates window_covariance()'s marginals (the last tick's linearization,
        the tick's lam, the prior and the factor on the angular velocity where they are on) to first
        order; process_noise adds one factor's worth of it, whatever the horizon (dyn_sigma^2 on the
        pose, angvel_sigma^2 or 0, cv_sigma^2: the graph's dynamics noise is per frame pair).  NaN
        covariances for a camera whose marginals failed.  Runs eagerly on the pipeline's stream,
        outside the captured tick graph.  With pre_ahead the window between ticks already belongs
        to the next tick: ValueError."""
        if self.pre_ahead:
            raise ValueError("predict(): with pre_ahead=True the window between ticks is already the next tick's "
                             "(advanced, its newest frame a prediction itself)")
        if self.L < 3:
            raise ValueError("predict(): the covariance needs pose_window >= 3")
        tau = np.asarray(taus, np.float64).reshape(-1)
        if self._pred is None or self._pred[1].Q != len(tau):
            marg = pipeline.MarginalsPlan(self.lin, T=self.n, L=self.L, lam=self.gn.lam, cross=True,
                                          prior=self.prior)
            self._pred = (marg, pipeline.PredictPlan(self.win, Q=len(tau), marg=marg, vel_frame=self.vel_frame),
                          self._q_diag)
        marg, pred, q = self._pred
        pred.q_diag = q if process_noise else None
        with torch.cuda.stream(self.stream):
            pred.tau.copy_(torch.as_tensor(tau).reshape(1, -1).expand(self.n, -1))
            marg.launch()
            pred.launch()
        self.stream.synchronize()
        return pred.out["pose"].cpu().numpy().copy(), pred.out["cov"].cpu().numpy().copy()

    def stage_timing(self, stamps, present, kp_mask) -> None:
        """timed: this tick's dt_new / mask_new into the pinned block (before anything else of the
        tick is staged or enqueued: a bad stamp raises ValueError and leaves the window untouched).
        stamps (n,) seconds per camera: dt_new = stamps - the previous tick's (the first tick after
        construction or a reset: the nominal dt); None: the nominal dt.  present (n,) bool: an absent
        camera gets mask 0 (its window still advances to its stamp, on the prediction alone; whatever
        its slot of the batch holds is run and ignored).  kp_mask (n,) ints, one bit per keypoint,
        ANDed with present.  All None: nominal dt, all measured."""
        if not self.timed:
            if stamps is not None or present is not None or kp_mask is not None:
                raise ValueError("stamps / present / kp_mask need a pipeline built with timed=True")
            return
        n = self.n
        s = None if stamps is None else np.asarray(stamps, np.float64).reshape(n)
        if s is None or self._stamps is None:
            dt_new = np.full(n, self.dt)
            if s is not None and not np.isfinite(s).all():
                raise ValueError(f"stamps must be finite, got {s}")
        else:
            dt_new = s - self._stamps
            if not (np.isfinite(dt_new).all() and (dt_new > 0).all()):
                raise ValueError(f"stamps must increase by a positive finite dt per camera, got dt {dt_new}")
        mask = np.full(n, 0xFFFFFFFF, np.int64)
        if kp_mask is not None:
            mask &= np.asarray(kp_mask).astype(np.int64).reshape(n)
        if present is not None:
            mask[~np.asarray(present, bool).reshape(n)] = 0
        self.dt_new_h.numpy()[:] = dt_new
        self.mask_new_h.numpy()[:] = mask.astype(np.uint32).view(np.int32)
        self._stamps = s if s is not None else (None if self._stamps is None else self._stamps + self.dt)

    def tick_keypoints(self, y, *, stamps=None, present=None, kp_mask=None) -> tuple:
        """The pose stage alone on given normalized keypoints y (n, 2K) (the detector's output
        convention, validate.py:139-141): the same launches as a tick's pose stage, from
        self.y, captured as their own graph when graph=True.  Returns (newest pose (n, 12),
        GN info (n,)).  For driving the smoother with known measurements.  The results come from
        the pinned output block, and under pre_ahead self.win / self.lin already hold the next
        tick's pre half.  stamps / present / kp_mask (timed=True only): see stage_timing."""
        self.stage_timing(stamps, present, kp_mask)
        self.y_h.numpy()[:] = np.asarray(y, np.float32).reshape(self.y_h.shape)
        with torch.cuda.stream(self.stream):
            if self._graph_req:
                if self.graph is None:  # captured on first use (every buffer exists already)
                    self.graph = capture(self.stream, self._enqueue_keypoints)
                self.graph.replay()
            else:
                self._enqueue_keypoints()
            if self.pre_ahead:
                self._done.record()
                self.pre()
        (self._done if self.pre_ahead else self.stream).synchronize()
        return self.pose_h.numpy().copy(), self.info_h.numpy().copy()

    def close(self) -> None:
        """Drop the captured graphs."""
        self.graph = self.pre_graph = None
