"""Config 4: multi-camera streaming keypoint inference -> pose, one captured HIP graph.

Mirrors the per-frame loop of `scripts/streaming.py:120-131` (grab BGR + depth,
`/255`, depth nan/inf -> 0 and `/0.035`, centre 256x256 crop, `model(x)`, kornia
denormalize) for `n_cams` cameras per tick, batched into one forward, and (with
`pose_window` = L > 0) the pose stage BASELINE.json configs[4] asks for ("end-to-end pose
latency"): a fixed-lag smoother per camera over its last L frames built from the
reference's own factors (perseus/smoother/factors.py: KeypointProjectionFactor :182-275
per keypoint, PoseDynamicsFactor :8-142 and ConstantVelocityFactor :145-171 per frame
pair).  The reference stops at pixels (streaming.py draws them); the factor graph and
its optimizer live in downstream GTSAM code, so this build defines the loop: one damped
Gauss-Newton step per tick.  Per tick:

  host: frames -> pinned staging (centre crop rows only, or the full frame)
  GPU (one hipGraph replay on a private stream): H2D -> pa_detector_forward_rgbd_px
       (B = n_cams; fp16: the preprocess runs inside the stem's row loads; fp16x3 / fp32: the
       preprocess kernel, then the forward; the denormalize in the head), in the small-batch
       latency mode for fp16 and fp16x3 (the parity-grade tick)
       [pose stage] the sequence pa_window_advance_n (window shifts one frame, the new
       keypoints appended, the new pose predicted by the dynamics model, the count of real
       frames + 1) -> pa_trajectory_linearize (whitened factors of every camera's window;
       frames not yet filled by a real tick carry no projection factors) ->
       pa_trajectory_gn_step (delta and info only) -> pa_window_retract_newest (pose
       Exp(delta), velocities += delta, newest poses out), run as the split tick for windows
       <= 24 frames: pa_window_pose_tick_pre (all of it that does not need the new keypoints,
       on the tick's stream while the forward runs on a second one; or, pre_ahead=True, right
       after the previous tick's results) and pa_window_pose_tick_post after the forward
       -> the pixels, info and newest poses land in the pinned output block (zero_copy_out;
       else one D2H), one H2D of [rgb | depth] at the start (or zero-copy reads of it)
  host: wait for the replay, return (n_cams, K, 2) pixel coordinates (and the poses).

A 3-channel (RGB) model runs the same tick on the colour frames alone, as streaming.py does
with `frame[:C]`: the staging block holds [rgb] only, a depth argument is ignored, and the
detector call is pa_detector_forward_rgb_px (crop only).

The graph removes the per-launch CPU cost of the ~26 launches (the forward at B=3
is launch-bound, not compute-bound).  Workspace and every pose-stage buffer are
allocated before capture so no allocation happens inside the graph.
"""

from __future__ import annotations

import ctypes as C

import warnings

import numpy as np
import torch

from . import _lib, pipeline, synth


class StreamingPipeline:
    """pose_window = L > 0 turns the pose stage on (module docstring).  Its parameters:
    K (fx, fy, s, u0, v0) of the 256x256 crop and the body-frame corners (defaults: the
    datagen camera and cube, synth.CAMERA_K / CUBE_CORNERS); dt = the camera period;
    sigmas of the diagonal noise models (pixels, dynamics tangent, velocity); lam = the
    LM damping; init_pose (n_cams, 12) / init_vel / init_angvel fill every frame of the
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
    window_covariance() use them.  tick() / tick_keypoints() take stamps=, present= and kp_mask=;
    the new pair's dt and the new frame's mask go through one small pinned block [dt_new (n) f64 |
    mask_new (n) u32] that the graph copies to the device on the stream that runs the advance
    (zero_copy: read in place), so one captured graph serves every tick.  Not with pre_ahead.
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
    pa_keypoint_gate on the detector's keypoints: a corner whose innovation exceeds gate_chi2 (13.816
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
    predict(taus): the newest pose with its covariance at horizons after the newest frame."""

    def __init__(self, model, n_cams: int = 3, src_hw=(720, 1280), bgr: bool = True, host_crop: bool = True,
                 graph: bool = True, near: float | None = None, far: float | None = None, device=None,
                 pose_window: int = 0, K=None, corners=None, dt: float = 1.0 / 30.0, vel_frame: str = "world",
                 proj_sigma: float = 1.0, dyn_sigma: float = 0.1, cv_sigma: float = 0.1, lam: float = 1e-2,
                 init_pose=None, init_vel=None, init_angvel=None, split_k: bool = True,
                 zero_copy: bool | None = None, split_pose: bool = True, pre_ahead: bool = False,
                 zero_copy_out: bool = True, proj_robust=None, marginalize: bool = False, timed: bool = False,
                 angvel_sigma: float | None = None, gate_chi2: float | None = None, gate_min_pass: int = 4,
                 gate_min_frames: int = 3):
        self.angvel_sigma = None if angvel_sigma is None else float(angvel_sigma)
        self.gate_chi2 = None if gate_chi2 is None else float(gate_chi2)
        self.gate_min_pass, self.gate_min_frames = int(gate_min_pass), int(gate_min_frames)
        self._gate = None
        if self.gate_chi2 is not None:
            if not timed:
                raise ValueError("StreamingPipeline: gate_chi2 needs timed=True (the gate writes the keypoint masks)")
            if not (np.isfinite(self.gate_chi2) and self.gate_chi2 > 0) or self.gate_min_pass < 0:
                raise ValueError(f"StreamingPipeline: gate_chi2 must be a positive finite number and gate_min_pass "
                                 f">= 0, got {gate_chi2}, {gate_min_pass}")
            if 0 < pose_window < 3:
                raise ValueError("StreamingPipeline: gate_chi2 needs pose_window >= 3 (the prediction's covariance "
                                 "takes frame L-2's angular velocity)")
        if not torch.cuda.is_available():
            raise RuntimeError("StreamingPipeline needs a ROCm GPU (no CPU fallback)")
        if timed and pre_ahead:
            raise ValueError("StreamingPipeline: timed=True cannot run with pre_ahead=True (the next tick's dt is "
                             "not known when its pre half runs)")
        if timed and not pose_window:
            raise ValueError("StreamingPipeline: timed=True needs the pose stage (pose_window > 0)")
        self.timed = bool(timed)
        self._timing_staged = False
        if marginalize and pre_ahead:
            raise ValueError("StreamingPipeline: marginalize=True cannot run with pre_ahead=True (between ticks the "
                             "factor outputs already belong to the next tick)")
        if marginalize and not pose_window:
            raise ValueError("StreamingPipeline: marginalize=True needs the pose stage (pose_window > 0)")
        self.marginalize = bool(marginalize)
        self.prior = None
        cam_K = K  # (the name K is the keypoint count below)
        # a 3-channel model takes the RGB half of each frame (scripts/streaming.py:104,126 with an
        # RGB model feeds frame[:C]: the depth is dropped): RGB-only staging, pa_detector_forward_rgb_px
        if model.num_channels not in (3, 4):
            raise ValueError("StreamingPipeline feeds RGBD (num_channels=4) or RGB (num_channels=3)")
        self.rgb_only = model.num_channels == 3
        if self.rgb_only and (near is not None or far is not None):
            raise ValueError("near / far clip the depth channel: an RGB model (num_channels=3) has none")
        self.dev = torch.device(device or torch.device("cuda", torch.cuda.current_device()))
        self.model = model
        self.n = n_cams
        self.Hs, self.Ws = src_hw
        self.H, self.W = model.H, model.W
        if self.Hs < self.H or self.Ws < self.W:
            raise ValueError(f"source {src_hw} smaller than the model input {self.H}x{self.W}")
        self.bgr = bgr
        self.host_crop = host_crop
        self.near = -1.0 if near is None else float(near)
        self.far = -1.0 if far is None else float(far)
        sh, sw = (self.H, self.W) if host_crop else (self.Hs, self.Ws)
        self.sh, self.sw = sh, sw
        self.r0, self.c0 = self.Hs // 2 - self.H // 2, self.Ws // 2 - self.W // 2
        n, K = n_cams, model.n_keypoints
        # One staging block per direction, so a tick is one H2D and one D2H copy (each copy is a
        # ~5-12 us operation on the stream, and a copy enqueued between kernels stalls them):
        #   in  = [rgb (n, sh, sw, 3) u8 | depth (n, sh, sw) f32]
        #   out = [px (n, K, 2) f32 | info (n,) i32 | pad to 8 B | newest pose (n, 12) f64]
        # (RGB model: in = [rgb] alone)
        nr = n * sh * sw * 3
        if nr % 4 and not self.rgb_only:
            raise ValueError(f"staging: {n} x {sh} x {sw} RGB bytes not 4-aligned for the depth block")
        nin = nr if self.rgb_only else nr + n * sh * sw * 4
        self._po = ((n * K * 2 + n) * 4 + 7) // 8 * 8
        self._px_bytes = n * K * 8
        nout = self._po + n * 12 * 8
        self.in_h = torch.empty(nin, dtype=torch.uint8).pin_memory()
        self.in_d = torch.empty(nin, dtype=torch.uint8, device=self.dev)
        self.out_h = torch.zeros(nout, dtype=torch.uint8).pin_memory()
        self.out_d = torch.zeros(nout, dtype=torch.uint8, device=self.dev)

        def views(i, o):
            return (i[:nr].view(n, sh, sw, 3),
                    None if self.rgb_only else i[nr:].view(torch.float32).view(n, sh, sw),
                    o[:n * K * 8].view(torch.float32).view(n, K, 2),
                    o[n * K * 8:n * K * 8 + n * 4].view(torch.int32),
                    o[self._po:].view(torch.float64).view(n, 12))

        self.rgb_h, self.depth_h, self.px_h, self.info_h, self.pose_h = views(self.in_h, self.out_h)
        self.rgb_d, self.depth_d, self.px_d, self.info_d, self.pose_d = views(self.in_d, self.out_d)
        # zero_copy: the stem (fp16) / the preprocess kernel (fp16x3, fp32) read the pinned staging
        # over PCIe, no H2D copy in the tick.  None: on for the preprocess-kernel precisions (its
        # coalesced reads beat the copy: fp16x3 pose tick 0.330 -> 0.322 ms device), off for fp16
        # (the stem's row loads over PCIe lose: 0.252 -> 0.267 ms; profiles/r04v/)
        self.zero_copy = (model.precision != "fp16") if zero_copy is None else bool(zero_copy)
        self._src = (self.rgb_d.data_ptr(), None if self.rgb_only else self.depth_d.data_ptr())
        if self.zero_copy:
            dp = C.c_void_p()
            _lib.check(_lib.lib().pa_host_device_pointer(C.c_void_p(self.in_h.data_ptr()), C.byref(dp)),
                       "host_device_pointer")
            self._src = (dp.value, dp.value + nr)
        # zero_copy_out: the head writes the pixels, and the split tick's post half info and the
        # newest poses, straight into the pinned output block over PCIe (a few hundred bytes), so
        # the tick has no D2H copy; the fused / four-launch pose stages keep the copy
        self._zc_out = bool(zero_copy_out)
        self._px_out = self.px_d.data_ptr()
        if self._zc_out:
            dp = C.c_void_p()
            _lib.check(_lib.lib().pa_host_device_pointer(C.c_void_p(self.out_h.data_ptr()), C.byref(dp)),
                       "host_device_pointer")
            self._out_dev = dp.value
            self._px_out = dp.value
        self.y = torch.empty((n, 2 * K), dtype=torch.float32, device=self.dev)
        self.y_h = torch.empty((n, 2 * K), dtype=torch.float32).pin_memory()  # tick_keypoints' input
        self.pose_graph = None
        self.stream = torch.cuda.Stream(self.dev)
        # A private handle: the captured graph holds its weight and workspace pointers, so
        # nothing the model does later (a larger batch growing its workspace, a weight
        # reload destroying its handle) may free them under the graph.  Weights are taken
        # as of construction.
        L = _lib.lib()
        self._h = model._new_handle(self.dev)
        _lib.check(L.pa_detector_set_precision(self._h, _lib.precision_code(model.precision)), "set_precision")
        _lib.check(L.pa_detector_reserve(self._h, n), "reserve")
        # latency mode: a batch of n_cams frames leaves most CUs idle in the batched kernels
        # (pa_detector_set_split_k; same results as model.set_split_k(n_cams) + forward;
        # fp16 and fp16x3, fp32 has no such mode)
        self.split_k = bool(split_k) and n <= 64 and model.precision != "fp32"
        _lib.check(L.pa_detector_set_split_k(self._h, n if self.split_k else 0), "set_split_k")
        self.pose_L = int(pose_window)
        self._split_pose_req = bool(split_pose)
        self._pre_ahead_req = bool(pre_ahead)
        self.fused_pose = self.split_pose = self.pre_ahead = False
        if self.pose_L:
            self._init_pose_stage(cam_K, corners, dt, vel_frame, proj_sigma, dyn_sigma, cv_sigma, lam, init_pose,
                                  init_vel, init_angvel, proj_robust)
        self.graph = None
        self.pre_graph = None
        with torch.cuda.stream(self.stream):
            if self.pre_ahead:
                self._enqueue_pose_pre()
            self._enqueue()  # eager warm-up (also builds the kernels' first-launch state)
        self.stream.synchronize()
        if self.pose_L:
            self.reset_window()  # the warm-up tick advanced it (pre_ahead: and prepares the next tick)
        if graph:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=self.stream):
                self._enqueue()
            self.graph = g
            if self.pre_ahead:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=self.stream):
                    self._enqueue_pose_pre()
                self.pre_graph = g
        self._done = torch.cuda.Event(enable_timing=True)  # (timed: the bench's latency path)

    def _enqueue(self):
        """H2D, preprocess + forward + denormalize, [pose stage], D2H on the current stream.
        Split pose tick: the forward runs on a second stream while this one runs the pre half
        (everything but the newest keypoints); the post half after the join.  (The other
        assignment, pre half on the second stream, measured 0.233 vs 0.218 ms per fp16 tick;
        the pre half is only partly hidden either way: 0.187 ms without it, profiles/r04fork/.)"""
        L = _lib.lib()
        cur = torch.cuda.current_stream(self.dev)
        split = self.pose_L and self.split_pose and not self.pre_ahead
        fw = cur
        if split:
            self.side.wait_stream(cur)
            fw = self.side
        with torch.cuda.stream(fw):
            if not self.zero_copy:
                self.in_d.copy_(self.in_h, non_blocking=True)
            # fp16: the preprocess runs inside the stem's row loads; fp16x3 / fp32: the
            # preprocess kernel into the handle's staging, then the forward; the denormalize in the head
            if self.rgb_only:  # the same with the RGB source (crop only: the cameras deliver >= 256 x 256)
                _lib.check(L.pa_detector_forward_rgb_px(self._h, self._src[0], self.n, self.sh, self.sw,
                                                        int(self.bgr), 0, self.y.data_ptr(), self._px_out,
                                                        fw.cuda_stream), "forward_rgb_px")
            else:
                _lib.check(L.pa_detector_forward_rgbd_px(self._h, self._src[0], self._src[1], self.n,
                                                         self.sh, self.sw, int(self.bgr), self.near, self.far,
                                                         self.y.data_ptr(), self._px_out, fw.cuda_stream),
                           "forward_rgbd_px")
        if split:
            self._enqueue_pose_pre()
            cur.wait_stream(self.side)
            self._enqueue_pose_post()
        elif self.pose_L:
            self._enqueue_pose()  # (pre_ahead: the post half alone)
        self._enqueue_out()

    def _enqueue_out(self):
        """pixels (+ info, newest poses) to the host: one D2H, or nothing (zero_copy_out)."""
        if not self._zc_out:
            self.out_h.copy_(self.out_d, non_blocking=True)
        elif self.pose_L and not self.split_pose:  # the fused / four-launch stages write the device block
            self.out_h[self._px_bytes:].copy_(self.out_d[self._px_bytes:], non_blocking=True)

    def _enqueue_prior_in(self):
        """marginalize: the last tick's new prior becomes the current one, and its gradient at
        frame 1 of the un-advanced window, the frame the tick's advance makes the oldest."""
        if self.prior is not None:
            self.prior.advance()
            self.prior.linearize(self.win["pose"], self.win["angvel"], self.win["vel"], frame=1)

    def _enqueue_prior_out(self, info):
        """marginalize: frame 0 of the tick's linearization becomes the next prior, re-centred at
        the retracted window."""
        if self.prior is not None:
            self.prior.marginalize(self.lin, self.win["pose"], self.win["angvel"], self.win["vel"], lam=self.gn.lam,
                                   delta=self.gn.out["delta"], gn_info=info, nvalid=self.nvalid,
                                   n_kp=self.model.n_keypoints)

    def _enqueue_timed_in(self):
        """timed: this tick's [dt_new | mask_new] to the device, on the stream that runs the advance
        and before it (one 12 n byte copy; zero_copy: nothing, the advance reads the pinned block)."""
        if self.timed and (not self.zero_copy or self._gate is not None):
            self.tm_d.copy_(self.tm_h, non_blocking=True)

    def _enqueue_gate_predict(self):
        """gate: the marginals of the window as the tick finds it (the last tick's linearization and
        prior, so before _enqueue_prior_in and before the tick overwrites the factor outputs), the
        prediction to this tick's dt_new (after _enqueue_timed_in), and nvalid before the advance."""
        if self._gate is not None:
            marg, pred, _ = self._gate
            self._gate_nvalid.copy_(self.nvalid)
            marg.launch()
            pred.launch()

    def _enqueue_gate(self):
        """gate: the detector's keypoints (self.y) against the prediction; clears bits of the new
        frame's mask word before the launch that reads it."""
        if self._gate is not None:
            self._gate[2].launch()

    def _enqueue_pose_pre(self):
        self._enqueue_timed_in()
        self._enqueue_gate_predict()
        self._enqueue_prior_in()
        pipeline.window_pose_tick_pre(self.traj_args, self.tick_ws, lam=self.gn.lam, prior=self.prior)

    def _enqueue_pose_post(self):
        self._enqueue_gate()  # (on the ring entry the pre half landed)
        if self._zc_out:  # info and the newest poses straight into the pinned output block
            info, newest = self._out_dev + self._px_bytes, self._out_dev + self._po
        else:
            info, newest = self.gn.out["info"], self.pose_d
        pipeline.window_pose_tick_post(self.traj_args, self.y, self.tick_ws, delta=self.gn.out["delta"], info=info,
                                       newest=newest)
        self._enqueue_prior_out(info)

    def _enqueue_pose(self):
        """The pose stage on the current stream, from the keypoints in self.y (HBM-resident window):
        advance -> linearize -> GN step -> retract, as pa_window_pose_tick_pre + _post (split),
        pa_window_pose_tick's two launches (fused) or the four separate ones (bit-identical to
        the fused form; windows above 24 frames)."""
        if self.split_pose:
            if not self.pre_ahead:
                self._enqueue_pose_pre()
            self._enqueue_pose_post()
            return
        self._enqueue_timed_in()
        self._enqueue_gate_predict()
        self._enqueue_gate()  # (on the device copy of mask_new, before the advance reads it)
        self._enqueue_prior_in()
        if self.fused_pose:
            pipeline.window_pose_tick(self.traj_args, self.y, lam=self.gn.lam, delta=self.gn.out["delta"],
                                      info=self.gn.out["info"], newest=self.pose_d, prior=self.prior)
        else:
            tm = dict(dt_new=self._tm_ptrs[0], mask_new=self._tm_ptrs[1]) if self.timed else {}
            pipeline.window_advance(self.y, self.win, dt=self.dt, vel_frame=self.vel_frame, nvalid=self.nvalid, **tm)
            pipeline.launch(self.traj_args, self.dev)
            self.gn.launch()  # delta, and info straight into the output block
            pipeline.window_retract(self.win, self.gn.out["delta"], self.gn.out["info"], newest=self.pose_d)
        self._enqueue_prior_out(self.gn.out["info"])

    def _init_pose_stage(self, K, corners, dt, vel_frame, proj_sigma, dyn_sigma, cv_sigma, lam, init_pose, init_vel,
                         init_angvel, proj_robust=None):
        n, Lw, nk, dev = self.n, self.pose_L, self.model.n_keypoints, self.dev
        if Lw < 2:
            raise ValueError("pose_window must be >= 2 frames (the dynamics factors couple frame pairs)")
        if vel_frame not in ("world", "body"):
            raise AssertionError("vel_frame must be 'world' or 'body'.")  # factors.py:41
        self.dt, self.vel_frame = float(dt), vel_frame
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
        # real frames per camera window (from its end): until L ticks have run, the frames
        # before them are the initial state with no measurement, and carry no projection factor
        self.nvalid = torch.zeros(n, dtype=torch.int32, device=dev)
        rings = {}
        if self.timed:
            # the rings, and the tick's [dt_new (n) f64 | mask_new (n) u32] block: pinned, and its
            # device copy (zero_copy: the advance reads the pinned block in place)
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
        if self.timed:
            assert self.traj_args.dt_pair == self.win["dt"].data_ptr()
            assert self.traj_args.kp_mask == self.win["mask"].data_ptr()
            base = self.tm_d.data_ptr()
            if self.zero_copy and self.gate_chi2 is None:  # (the gate writes the device copy's masks)
                dp = C.c_void_p()
                _lib.check(_lib.lib().pa_host_device_pointer(C.c_void_p(self.tm_h.data_ptr()), C.byref(dp)),
                           "host_device_pointer")
                base = dp.value
            self._tm_ptrs = (base, base + n * 8)
            self.traj_args.dt_new, self.traj_args.mask_new = self._tm_ptrs
        if self.marginalize:
            # the prior on frame 0: the fused / split ticks get it beside the pa_traj_args (the _prior
            # entry points), the four-launch path's GN step from the plan
            self.prior = pipeline.PriorPlan(T=n, L=Lw, device=dev)
        self.gn = pipeline.GNPlan(self.lin, T=n, L=Lw, lam=lam, prior=self.prior)
        self.gn.out["info"] = self.info_d  # the GN step writes info into the output block
        # pa_window_pose_tick: one workgroup per camera of up to 24 frames, at most one per CU
        self.fused_pose = (Lw <= pipeline.TICK_MAX_L
                           and n <= torch.cuda.get_device_properties(dev).multi_processor_count)
        # the split tick (pa_window_pose_tick_pre / _post, same limits): everything but the
        # newest frame's projection factors runs beside the forward, which gets its own stream
        self.split_pose = self.fused_pose and self._split_pose_req
        # pre_ahead: the pre half of tick k + 1 runs right after tick k's results are on the host
        # (in the gap before the next camera frames), so a tick's latency path is H2D, forward,
        # post half, D2H.  The window and factor outputs then already hold the next tick's advance.
        self.pre_ahead = self.split_pose and self._pre_ahead_req
        if self._pre_ahead_req and not self.pre_ahead:  # never drop the request silently
            why = ("split_pose=False" if not self._split_pose_req else
                   f"pose_window {Lw} > {pipeline.TICK_MAX_L}" if Lw > pipeline.TICK_MAX_L else
                   f"{n} cameras > the device's CUs")
            warnings.warn(f"StreamingPipeline: pre_ahead needs the split pose tick ({why}); running the full-latency "
                          f"tick (self.pre_ahead is False)", RuntimeWarning, stacklevel=3)
        if self.split_pose and self._zc_out:
            # the post half writes info and the newest poses straight into the pinned output block
            # (self.info_h / self.pose_h); nothing writes a device copy, so none is exposed
            self.gn.out["info"] = None
        self.tick_ws = pipeline.window_pose_tick_workspace(n, Lw, dev)
        self.side = torch.cuda.Stream(dev)
        self._sigmas = (float(dyn_sigma), float(cv_sigma))
        self._pred = None  # predict()'s plans, built on first use
        if self.gate_chi2 is not None:
            # the gate's three launches.  Marginals and prediction read the window and the factor
            # outputs as the tick finds them; the gate itself acts on the new frame's mask word: the
            # ring entry the pre half has landed (split tick: strides L and 12 L, the predicted pose is
            # the advanced window's newest frame), or the device copy of mask_new (fused / four-launch)
            marg = pipeline.MarginalsPlan(self.lin, T=n, L=Lw, lam=lam, cross=True, prior=self.prior)
            self._gate_nvalid = torch.zeros(n, dtype=torch.int32, device=dev)  # nvalid as the tick starts
            pred = pipeline.PredictPlan(self.win, Q=1, marg=marg, q_diag=self._process_noise(), vel_frame=vel_frame,
                                        tau=self._tm_ptrs[0])
            _, _, _, _, Cn, Kt, Tc, isp = self.lin["_keep"][:8]
            if self.split_pose:
                tgt = dict(pose_pred=self.win["pose"].data_ptr() + (Lw - 1) * 12 * 8, pose_stride=12 * Lw,
                           mask=self.win["mask"].data_ptr() + (Lw - 1) * 4, mask_stride=Lw)
            else:
                tgt = dict(pose_pred=pred.out["pose"], pose_stride=12, mask=self._tm_ptrs[1], mask_stride=1)
            gate = pipeline.GatePlan(self.y, tgt.pop("pose_pred"), pred.out["cov"], Cn, Kt, isp, tgt.pop("mask"),
                                     chi2=self.gate_chi2, min_pass=self.gate_min_pass,
                                     min_frames=self.gate_min_frames, nvalid=self._gate_nvalid, tcam=Tc, H=self.H,
                                     W=self.W, **tgt)
            self._gate = (marg, pred, gate)

    def _process_noise(self) -> torch.Tensor:
        """One factor's worth of process noise, [dyn_sigma^2 x 6 | angvel_sigma^2 or 0 x 3 | cv_sigma^2
        x 3]: the graph's dynamics noise is per frame pair, not per second."""
        sd, sc = self._sigmas
        sw = 0.0 if self.angvel_sigma is None else self.angvel_sigma
        return torch.tensor([sd * sd] * 6 + [sw * sw] * 3 + [sc * sc] * 3, dtype=torch.float64, device=self.dev)

    def reset_window(self) -> None:
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
                self._enqueue_pose_pre()
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
        if not self.pose_L:
            raise RuntimeError("solve_window() needs the pose stage (pose_window > 0)")
        if self.pose_L > pipeline.TICK_MAX_L:
            raise ValueError(f"solve_window(): pose_window {self.pose_L} > {pipeline.TICK_MAX_L}, the range of the "
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
            self._lm = pipeline.LMPlan(self.traj_args, self.lin, T=self.n, L=self.pose_L, max_iters=max_iters,
                                       newest_pending=self.pre_ahead, prior=self.prior if with_prior else None,
                                       **params)
            self._lm_key = key
        with torch.cuda.stream(self.stream):
            self._lm.launch()
            if with_prior:  # the next prior from the linearization at the solved window
                self.prior.marginalize(self.lin, self.win["pose"], self.win["angvel"], self.win["vel"],
                                       lam=self.gn.lam, delta=None, gn_info=None, nvalid=self.nvalid,
                                       n_kp=self.model.n_keypoints)
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
        if not self.pose_L:
            raise RuntimeError("window_covariance() needs the pose stage (pose_window > 0)")
        lam = self.gn.lam if lam is None else float(lam)
        if getattr(self, "_marg", None) is None:
            self._marg = pipeline.MarginalsPlan(self.lin, T=self.n, L=self.pose_L, lam=lam, prior=self.prior)
        self._marg.lam = lam
        with torch.cuda.stream(self.stream):
            self._marg.launch()
        self.stream.synchronize()
        return {"cov": self._marg.out["cov"].view(self.n, self.pose_L, 12, 12).cpu().numpy().copy(),
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
        if not self.pose_L:
            raise RuntimeError("predict() needs the pose stage (pose_window > 0)")
        if self.pre_ahead:
            raise ValueError("predict(): with pre_ahead=True the window between ticks is already the next tick's "
                             "(advanced, its newest frame a prediction itself)")
        if self.pose_L < 3:
            raise ValueError("predict(): the covariance needs pose_window >= 3")
        tau = np.asarray(taus, np.float64).reshape(-1)
        if self._pred is None or self._pred[1].Q != len(tau):
            marg = pipeline.MarginalsPlan(self.lin, T=self.n, L=self.pose_L, lam=self.gn.lam, cross=True,
                                          prior=self.prior)
            self._pred = (marg, pipeline.PredictPlan(self.win, Q=len(tau), marg=marg, vel_frame=self.vel_frame),
                          self._process_noise())
        marg, pred, q = self._pred
        pred.q_diag = q if process_noise else None
        with torch.cuda.stream(self.stream):
            pred.tau.copy_(torch.as_tensor(tau).reshape(1, -1).expand(self.n, -1))
            marg.launch()
            pred.launch()
        self.stream.synchronize()
        return pred.out["pose"].cpu().numpy().copy(), pred.out["cov"].cpu().numpy().copy()

    def stage(self, rgb: np.ndarray, depth: np.ndarray | None = None) -> None:
        """Copy one tick of camera frames (n, Hs, Ws, 3) uint8 + (n, Hs, Ws) f32 metres
        into the pinned staging buffers (centre crop only when host_crop).  An RGB model
        stages the colour frames alone; a depth argument is ignored."""
        if self.rgb_only:
            if rgb.shape != (self.n, self.Hs, self.Ws, 3):
                raise ValueError(f"expected ({self.n},{self.Hs},{self.Ws},3) rgb")
            if self.host_crop:
                r0, c0 = self.r0, self.c0
                self.rgb_h.numpy()[:] = rgb[:, r0:r0 + self.H, c0:c0 + self.W]
            else:
                self.rgb_h.numpy()[:] = rgb
            return
        if depth is None:
            raise ValueError("an RGBD model (num_channels=4) needs the depth frames")
        if rgb.shape != (self.n, self.Hs, self.Ws, 3) or depth.shape != (self.n, self.Hs, self.Ws):
            raise ValueError(f"expected ({self.n},{self.Hs},{self.Ws},3) rgb and ({self.n},{self.Hs},{self.Ws}) depth")
        if self.host_crop:
            r0, c0 = self.r0, self.c0
            self.rgb_h.numpy()[:] = rgb[:, r0:r0 + self.H, c0:c0 + self.W]
            self.depth_h.numpy()[:] = depth[:, r0:r0 + self.H, c0:c0 + self.W]
        else:
            self.rgb_h.numpy()[:] = rgb
            self.depth_h.numpy()[:] = depth

    def replay(self) -> None:
        """One tick's device work on the current stream, no wait (pre_ahead: then the next
        tick's pre half, after self._done is recorded)."""
        if self.graph is not None:
            self.graph.replay()
        else:
            self._enqueue()
        if self.pre_ahead:
            self._done.record()
            self._pre()

    def _pre(self):
        if self.pre_graph is not None:
            self.pre_graph.replay()
        else:
            self._enqueue_pose_pre()

    def run(self) -> np.ndarray:
        """Process the staged tick; returns a copy of the (n, K, 2) pixel coordinates.
        timed: called without tick() having staged this tick's timing (run() or pipe(rgb, depth)
        directly), the tick takes the nominal dt and all keypoints measured, and the last stamps
        move on by dt, as tick() without keywords.  (replay() alone stages nothing: it runs
        whatever dt_new / mask_new the pinned block holds.)"""
        if self.timed and not self._timing_staged:
            self._stage_timing(None, None, None)
        self._timing_staged = False  # (this tick's; the next one stages its own)
        with torch.cuda.stream(self.stream):  # replay() launches on the current stream
            self.replay()
        if self.pre_ahead:
            self._done.synchronize()  # the results; the next tick's pre half keeps running
        else:
            self.stream.synchronize()
        return self.px_h.numpy().copy()

    def __call__(self, rgb: np.ndarray, depth: np.ndarray | None = None) -> np.ndarray:
        self.stage(rgb, depth)
        return self.run()

    def _stage_timing(self, stamps, present, kp_mask) -> None:
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
        self._timing_staged = True  # (run() stages the nominal timing itself when a caller skipped this)

    def tick(self, rgb: np.ndarray, depth: np.ndarray | None = None, *, stamps=None, present=None, kp_mask=None):
        """One camera tick through the pose stage: (pixels (n, K, 2), newest pose of each
        camera's window (n, 12: R row-major, t), GN info (n,) int32, 0 = solved).
        stamps / present / kp_mask (timed=True only): see _stage_timing.

        The results are read from the pinned output block (self.px_h / pose_h / info_h), the
        only place every tick form writes them.  With pre_ahead, the next tick's pre half has
        already run when this returns: self.win, self.lin (the factor outputs, status 3 on
        the newest frame's projection factors) and the tick workspace hold the NEXT tick's
        advanced window, not this tick's (window_state() says the same)."""
        if not self.pose_L:
            raise RuntimeError("tick() needs the pose stage (pose_window > 0)")
        self._stage_timing(stamps, present, kp_mask)
        px = self(rgb, depth)
        return px, self.pose_h.numpy().copy(), self.info_h.numpy().copy()

    def tick_keypoints(self, y, *, stamps=None, present=None, kp_mask=None) -> tuple:
        """The pose stage alone on given normalized keypoints y (n, 2K) (the detector's output
        convention, validate.py:139-141): the same launches as a tick's pose stage, from
        self.y, captured as their own graph when graph=True.  Returns (newest pose (n, 12),
        GN info (n,)).  For driving the smoother with known measurements.  As tick(): the
        results come from the pinned output block, and under pre_ahead self.win / self.lin
        already hold the next tick's pre half."""
        if not self.pose_L:
            raise RuntimeError("tick_keypoints() needs the pose stage (pose_window > 0)")
        self._stage_timing(stamps, present, kp_mask)
        self._timing_staged = False  # (consumed by this tick, which does not go through run())
        self.y_h.numpy()[:] = np.asarray(y, np.float32).reshape(self.y_h.shape)

        def enqueue():
            self.y.copy_(self.y_h, non_blocking=True)
            self._enqueue_pose()
            self._enqueue_out()

        with torch.cuda.stream(self.stream):
            if self.graph is not None:
                if self.pose_graph is None:  # captured on first use (every buffer exists already)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=self.stream):
                        enqueue()
                    self.pose_graph = g
                self.pose_graph.replay()
            else:
                enqueue()
            if self.pre_ahead:
                self._done.record()
                self._pre()
        (self._done if self.pre_ahead else self.stream).synchronize()
        return self.pose_h.numpy().copy(), self.info_h.numpy().copy()

    def close(self) -> None:
        """Drop the graphs, then the handle they captured."""
        self.graph = None
        self.pose_graph = None
        self.pre_graph = None
        if getattr(self, "_h", None) is not None:
            torch.cuda.synchronize(self.dev)
            _lib.lib().pa_detector_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
