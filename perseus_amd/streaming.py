"""Config 4: multi-camera streaming keypoint inference -> pose, one captured HIP graph.

Mirrors the per-frame loop of `scripts/streaming.py:120-131` (grab BGR + depth,
`/255`, depth nan/inf -> 0 and `/0.035`, centre 256x256 crop, `model(x)`, kornia
denormalize) for `n_cams` cameras per tick, batched into one forward, and (with
`pose_window` = L > 0) the pose stage BASELINE.json configs[4] asks for ("end-to-end pose
latency"): a fixed-lag smoother per camera over its last L frames, one damped Gauss-Newton
step per tick (pose_stage.PoseStage: the window, its factors, the three tick forms and
everything that can be asked of the window).  Per tick:

  host: frames -> pinned staging (centre crop rows only, or the full frame)
  GPU (one hipGraph replay on a private stream): H2D -> pa_detector_forward_rgbd_px
       (B = n_cams; fp16: the preprocess runs inside the stem's row loads; fp16x3 / fp32: the
       preprocess kernel, then the forward; the denormalize in the head), in the small-batch
       latency mode for fp16 and fp16x3 (the parity-grade tick)
       [pose stage] PoseStage's tick from the detector's keypoints, run as the split tick for
       windows <= 24 frames: its pre half (all of it that does not need the new keypoints) on the
       tick's stream while the forward runs on a second one (or, pre_ahead=True, right after the
       previous tick's results), and its post half after the forward
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

import numpy as np
import torch

from . import _lib
from .pose_stage import PoseStage, capture, mapped_address


def _of_pose(attr: str, off=None) -> property:
    """self.pose's attribute `attr` (read and write); `off` is its value without a pose stage."""
    return property(lambda self: off if self.pose is None else getattr(self.pose, attr),
                    lambda self, v: setattr(self.pose, attr, v))


def _pose_method(name: str, of: str | None = None):
    """The pipeline's method `name`: self.pose's method `of` (default: the same name), with its
    arguments and result; RuntimeError without a pose stage."""
    def method(self, *args, **kw):
        if self.pose is None:
            raise RuntimeError(f"{name}() needs the pose stage (pose_window > 0)")
        return getattr(self.pose, of or name)(*args, **kw)
    method.__name__, method.__doc__ = name, f"PoseStage.{of or name} of self.pose, on the pipeline's stream."
    return method


class StreamingPipeline:
    """The detector's tick: staging, the forward, the captured graph (module docstring).
    pose_window = L > 0 turns the pose stage on: one PoseStage of n_cams windows of L frames as
    self.pose, on the pipeline's stream and output block.  K (of the 256x256 crop), corners, dt,
    vel_frame, the sigmas, lam, init_pose / init_vel / init_angvel, proj_robust, marginalize, timed,
    angvel_sigma, gate_chi2 / gate_min_pass / gate_min_frames, split_pose and pre_ahead are
    PoseStage's keywords and are explained there; solve_window(), window_state(),
    window_covariance(), gate_state(), predict(), reset_window() and tick_keypoints() are its
    methods, and its state reads under the same names here (the properties below)."""

    def __init__(self, model, n_cams: int = 3, src_hw=(720, 1280), bgr: bool = True, host_crop: bool = True,
                 graph: bool = True, near: float | None = None, far: float | None = None, device=None,
                 pose_window: int = 0, K=None, corners=None, dt: float = 1.0 / 30.0, vel_frame: str = "world",
                 proj_sigma: float = 1.0, dyn_sigma: float = 0.1, cv_sigma: float = 0.1, lam: float = 1e-2,
                 init_pose=None, init_vel=None, init_angvel=None, split_k: bool = True,
                 zero_copy: bool | None = None, split_pose: bool = True, pre_ahead: bool = False,
                 zero_copy_out: bool = True, proj_robust=None, marginalize: bool = False, timed: bool = False,
                 angvel_sigma: float | None = None, gate_chi2: float | None = None, gate_min_pass: int = 4,
                 gate_min_frames: int = 3):
        self.pose = None
        PoseStage.check_args(pose_window, timed=timed, marginalize=marginalize, pre_ahead=pre_ahead,
                             gate_chi2=gate_chi2, gate_min_pass=gate_min_pass)
        if not torch.cuda.is_available():
            raise RuntimeError("StreamingPipeline needs a ROCm GPU (no CPU fallback)")
        if timed and not pose_window:
            raise ValueError("StreamingPipeline: timed=True needs the pose stage (pose_window > 0)")
        self.timed = bool(timed)
        self._timing_staged = False
        if marginalize and not pose_window:
            raise ValueError("StreamingPipeline: marginalize=True needs the pose stage (pose_window > 0)")
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
        # (RGB model: in = [rgb] alone; out after the pixels is PoseStage's output block)
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
            dp = mapped_address(self.in_h)
            self._src = (dp, dp + nr)
        # zero_copy_out: the head writes the pixels, and the split tick's post half info and the
        # newest poses, straight into the pinned output block over PCIe (a few hundred bytes), so
        # the tick has no D2H copy; the fused / four-launch pose stages keep the copy
        self._zc_out = bool(zero_copy_out)
        self._out_dev = mapped_address(self.out_h) if self._zc_out else None
        self._px_out = self._out_dev if self._zc_out else self.px_d.data_ptr()
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
        if self.pose_L:
            # the stage's output block is this one's after the pixels, its copy to the host this
            # one's; with the gate on, the stage never reads the timed block in place (PoseStage)
            self.pose = PoseStage(
                n, self.pose_L, K, device=self.dev, H=self.H, W=self.W, K=cam_K, corners=corners, dt=dt,
                vel_frame=vel_frame, proj_sigma=proj_sigma, dyn_sigma=dyn_sigma, cv_sigma=cv_sigma, lam=lam,
                init_pose=init_pose, init_vel=init_vel, init_angvel=init_angvel, proj_robust=proj_robust,
                marginalize=marginalize, timed=timed, angvel_sigma=angvel_sigma, gate_chi2=gate_chi2,
                gate_min_pass=gate_min_pass, gate_min_frames=gate_min_frames, split_pose=split_pose,
                pre_ahead=pre_ahead, graph=graph, stream=self.stream, out_h=self.out_h[self._px_bytes:],
                out_d=self.out_d[self._px_bytes:],
                out_mapped=self._out_dev + self._px_bytes if self._zc_out else None, flush=self._enqueue_out,
                timed_zero_copy=self.zero_copy)
            self.side = torch.cuda.Stream(self.dev)  # the split tick's forward, beside the pre half
        # the detector's keypoints: with a pose stage its keypoint buffer (tick_keypoints writes it too)
        self.y = self.pose.y if self.pose else torch.empty((n, 2 * K), dtype=torch.float32, device=self.dev)
        self.graph = None
        with torch.cuda.stream(self.stream):
            if self.pre_ahead:
                self.pose.enqueue_pre()
            self._enqueue()  # eager warm-up (also builds the kernels' first-launch state)
        self.stream.synchronize()
        if self.pose:
            self.pose.reset()  # the warm-up tick advanced it (pre_ahead: and prepares the next tick)
        if graph:
            self.graph = capture(self.stream, self._enqueue)
            if self.pre_ahead:
                self.pose.pre_graph = capture(self.stream, self.pose.enqueue_pre)
        self._done = torch.cuda.Event(enable_timing=True)  # (timed: the bench's latency path)

    # the pose stage's state and tick form under the names they have always had here
    win, lin, gn, traj_args, tick_ws, nvalid, dt = (_of_pose(k) for k in (
        "win", "lin", "gn", "traj_args", "tick_ws", "nvalid", "dt"))
    prior, _gate = _of_pose("prior"), _of_pose("_gate")
    pose_graph = _of_pose("graph")  # tick_keypoints' graph, captured on first use
    fused_pose, split_pose, pre_ahead = (_of_pose(k, False) for k in ("fused_pose", "split_pose", "pre_ahead"))
    # and its methods; tick_keypoints(y) is the pose stage alone on given normalized keypoints (n, 2K), on the
    # pipeline's stream and output block, captured as its own graph (self.pose_graph) when graph=True
    reset_window = _pose_method("reset_window", "reset")
    solve_window, window_state, window_covariance, gate_state, predict, tick_keypoints = (_pose_method(k) for k in (
        "solve_window", "window_state", "window_covariance", "gate_state", "predict", "tick_keypoints"))

    def _enqueue(self):
        """H2D, preprocess + forward + denormalize, [pose stage], D2H on the current stream.
        Split pose tick: the forward runs on a second stream while this one runs the pre half
        (everything but the newest keypoints); the post half after the join.  (The other
        assignment, pre half on the second stream, measured 0.233 vs 0.218 ms per fp16 tick;
        the pre half is only partly hidden either way: 0.187 ms without it, profiles/r04fork/.)"""
        L = _lib.lib()
        cur = torch.cuda.current_stream(self.dev)
        split = self.split_pose and not self.pre_ahead
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
            self.pose.enqueue_pre()
            cur.wait_stream(self.side)
            self.pose.enqueue_post(self.y)
        elif self.pose:
            self.pose.enqueue(self.y)  # (pre_ahead: the post half alone)
        self._enqueue_out()

    def _enqueue_out(self):
        """pixels (+ info, newest poses) to the host: one D2H, or nothing (zero_copy_out)."""
        if not self._zc_out:
            self.out_h.copy_(self.out_d, non_blocking=True)
        elif self.pose and not self.split_pose:  # the fused / four-launch stages write the device block
            self.out_h[self._px_bytes:].copy_(self.out_d[self._px_bytes:], non_blocking=True)

    def stage(self, rgb: np.ndarray, depth: np.ndarray | None = None) -> None:
        """Copy one tick of camera frames (n, Hs, Ws, 3) uint8 + (n, Hs, Ws) f32 metres
        into the pinned staging buffers (centre crop only when host_crop).  An RGB model
        stages the colour frames alone; a depth argument is ignored."""
        if self.rgb_only:
            if rgb.shape != (self.n, self.Hs, self.Ws, 3):
                raise ValueError(f"expected ({self.n},{self.Hs},{self.Ws},3) rgb")
        elif depth is None:
            raise ValueError("an RGBD model (num_channels=4) needs the depth frames")
        elif rgb.shape != (self.n, self.Hs, self.Ws, 3) or depth.shape != (self.n, self.Hs, self.Ws):
            raise ValueError(f"expected ({self.n},{self.Hs},{self.Ws},3) rgb and ({self.n},{self.Hs},{self.Ws}) depth")
        crop = (slice(None), slice(self.r0, self.r0 + self.H), slice(self.c0, self.c0 + self.W))
        self.rgb_h.numpy()[:] = rgb[crop] if self.host_crop else rgb
        if not self.rgb_only:
            self.depth_h.numpy()[:] = depth[crop] if self.host_crop else depth

    def replay(self) -> None:
        """One tick's device work on the current stream, no wait (pre_ahead: then the next
        tick's pre half, after self._done is recorded)."""
        if self.graph is not None:
            self.graph.replay()
        else:
            self._enqueue()
        if self.pre_ahead:
            self._done.record()
            self.pose.pre()

    def run(self) -> np.ndarray:
        """Process the staged tick; returns a copy of the (n, K, 2) pixel coordinates.
        timed: called without tick() having staged this tick's timing (run() or pipe(rgb, depth)
        directly), the tick takes the nominal dt and all keypoints measured, and the last stamps
        move on by dt, as tick() without keywords.  (replay() alone stages nothing: it runs
        whatever dt_new / mask_new the pinned block holds.)"""
        if self.timed and not self._timing_staged:
            self.pose.stage_timing(None, None, None)
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

    def tick(self, rgb: np.ndarray, depth: np.ndarray | None = None, *, stamps=None, present=None, kp_mask=None):
        """One camera tick through the pose stage: (pixels (n, K, 2), newest pose of each
        camera's window (n, 12: R row-major, t), GN info (n,) int32, 0 = solved).
        stamps / present / kp_mask (timed=True only): see PoseStage.stage_timing.

        The results are read from the pinned output block (self.px_h / pose_h / info_h), the
        only place every tick form writes them.  With pre_ahead, the next tick's pre half has
        already run when this returns: self.win, self.lin (the factor outputs, status 3 on
        the newest frame's projection factors) and the tick workspace hold the NEXT tick's
        advanced window, not this tick's (window_state() says the same)."""
        if self.pose is None:
            raise RuntimeError("tick() needs the pose stage (pose_window > 0)")
        self.pose.stage_timing(stamps, present, kp_mask)
        self._timing_staged = True  # (run() stages the nominal timing itself when a caller skipped this)
        px = self(rgb, depth)
        return px, self.pose_h.numpy().copy(), self.info_h.numpy().copy()

    def close(self) -> None:
        """Drop the graphs, then the handle they captured."""
        self.graph = None
        if self.pose:
            self.pose.close()
        if getattr(self, "_h", None) is not None:
            torch.cuda.synchronize(self.dev)
            _lib.lib().pa_detector_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
