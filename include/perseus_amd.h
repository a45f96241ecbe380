/*
 * perseus_amd — C ABI of the MI355X keypoint-inference path (libperseus_amd.so).
 *
 * Plain pointers and sizes only; every array argument named *_dev is a device
 * pointer (hipMalloc / torch CUDA tensor storage) owned by the caller, every
 * `stream` is a hipStream_t passed as void* (NULL = default stream).  All entry
 * points return 0 on success and a negative PA_E* code on failure, with a
 * thread-local message in pa_last_error().  Nothing here synchronises the
 * stream; results are ready when the caller's stream work completes.
 *
 * Reference interfaces replaced (paths relative to pculbertson/perseus):
 *   detector  perseus/detector/models.py:6-40   KeypointCNN.__init__/forward
 *             perseus/detector/validate.py:92-98 ckpt load ("module." strip) + eval
 *   factors   perseus/smoother/factors.py:54-142  PoseDynamicsFactor.error_func
 *             perseus/smoother/factors.py:160-171 ConstantVelocityFactor.error_func
 *             perseus/smoother/factors.py:216-275 KeypointProjectionFactor.error_func
 */
#ifndef PERSEUS_AMD_H
#define PERSEUS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PA_OK 0
#define PA_EINVAL -1   /* bad argument (shape, size, null pointer)           */
#define PA_EHIP -2     /* HIP runtime error (message has hipGetErrorString)   */
#define PA_ENOMEM -3   /* device allocation failed                            */

#define PA_PREC_FP16 0   /* fp16 NHWC activations/weights, fp32 MFMA accumulate     */
#define PA_PREC_FP32 1   /* fp32 NHWC, exact-f32 MFMA (reference parity mode)     */
#define PA_PREC_FP16X3 2 /* fast parity mode: hi/lo fp16 planes, 3 fp16 MFMA products
                            per MAC (x_hi w_hi + x_lo w_hi + x_hi w_lo), f32 accumulate */

#define PA_VEL_WORLD 0 /* factors.py:41 vel_frame="world" */
#define PA_VEL_BODY 1  /* vel_frame="body"                */

#define PA_ROBUST_NONE 0   /* plain Gaussian noise model: err = 0.5 |r_w|^2            */
#define PA_ROBUST_HUBER 1  /* noiseModel::Robust(mEstimator::Huber(k), Diagonal)       */
#define PA_ROBUST_CAUCHY 2 /* noiseModel::Robust(mEstimator::Cauchy(k), Diagonal)      */

const char* pa_last_error(void);
const char* pa_version(void);

/* ------------------------------------------------------------------ detector */
typedef struct pa_detector pa_detector;

/* Replaces KeypointCNN(n_keypoints, num_channels, H, W) + load_state_dict + eval()
 * (models.py:9-32, validate.py:92-98).
 * weights: HOST f32 blob = the state-dict float tensors in torchvision resnet18
 * order with the "resnet." prefix and without the 20 num_batches_tracked
 * counters (conv1.weight [64,C,7,7]; bn1.{weight,bias,running_mean,running_var};
 * layer1.0.conv1.weight ... ; fc.weight [2K,512]; fc.bias [2K]) — 102 tensors,
 * nbytes must equal the sum of their sizes.  BatchNorm (eps 1e-5) is folded and
 * weights are packed for the GPU here, once.  Only H = W = 256 and
 * 1 <= in_ch <= 4 are supported (the trained configurations). */
int pa_detector_create(const float* weights, size_t nbytes, int in_ch, int n_kp, int H, int W,
                       pa_detector** out);
void pa_detector_destroy(pa_detector* d);

/* Pre-size the activation workspace for batches up to max_batch (clamped to the
 * 1,024-frame chunk a forward runs in), and for 4-channel models in fp16x3 / fp32 also
 * forward_rgbd's f32 input staging, for 3-channel models forward_rgb's (a later
 * set_precision keeps the reservation).
 * Without it, allocation is done lazily by the first call of a larger batch, which
 * frees the smaller buffer: capture a graph only after reserve() (or after an eager
 * call of the same batch), and reserve the largest batch any graph will replay. */
int pa_detector_reserve(pa_detector* d, int max_batch);

/* PA_PREC_FP16 (default), PA_PREC_FP32 or PA_PREC_FP16X3. */
int pa_detector_set_precision(pa_detector* d, int precision);

/* Latency mode for small batches (the streaming pose stage, streaming.py:101-166: one
 * frame per camera per tick).  fp16 and fp16x3 forwards whose whole batch is
 * B <= max_batch frames run the stem on short bands, layer1 on small tiles and the convs
 * of layers 2-4 as split-K launches + a fixed-order reduce (layer2's stride-2 entry, with
 * 64 input channels, on one-tile workgroups instead), which fills the chip at a few
 * frames (deterministic, but not bit-identical to the batched kernels: the f32 sums are
 * taken in another order; fp16x3 stays within its 1e-3 px parity bar).  Allocates
 * max_batch MiB of partials.  max_batch = 0 (default) turns it off; at most 64. */
int pa_detector_set_split_k(pa_detector* d, int max_batch);

/* Replaces KeypointCNN.forward (models.py:34-40): x (B,C,H,W) f32 NCHW contiguous
 * on the device -> y (B, 2K) f32, y[:,2k] = x_k, y[:,2k+1] = y_k in [-1,1]
 * normalized image coordinates.  B = 0 is a no-op. */
int pa_detector_forward(pa_detector* d, const float* x_dev, int B, float* y_dev, void* stream);

/* Camera frames -> keypoints: uint8 HWC RGB (bgr != 0: BGR byte order, as
 * the ZED delivers) + f32 depth in metres, both [B][Hs][Ws], centre-cropped to 256x256;
 * pa_preprocess_rgbd's arithmetic (streaming.py:68-80, deterministic near/far clip, < 0 =
 * off).  fp16: applied inside the stem's row loads, so the f32 (B,4,256,256) input is never
 * written; fp16x3 / fp32: the preprocess kernel into the handle's own f32 staging (sized by
 * pa_detector_reserve, else by the first call of a larger batch), then the forward.  Output
 * bit-identical to pa_preprocess_rgbd + pa_detector_forward.  4-channel models only. */
int pa_detector_forward_rgbd(pa_detector* d, const uint8_t* rgb_dev, const float* depth_dev, int B, int Hs, int Ws,
                             int bgr, float near_m, float far_m, float* y_dev, void* stream);

/* pa_detector_forward_rgbd + pa_keypoints_postprocess (no target) in the same launches:
 * the head also writes the pixel coordinates px (B, n_kp, 2) f32, kornia's denormalize
 * (streaming.py:128-131), bit-identical to the separate postprocess.  The streaming
 * tick's detector call (one launch fewer per tick). */
int pa_detector_forward_rgbd_px(pa_detector* d, const uint8_t* rgb_dev, const float* depth_dev, int B, int Hs, int Ws,
                                int bgr, float near_m, float far_m, float* y_dev, float* px_dev, void* stream);

/* RGB-only frames -> keypoints, for 3-channel models (scripts/streaming.py:104,112-128 with an
 * RGB model; perseus/detector/validate_real.py:62-74): uint8 HWC [B][Hs][Ws][3], RGB byte
 * order (bgr != 0: BGR).  resize_short = 0: x = u8 / 255 at the centre 256x256 window (origin
 * Hs/2 - 128, Ws/2 - 128; needs Hs, Ws >= 256).  resize_short = S >= 256: u8 / 255, bilinear
 * resize (align_corners false, no antialiasing: torch.nn.functional.interpolate's f32
 * arithmetic) so that the short side is S (kornia resize, side = "short"), then the centre
 * 256x256 window of the resized image (kornia center_crop); any Hs, Ws >= 1.  Other values
 * of resize_short, a model that is not 3-channel and null pointers return PA_EINVAL before
 * any launch; B = 0 is a no-op.  fp16: applied inside the stem's row loads (the f32 input is
 * never written); fp16x3 / fp32: pa_preprocess_rgb's kernel into the handle's f32 staging
 * (sized by pa_detector_reserve, else by the first call of a larger batch), then the forward.
 * Output bit-identical to pa_preprocess_rgb + pa_detector_forward. */
int pa_detector_forward_rgb(pa_detector* d, const uint8_t* rgb_dev, int B, int Hs, int Ws, int bgr,
                            int resize_short, float* y_dev, void* stream);
/* The same, the head also writing the pixel coordinates px (B, n_kp, 2) as
 * pa_detector_forward_rgbd_px does: the RGB streaming tick's detector call. */
int pa_detector_forward_rgb_px(pa_detector* d, const uint8_t* rgb_dev, int B, int Hs, int Ws, int bgr,
                               int resize_short, float* y_dev, float* px_dev, void* stream);
/* pa_detector_profile of pa_detector_forward_rgb (same outputs; diagnostics only). */
int pa_detector_profile_rgb(pa_detector* d, const uint8_t* rgb_dev, int B, int Hs, int Ws, int bgr,
                            int resize_short, float* y_dev, void* stream, float* ms_out, const char** names_out,
                            int max_n);
/* The arithmetic of pa_detector_forward_rgb's input alone: x (B,3,H,W) f32 NCHW on the device
 * (H = W = 256 only). */
int pa_preprocess_rgb(const uint8_t* rgb_dev, int B, int Hs, int Ws, int bgr, int resize_short, int H, int W,
                      float* x_dev, void* stream);

/* The device address of a mapped pinned host buffer (hipHostGetDevicePointer): forward_rgbd
 * may read the camera frames straight from host memory over PCIe (zero-copy), so a tick
 * needs no H2D copy before the stem (StreamingPipeline(zero_copy=True)). */
int pa_host_device_pointer(const void* host, void** dev);

/* Same forward with a HIP event after every kernel: writes up to max_n per-kernel
 * durations (ms) into ms_out and their names into names_out (may be NULL), returns
 * the number of kernels or <0.  Synchronises the stream (diagnostics only). */
int pa_detector_profile(pa_detector* d, const float* x_dev, int B, float* y_dev, void* stream,
                        float* ms_out, const char** names_out, int max_n);

/* Average device time of ONE launch of the forward (index in pa_detector_profile
 * order): the forward runs once with that launch issued `reps` times back to back
 * between two HIP events on `stream`.  y_dev and the activations are scratch
 * afterwards (an in-place residual launch accumulates); run a normal forward before
 * using outputs.  Test/measurement entry point, not part of the drop-in surface. */
int pa_detector_time_launch(pa_detector* d, const float* x_dev, int B, float* y_dev, void* stream, int index,
                            int reps, float* avg_ms_out, const char** name_out);

/* Algorithmic FLOPs of one frame's forward (2 x MAC over the 20 convs + fc). */
double pa_detector_flops_per_frame(const pa_detector* d);

/* Fused preprocessing (streaming.py:59-82, augmentations.py:128-169
 * val mode): RGB uint8 (B,Hs,Ws,3, BGR if bgr) + f32 depth metres (B,Hs,Ws),
 * centre crop to H x W, rgb/255, depth nan/inf -> 0, depth/0.035, then the
 * deterministic near/far clip (scaled depth < near or > far -> 0; pass near<0 /
 * far<0 to skip) -> x (B,4,H,W) f32 NCHW on the device. */
int pa_preprocess_rgbd(const uint8_t* rgb_dev, const float* depth_dev, int B, int Hs, int Ws, int bgr,
                       float near_m, float far_m, int H, int W, float* x_dev, void* stream);

/* Keypoint post-processing on device (validate.py:130-153): px = (n+1)(S-1)/2 into
 * px_dev (B,K,2); if target_dev != NULL (B,2K normalized), SmoothL1(beta=1) per
 * element into loss_dev (B,2K). */
int pa_keypoints_postprocess(const float* y_dev, const float* target_dev, int B, int n_kp, int H, int W,
                             float* px_dev, float* loss_dev, void* stream);

/* Validation loss statistics (validate.py:162-168, the "Validation Loss" block):
 * over n f32 losses on the device, stats_dev[0..4] (f64, device) = mean, stdev
 * (unbiased, torch.std; NaN for n = 1), min, max, median (torch.median: the
 * element of sorted index (n-1)/2).  ws_dev: device scratch of
 * pa_loss_statistics_workspace(n) bytes, 16-byte aligned.  Stream-ordered, no
 * host sync.  n must be > 0 (torch.median raises on an empty tensor). */
size_t pa_loss_statistics_workspace(long long n);
int pa_loss_statistics(const float* loss_dev, long long n, double* stats_dev, void* ws_dev, size_t ws_bytes,
                       void* stream);

/* ------------------------------------------------------------------- factors */
/* Pose encoding: 12 f64 per pose = R row-major (9) then t (3).  Jacobians are
 * column-major per factor (Eigen/GTSAM order), tangent order [omega; v].
 * inv_sigma (may be NULL): per-dimension 1/sigma of a diagonal noise model; when
 * given, r and every J are whitened in place (A = J/sigma, r_w = r/sigma) and
 * err_dev[i] = 0.5 * ||r_w||^2 (GTSAM NoiseModelFactor::error). err_dev may be NULL. */

/* KeypointProjectionFactor (factors.py:216-275): r = pi(K, Tcam^-1 Tbody p_b) - z,
 * J = d r / d Tbody (2x6).  K = (fx, fy, s, u0, v0); k_stride / tcam_stride = 0
 * share one K / camera pose across factors, 5 / 12 give one per factor; tcam_dev
 * NULL = identity camera (factors.py:211).  status[i] = 1 on cheirality (point
 * behind the camera: GTSAM CheiralityException), r and J then hold NaN. */
int pa_proj_linearize(int n, const double* tbody_dev, const double* pb_dev, const double* z_dev,
                      const double* k_dev, int k_stride, const double* tcam_dev, int tcam_stride,
                      const double* inv_sigma_dev, double* r_dev, double* j_dev, double* err_dev,
                      int32_t* status_dev, void* stream);

/* Robust noise models on the projection factor (GTSAM's noiseModel::Robust over a diagonal
 * model; the keypoints come from a CNN, and one occluded corner is tens of pixels off).  With
 * the whitened residual r_w = r * inv_sigma (unit sigma when inv_sigma is NULL), the whitened
 * Jacobian J_w, n = |r_w|_2 and k > 0 in whitened units:
 *   PA_ROBUST_HUBER   w = 1 if n <= k, else k / n;   rho = n^2 / 2 if n <= k, else k (n - k / 2)
 *   PA_ROBUST_CAUCHY  w = 1 / (1 + n^2 / k^2);       rho = (k^2 / 2) log1p(n^2 / k^2)
 * the outputs are r = sqrt(w) r_w, J = sqrt(w) J_w (Robust::WhitenSystem) and err = rho, NOT
 * 0.5 |r_w|^2.  status is unchanged: cheirality still gives NaN and status 1 (and in
 * pa_trajectory_linearize frames outside nvalid zeros and status 2).  Everything that consumes
 * the outputs (pa_trajectory_gn_step, pa_trajectory_marginals, the Levenberg-Marquardt cost,
 * the streaming ticks) then does iteratively reweighted least squares unchanged, without a
 * second-order (Triggs) term, as GTSAM does.  PA_ROBUST_NONE: the plain factor, bit for bit;
 * k is then ignored.  A kind outside the three, or a kind != PA_ROBUST_NONE with k not a
 * positive finite number, returns PA_EINVAL before any launch (every entry point that takes
 * the kind checks it the same way).
 * pa_proj_linearize_robust: pa_proj_linearize with the noise model's robust part. */
int pa_proj_linearize_robust(int n, const double* tbody_dev, const double* pb_dev, const double* z_dev,
                             const double* k_dev, int k_stride, const double* tcam_dev, int tcam_stride,
                             const double* inv_sigma_dev, int robust_kind, double robust_k, double* r_dev,
                             double* j_dev, double* err_dev, int32_t* status_dev, void* stream);

/* PoseDynamicsFactor (factors.py:54-142): r = Log((T1 Exp(dt[w; v_b]))^-1 T2),
 * v_b = R1^T v if vel_frame == PA_VEL_WORLD.  J0 6x6 (pose1), J1 6x3 (ang_vel1),
 * J2 6x3 (vel1), J3 6x6 (pose2); any J pointer may be NULL (error-only). */
int pa_dyn_linearize(int n, const double* t1_dev, const double* w_dev, const double* v_dev,
                     const double* t2_dev, double dt, int vel_frame, const double* inv_sigma_dev,
                     double* r_dev, double* j0_dev, double* j1_dev, double* j2_dev, double* j3_dev,
                     double* err_dev, void* stream);

/* pa_dyn_linearize with one dt per factor: dt_dev (n) device doubles (not validated: a
 * non-finite dt gives that factor NaN outputs). */
int pa_dyn_linearize_dt(int n, const double* t1_dev, const double* w_dev, const double* v_dev,
                        const double* t2_dev, const double* dt_dev, int vel_frame, const double* inv_sigma_dev,
                        double* r_dev, double* j0_dev, double* j1_dev, double* j2_dev, double* j3_dev,
                        double* err_dev, void* stream);

/* ConstantVelocityFactor (factors.py:160-171): r = v2 - v1, J0 = -I3, J1 = I3. */
int pa_cv_linearize(int n, const double* v1_dev, const double* v2_dev, const double* inv_sigma_dev,
                    double* r_dev, double* j0_dev, double* j1_dev, double* err_dev, void* stream);

/* Config 3: every factor of T trajectories x L frames in ONE launch,
 * keypoint measurements taken straight from the detector output y (B = T*L rows of
 * 2K normalized coordinates, denormalized on device as validate.py:144-153 does).
 * Per frame f (= t*L + l): K projection factors (corner k: p_b = corners[k], z =
 * pixel k of frame f, body pose pose[f]); per consecutive pair (l, l+1) of a
 * trajectory: one PoseDynamicsFactor (pose[f], angvel[f], vel[f], pose[f+1]) and
 * one ConstantVelocityFactor (vel[f], vel[f+1]).  Outputs use the per-factor
 * layouts of the batched entry points above; proj arrays have T*L*K rows, dyn
 * and cv arrays T*(L-1).  inv_sigma / err / J / status pointers may be NULL.
 * nvalid (may be NULL): per trajectory the number of trailing frames that hold a real
 * measurement (the streaming window before it has filled, pa_window_advance_n); the
 * projection factors of frames l < L - nvalid[t] get status 2 and r = J = err = 0, so the
 * GN step skips them.
 * robust_proj / robust_proj_k: the projection factors' robust noise model (see
 * pa_proj_linearize_robust: r_proj and j_proj are then sqrt(w)-scaled and err_proj is rho).  A
 * zero-initialised pair means none, so callers that never set them keep the plain factors.
 * Every entry point that takes a pa_traj_args (pa_trajectory_linearize, pa_trajectory_lm_solve,
 * pa_window_lm_solve, pa_window_pose_tick and its _pre / _post / _reduce forms) honours them
 * and rejects a bad pair with PA_EINVAL.
 * dt_pair / kp_mask: real timestamps (cameras drop frames, so consecutive frames are 1, 2 or 3
 * periods apart, and a hand hides single corners).  Both are device arrays read at every launch,
 * optional and independent; zero-initialised means none, as for the robust pair.
 *   dt_pair: the PoseDynamicsFactor of pair (l, l+1) of trajectory t uses dt_pair[t*(L-1)+l]
 *     instead of dt.  The contents are not validated on the host: a non-finite or non-positive
 *     value gives NaN factors and a non-zero info downstream, as a NaN pose does.
 *   kp_mask: bit k of kp_mask[t*L+l] set = keypoint k of frame l was measured.  A cleared bit gives
 *     that projection factor status 2 and r = J = err = 0, exactly the bits nvalid gives a frame
 *     outside the filled part; the two combine by OR of "off", and off wins over cheirality (a
 *     masked factor behind the camera has status 2, not 1).  Requires n_kp <= 32 (PA_EINVAL
 *     otherwise); bits at and above n_kp are ignored.
 *   dt_new / mask_new (T each): what the entry points that ADVANCE the window (pa_window_pose_tick,
 *     pa_window_pose_tick_pre and their _prior forms) store as the new last pair's dt and the
 *     new last frame's mask after shifting both rings one frame towards l = 0 with the window;
 *     dt_new[t] also predicts the new frame.  They return PA_EINVAL before any launch when
 *     exactly one of (dt_pair, dt_new) or exactly one of (kp_mask, mask_new) is NULL.  Every
 *     other entry point ignores the _new pair: pa_trajectory_linearize, the four LM solves and
 *     pa_window_pose_tick_reduce(_prior) do not advance, and pa_window_pose_tick_post lands the
 *     new keypoints on the frame its pre half already advanced, reading kp_mask there (it must be
 *     given the same dt_pair / kp_mask pointers as the pre half).  On the newest frame of a pre
 *     half the order of statuses is unchanged: the mask gives 2, the pre half then stamps 3 on
 *     all of that frame, and the post half re-evaluates with the mask.
 * isig_cw / r_cw / err_cw: the ConstantVelocityFactor on the ANGULAR velocity ("cw"; the reference's
 * factor, factors.py:145-171, is generic in its keys and GTSAM users put it on the angular-velocity
 * keys as well): per pair (l, l+1) of trajectory t, r = (angvel[l+1] - angvel[l]) * isig_cw, with the
 * constant Jacobians -diag(isig_cw) and +diag(isig_cw) (not written) and no dt scaling, also with
 * dt_pair.  r_cw != NULL switches it on, for every pair whatever nvalid, kp_mask or the statuses
 * say (as the factor on the linear velocity); a zero-initialised triple means off, and off is the
 * kernels and the bits from before the fields existed.  err_cw may be NULL; isig_cw NULL means
 * unwhitened in pa_trajectory_linearize only.  Every entry point that takes a pa_traj_args honours
 * it: the four LM solves (they require isig_cw and err_cw once it is on; err_cw's entries enter the
 * cost's fixed-order sum right after err_cv's) and pa_window_pose_tick with its _pre / _post /
 * _reduce / _prior forms (isig_cw required; the factor needs no keypoints, so the pre half has the
 * newest pair's).  Inconsistent fields return PA_EINVAL before any launch, after every older check.
 * The entry points with explicit pointer lists have the siblings pa_trajectory_gn_step_cw,
 * pa_trajectory_marginals_cw and pa_window_marginalize_cw below.
 * A frame without any measured keypoint is held by its two dynamics factors and the constant-
 * velocity factors alone.  WITHOUT the factor on the angular velocity its rotation is NOT
 * observable: nothing couples successive angular velocities, so frame l's rotation and the angular
 * velocities of frames l-1 and l can move together at no cost: 9 equations for the frame's 12
 * unknowns.  Such a frame then needs a lambda of the streaming tick's order (1e-2), exactly as a
 * partly filled window does (see pa_trajectory_marginals); the tick holds it at its prediction.
 * WITH the factor the three missing equations are there: the frame's rotation is observable through
 * its neighbours' (12 equations), its marginal covariance is finite at lambda -> 0, and partly filled
 * or timed windows no longer lean on the damping.  pa_trajectory_gn_step, pa_trajectory_marginals and
 * pa_window_marginalize consume statuses and factor outputs only and need nothing else. */
typedef struct pa_traj_args {
  int T, L, n_kp, H, W;
  const float* y;          /* (T*L, 2K) normalized keypoints */
  const double* pose;      /* (T*L, 12) */
  const double* vel;       /* (T*L, 3) linear velocity (vel_frame) */
  const double* angvel;    /* (T*L, 3) body angular velocity */
  const double* corners;   /* (K, 3) body-frame keypoints */
  const double* K;         /* (5) fx, fy, s, u0, v0 */
  const double* tcam;      /* (12) camera pose or NULL = identity */
  double dt;
  int vel_frame;
  const double* isig_proj; /* (2) or NULL */
  const double* isig_dyn;  /* (6) or NULL */
  const double* isig_cv;   /* (3) or NULL */
  const double* isig_cw;   /* (3) or NULL: the angular-velocity factor's whitening (see r_cw) */
  double *r_proj, *j_proj, *err_proj;
  int32_t* status;
  double *r_dyn, *j_dyn0, *j_dyn1, *j_dyn2, *j_dyn3, *err_dyn;
  /* the constant-velocity factor on the ANGULAR velocity ("cw"; r_cw NULL = off: every kernel and
   * output bit is then what it was before the field existed).  r_cw (T*(L-1), 3), err_cw (T*(L-1))
   * or NULL; its Jacobians are the constants -+ diag(isig_cw) and are not written. */
  double *r_cw, *err_cw;
  double *r_cv, *j_cv0, *j_cv1, *err_cv;
  /* real timestamps (all four NULL = none: every kernel, output bit and captured graph is then what
   * it was before these fields existed).  They stand before nvalid, not at the struct's end: the
   * struct still ends in nvalid, robust_proj, robust_proj_k, which tests/test_robust_capi.py pins. */
  const double* dt_pair;     /* (T*(L-1)) or NULL: pair (l, l+1) of trajectory t uses dt_pair[t*(L-1)+l], not dt */
  const uint32_t* kp_mask;   /* (T*L) or NULL: bit k of word t*L+l set = keypoint k of that frame was measured */
  const double* dt_new;      /* (T): the new last pair's dt; read only by entry points that advance the window */
  const uint32_t* mask_new;  /* (T): the new last frame's mask; read only by entry points that advance */
  const int32_t* nvalid;   /* (T) or NULL: frames with measurements, from the window's end */
  int robust_proj;         /* PA_ROBUST_*: the projection factors' robust noise model (0 = none) */
  double robust_proj_k;    /* its k > 0, in whitened units (host scalar; ignored for PA_ROBUST_NONE) */
} pa_traj_args;

int pa_trajectory_linearize(const pa_traj_args* args, void* stream);

/* Factor-graph consumer (the graph and optimizer are not in the
 * reference -- GTSAM's LM runs on the host -- so this build defines them): one damped
 * Gauss-Newton / LM step per trajectory from pa_trajectory_linearize's WHITENED outputs
 * (same layouts; every Jacobian required).  Per frame the variable block is
 * x = [pose tangent (6, [omega; v]) | angular velocity (3) | velocity (3)]; the step
 * solves (J^T J + lambda I) delta = -J^T r.  Outputs: D (T*L, 12, 12) diagonal and
 * E (T*(L-1), 12, 12) off-diagonal blocks of J^T J (E_l couples frame l rows with
 * frame l+1 columns), g (T*L, 12) = J^T r, delta (T*L, 12), info (T) = 0 or the
 * 1-based frame of a pivot block found not positive definite (delta NaN; which frame
 * depends on the elimination order: launches of few trajectories with L <= 24 run block
 * cyclic reduction, others a two-ended block elimination).  D, E and g
 * may all be NULL (then the blocks stay on chip: the step's HBM traffic is the factors in
 * and delta out).  Projection factors with status != 0 (cheirality, or a frame outside a
 * window's filled part) are skipped; with n_kp = 0 r_proj / j_proj may be NULL.
 * ws: pa_trajectory_gn_workspace. */
size_t pa_trajectory_gn_workspace(int T, int L);
int pa_trajectory_gn_step(int T, int L, int n_kp, const double* r_proj, const double* j_proj,
                          const int32_t* status_proj, const double* r_dyn, const double* j_dyn0,
                          const double* j_dyn1, const double* j_dyn2, const double* j_dyn3, const double* r_cv,
                          const double* j_cv0, const double* j_cv1, double lambda, double* D, double* E, double* g,
                          double* delta, int32_t* info, void* ws, size_t ws_bytes, void* stream);

/* Marginal covariances of the same graph (what gtsam.Marginals(graph, values)
 * .marginalCovariance(key) gives the reference's users on the host), per trajectory, from the
 * same WHITENED factors in the same order as pa_trajectory_gn_step (same layouts, same null
 * rules; projection factors with status != 0 are skipped):
 *   Sigma = (J^T J + lambda I)^-1,  lambda >= 0,
 * lambda I being an isotropic prior of precision lambda on every variable.  Outputs:
 * cov (T*L, 12, 12) the diagonal blocks Sigma_{l,l}, the marginal covariance of frame l's
 * [pose tangent (6, [omega; v]) | angular velocity (3) | velocity (3)] in the tangent space of
 * pa_window_retract's chart (a right perturbation, GTSAM's Pose3 convention); cross
 * (T*(L-1), 12, 12) or NULL, Sigma_{l,l+1} row-major with frame l on rows and frame l+1 on
 * columns (E's convention; requires cov); cov_newest (T, 12, 12) or NULL, Sigma_{L-1,L-1}
 * alone, bit for bit cov's last block (given without cov, only the forward elimination runs);
 * at least one of cov / cov_newest.  Every block is exactly symmetric.  info (T, required) = 0
 * or the 1-based frame whose pivot block of the top-down block elimination was not positive
 * definite; every output block of that trajectory is then NaN.
 * lambda = 0 has no special case.  Without the factor on the angular velocity (pa_traj_args.r_cw,
 * the _cw sibling below) the last frame's angular velocity of a full window is in no factor, so
 * lambda = 0 fails at frame L (as pa_trajectory_gn_step does); pass a small lambda (for example
 * 1e-9) for the undamped Gauss-Newton covariance -- the unconstrained variable is decoupled and
 * gets variance 1 / lambda.  Partly filled windows (nvalid < L) and a pending newest frame (status
 * 3) are then singular at lambda = 0 for a real reason (9 equations for 12 unknowns per frame
 * without keypoints) and need a lambda of the streaming tick's order (1e-2).  With the factor every
 * angular velocity is in a factor: lambda = 0 solves a full window (info 0), and frames without
 * keypoints between measured ones have finite variances at lambda -> 0.
 * T >= 0 (0 is a no-op), L >= 2, 0 <= n_kp <= 16; everything else returns PA_EINVAL before any
 * launch.  One launch on `stream`, no host synchronisation (capturable).
 * ws: pa_trajectory_marginals_workspace bytes. */
size_t pa_trajectory_marginals_workspace(int T, int L);
int pa_trajectory_marginals(int T, int L, int n_kp, const double* r_proj, const double* j_proj,
                            const int32_t* status_proj, const double* r_dyn, const double* j_dyn0,
                            const double* j_dyn1, const double* j_dyn2, const double* j_dyn3, const double* r_cv,
                            const double* j_cv0, const double* j_cv1, double lambda, double* cov, double* cross,
                            double* cov_newest, int32_t* info, void* ws, size_t ws_bytes, void* stream);

/* Levenberg-Marquardt over the same graph (what GTSAM's LevenbergMarquardtOptimizer::optimize
 * does on the host for the reference's users), per trajectory and independently, all on the
 * device: 1 + 2 max_iters launches on `stream`, no host synchronisation (capturable).
 * args: the pa_traj_args of pa_trajectory_linearize; isig_proj, isig_dyn and isig_cv are required
 * (the cost is defined on whitened residuals), as is every factor output and Jacobian pointer (r_cw,
 * err_cw and isig_cw only together, as the switch of the factor on the angular velocity); n_kp >= 1;
 * nvalid is honoured.  args->pose / vel / angvel are updated IN PLACE to the final accepted
 * state, and on return the factor outputs hold the linearization at that state.
 *   1. C = sum of err (0.5 |r_w|^2) over the dynamics and constant-velocity factors (with r_cw: those
 *      on the angular velocity too, right after the ones on the linear velocity) and the
 *      projection factors with status 0 at the state x (with args->robust_proj their err is the
 *      m-estimator's rho, so C is the robust cost); lambda = lambda0; cost0 = cost_hist[0] = C.
 *   2. iteration k = 1..max_iters: (J^T J + lambda I) delta = -J^T r (pa_trajectory_gn_step's
 *      system).  A failed pivot rejects the step.  Else x' = retract(x, delta) (pa_window_retract's
 *      arithmetic), C' = the cost at x'; x' is rejected if a projection factor with status 0 at x
 *      has status 1 (cheirality) at x'; otherwise it is accepted iff C' < C.
 *   3. accept: x = x', lambda = max(lambda / lambda_down, lambda_min), status CONVERGED and stop
 *      if C - C' <= rel_tol * |C| + abs_tol (C >= 0 without a prior); then C = C'.
 *   4. reject: lambda *= lambda_up, status STALLED and stop if that exceeds lambda_max; x stays.
 *   5. cost_hist[k] = C after the decision; entries after the stop are NaN.
 * A trajectory still running after iteration max_iters stops with MAX_ITERS.
 * Outputs (device, per trajectory): cost0, cost (final), iters (trial steps taken), status
 * (PA_LM_*), lambda (final; on STALLED the value that exceeded lambda_max), cost_hist
 * (T, max_iters + 1) or NULL.  2 <= L <= 24, 1 <= n_kp <= 16, any T >= 1 (one workgroup per
 * trajectory); a finished trajectory's workgroups return at once in the later launches.
 * Everything else returns PA_EINVAL before any launch; T = 0 is a no-op.
 * ws: pa_trajectory_lm_workspace bytes (0 for shapes outside the limits), 16-byte aligned. */
typedef struct pa_lm_params {
  int max_iters;        /* >= 1; every trial step, accepted or not, counts as one */
  double lambda0;       /* > 0 initial damping, per trajectory */
  double lambda_up;     /* > 1, on reject / failed pivot */
  double lambda_down;   /* > 1, on accept: lambda /= lambda_down */
  double lambda_min, lambda_max;
  double rel_tol, abs_tol; /* stop after an ACCEPTED step with C - C' <= rel_tol*C + abs_tol */
} pa_lm_params;

#define PA_LM_CONVERGED 1   /* stopped by rel_tol / abs_tol                  */
#define PA_LM_MAX_ITERS 2   /* ran out of iterations                          */
#define PA_LM_STALLED   3   /* lambda would exceed lambda_max                 */

size_t pa_trajectory_lm_workspace(int T, int L, int n_kp, int max_iters);
int pa_trajectory_lm_solve(const pa_traj_args* args, const pa_lm_params* p,
                           double* cost0_dev, double* cost_dev, int32_t* iters_dev,
                           int32_t* status_dev, double* lambda_dev,
                           double* cost_hist_dev /* (T, max_iters+1) or NULL */,
                           void* ws_dev, size_t ws_bytes, void* stream);
/* The same solve on a streaming window.  newest_pending != 0: the window is the one
 * pa_window_pose_tick_pre leaves between ticks (advanced, frame L-1 predicted, its keypoint slot
 * still stale): frame L-1's projection factors get status 3 and stay out of the cost, the guard
 * and the step, so frame L-1 is held by its dynamics factor alone.  On return the factor outputs
 * are what the pre half's linearize leaves at the solved window; pa_window_pose_tick_reduce then
 * rebuilds the reduced system for the post half.  newest_pending = 0: pa_trajectory_lm_solve. */
int pa_window_lm_solve(const pa_traj_args* args, const pa_lm_params* p, int newest_pending,
                       double* cost0_dev, double* cost_dev, int32_t* iters_dev, int32_t* status_dev,
                       double* lambda_dev, double* cost_hist_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* Fixed-lag window of the config-4 streaming pose stage (the smoother loop the reference
 * leaves to downstream GTSAM code; scripts/streaming.py:121-155 runs the detector only).
 * Per trajectory t the window holds frames l = 0..L-1 of y (T*L, 2K) f32, pose (T*L, 12),
 * angvel and vel (T*L, 3), all device, frame f = t*L + l.
 * pa_window_advance: shifts every array one frame towards l = 0 (frame 0 dropped),
 * writes y_new[t] (T, 2K) as frame L-1 and predicts pose[L-1] = pose[L-2] Exp(dt [w; v_b])
 * (the PoseDynamicsFactor model, factors.py:100-105; v_b = R^T v for PA_VEL_WORLD), v = vel
 * of frame L-2 carried over and w = the angular velocity frame L-2 held before the shift
 * (the newest one a factor constrains; L >= 3), which frames L-2 and L-1 both take.
 * pa_window_retract: pose <- pose Exp(delta[0:6]) (Pose3 retract, Expmap chart),
 * angvel += delta[6:9], vel += delta[9:12] for pa_trajectory_gn_step's delta (T*L, 12);
 * trajectories with info[t] != 0 are left unchanged (info may be NULL). */
int pa_window_advance(int T, int L, int n_kp, const float* y_new_dev, float* y_dev, double* pose_dev,
                      double* angvel_dev, double* vel_dev, double dt, int vel_frame, void* stream);
/* pa_window_advance that also counts the window's real frames: nvalid_dev (T) int32 += 1 up
 * to L per advance (zero it with the window's reset; pa_traj_args.nvalid reads it). */
int pa_window_advance_n(int T, int L, int n_kp, const float* y_new_dev, float* y_dev, double* pose_dev,
                        double* angvel_dev, double* vel_dev, int32_t* nvalid_dev, double dt, int vel_frame,
                        void* stream);
/* pa_window_advance_n with the rings of pa_traj_args' real timestamps: dt_pair_dev (T*(L-1)) and
 * kp_mask_dev (T*L) shift one frame towards l = 0 with the window, dt_new_dev[t] lands at pair
 * L-2 and mask_new_dev[t] at frame L-1, and frame L-1 is predicted with dt_new_dev[t] instead
 * of dt.  Either ring may be absent: (dt_pair_dev, dt_new_dev) are given together or both NULL,
 * and so are (kp_mask_dev, mask_new_dev), else PA_EINVAL before any launch; without the dt ring
 * the prediction uses dt.  nvalid_dev may be NULL. */
int pa_window_advance_t(int T, int L, int n_kp, const float* y_new_dev, float* y_dev, double* pose_dev,
                        double* angvel_dev, double* vel_dev, int32_t* nvalid_dev, double* dt_pair_dev,
                        uint32_t* kp_mask_dev, const double* dt_new_dev, const uint32_t* mask_new_dev, double dt,
                        int vel_frame, void* stream);
int pa_window_retract(int T, int L, const double* delta_dev, const int32_t* info_dev, double* pose_dev,
                      double* angvel_dev, double* vel_dev, void* stream);
/* pa_window_retract that also writes each trajectory's newest (last-frame) pose after the
 * update to newest_pose_dev (T, 12) -- the streaming tick's pose output, no strided gather. */
int pa_window_retract_newest(int T, int L, const double* delta_dev, const int32_t* info_dev, double* pose_dev,
                             double* angvel_dev, double* vel_dev, double* newest_pose_dev, void* stream);

/* One streaming tick's pose stage (config 4) in two launches, bit for bit the sequence
 * pa_window_advance_n(y_new) -> pa_trajectory_linearize(args) -> pa_trajectory_gn_step
 * (lambda; delta, info; D / E / g not written) -> pa_window_retract_newest(newest_pose).
 * args: the window's pa_traj_args (args->y / pose / vel / angvel ARE the window arrays,
 * advanced and retracted in place; nvalid required; every factor output and Jacobian
 * required, whitening as the caller wants it for the GN step).  T <= the device's CU count,
 * 2 <= L <= 24, n_kp <= 16 (PA_EINVAL otherwise: use the four calls). */
int pa_window_pose_tick(const pa_traj_args* args, const float* y_new_dev, double lambda, double* delta_dev,
                        int32_t* info_dev, double* newest_pose_dev, void* stream);

/* The same tick split around the keypoints, so that most of it runs before they exist (the
 * streaming graph runs the pre half on a second stream beside the detector forward):
 *   pa_window_pose_tick_pre: the window advances WITHOUT the new keypoints, every factor but
 *     frame L-1's projections is linearized (those are marked status 3 for now), and the GN
 *     system is assembled and reduced by block cyclic reduction down to frame L-1 (the root),
 *     into ws (pa_window_pose_tick_workspace bytes);
 *   pa_window_pose_tick_post: y_new lands as frame L-1's keypoints, its projection factors
 *     are linearized into the factor outputs (as pa_trajectory_linearize writes them), added
 *     to the reduced root, and the step is solved (delta, info) and retracted (newest_pose).
 * Pre then post on the same window = pa_window_pose_tick up to f64 rounding (another
 * elimination order; the window's keypoints and factor outputs are bit-identical; info names
 * a frame whose pivot failed in that order).  Same limits as pa_window_pose_tick. */
size_t pa_window_pose_tick_workspace(int T, int L);
int pa_window_pose_tick_pre(const pa_traj_args* args, double lambda, void* ws_dev, size_t ws_bytes, void* stream);
int pa_window_pose_tick_post(const pa_traj_args* args, const float* y_new_dev, const void* ws_dev, size_t ws_bytes,
                             double* delta_dev, int32_t* info_dev, double* newest_pose_dev, void* stream);
/* The second launch of pa_window_pose_tick_pre alone: the GN system assembled from the factor
 * outputs AS THEY STAND and reduced to frame L-1 into ws; the window does not advance and nothing
 * is linearized.  After pa_window_pose_tick_pre it rewrites the same ws bit for bit; after
 * pa_window_lm_solve (newest_pending) it prepares the post half for the solved window. */
int pa_window_pose_tick_reduce(const pa_traj_args* args, double lambda, void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------- fixed-lag marginalization
 * What GTSAM's BatchFixedLagSmoother / IncrementalFixedLagSmoother do when the oldest state leaves
 * the lag: it is marginalized, and the Schur complement of its factors stays behind as a linear
 * prior on the state that is now oldest (a LinearContainerFactor with its linearization point),
 * instead of pa_window_advance simply forgetting frame 0.
 * The prior is held per trajectory, f64, on the device, in INFORMATION form (the marginal is only
 * positive semi-definite -- without the factor on the angular velocity (pa_window_marginalize_cw)
 * frame 1's angular velocity gets no information from frame 0; with it, it gets the factor's --
 * so the form that always exists is kept):
 *   info (T, 12, 12) row-major, the symmetric Lambda over the frame block [pose tangent 6 |
 *   angvel 3 | vel 3] in pa_window_retract's chart;  eta (T, 12);  xbar_pose (T, 12), xbar_angvel
 *   (T, 3), xbar_vel (T, 3): the state it was linearized at.
 * With xi = [Logmap(xbar_pose^-1 pose); angvel - xbar_angvel; vel - xbar_vel] the prior's cost is
 * 0.5 xi^T Lambda xi - eta^T xi.  As LinearContainerFactor does, Lambda is kept fixed and the
 * chart's Jacobian is taken as the identity, so at a state x the prior contributes
 *   D_0 += Lambda,  g_0 += Lambda xi - eta
 * to the normal equations of pa_trajectory_gn_step (frame 0's blocks).
 *
 * pa_window_prior_linearize: xi of window frame `frame` (0 <= frame < L; pose (T*L, 12), angvel,
 * vel (T*L, 3)) against xbar, grad (T, 12) = Lambda xi - eta and err (T) or NULL = 0.5 xi^T Lambda xi
 * - eta^T xi.  One launch, no host synchronisation. */
int pa_window_prior_linearize(int T, int L, int frame, const double* info, const double* eta,
                              const double* xbar_pose, const double* xbar_angvel, const double* xbar_vel,
                              const double* pose, const double* angvel, const double* vel, double* grad_out,
                              double* err_out, void* stream);

/* pa_window_marginalize: marginalizes frame 0 of every trajectory's window, from the WHITENED
 * factor outputs pa_trajectory_gn_step takes (same layouts and null rules; status != 0 skipped)
 * and the prior the window carried so far (prior_info_in (T, 12, 12), prior_grad_in (T, 12): its
 * gradient at the factors' linearization point; both NULL = no prior yet):
 *   H = D_0 + Lambda_in + lambda I,   F = B^T B,  h = B^T r  (B: the x_1 part of the dynamics and
 *   constant-velocity factors (0, 1), r their residuals),
 *   Lambda' = F - E_0^T H^-1 E_0  (exactly symmetric),   g' = h - E_0^T H^-1 (g_0 + grad_in).
 * delta (T*L, 12) or NULL with gn_info (T) or NULL: the step the window was retracted by after the
 * factors were linearized; where given and gn_info[t] == 0 (or gn_info NULL), the prior is
 * re-centred to first order at the retracted state, g' += Lambda' delta[t, frame 1].
 * Outputs: info_out = Lambda', eta_out = -g', xbar_* = window frame 1's state (pose (T*L, 12),
 * angvel, vel (T*L, 3)) as it stands, and minfo (T): 0 = computed; 1 = H not positive definite;
 * 2 = nvalid[t] < L (nvalid (T) or NULL: the window is not full, frame 0 is a copy of the initial
 * guess and no measurement).  In both non-zero cases the new prior is zero (xbar still written).
 * Solving frames 1..L-1's own factors with this prior on frame 1 gives the delta that solving
 * all L frames with the input prior gives for them (the Schur complement identity).
 * T >= 0 (0 is a no-op), L >= 2, 0 <= n_kp <= 16, lambda >= 0; everything else returns PA_EINVAL
 * before any launch.  One launch, one workgroup per trajectory, no host synchronisation. */
int pa_window_marginalize(int T, int L, int n_kp, const double* r_proj, const double* j_proj,
                          const int32_t* status_proj, const double* r_dyn, const double* j_dyn0,
                          const double* j_dyn1, const double* j_dyn2, const double* j_dyn3, const double* r_cv,
                          const double* j_cv0, const double* j_cv1, const double* prior_info_in,
                          const double* prior_grad_in, double lambda, const double* delta, const int32_t* gn_info,
                          const int32_t* nvalid, const double* pose, const double* angvel, const double* vel,
                          double* info_out, double* eta_out, double* xbar_pose_out, double* xbar_angvel_out,
                          double* xbar_vel_out, int32_t* minfo, void* stream);

/* pa_trajectory_gn_step / pa_trajectory_marginals and the streaming ticks with the prior on
 * frame 0: the parent plus prior_info (T, 12, 12) and prior_grad (T, 12), given together; both NULL
 * is the parent, bit for bit.  (pa_traj_args itself is unchanged: the prior travels beside it.
 * pa_window_pose_tick_post needs no sibling, the prior is in the system the pre half reduced.)
 * pa_trajectory_lm_solve and pa_window_lm_solve have their siblings too, pa_trajectory_lm_prior_solve
 * and pa_window_lm_prior_solve below: their cost needs the prior's err and a re-linearization per
 * iteration, so they take the whole prior (pa_lm_prior), not its gradient.  (Named ..._lm_prior_solve,
 * after pa_trajectory_lm_prior_workspace, not ..._lm_solve_prior: the two-pointer convention of the
 * _prior siblings here does not fit them, and tests/test_prior_capi.py pins that no entry point
 * of that name takes it.) */
int pa_trajectory_gn_step_prior(int T, int L, int n_kp, const double* r_proj, const double* j_proj,
                                const int32_t* status_proj, const double* r_dyn, const double* j_dyn0,
                                const double* j_dyn1, const double* j_dyn2, const double* j_dyn3,
                                const double* r_cv, const double* j_cv0, const double* j_cv1, double lambda,
                                double* D, double* E, double* g, double* delta, int32_t* info, void* ws,
                                size_t ws_bytes, const double* prior_info, const double* prior_grad, void* stream);
int pa_trajectory_marginals_prior(int T, int L, int n_kp, const double* r_proj, const double* j_proj,
                                  const int32_t* status_proj, const double* r_dyn, const double* j_dyn0,
                                  const double* j_dyn1, const double* j_dyn2, const double* j_dyn3,
                                  const double* r_cv, const double* j_cv0, const double* j_cv1, double lambda,
                                  double* cov, double* cross, double* cov_newest, int32_t* info, void* ws,
                                  size_t ws_bytes, const double* prior_info, const double* prior_grad,
                                  void* stream);
/* The same three with the ConstantVelocityFactor on the angular velocity (pa_traj_args.r_cw): the
 * _prior argument lists plus r_cw (T*(L-1), 3), the factor's WHITENED residuals as
 * pa_trajectory_linearize writes them, and isig_cw (3), its whitening (required with r_cw: the
 * Jacobians are -+ diag(isig_cw)), both before lambda.  The factor has constant Jacobians, so it is
 * folded into the blocks in closed form: per pair touching frame l, D_l[6+i][6+i] += isig_cw_i^2,
 * E_l[6+i][6+i] -= isig_cw_i^2 and g_l[6+i] += isig_cw_i (r_{l-1,i} - r_{l,i}) (a term left out at
 * the window's ends); for pa_window_marginalize_cw, F = B^T B and h = B^T r gain the pair (0, 1)'s
 * frame-1 part.  Prior pointers both NULL: no prior.  r_cw NULL: the _prior parent (for
 * pa_window_marginalize_cw: pa_window_marginalize), bit for bit.  Workspace sizes: the parents'. */
int pa_trajectory_gn_step_cw(int T, int L, int n_kp, const double* r_proj, const double* j_proj,
                             const int32_t* status_proj, const double* r_dyn, const double* j_dyn0,
                             const double* j_dyn1, const double* j_dyn2, const double* j_dyn3, const double* r_cv,
                             const double* j_cv0, const double* j_cv1, const double* r_cw, const double* isig_cw,
                             double lambda, double* D, double* E, double* g, double* delta, int32_t* info, void* ws,
                             size_t ws_bytes, const double* prior_info, const double* prior_grad, void* stream);
int pa_trajectory_marginals_cw(int T, int L, int n_kp, const double* r_proj, const double* j_proj,
                               const int32_t* status_proj, const double* r_dyn, const double* j_dyn0,
                               const double* j_dyn1, const double* j_dyn2, const double* j_dyn3, const double* r_cv,
                               const double* j_cv0, const double* j_cv1, const double* r_cw, const double* isig_cw,
                               double lambda, double* cov, double* cross, double* cov_newest, int32_t* info, void* ws,
                               size_t ws_bytes, const double* prior_info, const double* prior_grad, void* stream);
int pa_window_marginalize_cw(int T, int L, int n_kp, const double* r_proj, const double* j_proj,
                             const int32_t* status_proj, const double* r_dyn, const double* j_dyn0,
                             const double* j_dyn1, const double* j_dyn2, const double* j_dyn3, const double* r_cv,
                             const double* j_cv0, const double* j_cv1, const double* prior_info_in,
                             const double* prior_grad_in, const double* r_cw, const double* isig_cw, double lambda,
                             const double* delta, const int32_t* gn_info, const int32_t* nvalid, const double* pose,
                             const double* angvel, const double* vel, double* info_out, double* eta_out,
                             double* xbar_pose_out, double* xbar_angvel_out, double* xbar_vel_out, int32_t* minfo,
                             void* stream);
int pa_window_pose_tick_prior(const pa_traj_args* args, const float* y_new_dev, double lambda, double* delta_dev,
                              int32_t* info_dev, double* newest_pose_dev, const double* prior_info,
                              const double* prior_grad, void* stream);
int pa_window_pose_tick_pre_prior(const pa_traj_args* args, double lambda, void* ws_dev, size_t ws_bytes,
                                  const double* prior_info, const double* prior_grad, void* stream);
int pa_window_pose_tick_reduce_prior(const pa_traj_args* args, double lambda, void* ws_dev, size_t ws_bytes,
                                     const double* prior_info, const double* prior_grad, void* stream);


/* Levenberg-Marquardt with the marginalization prior on frame 0: what GTSAM's BatchFixedLagSmoother
 * runs on the host, an LM solve over the window's factors plus the marginal prior.  The parents'
 * steps 1-5 (pa_trajectory_lm_solve above) with three additions:
 *   cost  C = (the parent's sum, in its fixed order) + e_prior,
 *         e_prior = sum_i xi_i (0.5 (Lambda xi)_i - eta_i), xi taken at frame 0 of the state being
 *         evaluated, in exactly pa_window_prior_linearize's operation order (the same device code);
 *         e_prior is added last, unfused.
 *   step  (J^T J + lambda I + Lambda on frame 0) delta = -(J^T r + (Lambda xi - eta) on frame 0), xi at
 *         the CURRENT state x (pa_trajectory_gn_step_prior's system): the gradient is re-evaluated
 *         with every trial state and kept with an accepted one.
 *   sign  -eta^T xi has no lower bound, so C can be negative: the convergence test of step 3 is
 *         C - C' <= rel_tol * |C| + abs_tol (for the parents C >= 0: the same bits).  The accept test
 *         stays C' < C.
 * prior == NULL is the parent, bit for bit, and accepts the parent's workspace size; the parents
 * are calls of these with NULL.  A non-null prior needs info, eta, xbar_* and grad (PA_EINVAL
 * before any launch otherwise) and pa_trajectory_lm_prior_workspace bytes (>= the parent's; 0
 * outside the limits).  On return grad / err hold the prior's gradient and cost at frame 0 of the
 * final accepted state, bit for bit what pa_window_prior_linearize(frame 0) gives there: grad is
 * the prior_grad_in that pa_window_marginalize takes with the factor outputs the solve leaves.
 * Limits, nvalid, robust_proj, newest_pending, launch count (1 + 2 max_iters, capturable): the
 * parents'. */
typedef struct pa_lm_prior {
  const double* info;        /* (T,12,12) Lambda, row-major, symmetric              */
  const double* eta;         /* (T,12)                                              */
  const double* xbar_pose;   /* (T,12)  the state the prior was linearized at       */
  const double* xbar_angvel; /* (T,3)                                               */
  const double* xbar_vel;    /* (T,3)                                               */
  double* grad;              /* (T,12) OUT, required: Lambda xi - eta at the final accepted state */
  double* err;               /* (T)    OUT or NULL: 0.5 xi'Lambda xi - eta'xi there */
} pa_lm_prior;

size_t pa_trajectory_lm_prior_workspace(int T, int L, int n_kp, int max_iters);
int pa_trajectory_lm_prior_solve(const pa_traj_args* args, const pa_lm_params* p, const pa_lm_prior* prior,
                                 double* cost0_dev, double* cost_dev, int32_t* iters_dev, int32_t* status_dev,
                                 double* lambda_dev, double* cost_hist_dev, void* ws_dev, size_t ws_bytes,
                                 void* stream);
int pa_window_lm_prior_solve(const pa_traj_args* args, const pa_lm_params* p, int newest_pending,
                             const pa_lm_prior* prior, double* cost0_dev, double* cost_dev, int32_t* iters_dev,
                             int32_t* status_dev, double* lambda_dev, double* cost_hist_dev, void* ws_dev,
                             size_t ws_bytes, void* stream);

/* ------------------------------------------------- prediction and keypoint gate
 * pa_window_predict: the newest state of every trajectory's window, predicted Q horizons ahead with
 * the PoseDynamicsFactor model pa_window_advance predicts the new frame with, and its covariance.
 * The state a prediction starts from is the one pa_window_advance starts from (see there): pose and
 * velocity of frame L-1, the angular velocity of frame L-2 (frame L-1's enters no factor; L = 2:
 * frame 1's).  Per trajectory t and query q, tau = tau[t*Q+q] seconds (device, not validated: a
 * non-finite tau gives NaN outputs):
 *   pose_out[t*Q+q] = T Exp(tau [w; v_b]),  v_b = R^T v for PA_VEL_WORLD,
 * in the advance's operation order: for tau equal to the dt of an advance it is bit for bit the frame
 * pa_window_advance_t predicts, for tau = 0 the input pose.
 * Covariance (cov_out (T*Q, 12, 12) or NULL; needs cov and cross, pa_trajectory_marginals' outputs
 * (T*L, 12, 12) and (T*(L-1), 12, 12), given together or both NULL, and then L >= 3): the predicted
 * state is x' = [pose' (right perturbation, [omega; v]) | w | v], and to first order
 *   F = [[-J0, -J1, -J2], [0, I, 0], [0, 0, I]],
 * J0, J1, J2 the unwhitened PoseDynamicsFactor Jacobians at (T, w, v, pose2 = pose', dt = tau), where
 * the residual is zero and J3 = I.  The input covariance Sigma* (12 x 12) is a principal sub-block of
 * the window's full covariance: pose and velocity rows / columns from cov[L-1], the angular velocity
 * block from cov[L-2][6:9, 6:9], the two coupled through cross[L-2][6:9, :]; the symmetric blocks are
 * read from their upper triangles.
 *   cov_out = F Sigma* F^T + diag(q_diag),
 * q_diag (12, device, or NULL = none) process-noise variances; every block is exactly symmetric.
 * cov_info (T) or NULL: pa_trajectory_marginals' info; a trajectory with cov_info != 0 gets NaN in
 * cov_out (its poses are still predicted).
 * PA_EINVAL before any launch: T < 0, Q < 1, L < 2; exactly one of cov / cross; cov_out without
 * them; cov with L < 3; a bad vel_frame; a NULL pose, angvel, vel, tau or pose_out.  T = 0 is a
 * no-op.  One launch (one lane per (t, q)), no host synchronisation (capturable). */
int pa_window_predict(int T, int L, int Q, const double* pose, const double* angvel, const double* vel,
                      const double* cov, const double* cross, const int32_t* cov_info, const double* q_diag,
                      const double* tau, int vel_frame, double* pose_out, double* cov_out, void* stream);

/* pa_keypoint_gate: an innovation (chi-square) test of the detector's keypoints against a predicted
 * pose, clearing the mask bits (pa_traj_args.kp_mask / mask_new) of the corners that fail it.
 * Inputs per trajectory t: y_new (T, 2K) f32 normalized keypoints; the predicted pose at
 * pose_pred + t*pose_stride (doubles, pose_stride >= 12); cov_pred (T, 12, 12), of which the 6 x 6
 * pose block P is used (pa_window_predict's cov_out); corners, K, tcam (NULL = identity) and
 * isig_proj (2, required: the inverse pixel sigmas) as in pa_traj_args; the mask word at
 * mask + t*mask_stride (mask_stride >= 1), in and out.  Both strides exist so that the gate can act
 * on the new-frame block (mask_new, strides 1 and 12) before a fused tick, or on the ring entry
 * kp_mask[t*L + L-1] (mask stride L, pose stride 12 L) between the two halves of a split tick.
 * Per keypoint k < n_kp whose bit is set in the incoming word: z = the pixel of y_new (f32 kornia
 * denormalize, as pa_trajectory_linearize); (zhat, H 2 x 6) the unwhitened KeypointProjectionFactor
 * at the predicted pose; S = H P H^T + diag(sigma_u^2, sigma_v^2); d2 = (zhat - z)^T S^-1 (zhat - z)
 * by the closed 2 x 2 form.  The keypoint passes iff there is no cheirality at the predicted pose, S
 * is finite with a positive determinant, and d2 <= chi2; d2 is NaN where it could not be formed.
 * Outputs: the mask word & the pass bits below n_kp (bits at and above n_kp are copied through);
 * d2 (T, K) or NULL, NaN for a bit that came in cleared; zhat (T, K, 2) or NULL, the predicted pixel
 * of every corner whatever its bit (NaN on cheirality); ginfo (T, required).
 * The gate abstains -- the mask word is left as it came -- and says why in ginfo, the first reason
 * in this order winning:
 *   PA_GATE_YOUNG   nvalid[t] < min_frames (nvalid (T) or NULL = never young); d2 NaN
 *   PA_GATE_NOCOV   a non-finite entry in P; d2 NaN
 *   PA_GATE_FEW     fewer than min(min_pass, popcount(incoming word's bits below n_kp)) keypoints
 *                   pass (a lost track: without it a track whose every corner is gated could never
 *                   recover); d2 still written
 *   PA_GATE_APPLIED otherwise.
 * PA_EINVAL before any launch: T < 0; n_kp outside [1, 32]; chi2 not a positive finite number;
 * min_pass < 0; pose_stride < 12; mask_stride < 1; a NULL required pointer.  T = 0 is a no-op.
 * One launch (32 lanes per trajectory, corner k on lane k), no host synchronisation (capturable). */
#define PA_GATE_APPLIED 0
#define PA_GATE_FEW 1
#define PA_GATE_NOCOV 2
#define PA_GATE_YOUNG 3
int pa_keypoint_gate(int T, int n_kp, int H, int W, const float* y_new, const double* pose_pred, long pose_stride,
                     const double* cov_pred, const double* corners, const double* K, const double* tcam,
                     const double* isig_proj, double chi2, int min_pass, const int32_t* nvalid, int min_frames,
                     uint32_t* mask, long mask_stride, double* d2, double* zhat, int32_t* ginfo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERSEUS_AMD_H */
