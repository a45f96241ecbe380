// Prediction of a window's newest state with its covariance (pa_window_predict) and the
// chi-square gate of the detector's keypoints against it (pa_keypoint_gate), all f64.
//
// The prediction is the PoseDynamicsFactor model (factors.py:100-105) that pa_window_advance
// predicts the new frame with, from the same state: pose and velocity of frame L-1, the angular
// velocity of frame L-2 (frame L-1's enters no factor; L = 2: frame 1's).  Its covariance is the
// first-order propagation of the window's marginals through that map, with the factor's own
// Jacobians: at pose2 = the predicted pose the residual is zero and J3 = I, so the predicted
// pose's perturbation is -(J0 d_pose + J1 d_angvel + J2 d_vel).
#include "factors_dev.h"

namespace pa {

// pose[L-1] Exp(dt [w; v_b]): window_advance_body's prediction, statement for statement, and kept
// out of line, so that the compiler contracts the same products in both places and a horizon equal
// to an advance's dt gives the advance's frame bit for bit.
__device__ __noinline__ void predict_pose(const double* __restrict__ Tp, const double* __restrict__ wp,
                                          const double* __restrict__ vp, double dt, int vel_frame,
                                          double* __restrict__ o) {
  const Pose T1 = load_pose(Tp);
  const V3 w = load3(wp), v = load3(vp);
  const V3 vb = vel_frame == PA_VEL_WORLD ? mtv(T1.R, v) : v;
  const V3 xw = dt * w, xv = dt * vb;
  const Pose P = compose(T1, pose_exp(xw, xv, ang(xw)));
#pragma unroll
  for (int i = 0; i < 9; ++i) o[i] = P.R.a[i];
  o[9] = P.t.x;
  o[10] = P.t.y;
  o[11] = P.t.z;
}

struct PredictArgs {
  int T, L, Q;
  const double *pose, *angvel, *vel, *cov, *cross;
  const int32_t* cov_info;
  const double *q_diag, *tau;
  int vel_frame;
  double *pose_out, *cov_out;
};

// One lane per (trajectory t, query q).
__global__ __launch_bounds__(64) void window_predict_kernel(PredictArgs a) {
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= (long)a.T * a.Q) return;
  const long t = i / a.Q;
  const long fp = t * a.L + a.L - 1;                      // pose and velocity: frame L-1
  const long fw = t * a.L + (a.L >= 3 ? a.L - 2 : a.L - 1);  // angular velocity: frame L-2 (L = 2: frame 1)
  const double tau = a.tau[i];
  const double* Tp = a.pose + fp * 12;
  const double* wp = a.angvel + fw * 3;
  const double* vp = a.vel + fp * 3;
  double* po = a.pose_out + i * 12;
  predict_pose(Tp, wp, vp, tau, a.vel_frame, po);
  if (!a.cov_out) return;
  double* co = a.cov_out + i * 144;
  if (a.cov_info && a.cov_info[t] != 0) {
    const double nan = __builtin_nan("");
    for (int k = 0; k < 144; ++k) co[k] = nan;
    return;
  }
  // the unwhitened PoseDynamicsFactor Jacobians at (T, w, v, pose2 = the prediction, dt = tau)
  double r[6], J0[36], J1[18], J2[18];
  dyn_one(Tp, wp, vp, po, tau, a.vel_frame, nullptr, r, J0, J1, J2, nullptr, nullptr);
  // Everything below is fully unrolled with constant indices, so A, M and the Jacobians live in
  // registers (rolled loops index them dynamically and put them in the private segment: 2 KB per
  // lane and 28 us per launch against 13), and Sigma* is read element by element where it is used.
  // A = [-J0 | -J1 | -J2] (6 x 12), the dense rows of F = [[A], [0 I]]
  double A[6][12];
#pragma unroll
  for (int c = 0; c < 12; ++c)
#pragma unroll
    for (int rr = 0; rr < 6; ++rr)
      A[rr][c] = -(c < 6 ? J0[c * 6 + rr] : c < 9 ? J1[(c - 6) * 6 + rr] : J2[(c - 9) * 6 + rr]);
  // Sigma*: pose and velocity from cov[L-1], the angular velocity from cov[L-2][6:9, 6:9], the two
  // coupled through cross[L-2][6:9, :] (frame L-2 on rows).  The symmetric blocks are read from
  // their upper triangles, so Sigma* is symmetric whatever the caller passes.
  const double* c1 = a.cov + fp * 144;
  const double* c2 = a.cov + (fp - 1) * 144;
  const double* cx = a.cross + (t * (a.L - 1) + a.L - 2) * 144;
  auto sig = [&](int p, int q) __attribute__((always_inline)) -> double {
    const int lo = p < q ? p : q, hi = p < q ? q : p;
    const bool wl = lo >= 6 && lo < 9, wh = hi >= 6 && hi < 9;
    return wl && wh ? c2[lo * 12 + hi] : !wl && !wh ? c1[lo * 12 + hi] : wl ? cx[lo * 12 + hi] : cx[hi * 12 + lo];
  };
  double M[6][12];  // A Sigma*
#pragma unroll
  for (int c = 0; c < 12; ++c) {
    double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const double sk = sig(k, c);
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) m[rr] += A[rr][k] * sk;
    }
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) M[rr][c] = m[rr];
  }
  // F Sigma* F^T = [[M A^T, M[:, 6:]], [., Sigma*[6:, 6:]]] + diag(q), written exactly symmetric
  double q[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) q[k] = a.q_diag ? a.q_diag[k] : 0.0;
#pragma unroll
  for (int rr = 0; rr < 6; ++rr)
#pragma unroll
    for (int c = rr; c < 6; ++c) {
      double sm = 0.0;
#pragma unroll
      for (int k = 0; k < 12; ++k) sm += M[rr][k] * A[c][k];
      if (rr == c) sm += q[rr];
      co[rr * 12 + c] = sm;
      co[c * 12 + rr] = sm;
    }
#pragma unroll
  for (int rr = 0; rr < 6; ++rr)
#pragma unroll
    for (int c = 6; c < 12; ++c) {
      co[rr * 12 + c] = M[rr][c];
      co[c * 12 + rr] = M[rr][c];
    }
#pragma unroll
  for (int rr = 6; rr < 12; ++rr)
#pragma unroll
    for (int c = rr; c < 12; ++c) {
      const double sm = sig(rr, c) + (rr == c ? q[rr] : 0.0);
      co[rr * 12 + c] = sm;
      co[c * 12 + rr] = sm;
    }
}

struct GateArgs {
  int T, n_kp, H, W;
  const float* y_new;
  const double* pose_pred;
  long pose_stride;
  const double *cov_pred, *corners, *K, *tcam, *isig_proj;
  double chi2;
  int min_pass;
  const int32_t* nvalid;
  int min_frames;
  uint32_t* mask;
  long mask_stride;
  double *d2, *zhat;
  int32_t* ginfo;
};

// Half a wave (32 lanes) per trajectory, corner k on lane k of its half, so a frame's corners sit
// in adjacent lanes and bit k of the half's ballot is corner k's verdict.
constexpr int GATE_TPB = 8;  // trajectories per workgroup of 256
__global__ __launch_bounds__(32 * GATE_TPB) void keypoint_gate_kernel(GateArgs a) {
  const int lane = threadIdx.x & 31;
  const long t = (long)blockIdx.x * GATE_TPB + (threadIdx.x >> 5);
  if (t >= a.T) return;  // (whole halves leave: the ballot below counts active lanes only)
  const bool kl = lane < a.n_kp;
  const int k = kl ? lane : a.n_kp - 1;  // spare lanes recompute the last corner, store nothing
  const uint32_t low = a.n_kp >= 32 ? 0xffffffffu : (1u << a.n_kp) - 1u;
  const uint32_t min = a.mask[t * a.mask_stride];
  const bool on = kl && ((min >> k) & 1u);
  const bool young = a.nvalid && a.nvalid[t] < a.min_frames;
  // the pose block of the predicted covariance
  const double* cp = a.cov_pred + t * 144;
  double P[6][6];
  bool fin = true;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      P[r][c] = cp[r * 12 + c];
      fin = fin && isfinite(P[r][c]);
    }
  const Pose Tb = load_pose(a.pose_pred + t * a.pose_stride);
  const Cam cam = load_cam<false>(a.K, a.tcam, nullptr, PA_ROBUST_NONE, 0.0);
  const V3 pb = load3(a.corners + 3 * k);
  const float* yf = a.y_new + (t * a.n_kp + k) * 2;
  const double zx = (double)kornia_denorm(yf[0], a.W), zy = (double)kornia_denorm(yf[1], a.H);
  // the unwhitened KeypointProjectionFactor against a zero measurement: r is the predicted pixel
  double zh[2], J[12], e;
  int32_t st;
  proj_eval<false>(Tb, pb, 0.0, 0.0, cam, zh, J, e, st);
  const double i0 = zh[0] - zx, i1 = zh[1] - zy;
  // S = H P H^T + diag(sigma_u^2, sigma_v^2), H (2 x 6) = J column-major
  double HP[2][6];
#pragma unroll
  for (int rr = 0; rr < 2; ++rr)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double s = 0.0;
#pragma unroll
      for (int d = 0; d < 6; ++d) s += J[d * 2 + rr] * P[d][c];
      HP[rr][c] = s;
    }
  double s00 = 0.0, s01 = 0.0, s11 = 0.0;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    s00 += HP[0][c] * J[c * 2];
    s01 += HP[0][c] * J[c * 2 + 1];
    s11 += HP[1][c] * J[c * 2 + 1];
  }
  const double iu = a.isig_proj[0], iv = a.isig_proj[1];
  s00 += 1.0 / (iu * iu);
  s11 += 1.0 / (iv * iv);
  const double det = s00 * s11 - s01 * s01;
  const bool ok = st == 0 && isfinite(s00) && isfinite(s01) && isfinite(s11) && det > 0.0;
  const double nan = __builtin_nan("");
  const double d2 = ok ? (s11 * i0 * i0 - 2.0 * s01 * i0 * i1 + s00 * i1 * i1) / det : nan;
  const bool pass = on && ok && d2 <= a.chi2;
  const unsigned long long b = __ballot(pass);
  const uint32_t passbits = (uint32_t)(b >> (threadIdx.x & 32));
  const int npass = __popc(passbits), nin = __popc(min & low);
  const int need = a.min_pass < nin ? a.min_pass : nin;
  const int32_t gi = young ? PA_GATE_YOUNG : !fin ? PA_GATE_NOCOV : npass < need ? PA_GATE_FEW : PA_GATE_APPLIED;
  if (kl) {
    if (a.d2) a.d2[t * a.n_kp + k] = (young || !fin || !on) ? nan : d2;
    if (a.zhat) {
      a.zhat[(t * a.n_kp + k) * 2] = zh[0];
      a.zhat[(t * a.n_kp + k) * 2 + 1] = zh[1];
    }
  }
  if (lane == 0) {
    a.ginfo[t] = gi;
    // (in place: every lane of this half read the word before the ballot, in this wave)
    if (gi == PA_GATE_APPLIED) a.mask[t * a.mask_stride] = (min & ~low) | (min & passbits);
  }
}

}  // namespace pa

extern "C" {

int pa_window_predict(int T, int L, int Q, const double* pose, const double* angvel, const double* vel,
                      const double* cov, const double* cross, const int32_t* cov_info, const double* q_diag,
                      const double* tau, int vel_frame, double* pose_out, double* cov_out, void* stream) {
  PA_CHECK(T >= 0 && Q >= 1 && L >= 2, "window predict: T=%d L=%d Q=%d (T >= 0, L >= 2, Q >= 1)", T, L, Q);
  PA_CHECK(!cov == !cross, "window predict: cov and cross are given together (or both NULL)");
  PA_CHECK(!cov_out || cov, "window predict: cov_out needs cov and cross");
  PA_CHECK(!cov || L >= 3, "window predict: the covariance needs L >= 3 (frame L-2's angular velocity), L=%d", L);
  PA_CHECK(vel_frame == PA_VEL_WORLD || vel_frame == PA_VEL_BODY, "vel_frame must be 'world' or 'body'.");
  PA_CHECK((long)T * Q <= 0x7fffffffL / 64, "window predict: T * Q = %ld too large", (long)T * Q);
  if (T == 0) return PA_OK;
  PA_CHECK(pose && angvel && vel && tau && pose_out, "window predict: null pointer");
  const long n = (long)T * Q;
  hipLaunchKernelGGL(pa::window_predict_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                     pa::PredictArgs{T, L, Q, pose, angvel, vel, cov, cross, cov_info, q_diag, tau, vel_frame, pose_out,
                                     cov_out});
  PA_LAUNCH_CHECK();
  return PA_OK;
}

int pa_keypoint_gate(int T, int n_kp, int H, int W, const float* y_new, const double* pose_pred, long pose_stride,
                     const double* cov_pred, const double* corners, const double* K, const double* tcam,
                     const double* isig_proj, double chi2, int min_pass, const int32_t* nvalid, int min_frames,
                     uint32_t* mask, long mask_stride, double* d2, double* zhat, int32_t* ginfo, void* stream) {
  PA_CHECK(T >= 0, "keypoint gate: T=%d", T);
  PA_CHECK(n_kp >= 1 && n_kp <= 32, "keypoint gate: n_kp=%d (one mask bit per keypoint: 1..32)", n_kp);
  PA_CHECK(chi2 > 0.0 && chi2 <= 1.79769313486231570e308, "keypoint gate: chi2 must be a positive finite number");
  PA_CHECK(min_pass >= 0, "keypoint gate: min_pass=%d", min_pass);
  PA_CHECK(pose_stride >= 12, "keypoint gate: pose_stride=%ld (>= 12)", pose_stride);
  PA_CHECK(mask_stride >= 1, "keypoint gate: mask_stride=%ld (>= 1)", mask_stride);
  if (T == 0) return PA_OK;
  PA_CHECK(y_new && pose_pred && cov_pred && corners && K && isig_proj && mask && ginfo, "keypoint gate: null pointer");
  hipLaunchKernelGGL(pa::keypoint_gate_kernel, dim3((unsigned)((T + pa::GATE_TPB - 1) / pa::GATE_TPB)),
                     dim3(32 * pa::GATE_TPB), 0, (hipStream_t)stream,
                     pa::GateArgs{T, n_kp, H, W, y_new, pose_pred, pose_stride, cov_pred, corners, K, tcam, isig_proj, chi2,
                                  min_pass, nvalid, min_frames, mask, mask_stride, d2, zhat, ginfo});
  PA_LAUNCH_CHECK();
  return PA_OK;
}

}  // extern "C"
