// The streaming pose tick: one tick's pose stage (window advance, linearize, GN step, retract)
// fused into two launches, and its split form around the detector forward.  The GN step is
// gn_cr_run (gn_cr_dev.h), the factors and the window updates are factors_dev.h's.
#include "gn_cr_dev.h"

namespace pa {

// ---------------------------------------------------------------- the streaming pose tick, fused
// pa_window_pose_tick: one tick's pose stage (config 4) as two launches instead of four, one
// workgroup per trajectory (camera) in each:
//   pose_tick_lin_kernel (6 waves)  advance: window_advance_body (the window shifts, y_new
//        lands, frame L-1 predicted); linearize: the trajectory's factors as a T = 1 view --
//        waves 0-1 its L-1 dynamics factors (traj_dyn_block), then one wave per 256
//        projection factors and one for the constant-velocity ones (traj_unit_wave)
//   pose_tick_gn_kernel (12 waves)  the GN step (gn_cr_run, block cyclic reduction), then the
//        retract (window_retract_one per frame, the newest pose to `newest`)
// (One 12-wave launch for all four would hold the dynamics factors' ~220 VGPRs at three waves
// per SIMD: 240 spilled.)  Every phase is its separate kernel's device code, so the window,
// the factors, delta, info and the newest poses are bit for bit the four-launch sequence's
// (tests/test_streaming_pose_gpu.py).
// y_new null (the split tick's pre half): the window advances without the new keypoints, and
// frame L - 1's projection factors (evaluated on the stale keypoints the slot still holds)
// are marked status 3 afterwards, so the GN assembly gives them zero rows; the post half
// evaluates them on y_new.
// RB (here and in pose_tick_post_kernel): ta.robust_proj names a robust noise model for the
// projection factors (proj_eval<true>); the host picks the instantiation.
// TM (here and in pose_tick_post_kernel): ta carries real timestamps (dt_pair / kp_mask; the host
// picks the instantiation, factors_dev.h): the advance moves both rings and lands dt_new /
// mask_new, the factors read them after the barrier that follows it.
// CW: ta carries the constant-velocity factor on the angular velocity (r_cw; the host picks the
// instantiation, factors_dev.h).  It needs no keypoints, so the pre half (y_new null) has all of it.
template <bool RB, bool TM, bool CW>
__global__ __launch_bounds__(64 * TICK_LIN_W) void pose_tick_lin_kernel(pa_traj_args ta, const float* __restrict__ y_new) {
  __shared__ __attribute__((aligned(16))) double st[LIN_STAGE];
  const int t = blockIdx.x, L = ta.L, K = ta.n_kp;
  if constexpr (TM)
    window_advance_body<true>(t, threadIdx.x, 64 * TICK_LIN_W, L, K, y_new, const_cast<float*>(ta.y),
                              const_cast<double*>(ta.pose), const_cast<double*>(ta.angvel),
                              const_cast<double*>(ta.vel), ta.dt, ta.vel_frame, const_cast<int32_t*>(ta.nvalid),
                              AdvRings{const_cast<double*>(ta.dt_pair), const_cast<uint32_t*>(ta.kp_mask), ta.dt_new,
                                       ta.mask_new});
  else
    window_advance_body(t, threadIdx.x, 64 * TICK_LIN_W, L, K, y_new, const_cast<float*>(ta.y),
                        const_cast<double*>(ta.pose), const_cast<double*>(ta.angvel), const_cast<double*>(ta.vel), ta.dt,
                        ta.vel_frame, const_cast<int32_t*>(ta.nvalid));
  __syncthreads();
  const pa_traj_args a1 = traj_view(ta, t, factor_set(ta));
  traj_lin_block<RB, TM, CW>(a1, st);
  if (!y_new) {  // (uniform)
    __syncthreads();  // the unit waves' status stores come first
    if ((int)threadIdx.x < K) a1.status[(long)(L - 1) * K + threadIdx.x] = 3;
  }
}

template <int RP>
__global__ __launch_bounds__(64 * GN_CR_W, 1) void pose_tick_gn_kernel(GnArgs g, double* pose, double* angvel,
                                                                        double* vel, double* newest) {
  constexpr int NS = GN_CR_NS<RP>;
  using Ld = GnCrLds<RP, NS>;
  __shared__ __attribute__((aligned(16))) double fb[Ld::LM][Ld::BLK];
  __shared__ __attribute__((aligned(16))) double pool[Ld::POOL];
  const int t = blockIdx.x, L = g.L;
  gn_cr_run<RP, NS>(g, t, fb, pool);
  __syncthreads();
  if ((int)threadIdx.x < L)
    window_retract_one((long)t * L + threadIdx.x, L, g.delta, g.info, pose, angvel, vel, newest);
}

// The split tick.  pa_window_pose_tick_pre (before the keypoints exist: it runs beside the
// detector forward on a second stream of the tick's graph) = pose_tick_lin_kernel(null) +
// pose_tick_pre_kernel: every factor but the newest frame's projections, assembled and
// reduced by cyclic reduction in the ROOT order down to frame L - 1 alone.  A projection
// factor touches only its own frame's diagonal block, and the root's S and b enter the
// reduction only additively (no elimination reads them), so the newest frame's projection
// rows can be added to the reduced root at the end:
//   pose_tick_post_kernel  y_new lands in the window, its K projection factors (the factor
//        outputs, as the linearize writes them), S_root += Jp^T Jp and b_root -= Jp^T rp on the
//        pose block, delta_root = S_root^-1 b_root, back substitution, delta / info, retract.
// The same normal equations as pa_window_pose_tick, another elimination order and f64
// rounding (tests/test_streaming_pose_gpu.py: within 1e-9 of its delta).
template <int RP>
__global__ __launch_bounds__(64 * GN_CR_W, 1) void pose_tick_pre_kernel(GnArgs g) {
  constexpr int NS = GN_CR_NS<RP>;
  using Ld = GnCrLds<RP, NS, true>;
  __shared__ __attribute__((aligned(16))) double fb[Ld::LM][Ld::BLK];
  __shared__ __attribute__((aligned(16))) double pool[Ld::POOL];
  gn_cr_run<RP, NS, true>(g, blockIdx.x, fb, pool);
}

template <bool RB, bool TM>
__global__ __launch_bounds__(64 * GN_CR_W, 1) void pose_tick_post_kernel(pa_traj_args ta, const float* __restrict__ y_new,
                                                                          const double* __restrict__ ws, double* delta,
                                                                          int32_t* info, double* newest) {
  using namespace gn;
  constexpr int KP = 2 * GN_KMAX, FD = GN_TICK_FRD, LM = GN_CR_LMAX;
  __shared__ __attribute__((aligned(16))) double dl[LM][NV];   // delta per frame
  __shared__ __attribute__((aligned(16))) double sr[NB + NV];  // the root's S | b
  __shared__ __attribute__((aligned(16))) double jt[7][KP];    // newest frame: Jp^T (6 x 2K) | rp
  __shared__ __attribute__((aligned(16))) GnChainLds C;
  __shared__ int fail_s;
  const int t = blockIdx.x, L = ta.L, K = ta.n_kp, ny = 2 * K;
  const int wv = threadIdx.x >> 6, i = threadIdx.x & 63;
  const long f0 = (long)t * L, fn = f0 + L - 1;
  const double* w = ws + (size_t)t * GN_TICK_WSD;
  // thread (l, r) < L x 12: row r of B_l and a_l[r], loaded first (in flight with the rest)
  const int tl = (int)threadIdx.x / NV, tr = (int)threadIdx.x - tl * NV;
  const bool brow = tl < L;
  double bv[NV], av = 0.0;
  if (brow) {
    const double* src = w + tl * FD;
#pragma unroll
    for (int k = 0; k < NV; k += 2) {
      const gn_d2 v = *reinterpret_cast<const gn_d2*>(src + tr * NV + k);
      bv[k] = v[0];
      bv[k + 1] = v[1];
    }
    av = src[NB + tr];
  }
  for (int e = threadIdx.x; e < NB + NV; e += 64 * GN_CR_W) sr[e] = w[LM * FD + e];
  if (threadIdx.x == 0) fail_s = reinterpret_cast<const int*>(w + LM * FD + NB + NV)[0];
  double s = 0.0;  // wave 0, lane o < 42: entry o of [Jp^T Jp | Jp^T rp] (6 x 7, row-major)
  if (wv == 0) {
    // y_new lands (pa_window_advance's last step) and frame L - 1's projection factors:
    // lane k, traj_unit_wave's evaluation
    if (i < ny) const_cast<float*>(ta.y)[fn * ny + i] = y_new[(size_t)t * ny + i];
    if (i < K) {
      Cam camv = load_cam<RB>(ta.K, ta.tcam, ta.isig_proj, ta.robust_proj, ta.robust_proj_k);
      if constexpr (TM) cam_to_vector(camv);
      const Cam cam = camv;
      const Pose T = load_pose(ta.pose + fn * 12);
      const V3 pb = load3(ta.corners + 3 * i);
      const float px = kornia_denorm(y_new[(size_t)t * ny + 2 * i], ta.W);
      const float py = kornia_denorm(y_new[(size_t)t * ny + 2 * i + 1], ta.H);
      bool off = ta.nvalid ? L - 1 < L - ta.nvalid[t] : false;
      if constexpr (TM) off = off || kp_masked(ta.kp_mask, fn, i);  // (the frame the pre half advanced)
      double r[2], J[12], e;
      int32_t st;
      proj_eval<RB>(T, pb, (double)px, (double)py, cam, r, J, e, st);
      if (off) {
        r[0] = r[1] = 0.0;
#pragma unroll
        for (int c = 0; c < 12; ++c) J[c] = 0.0;
        e = 0.0;
        st = 2;
      }
      const long u = fn * K + i;
      ta.r_proj[u * 2] = r[0];
      ta.r_proj[u * 2 + 1] = r[1];
#pragma unroll
      for (int c = 0; c < 12; ++c) ta.j_proj[u * 12 + c] = J[c];
      if (ta.err_proj) ta.err_proj[u] = e;
      ta.status[u] = st;
      // the GN assembly's rows: a failed projection (status != 0) gives zero rows
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        jt[c][2 * i] = st == 0 ? J[c * 2] : 0.0;
        jt[c][2 * i + 1] = st == 0 ? J[c * 2 + 1] : 0.0;
      }
      jt[6][2 * i] = st == 0 ? r[0] : 0.0;
      jt[6][2 * i + 1] = st == 0 ? r[1] : 0.0;
    }
    wave_order();
    if (i < 42) {
      const int ra = i < 36 ? i / 6 : i - 36, cb = i < 36 ? i - 6 * (i / 6) : 6;
      for (int q = 0; q < ny; ++q) s += jt[ra][q] * jt[cb][q];
    }
  }
  __syncthreads();  // the root's S | b, the failure word
  if (wv == 0) {
    // the newest frame's projections into the root (S += Jp^T Jp on the pose block, b -= Jp^T rp)
    if (i < 36) sr[(i / 6) * NV + i - 6 * (i / 6)] += s;
    else if (i < 42) sr[NB + i - 36] -= s;
    wave_order();
    if (fail_s == 0) {  // delta_root = S^-1 b
      const bool act = i < 36;
      const int ii = act ? i : 35;
      const int r = ii / 3, c0 = 4 * (ii - 3 * (ii / 3));
      double sv[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) sv[c] = sr[r * NV + c0 + c];
      const double b = sr[NB + r];
      if (!gn_sweep(sv, C.rk2, r, c0, act)) {
        if (i == 0) fail_s = L;
      } else {
        const double z = gn_finish(sv, b, C, r, c0, act);
        wave_order();
        if (act && c0 == 0) dl[L - 1][r] = z;
      }
    }
  }
  __syncthreads();
  const int inf = fail_s;
  // every frame at once: delta_l = a_l + B_l delta_root
  double dv = NAN;
  if (brow && !inf) {
    double d0 = av, d1 = 0.0;
#pragma unroll
    for (int k = 0; k < NV; k += 2) {
      d0 += bv[k] * dl[L - 1][k];
      d1 += bv[k + 1] * dl[L - 1][k + 1];
    }
    dv = d0 + d1;
  }
  __syncthreads();  // every read of delta_root is done
  if (brow) {
    dl[tl][tr] = dv;
    delta[(size_t)f0 * NV + threadIdx.x] = dv;
  }
  if (threadIdx.x == 0) info[t] = inf;
  __syncthreads();
  if ((int)threadIdx.x < L)
    window_retract_frame(f0 + threadIdx.x, L, dl[threadIdx.x], inf == 0, const_cast<double*>(ta.pose),
                         const_cast<double*>(ta.angvel), const_cast<double*>(ta.vel), newest);
}

template <bool CW>
static auto pose_tick_lin_pick(bool rb, bool tm) {
  return tm ? (rb ? pose_tick_lin_kernel<true, true, CW> : pose_tick_lin_kernel<false, true, CW>)
            : (rb ? pose_tick_lin_kernel<true, false, CW> : pose_tick_lin_kernel<false, false, CW>);
}

}  // namespace pa

extern "C" {

size_t pa_window_pose_tick_workspace(int T, int L) {
  return (T > 0 && L > 0) ? (size_t)T * pa::GN_TICK_WSD * sizeof(double) : 0;
}

// the checks of pa_window_pose_tick, in its order; PA_OK at T == 0 (nothing to do: the caller
// returns) before the pointers are looked at
// advancing: the entry point moves the window, so the real timestamps' rings need their new
// elements (dt_pair with dt_new, kp_mask with mask_new: together or not at all)
static int pose_tick_check(const pa_traj_args* ta, double lambda, const char* who, bool advancing = false) {
  PA_CHECK(ta, "%s: null args", who);
  if (const int rc = pa::robust_check(*ta, who)) return rc;
  if (advancing) {
    PA_CHECK(!ta->dt_pair == !ta->dt_new, "%s: dt_pair and dt_new are given together (or both NULL)", who);
    PA_CHECK(!ta->kp_mask == !ta->mask_new, "%s: kp_mask and mask_new are given together (or both NULL)", who);
  }
  const int T = ta->T, L = ta->L, K = ta->n_kp;
  // one workgroup per trajectory: correct at any T (the CU count is a performance choice of the
  // caller, StreamingPipeline's fused_pose / split_pose eligibility)
  PA_CHECK(T >= 0 && L >= 2 && L <= pa::GN_CR_LMAX && K >= 0 && K <= pa::GN_KMAX,
           "%s: T %d, L %d (2..%d), n_kp %d (<= %d)", who, T, L, pa::GN_CR_LMAX, K, pa::GN_KMAX);
  if (T == 0) return PA_OK;
  if (advancing) {
    PA_CHECK(!ta->dt_pair == !ta->dt_new, "%s: dt_pair and dt_new are given together (or both NULL)", who);
    PA_CHECK(!ta->kp_mask == !ta->mask_new, "%s: kp_mask and mask_new are given together (or both NULL)", who);
  }
  PA_CHECK(lambda >= 0.0, "%s: lambda %g < 0", who, lambda);
  PA_CHECK(ta->y && ta->pose && ta->vel && ta->angvel && ta->corners && ta->K && ta->nvalid,
           "%s: null window / model pointer", who);
  PA_CHECK((K == 0 || (ta->r_proj && ta->j_proj && ta->status)) && ta->r_dyn && ta->j_dyn0 && ta->j_dyn1 &&
               ta->j_dyn2 && ta->j_dyn3 && ta->r_cv && ta->j_cv0 && ta->j_cv1,
           "%s: the factor outputs and every Jacobian are required", who);
  return PA_OK;
}

// the factor on the angular velocity (r_cw switches it on): the step needs its whitening.  Every
// entry point runs this after all of its older checks
static int pose_tick_cw_check(const pa_traj_args* ta, const char* who) {
  PA_CHECK(!ta->r_cw || ta->isig_cw, "%s: r_cw is given without isig_cw (the step needs the factor whitened)", who);
  PA_CHECK(ta->r_cw || !ta->err_cw, "%s: err_cw is given without r_cw (r_cw switches the factor on)", who);
  return PA_OK;
}

static int pose_tick_ws_check(const pa_traj_args* ta, const void* ws, size_t ws_bytes, const char* who) {
  const size_t need = pa_window_pose_tick_workspace(ta->T, ta->L);
  PA_CHECK(ws && ws_bytes >= need, "%s: workspace %zu < %zu", who, ws_bytes, need);
  return PA_OK;
}

// advance + linearize (y_new null: the split tick's pre half), with or without a robust noise model
static void launch_lin(const pa_traj_args* ta, const float* y_new, hipStream_t s) {
  const bool rb = ta->robust_proj != PA_ROBUST_NONE, tm = ta->dt_pair || ta->kp_mask;
  const auto kernel = ta->r_cw ? pa::pose_tick_lin_pick<true>(rb, tm) : pa::pose_tick_lin_pick<false>(rb, tm);
  hipLaunchKernelGGL(kernel, dim3(ta->T), dim3(64 * pa::TICK_LIN_W), 0, s, *ta, y_new);
}

// the cyclic reduction in the ROOT order into the tick workspace (the pre half's second launch)
static void launch_pre(const pa_traj_args* ta, double lambda, void* ws, const double* pi, const double* pg,
                       hipStream_t s) {
  pa::GnArgs g = pa::gn_args(*ta, lambda, nullptr, nullptr, (double*)ws);
  g.p_info = pi;
  g.p_grad = pg;
  pa::gn_for_kp(ta->n_kp, [&](auto rp) {
    hipLaunchKernelGGL(pa::pose_tick_pre_kernel<decltype(rp)::value>, dim3(ta->T), dim3(64 * pa::GN_CR_W), 0, s, g);
  });
}

// the marginalization prior on frame 0 (prior.hip), given together or not at all
static int prior_pair_check(const double* pi, const double* pg, const char* who) {
  PA_CHECK(!pi == !pg, "%s: prior_info and prior_grad are given together (or both NULL)", who);
  return PA_OK;
}

int pa_window_pose_tick_prior(const pa_traj_args* ta, const float* y_new, double lambda, double* delta, int32_t* info,
                              double* newest_pose, const double* prior_info, const double* prior_grad, void* stream) {
  PA_CHECK(ta && y_new && delta && info, "pose tick: null args / y_new / delta / info");
  int rc = pose_tick_check(ta, lambda, "pose tick", true);
  if (rc != PA_OK || ta->T == 0) return rc;
  if ((rc = prior_pair_check(prior_info, prior_grad, "pose tick")) != PA_OK) return rc;
  if ((rc = pose_tick_cw_check(ta, "pose tick")) != PA_OK) return rc;
  const int T = ta->T;
  pa::GnArgs g = pa::gn_args(*ta, lambda, delta, info, nullptr);
  g.p_info = prior_info;
  g.p_grad = prior_grad;
  const hipStream_t s = (hipStream_t)stream;
  if (!(pa::g_gn_na & 2048)) launch_lin(ta, y_new, s);
  if (pa::g_gn_na & 1024) { PA_LAUNCH_CHECK(); return PA_OK; }
  double* pose = const_cast<double*>(ta->pose);
  double* angvel = const_cast<double*>(ta->angvel);
  double* vel = const_cast<double*>(ta->vel);
  pa::gn_for_kp(ta->n_kp, [&](auto rp) {
    hipLaunchKernelGGL(pa::pose_tick_gn_kernel<decltype(rp)::value>, dim3(T), dim3(64 * pa::GN_CR_W), 0, s, g, pose, angvel,
                       vel, newest_pose);
  });
  PA_LAUNCH_CHECK();
  return PA_OK;
}

int pa_window_pose_tick(const pa_traj_args* ta, const float* y_new, double lambda, double* delta, int32_t* info,
                        double* newest_pose, void* stream) {
  return pa_window_pose_tick_prior(ta, y_new, lambda, delta, info, newest_pose, nullptr, nullptr, stream);
}

int pa_window_pose_tick_pre_prior(const pa_traj_args* ta, double lambda, void* ws, size_t ws_bytes,
                                  const double* prior_info, const double* prior_grad, void* stream) {
  int rc = pose_tick_check(ta, lambda, "pose tick pre", true);
  if (rc != PA_OK || ta->T == 0) return rc;
  if ((rc = prior_pair_check(prior_info, prior_grad, "pose tick pre")) != PA_OK) return rc;
  if ((rc = pose_tick_ws_check(ta, ws, ws_bytes, "pose tick pre")) != PA_OK) return rc;
  if ((rc = pose_tick_cw_check(ta, "pose tick pre")) != PA_OK) return rc;
  const hipStream_t s = (hipStream_t)stream;
  launch_lin(ta, nullptr, s);
  launch_pre(ta, lambda, ws, prior_info, prior_grad, s);
  PA_LAUNCH_CHECK();
  return PA_OK;
}

int pa_window_pose_tick_pre(const pa_traj_args* ta, double lambda, void* ws, size_t ws_bytes, void* stream) {
  return pa_window_pose_tick_pre_prior(ta, lambda, ws, ws_bytes, nullptr, nullptr, stream);
}

int pa_window_pose_tick_reduce_prior(const pa_traj_args* ta, double lambda, void* ws, size_t ws_bytes,
                                     const double* prior_info, const double* prior_grad, void* stream) {
  int rc = pose_tick_check(ta, lambda, "pose tick reduce");
  if (rc != PA_OK || ta->T == 0) return rc;
  if ((rc = prior_pair_check(prior_info, prior_grad, "pose tick reduce")) != PA_OK) return rc;
  if ((rc = pose_tick_ws_check(ta, ws, ws_bytes, "pose tick reduce")) != PA_OK) return rc;
  if ((rc = pose_tick_cw_check(ta, "pose tick reduce")) != PA_OK) return rc;
  launch_pre(ta, lambda, ws, prior_info, prior_grad, (hipStream_t)stream);
  PA_LAUNCH_CHECK();
  return PA_OK;
}

int pa_window_pose_tick_reduce(const pa_traj_args* ta, double lambda, void* ws, size_t ws_bytes, void* stream) {
  return pa_window_pose_tick_reduce_prior(ta, lambda, ws, ws_bytes, nullptr, nullptr, stream);
}

int pa_window_pose_tick_post(const pa_traj_args* ta, const float* y_new, const void* ws, size_t ws_bytes,
                             double* delta, int32_t* info, double* newest_pose, void* stream) {
  int rc = pose_tick_check(ta, 0.0, "pose tick post");
  if (rc != PA_OK || ta->T == 0) return rc;
  PA_CHECK(y_new && delta && info, "pose tick post: null y_new / delta / info");
  if ((rc = pose_tick_ws_check(ta, ws, ws_bytes, "pose tick post")) != PA_OK) return rc;
  if ((rc = pose_tick_cw_check(ta, "pose tick post")) != PA_OK) return rc;
  const bool rb = ta->robust_proj != PA_ROBUST_NONE, tm = ta->kp_mask != nullptr;
  const auto kernel = tm ? (rb ? pa::pose_tick_post_kernel<true, true> : pa::pose_tick_post_kernel<false, true>)
                         : (rb ? pa::pose_tick_post_kernel<true, false> : pa::pose_tick_post_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(ta->T), dim3(64 * pa::GN_CR_W), 0, (hipStream_t)stream, *ta, y_new, (const double*)ws,
                     delta, info, newest_pose);
  PA_LAUNCH_CHECK();
  return PA_OK;
}

}  // extern "C"
