// Fixed-lag marginalization: the frame a window drops is carried forward as a linear prior on
// the frame that is now oldest -- what GTSAM's BatchFixedLagSmoother / IncrementalFixedLagSmoother
// do with the states that leave the lag (the Schur complement of their factors, kept as a
// LinearContainerFactor with its linearization point), instead of pa_window_advance forgetting
// frame 0 together with everything its factors knew.
//
// The prior, per trajectory, f64, in INFORMATION form (the marginal is only positive
// semi-definite: frame 1's angular velocity gets no information from frame 0, so a Cholesky
// factor does not exist):  Lambda (12 x 12, row-major, symmetric) over the frame block
// [pose tangent 6 | angvel 3 | vel 3] of gn.hip, eta (12), and the state xbar it was linearized
// at.  With xi = [Logmap(xbar_pose^-1 pose); angvel - wbar; vel - vbar] its cost is
//   0.5 xi^T Lambda xi - eta^T xi,
// and, Lambda kept fixed and the chart's Jacobian taken as the identity (LinearContainerFactor),
// it adds  D_0 += Lambda,  g_0 += Lambda xi - eta  to the normal equations: gn_build_frame does
// that for frame 0 when GnArgs.p_info / p_grad are set, so the Gauss-Newton step, the cyclic
// reduction, the ticks and the marginals all honour it at that one place.
//
// pa_window_prior_linearize: xi, grad = Lambda xi - eta, err.  One wave per trajectory.
// pa_window_marginalize: one wave (one workgroup) per trajectory.  Frame 0 is assembled by
// gn_load_frame / gn_build_frame with the input prior (so cheirality and nvalid statuses count
// as in every consumer): D_0 + Lambda_in, E_0, g_0 + grad_in.  Then
//   H = D_0 + Lambda_in + lambda I,  M = H^-1 (gn_sweep),  z = M (g_0 + grad_in) (gn_finish),
//   [F | h] = B^T [B | r]  from the staged x_1 part B of the pair (0, 1)'s factors (one MFMA
//             chain: the staging's BT rows against themselves, r in column 12),
//   Lambda' = F - E_0^T M E_0,  g' = h - E_0^T z  (gn_couple_mfma: both products on the f64
//             matrix cores, and the right-hand side in its column 12),
// Lambda' symmetrized as (X + X^T) / 2 through LDS exactly as the marginals kernel does, and
// re-centred to first order at the retracted state: g' += Lambda' delta_1.
#include "prior_dev.h"

namespace pa {

struct MargArgs {
  const double* delta;
  const int32_t *gn_info, *nvalid;
  const double *pose, *angvel, *vel;
  double *info_out, *eta_out, *xp, *xw, *xv;
  int32_t* minfo;
};

__global__ __launch_bounds__(64) void prior_lin_kernel(int L, int frame, const double* __restrict__ info,
                                                       const double* __restrict__ eta, const double* __restrict__ xp,
                                                       const double* __restrict__ xw, const double* __restrict__ xv,
                                                       const double* __restrict__ pose, const double* __restrict__ angvel,
                                                       const double* __restrict__ vel, double* __restrict__ grad,
                                                       double* __restrict__ err) {
  using namespace gn;
  __shared__ double xi[NV], es[NV];
  const int t = blockIdx.x, i = threadIdx.x;
  const long f = (long)t * L + frame;
  const double s = prior_lin_wave(i, info + (size_t)t * NB, eta + (size_t)t * NV, xp + (size_t)t * 12,
                                  xw + (size_t)t * 3, xv + (size_t)t * 3, pose + f * 12, angvel + f * 3, vel + f * 3,
                                  grad + (size_t)t * NV, xi, es);
  if (err && i == 0) err[t] = s;
}

template <int RP>
__global__ __launch_bounds__(64) void marginalize_kernel(GnArgs a, MargArgs m) {
  using namespace gn;
  typedef double d4_t __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) GnStage<RP> st;
  __shared__ __attribute__((aligned(16))) double blk[2 * NB + NV];  // D_0 + Lambda_in | E_0 | g_0 + grad_in
  __shared__ __attribute__((aligned(16))) GnChainLds C;
  __shared__ __attribute__((aligned(16))) double Fx[NV * 13];  // [F | h]
  __shared__ __attribute__((aligned(16))) double Ps[NB];       // the block to symmetrize, then Lambda'
  __shared__ double dl[NV];                                    // delta of frame 1
  const int t = blockIdx.x, i = threadIdx.x;
  const int L = a.L;
  const long f0 = (long)t * L;
  // xbar: window frame 1's state as it stands
  if (i < 12)
    m.xp[(size_t)t * 12 + i] = m.pose[(f0 + 1) * 12 + i];
  else if (i < 15)
    m.xw[(size_t)t * 3 + i - 12] = m.angvel[(f0 + 1) * 3 + i - 12];
  else if (i < 18)
    m.xv[(size_t)t * 3 + i - 15] = m.vel[(f0 + 1) * 3 + i - 15];
  const bool act = i < 36;
  const int ii = act ? i : 35;  // lanes >= 36 shadow lane 35 (no stores)
  const int r = ii / 3, c0 = 4 * (ii - 3 * (ii / 3));
  const int e0 = r * NV + c0;
  int mi = (m.nvalid && m.nvalid[t] < L) ? 2 : 0;  // (uniform)
  double s[4] = {0.0, 0.0, 0.0, 0.0}, b = 0.0;
  if (!mi) {
    gn_zero_stage<RP>(st);
    GnFrameLoads<RP> ld;
    gn_load_frame<RP>(a, f0, ld);
    gn_build_frame<RP, false>(a, f0, ld, st, blk);
    wave_order();
    double sv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) sv[c] = blk[e0 + c] + (r == c0 + c ? a.lambda : 0.0);
    if (!gn_sweep(sv, C.rk2, r, c0, act)) {
      mi = 1;
    } else {
      gn_finish(sv, blk[2 * NB + r], C, r, c0, act);  // C.M = H^-1, C.z = H^-1 (g_0 + grad_in)
      // [F | h] = B^T [B | r]: the staging's BT (12 x 9 transposed, zero-padded to 16 x 12) as
      // both operands, the pair's residuals (rows 2K .. 2K + 8 of the staged r) in column 12
      const int li = i & 15, lk = i >> 4, rn = 2 * a.K;
      d4_t cF = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int k = 4 * q + lk;
        const double av = st.BT[li][k];
        const double rv = k < 9 ? st.AT[NV][rn + k] : 0.0;
        cF = __builtin_amdgcn_mfma_f64_16x16x4f64(av, li == NV ? rv : av, cF, 0, 0, 0);
      }
#pragma unroll
      for (int v = 0; v < 3; ++v)  // rows lk + 4v < 12
        if (li <= NV) Fx[(lk + 4 * v) * 13 + li] = cF[v];
      wave_order();
      // the pair (0, 1)'s factor on the angular velocity (gn_build_frame's closed form): its x_1
      // part is +s_i on variable 6 + i, so F[6+i][6+i] += s_i^2 and h[6+i] += s_i r_{0,i}
      if (a.r_cw != nullptr) {  // (uniform)
        if (i < 3) {
          const double s = a.isig_cw[i];
          Fx[(6 + i) * 13 + 6 + i] += s * s;
          Fx[(6 + i) * 13 + NV] += s * a.r_cw[(size_t)t * (L - 1) * 3 + i];
        }
        wave_order();
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) sv[c] = Fx[r * 13 + c0 + c];
      b = Fx[r * 13 + NV];
      // sv -= E_0^T (M E_0),  b -= E_0^T z
      gn_couple_mfma<false>(C.M, C.z, blk + NB, nullptr, nullptr, C.G, r, c0, sv, b);
      // X -> (X + X^T) / 2, as gn_marginals_kernel symmetrizes its blocks
      wave_order();
      if (act) {
#pragma unroll
        for (int c = 0; c < 4; ++c) Ps[e0 + c] = sv[c];
      }
      wave_order();
#pragma unroll
      for (int c = 0; c < 4; ++c) s[c] = 0.5 * (sv[c] + Ps[(c0 + c) * NV + r]);
      // re-centre at the retracted state (a failed step retracted nothing)
      if (m.delta && (!m.gn_info || m.gn_info[t] == 0)) {  // (uniform)
        wave_order();  // every lane is past its reads of Ps
        if (act) {
#pragma unroll
          for (int c = 0; c < 4; ++c) Ps[e0 + c] = s[c];
        }
        if (i < NV) dl[i] = m.delta[(f0 + 1) * NV + i];
        wave_order();
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < NV; ++k) acc = fma(Ps[r * NV + k], dl[k], acc);
        b += acc;
      }
    }
  }
  const bool ok = mi == 0;
  if (act) {
#pragma unroll
    for (int c = 0; c < 4; ++c) m.info_out[(size_t)t * NB + e0 + c] = ok ? s[c] : 0.0;
    if (c0 == 0) m.eta_out[(size_t)t * NV + r] = ok ? -b : 0.0;
  }
  if (i == 0) m.minfo[t] = mi;
}

}  // namespace pa

extern "C" {

int pa_window_prior_linearize(int T, int L, int frame, const double* info, const double* eta, const double* xbar_pose,
                              const double* xbar_angvel, const double* xbar_vel, const double* pose,
                              const double* angvel, const double* vel, double* grad_out, double* err_out,
                              void* stream) {
  PA_CHECK(T >= 0 && L >= 2, "prior linearize: T %d L %d (>= 2)", T, L);
  PA_CHECK(frame >= 0 && frame < L, "prior linearize: frame %d outside the window (0..%d)", frame, L - 1);
  if (T == 0) return PA_OK;
  PA_CHECK(info && eta && xbar_pose && xbar_angvel && xbar_vel, "prior linearize: null prior pointer");
  PA_CHECK(pose && angvel && vel, "prior linearize: null window pointer");
  PA_CHECK(grad_out, "prior linearize: null grad_out");
  hipLaunchKernelGGL(pa::prior_lin_kernel, dim3(T), dim3(64), 0, (hipStream_t)stream, L, frame, info, eta, xbar_pose,
                     xbar_angvel, xbar_vel, pose, angvel, vel, grad_out, err_out);
  PA_LAUNCH_CHECK();
  return PA_OK;
}

// pa_window_marginalize with the constant-velocity factor on the angular velocity (r_cw null: the parent)
int pa_window_marginalize_cw(int T, int L, int n_kp, const double* r_proj, const double* j_proj,
                             const int32_t* status_proj, const double* r_dyn, const double* j_dyn0,
                             const double* j_dyn1, const double* j_dyn2, const double* j_dyn3, const double* r_cv,
                             const double* j_cv0, const double* j_cv1, const double* prior_info_in,
                             const double* prior_grad_in, const double* r_cw, const double* isig_cw, double lambda,
                             const double* delta, const int32_t* gn_info, const int32_t* nvalid, const double* pose,
                             const double* angvel, const double* vel, double* info_out, double* eta_out,
                             double* xbar_pose_out, double* xbar_angvel_out, double* xbar_vel_out, int32_t* minfo,
                             void* stream) {
  PA_CHECK(T >= 0 && L >= 2 && n_kp >= 0 && n_kp <= pa::GN_KMAX, "marginalize: T %d L %d (>= 2) n_kp %d (<= %d)", T, L,
           n_kp, pa::GN_KMAX);
  PA_CHECK(lambda >= 0.0, "marginalize: lambda %g < 0", lambda);
  if (T == 0) return PA_OK;
  PA_CHECK(n_kp == 0 || (r_proj && j_proj), "marginalize: null projection factors");
  PA_CHECK(r_dyn && j_dyn0 && j_dyn1 && j_dyn2 && j_dyn3 && r_cv && j_cv0 && j_cv1,
           "marginalize: null dynamics / constant-velocity factors (Jacobians are required)");
  PA_CHECK(!prior_info_in == !prior_grad_in,
           "marginalize: prior_info_in and prior_grad_in are given together (or both NULL)");
  PA_CHECK(pose && angvel && vel, "marginalize: null window pointer");
  PA_CHECK(info_out && eta_out && xbar_pose_out && xbar_angvel_out && xbar_vel_out && minfo,
           "marginalize: null output pointer");
  const pa::GnArgs a{T,     L,     n_kp,  r_proj, j_proj,  status_proj, r_dyn,   j_dyn0,  j_dyn1,  j_dyn2,  j_dyn3,
                     r_cv,  j_cv0, j_cv1, lambda, nullptr, nullptr,     nullptr, nullptr, nullptr, nullptr, nullptr,
                     prior_info_in, prior_grad_in, r_cw, isig_cw};
  PA_CHECK(!r_cw || isig_cw,
           "marginalize: r_cw is given without isig_cw (the factor's Jacobians are -+ diag(isig_cw))");
  const pa::MargArgs m{delta, gn_info, nvalid, pose, angvel, vel, info_out, eta_out, xbar_pose_out, xbar_angvel_out,
                       xbar_vel_out, minfo};
  pa::gn_for_kp(n_kp, [&](auto rp) {
    hipLaunchKernelGGL(pa::marginalize_kernel<decltype(rp)::value>, dim3(T), dim3(64), 0, (hipStream_t)stream, a, m);
  });
  PA_LAUNCH_CHECK();
  return PA_OK;
}

int pa_window_marginalize(int T, int L, int n_kp, const double* r_proj, const double* j_proj,
                          const int32_t* status_proj, const double* r_dyn, const double* j_dyn0, const double* j_dyn1,
                          const double* j_dyn2, const double* j_dyn3, const double* r_cv, const double* j_cv0,
                          const double* j_cv1, const double* prior_info_in, const double* prior_grad_in, double lambda,
                          const double* delta, const int32_t* gn_info, const int32_t* nvalid, const double* pose,
                          const double* angvel, const double* vel, double* info_out, double* eta_out,
                          double* xbar_pose_out, double* xbar_angvel_out, double* xbar_vel_out, int32_t* minfo,
                          void* stream) {
  return pa_window_marginalize_cw(T, L, n_kp, r_proj, j_proj, status_proj, r_dyn, j_dyn0, j_dyn1, j_dyn2, j_dyn3, r_cv,
                                  j_cv0, j_cv1, prior_info_in, prior_grad_in, nullptr, nullptr, lambda, delta, gn_info,
                                  nvalid, pose, angvel, vel, info_out, eta_out, xbar_pose_out, xbar_angvel_out,
                                  xbar_vel_out, minfo, stream);
}

}  // extern "C"
