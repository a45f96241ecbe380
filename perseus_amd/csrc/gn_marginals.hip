// pa_trajectory_marginals: the marginal covariances of the trajectory smoother, what a GTSAM
// user reads from Marginals(graph, values).marginalCovariance(key), on the device.  With J the
// stacked whitened Jacobian of pa_trajectory_gn_step (gn.hip's opening comment has the graph
// and the 12-variable frame block),
//   Sigma = (J^T J + lambda I)^-1,
// and the outputs are its diagonal blocks Sigma_{l,l} (cov), optionally the super-diagonal
// blocks Sigma_{l,l+1} (cross, frame l on rows) and the newest frame's block alone (cov_newest).
// The blocks live in the tangent space of pa_window_retract's chart (a right perturbation,
// GTSAM's Pose3 convention).
//
// Chosen form: the ONE-SIDED recursion on the top-down chain of gn_step_kernel<.., SOLVER 1>,
//   forward   S_0 = D_0 + lambda I,  M_l = S_l^-1 (gn_sweep),  G_l = M_l E_l (gn_couple_mfma),
//             S_{l+1} = D_{l+1} + lambda I - E_l^T G_l;           M_l, G_l -> workspace
//   backward  Sigma_{L-1} = M_{L-1},
//             P_l = G_l Sigma_{l+1},  Sigma_{l,l+1} = -P_l,  Sigma_l = M_l + P_l G_l^T
// rather than the two-sided Sigma_l = (A_l + B_l - D_l - lambda I)^-1 of forward and backward
// Schur complements: the backward pass here is two 12 x 12 x 12 products per frame with no
// pivot sequence (the two-sided form inverts a third block per frame, 6 more dependent pivot
// steps each), Sigma_l is a sum of positive semi-definite terms (the two-sided form subtracts
// D_l from A_l + B_l, which cancels where a variable is held by its neighbours alone), the
// cross blocks fall out of the first product, and the cov_newest-only call is the forward
// chain with nothing stored.  The price is a serial depth of 2 L block operations.
//
// One workgroup of two waves per trajectory: wave 0 assembles frame j (gn_build_frame; frame
// j + 1's loads are in flight meanwhile) into a ring of three LDS slots while wave 1 eliminates
// frame j - 1; one LDS-only workgroup barrier per frame hands a slot over (slot j % 3 is
// neither frame j - 1's nor frame j - 2's, whose E block the elimination of j - 1 reads).
// There is no other wait: both waves pass L + 1 barriers whatever happens, and after a failed
// pivot the solver wave idles through the remaining ones.  Wave 1 then runs the backward pass
// alone, from the workspace, one frame's M / G loaded ahead.  36 lanes hold a 12 x 12 block
// (lane: row r, columns c0 .. c0 + 3), as in the step's solvers.  Every output block is
// symmetrized as (X + X^T) / 2 through LDS (Sigma_{L-1} = M_{L-1} too, in both the full and
// the cov_newest-only call), so cov[l] == cov[l]^T bit for bit, and the symmetrized block
// is what the recursion carries on.  Whether cross / cov_newest are written changes no
// arithmetic.
//
// lambda = 0 gets no special case: on a full window the last frame's angular velocity is in no
// factor, so its pivot block fails (info = L, as pa_trajectory_gn_step); a small lambda
// (1e-9) gives the undamped Gauss-Newton covariance, that variable's block decoupled at
// 1 / lambda.  f64 throughout.
#include "gn_dev.h"

namespace pa {

constexpr int MG_WSF = 2 * gn::NB;  // workspace doubles per frame: M_l | G_l

template <int RP>
__global__ __launch_bounds__(128) void gn_marginals_kernel(GnArgs a, double* cov, double* cross, double* cov_newest) {
  using namespace gn;
  constexpr int BLK = 2 * NB + NV;  // D | E | g of one frame
  constexpr int R = 3;
  __shared__ __attribute__((aligned(16))) GnStage<RP> st;
  __shared__ __attribute__((aligned(16))) double blk[R][BLK];
  __shared__ __attribute__((aligned(16))) GnChainLds C;
  __shared__ __attribute__((aligned(16))) double Sg[NB];  // Sigma_{l+1}
  __shared__ __attribute__((aligned(16))) double Gs[NB];  // G_l
  __shared__ __attribute__((aligned(16))) double Ps[NB];  // P_l, then the block to symmetrize
  const int t = blockIdx.x;
  const int wv = threadIdx.x >> 6;
  const int i = threadIdx.x & 63;
  const int L = a.L;
  const long f0 = (long)t * L;
  const bool full = cov != nullptr;  // uniform
  double* ws = a.ws + (size_t)t * L * MG_WSF;
  const bool act = i < 36;
  const int ii = act ? i : 35;  // lanes >= 36 shadow lane 35 (no stores)
  const int r = ii / 3, c0 = 4 * (ii - 3 * (ii / 3));
  const int e0 = r * NV + c0;  // this lane's four elements of a row-major block
  int info = 0;
  double sv[4] = {0.0, 0.0, 0.0, 0.0};  // wave 1: row r of -M_l after frame l's sweep
  GnFrameLoads<RP> ld;
  if (wv == 0) {
    gn_zero_stage<RP>(st);
    gn_load_frame<RP>(a, f0, ld);
  } else if (i < NV) {
    C.z[i] = 0.0;  // (gn_couple_mfma's right-hand-side column: not used here)
  }
  for (int j = 0; j <= L; ++j) {
    if (wv == 0) {
      if (j < L) {
        const GnFrameLoads<RP> cu = ld;
        if (j + 1 < L) gn_load_frame<RP>(a, f0 + j + 1, ld);
        gn_build_frame<RP, false>(a, f0 + j, cu, st, blk[j % R]);
      }
    } else if (j > 0 && !info) {
      const int l = j - 1;
      const double* bc = blk[l % R];
#pragma unroll
      for (int c = 0; c < 4; ++c) sv[c] = bc[e0 + c] + (r == c0 + c ? a.lambda : 0.0);
      double b = 0.0;
      if (l > 0)  // G_{l-1} = M_{l-1} E_{l-1} (to the workspace for the backward pass)
        gn_couple_mfma<false>(C.M, C.z, blk[(l + R - 1) % R] + NB, nullptr,
                              full ? ws + (size_t)(l - 1) * MG_WSF + NB : nullptr, C.G, r, c0, sv, b);
      if (!gn_sweep(sv, C.rk2, r, c0, act)) {
        info = l + 1;  // idles through the remaining frames' barriers
      } else {
        wave_order();
        if (act) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            C.M[e0 + c] = -sv[c];
            if (full) ws[(size_t)l * MG_WSF + e0 + c] = -sv[c];
          }
        }
        wave_order();
      }
    }
    lds_barrier();
  }
  if (wv == 0) return;
  if (i == 0) a.info[t] = info;
  double* covt = full ? cov + (size_t)f0 * NB : nullptr;
  double* crt = cross ? cross + (size_t)t * (L - 1) * NB : nullptr;
  double* nwt = cov_newest ? cov_newest + (size_t)t * NB : nullptr;
  if (info) {
    if (covt)
      for (int e = i; e < L * NB; e += 64) covt[e] = NAN;
    if (crt)
      for (int e = i; e < (L - 1) * NB; e += 64) crt[e] = NAN;
    if (nwt)
      for (int e = i; e < NB; e += 64) nwt[e] = NAN;
    return;
  }
  // X -> (X + X^T) / 2 (lane: its four elements of X in, of the result out)
  auto sym = [&](const double (&x)[4], double (&y)[4]) __attribute__((always_inline)) {
    wave_order();  // every lane is past its reads of Ps
    if (act) {
#pragma unroll
      for (int c = 0; c < 4; ++c) Ps[e0 + c] = x[c];
    }
    wave_order();
#pragma unroll
    for (int c = 0; c < 4; ++c) y[c] = 0.5 * (x[c] + Ps[(c0 + c) * NV + r]);
  };
  double s[4];  // Sigma_l, this lane's elements
  {
    const double m[4] = {-sv[0], -sv[1], -sv[2], -sv[3]};
    sym(m, s);  // Sigma_{L-1} = M_{L-1}
  }
  if (act) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (covt) covt[(size_t)(L - 1) * NB + e0 + c] = s[c];
      if (nwt) nwt[e0 + c] = s[c];
    }
  }
  if (!full) return;
  // M_l / G_l were stored by other lanes of this wave: the stores have reached the L2 and no
  // stale line of the vector L1 serves the loads
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
  double mn[4], gnx[4];
  auto load = [&](int l) __attribute__((always_inline)) {
    const double* w = ws + (size_t)l * MG_WSF + e0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      mn[c] = w[c];
      gnx[c] = w[NB + c];
    }
  };
  load(L - 2);
  for (int l = L - 2; l >= 0; --l) {
    const double mc[4] = {mn[0], mn[1], mn[2], mn[3]}, gc[4] = {gnx[0], gnx[1], gnx[2], gnx[3]};
    if (l > 0) load(l - 1);
    wave_order();  // every lane is past its reads of Sg / Gs
    if (act) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        Sg[e0 + c] = s[c];
        Gs[e0 + c] = gc[c];
      }
    }
    wave_order();
    double p[4] = {0.0, 0.0, 0.0, 0.0};  // P = G_l Sigma_{l+1}
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const double g = Gs[r * NV + k];
#pragma unroll
      for (int c = 0; c < 4; ++c) p[c] = fma(g, Sg[k * NV + c0 + c], p[c]);
    }
    wave_order();  // (Ps: sym's reads of the previous frame)
    if (act) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        Ps[e0 + c] = p[c];
        if (crt) crt[(size_t)l * NB + e0 + c] = -p[c];
      }
    }
    wave_order();
    double u[4] = {mc[0], mc[1], mc[2], mc[3]};  // M_l + P G_l^T
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const double pk = Ps[r * NV + k];
#pragma unroll
      for (int c = 0; c < 4; ++c) u[c] = fma(pk, Gs[(c0 + c) * NV + k], u[c]);
    }
    sym(u, s);
    if (act) {
#pragma unroll
      for (int c = 0; c < 4; ++c) covt[(size_t)l * NB + e0 + c] = s[c];
    }
  }
}

}  // namespace pa

extern "C" {

size_t pa_trajectory_marginals_workspace(int T, int L) {
  return (T > 0 && L > 0) ? (size_t)T * L * pa::MG_WSF * sizeof(double) : 0;
}

// pa_trajectory_marginals with the marginalization prior on frame 0 (prior_info / prior_grad null: none)
// and the constant-velocity factor on the angular velocity (r_cw null: none); both null: the parent
int pa_trajectory_marginals_cw(int T, int L, int n_kp, const double* r_proj, const double* j_proj,
                               const int32_t* status_proj, const double* r_dyn, const double* j_dyn0,
                               const double* j_dyn1, const double* j_dyn2, const double* j_dyn3, const double* r_cv,
                               const double* j_cv0, const double* j_cv1, const double* r_cw, const double* isig_cw,
                               double lambda, double* cov, double* cross, double* cov_newest, int32_t* info, void* ws,
                               size_t ws_bytes, const double* prior_info, const double* prior_grad, void* stream) {
  PA_CHECK(T >= 0 && L >= 2 && n_kp >= 0 && n_kp <= pa::GN_KMAX, "marginals: T %d L %d (>= 2) n_kp %d (<= %d)", T, L,
           n_kp, pa::GN_KMAX);
  if (T == 0) return PA_OK;
  PA_CHECK(lambda >= 0.0, "marginals: lambda %g < 0", lambda);
  PA_CHECK(cov || cov_newest, "marginals: null cov and cov_newest (one of them is required)");
  PA_CHECK(!cross || cov, "marginals: cross is given with cov only");
  PA_CHECK(info && ws, "marginals: null info / workspace pointer");
  PA_CHECK(!prior_info == !prior_grad, "marginals: prior_info and prior_grad are given together (or both NULL)");
  PA_CHECK(n_kp == 0 || (r_proj && j_proj), "marginals: null projection factors");
  PA_CHECK(r_dyn && j_dyn0 && j_dyn1 && j_dyn2 && j_dyn3 && r_cv && j_cv0 && j_cv1,
           "marginals: null dynamics / constant-velocity factors (Jacobians are required)");
  PA_CHECK(ws_bytes >= pa_trajectory_marginals_workspace(T, L), "marginals: workspace %zu < %zu", ws_bytes,
           pa_trajectory_marginals_workspace(T, L));
  const pa::GnArgs a{T,     L,     n_kp,  r_proj, j_proj,  status_proj, r_dyn,   j_dyn0,  j_dyn1, j_dyn2,      j_dyn3,
                     r_cv,  j_cv0, j_cv1, lambda, nullptr, nullptr,     nullptr, nullptr, info,   (double*)ws, nullptr,
                     prior_info, prior_grad, r_cw, isig_cw};
  PA_CHECK(!r_cw || isig_cw,
           "marginals: r_cw is given without isig_cw (the factor's Jacobians are -+ diag(isig_cw))");
  const hipStream_t s = (hipStream_t)stream;
  pa::gn_for_kp(n_kp, [&](auto rp) {
    hipLaunchKernelGGL(pa::gn_marginals_kernel<decltype(rp)::value>, dim3(T), dim3(128), 0, s, a, cov, cross,
                       cov_newest);
  });
  PA_LAUNCH_CHECK();
  return PA_OK;
}

int pa_trajectory_marginals_prior(int T, int L, int n_kp, const double* r_proj, const double* j_proj,
                                  const int32_t* status_proj, const double* r_dyn, const double* j_dyn0,
                                  const double* j_dyn1, const double* j_dyn2, const double* j_dyn3,
                                  const double* r_cv, const double* j_cv0, const double* j_cv1, double lambda,
                                  double* cov, double* cross, double* cov_newest, int32_t* info, void* ws,
                                  size_t ws_bytes, const double* prior_info, const double* prior_grad,
                                  void* stream) {
  return pa_trajectory_marginals_cw(T, L, n_kp, r_proj, j_proj, status_proj, r_dyn, j_dyn0, j_dyn1, j_dyn2, j_dyn3,
                                    r_cv, j_cv0, j_cv1, nullptr, nullptr, lambda, cov, cross, cov_newest, info, ws,
                                    ws_bytes, prior_info, prior_grad, stream);
}

int pa_trajectory_marginals(int T, int L, int n_kp, const double* r_proj, const double* j_proj,
                            const int32_t* status_proj, const double* r_dyn, const double* j_dyn0,
                            const double* j_dyn1, const double* j_dyn2, const double* j_dyn3, const double* r_cv,
                            const double* j_cv0, const double* j_cv1, double lambda, double* cov, double* cross,
                            double* cov_newest, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
  return pa_trajectory_marginals_prior(T, L, n_kp, r_proj, j_proj, status_proj, r_dyn, j_dyn0, j_dyn1, j_dyn2, j_dyn3, r_cv, j_cv0,
                        j_cv1, lambda, cov, cross, cov_newest, info, ws, ws_bytes, nullptr, nullptr, stream);
}

}  // extern "C"
