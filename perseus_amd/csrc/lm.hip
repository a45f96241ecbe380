// pa_trajectory_lm_solve / pa_window_lm_solve and their ..._lm_prior_solve siblings (the
// marginalization prior on frame 0 in the cost and the steps): Levenberg-Marquardt per trajectory
// on the device, around the damped step of gn_cr_run (gn_cr_dev.h) and the factors of factors_dev.h.
#include "gn_cr_dev.h"
#include "prior_dev.h"

namespace pa {

// ---------------------------------------------------------------- Levenberg-Marquardt
// pa_trajectory_lm_solve: the accept / reject loop around the damped step, per trajectory, all
// of it on the device (no host synchronisation; the launches can be captured).  Two kernels,
// one workgroup per trajectory in each, built from the tick's device code:
//   lm_lin_kernel (6 waves)    the factors of a state (traj_dyn_block / traj_unit_wave on a T = 1
//        view, as pose_tick_lin_kernel), the cost C' = sum of err in a fixed order, and the
//        decision: accept iff C' < C (and no measurement lost to cheirality), lambda, the
//        convergence test, the outputs.  Launch 0 evaluates the initial state.
//   lm_step_kernel (12 waves)  (J^T J + lambda_t I) delta = -J^T r by gn_cr_run with the
//        trajectory's own lambda from device memory, then the trial state x' = retract(x, delta)
//        (window_retract_one on a copy of x).
// so a solve is 1 + 2 max_iters launches.  (One kernel for both would hold the dynamics factors'
// ~220 VGPRs at three waves per SIMD, see pose_tick_lin_kernel.)  The trial state is linearized
// into the factor set that is NOT current (set 0: the caller's outputs, set 1: the workspace's);
// an accepted step flips the trajectory's selector, a rejected one costs no re-linearization.
// A trajectory that stops leaves its final linearization in the caller's outputs (copied from
// set 1 if that was current) and its workgroups return at once in every later launch.  No
// workgroup reads what another writes within a launch.
//
// With a marginalization prior on frame 0 (pa_trajectory_lm_prior_solve; prior.hip):
//   cost    C = (the sum above) + e_prior, e_prior = sum_i xi_i (0.5 (Lambda xi)_i - eta_i) with xi at
//           frame 0 of the state being evaluated, by prior_lin_wave (pa_window_prior_linearize's
//           instructions), added last on the deciding lane with contraction off.  lm_lin_kernel's
//           last wave, which traj_lin_block leaves idle, evaluates it before the first barrier.
//   step    (J^T J + lambda_t I + Lambda on frame 0) delta = -(J^T r + (Lambda xi - eta) on frame 0):
//           GnArgs.p_info / p_grad.  The gradient belongs to a linearization, so it lives per
//           factor set (set 0: the caller's prior->grad, set 1: the workspace's), is written with
//           the target set's factors and goes to the caller with them when a trajectory stops
//           with set 1 current.
//   sign    -eta^T xi has no lower bound, so C may be negative: the convergence test is
//           C - C' <= rel_tol |C| + abs_tol (the same bits where C >= 0).
struct LmPriorDev {
  const double *info, *eta, *xp, *xw, *xv;  // the caller's prior; info == nullptr: none
  double *g0, *g1;                          // (T, 12) the gradient of set 0 (the caller's), set 1 (the workspace's)
  double *err, *err_out;                    // (T) e_prior at the current state (workspace), the caller's or nullptr
};
struct LmDev {
  FactorSetReq s0, s1;           // the caller's factor outputs, the workspace's (the required ones; cw0 / cw1 below)
  double *pose, *vel, *angvel;   // the trial state (T*L, 12 / 3 / 3)
  double* delta;                 // (T*L, 12)
  double *C, *lam;               // (T) the current cost and damping
  int32_t *done, *cur, *info;    // (T) status once stopped (0: running), current set, pivot failure
  double* hist;                  // (T, max_iters + 1): the caller's cost_hist or the workspace's
  double *cost0, *cost, *lam_out;
  int32_t *iters, *status;
  pa_lm_params p;
  int pending;  // the newest frame's keypoints are not in yet (pa_window_lm_solve): its projections get status 3
  LmPriorDev pr;
  // the factor on the angular velocity: its outputs in set 0 / set 1 (r_cw null in both: off) and
  // its whitening.  Last, so that everything above sits where it did before the factor existed
  double *r_cw0, *err_cw0, *r_cw1, *err_cw1;
  const double* isig_cw;
};

// set `which`: per pointer a select between the two kernel-argument structs (uniform; an indexed
// copy, sets[which], would put both sets in scratch)
__device__ __forceinline__ FactorSet lm_pick(const LmDev& d, int which) {
  const bool w = which != 0;
  FactorSet s;
#define PA_X(f, V, n, u) s.f = w ? d.s1.f : d.s0.f;
  PA_FACTOR_OUTPUTS(PA_X)
#undef PA_X
  s.r_cw = w ? d.r_cw1 : d.r_cw0;
  s.err_cw = w ? d.err_cw1 : d.err_cw0;
  return s;
}

// loads of what this workgroup's other waves stored earlier in the launch (after a
// __syncthreads): device-scope loads, served by the L2 the stores went through to
__device__ __forceinline__ double lm_ld(const double* p) {
  return __builtin_bit_cast(double, __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ int32_t lm_ld(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename V>
__device__ __forceinline__ void lm_copy(V* dst, const V* src, long n) {
  for (long e = threadIdx.x; e < n; e += blockDim.x) dst[e] = lm_ld(src + e);
}

// launch k = 0: the initial state (ta.pose / vel / angvel) into set 0; k >= 1: the trial state of
// iteration k into the set that is not current, then the decision.  RB: ta.robust_proj names a
// robust noise model (the cost is then the sum of its rho; the decision logic is the same).
// PR: d.pr holds a prior on frame 0.  TM: ta carries real timestamps (dt_pair / kp_mask,
// factors_dev.h; traj_view hands the trajectory's slices on).  CW: ta carries the constant-velocity
// factor on the angular velocity (r_cw / err_cw): its err entries enter the cost right after
// err_cv's; CW = false is the code, the index layout and the bits it was
template <bool RB, bool PR, bool TM, bool CW>
__global__ __launch_bounds__(64 * TICK_LIN_W) void lm_lin_kernel(pa_traj_args ta, LmDev d, int k) {
  __shared__ __attribute__((aligned(16))) double st[LIN_STAGE];
  __shared__ int dec_s;
  const int t = blockIdx.x, L = ta.L, K = ta.n_kp, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int M1 = d.p.max_iters + 1;
  if (k > 0 && d.done[t] != 0) return;  // (uniform; nothing writes done[t] before the barriers below)
  const int cur = k > 0 ? d.cur[t] : 0;
  const int tgt = k > 0 ? 1 - cur : 0;
  const bool pivot = k > 0 && d.info[t] != 0;  // the step's solve failed: a reject, nothing to evaluate
  [[maybe_unused]] const double* pe_p = nullptr;
  const FactorSet so = lm_pick(d, tgt), sc = lm_pick(d, cur);
  const long f0 = (long)t * L, p0 = f0 * K, d0 = (long)t * (L - 1);
  double* xp = const_cast<double*>(ta.pose) + f0 * 12;
  double* xv = const_cast<double*>(ta.vel) + f0 * 3;
  double* xw = const_cast<double*>(ta.angvel) + f0 * 3;
  if (!pivot) {
    pa_traj_args a1 = traj_view<false>(ta, t, so);  // (lm_solve_impl requires every output)
    a1.pose = k > 0 ? d.pose + f0 * 12 : xp;  // (the trial state)
    a1.vel = k > 0 ? d.vel + f0 * 3 : xv;
    a1.angvel = k > 0 ? d.angvel + f0 * 3 : xw;
    traj_lin_block<RB, TM, CW>(a1, st);
    if constexpr (PR) {
      // the prior at frame 0 of the state just linearized: grad to the target set, e_prior to wave 0
      __shared__ double pxi[gn::NV], pes[gn::NV], pe_s;
      if (wv == TICK_LIN_W - 1) {
        const LmPriorDev& q = d.pr;
        const double e = prior_lin_wave(lane, q.info + (size_t)t * gn::NB, q.eta + (size_t)t * gn::NV,
                                        q.xp + (size_t)t * 12, q.xw + (size_t)t * 3, q.xv + (size_t)t * 3, a1.pose,
                                        a1.angvel, a1.vel, (tgt ? q.g1 : q.g0) + (size_t)t * gn::NV, pxi, pes);
        if (lane == 0) pe_s = e;
      }
      pe_p = &pe_s;
    }
  }
  if (k == 0)
    for (int e = 1 + (int)threadIdx.x; e < M1; e += 64 * TICK_LIN_W) d.hist[(size_t)t * M1 + e] = NAN;
  __syncthreads();  // every factor store of this trajectory is done
  if (wv == 0) {
    // C' = the dynamics, constant-velocity and status-0 projection errors in a fixed order: lane
    // j sums entries j, j + 64, ..., then a butterfly over the lanes (the same sum on every lane).
    // bad: a projection the current state measures (status 0) is behind the camera at the trial
    double s = 0.0;
    bool bad = false;
    if (!pivot) {
      constexpr int NPF = CW ? 3 : 2;  // pair factors: dynamics, constant velocity (, angular velocity)
      const int nd = L - 1, np = L * K, n = NPF * nd + np;
      for (int i = lane; i < n; i += 64) {
        double v;
        if (i < nd) {
          v = lm_ld(so.err_dyn + d0 + i);
        } else if (i < 2 * nd) {
          v = lm_ld(so.err_cv + d0 + i - nd);
        } else if (CW && i < 3 * nd) {
          v = lm_ld(so.err_cw + d0 + i - 2 * nd);
        } else {
          const int j = i - NPF * nd;
          int32_t sn = lm_ld(so.status + p0 + j);
          if (d.pending && j >= (L - 1) * K) {  // out of the cost, the guard and (status 3) the step's assembly
            sn = 3;
            so.status[p0 + j] = 3;
          }
          const double e = lm_ld(so.err_proj + p0 + j);
          v = sn == 0 ? e : 0.0;
          if (k > 0 && sn == 1 && sc.status[p0 + j] == 0) bad = true;
        }
        s += v;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    }
    const bool anybad = __ballot(bad) != 0ull;
    if (lane == 0) {
#pragma clang fp contract(off)
      const pa_lm_params& p = d.p;
      double C, lam;
      int status = 0, acc = 0, ncur = cur;
      [[maybe_unused]] double pe = 0.0;
      if constexpr (PR) {
        if (!pivot) {
          pe = *pe_p;
          s = s + pe;
        }
      }
      if (k == 0) {
        C = s;
        lam = p.lambda0;
        d.cost0[t] = C;
      } else {
        C = d.C[t];
        lam = d.lam[t];
        if (!pivot && !anybad && s < C) {
          acc = 1;
          ncur = tgt;
          lam = fmax(lam / p.lambda_down, p.lambda_min);
          const double tol = p.rel_tol * fabs(C);
          if (C - s <= tol + p.abs_tol) status = PA_LM_CONVERGED;
          C = s;
        } else {
          lam = lam * p.lambda_up;
          if (lam > p.lambda_max) status = PA_LM_STALLED;
        }
        if (status == 0 && k == p.max_iters) status = PA_LM_MAX_ITERS;
      }
      d.C[t] = C;
      d.lam[t] = lam;
      d.cur[t] = ncur;
      d.done[t] = status;
      d.hist[(size_t)t * M1 + k] = C;
      d.cost[t] = C;
      d.lam_out[t] = lam;
      d.iters[t] = k;
      d.status[t] = status;
      if constexpr (PR) {  // e_prior at the current state: the evaluated one's on launch 0 and on an accept
        const double ce = (k == 0 || acc) ? pe : d.pr.err[t];
        d.pr.err[t] = ce;
        if (d.pr.err_out) d.pr.err_out[t] = ce;
      }
      dec_s = acc | (status != 0 ? 2 : 0) | (ncur << 2);
    }
  }
  __syncthreads();
  const int dec = dec_s;
  if (dec & 1) {  // accepted: x = x'
    lm_copy(xp, d.pose + f0 * 12, (long)L * 12);
    lm_copy(xv, d.vel + f0 * 3, (long)L * 3);
    lm_copy(xw, d.angvel + f0 * 3, (long)L * 3);
  }
  if ((dec & 2) && (dec >> 2)) {  // stopped with set 1 current: the final linearization to the caller's outputs
    const long np = (long)L * K, nd = L - 1;
#define PA_X(f, V, n, u) \
  lm_copy(d.s0.f + factor_units(u, p0, d0) * n, d.s1.f + factor_units(u, p0, d0) * n, factor_units(u, np, nd) * n);
    PA_FACTOR_OUTPUTS(PA_X)
#undef PA_X
    if constexpr (CW) {
      lm_copy(d.r_cw0 + d0 * 3, d.r_cw1 + d0 * 3, nd * 3);
      lm_copy(d.err_cw0 + d0, d.err_cw1 + d0, nd);
    }
    if constexpr (PR) lm_copy(d.pr.g0 + (size_t)t * gn::NV, d.pr.g1 + (size_t)t * gn::NV, (long)gn::NV);
  }
}

// iteration k's damped step from the current set, then the trial state into d.pose / vel / angvel.
// PR: with d.pr's Lambda and the current set's prior gradient on frame 0 (the instantiations
// without it are the code they were before the prior existed)
template <int RP, bool PR>
__global__ __launch_bounds__(64 * GN_CR_W, 1) void lm_step_kernel(int T, int L, int K, LmDev d,
                                                                   const double* __restrict__ pose,
                                                                   const double* __restrict__ vel,
                                                                   const double* __restrict__ angvel) {
  constexpr int NS = GN_CR_NS<RP>;
  using Ld = GnCrLds<RP, NS>;
  __shared__ __attribute__((aligned(16))) double fb[Ld::LM][Ld::BLK];
  __shared__ __attribute__((aligned(16))) double pool[Ld::POOL];
  const int t = blockIdx.x;
  if (d.done[t] != 0) return;  // (uniform)
  const int cur = d.cur[t];
  GnArgs g = gn_args(T, L, K, lm_pick(d, cur), d.lam[t], d.delta, d.info, nullptr, d.isig_cw);
  if constexpr (PR) {
    g.p_info = d.pr.info;
    g.p_grad = cur ? d.pr.g1 : d.pr.g0;
  }
  gn_cr_run<RP, NS>(g, t, fb, pool);
  __syncthreads();
  if ((int)threadIdx.x < L) {
    const long f = (long)t * L + threadIdx.x;
#pragma unroll
    for (int i = 0; i < 12; ++i) d.pose[f * 12 + i] = pose[f * 12 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      d.vel[f * 3 + i] = vel[f * 3 + i];
      d.angvel[f * 3 + i] = angvel[f * 3 + i];
    }
    window_retract_one(f, L, d.delta, d.info, d.pose, d.angvel, d.vel, nullptr);
  }
}

// the workspace: set 1 of the factor outputs, the trial state, delta, the per-trajectory LM
// state and a cost history (used when the caller passes none); with a prior, after all of that,
// set 1's prior gradient (T, 12) and the current e_prior (T); every array 16-B aligned
struct LmLayout {
#define PA_X(f, V, n, u) size_t f;
  PA_FACTOR_OUTPUTS_ALL(PA_X)
#undef PA_X
  size_t pose, vel, angvel, delta, C, lam, done, cur, info, hist, pgrad, perr, bytes;
};
static LmLayout lm_layout(int T, int L, int K, int max_iters, bool prior) {
  LmLayout o;
  size_t at = 0;
  auto take = [&](size_t n, size_t el) {
    const size_t r = at;
    at += (n * el + 15) / 16 * 16;
    return r;
  };
  const size_t F = (size_t)T * L, np = F * K, nd = (size_t)T * (L - 1);
#define PA_X(f, V, n, u) o.f = take(factor_units(u, np, nd) * n, sizeof(V));
  PA_FACTOR_OUTPUTS_ALL(PA_X)  // (the optional pair always has its room: the size does not depend on the switch)
#undef PA_X
  o.pose = take(F * 12, 8);
  o.vel = take(F * 3, 8);
  o.angvel = take(F * 3, 8);
  o.delta = take(F * 12, 8);
  o.C = take(T, 8);
  o.lam = take(T, 8);
  o.done = take(T, 4);
  o.cur = take(T, 4);
  o.info = take(T, 4);
  o.hist = take((size_t)T * ((size_t)max_iters + 1), 8);
  o.pgrad = o.perr = at;
  if (prior) {
    o.pgrad = take((size_t)T * 12, 8);
    o.perr = take(T, 8);
  }
  o.bytes = at;
  return o;
}

template <bool CW>
static auto lm_lin_pick(bool rb, bool prior, bool tm) {
  return tm ? (prior ? (rb ? lm_lin_kernel<true, true, true, CW> : lm_lin_kernel<false, true, true, CW>)
                     : (rb ? lm_lin_kernel<true, false, true, CW> : lm_lin_kernel<false, false, true, CW>))
            : (prior ? (rb ? lm_lin_kernel<true, true, false, CW> : lm_lin_kernel<false, true, false, CW>)
                     : (rb ? lm_lin_kernel<true, false, false, CW> : lm_lin_kernel<false, false, false, CW>));
}

}  // namespace pa

extern "C" {

size_t pa_trajectory_lm_workspace(int T, int L, int n_kp, int max_iters) {
  if (T < 1 || L < 2 || L > pa::GN_CR_LMAX || n_kp < 1 || n_kp > pa::GN_KMAX || max_iters < 1) return 0;
  return pa::lm_layout(T, L, n_kp, max_iters, false).bytes;
}

size_t pa_trajectory_lm_prior_workspace(int T, int L, int n_kp, int max_iters) {
  if (T < 1 || L < 2 || L > pa::GN_CR_LMAX || n_kp < 1 || n_kp > pa::GN_KMAX || max_iters < 1) return 0;
  return pa::lm_layout(T, L, n_kp, max_iters, true).bytes;
}

static int lm_solve_impl(const pa_traj_args* ta, const pa_lm_params* p, int pending, const pa_lm_prior* prior,
                         double* cost0, double* cost, int32_t* iters, int32_t* status, double* lambda,
                         double* cost_hist, void* ws, size_t ws_bytes, void* stream) {
  PA_CHECK(ta && p, "lm: null args / params");
  PA_CHECK(!prior || (prior->info && prior->eta && prior->xbar_pose && prior->xbar_angvel && prior->xbar_vel),
           "lm: null info / eta / xbar_pose / xbar_angvel / xbar_vel in a non-null prior");
  PA_CHECK(!prior || prior->grad, "lm: null grad in a non-null prior (the final gradient is a required output)");
  if (const int rc = pa::robust_check(*ta, "lm")) return rc;
  const int T = ta->T, L = ta->L, K = ta->n_kp;
  PA_CHECK(T >= 0 && L >= 2 && L <= pa::GN_CR_LMAX && K >= 1 && K <= pa::GN_KMAX,
           "lm: T %d, L %d (2..%d), n_kp %d (1..%d)", T, L, pa::GN_CR_LMAX, K, pa::GN_KMAX);
  PA_CHECK(p->max_iters >= 1, "lm: max_iters %d < 1", p->max_iters);
  PA_CHECK(p->lambda0 > 0.0 && p->lambda0 < INFINITY, "lm: lambda0 %g is not a positive finite number", p->lambda0);
  PA_CHECK(p->lambda_up > 1.0 && p->lambda_up < INFINITY, "lm: lambda_up %g must be > 1", p->lambda_up);
  PA_CHECK(p->lambda_down > 1.0 && p->lambda_down < INFINITY, "lm: lambda_down %g must be > 1", p->lambda_down);
  PA_CHECK(p->lambda_min >= 0.0 && p->lambda_max >= p->lambda_min,
           "lm: lambda_min %g, lambda_max %g (0 <= lambda_min <= lambda_max)", p->lambda_min, p->lambda_max);
  PA_CHECK(p->rel_tol >= 0.0 && p->abs_tol >= 0.0, "lm: rel_tol %g, abs_tol %g must be >= 0", p->rel_tol, p->abs_tol);
  if (T == 0) return PA_OK;
  PA_CHECK(ta->y && ta->pose && ta->vel && ta->angvel && ta->corners && ta->K, "lm: null state / model pointer");
  PA_CHECK(ta->isig_proj, "lm: null isig_proj (the cost is defined on whitened residuals)");
  PA_CHECK(ta->isig_dyn, "lm: null isig_dyn (the cost is defined on whitened residuals)");
  PA_CHECK(ta->isig_cv, "lm: null isig_cv (the cost is defined on whitened residuals)");
#define PA_X(f, V, n, u) PA_CHECK(ta->f, "lm: null factor output " #f " (every output and Jacobian is required)");
  PA_FACTOR_OUTPUTS(PA_X)
#undef PA_X
  PA_CHECK(cost0 && cost && iters && status && lambda, "lm: null cost0 / cost / iters / status / lambda output");
  const pa::LmLayout o = pa::lm_layout(T, L, K, p->max_iters, prior != nullptr);
  PA_CHECK(ws && ws_bytes >= o.bytes, "lm: workspace %zu < %zu", ws ? ws_bytes : (size_t)0, o.bytes);
  PA_CHECK(((uintptr_t)ws & 15) == 0, "lm: workspace not 16-byte aligned");
  // the factor on the angular velocity (r_cw switches it on; off, neither of the two is looked at)
  PA_CHECK(!ta->r_cw || ta->isig_cw, "lm: r_cw is given without isig_cw (the cost is defined on whitened residuals)");
  PA_CHECK(!ta->r_cw || ta->err_cw, "lm: r_cw is given without err_cw (the cost sums the factor's err)");
  char* w = (char*)ws;
  auto f64 = [&](size_t off) { return (double*)(w + off); };
  auto i32 = [&](size_t off) { return (int32_t*)(w + off); };
  pa::LmDev d;
  d.s0 = pa::factor_set(*ta);
#define PA_X(f, V, n, u) d.s1.f = (V*)(w + o.f);
  PA_FACTOR_OUTPUTS(PA_X)
#undef PA_X
  const bool cw = ta->r_cw != nullptr;
  d.r_cw0 = ta->r_cw;
  d.err_cw0 = cw ? ta->err_cw : nullptr;
  d.r_cw1 = cw ? f64(o.r_cw) : nullptr;  // (off in both sets)
  d.err_cw1 = cw ? f64(o.err_cw) : nullptr;
  d.isig_cw = ta->isig_cw;
  d.pose = f64(o.pose);
  d.vel = f64(o.vel);
  d.angvel = f64(o.angvel);
  d.delta = f64(o.delta);
  d.C = f64(o.C);
  d.lam = f64(o.lam);
  d.done = i32(o.done);
  d.cur = i32(o.cur);
  d.info = i32(o.info);
  d.hist = cost_hist ? cost_hist : f64(o.hist);
  d.cost0 = cost0;
  d.cost = cost;
  d.lam_out = lambda;
  d.iters = iters;
  d.status = status;
  d.p = *p;
  d.pending = pending;
  d.pr = pa::LmPriorDev{};
  if (prior)
    d.pr = pa::LmPriorDev{prior->info, prior->eta, prior->xbar_pose, prior->xbar_angvel, prior->xbar_vel,
                          prior->grad, f64(o.pgrad), f64(o.perr), prior->err};
  const hipStream_t s = (hipStream_t)stream;
  const bool rb = ta->robust_proj != PA_ROBUST_NONE;
  const bool tm = ta->dt_pair || ta->kp_mask;
  const auto lin_kernel = cw ? pa::lm_lin_pick<true>(rb, prior != nullptr, tm) : pa::lm_lin_pick<false>(rb, prior != nullptr, tm);
  for (int k = 0; k <= p->max_iters; ++k) {
    if (k > 0)
      pa::gn_for_kp(K, [&](auto rp) {
        constexpr int RP = decltype(rp)::value;
        const auto step_kernel = prior ? pa::lm_step_kernel<RP, true> : pa::lm_step_kernel<RP, false>;
        hipLaunchKernelGGL(step_kernel, dim3(T), dim3(64 * pa::GN_CR_W), 0, s, T, L, K, d, ta->pose, ta->vel,
                           ta->angvel);
      });
    hipLaunchKernelGGL(lin_kernel, dim3(T), dim3(64 * pa::TICK_LIN_W), 0, s, *ta, d, k);
  }
  PA_LAUNCH_CHECK();
  return PA_OK;
}

int pa_trajectory_lm_prior_solve(const pa_traj_args* ta, const pa_lm_params* p, const pa_lm_prior* prior,
                                 double* cost0, double* cost, int32_t* iters, int32_t* status, double* lambda,
                                 double* cost_hist, void* ws, size_t ws_bytes, void* stream) {
  return lm_solve_impl(ta, p, 0, prior, cost0, cost, iters, status, lambda, cost_hist, ws, ws_bytes, stream);
}

int pa_window_lm_prior_solve(const pa_traj_args* ta, const pa_lm_params* p, int newest_pending,
                             const pa_lm_prior* prior, double* cost0, double* cost, int32_t* iters, int32_t* status,
                             double* lambda, double* cost_hist, void* ws, size_t ws_bytes, void* stream) {
  return lm_solve_impl(ta, p, newest_pending != 0, prior, cost0, cost, iters, status, lambda, cost_hist, ws, ws_bytes,
                       stream);
}

int pa_trajectory_lm_solve(const pa_traj_args* ta, const pa_lm_params* p, double* cost0, double* cost, int32_t* iters,
                           int32_t* status, double* lambda, double* cost_hist, void* ws, size_t ws_bytes,
                           void* stream) {
  return pa_trajectory_lm_prior_solve(ta, p, nullptr, cost0, cost, iters, status, lambda, cost_hist, ws, ws_bytes,
                                      stream);
}

int pa_window_lm_solve(const pa_traj_args* ta, const pa_lm_params* p, int newest_pending, double* cost0, double* cost,
                       int32_t* iters, int32_t* status, double* lambda, double* cost_hist, void* ws, size_t ws_bytes,
                       void* stream) {
  return pa_window_lm_prior_solve(ta, p, newest_pending, nullptr, cost0, cost, iters, status, lambda, cost_hist, ws,
                                  ws_bytes, stream);
}

}  // extern "C"
