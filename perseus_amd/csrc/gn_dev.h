// Device code of the Gauss-Newton step shared by gn.hip (pa_trajectory_gn_step), pose_tick.hip
// (the streaming pose tick) and lm.hip (the LM solve): the kernel arguments, one frame's
// assembly, and the pieces of the block-Thomas chain (coupling, swept inverse).  The cyclic
// reduction built on them is gn_cr_dev.h; gn.hip's opening comment has the design.
#pragma once
#include <type_traits>

#include "common.h"
#include "factors_dev.h"

namespace pa {

namespace gn {
constexpr int NV = 12;  // variables per frame
constexpr int NB = NV * NV;
}  // namespace gn

struct GnArgs {
  int T, L, K;
  const double *r_proj, *j_proj;
  const int32_t* st_proj;
  const double *r_dyn, *j0, *j1, *j2, *j3, *r_cv, *jc0, *jc1;
  double lambda;
  double *D, *E, *g, *delta;
  int32_t* info;
  double* ws;
  unsigned long long* trace;  // timing only (pa_debug_gn_set_trace): 256 s_memrealtime stamps per trajectory
  // the marginalization prior on frame 0 (prior.hip): Lambda (T, 12, 12) and its gradient
  // Lambda xi - eta (T, 12), added to D_0 / g_0 by gn_build_frame; null = no prior
  const double *p_info, *p_grad;
  // the constant-velocity factor on the angular velocity (pa_traj_args.r_cw): its whitened
  // residuals (T*(L-1), 3) and its whitening (3), folded into the blocks in closed form by
  // gn_build_frame; r_cw null = off
  const double *r_cw, *isig_cw;
};

// the step on the factor set s (delta only: no D / E / g outputs, no trace); isig_cw: the
// whitening that goes with s.r_cw (not looked at when that is null)
__host__ __device__ __forceinline__ GnArgs gn_args(int T, int L, int K, const FactorSet& s, double lambda,
                                                   double* delta, int32_t* info, double* ws,
                                                   const double* isig_cw = nullptr) {
  return GnArgs{T,      L,        K,        s.r_proj, s.j_proj, s.status, s.r_dyn, s.j_dyn0, s.j_dyn1, s.j_dyn2, s.j_dyn3,
                s.r_cv, s.j_cv0,  s.j_cv1,  lambda,   nullptr,  nullptr,  nullptr, delta,    info,     ws,       nullptr,
                nullptr, nullptr, s.r_cw,   isig_cw};
}
// ... on the factor outputs ta names
inline GnArgs gn_args(const pa_traj_args& ta, double lambda, double* delta, int32_t* info, double* ws) {
  return gn_args(ta.T, ta.L, ta.n_kp, factor_set(ta), lambda, delta, info, ws, ta.isig_cw);
}

// assembler waves per trajectory and solver (pa_debug_gn_set_assemblers: na + 8 * legacy;
// 0 = the shipped choice); gn.hip defines it, pa_window_pose_tick reads its bits 1024 / 2048
extern int g_gn_na;

// slot s of trajectory t's trace (lane 0 of the calling wave only)
__device__ __forceinline__ void gn_stamp(const GnArgs& a, int t, int slot) {
  if (a.trace && (threadIdx.x & 63) == 0 && slot < 256) a.trace[(size_t)t * 256 + slot] = __builtin_amdgcn_s_memrealtime();
}

// ---------------------------------------------------------------- assembly
// One wave, frame l (of trajectory t).  The factor rows touching x_l are stacked in
// LDS, transposed, as A^T (12 x R, in x_l coordinates; zero rows for cheirality-failed
// projections) with their residuals r, and the rows of the factors (l, l+1) also as the
// 12 x 10 pair (A_next^T, B^T) (B: their x_{l+1} part):
//   projection k of frame l   2 rows  A = [J_k | 0 | 0]
//   dynamics (l, l+1)         6 rows  A = [J0 | J1 | J2]   B = [J3 | 0 | 0]
//   const-velocity (l, l+1)   3 rows  A = [0 | 0 | C0]     B = [0 | 0 | C1]
//   dynamics (l-1, l)         6 rows  A = [J3 | 0 | 0]
//   const-velocity (l-1, l)   3 rows  A = [0 | 0 | C1]
// Then D = A^T A, E = A_next^T B, g = A^T r as 108 work items (an output row i x 3
// columns, or one g entry) over the wave's lanes, reading 2 rows per 16-B LDS read.
constexpr int GN_KMAX = 16;  // keypoints per frame supported
// The kernels over frame assemblies are templates on RP, the factor rows per frame (2 K + 18):
// one instantiation for the cube's K = 8 and one that holds GN_KMAX.  f(rp) is called with
// the integral constant of the one for K keypoints.
template <typename F>
inline void gn_for_kp(int K, F&& f) {
  if (K == 8)
    f(std::integral_constant<int, 34>{});
  else
    f(std::integral_constant<int, 2 * GN_KMAX + 18>{});
}
constexpr int GN_WSF = 2 * gn::NB + 2 * gn::NV;  // workspace doubles per frame: L_l, W_l, y_l, 1 / diag(L_l)
// wave-local LDS ordering (one wave's ds ops run in order; the wait and the "memory" clobber
// keep the compiler from moving LDS accesses across it)
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// compiler-only fence: one wave's LDS instructions execute in issue order, so a read
// issued after another lane's write of the same wave sees it without a wait; this only
// keeps the compiler from moving LDS accesses across it
__device__ __forceinline__ void wave_order() { asm volatile("" ::: "memory"); }

// RP factor rows padded to whole 4-row MFMA k-steps (the pad rows stay zero)
// Rows 12..15 pad the variables to the MFMA's 16 so the operand reads need no lane test:
// AT row 12 holds r (B's column 12 -> g), AT rows 13..15 are don't-care (they only feed
// output rows / columns >= 13, never stored) and take the branch-free staging's dummy writes;
// ANT / BT rows 12..15 stay zero.
template <int RP>
struct GnStage {
  static constexpr int RPP = (RP + 3) / 4 * 4;
  double AT[16][RPP];
  double ANT[16][12];
  double BT[16][12];
};

static __device__ int32_t gn_zero_i32[1];  // status source when no status array is given (zero-initialised)
static __device__ double gn_zero_f64[2];   // projection source when K == 0 (the pointers may be null then)

// Assembles frame f (of trajectory t, frame index l) with one wave: D_l, E_l (if l + 1 < L)
// and g_l to the outputs a.D / a.E / a.g and to the LDS block `blk` (D | E | g).
// The per-lane values of one frame's factors (gn_load_frame), fetched before any is used.
template <int RP>
struct GnFrameLoads {
  static constexpr int KM = (RP - 18) / 2;        // keypoints this instantiation holds
  static constexpr int JR = (KM * 12 + 63) / 64;  // projection Jacobian entries per lane
  double jv[JR];
  int js[JR];
  double rv;
  int rs;
  double n0, n3, n1, n2, p3;
};

// Loads of frame f: every value is fetched from an address clamped to a valid element, then
// selected -- one memory latency per frame (branches around guarded loads made the compiler
// wait out each load in turn: ~10 round trips).  Nothing loaded decides a branch here, so a
// caller can issue the next frame's loads before building the current one.
template <int RP>
__device__ __forceinline__ void gn_load_frame(const GnArgs& a, long f, GnFrameLoads<RP>& ld) {
  constexpr int JR = GnFrameLoads<RP>::JR;
  const int lane = threadIdx.x & 63;
  const int t = (int)(f / a.L), l = (int)(f - (long)t * a.L);
  const int npair = a.L - 1;
  const int K = a.K;
  const bool nxt = l + 1 < a.L, prv = l > 0;
  const long fk = f * K;
  // (the status pointer test is uniform)
  const bool has_st = a.st_proj != nullptr;
  const int32_t* stp = has_st ? a.st_proj : gn_zero_i32;  // always a valid address
  // K == 0: every projection load below is clamped to element 0 of a valid dummy (the
  // caller may pass null projection arrays), and no lane uses the value
  const double* jproj = K > 0 ? a.j_proj : gn_zero_f64;
  const double* rproj = K > 0 ? a.r_proj : gn_zero_f64;
#pragma unroll
  for (int q = 0; q < JR; ++q) {
    const int e = lane + 64 * q;
    const bool v = e < K * 12;
    const long u = fk + (v ? e / 12 : 0);
    ld.jv[q] = jproj[v ? fk * 12 + e : (K > 0 ? fk * 12 : 0)];  // (u, c, row) = (e / 12, (e % 12) / 2, e & 1)
    ld.js[q] = stp[has_st ? u : 0];
  }
  const bool vr = lane < 2 * K;
  const long ur = fk + (vr ? lane >> 1 : 0);
  ld.rv = rproj[vr ? fk * 2 + lane : (K > 0 ? fk * 2 : 0)];
  ld.rs = stp[has_st ? ur : 0];
  // pair factors: lane classes [0, 36) dynamics J (6 x 6 column-major; < 18 also the 6 x 3
  // J1 / J2), [36, 45) constant velocity (3 x 3), [45, 51) dynamics r, [51, 54) const-vel r
  ld.n0 = ld.n3 = ld.n1 = ld.n2 = ld.p3 = 0.0;
  if (npair > 0) {
    const long un = (long)t * npair + (nxt ? l : 0), up = (long)t * npair + (prv ? l - 1 : 0);
    const int e36 = lane < 36 ? lane : 0, e9 = lane >= 36 && lane < 45 ? lane - 36 : 0;
    const int e6 = lane >= 45 && lane < 51 ? lane - 45 : 0, e3 = lane >= 51 && lane < 54 ? lane - 51 : 0;
    const int cls = lane < 36 ? 0 : lane < 45 ? 1 : lane < 51 ? 2 : lane < 54 ? 3 : 4;
    // per lane: the (l, l+1) factor's A-part value, its B-part value, and the (l-1, l) B-part
    const double* sa = cls == 0 ? a.j0 + un * 36 + e36 : cls == 1 ? a.jc0 + un * 9 + e9
                     : cls == 2 ? a.r_dyn + un * 6 + e6 : cls == 3 ? a.r_cv + un * 3 + e3 : a.j0;
    const double* sb = cls == 0 ? a.j3 + un * 36 + e36 : cls == 1 ? a.jc1 + un * 9 + e9 : a.j3;
    const double* sp = cls == 0 ? a.j3 + up * 36 + e36 : cls == 1 ? a.jc1 + up * 9 + e9
                     : cls == 2 ? a.r_dyn + up * 6 + e6 : cls == 3 ? a.r_cv + up * 3 + e3 : a.j3;
    const int e18 = lane < 18 ? lane : 0;
    ld.n0 = *sa;
    ld.n3 = *sb;
    ld.p3 = *sp;
    ld.n1 = a.j1[un * 18 + e18];
    ld.n2 = a.j2[un * 18 + e18];
  }
}

template <int RP, bool ZERO = true>
__device__ __forceinline__ void gn_build_frame(const GnArgs& a, long f, const GnFrameLoads<RP>& ld, GnStage<RP>& st,
                                               double* blk);

// the staging zeroed once (the pad rows and every position no factor writes stay zero;
// gn_build_frame<RP, false> then writes only the factor positions, zeros included)
template <int RP>
__device__ __forceinline__ void gn_zero_stage(GnStage<RP>& st) {
  const int lane = threadIdx.x & 63;
  for (int e = lane; e < (int)(sizeof(GnStage<RP>) / sizeof(double)); e += 64) (&st.AT[0][0])[e] = 0.0;
  wave_order();
}

template <int RP>
__device__ __forceinline__ void gn_assemble_frame(const GnArgs& a, long f, GnStage<RP>& st, double* blk) {
  GnFrameLoads<RP> ld;
  gn_load_frame<RP>(a, f, ld);
  gn_build_frame<RP>(a, f, ld, st, blk);
}

template <int RP, bool ZERO>
__device__ __forceinline__ void gn_build_frame(const GnArgs& a, long f, const GnFrameLoads<RP>& ld, GnStage<RP>& st,
                                               double* blk) {
  using namespace gn;
  constexpr int RPP = GnStage<RP>::RPP;
  constexpr int JR = GnFrameLoads<RP>::JR;
  double(&AT)[16][RPP] = st.AT;
  double(&rT)[RPP] = st.AT[NV];
  double(&ANT)[16][12] = st.ANT;
  double(&BT)[16][12] = st.BT;
  const int lane = threadIdx.x & 63;
  const int t = (int)(f / a.L), l = (int)(f - (long)t * a.L);
  const int npair = a.L - 1;
  const int K = a.K;
  const bool nxt = l + 1 < a.L, prv = l > 0;
  const bool vr = lane < 2 * K;
  const double(&jv)[JR] = ld.jv;
  const int(&js)[JR] = ld.js;
  const double rv = ld.rv, n0 = ld.n0, n3 = ld.n3, n1 = ld.n1, n2 = ld.n2, p3 = ld.p3;
  const int rs = ld.rs;
  // ---- staging: zero (ZERO; else once per launch, gn_zero_stage), then fill (one wave: its LDS
  // ops run in order).  Without the per-frame zeroing every factor position is written, with
  // 0 for a missing neighbour pair (first / last frame)
  if constexpr (ZERO) {
    for (int e = lane; e < NV * RPP; e += 64) (&AT[0][0])[e] = 0.0;
    for (int e = lane; e < NV * 12; e += 64) {
      (&ANT[0][0])[e] = 0.0;
      (&BT[0][0])[e] = 0.0;
    }
    for (int e = lane; e < RPP; e += 64) rT[e] = 0.0;
    wave_order();
  }
  typedef double d4_t __attribute__((ext_vector_type(4)));
  const int li = lane & 15, lk = lane >> 4;
  d4_t cD = {0.0, 0.0, 0.0, 0.0}, cE = {0.0, 0.0, 0.0, 0.0};
  const int rn = 2 * K, rp = rn + 9;  // first row of the (l, l+1) / (l-1, l) blocks
  if constexpr (!ZERO) {
    // branch-free staging: every lane writes its fixed positions (offsets in doubles from
    // AT[0][0]; unused slots go to the don't-care row 13 + lane / RPP), selects instead of
    // lane-class branches
    double* S = &AT[0][0];
    constexpr int OA = 0, ON = 16 * RPP, OB = 16 * RPP + 16 * 12;
    const int dummy = 13 * RPP + lane;
#pragma unroll
    for (int q = 0; q < JR; ++q) {
      const int e = lane + 64 * q;
      const int k = e / 12, c = (e - k * 12) >> 1, row = e & 1;
      S[e < K * 12 ? OA + c * RPP + 2 * k + row : dummy] = js[q] == 0 ? jv[q] : 0.0;
    }
    S[vr ? OA + NV * RPP + lane : dummy] = rs == 0 ? rv : 0.0;
    const double m0 = nxt ? n0 : 0.0, m3 = nxt ? n3 : 0.0, m1 = nxt ? n1 : 0.0, m2 = nxt ? n2 : 0.0;
    const double q3 = prv ? p3 : 0.0;
    const bool d36 = lane < 36, c9 = lane >= 36 && lane < 45, r6 = lane >= 45 && lane < 51, r3 = lane >= 51 && lane < 54;
    const int c6 = lane / 6, w6 = lane - c6 * 6;                  // dynamics: column, row
    const int c3 = (lane - 36) / 3, w3 = (lane - 36) - c3 * 3;    // const velocity (lane 36..44)
    auto at_row = [&](int r0) {  // AT offset of this lane's (l, l+1) or (l-1, l) element (rows from r0)
      return d36 ? OA + c6 * RPP + r0 + w6
           : c9  ? OA + (9 + c3) * RPP + r0 + 6 + w3
           : r6  ? OA + NV * RPP + r0 + lane - 45
           : r3  ? OA + NV * RPP + r0 + 6 + lane - 51
                 : dummy;
    };
    S[at_row(rn)] = m0;
    S[d36 ? ON + c6 * 12 + w6 : c9 ? ON + (9 + c3) * 12 + 6 + w3 : dummy] = m0;
    S[d36 ? OB + c6 * 12 + w6 : c9 ? OB + (9 + c3) * 12 + 6 + w3 : dummy] = m3;
    const bool d18 = lane < 18;
    S[d18 ? OA + (6 + c6) * RPP + rn + w6 : dummy] = m1;
    S[d18 ? ON + (6 + c6) * 12 + w6 : dummy] = m1;
    S[d18 ? OA + (9 + c6) * RPP + rn + w6 : dummy] = m2;
    S[d18 ? ON + (9 + c6) * 12 + w6 : dummy] = m2;
    S[at_row(rp)] = q3;
    wave_order();
    // [D_l | g_l] = A^T [A | r], E_l = A_next^T B: the operands straight from the padded rows
#pragma unroll
    for (int q = 0; q < RPP / 4; ++q) {
      const double v = AT[li][4 * q + lk];
      cD = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, cD, 0, 0, 0);
    }
    if (nxt) {
#pragma unroll
      for (int q = 0; q < 3; ++q)
        cE = __builtin_amdgcn_mfma_f64_16x16x4f64(ANT[li][4 * q + lk], BT[li][4 * q + lk], cE, 0, 0, 0);
    }
  } else {
    // projections: rows 2k, 2k + 1; J column-major 2 x 6
#pragma unroll
    for (int q = 0; q < JR; ++q) {
      const int e = lane + 64 * q;
      if (e < K * 12) {
        const int k = e / 12, c = (e - k * 12) >> 1, row = e & 1;
        AT[c][2 * k + row] = js[q] == 0 ? jv[q] : 0.0;
      }
    }
    if (vr) rT[lane] = rs == 0 ? rv : 0.0;
    if (nxt || !ZERO) {
      const double m0 = nxt ? n0 : 0.0, m3 = nxt ? n3 : 0.0, m1 = nxt ? n1 : 0.0, m2 = nxt ? n2 : 0.0;
      if (lane < 36) {  // dynamics: 6 x 6 / 6 x 3 / 6 x 3, column-major
        const int c = lane / 6, row = lane - c * 6;
        AT[c][rn + row] = m0;
        ANT[c][row] = m0;
        BT[c][row] = m3;
        if (lane < 18) {
          AT[6 + c][rn + row] = m1;
          ANT[6 + c][row] = m1;
          AT[9 + c][rn + row] = m2;
          ANT[9 + c][row] = m2;
        }
      } else if (lane < 45) {  // const velocity: 3 x 3 on the velocity block
        const int e = lane - 36, c = e / 3, row = e - c * 3;
        AT[9 + c][rn + 6 + row] = m0;
        ANT[9 + c][6 + row] = m0;
        BT[9 + c][6 + row] = m3;
      } else if (lane < 51) {
        rT[rn + lane - 45] = m0;
      } else if (lane < 54) {
        rT[rn + 6 + lane - 51] = m0;
      }
    }
    if (prv || !ZERO) {
      const double q3 = prv ? p3 : 0.0;
      if (lane < 36) {
        const int c = lane / 6, row = lane - c * 6;
        AT[c][rp + row] = q3;
      } else if (lane < 45) {
        const int e = lane - 36, c = e / 3, row = e - c * 3;
        AT[9 + c][rp + 6 + row] = q3;
      } else if (lane < 51) {
        rT[rp + lane - 45] = q3;
      } else if (lane < 54) {
        rT[rp + 6 + lane - 51] = q3;
      }
    }
    wave_order();
    // [D_l | g_l] = A^T [A | r] and E_l = A_next^T B on the f64 matrix cores
    // (v_mfma_f64_16x16x4_f64, MI355X_MICROARCH.md / cdna_hip_programming.md fragment maps:
    // A operand lane l = (i = l & 15, k = l >> 4), B operand (k = l >> 4, j = l & 15),
    // C/D lane l, register v = (row (l >> 4) + 4 v, col l & 15)).  Rows of the staged
    // transposes are the k dimension, 4 per instruction; variables 12..15 are zero padding
    // except B's column 12, which carries r so that C[:, 12] = A^T r = g.
#pragma unroll
    for (int q = 0; q < RPP / 4; ++q) {
      const int row = 4 * q + lk;
      const double at = li < NV ? AT[li][row] : 0.0;
      const double bv = li < NV ? at : (li == NV ? rT[row] : 0.0);
      cD = __builtin_amdgcn_mfma_f64_16x16x4f64(at, bv, cD, 0, 0, 0);
    }
    if (nxt) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int row = 4 * q + lk;
        const double an = li < NV ? ANT[li][row] : 0.0;
        const double bt = li < NV ? BT[li][row] : 0.0;
        cE = __builtin_amdgcn_mfma_f64_16x16x4f64(an, bt, cE, 0, 0, 0);
      }
    }
  }
  // the constant-velocity factor on the angular velocity, pairs (l-1, l) and (l, l+1): its rows
  // are -s_i on x_l's variable 6 + i and +s_i on x_{l+1}'s (s = isig_cw), so with r the whitened
  // residuals  D_l[6+i][6+i] += s_i^2 per pair,  E_l[6+i][6+i] -= s_i^2,
  // g_l[6+i] += s_i (r_{l-1,i} - r_{l,i})  -- no staged rows.  Rows 6, 7, 8 of the C layout are
  // (lk, v) = (2, 1), (3, 1), (0, 2); one lane each holds the diagonal entry (li == row) and the
  // g entry (li == NV).  (The branch is uniform; with the factor off nothing here changes cD / cE.)
  if (a.r_cw != nullptr && npair > 0) {
    const int i = lk >= 2 ? lk - 2 : 2, row = 6 + i;
    const bool hd = lk != 1 && li == row, hg = lk != 1 && li == NV;
    if (hd || hg) {
      const double s = a.isig_cw[i];
      const long un = (long)t * npair + (nxt ? l : 0), up = (long)t * npair + (prv ? l - 1 : 0);
      const double rn = nxt ? a.r_cw[un * 3 + i] : 0.0, rq = prv ? a.r_cw[up * 3 + i] : 0.0;
      const double s2 = s * s;
      const double addD = hd ? (nxt ? s2 : 0.0) + (prv ? s2 : 0.0) : s * (rq - rn);
      if (lk >= 2)
        cD[1] += addD;
      else
        cD[2] += addD;
      if (hd && nxt) {
        if (lk >= 2)
          cE[1] -= s2;
        else
          cE[2] -= s2;
      }
    }
  }
  // the marginalization prior on the oldest frame: D_0 += Lambda, g_0 += Lambda xi - eta (the
  // branch is uniform; without a prior nothing here changes cD)
  if (l == 0 && a.p_info != nullptr) {
    const double* pi = a.p_info + (size_t)t * NB;
    const double* pg = a.p_grad + (size_t)t * NV;
#pragma unroll
    for (int v = 0; v < 3; ++v) {  // rows lk + 4v < 12
      const int i = lk + 4 * v;
      if (li < NV)
        cD[v] += pi[i * NV + li];
      else if (li == NV)
        cD[v] += pg[i];
    }
  }
  // D / E / g go to the API outputs only when the caller asked for them (a.D null: the
  // blocks stay in the solver's LDS ring; the streaming tick and GNPlan use delta only)
  const bool out = a.D != nullptr;  // uniform
  double* Dl = out ? a.D + f * NB : nullptr;
  double* El = (out && nxt) ? a.E + ((long)t * npair + l) * NB : nullptr;
  double* gl = out ? a.g + f * NV : nullptr;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int i = lk + 4 * v;
    if (i >= NV) continue;
    if (li < NV) {
      if (out) Dl[i * NV + li] = cD[v];
      blk[i * NV + li] = cD[v];
      if (nxt) {
        if (out) El[i * NV + li] = cE[v];
        blk[NB + i * NV + li] = cE[v];
      }
    } else if (li == NV) {
      if (out) gl[i] = cD[v];
      blk[2 * NB + i] = cD[v];
    }
  }
}

// ---------------------------------------------------------------- chain pieces
// 1 / x for x > 0: the hardware estimate + two Newton steps (f64 accurate)
__device__ __forceinline__ double gn_rcp(double x) {
  double y = __builtin_amdgcn_rcp(x);
  y = y * (2.0 - x * y);
  y = y * (2.0 - x * y);
  return y;
}

typedef double gn_d2 __attribute__((ext_vector_type(2)));
#ifndef GN_CU
#define GN_CU 3  // k-pair unroll of gn_couple's loops (6 = fully unrolled)
#endif

// One eliminated frame's state in LDS (a solver wave's own): M = S^-1 (row-major), G =
// M E' (the S update reads it across lanes), z, this frame's b, the sweep's pivot rows.
struct GnChainLds {
  double M[gn::NB];
  double G[gn::NV * 13];  // gn_couple: G (row-major 12 x 12); gn_couple_mfma: E'^T [G | zprev] (12 x 13)
  double z[gn::NV];
  double bs[gn::NV];
  double rk2[2 * gn::NV];
};

// gn_couple on the f64 matrix cores (v_mfma_f64_16x16x4f64, operand maps as in
// gn_build_frame): G = Mprev E' as 3 k-steps with A = Mprev (lane: row l & 15, k = l >> 4) and
// B = E' (k = l >> 4, column l & 15); G lands in the C layout (register v: row (l >> 4) + 4v,
// column l & 15), which for k-step q is exactly the B operand E'^T G needs (row 4q + (l >> 4)),
// and E'^T's A operand is E' read as B was -- so the second product needs no exchange.
// Column 12 of that B carries zprev, so T = E'^T [G | zprev] gives the b update too. T goes
// through LDS (xch, 12 x 13) once to reach the row layout (lane: row r, columns c0 .. c0 + 3).
// Gout (LDS, row-major) and gws (workspace) receive G when given.
template <bool MIR>
__device__ __forceinline__ void gn_couple_mfma(const double* Mprev, const double* zprev, const double* eb,
                                               double* Gout, double* gws, double* xch, int r, int c0,
                                               double (&sv)[4], double& b) {
  using namespace gn;
  typedef double d4_t __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const bool in = li < NV;
  const int lr = in ? li : 0;  // a valid row / column for the lanes of the padding
  double e[3];
  d4_t cG = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int k = 4 * q + lk;
    const double m = in ? Mprev[lr * NV + k] : 0.0;
    e[q] = in ? (MIR ? eb[lr * NV + k] : eb[k * NV + lr]) : 0.0;  // E'(k, li)
    cG = __builtin_amdgcn_mfma_f64_16x16x4f64(m, e[q], cG, 0, 0, 0);
  }
  d4_t cT = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double bz = li == NV ? zprev[4 * q + lk] : 0.0;
    cT = __builtin_amdgcn_mfma_f64_16x16x4f64(e[q], in ? cG[q] : bz, cT, 0, 0, 0);
  }
  wave_order();  // every lane is past its reads of xch / Gout's previous contents
#pragma unroll
  for (int v = 0; v < 3; ++v) {  // rows lk + 4v < 12
    const int i = lk + 4 * v;
    if (li <= NV) xch[i * 13 + li] = cT[v];
    if (in) {
      if (Gout) Gout[i * NV + li] = cG[v];
      if (gws) gws[i * NV + li] = cG[v];
    }
  }
  wave_order();
#pragma unroll
  for (int c = 0; c < 4; ++c) sv[c] -= xch[r * 13 + c0 + c];  // (8-byte aligned rows)
  b -= xch[r * 13 + NV];
}

// (sv, b) -= the coupling to the previously eliminated frame (lane: row r, columns c0 .. c0 + 3):
//   G = Mprev E',   sv -= E'^T G,   b -= E'^T zprev,
// with E'(k, c) = eb[k * NV + c] (MIR = false: E_{l-1}, from the previous frame's slot) or
// eb[c * NV + k] (MIR = true: the current frame's own E_l, transposed -- the bottom-up chain).
// G goes to Gout (LDS) and, when gws is given, to the workspace (row-major, back substitution).
template <bool MIR, int CU = GN_CU>
__device__ __forceinline__ void gn_couple(const double* Mprev, const double* zprev, const double* eb, double* Gout,
                                          double* gws, int r, int c0, bool act, double (&sv)[4], double& b) {
  using namespace gn;
  double pv[4] = {0.0, 0.0, 0.0, 0.0}, ph[4] = {0.0, 0.0, 0.0, 0.0};  // even / odd k
  // k in pairs, the pair loop unrolled by NU only: fully unrolled, the compiler hoists all
  // 60 LDS reads and the 4-wave workgroup's 128-VGPR budget spills
#pragma unroll CU
  for (int k2 = 0; k2 < NV; k2 += 2) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = k2 + h;
      const double m = Mprev[r * NV + k];
      double e[4];
      if constexpr (MIR) {
#pragma unroll
        for (int c = 0; c < 4; ++c) e[c] = eb[(c0 + c) * NV + k];
      } else {
        const gn_d2 e0 = *reinterpret_cast<const gn_d2*>(eb + k * NV + c0);
        const gn_d2 e1 = *reinterpret_cast<const gn_d2*>(eb + k * NV + c0 + 2);
        e[0] = e0[0];
        e[1] = e0[1];
        e[2] = e1[0];
        e[3] = e1[1];
      }
      double* acc = h ? ph : pv;
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] += m * e[c];
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) pv[c] += ph[c];
  wave_order();  // every lane is past its reads of Gout's previous contents
  if (act) {
    *reinterpret_cast<gn_d2*>(Gout + r * NV + c0) = gn_d2{pv[0], pv[1]};
    *reinterpret_cast<gn_d2*>(Gout + r * NV + c0 + 2) = gn_d2{pv[2], pv[3]};
    if (gws)
#pragma unroll
      for (int c = 0; c < 4; ++c) gws[r * NV + c0 + c] = pv[c];
  }
  wave_order();
  double s2[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}}, b2[2] = {0.0, 0.0};
#pragma unroll CU
  for (int k2 = 0; k2 < NV; k2 += 2) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = k2 + h;
      const double ek = MIR ? eb[r * NV + k] : eb[k * NV + r];
      const gn_d2 p0 = *reinterpret_cast<const gn_d2*>(Gout + k * NV + c0);
      const gn_d2 p1 = *reinterpret_cast<const gn_d2*>(Gout + k * NV + c0 + 2);
      s2[h][0] += ek * p0[0];
      s2[h][1] += ek * p0[1];
      s2[h][2] += ek * p1[0];
      s2[h][3] += ek * p1[1];
      b2[h] += ek * zprev[k];
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) sv[c] -= s2[0][c] + s2[1][c];
  b -= b2[0] + b2[1];
}

// M = S^-1 by the symmetric sweep operator with 2 x 2 pivot blocks K = {k, k + 1}, k = 0, 2, .., 10
// (ends with -S^-1):  S_KK <- -P^-1,  S_iK <- S_iK P^-1,  S_Kj <- P^-1 S_Kj,
// S_ij <- S_ij - S_iK P^-1 S_Kj  (P = S_KK).  P is positive definite iff a > 0 and
// det > 0 -- the two scalar pivots a, d - b^2 / a of the Cholesky / LDL^T test.  Returns
// false on a pivot block that is not positive definite; otherwise sv is row r of -M.
__device__ __forceinline__ bool gn_sweep(double (&sv)[4], double* rk2, int r, int c0, bool act) {
  using namespace gn;
  bool bad = false;
#pragma unroll 1
  for (int k = 0; k < NV; k += 2) {
    if (act && (r >> 1) == (k >> 1)) {  // rows k, k + 1 -> the pivot-row buffer
      double* dst = rk2 + (r - k) * NV + c0;
      *reinterpret_cast<gn_d2*>(dst) = gn_d2{sv[0], sv[1]};
      *reinterpret_cast<gn_d2*>(dst + 2) = gn_d2{sv[2], sv[3]};
    }
    wave_order();
    const gn_d2 pa = *reinterpret_cast<const gn_d2*>(rk2 + k);  // S[k][k], S[k][k+1]
    const double pd = rk2[NV + k + 1];                          // S[k+1][k+1]
    const double u0 = rk2[r], u1 = rk2[NV + r];                 // S[r][k], S[r][k+1] (symmetric)
    const gn_d2 x0 = *reinterpret_cast<const gn_d2*>(rk2 + c0);
    const gn_d2 x1 = *reinterpret_cast<const gn_d2*>(rk2 + c0 + 2);
    const gn_d2 y0 = *reinterpret_cast<const gn_d2*>(rk2 + NV + c0);
    const gn_d2 y1 = *reinterpret_cast<const gn_d2*>(rk2 + NV + c0 + 2);
    const double vk[4] = {x0[0], x0[1], x1[0], x1[1]};   // S[k][c0 ..]
    const double vk1[4] = {y0[0], y0[1], y1[0], y1[1]};  // S[k+1][c0 ..]
    double a0 = pa[0], b0 = pa[1], d0 = pd;
    double det = a0 * d0 - b0 * b0;
    if (!(a0 > 0.0) || !(det > 0.0)) {
      bad = true;
      a0 = 1.0;
      b0 = 0.0;
      d0 = 1.0;
      det = 1.0;
    }
    const double id = gn_rcp(det);
    const double q00 = d0 * id, q01 = -b0 * id, q11 = a0 * id;  // P^-1 (symmetric)
    // one formula for every element (branch-free): with (al0, al1) = row r - k of P^-1
    // for the pivot rows and -(S_rK P^-1) otherwise,
    //   j not in K:  S'[r][j] = (r in K ? 0 : S[r][j]) + al0 S[k][j] + al1 S[k+1][j]
    //   j in K:      S'[r][j] = -(j == k ? al0 : al1)
    const bool rk = (r >> 1) == (k >> 1);
    const double al0 = rk ? (r == k ? q00 : q01) : -(u0 * q00 + u1 * q01);
    const double al1 = rk ? (r == k ? q01 : q11) : -(u0 * q01 + u1 * q11);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = c0 + c;
      const double gen = fma(al0, vk[c], fma(al1, vk1[c], rk ? 0.0 : sv[c]));
      sv[c] = (j >> 1) == (k >> 1) ? -(j == k ? al0 : al1) : gen;
    }
  }
  return !bad;
}

// after a successful sweep: M (= -sv) and b to LDS, z = M b (returned on every lane for its row r)
__device__ __forceinline__ double gn_finish(const double (&sv)[4], double b, GnChainLds& C, int r, int c0, bool act) {
  using namespace gn;
  wave_order();
  if (act) {
    *reinterpret_cast<gn_d2*>(C.M + r * NV + c0) = gn_d2{-sv[0], -sv[1]};
    *reinterpret_cast<gn_d2*>(C.M + r * NV + c0 + 2) = gn_d2{-sv[2], -sv[3]};
    if (c0 == 0) C.bs[r] = b;
  }
  wave_order();
  double z0 = 0.0, z1 = 0.0;
#pragma unroll
  for (int j = 0; j < NV; j += 2) {
    z0 += C.M[r * NV + j] * C.bs[j];
    z1 += C.M[r * NV + j + 1] * C.bs[j + 1];
  }
  wave_order();
  if (act && c0 == 0) C.z[r] = z0 + z1;
  return z0 + z1;
}

}  // namespace pa
