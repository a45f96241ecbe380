// The factor outputs of pa_trajectory_linearize (the output pointers of pa_traj_args,
// include/perseus_amd.h), listed once: X(field, element type, elements per unit, unit), the unit
// a projection (T*L*K of them) or a frame pair (T*(L-1)).  Everything that treats them as a set
// -- the struct of the pointers, the T = 1 view of one trajectory, the LM workspace's copy of
// the set with its select between the two, its null checks and its final copy (lm.hip) --
// expands this list, so a new output is added here (and to the public header and
// _lib.py).  Every expansion is unrolled by the preprocessor: no table is indexed at run time.
#pragma once
#include <cmath>

#include "common.h"

#define PA_FACTOR_OUTPUTS(X)       \
  X(r_proj, double, 2, FU_PROJ)    \
  X(j_proj, double, 12, FU_PROJ)   \
  X(err_proj, double, 1, FU_PROJ)  \
  X(status, int32_t, 1, FU_PROJ)   \
  X(r_dyn, double, 6, FU_PAIR)     \
  X(j_dyn0, double, 36, FU_PAIR)   \
  X(j_dyn1, double, 18, FU_PAIR)   \
  X(j_dyn2, double, 18, FU_PAIR)   \
  X(j_dyn3, double, 36, FU_PAIR)   \
  X(err_dyn, double, 1, FU_PAIR)   \
  X(r_cv, double, 3, FU_PAIR)      \
  X(j_cv0, double, 9, FU_PAIR)     \
  X(j_cv1, double, 9, FU_PAIR)     \
  X(err_cv, double, 1, FU_PAIR)
// The optional outputs: those of the constant-velocity factor on the angular velocity ("cw",
// pa_traj_args.r_cw; null = the factor is off).  Every expansion that only carries pointers takes
// both lists (PA_FACTOR_OUTPUTS_ALL); the LM solve's null checks take the required list alone, and
// it keeps this pair beside its two sets (LmDev, lm.hip) and copies it under the switch.
#define PA_FACTOR_OUTPUTS_CW(X) \
  X(r_cw, double, 3, FU_PAIR)   \
  X(err_cw, double, 1, FU_PAIR)
#define PA_FACTOR_OUTPUTS_ALL(X) PA_FACTOR_OUTPUTS(X) PA_FACTOR_OUTPUTS_CW(X)

namespace pa {

// The robust noise model's arguments (include/perseus_amd.h, pa_proj_linearize_robust), checked
// the same way by every entry point that takes them: `kind` / `k` name the caller's fields
// (robust_proj / robust_proj_k of a pa_traj_args).  k is not looked at for PA_ROBUST_NONE.
inline int robust_check(int kind, double k, const char* who, const char* kind_name, const char* k_name) {
  PA_CHECK(kind == PA_ROBUST_NONE || kind == PA_ROBUST_HUBER || kind == PA_ROBUST_CAUCHY,
           "%s: %s %d is not PA_ROBUST_NONE (0), PA_ROBUST_HUBER (1) or PA_ROBUST_CAUCHY (2)", who, kind_name, kind);
  PA_CHECK(kind == PA_ROBUST_NONE || (k > 0.0 && k < INFINITY), "%s: %s %g must be a positive finite number (%s %d)",
           who, k_name, k, kind_name, kind);
  return PA_OK;
}
inline int robust_check(const pa_traj_args& ta, const char* who) {
  return robust_check(ta.robust_proj, ta.robust_proj_k, who, "robust_proj", "robust_proj_k");
}

enum FactorUnit { FU_PROJ, FU_PAIR };
// units of kind u among np projections and nd frame pairs (u is a constant at every use)
template <typename N>
__host__ __device__ constexpr N factor_units(FactorUnit u, N np, N nd) {
  return u == FU_PROJ ? np : nd;
}

// the required outputs alone (lm.hip keeps its two sets in this form, the layout they had before
// the optional pair existed, and the pair beside them)
struct FactorSetReq {
#define PA_X(f, V, n, u) V* f;
  PA_FACTOR_OUTPUTS(PA_X)
#undef PA_X
};
struct FactorSet : FactorSetReq {
#define PA_X(f, V, n, u) V* f;
  PA_FACTOR_OUTPUTS_CW(PA_X)
#undef PA_X
};

// the set a pa_traj_args names
__host__ __device__ __forceinline__ FactorSet factor_set(const pa_traj_args& ta) {
  FactorSet s;
#define PA_X(f, V, n, u) s.f = ta.f;
  PA_FACTOR_OUTPUTS_ALL(PA_X)
#undef PA_X
  return s;
}

// trajectory t's factors: the arrays of a T = 1 problem start at its records.  The state
// (y, pose, vel, angvel) is ta's, the factor outputs are s's (factor_set(ta): ta's own); a
// null nvalid / dt_pair / kp_mask / dt_new / mask_new stays null, and so does a null output (err_*, the projection arrays at K = 0)
// unless the caller knows that s has none (NULLS = false: no tests; lm_lin_kernel, which is
// at the edge of its register budget).
template <bool NULLS = true>
__device__ __forceinline__ pa_traj_args traj_view(const pa_traj_args& ta, int t, const FactorSet s) {
  const int L = ta.L, K = ta.n_kp;
  const long f0 = (long)t * L, p0 = f0 * K, d0 = (long)t * (L - 1);
  auto off = [](auto* q, long n) { return q ? q + n : q; };
  pa_traj_args a1 = ta;
  a1.T = 1;
  a1.y = ta.y + f0 * 2 * K;
  a1.pose = ta.pose + f0 * 12;
  a1.vel = ta.vel + f0 * 3;
  a1.angvel = ta.angvel + f0 * 3;
#define PA_X(f, V, n, u) a1.f = NULLS ? off(s.f, factor_units(u, p0, d0) * n) : s.f + factor_units(u, p0, d0) * n;
  PA_FACTOR_OUTPUTS(PA_X)
#undef PA_X
  // the optional pair keeps its nulls whatever NULLS says: r_cw null is the factor's switch
  // (read only by the CW instantiations, factors_dev.h)
#define PA_X(f, V, n, u) a1.f = off(s.f, factor_units(u, p0, d0) * n);
  PA_FACTOR_OUTPUTS_CW(PA_X)
#undef PA_X
  a1.nvalid = off(ta.nvalid, (long)t);
  // the real timestamps (read only by the TM instantiations, factors_dev.h)
  a1.dt_pair = off(ta.dt_pair, d0);
  a1.kp_mask = off(ta.kp_mask, f0);
  a1.dt_new = off(ta.dt_new, (long)t);
  a1.mask_new = off(ta.mask_new, (long)t);
  return a1;
}

}  // namespace pa
