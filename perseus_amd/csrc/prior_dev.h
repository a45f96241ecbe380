// Device code of the marginalization prior's evaluation (prior_lin_wave), shared by
// pa_window_prior_linearize (prior.hip) and the Levenberg-Marquardt solve with a prior (lm.hip),
// so that both evaluate xi, grad and err with the same instructions in the same order.
#pragma once
#include "gn_dev.h"

namespace pa {

// One wave, lane i: the prior (info (12 x 12), eta, xbar = xp / xw / xv, all of ONE trajectory) at
// the frame state pose (12) / angvel (3) / vel (3):
//   xi = [Logmap(xbar_pose^-1 pose); angvel - wbar; vel - vbar],  grad (12) = Lambda xi - eta,
//   returns err = sum_i xi_i (0.5 (Lambda xi)_i - eta_i), summed in index order (the same value on
//   every lane).
// xi, es: NV doubles of LDS each, this wave's alone.
__device__ __forceinline__ double prior_lin_wave(int i, const double* __restrict__ info,
                                                 const double* __restrict__ eta, const double* __restrict__ xp,
                                                 const double* __restrict__ xw, const double* __restrict__ xv,
                                                 const double* pose, const double* angvel, const double* vel,
                                                 double* grad, double* xi, double* es) {
  using namespace gn;
  // every lane evaluates the same xi (uniform addresses: one Logmap's worth of instructions)
  const Pose d = compose(inverse(load_pose(xp)), load_pose(pose));
  V3 w, u;
  pose_log(d, w, u);
  const V3 dw = load3(angvel) - load3(xw);
  const V3 dv = load3(vel) - load3(xv);
  if (i == 0) {
    xi[0] = w.x, xi[1] = w.y, xi[2] = w.z;
    xi[3] = u.x, xi[4] = u.y, xi[5] = u.z;
    xi[6] = dw.x, xi[7] = dw.y, xi[8] = dw.z;
    xi[9] = dv.x, xi[10] = dv.y, xi[11] = dv.z;
  }
  wave_order();
  if (i < NV) {
    const double* row = info + i * NV;
    double lx = 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k) lx = fma(row[k], xi[k], lx);
    const double e = eta[i];
    grad[i] = lx - e;
    es[i] = xi[i] * (0.5 * lx - e);
  }
  wave_order();
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < NV; ++k) s += es[k];
  return s;
}

}  // namespace pa
