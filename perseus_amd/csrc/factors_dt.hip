// pa_dyn_linearize_dt: the batched PoseDynamicsFactor (factors.hip dyn_kernel) with one dt per
// factor.  Its own translation unit: dyn_one has one caller in each, so each kernel inlines it
// (as a second caller beside dyn_kernel it became a call, and dyn_kernel went from no private
// segment to 380 B per lane).
#include "factors_dev.h"

namespace pa {

__global__ __launch_bounds__(64) void dyn_dt_kernel(int n, const double* __restrict__ T1p, const double* __restrict__ wp,
                                                    const double* __restrict__ vp, const double* __restrict__ T2p,
                                                    const double* __restrict__ dtp, int vel_frame,
                                                    const double* __restrict__ isig, double* __restrict__ r_out,
                                                    double* __restrict__ J0, double* __restrict__ J1,
                                                    double* __restrict__ J2, double* __restrict__ J3,
                                                    double* __restrict__ err) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const size_t u = i;
  dyn_one(T1p + u * 12, wp + u * 3, vp + u * 3, T2p + u * 12, dtp[u], vel_frame, isig, r_out + u * 6,
          J0 ? J0 + u * 36 : nullptr, J1 ? J1 + u * 18 : nullptr, J2 ? J2 + u * 18 : nullptr,
          J3 ? J3 + u * 36 : nullptr, err ? err + u : nullptr);
}

}  // namespace pa

extern "C" {

int pa_dyn_linearize_dt(int n, const double* t1, const double* w, const double* v, const double* t2, const double* dt,
                        int vel_frame, const double* inv_sigma, double* r, double* j0, double* j1, double* j2,
                        double* j3, double* err, void* stream) {
  PA_CHECK(n >= 0, "n %d", n);
  if (n == 0) return PA_OK;
  PA_CHECK(t1 && w && v && t2 && dt && r, "null pointer");
  PA_CHECK(vel_frame == PA_VEL_WORLD || vel_frame == PA_VEL_BODY, "vel_frame must be 'world' or 'body'.");
  hipLaunchKernelGGL(pa::dyn_dt_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, n, t1, w, v, t2, dt,
                     vel_frame, inv_sigma, r, j0, j1, j2, j3, err);
  PA_LAUNCH_CHECK();
  return PA_OK;
}

}  // extern "C"
