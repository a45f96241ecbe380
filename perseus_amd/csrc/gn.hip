// Factor-graph consumer: one damped Gauss-Newton / LM step over each
// trajectory, from the whitened factors of pa_trajectory_linearize, on the device.
// The graph and optimizer are not in the reference (GTSAM's LM runs on the host), so
// this build defines them: per frame l the variable block is
//   x_l = [ pose tangent (6, GTSAM order [omega; v]) | angular velocity (3) | velocity (3) ]
// and the step solves (J^T J + lambda I) delta = -J^T r.  The normal matrix of one
// trajectory is block tridiagonal in 12 x 12 blocks:
//   D_l (diagonal): the K projection factors of frame l (pose), the dynamics factors
//                   (l-1, l) and (l, l+1), the constant-velocity factors around l;
//   E_l (x_l rows, x_{l+1} cols): the dynamics and constant-velocity factors (l, l+1).
// One launch, one workgroup per trajectory.  Assembler waves build D_l, E_l, g_l = J^T r
// from the factors touching frame l (each block has one writer, no atomics) into LDS rings
// while solver waves eliminate frame by frame.  Shipped (gn_twisted_kernel, SOLVER 2): four
// waves -- a top-down and a bottom-up chain, each one assembler + one solver wave, meeting
// at frame L / 2 (block Thomas with the Schur complements inverted by the symmetric sweep
// operator, run from both ends).  Kept as variants (gn_step_kernel): SOLVER 1, the same
// elimination as one top-down chain fed by NA assembler waves; SOLVER 0, the round-2 block
// Cholesky (L_l L_l^T = D_l + lambda I - W_l^T W_l, W_l = L_{l-1}^{-1} E_{l-1}) with
// forward and back substitution.  Launches of at most as many trajectories as CUs (the
// streaming tick's T = 3) with L <= 24 run gn_cr_kernel instead: block cyclic reduction,
// 5 serial pivots at L = 24 instead of 13.  D / E / g are optional outputs.
// pa_trajectory_lm_solve (lm.hip, "Levenberg-Marquardt") iterates that step per trajectory with
// accept / reject and adaptive damping, on the device.
// f64 throughout.
// Jacobians are column-major per factor (include/perseus_amd.h).
// This file: the step's kernels and entry points.  The assembly, the chain pieces and the
// cyclic reduction are gn_dev.h / gn_cr_dev.h, shared with pose_tick.hip and lm.hip.
#include "gn_cr_dev.h"

namespace pa {

// ---------------------------------------------------------------- solve
// The solver wave of a trajectory: block Cholesky of the block-tridiagonal normal matrix, frame
// by frame,
//   W_l = L_{l-1}^{-1} E_{l-1}                 lane c < 12: column c, forward substitution
//                                              with L_{l-1} read from LDS (uniform addresses)
//   S_l = D_l + lambda I - W_l^T W_l           lane i: row i (its own W column, all of W
//   rhs_l = -g_l - W_l^T y_{l-1}                from LDS)
//   L_l L_l^T = S_l                            right-looking, column j final at step j; the
//                                              raw column j reaches every lane by v_readlane
//   y_l = L_l^{-1} rhs_l
// then back substitution L_l^T delta_l = y_l - W_{l+1} delta_{l+1}.  L_l, W_l, y_l go to the
// workspace for the backward pass.  Frame l's D / E / g come from the LDS ring, built by
// the assembler wave during frame l - 1 (one LDS-only barrier per frame hands a slot
// over; the solver's own LDS exchanges are wave-local).  Round 2a ran assembly (one
// wave per frame) and solve (one wave per trajectory) as two launches: 54 + 175 us per
// 1000 x 24.  (Round 1 ran one thread per trajectory with the blocks in
// LDS, 16-thread workgroups: 2.2 ms per 1000 x 24.)
// 1 / sqrt(x) for x > 0: the hardware estimate + two Newton steps (f64 accurate; the IEEE
// sqrt + divide sequences were a third of the solve's instructions)
__device__ __forceinline__ double gn_rsqrt(double x) {
  double y = __builtin_amdgcn_rsq(x);
  const double hx = 0.5 * x;
  y = y * (1.5 - hx * y * y);
  y = y * (1.5 - hx * y * y);
  return y;
}

__device__ __forceinline__ double gn_bcast(double v, int src) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, src);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ int lds_load_acquire(const int* p) {
  const int v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
  return v;
}
__device__ __forceinline__ void lds_store_release(int* p, int v) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");  // LDS only: global stores stay in flight
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Back substitution along n frames f = f0, f0 + step, ..:  delta_f = z_f - G_f delta_prev
// (lane i < 12: row i).  G_f rows and z_f come from the workspace slot of f, loaded one frame
// ahead (two register sets), except the first frame's G (G0, LDS) when given; delta_prev
// starts as d0 (LDS) or, without one, the first frame has no coupling term.
// dl: 12 doubles of LDS scratch (this wave's).
__device__ __forceinline__ void gn_backsub(const double* ws, int f0, int step, int n, const double* G0,
                                           const double* d0, double* dl, double* delta, int i) {
  using namespace gn;
  if (n <= 0) return;
  const int ir = i < NV ? i : NV - 1;
  double Gn[NV], zn;
  auto ld = [&](int u) __attribute__((always_inline)) {
    const double* wn = ws + (size_t)(f0 + u * step) * GN_WSF;
    const double* gr = (u == 0 && G0) ? G0 + ir * NV : wn + ir * NV;
#pragma unroll
    for (int k = 0; k < NV; ++k) Gn[k] = gr[k];
    zn = wn[NB + ir];
  };
  if (d0 && i < NV) dl[i] = d0[i];
  wave_order();
  ld(0);
  for (int u = 0; u < n; ++u) {
    double Gc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) Gc[k] = Gn[k];
    double d = zn;
    if (u + 1 < n) ld(u + 1);
    if (u > 0 || d0) {
      double e0 = 0.0, e1 = 0.0;
#pragma unroll
      for (int k = 0; k < NV; k += 2) {
        e0 += Gc[k] * dl[k];
        e1 += Gc[k + 1] * dl[k + 1];
      }
      d -= e0 + e1;
    }
    wave_order();
    if (i < NV) {
      dl[i] = d;
      delta[(size_t)(f0 + u * step) * NV + i] = d;
    }
    wave_order();
  }
}

// NA assembler waves (wave a builds frames a, a + NA, ...) and one solver wave per
// trajectory, handing frames over through an LDS ring of NA + 2 slots with two LDS
// counters: ready[slot] = frame + 1 once the slot holds that frame, `consumed` = frames
// the solver has finished (frame m may overwrite slot m % R once the solver is past frame
// m - R + 1, whose E block it reads last).  Every wait is satisfied by waves of the same
// workgroup that are already running, and the solver publishes `consumed` even for frames
// it skips after a failed pivot, so every wave runs to its end.
//
// SOLVER = 1 (round 3): block Thomas with explicit inverses, so the per-frame chain has ONE
// 12-step sequence instead of three (W solve, Cholesky, y solve):
//   G_{l-1} = M_{l-1} E_{l-1}                   (M = S^-1; 12 x 12 x 12, no chain)
//   S_l = D_l + lambda I - E_{l-1}^T G_{l-1}    (no chain)
//   b_l = -g_l - E_{l-1}^T z_{l-1}
//   M_l = S_l^-1 by the symmetric sweep operator (12 pivots; the pivots are S_l's LDL^T
//          pivots, so a pivot <= 0 <=> S_l not positive definite, as the Cholesky test)
//   z_l = M_l b_l;  backward  delta_l = z_l - G_l delta_{l+1}  (one mat-vec per frame).
// 36 lanes hold a 12 x 12 block, lane i: row i / 3, columns 4 (i % 3) .. + 3; the sweep
// hands row k round through LDS (one wave: LDS ops run in order) and uses symmetry for
// column k.
template <int RP, int NA, int SOLVER>
__global__ __launch_bounds__(64 * (NA + 1), 3) void gn_step_kernel(GnArgs a) {
  using namespace gn;
  constexpr int BLK = 2 * NB + NV;  // D | E | g of one frame
  constexpr int R = NA + 2;
  __shared__ __attribute__((aligned(16))) GnStage<RP> st[NA];  // assembler staging
  __shared__ __attribute__((aligned(16))) double blk[R][BLK];   // frame ring
  __shared__ __attribute__((aligned(16))) double Lp[NB];        // L_{l-1}, row-major
  __shared__ double Ld[NV];                                     // 1 / L_{l-1}[i][i]
  __shared__ __attribute__((aligned(16))) double Wt[NB];        // W_l^T: row c = column c of W
  __shared__ __attribute__((aligned(16))) double ys[NV];        // y_{l-1}
  __shared__ int ready[R];
  __shared__ int consumed;
  const int t = blockIdx.x;
  const int wv = threadIdx.x >> 6;
  const int i = threadIdx.x & 63;
  const int L = a.L;
  const long f0 = (long)t * L;
  if (threadIdx.x < R) ready[threadIdx.x] = 0;
  if (threadIdx.x == 0) consumed = 0;
  __syncthreads();
  if (wv < NA) {
    for (int l = wv; l < L; l += NA) {
      while (lds_load_acquire(&consumed) < l - R + 2) __builtin_amdgcn_s_sleep(2);
      gn_stamp(a, t, 2 * l);  // assembler: frame l start (slot 2 l) / published (2 l + 1)
      gn_assemble_frame<RP>(a, f0 + l, st[wv], blk[l % R]);
      if (i == 0) lds_store_release(&ready[l % R], l + 1);
      gn_stamp(a, t, 2 * l + 1);
    }
    return;
  }
  double* ws = a.ws + (size_t)t * L * GN_WSF;
  int info = 0;
  if constexpr (SOLVER == 1) {
    // the solver's chain is the launch's critical path: it wins issue arbitration against
    // the assembler waves of its own and of the CU's other workgroups
    __builtin_amdgcn_s_setprio(3);
    __shared__ __attribute__((aligned(16))) GnChainLds C;
    const bool act = i < 36;
    const int ii = act ? i : 35;
    const int r = ii / 3, c0 = 4 * (ii - 3 * (ii / 3));
    for (int l = 0; l < L; ++l) {
      const int cur = l % R, prv = (l + R - 1) % R;
      gn_stamp(a, t, 64 + 4 * l);  // solver: frame l wait start / data ready / sweep start / done
      while (lds_load_acquire(&ready[cur]) != l + 1) __builtin_amdgcn_s_sleep(1);
      gn_stamp(a, t, 65 + 4 * l);
      if (!info) {
        const double* bc = blk[cur];
        double sv[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) sv[c] = bc[r * NV + c0 + c] + (r == c0 + c ? a.lambda : 0.0);
        double b = -bc[2 * NB + r];
        if (l > 0)  // G_{l-1} = M_{l-1} E_{l-1} (to the workspace for the backward pass)
          gn_couple<false>(C.M, C.z, blk[prv] + NB, C.G, ws + (size_t)(l - 1) * GN_WSF, r, c0, act, sv, b);
        gn_stamp(a, t, 66 + 4 * l);
        if (!gn_sweep(sv, C.rk2, r, c0, act)) {
          info = l + 1;  // the solver wave idles through the remaining frames' hand-overs
        } else {
          const double z = gn_finish(sv, b, C, r, c0, act);
          if (act && c0 == 0) ws[(size_t)l * GN_WSF + NB + r] = z;
        }
      }
      if (i == 0) lds_store_release(&consumed, l + 1);
      gn_stamp(a, t, 67 + 4 * l);
    }
    gn_stamp(a, t, 250);
    if (!info) {
      // backward: delta_l = z_l - G_l delta_{l+1}, l = L - 1 .. 0
      gn_backsub(ws, L - 1, -1, L, nullptr, nullptr, C.bs, a.delta + (size_t)t * L * NV, i);
    } else {
      for (int e = i; e < L * NV; e += 64) a.delta[(size_t)t * L * NV + e] = NAN;
    }
    if (a.info && i == 0) a.info[t] = info;
    gn_stamp(a, t, 251);
    return;
  }
  const int ic = i < NV ? i : NV - 1;  // lanes >= 12 shadow row / column 11 (no stores)
  const bool act = i < NV;
  for (int l = 0; l < L; ++l) {
    const int cur = l % R, prv = (l + R - 1) % R;
    while (lds_load_acquire(&ready[cur]) != l + 1) __builtin_amdgcn_s_sleep(1);
    if (!info) {
      double* wl = ws + (size_t)l * GN_WSF;
      const double* bc = blk[cur];
      const double* bp = blk[prv];
      double S[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) S[j] = bc[ic * NV + j] + (j == ic ? a.lambda : 0.0);
      double rhs = -bc[2 * NB + ic];
      if (l > 0) {
        // W column ic: L_{l-1} w = E_{l-1}[:, ic]
        double w[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          double s0 = bp[NB + k * NV + ic], s1 = 0.0;
#pragma unroll
          for (int m = 0; m < k; ++m) {
            if (m & 1)
              s1 -= Lp[k * NV + m] * w[m];
            else
              s0 -= Lp[k * NV + m] * w[m];
          }
          w[k] = (s0 + s1) * Ld[k];
        }
        if (act) {
#pragma unroll
          for (int k = 0; k < NV; ++k) {
            Wt[i * NV + k] = w[k];
            wl[NB + k * NV + i] = w[k];  // W_l row-major in the workspace
          }
        }
        wave_lds_sync();
        // S[ic][j] -= sum_k W[k][ic] W[k][j];  rhs -= sum_k W[k][ic] y_{l-1}[k]
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          double s0 = 0.0, s1 = 0.0;
#pragma unroll
          for (int k = 0; k < NV; k += 2) {
            s0 += w[k] * Wt[j * NV + k];
            s1 += w[k + 1] * Wt[j * NV + k + 1];
          }
          S[j] -= s0 + s1;
        }
        double r0 = 0.0, r1 = 0.0;
#pragma unroll
        for (int k = 0; k < NV; k += 2) {
          r0 += w[k] * ys[k];
          r1 += w[k + 1] * ys[k + 1];
        }
        rhs -= r0 + r1;
      }
      // S = L L^T, right-looking; lane ic's S becomes row ic of L (a non-positive pivot sets
      // `bad`; the loop runs on with a dummy pivot so it stays fully unrolled)
      bool bad = false;
      double invd = 1.0;  // 1 / L[ic][ic]
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        double col[NV];  // raw column j: S[m][j], final for m >= j
#pragma unroll
        for (int m = j; m < NV; ++m) col[m] = gn_bcast(S[j], m);
        double d2 = col[j];
        if (!(d2 > 0.0)) {
          bad = true;
          d2 = 1.0;
        }
        const double inv = gn_rsqrt(d2);
        const double lij = S[j] * inv;  // L[ic][j] for ic > j
        if (ic >= j) S[j] = ic == j ? d2 * inv : lij;
        invd = ic == j ? inv : invd;
#pragma unroll
        for (int m = j + 1; m < NV; ++m)
          if (ic > j) S[m] -= lij * (col[m] * inv);
      }
      if (bad) {
        info = l + 1;  // the solver wave idles through the remaining frames' barriers
      } else {
#pragma unroll
        for (int j = 0; j < NV; ++j)
          if (j > ic) S[j] = 0.0;
        // y = L^{-1} rhs
        double y[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          if (ic == k) rhs *= invd;
          y[k] = gn_bcast(rhs, k);
          if (ic > k) rhs -= S[k] * y[k];
        }
        wave_lds_sync();  // every lane is past its reads of Lp / Ld / Wt / ys
        if (act) {
#pragma unroll
          for (int j = 0; j < NV; ++j) {
            Lp[i * NV + j] = S[j];
            wl[i * NV + j] = S[j];
          }
          Ld[i] = invd;
          ys[i] = y[i];
          wl[2 * NB + i] = y[i];
          wl[2 * NB + NV + i] = invd;
        }
      }
    }
    if (i == 0) lds_store_release(&consumed, l + 1);
  }
  if (!info) {
    double xn[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) xn[j] = 0.0;
    // frame l's column ic of L_l, y_l[ic] and row ic of W_{l+1}, loaded one frame ahead
    double Lc_n[NV], Wr_n[NV], y_n = 0.0, di_n = 0.0;
    auto load_b = [&](int l) {
      const double* wl = ws + (size_t)l * GN_WSF;
#pragma unroll
      for (int k = 0; k < NV; ++k) Lc_n[k] = wl[k * NV + ic];
      y_n = wl[2 * NB + ic];
      di_n = wl[2 * NB + NV + ic];
      if (l + 1 < L) {
        const double* Wn = ws + (size_t)(l + 1) * GN_WSF + NB + ic * NV;
#pragma unroll
        for (int k = 0; k < NV; ++k) Wr_n[k] = Wn[k];
      }
    };
    load_b(L - 1);
    for (int l = L - 1; l >= 0; --l) {
      double Lc[NV], Wr[NV];  // column ic of L_l = row ic of L_l^T; row ic of W_{l+1}
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        Lc[k] = Lc_n[k];
        Wr[k] = Wr_n[k];
      }
      double rhs = y_n;
      const double di = di_n;  // 1 / L_l[ic][ic]
      if (l > 0) load_b(l - 1);
      if (l + 1 < L) {  // rhs -= W_{l+1} delta_{l+1}
        double r0 = 0.0, r1 = 0.0;
#pragma unroll
        for (int k = 0; k < NV; k += 2) {
          r0 += Wr[k] * xn[k];
          r1 += Wr[k + 1] * xn[k + 1];
        }
        rhs -= r0 + r1;
      }
#pragma unroll
      for (int k = NV - 1; k >= 0; --k) {  // L^T x = rhs, right-looking from the last row
        if (ic == k) rhs *= di;
        xn[k] = gn_bcast(rhs, k);
        if (ic < k) rhs -= Lc[k] * xn[k];
      }
      if (act) a.delta[((size_t)t * L + l) * NV + i] = xn[i];
    }
  } else {
    for (int e = i; e < L * NV; e += 64) a.delta[(size_t)t * L * NV + e] = NAN;
  }
  if (a.info && i == 0) a.info[t] = info;
}

// SOLVER 2 (round 3, shipped): SOLVER 1's block Thomas elimination run from BOTH ends of the
// trajectory at once (twisted / "burn at both ends" factorization).  Frames 0 .. m - 1 are
// eliminated top-down by one solver wave and frames L - 1 .. m + 1 bottom-up by another, each
// fed by its own assembler wave and LDS ring (R = 3 slots, the SOLVER 1 protocol); the top
// solver then eliminates frame m against both neighbours,
//   Z_m = D_m + lambda I - E_{m-1}^T M_{m-1} E_{m-1} - E_m N_{m+1} E_m^T,
//   z_m = Z_m^-1 (-g_m - E_{m-1}^T z_{m-1} - E_m w_{m+1}) = delta_m,
// and the two back substitutions run outward from delta_m concurrently:
//   delta_l = z_l - G_l delta_{l+1} (l < m),   delta_l = w_l - H_l delta_{l-1} (l > m),
// H_l = N_l E_{l-1}^T.  The bottom chain is the top chain's algorithm on the mirrored problem
// (frame j = L - 1 - l, coupling block E'_{j-1} = E_l^T, read transposed from frame l's own
// slot: gn_couple<true>); the merge's extra term is one more gn_couple<true> with the bottom
// chain's N_{m+1}, w_{m+1} and frame m's E_m.  m = L / 2: the serial depth is L - m + 1 frame
// eliminations (13 at L = 24) instead of L.  Workspace slot l holds G_l, z_l (l <= m) or H_l,
// w_l (l > m).  Waves: 0 / 1 top / bottom assembler, 2 / 3 top / bottom solver.  info: the
// bottom chain's failed frame if it failed, else the top chain's (1-based; 0 = solved).
// OCC workgroups per CU: 4 (k loops unrolled by pairs, <= 128 VGPRs) for launches of more
// trajectories than 2 per CU, else 2 (fully unrolled, <= 256 VGPRs: a shorter solver chain)
template <int RP, int OCC = 4>
__global__ __launch_bounds__(256, OCC) void gn_twisted_kernel(GnArgs a) {
  constexpr int CU = OCC >= 4 ? GN_CU : 6;
  using namespace gn;
  constexpr int BLK = 2 * NB + NV;
  constexpr int R = 3;
  __shared__ __attribute__((aligned(16))) GnStage<RP> st[2];
  __shared__ __attribute__((aligned(16))) double blk[2][R][BLK];  // [chain][slot]
  __shared__ __attribute__((aligned(16))) GnChainLds ch[2];
  __shared__ __attribute__((aligned(16))) double Hm[NB];  // H_{m+1} = N_{m+1} E_m^T (the merge)
  __shared__ int ready[2][R];
  __shared__ int consumed[2];
  __shared__ int bdone, binfo, mdone;
  const int t = blockIdx.x;
  const int wv = threadIdx.x >> 6;
  const int i = threadIdx.x & 63;
  const int L = a.L;
  const int m = L / 2, nb = L - 1 - m;  // merge frame; bottom-chain frames L - 1 .. m + 1
  const long f0 = (long)t * L;
  if (threadIdx.x < 2 * R) (&ready[0][0])[threadIdx.x] = 0;
  if (threadIdx.x < 2) consumed[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    bdone = 0;
    binfo = 0;
    mdone = 0;
  }
  __syncthreads();
  if (wv < 2) {  // assembler of chain wv: top frames 0 .. m, bottom frames L - 1 .. m + 1
    // the next frame's loads are issued before the current frame is built, so the
    // factors' memory latency is off the chain
    const int n = wv == 0 ? m + 1 : nb;
    gn_zero_stage<RP>(st[wv]);
    // frame j + 1's loads are issued before frame j is built (an unrolled pair of load sets
    // without the copy measured the same, 83.1 vs 84.4 us, and needs more registers)
    GnFrameLoads<RP> ld0;
    if (n > 0) gn_load_frame<RP>(a, f0 + (wv == 0 ? 0 : L - 1), ld0);
    auto step = [&](int j, const GnFrameLoads<RP>& cu, GnFrameLoads<RP>& nx) __attribute__((always_inline)) {
      const int l = wv == 0 ? j : L - 1 - j;
      if (j + 1 < n) gn_load_frame<RP>(a, f0 + (wv == 0 ? l + 1 : l - 1), nx);
      while (lds_load_acquire(&consumed[wv]) < j - R + 2) __builtin_amdgcn_s_sleep(2);
      gn_stamp(a, t, 2 * l);
      gn_build_frame<RP, false>(a, f0 + l, cu, st[wv], blk[wv][j % R]);
      if (i == 0) lds_store_release(&ready[wv][j % R], j + 1);
      gn_stamp(a, t, 2 * l + 1);
    };
    for (int j = 0; j < n; ++j) {
      const GnFrameLoads<RP> cu = ld0;
      step(j, cu, ld0);
    }
    return;
  }
  const int sc = wv - 2;  // solver chain: 0 top, 1 bottom
  if (sc == 1 && nb == 0) return;
  __builtin_amdgcn_s_setprio(3);  // the solvers' chains are the launch's critical path
  double* ws = a.ws + (size_t)t * L * GN_WSF;
  double* delta = a.delta + (size_t)t * L * NV;
  GnChainLds& C = ch[sc];
  const bool act = i < 36;
  const int ii = act ? i : 35;
  const int r = ii / 3, c0 = 4 * (ii - 3 * (ii / 3));
  int info = 0;
  const int n = sc == 0 ? m + 1 : nb;
  for (int j = 0; j < n; ++j) {
    const int l = sc == 0 ? j : L - 1 - j;
    const int cur = j % R, prv = (j + R - 1) % R;
    gn_stamp(a, t, 64 + 4 * l);
    while (lds_load_acquire(&ready[sc][cur]) != j + 1) __builtin_amdgcn_s_sleep(1);
    gn_stamp(a, t, 65 + 4 * l);
    const double* bc = blk[sc][cur];
    const bool merge = sc == 0 && j == m && nb > 0;
    bool bfail = false;
    if (merge) {  // the bottom chain's N_{m+1}, w_{m+1} (or its failure)
      int bd;
      while ((bd = lds_load_acquire(&bdone)) == 0) __builtin_amdgcn_s_sleep(1);
      bfail = bd == 2;
    }
    if (!info && !bfail) {
      double sv[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) sv[c] = bc[r * NV + c0 + c] + (r == c0 + c ? a.lambda : 0.0);
      double b = -bc[2 * NB + r];
      if (j > 0) {
        if (sc == 0)  // G_{l-1} = M_{l-1} E_{l-1} -> workspace slot l - 1
          gn_couple_mfma<false>(C.M, C.z, blk[0][prv] + NB, nullptr, ws + (size_t)(l - 1) * GN_WSF, C.G, r, c0, sv, b);
        else  // H_{l+1} = N_{l+1} E_l^T -> workspace slot l + 1
          gn_couple_mfma<true>(C.M, C.z, bc + NB, nullptr, ws + (size_t)(l + 1) * GN_WSF, C.G, r, c0, sv, b);
      }
      if (merge) gn_couple_mfma<true>(ch[1].M, ch[1].z, bc + NB, Hm, nullptr, C.G, r, c0, sv, b);
      gn_stamp(a, t, 66 + 4 * l);
      if (!gn_sweep(sv, C.rk2, r, c0, act)) {
        info = l + 1;  // idles through the remaining frames' hand-overs
      } else {
        const double z = gn_finish(sv, b, C, r, c0, act);
        if (act && c0 == 0) ws[(size_t)l * GN_WSF + NB + r] = z;
      }
    }
    if (i == 0) lds_store_release(&consumed[sc], j + 1);
    gn_stamp(a, t, 67 + 4 * l);
  }
  if (sc == 1) {
    if (i == 0) {
      binfo = info;
      lds_store_release(&bdone, info ? 2 : 1);
    }
    int md;
    while ((md = lds_load_acquire(&mdone)) == 0) __builtin_amdgcn_s_sleep(1);
    gn_stamp(a, t, 252);
    if (md == 1)  // delta_l = w_l - H_l delta_{l-1}, l = m + 1 .. L - 1, from delta_m = z_m (top's C.z)
      gn_backsub(ws, m + 1, 1, nb, Hm, ch[0].z, C.bs, delta, i);
    else
      for (int e = i; e < nb * NV; e += 64) delta[(size_t)(m + 1) * NV + e] = NAN;
    gn_stamp(a, t, 253);
    return;
  }
  // top solver: final info (the bottom chain's failure first), release the bottom solver
  if (nb > 0) {
    int bd;
    while ((bd = lds_load_acquire(&bdone)) == 0) __builtin_amdgcn_s_sleep(1);
    if (bd == 2) info = lds_load_acquire(&binfo);
  }
  if (i == 0) lds_store_release(&mdone, info ? 2 : 1);
  gn_stamp(a, t, 250);
  if (!info)  // delta_l = z_l - G_l delta_{l+1}, l = m .. 0 (delta_m = z_m)
    gn_backsub(ws, m, -1, m + 1, nullptr, nullptr, C.bs, delta, i);
  else
    for (int e = i; e < (m + 1) * NV; e += 64) delta[e] = NAN;
  if (a.info && i == 0) a.info[t] = info;
  gn_stamp(a, t, 251);
}

template <int RP, int NS>
__global__ __launch_bounds__(64 * GN_CR_W, 1) void gn_cr_kernel(GnArgs a) {
  using Ld = GnCrLds<RP, NS>;
  __shared__ __attribute__((aligned(16))) double fb[Ld::LM][Ld::BLK];
  __shared__ __attribute__((aligned(16))) double pool[Ld::POOL];
  gn_cr_run<RP, NS>(a, blockIdx.x, fb, pool);
}

int g_gn_na = 0;  // (gn_dev.h)
// CUs of the CURRENT device (cached per device id: a host with GPUs of different CU counts
// gets each one's own); only the cyclic-reduction vs two-ended choice in launch_gn uses it
static int g_gn_cus() {
  static int cache[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 256;
  if (dev < 64 && cache[dev] > 0) return cache[dev];
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  if (dev < 64) cache[dev] = n;
  return n;
}
static unsigned long long* g_gn_trace = nullptr;

template <int RP, int SV>
static void launch_gn_sv(const GnArgs& a, int na, hipStream_t s) {
  switch (na) {
    case 1: hipLaunchKernelGGL((gn_step_kernel<RP, 1, SV>), dim3(a.T), dim3(64 * 2), 0, s, a); break;
    case 3: hipLaunchKernelGGL((gn_step_kernel<RP, 3, SV>), dim3(a.T), dim3(64 * 4), 0, s, a); break;
    case 4: hipLaunchKernelGGL((gn_step_kernel<RP, 4, SV>), dim3(a.T), dim3(64 * 5), 0, s, a); break;
    default: hipLaunchKernelGGL((gn_step_kernel<RP, 2, SV>), dim3(a.T), dim3(64 * 3), 0, s, a); break;
  }
}

// shipped: solver 2 (the two-ended elimination); v & 16 selects solver 1 (one top-down chain of
// swept inverses) and v & 8 the round-2 block Cholesky, both with v & 7 assembler waves
// cyclic reduction for launches of few trajectories (v & 64 forces it, v & 128 never)
template <int RP>
static void launch_gn(const GnArgs& a, int v, hipStream_t s) {
  v &= 255;
  const bool cr_ok = a.L <= GN_CR_LMAX && !(v & 63);
  // (T x 24, us, two-ended / cyclic: 3: 41.3 / 33.4, 64: 41.9 / 33.9, 256: 42.6 / 34.4,
  // 512: 54.1 / 66.6, 1000: 71.3 / 130.8; profiles/r04i/gn_cr_ab.log)
  if (cr_ok && ((v & 64) || (!(v & 128) && a.T <= g_gn_cus())))
    hipLaunchKernelGGL((gn_cr_kernel<RP, GN_CR_NS<RP>>), dim3(a.T), dim3(64 * GN_CR_W), 0, s, a);
  else if (v & 8)
    launch_gn_sv<RP, 0>(a, v & 7, s);
  else if (v & 16)
    launch_gn_sv<RP, 1>(a, v & 7, s);
  else if ((v & 32) || a.T > 2 * g_gn_cus())  // 32: force the 4-per-CU form
    hipLaunchKernelGGL((gn_twisted_kernel<RP, 4>), dim3(a.T), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((gn_twisted_kernel<RP, 2>), dim3(a.T), dim3(256), 0, s, a);
}

}  // namespace pa

extern "C" {

int pa_debug_gn_set_trace(unsigned long long* trace_dev) {
  pa::g_gn_trace = trace_dev;
  return PA_OK;
}

int pa_debug_gn_set_assemblers(int na) {
  PA_CHECK((na & 7) <= 4 && na >= 0 && na < 4096 && !((na & 8) && (na & 16)) && !((na & 64) && (na & 128)),
           "gn variant %d: assembler waves (0..4) + 8 * legacy Cholesky or 16 * single-chain solver, 32: "
           "two-ended kernel in its 4-per-CU form, 64: cyclic reduction (L <= 24), 128: never cyclic "
           "reduction; pa_window_pose_tick debugging: 1024 its linearize launch only, 2048 its GN launch only",
           na);
  pa::g_gn_na = na;
  return PA_OK;
}

size_t pa_trajectory_gn_workspace(int T, int L) {
  return (T > 0 && L > 0) ? (size_t)T * L * pa::GN_WSF * sizeof(double) : 0;
}

// pa_trajectory_gn_step with the marginalization prior on frame 0 (prior_info / prior_grad null: none)
// and the constant-velocity factor on the angular velocity (r_cw null: none); both null: the parent
int pa_trajectory_gn_step_cw(int T, int L, int n_kp, const double* r_proj, const double* j_proj,
                             const int32_t* status_proj, const double* r_dyn, const double* j_dyn0,
                             const double* j_dyn1, const double* j_dyn2, const double* j_dyn3, const double* r_cv,
                             const double* j_cv0, const double* j_cv1, const double* r_cw, const double* isig_cw,
                             double lambda, double* D, double* E, double* g, double* delta, int32_t* info, void* ws,
                             size_t ws_bytes, const double* prior_info, const double* prior_grad, void* stream) {
  PA_CHECK(T >= 0 && L >= 1 && n_kp >= 0 && n_kp <= pa::GN_KMAX, "gn: T %d L %d n_kp %d (<= %d)", T, L, n_kp,
           pa::GN_KMAX);
  if (T == 0) return PA_OK;
  PA_CHECK(lambda >= 0.0, "gn: lambda %g < 0", lambda);
  PA_CHECK(delta && ws, "gn: null delta / workspace pointer");
  PA_CHECK(!prior_info == !prior_grad, "gn: prior_info and prior_grad are given together (or both NULL)");
  PA_CHECK((!D && !E && !g) || (D && g && (L == 1 || E)), "gn: D, E, g are given together (or all NULL)");
  PA_CHECK(n_kp == 0 || (r_proj && j_proj), "gn: null projection factors");
  PA_CHECK(L == 1 || (r_dyn && j_dyn0 && j_dyn1 && j_dyn2 && j_dyn3 && r_cv && j_cv0 && j_cv1),
           "gn: null dynamics / constant-velocity factors (Jacobians are required)");
  PA_CHECK(ws_bytes >= pa_trajectory_gn_workspace(T, L), "gn: workspace %zu < %zu", ws_bytes,
           pa_trajectory_gn_workspace(T, L));
  const pa::GnArgs a{T,     L,      n_kp,   r_proj, j_proj, status_proj, r_dyn, j_dyn0, j_dyn1, j_dyn2, j_dyn3,
                     r_cv,  j_cv0,  j_cv1,  lambda, D,      E,           g,     delta,  info,   (double*)ws,
                     pa::g_gn_trace, prior_info, prior_grad, r_cw, isig_cw};
  PA_CHECK(!r_cw || isig_cw, "gn: r_cw is given without isig_cw (the factor's Jacobians are -+ diag(isig_cw))");
  const hipStream_t s = (hipStream_t)stream;
  pa::gn_for_kp(n_kp, [&](auto rp) { pa::launch_gn<decltype(rp)::value>(a, pa::g_gn_na, s); });
  PA_LAUNCH_CHECK();
  return PA_OK;
}

int pa_trajectory_gn_step_prior(int T, int L, int n_kp, const double* r_proj, const double* j_proj,
                                const int32_t* status_proj, const double* r_dyn, const double* j_dyn0,
                                const double* j_dyn1, const double* j_dyn2, const double* j_dyn3, const double* r_cv,
                                const double* j_cv0, const double* j_cv1, double lambda, double* D, double* E,
                                double* g, double* delta, int32_t* info, void* ws, size_t ws_bytes,
                                const double* prior_info, const double* prior_grad, void* stream) {
  return pa_trajectory_gn_step_cw(T, L, n_kp, r_proj, j_proj, status_proj, r_dyn, j_dyn0, j_dyn1, j_dyn2, j_dyn3, r_cv,
                                  j_cv0, j_cv1, nullptr, nullptr, lambda, D, E, g, delta, info, ws, ws_bytes,
                                  prior_info, prior_grad, stream);
}

int pa_trajectory_gn_step(int T, int L, int n_kp, const double* r_proj, const double* j_proj,
                          const int32_t* status_proj, const double* r_dyn, const double* j_dyn0,
                          const double* j_dyn1, const double* j_dyn2, const double* j_dyn3, const double* r_cv,
                          const double* j_cv0, const double* j_cv1, double lambda, double* D, double* E, double* g,
                          double* delta, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
  return pa_trajectory_gn_step_prior(T, L, n_kp, r_proj, j_proj, status_proj, r_dyn, j_dyn0, j_dyn1, j_dyn2, j_dyn3, r_cv, j_cv0, j_cv1,
                      lambda, D, E, g, delta, info, ws, ws_bytes, nullptr, nullptr, stream);
}

}  // extern "C"
