// Device code of the block cyclic reduction over one trajectory's frames (gn_cr_run), shared
// by gn_cr_kernel (gn.hip), the streaming pose tick (pose_tick.hip) and the LM step (lm.hip).
#pragma once
#include "gn_dev.h"

namespace pa {

// ---------------------------------------------------------------- cyclic reduction (few trajectories)
// At T = 3 (the streaming tick) the two-ended elimination (gn.hip, gn_twisted_kernel) is a 13-frame serial chain on
// 3 CUs.  Block cyclic reduction cuts the serial depth to log2(L) levels by eliminating every
// other active frame at once.  One workgroup of 12 waves per trajectory, all blocks in LDS:
//   assembly   the waves build frames w, w + NS, .. (gn_build_frame) straight into fb[l] = D | E | g,
//              then S_l = D_l + lambda I, b_l = -g_l, C_l = E_l (the coupling to the next
//              active frame)
//   level      active frames a_0 .. a_{n-1}; n even: the odd positions are eliminated, n odd:
//              the even ones (so every eliminated frame's neighbours survive).  Eliminated i
//              with neighbours p < i < q (either may be absent):
//                M_i = S_i^-1 (gn_sweep: the PD test of the pivot), z_i = M_i b_i,
//                PM_i = C_p M_i,  QM_i = C_i^T M_i                    (one wave each)
//              then each survivor s with eliminated neighbours h < s < i and next survivor q:
//                S_s -= QM_h C_h + PM_i C_s^T,  b_s -= C_h^T z_h + C_s z_i,
//                C_s <- -PM_i C_i                                     (one wave each)
//   last       n = 1: delta = S^-1 b
//   back       levels in reverse: delta_i = z_i - PM_i^T delta_p - QM_i^T delta_q.
// L = 24: 5 sweeps in series (24 -> 12 -> 6 -> 3 -> 1 -> solve) instead of 13; about twice
// the flops of the elimination, so it is the form for launches that leave CUs idle.  The
// 12 x 12 products run on the f64 matrix cores.  info: the 1-based frame of the first
// level's (lowest) pivot block that is not positive definite, 0 = solved.
constexpr int GN_CR_LMAX = 24;
constexpr int GN_CR_W = 12;  // waves per workgroup
typedef double gn_d4 __attribute__((ext_vector_type(4)));

// acc += A B for 12 x 12 row-major LDS blocks (A read transposed when TA, B when TB), on the
// f64 matrix cores: A operand lane l = (row l & 15, k = l >> 4), B operand (k = l >> 4,
// column l & 15), result register v = (row (l >> 4) + 4 v, column l & 15); rows / columns
// 12..15 are zero padding
template <bool TA, bool TB>
__device__ __forceinline__ gn_d4 gn_mm_acc(const double* A, const double* B, gn_d4 acc) {
  using namespace gn;
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const bool in = li < NV;
  const int lr = in ? li : 0;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int k = 4 * q + lk;
    const double av = in ? (TA ? A[k * NV + lr] : A[lr * NV + k]) : 0.0;
    const double bv = in ? (TB ? B[lr * NV + k] : B[k * NV + lr]) : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
  }
  return acc;
}

// a C-layout result to a 12 x 12 row-major LDS block (scaled by s)
__device__ __forceinline__ void gn_mm_store(double* out, const gn_d4& c, double s) {
  using namespace gn;
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  if (li < NV)
#pragma unroll
    for (int v = 0; v < 3; ++v) out[(lk + 4 * v) * NV + li] = s * c[v];
}

// assembler waves of the RP instantiation (the general-K one's staging does not fit 12 times)
template <int RP>
constexpr int GN_CR_NS = RP <= 34 ? 12 : 8;

// LDS of gn_cr_run: fb (S | C | b per frame) and the pool (assembly staging, then the level data)
template <int RP, int NS, bool ROOT = false>
struct GnCrLds {
  static constexpr int BLK = 2 * gn::NB + gn::NV;
  static constexpr int LM = GN_CR_LMAX, W = GN_CR_W;
  static constexpr int CHD = (int)(sizeof(GnChainLds) / sizeof(double));
  static constexpr int STGD = (int)(sizeof(GnStage<RP>) / sizeof(double));
  static constexpr int FR = 2 * gn::NB + gn::NV;  // per eliminated frame: PM | QM | z
  // PAIR (one assembler wave per two frames, NS = W): wave w builds frames 2w, 2w + 1 and
  // eliminates 2w + 1 at once (level 0 eliminates the odd positions whatever L's parity), so
  // level 0 needs no barrier of its own.  Its slab of the pool is its staging, then the
  // PM | QM | z of frames 2w + 1 and 2w and its sweep scratch.  Otherwise (the general-K
  // instance: its staging does not fit 12 times) NS waves assemble, then every wave starts.
  static constexpr bool PAIR = !ROOT && NS == W && 2 * W >= LM;
  static constexpr int SLAB0 = 2 * FR + CHD > STGD ? 2 * FR + CHD : STGD;
  static constexpr int SLAB = (SLAB0 + 1) / 2 * 2;
  static constexpr int POST = LM * FR + W * CHD;
  static constexpr int STG = NS * STGD;
  static constexpr int POOL = PAIR ? W * SLAB : (POST > STG ? POST : STG);
};

// The split streaming tick (pa_window_pose_tick_pre / _post): per trajectory, what the pre
// half leaves for the post half in the workspace a.ws (doubles): per frame B_l | a_l (the
// back substitution run on the root's delta as an unknown: delta_l = a_l + B_l delta_root),
// the root's S | b, the failure word
constexpr int GN_TICK_FRD = gn::NB + gn::NV;
constexpr int GN_TICK_WSD = GN_CR_LMAX * GN_TICK_FRD + gn::NB + gn::NV + 2;

// the level lists: frames active at each level, the parity of the eliminated positions
// (pe), the level count.  Shipped order: n even -> the odd positions, n odd -> the even ones
// (PAIR: level 0 the odd ones whatever the parity).  ROOT (the split tick): n even -> the
// even positions, n odd -> the odd ones, so position n - 1, frame L - 1, is never eliminated
// and stays as the root of the reduction (24 -> 12 -> 6 -> 3 -> 2 -> 1: one level more).
template <bool PAIR, bool ROOT>
__device__ __forceinline__ int gn_cr_lists(int L, signed char (*lst)[GN_CR_LMAX], int* lcnt, int* lpe) {
  int n = L, lv = 0;
  for (int l = 0; l < L; ++l) lst[0][l] = (signed char)l;
  while (n > 1) {
    const int pe = ROOT ? (n & 1) : ((PAIR && lv == 0) || !(n & 1) ? 1 : 0);
    int m = 0;
    for (int p = 0; p < n; ++p)
      if ((p & 1) != pe) lst[lv + 1][m++] = lst[lv][p];
    lcnt[lv] = n;
    lpe[lv] = pe;
    n = m;
    ++lv;
  }
  lcnt[lv] = 1;
  return lv;
}

// trajectory t on this workgroup (64 * GN_CR_W threads); fb / pool: GnCrLds<RP, NS, ROOT> in LDS.
// ROOT (pa_window_pose_tick_pre): the ROOT level order, and after the last level the reduced
// system goes to the workspace (GN_TICK_WSD per trajectory) instead of being solved.
template <int RP, int NS, bool ROOT = false>
__device__ __forceinline__ void gn_cr_run(const GnArgs& a, int t, double (*fb)[GnCrLds<RP, NS, ROOT>::BLK], double* pool) {
  using namespace gn;
  using Ld = GnCrLds<RP, NS, ROOT>;
  constexpr int LM = Ld::LM, W = Ld::W, CHD = Ld::CHD, FR = Ld::FR, SLAB = Ld::SLAB;
  constexpr bool PAIR = Ld::PAIR;
  constexpr int NOFAIL = 0x7fffffff;
  static_assert(NS <= W, "assembler waves");
  __shared__ signed char lst[8][LM];  // active frames per level
  __shared__ int lcnt[8], lpe[8];
  __shared__ int nlev_s, fail;
  const int wv = threadIdx.x >> 6;
  const int i = threadIdx.x & 63;
  const int L = a.L;
  const long f0 = (long)t * L;
  auto fr = [&](int f) __attribute__((always_inline)) -> double* {  // PM | QM | z of frame f
    return PAIR ? pool + (f >> 1) * SLAB + ((f & 1) ? 0 : FR) : pool + f * FR;
  };
  GnChainLds& C = *reinterpret_cast<GnChainLds*>(PAIR ? pool + wv * SLAB + 2 * FR : pool + LM * FR + wv * CHD);
  auto dl = [&](int f) __attribute__((always_inline)) -> double* { return fb[f]; };
  if (threadIdx.x == 0) {
    nlev_s = gn_cr_lists<PAIR, ROOT>(L, lst, lcnt, lpe);
    fail = NOFAIL;
  }
  // the level lists and `fail` are in place before any wave eliminates or reads them (LDS
  // holds whatever the previous kernel left: an unsynchronised read of nlev_s gave waves
  // different level counts, i.e. different barrier counts -- a hang)
  __syncthreads();
  if (wv == 0) gn_stamp(a, t, 0);
  const bool act = i < 36;
  const int ii = act ? i : 35;
  const int r = ii / 3, c0 = 4 * (ii - 3 * (ii / 3));
  // eliminate frame fi (neighbours fp, fq, or -1): M = S^-1 (false if S is not PD), z = M b,
  // PM = C_p M, QM = C_fi^T M
  auto eliminate = [&](int fi, int fp, int fq) __attribute__((always_inline)) {
    double sv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) sv[c] = fb[fi][r * NV + c0 + c];
    const double b = fb[fi][2 * NB + r];
    if (!gn_sweep(sv, C.rk2, r, c0, act)) {
      if (i == 0) __hip_atomic_fetch_min(&fail, fi + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      return;
    }
    double* o = fr(fi);
    const double z = gn_finish(sv, b, C, r, c0, act);  // C.M = M
    if (act && c0 == 0) o[2 * NB + r] = z;
    if (fp >= 0) gn_mm_store(o, gn_mm_acc<false, false>(fb[fp] + NB, C.M, gn_d4{0, 0, 0, 0}), 1.0);
    if (fq >= 0) gn_mm_store(o + NB, gn_mm_acc<true, false>(fb[fi] + NB, C.M, gn_d4{0, 0, 0, 0}), 1.0);
  };
  // S = D + lambda I, b = -g (frame l; lanes < 12 of one wave)
  auto init = [&](int l) __attribute__((always_inline)) {
    if (i < NV) {
      fb[l][i * NV + i] += a.lambda;
      fb[l][2 * NB + i] = -fb[l][2 * NB + i];
    }
  };
  if constexpr (PAIR) {
    // ---- wave w: frames 2w, 2w + 1 (both loads issued before either is built), then the
    // level-0 elimination of 2w + 1
    const int la = 2 * wv, lb = 2 * wv + 1;
    if (la < L) {
      GnStage<RP>& st = *reinterpret_cast<GnStage<RP>*>(pool + wv * SLAB);
      gn_zero_stage<RP>(st);
      GnFrameLoads<RP> ld0, ld1;
      gn_load_frame<RP>(a, f0 + la, ld0);
      if (lb < L) gn_load_frame<RP>(a, f0 + lb, ld1);
      gn_build_frame<RP, false>(a, f0 + la, ld0, st, fb[la]);
      if (lb < L) gn_build_frame<RP, false>(a, f0 + lb, ld1, st, fb[lb]);
      wave_order();
      init(la);
      if (lb < L) init(lb);
      wave_order();
      if (wv == 0) gn_stamp(a, t, 2);
      if (lb < L) eliminate(lb, la, lb + 1 < L ? lb + 1 : -1);  // (the staging is dead: the slab's new use)
    }
  } else {
    if (wv < NS) {
      GnStage<RP>& st = reinterpret_cast<GnStage<RP>*>(pool)[wv];
      gn_zero_stage<RP>(st);
      GnFrameLoads<RP> ld0;
      if (wv < L) gn_load_frame<RP>(a, f0 + wv, ld0);
      for (int l = wv; l < L; l += NS) {
        const GnFrameLoads<RP> cu = ld0;
        if (l + NS < L) gn_load_frame<RP>(a, f0 + l + NS, ld0);
        gn_build_frame<RP, false>(a, f0 + l, cu, st, fb[l]);
      }
      if (wv == 0) gn_stamp(a, t, 2);
    }
    __syncthreads();
    for (int l = wv; l < L; l += W) init(l);
  }
  __syncthreads();
  const int nlev = nlev_s;  // (after a barrier: thread 0 wrote it)
  if (wv == 0) gn_stamp(a, t, 1);
  int lv = 0;
  for (; lv < nlev; ++lv) {
    const int n = lcnt[lv], pe = lpe[lv];
    const int ne = pe ? n / 2 : (n + 1) / 2;
    if (!(PAIR && lv == 0)) {
      for (int e = wv; e < ne; e += W) {  // eliminated frames
        const int pos = 2 * e + pe;
        eliminate(lst[lv][pos], pos > 0 ? lst[lv][pos - 1] : -1, pos + 1 < n ? lst[lv][pos + 1] : -1);
      }
      __syncthreads();
    }
    if (wv == 0) gn_stamp(a, t, 10 + 2 * lv);
    if (fail != NOFAIL) break;
    const int ns = n - ne;
    for (int s = wv; s < ns; s += W) {  // survivors
      const int pos = 2 * s + (1 - pe);
      const int fs = lst[lv][pos];
      const int fh = pos > 0 ? lst[lv][pos - 1] : -1;
      const int fi = pos + 1 < n ? lst[lv][pos + 1] : -1;
      const bool cq = fi >= 0 && pos + 2 < n;  // a next survivor: new coupling
      gn_d4 acc = {0.0, 0.0, 0.0, 0.0}, cn = {0.0, 0.0, 0.0, 0.0};
      if (fh >= 0) acc = gn_mm_acc<false, false>(fr(fh) + NB, fb[fh] + NB, acc);
      if (fi >= 0) acc = gn_mm_acc<false, true>(fr(fi), fb[fs] + NB, acc);
      if (cq) cn = gn_mm_acc<false, false>(fr(fi), fb[fi] + NB, cn);
      double db0 = 0.0, db1 = 0.0;
      if (i < NV) {
        if (fh >= 0) {
          const double* zh = fr(fh) + 2 * NB;
#pragma unroll
          for (int k = 0; k < NV; ++k) db0 += fb[fh][NB + k * NV + i] * zh[k];
        }
        if (fi >= 0) {
          const double* zi = fr(fi) + 2 * NB;
#pragma unroll
          for (int k = 0; k < NV; ++k) db1 += fb[fs][NB + i * NV + k] * zi[k];
        }
      }
      wave_order();  // this wave's reads of fb[fs] are issued before its writes
      const int li = i & 15, lk = i >> 4;
      if (li < NV)
#pragma unroll
        for (int v = 0; v < 3; ++v) fb[fs][(lk + 4 * v) * NV + li] -= acc[v];
      if (cq) gn_mm_store(fb[fs] + NB, cn, -1.0);
      if (i < NV) fb[fs][2 * NB + i] -= db0 + db1;
    }
    __syncthreads();
    if (wv == 0) gn_stamp(a, t, 11 + 2 * lv);
  }
  if constexpr (ROOT) {
    // the root (frame L - 1) S | b and the failure word to the workspace, then the back
    // substitution with delta_root unknown: delta_l = a_l + B_l delta_root, B_root = I, a_root = 0,
    //   B_i = -(PM_i^T B_p + QM_i^T B_q),  a_i = z_i - PM_i^T a_p - QM_i^T a_q
    // level by level in reverse (the products on the f64 matrix cores), into fb[l] (its S and C
    // are dead): B_l | a_l, then to the workspace
    constexpr int FD = GN_TICK_FRD;
    double* w = a.ws + (size_t)t * GN_TICK_WSD;
    const int rt = L - 1;
    for (int e = threadIdx.x; e < NB + NV; e += 64 * W) w[LM * FD + e] = e < NB ? fb[rt][e] : fb[rt][NB + e];
    if (threadIdx.x == 0) reinterpret_cast<int*>(w + LM * FD + NB + NV)[0] = fail == NOFAIL ? 0 : fail;
    if (fail != NOFAIL) return;  // (uniform: read after the last level's barrier)
    __syncthreads();  // every read of the root's S | b is done
    for (int e = threadIdx.x; e < FD; e += 64 * W) fb[rt][e] = (e < NB && e % (NV + 1) == 0) ? 1.0 : 0.0;
    __syncthreads();
    for (lv = nlev - 1; lv >= 0; --lv) {
      const int n = lcnt[lv], pe = lpe[lv];
      const int ne = pe ? n / 2 : (n + 1) / 2;
      for (int e = wv; e < ne; e += W) {
        const int pos = 2 * e + pe;
        const int fi = lst[lv][pos];
        const int fp = pos > 0 ? lst[lv][pos - 1] : -1, fq = pos + 1 < n ? lst[lv][pos + 1] : -1;
        const double* o = fr(fi);
        gn_d4 acc = {0.0, 0.0, 0.0, 0.0};
        if (fp >= 0) acc = gn_mm_acc<true, false>(o, fb[fp], acc);
        if (fq >= 0) acc = gn_mm_acc<true, false>(o + NB, fb[fq], acc);
        double av = 0.0;
        if (i < NV) {
          double d0 = o[2 * NB + i], d1 = 0.0;
          if (fp >= 0)
#pragma unroll
            for (int k = 0; k < NV; ++k) d0 -= o[k * NV + i] * fb[fp][NB + k];
          if (fq >= 0)
#pragma unroll
            for (int k = 0; k < NV; ++k) d1 += o[NB + k * NV + i] * fb[fq][NB + k];
          av = d0 - d1;
        }
        gn_mm_store(fb[fi], acc, -1.0);  // (fb[fi] is this wave's alone; nothing above reads it)
        if (i < NV) fb[fi][NB + i] = av;
      }
      __syncthreads();
    }
    for (int e = threadIdx.x; e < L * FD / 2; e += 64 * W) {
      const int l = e / (FD / 2), c = e - l * (FD / 2);
      reinterpret_cast<gn_d2*>(w + l * FD)[c] = reinterpret_cast<const gn_d2*>(fb[l])[c];
    }
    return;
  }
  if (fail == NOFAIL && wv == 0) {  // the last active frame: delta = S^-1 b (over its S block)
    const int ff = lst[nlev][0];
    double sv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) sv[c] = fb[ff][r * NV + c0 + c];
    const double b = fb[ff][2 * NB + r];
    if (!gn_sweep(sv, C.rk2, r, c0, act)) {
      if (i == 0) __hip_atomic_fetch_min(&fail, ff + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
      const double z = gn_finish(sv, b, C, r, c0, act);
      wave_order();  // every lane's S reads are done
      if (act && c0 == 0) dl(ff)[r] = z;
    }
  }
  __syncthreads();
  if (wv == 0) gn_stamp(a, t, 30);
  const int info = fail == NOFAIL ? 0 : fail;
  if (!info) {
    for (lv = nlev - 1; lv >= 0; --lv) {  // delta_i over S_i's first row (dead since its elimination)
      const int n = lcnt[lv], pe = lpe[lv];
      const int ne = pe ? n / 2 : (n + 1) / 2;
      for (int e = wv; e < ne; e += W) {
        const int pos = 2 * e + pe;
        const int fi = lst[lv][pos];
        const int fp = pos > 0 ? lst[lv][pos - 1] : -1, fq = pos + 1 < n ? lst[lv][pos + 1] : -1;
        const double* o = fr(fi);
        if (i < NV) {
          double d0 = o[2 * NB + i], d1 = 0.0;
          if (fp >= 0)
#pragma unroll
            for (int k = 0; k < NV; ++k) d0 -= o[k * NV + i] * dl(fp)[k];
          if (fq >= 0)
#pragma unroll
            for (int k = 0; k < NV; ++k) d1 += o[NB + k * NV + i] * dl(fq)[k];
          dl(fi)[i] = d0 - d1;
        }
      }
      __syncthreads();
      if (wv == 0) gn_stamp(a, t, 31 + lv);
    }
  }
  double* delta = a.delta + (size_t)f0 * NV;
  for (int e = threadIdx.x; e < L * NV; e += 64 * W) {
    const int l = e / NV;
    delta[e] = info ? NAN : dl(l)[e - l * NV];
  }
  if (a.info && threadIdx.x == 0) a.info[t] = info;
  if (wv == 0) gn_stamp(a, t, 40);
}

}  // namespace pa
