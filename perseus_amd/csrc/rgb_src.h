// RGB-only camera / image frames (scripts/streaming.py:104,112-128 with an RGB model;
// perseus/detector/validate_real.py:62-74): uint8 HWC [B][Hs][Ws][3] -> the f32 NCHW
// (B,3,256,256) model input.  Two forms, chosen on the host:
//   crop only   x = (float)u8 / 255.0f at the centre 256 x 256 window (origin Hs/2 - 128,
//               Ws/2 - 128, as the RGBD path);
//   resize      v = (float)u8 / 255.0f, bilinear resize of v (align_corners = false, no
//               antialiasing: torch.nn.functional.interpolate's f32 arithmetic, which kornia's
//               resize calls) to kornia's side = "short" size for resize_short, then the centre
//               256 x 256 window of the resized image; only that window is computed.
// The per-pixel arithmetic lives here, once, for preprocess_rgb_kernel (conv.hip) and the fused
// source of the fp16 stem (stem.hip): both give the same bits.  Every step is an explicit
// single-rounding intrinsic, so -ffp-contract can neither add nor remove a fusion.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pa {

struct RgbSrc {
  const uint8_t* rgb;
  int Hs, Ws, bgr;
  int resize;    // 0: centre crop only (r0, c0 in the source)
  int r0, c0;    // origin of the 256 x 256 window in the source (crop) / resized image (resize)
  float sy, sx;  // resize: (float)Hs / (float)Hr, (float)Ws / (float)Wr
};

// kornia's side = "short" size rule (written from its published source), in double on the host;
// the one place it lives on the C side (perseus_amd.detector.real_image_size on the Python side)
void real_image_size(int Hs, int Ws, int S, int* Hr, int* Wr);
// validates the arguments of pa_preprocess_rgb / pa_detector_forward_rgb (no GPU call) and
// fills the kernels' source description
int make_rgb_src(const uint8_t* rgb, int Hs, int Ws, int bgr, int resize_short, RgbSrc* out);
int launch_preprocess_rgb(const RgbSrc& src, int B, float* x, hipStream_t s);
int launch_stem_pool_rgb(const RgbSrc& src, int B, const _Float16* w, const float* bias, _Float16* out,
                         hipStream_t s);

#if defined(__HIPCC__)
__device__ __forceinline__ float rgb_unit(uint8_t v) { return __fdiv_rn((float)v, 255.0f); }

// one axis of the bilinear resize: destination index dst of an axis resized from n samples
// with scale = (float)n / (float)m -> taps i0, i1 and their weights l0, l1
struct RgbTap {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ RgbTap rgb_tap(int dst, int n, float scale) {
  float src = __fmaf_rn(scale, __fadd_rn((float)dst, 0.5f), -0.5f);
  if (src < 0.f) src = 0.f;
  RgbTap t;
  t.i0 = min((int)src, n - 1);
  t.i1 = min(t.i0 + 1, n - 1);
  t.l1 = fminf(fmaxf(__fsub_rn(src, (float)t.i0), 0.f), 1.f);
  t.l0 = __fsub_rn(1.0f, t.l1);
  return t;
}
// width first, then height: a, b = row i0's taps at columns i0, i1; c, d = row i1's
__device__ __forceinline__ float rgb_lerp(const RgbTap& ty, const RgbTap& tx, float a, float b, float c, float d) {
  const float top = __fmaf_rn(tx.l0, a, __fmul_rn(tx.l1, b));
  const float bot = __fmaf_rn(tx.l0, c, __fmul_rn(tx.l1, d));
  return __fmaf_rn(ty.l0, top, __fmul_rn(ty.l1, bot));
}
// channel ch (0 = R) of the resized image at (row tap ty, column tap tx) of frame `f`
__device__ __forceinline__ float rgb_resized(const uint8_t* f, int Ws, int sc, const RgbTap& ty, const RgbTap& tx) {
  const uint8_t* r0 = f + (size_t)ty.i0 * Ws * 3 + sc;
  const uint8_t* r1 = f + (size_t)ty.i1 * Ws * 3 + sc;
  return rgb_lerp(ty, tx, rgb_unit(r0[(size_t)tx.i0 * 3]), rgb_unit(r0[(size_t)tx.i1 * 3]),
                  rgb_unit(r1[(size_t)tx.i0 * 3]), rgb_unit(r1[(size_t)tx.i1 * 3]));
}
#endif

}  // namespace pa
