// The data format every detector conv kernel shares, defined once: the LDS tile
// image and its swizzles, the lane -> pixel map of an MFMA fragment, the output-channel
// order of the weight rows, the tap order of the VGPR-resident weights, and the small
// device primitives (MFMA wrapper, compile-time loop, LDS-DMA, vmcnt wait, 8-byte
// store, hi / lo split) the kernels are written in.  The pure index functions are
// __host__ __device__ constexpr: the host weight packer (detector.hip) and the kernels
// call the same function, and the static_asserts below check each one at compile time.
#pragma once
#include <type_traits>

#include "common.h"

namespace pa {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// elements per 128-byte K step (one LDS row): 64 fp16 or 32 f32
template <typename T>
constexpr int kstep_elems = 128 / (int)sizeof(T);

// ------------------------------------------------------------- LDS tile image
// Rows of 128 B (one K-step: one pixel's or one output channel's 64 fp16 / 32 f32 of
// the current channel block), 8 chunks of 16 B; chunk c of row r lives at chunk slot
// c ^ ((r >> 1) & 7).  A 16x16x32 (f16) or 16x16x4 (f32) fragment read has 16
// consecutive rows x one chunk per 16-lane group, which this XOR spreads over all 16
// bank slots of a 256-B bank row for every ds_read_b128 lane group.
__host__ __device__ constexpr int tile_swz(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

// Rows of 256 B (16 chunks of 16 B: a pixel's 64 f32, or a weight row's 128 fp16),
// chunk c of row r at chunk slot c ^ (r & 15): 16 rows read at one chunk hit 16
// different bank quads.
__host__ __device__ constexpr int tile_swz256(int row, int chunk) { return row * 256 + ((chunk ^ (row & 15)) << 4); }

// Lane -> pixel map of a 16-pixel MFMA fragment: lanes whose ds_read_b128 lane
// groups read chunk c0 take the even pixel offsets, the others the odd ones, so
// with the (p >> 1) & 7 XOR swizzle every 16-lane group hits 16 distinct bank
// slots for ANY starting pixel (the 9 taps shift the start by 1 and by the patch width).
__host__ __device__ constexpr int frag_pixel(int r) { return r < 4 ? 2 * r : (r < 12 ? 2 * (r - 4) + 1 : 2 * (r - 8)); }

// Output-channel order of the weight rows inside each group of 32: LDS row
// rho = 16 t + 4 q + v (MFMA tile t of a pair, lane quad q, accumulator slot v)
// holds channel 8 q + 4 t + v, so a lane's two tiles of a pair cover 8
// consecutive channels of its pixel -> 16-byte residual loads and output stores.
__host__ __device__ constexpr int cout_perm(int rho) {
  return (rho & ~31) | (((rho >> 2) & 3) << 3) | (((rho >> 4) & 1) << 2) | (rho & 3);
}

// Kernels that hold the weights in VGPRs (conv_s2v.hip, conv_x3s2v.hip, conv_x3s2k.hip)
// walk a tile's K loop in groups g: conv_s2w.h's tap order [3 4 5 0 1 2 6 7 8][g / 2],
// half g & 1 of the tap's 64 channels.
__host__ __device__ constexpr int vgpr_tap(int g) {
  return (g >> 1) < 3 ? 3 + (g >> 1) : ((g >> 1) < 6 ? (g >> 1) - 3 : (g >> 1));
}

namespace tile_check {
// f(base + i), i < n, takes every value of [base, base + n) once
template <typename F>
constexpr bool is_perm(F f, int base, int n) {
  unsigned long long seen = 0;
  for (int i = 0; i < n; ++i) {
    const int v = f(base + i) - base;
    if (v < 0 || v >= n || ((seen >> v) & 1)) return false;
    seen |= 1ull << v;
  }
  return true;
}
// the chunks of every row map onto the row's own 16-byte slots, one each (the XOR terms have period 16 in the row)
template <typename F>
constexpr bool swz_bijective(F f, int rowb) {
  for (int row = 0; row < 32; ++row) {
    unsigned seen = 0;
    for (int c = 0; c < rowb / 16; ++c) {
      const int o = f(row, c) - row * rowb;
      if (o < 0 || o >= rowb || (o & 15) || ((seen >> (o >> 4)) & 1)) return false;
      seen |= 1u << (o >> 4);
    }
  }
  return true;
}
constexpr bool cout_perm_ok() {
  for (int g = 0; g < 512; g += 32) {
    if (!is_perm(cout_perm, g, 32)) return false;
    for (int i = 0; i < 32; ++i)
      if ((cout_perm(g + i) & ~31) != g) return false;
  }
  return true;
}
constexpr bool vgpr_tap_ok() {
  for (int g = 0; g < 18; g += 2)
    if (vgpr_tap(g) != vgpr_tap(g + 1)) return false;
  return is_perm([](int t) { return vgpr_tap(2 * t); }, 0, 9);
}
static_assert(swz_bijective(tile_swz, 128) && swz_bijective(tile_swz256, 256), "swizzle: a bijection on a row's chunks");
static_assert(is_perm(frag_pixel, 0, 16), "fragment map: a permutation of 0..15");
static_assert(cout_perm_ok(), "channel order: a permutation of every 32-row group");
static_assert(vgpr_tap_ok(), "tap order: a permutation of 0..8, two halves per tap");
}  // namespace tile_check

// ------------------------------------------------------------ device primitives
template <int V>
using int_c = std::integral_constant<int, V>;

// compile-time loop: f(integral_constant<int, I>) for I in [B, E)
template <int B, int E, typename F>
__device__ __forceinline__ void const_for(F&& f) {
  if constexpr (B < E) {
    f(int_c<B>{});
    const_for<B + 1, E>(f);
  }
}

// One 16-byte K-chunk per lane: lane l holds A[row l&15][chunk l>>4] and
// B[k][col l&15] for the same k range.
template <typename T>
__device__ __forceinline__ void mfma16(f32x4& acc, const u32x4& a, const u32x4& b);
template <>
__device__ __forceinline__ void mfma16<_Float16>(f32x4& acc, const u32x4& a, const u32x4& b) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b), acc, 0, 0,
                                               0);
}
template <>
__device__ __forceinline__ void mfma16<float>(f32x4& acc, const u32x4& a, const u32x4& b) {
  // The 16 B per lane hold k = 4q..4q+3 (q = lane>>4); MFMA step j consumes
  // element j of every lane, i.e. k = 4q + j.  A and B use the same permutation
  // of k, so the sum over k is unchanged.
  f32x4 fa = __builtin_bit_cast(f32x4, a), fb = __builtin_bit_cast(f32x4, b);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[0], fb[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[1], fb[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[2], fb[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[3], fb[3], acc, 0, 0, 0);
}

// 8-byte write-through store of a half4 at byte offset `off` from the wave-uniform base
// (conv.h store16's narrow form)
__device__ __forceinline__ void store_half4(void* base, unsigned off, half4 v) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7fffffff, 0x00020000);
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, (int)off, 0, 16);
}

// hi / lo fp16 pair of an f32 value (hi + lo == v to 2^-22 relative)
struct HiLo {
  _Float16 hi, lo;
};
__device__ __forceinline__ HiLo split_x3(float v) {
  const _Float16 h = (_Float16)v;
  return HiLo{h, (_Float16)(v - (float)h)};
}

template <int N>
__device__ __forceinline__ void xwait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (0x7 << 4) | (0xF << 8));
#endif
}
// 16 B per lane global -> LDS (wave-uniform LDS base + lane * 16), as inline asm:
// with the builtin, hipcc's waitcnt pass stops counting LDS reads in order once an
// LDS-DMA is pending and waits lgkmcnt(0) at the next use of any LDS read (every
// step, right after the barrier).  The pass does not see these VMEM ops, so every
// wait for DMA'd data is the explicit xwait_vm; its own vmcnt waits (bias,
// residual) only get more conservative.  M0 write -> LDS-DMA needs one wait state.
__device__ __forceinline__ void xdma16(const void* src, char* lds) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned off = __builtin_amdgcn_readfirstlane(
      (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds);
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"  // m0 is reserved: nothing else in these kernels keeps it live
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(off), "v"(src) : "memory", "m0");
#pragma clang diagnostic pop
#endif
}

// 16 B per lane from a buffer resource -> LDS (wave-uniform LDS base + lane * 16), as inline
// asm like xdma16 (its waits are explicit).  A lane whose 32-bit byte offset is
// out of the resource's range (S2W_OOB) reads zeros: the halo needs no pointer select and
// the per-lane address is one 32-bit VGPR (the 64-bit pointer math of xdma16 kept ~75
// VGPRs live across conv_s2w.h's unrolled loop and spilled).
constexpr unsigned S2W_OOB = 0x80000000u;
__device__ __forceinline__ u32x4 s2w_rsrc(const void* base, unsigned bytes) {
  // wave-uniform by construction; readfirstlane puts it in SGPRs for the asm's "s" operand
  const unsigned long long b = (unsigned long long)base;
  return u32x4{(unsigned)__builtin_amdgcn_readfirstlane((unsigned)b),
               (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(b >> 32) & 0xffffu),
               (unsigned)__builtin_amdgcn_readfirstlane(bytes), 0x00020000u};
}
__device__ __forceinline__ void s2w_dma16(u32x4 rsrc, unsigned voff, char* lds) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned off = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)lds);
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"  // m0 is reserved: nothing else in these kernels keeps it live
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(off), "v"(voff),
               "s"(rsrc) : "memory", "m0");
#pragma clang diagnostic pop
#endif
}

}  // namespace pa
