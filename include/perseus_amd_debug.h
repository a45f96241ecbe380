/*
 * perseus_amd — tuning / measurement hooks of libperseus_amd.so.  Not part of the
 * drop-in surface (include/perseus_amd.h); nothing in production calls these.
 * Both settings belong to one pa_detector handle and apply to that handle's
 * forwards only (another handle in the same process keeps its own).
 */
#ifndef PERSEUS_AMD_DEBUG_H
#define PERSEUS_AMD_DEBUG_H

#include "perseus_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Interleaved A/B timing (tools/layer_ab.py, tools/head_ab.py): select kernel variant
 * `variant` for layer 1..4 (stage), 0 (stem), 5-7 (stride-2 entry / head options);
 * 0 = the shipped choice. */
int pa_detector_debug_set_variant(pa_detector* d, int layer, int variant);
/* Variants that give wrong results by construction (timing experiments) exist only in a
 * measurement build (PERSEUS_AMD_TIMING_VARIANTS=1 when building); the release library
 * returns PA_EINVAL for their ids (checked before the handle).  1 in a measurement build. */
int pa_debug_timing_variants_built(void);

/* Timestamping kernel variants write s_memrealtime stamps (100 MHz) to
 * trace_dev + launch * 65536 + workgroup * 64 (launch = index in the forward, stem = 0);
 * NULL turns it off. */
int pa_detector_debug_set_trace(pa_detector* d, unsigned long long* trace_dev);

/* Single-launch checks (tests/test_detector_layers_gpu.py): one launch of a forward, described as
 * an optional convolution (+ folded bias, + residual, ReLU), an optional 3x3 s2 p1 max pool behind
 * it and an optional avgpool + fc behind that.  conv / conv2 index the convolutions in weight-blob
 * order (0 = stem; then per block conv1, conv2 and, where the block has one, downsample); -1 = none.
 * B, Hin, Cin, Hout, Cout, ks, stride are the convolution's (square maps), or the pool's / head's
 * when the launch has no convolution. */
#define PA_TAP_RELU 1     /* ReLU after the bias / residual add                              */
#define PA_TAP_RES 2      /* the launch adds the residual map `res`                          */
#define PA_TAP_MAXPOOL 4  /* max pool 3x3 s2 p1 after the convolution (or alone)             */
#define PA_TAP_HEAD 8     /* mean over H x W, then the fc (alone or behind the convolution)  */
typedef struct pa_debug_tap {
  /* set by the caller: device buffers of `cap` bytes each (NULL = that map is not wanted) */
  void* in;
  void* res;
  void* out;
  void* out2;
  size_t cap;
  /* filled by the call: bytes copied into each buffer (0 = the launch has no such map, or the
   * buffer was NULL), the launch's profile name (static storage) and its description */
  size_t in_bytes, res_bytes, out_bytes, out2_bytes;
  const char* name;
  int conv, conv2, flags;
  int B, Hin, Cin, Hout, Cout, ks, stride;
} pa_debug_tap;

/* A normal forward of x_dev (the handle's precision, variants and split-K setting; y_dev gets
 * the keypoints) that also copies out the maps launch `index` touched, device to device on
 * `stream`, in the library's own layout: NHWC fp16 / f32, or fp16x3's [hi (C) | lo (C)] fp16
 * pair per pixel.  `index` counts launches as pa_detector_profile / _time_launch do (stem = 0; a
 * latency-mode conv and its reduce are one launch).  in: the map the launch reads; res: its
 * residual map, copied before the launch (identity blocks add it in place); out: the map it
 * writes; out2: the downsample map of a fused stride-2 + downsample launch (conv2 names its
 * convolution).  The stem's `in` is x_dev itself and a head's `out` is y_dev: neither is copied.
 * PA_EINVAL for B above one chunk (1,024 frames), an index past the last launch or a map
 * larger than `cap`. */
int pa_detector_debug_tap(pa_detector* d, const float* x_dev, int B, float* y_dev, void* stream, int index,
                          pa_debug_tap* tap);

/* Timing only: pa_trajectory_linearize with mode 1 = only the dynamics workgroups,
 * 2 = only the projection / constant-velocity workgroups (the other outputs are left
 * unwritten); mode 0 is pa_trajectory_linearize itself.  A non-NULL trace_dev (8 u64
 * per wave, 2 waves per workgroup) receives s_memrealtime stamps at each wave's phases. */
int pa_debug_trajectory_linearize(const pa_traj_args* args, int mode, unsigned long long* trace_dev, void* stream);

/* Timing / debugging only, process-wide: pa_trajectory_gn_step variant = assembler waves
 * per trajectory (1..4; 0 = the shipped count) + 8: the round-2 block-Cholesky solver, 16:
 * the single-chain swept-inverse solver, 32: the two-ended kernel's 4-per-CU form, 64: block
 * cyclic reduction forced (L <= 24), 128: never cyclic reduction; pa_window_pose_tick: 1024
 * launches its linearize kernel only, 2048 its GN kernel only. */
int pa_debug_gn_set_assemblers(int na);
/* Timing only: pa_trajectory_gn_step writes s_memrealtime stamps (100 MHz), 256 per
 * trajectory, to trace_dev (assembler frame l: slots 2l, 2l+1; solver frame l: 64+4l ..
 * 67+4l; solver-1 backward 250, 251); NULL turns it off.  Process-wide. */
int pa_debug_gn_set_trace(unsigned long long* trace_dev);

#ifdef __cplusplus
}
#endif
#endif /* PERSEUS_AMD_DEBUG_H */
