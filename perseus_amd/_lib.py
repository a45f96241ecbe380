"""ctypes binding of libperseus_amd.so (the C ABI in include/perseus_amd.h).

The library is the product: there is no fallback.  If it is missing or fails to
load, `lib()` raises; build it with `python -m perseus_amd.build`.
"""

from __future__ import annotations

import ctypes as C
import os

from . import build as _build

_LIB = None

c_double_p = C.POINTER(C.c_double)
c_float_p = C.POINTER(C.c_float)


class PerseusError(RuntimeError):
    pass


class TrajArgs(C.Structure):
    """Mirror of `pa_traj_args` (include/perseus_amd.h)."""

    _fields_ = [("T", C.c_int), ("L", C.c_int), ("n_kp", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("y", C.c_void_p), ("pose", C.c_void_p), ("vel", C.c_void_p), ("angvel", C.c_void_p),
                ("corners", C.c_void_p), ("K", C.c_void_p), ("tcam", C.c_void_p), ("dt", C.c_double),
                ("vel_frame", C.c_int), ("isig_proj", C.c_void_p), ("isig_dyn", C.c_void_p),
                ("isig_cv", C.c_void_p), ("isig_cw", C.c_void_p),
                ("r_proj", C.c_void_p), ("j_proj", C.c_void_p), ("err_proj", C.c_void_p),
                ("status", C.c_void_p), ("r_dyn", C.c_void_p), ("j_dyn0", C.c_void_p), ("j_dyn1", C.c_void_p),
                ("j_dyn2", C.c_void_p), ("j_dyn3", C.c_void_p), ("err_dyn", C.c_void_p),
                ("r_cw", C.c_void_p), ("err_cw", C.c_void_p), ("r_cv", C.c_void_p),
                ("j_cv0", C.c_void_p), ("j_cv1", C.c_void_p), ("err_cv", C.c_void_p),
                ("dt_pair", C.c_void_p), ("kp_mask", C.c_void_p), ("dt_new", C.c_void_p), ("mask_new", C.c_void_p),
                ("nvalid", C.c_void_p), ("robust_proj", C.c_int), ("robust_proj_k", C.c_double)]


class LMParams(C.Structure):
    """Mirror of `pa_lm_params` (include/perseus_amd.h)."""

    _fields_ = [("max_iters", C.c_int), ("lambda0", C.c_double), ("lambda_up", C.c_double),
                ("lambda_down", C.c_double), ("lambda_min", C.c_double), ("lambda_max", C.c_double),
                ("rel_tol", C.c_double), ("abs_tol", C.c_double)]


class LMPrior(C.Structure):
    """Mirror of `pa_lm_prior` (include/perseus_amd.h)."""

    _fields_ = [("info", C.c_void_p), ("eta", C.c_void_p), ("xbar_pose", C.c_void_p), ("xbar_angvel", C.c_void_p),
                ("xbar_vel", C.c_void_p), ("grad", C.c_void_p), ("err", C.c_void_p)]


class DebugTap(C.Structure):
    """Mirror of `pa_debug_tap` (include/perseus_amd_debug.h)."""

    _fields_ = [("in_", C.c_void_p), ("res", C.c_void_p), ("out", C.c_void_p), ("out2", C.c_void_p),
                ("cap", C.c_size_t), ("in_bytes", C.c_size_t), ("res_bytes", C.c_size_t),
                ("out_bytes", C.c_size_t), ("out2_bytes", C.c_size_t), ("name", C.c_char_p),
                ("conv", C.c_int), ("conv2", C.c_int), ("flags", C.c_int), ("B", C.c_int), ("Hin", C.c_int),
                ("Cin", C.c_int), ("Hout", C.c_int), ("Cout", C.c_int), ("ks", C.c_int), ("stride", C.c_int)]


TAP_RELU = 1
TAP_RES = 2
TAP_MAXPOOL = 4
TAP_HEAD = 8

LM_CONVERGED = 1
LM_MAX_ITERS = 2
LM_STALLED = 3

GATE_APPLIED = 0
GATE_FEW = 1
GATE_NOCOV = 2
GATE_YOUNG = 3

# name -> (restype, argtypes)
_SIGS = {
    "pa_trajectory_lm_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "pa_trajectory_lm_solve": (C.c_int, [C.POINTER(TrajArgs), C.POINTER(LMParams)] + [C.c_void_p] * 7
                               + [C.c_size_t, C.c_void_p]),
    "pa_window_lm_solve": (C.c_int, [C.POINTER(TrajArgs), C.POINTER(LMParams), C.c_int] + [C.c_void_p] * 7
                           + [C.c_size_t, C.c_void_p]),
    "pa_trajectory_lm_prior_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "pa_trajectory_lm_prior_solve": (C.c_int, [C.POINTER(TrajArgs), C.POINTER(LMParams), C.POINTER(LMPrior)]
                                     + [C.c_void_p] * 7 + [C.c_size_t, C.c_void_p]),
    "pa_window_lm_prior_solve": (C.c_int, [C.POINTER(TrajArgs), C.POINTER(LMParams), C.c_int, C.POINTER(LMPrior)]
                                 + [C.c_void_p] * 7 + [C.c_size_t, C.c_void_p]),
    "pa_window_pose_tick_reduce": (C.c_int, [C.POINTER(TrajArgs), C.c_double, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pa_trajectory_linearize": (C.c_int, [C.POINTER(TrajArgs), C.c_void_p]),
    "pa_debug_trajectory_linearize": (C.c_int, [C.POINTER(TrajArgs), C.c_int, C.c_void_p, C.c_void_p]),
    "pa_last_error": (C.c_char_p, []),
    "pa_version": (C.c_char_p, []),
    "pa_detector_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(C.c_void_p)]),
    "pa_detector_destroy": (None, [C.c_void_p]),
    "pa_detector_reserve": (C.c_int, [C.c_void_p, C.c_int]),
    "pa_detector_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "pa_detector_set_split_k": (C.c_int, [C.c_void_p, C.c_int]),
    "pa_detector_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "pa_detector_profile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int]),
    "pa_detector_flops_per_frame": (C.c_double, [C.c_void_p]),
    "pa_detector_time_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_int, C.c_void_p, C.c_void_p]),
    "pa_detector_debug_set_variant": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "pa_detector_debug_set_trace": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pa_detector_debug_tap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                        C.POINTER(DebugTap)]),
    "pa_debug_timing_variants_built": (C.c_int, []),
    "pa_preprocess_rgbd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pa_keypoints_postprocess": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "pa_detector_forward_rgbd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "pa_detector_forward_rgbd_px": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pa_preprocess_rgb": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p, C.c_void_p]),
    "pa_detector_forward_rgb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p]),
    "pa_detector_forward_rgb_px": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "pa_detector_profile_rgb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "pa_trajectory_gn_workspace": (C.c_size_t, [C.c_int, C.c_int]),
    "pa_trajectory_gn_step": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11 + [C.c_double]
                              + [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p]),
    "pa_trajectory_marginals_workspace": (C.c_size_t, [C.c_int, C.c_int]),
    "pa_trajectory_marginals": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11 + [C.c_double]
                                + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]),
    "pa_trajectory_gn_step_prior": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11 + [C.c_double]
                                    + [C.c_void_p] * 6 + [C.c_size_t] + [C.c_void_p] * 3),
    "pa_trajectory_marginals_prior": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11 + [C.c_double]
                                      + [C.c_void_p] * 5 + [C.c_size_t] + [C.c_void_p] * 3),
    # the _prior siblings plus r_cw, isig_cw before lambda (the factor on the angular velocity)
    "pa_trajectory_gn_step_cw": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 13 + [C.c_double]
                                 + [C.c_void_p] * 6 + [C.c_size_t] + [C.c_void_p] * 3),
    "pa_trajectory_marginals_cw": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 13 + [C.c_double]
                                   + [C.c_void_p] * 5 + [C.c_size_t] + [C.c_void_p] * 3),
    "pa_window_marginalize_cw": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 15 + [C.c_double]
                                 + [C.c_void_p] * 13),
    "pa_window_pose_tick_prior": (C.c_int, [C.POINTER(TrajArgs), C.c_void_p, C.c_double] + [C.c_void_p] * 6),
    "pa_window_pose_tick_pre_prior": (C.c_int, [C.POINTER(TrajArgs), C.c_double, C.c_void_p, C.c_size_t]
                                      + [C.c_void_p] * 3),
    "pa_window_pose_tick_reduce_prior": (C.c_int, [C.POINTER(TrajArgs), C.c_double, C.c_void_p, C.c_size_t]
                                         + [C.c_void_p] * 3),
    "pa_window_prior_linearize": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11),
    "pa_window_marginalize": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 13 + [C.c_double]
                              + [C.c_void_p] * 13),
    "pa_window_advance": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_double, C.c_int,
                                                                                     C.c_void_p]),
    "pa_window_advance_n": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_double, C.c_int,
                                                                                       C.c_void_p]),
    "pa_window_advance_t": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 10 + [C.c_double, C.c_int,
                                                                                        C.c_void_p]),
    "pa_window_predict": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8 + [C.c_int] + [C.c_void_p] * 3),
    "pa_keypoint_gate": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_long]
                         + [C.c_void_p] * 5 + [C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_long]
                         + [C.c_void_p] * 4),
    "pa_window_retract": (C.c_int, [C.c_int, C.c_int] + [C.c_void_p] * 6),
    "pa_debug_gn_set_assemblers": (C.c_int, [C.c_int]),
    "pa_window_retract_newest": (C.c_int, [C.c_int, C.c_int] + [C.c_void_p] * 7),
    "pa_debug_gn_set_trace": (C.c_int, [C.c_void_p]),
    "pa_host_device_pointer": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "pa_window_pose_tick": (C.c_int, [C.POINTER(TrajArgs), C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "pa_window_pose_tick_workspace": (C.c_size_t, [C.c_int, C.c_int]),
    "pa_window_pose_tick_pre": (C.c_int, [C.POINTER(TrajArgs), C.c_double, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pa_window_pose_tick_post": (C.c_int, [C.POINTER(TrajArgs), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "pa_loss_statistics_workspace": (C.c_size_t, [C.c_longlong]),
    "pa_loss_statistics": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pa_proj_linearize": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "pa_proj_linearize_robust": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pa_dyn_linearize": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                   C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "pa_dyn_linearize_dt": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "pa_cv_linearize": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    # include/perseus_amd_loader.h (host pointers)
    "pa_png_info": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pa_png_decode": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t]),
    "pa_tiff_info": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pa_tiff_decode_f32": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "pa_load_keypoint_items": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                         C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
}

PREC_FP16 = 0
PREC_FP32 = 1
PREC_FP16X3 = 2
PRECISIONS = {"fp16": PREC_FP16, "fp32": PREC_FP32, "fp16x3": PREC_FP16X3}


def precision_code(name: str) -> int:
    try:
        return PRECISIONS[name]
    except KeyError:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {name!r}") from None

VEL_WORLD = 0
VEL_BODY = 1

ROBUST_NONE = 0
ROBUST_HUBER = 1
ROBUST_CAUCHY = 2
ROBUST = {"huber": ROBUST_HUBER, "cauchy": ROBUST_CAUCHY}


def robust_code(robust) -> tuple:
    """(PA_ROBUST_* kind, k) of a projection noise model's robust part: None (plain), a
    ("huber" | "cauchy", k) pair, or an object with `.kind` and `.k` (smoother.noiseModel.mEstimator)."""
    if robust is None:
        return ROBUST_NONE, 0.0
    kind, k = (robust.kind, robust.k) if hasattr(robust, "kind") else robust
    try:
        return ROBUST[kind], float(k)
    except KeyError:
        raise ValueError(f"robust kind must be one of {sorted(ROBUST)}, got {kind!r}") from None


def lib_path() -> str:
    return _build.LIB


def lib(build_if_missing: bool = True):
    """Load (and on first use, if absent and a compiler exists, build) the library."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # PERSEUS_AMD_LIB_AB: another build of the library, for tools/so_ab.py's interleaved A/B of
    # two builds on one box (measurement tooling only; unset, the in-tree build is the library)
    path = os.environ.get("PERSEUS_AMD_LIB_AB") or _build.LIB
    if not os.path.exists(path) and build_if_missing and path == _build.LIB:
        _build.build()
    if not os.path.exists(path):
        raise PerseusError(f"{path} not found: run `python -m perseus_amd.build`")
    L = C.CDLL(path)
    missing = []
    for name, (res, args) in _SIGS.items():
        if path != _build.LIB and not hasattr(L, name):
            # an older build under A/B lacks the newer entry points (the in-tree library must have all)
            missing.append(name)
            continue
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    if missing:
        import warnings

        warnings.warn(f"{path} (PERSEUS_AMD_LIB_AB) lacks {', '.join(missing)}: calling them raises AttributeError",
                      RuntimeWarning, stacklevel=2)
    _LIB = L
    return L


def check(rc: int, what: str = "") -> int:
    if rc < 0:
        msg = lib().pa_last_error().decode(errors="replace")
        raise PerseusError(f"{what}: {msg} (code {rc})" if what else f"{msg} (code {rc})")
    return rc


def ptr(t) -> int | None:
    """Device pointer of a torch tensor (None for None; an int is taken as a device address)."""
    if t is None or isinstance(t, int):
        return t
    return t.data_ptr()


def stream_of(device) -> int:
    import torch

    return torch.cuda.current_stream(device).cuda_stream
