"""The RGB-only frame path's arithmetic, pinned on the CPU (no GPU): a numpy oracle that follows
the kernels op by op in f32 (perseus_amd/csrc/rgb_src.h), checked against
torch.nn.functional.interpolate (what kornia's resize calls, validate_real.py:69-71), the
resized-size rule, the validate_real tool's file list and the C ABI's argument checks."""
import ctypes
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

from perseus_amd import _lib
from perseus_amd.detector import real_image_size

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


def _fma(a, b, c):
    """fmaf(a, b, c): the f32 product is exact in f64."""
    return (np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64) + np.asarray(c, f32).astype(f64)).astype(f32)


def _taps(n, m, start, count=256):
    """One axis: destination indices start .. start + count of an axis resized n -> m."""
    scale = f32(n) / f32(m)
    dst = np.arange(start, start + count).astype(f32)
    src = np.maximum(_fma(scale, dst + f32(0.5), f32(-0.5)), f32(0))
    i0 = np.minimum(src.astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = np.clip(src - i0.astype(f32), f32(0), f32(1)).astype(f32)
    return i0, i1, f32(1) - l1, l1


def rgb_oracle(u8, bgr, S):
    """uint8 (B,Hs,Ws,3) -> f32 (B,3,256,256): pa_preprocess_rgb's arithmetic (S = resize_short)."""
    u8 = np.asarray(u8)
    B, Hs, Ws, _ = u8.shape
    if bgr:
        u8 = u8[..., ::-1]
    v = (u8.astype(f32) / f32(255.0)).transpose(0, 3, 1, 2)  # (B,3,Hs,Ws)
    if not S:
        r0, c0 = Hs // 2 - 128, Ws // 2 - 128
        return np.ascontiguousarray(v[:, :, r0:r0 + 256, c0:c0 + 256])
    Hr, Wr = real_image_size(Hs, Ws, S)
    r0, c0 = int(Hr / 2.0 - 128), int(Wr / 2.0 - 128)
    y0, y1, ly0, ly1 = _taps(Hs, Hr, r0)
    x0, x1, lx0, lx1 = _taps(Ws, Wr, c0)
    a, b = v[:, :, y0][..., x0], v[:, :, y0][..., x1]
    c, d = v[:, :, y1][..., x0], v[:, :, y1][..., x1]
    top = _fma(lx0, a, lx1 * b)  # width first
    bot = _fma(lx0, c, lx1 * d)
    ly0, ly1 = ly0[:, None], ly1[:, None]
    return _fma(ly0, top, ly1 * bot)


def _image(seed, B, Hs, Ws):
    return np.random.default_rng(seed).integers(0, 256, (B, Hs, Ws, 3), dtype=np.uint8)


def test_oracle_matches_interpolate():
    """validate_real.py:69-71 (kornia resize = F.interpolate bilinear, align_corners=False, then
    center_crop) against the oracle.  Bound 2^-22: admits an ATen build whose lerps fuse
    differently (1.2-1.8e-7), rejects any wrong index formula (>= 1.7e-6)."""
    for (Hs, Ws), S in (((37, 53), 256), ((53, 37), 256), ((97, 131), 256), ((300, 400), 460), ((1080, 1920), 460)):
        u8 = _image(Hs, 1, Hs, Ws)
        Hr, Wr = real_image_size(Hs, Ws, S)
        img = torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 255.0
        ref = F.interpolate(img, size=(Hr, Wr), mode="bilinear", align_corners=False).numpy()
        r0, c0 = int(Hr / 2.0 - 128), int(Wr / 2.0 - 128)
        ref = ref[:, :, r0:r0 + 256, c0:c0 + 256]
        got = rgb_oracle(u8, False, S)
        assert got.shape == ref.shape == (1, 3, 256, 256) and got.dtype == np.float32
        err = float(np.abs(got.astype(f64) - ref.astype(f64)).max())
        print(f"{Hs}x{Ws} -> {Hr}x{Wr}: max |oracle - interpolate| = {err:.3e}")
        assert err <= 2.0 ** -22


def test_real_image_size():
    assert real_image_size(720, 1280, 460) == (460, 817)
    assert real_image_size(1280, 720, 460) == (817, 460)
    assert real_image_size(200, 200, 460) == (460, 460)
    assert real_image_size(480, 640, 460) == (460, 613)


def test_source_at_the_resized_size_is_the_identity():
    u8 = _image(5, 2, 460, 600)
    assert real_image_size(460, 600, 460) == (460, 600)
    np.testing.assert_array_equal(rgb_oracle(u8, True, 460), (u8[..., ::-1].astype(f32) / f32(255.0))
                                  .transpose(0, 3, 1, 2)[:, :, 102:358, 172:428])


def test_no_resize_is_the_centre_crop():
    u8 = _image(6, 2, 300, 301)
    np.testing.assert_array_equal(rgb_oracle(u8, False, 0),
                                  (u8 / 255.0).astype(f32).transpose(0, 3, 1, 2)[:, :, 22:278, 22:278])


def test_tool_file_filter_and_order(tmp_path):
    """validate_real.py:53-54: the sorted *.png without "segmentation" in the name."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import validate_real
    finally:
        sys.path.pop(0)
    for name in ("b_10.png", "a.png", "b_2.png", "a_segmentation.png", "segmentation_3.png", "notes.txt", "c.jpg"):
        (tmp_path / name).write_bytes(b"")
    assert [os.path.basename(p) for p in validate_real.image_files(str(tmp_path))] == ["a.png", "b_10.png", "b_2.png"]


def test_bad_arguments_return_einval_without_touching_the_gpu():
    L = _lib.lib()
    p = ctypes.c_void_p(8)  # (never dereferenced: every case fails before a launch)

    def pre(rgb, Hs, Ws, S, x=p, H=256, W=256):
        return L.pa_preprocess_rgb(rgb, 1, Hs, Ws, 1, S, H, W, x, None)

    for S in (1, 100, 255, -1, -460):
        assert pre(p, 300, 400, S) == -1 and b"resize_short" in L.pa_last_error()
    assert pre(p, 255, 400, 0) == -1 and b"smaller than 256x256" in L.pa_last_error()
    assert pre(p, 400, 200, 0) == -1 and b"smaller than 256x256" in L.pa_last_error()
    assert pre(None, 300, 400, 0) == -1 and b"null" in L.pa_last_error()
    assert pre(p, 300, 400, 0, x=None) == -1 and b"null" in L.pa_last_error()
    assert pre(p, 300, 400, 0, H=128, W=128) == -1 and b"256x256" in L.pa_last_error()
    assert pre(p, 0, 400, 460) == -1
    assert L.pa_preprocess_rgb(p, -1, 300, 400, 1, 0, 256, 256, p, None) == -1
    assert L.pa_preprocess_rgb(None, 0, 300, 400, 1, 0, 256, 256, None, None) == 0  # B = 0: a no-op
    assert L.pa_detector_forward_rgb(None, p, 1, 300, 400, 1, 0, p, None) == -1 and b"null detector" in L.pa_last_error()
    assert L.pa_detector_forward_rgb_px(None, p, 1, 300, 400, 1, 0, p, None, None) == -1
    assert L.pa_detector_forward_rgb_px(None, p, 1, 300, 400, 1, 0, p, p, None) == -1
