"""The RGB streaming tick (a 3-channel model, scripts/streaming.py:104,112-128 feeding
frame[:C]): graph replay == eager, the reference's frame arithmetic, zero-copy == copying, and
the arguments an RGB pipeline ignores or refuses."""
import numpy as np
import pytest
import torch

from oracle import resnet_ref as R
from perseus_amd import synth
from perseus_amd.detector import KeypointCNN
from perseus_amd.streaming import StreamingPipeline

pytestmark = pytest.mark.gpu


def _load(precision="fp16", in_ch=3):
    m = KeypointCNN(num_channels=in_ch, precision=precision)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synthetic_state_dict(0, in_ch).items()})
    return m


@pytest.fixture(scope="module")
def model():
    return _load()


def _frames(seed, n=3, Hs=720, Ws=1280):
    return np.random.default_rng(seed).integers(0, 256, (n, Hs, Ws, 3), dtype=np.uint8)


@pytest.mark.parametrize("host_crop", [True, False])
def test_graph_matches_eager(model, host_crop):
    g = StreamingPipeline(model, host_crop=host_crop, graph=True)
    e = StreamingPipeline(model, host_crop=host_crop, graph=False)
    assert g.rgb_only and g.depth_h is None and g.in_h.numel() == g.rgb_h.numel()  # RGB-only staging
    for seed in (1, 2):
        rgb = _frames(seed)
        out = g(rgb)
        np.testing.assert_array_equal(out, e(rgb))
        assert np.isfinite(out).all()
    g.close()
    e.close()


def test_matches_reference_frame_arithmetic(model):
    rgb = _frames(3)
    pipe = StreamingPipeline(model)
    out = pipe(rgb)
    pipe.close()
    model.set_split_k(3)  # the pipeline's latency mode: same kernels, same bits
    try:
        y_rgb = model.forward_rgb(torch.as_tensor(rgb).cuda(), bgr=True)
        # streaming.py:68-69 (BGR -> RGB, / 255 in f64) and :79-80 (centre crop), then the model
        x = np.stack([(f[..., ::-1] / 255.0)[360 - 128:360 + 128, 640 - 128:640 + 128] for f in rgb])
        y = model(torch.from_numpy(x).permute(0, 3, 1, 2).float().cuda())
    finally:
        model.set_split_k(0)
    np.testing.assert_array_equal(out, R.denormalize_f32(y_rgb.cpu().numpy()).reshape(3, -1, 2))
    np.testing.assert_array_equal(out, R.denormalize_f32(y.cpu().numpy()).reshape(3, -1, 2))


@pytest.mark.parametrize("precision", ["fp16", "fp16x3"])
def test_zero_copy_tick_matches_copying_tick(model, precision):
    m = model if precision == "fp16" else _load(precision)
    a = StreamingPipeline(m, n_cams=3, graph=True, zero_copy=False, pose_window=6)
    b = StreamingPipeline(m, n_cams=3, graph=True, zero_copy=True, pose_window=6)
    assert b.zero_copy and not a.zero_copy
    for seed in range(3):
        rgb = _frames(40 + seed)
        for x, y in zip(a.tick(rgb), b.tick(rgb)):
            np.testing.assert_array_equal(x, y)
    a.close()
    b.close()


def test_depth_argument_is_ignored(model):
    rgb = _frames(5)
    pipe = StreamingPipeline(model)
    ref = pipe(rgb)
    depth = np.full((3, 720, 1280), np.nan, np.float32)
    np.testing.assert_array_equal(pipe(rgb, depth), ref)
    pipe.stage(rgb, depth=None)
    np.testing.assert_array_equal(pipe.run(), ref)
    pipe.close()


def test_near_far_need_a_depth_channel(model):
    with pytest.raises(ValueError):
        StreamingPipeline(model, near=0.1)
    with pytest.raises(ValueError):
        StreamingPipeline(model, far=0.5)


def test_two_channel_model_is_refused():
    with pytest.raises(ValueError):
        StreamingPipeline(_load(in_ch=2))
