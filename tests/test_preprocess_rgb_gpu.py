"""GPU: the RGB-only frame path (pa_preprocess_rgb, pa_detector_forward_rgb) against the numpy
oracle of tests/test_preprocess_rgb.py bit for bit, the fused stem source against the
preprocess kernel + f32 forward bit for bit, and the keypoints against the f64 oracle."""
import numpy as np
import pytest
import torch

from oracle import resnet_ref as R
from perseus_amd import _lib, synth
from perseus_amd.detector import KeypointCNN, preprocess_rgb
from test_detector_gpu import FP16_PX_MAX, FP32_PX_MAX, PX
from test_preprocess_rgb import rgb_oracle

pytestmark = pytest.mark.gpu


def _image(seed, B, Hs, Ws):
    return np.random.default_rng(seed).integers(0, 256, (B, Hs, Ws, 3), dtype=np.uint8)


_MODELS = {}


def _model(precision="fp16", in_ch=3):
    key = (precision, in_ch)
    if key not in _MODELS:
        m = KeypointCNN(num_channels=in_ch, precision=precision)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synthetic_state_dict(0, in_ch).items()})
        _MODELS[key] = m.eval()
    return _MODELS[key]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("Hs,Ws,S", [
    (256, 256, 0), (257, 259, 0), (300, 301, 0),  # crop only; 300x301: cropped rows start at odd byte offsets
    (37, 53, 256), (53, 37, 256),                 # the crop spans the short side: src < 0 and i1 = n - 1 clamps
    (300, 400, 460), (720, 1280, 460),
])
def test_preprocess_rgb_equals_oracle_bit_for_bit(Hs, Ws, S, bgr, B):
    u8 = _image(Hs + Ws + B, B, Hs, Ws)
    x = preprocess_rgb(torch.from_numpy(u8).cuda(), bgr=bgr, resize_short=S).cpu().numpy()
    np.testing.assert_array_equal(x, rgb_oracle(u8, bgr, S))


SOURCES = [(300, 301, 0), (300, 400, 460)]


@pytest.mark.parametrize("B", [1, 3, 5, 9, 25])  # one per stem band size
@pytest.mark.parametrize("Hs,Ws,S", SOURCES)
@pytest.mark.parametrize("precision", ["fp16", "fp16x3", "fp32"])
def test_forward_rgb_equals_preprocess_then_forward(precision, Hs, Ws, S, B):
    m = _model(precision)
    rgb = torch.from_numpy(_image(B, B, Hs, Ws)).cuda()
    for bgr in (True, False):
        ref = m(preprocess_rgb(rgb, bgr=bgr, resize_short=S))
        assert torch.equal(m.forward_rgb(rgb, bgr=bgr, resize_short=S), ref)
    assert torch.isfinite(ref).all()


@pytest.mark.parametrize("Hs,Ws,S", SOURCES)
@pytest.mark.parametrize("precision", ["fp16", "fp16x3", "fp32"])
def test_forward_rgb_latency_mode(precision, Hs, Ws, S):
    m = _model(precision)
    rgb = torch.from_numpy(_image(3, 3, Hs, Ws)).cuda()
    m.set_split_k(3)
    try:
        ref = m(preprocess_rgb(rgb, resize_short=S))
        out = torch.empty_like(ref)
        assert m.forward_rgb(rgb, resize_short=S, out=out) is out
        assert torch.equal(out, ref)
    finally:
        m.set_split_k(0)


@pytest.fixture(scope="module")
def oracle_case():
    u8 = _image(77, 3, 300, 400)
    x = rgb_oracle(u8, True, 460)
    return u8, R.run(synth.synthetic_state_dict(0, 3), x, torch.float64)


@pytest.mark.parametrize("precision", ["fp32", "fp16x3", "fp16"])
def test_forward_rgb_against_f64_oracle(oracle_case, precision):
    u8, y64 = oracle_case
    y = _model(precision).forward_rgb(torch.from_numpy(u8).cuda(), bgr=True, resize_short=460).cpu().numpy()
    d = np.abs(y - y64).reshape(3, -1, 2) * PX
    l2 = np.sqrt((d ** 2).sum(-1)).max()
    print(f"forward_rgb {precision}: px-L2 max {l2:.3e}, max |dpx| {d.max():.3e}")
    assert l2 <= (FP16_PX_MAX if precision == "fp16" else FP32_PX_MAX)


def test_forward_real():
    m = _model()
    a = torch.from_numpy(_image(1, 2, 256, 256)).cuda()
    assert torch.equal(m.forward_real(a), m.forward_rgb(a, bgr=False))  # already H x W: no resize
    b = torch.from_numpy(_image(2, 2, 300, 400)).cuda()
    want = m.forward_rgb(b, bgr=False, resize_short=460)  # int(1.8 * 256)
    assert torch.equal(m.forward_real(b), want)
    one = m.forward_real(b[0].cpu().numpy())  # one host image, as the tool passes a decoded PNG
    assert one.device.type == "cpu" and torch.equal(one, want[:1].cpu())


def test_forward_rgb_on_a_four_channel_model_raises():
    rgb = torch.from_numpy(_image(3, 1, 300, 400)).cuda()
    with pytest.raises(_lib.PerseusError, match="needs a 3-channel"):
        _model(in_ch=4).forward_rgb(rgb)
    with pytest.raises(_lib.PerseusError, match="resize_short"):
        _model().forward_rgb(rgb, resize_short=100)
    with pytest.raises(_lib.PerseusError, match="smaller than 256x256"):
        _model().forward_rgb(rgb[:, :200])


@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
def test_reserve_then_capture_forward_rgb(precision):
    """reserve() sizes forward_rgb's f32 staging for 3-channel models too: a graph captured with
    no eager call before it allocates nothing and replays to the eager bits."""
    m = KeypointCNN(num_channels=3, precision=precision)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synthetic_state_dict(0, 3).items()})
    dev = torch.device("cuda", 0)
    rgb = torch.from_numpy(_image(21, 3, 300, 400)).to(dev)
    m.reserve(3, dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        y_graph = m.forward_rgb(rgb, resize_short=460)
    g.replay()
    torch.cuda.synchronize(dev)
    got = y_graph.clone()
    want = m.forward_rgb(rgb, resize_short=460)
    torch.cuda.synchronize(dev)
    assert torch.equal(got, want)
    assert torch.isfinite(got).all()
