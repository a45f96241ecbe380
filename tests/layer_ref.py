"""TEST HELPER (not a test): f64 reference of ONE launch of the detector's forward, with a
per-element error bound (tests/test_detector_layers_gpu.py feeds it the maps that
KeypointCNN.tap copies out of a real forward; tests/test_layer_ref.py shows on the CPU what
the two checks catch).

A launch is an optional convolution with BatchNorm folded (+ bias, + residual, ReLU), an optional
3x3 s2 p1 max pool behind it and an optional head (mean over H x W, then the fc) -- a plain
restatement in torch f64 on the CPU, not a port of the kernels.

Folded weights (`fold`): as the library's build() folds them -- scale = g / sqrt(var + 1e-5) in
f64, w * scale rounded to f32, bias = (float)(b - mu * scale); fp16 mode rounds the f32 weight to
fp16 (bit for bit the library's), fp32 and fp16x3 use the f32 weight (fp16x3's hi / lo split of
w 2^e represents it to 2^-22 relative: in the bound).

Rigorous check: |gpu - ref| <= bound for every element, ref the f64 value itself: the bound's store
term is the one rounding of the GPU's value on its way to memory.  (Against a ref rounded to the
storage format the same bound is not a bound: a sum that is off by far less than a storage ulp can
round to the neighbouring fp16 value, one whole ulp = up to 2^-10 |ref| from the rounded ref; torch's
CPU f32 conv2d of the same fp16 inputs exceeds it by 1.86 x on the layer2 downsample, K = 64.)
With S = conv(|in|, |w|) + |bias| + |res|, K accumulated terms and u = 2^-23 (one f32 ulp: covers an
accumulator that truncates):
    fp16     (K + 2) u S + 2^-11 |ref| + 2^-25         (store rounding, subnormal floor)
    fp32     (K + 2) u S + 2^-24 |ref|
    fp16x3   (3K + 2) u S + 2 2^-22 S + 2^-22 |ref| + 2^-25   (dropped x_lo w_lo, weight split)
    max pool the max of the window's bounds;  head: the same with K = H W + C and an f32 store
    (the keypoints are f32 in every mode; fp16x3: one more u S for hi + lo added in f32)

Statistical check: q = |gpu - ref| / (sqrt(K) 2^-24 sqrt(conv(in^2, w^2)) + store term), its maximum
per frame.  A round-to-nearest f32 sum of K terms has an error of that order whatever the order of
summation; a missing or misplaced product has not.  The yardstick is torch's CPU f32 conv2d run on
the same inputs (`cpu_f32`, q_cpu): the GPU's q may be at most Q_FACTOR x the largest q_cpu of the
launch shape (Q_CPU below; the kernels sum in blocked orders and three product groups, which changes
the constant and not the sqrt(K) growth).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

MODES = ("fp16", "fp32", "fp16x3")
U_ACC = 2.0 ** -23
Q_FACTOR = 4.0

# Largest per-frame q of the same launch in torch's CPU f32 arithmetic (cpu_f32 below: inputs, weights
# and the stored result in the mode's formats, f32 conv2d / mean + linear between) on the f64 oracle's
# own activations of synthetic_frames(6, 3), 4-channel model seed 0 and 3-channel model seed 2, per mode
# and launch shape (ks, stride, Cin, Cout, residual, head); a max pool behind the conv does not change
# the key.  The 1- and 2-channel stems and the heads of another width than 16: from the stem and the head
# of SHAPE_MODELS (below) on the first in_ch channels of the same frames.  Measured with measure_q_cpu() (python tests/layer_ref.py prints this table).  fp16's rows sit at 1: the storage rounding alone is
# up to half an fp16 ulp = q 1.  The GPU's q is held to Q_FACTOR x these.
Q_CPU = {
    "fp16": {
        (7, 2, 4, 64, False, False): 0.999,
        (3, 1, 64, 64, False, False): 0.997,
        (3, 1, 64, 64, True, False): 0.999,
        (3, 2, 64, 128, False, False): 0.993,
        (1, 2, 64, 128, False, False): 0.998,
        (3, 1, 128, 128, True, False): 0.998,
        (3, 1, 128, 128, False, False): 0.995,
        (3, 2, 128, 256, False, False): 0.995,
        (1, 2, 128, 256, False, False): 0.996,
        (3, 1, 256, 256, True, False): 0.998,
        (3, 1, 256, 256, False, False): 0.994,
        (3, 2, 256, 512, False, False): 0.992,
        (1, 2, 256, 512, False, False): 0.997,
        (3, 1, 512, 512, True, False): 0.994,
        (3, 1, 512, 512, False, False): 0.985,
        (1, 1, 512, 16, False, True): 1.324,
        (7, 2, 3, 64, False, False): 0.998,
        (7, 2, 1, 64, False, False): 0.997,
        (1, 1, 512, 2, False, True): 0.794,
        (7, 2, 2, 64, False, False): 0.997,
        (1, 1, 512, 32, False, True): 1.398,
        (1, 1, 512, 10, False, True): 1.296,
        (1, 1, 512, 26, False, True): 1.207,
    },
    "fp32": {
        (7, 2, 4, 64, False, False): 2.558,
        (3, 1, 64, 64, False, False): 1.063,
        (3, 1, 64, 64, True, False): 0.893,
        (3, 2, 64, 128, False, False): 1.019,
        (1, 2, 64, 128, False, False): 2.252,
        (3, 1, 128, 128, True, False): 0.682,
        (3, 1, 128, 128, False, False): 0.584,
        (3, 2, 128, 256, False, False): 0.488,
        (1, 2, 128, 256, False, False): 2.263,
        (3, 1, 256, 256, True, False): 0.903,
        (3, 1, 256, 256, False, False): 0.641,
        (3, 2, 256, 512, False, False): 0.388,
        (1, 2, 256, 512, False, False): 4.712,
        (3, 1, 512, 512, True, False): 0.863,
        (3, 1, 512, 512, False, False): 0.623,
        (1, 1, 512, 16, False, True): 1.792,
        (7, 2, 3, 64, False, False): 3.158,
        (7, 2, 1, 64, False, False): 2.457,
        (1, 1, 512, 2, False, True): 0.465,
        (7, 2, 2, 64, False, False): 2.506,
        (1, 1, 512, 32, False, True): 1.797,
        (1, 1, 512, 10, False, True): 1.042,
        (1, 1, 512, 26, False, True): 1.088,
    },
    "fp16x3": {
        (7, 2, 4, 64, False, False): 1.930,
        (3, 1, 64, 64, False, False): 1.060,
        (3, 1, 64, 64, True, False): 0.820,
        (3, 2, 64, 128, False, False): 0.938,
        (1, 2, 64, 128, False, False): 1.400,
        (3, 1, 128, 128, True, False): 0.673,
        (3, 1, 128, 128, False, False): 0.564,
        (3, 2, 128, 256, False, False): 0.505,
        (1, 2, 128, 256, False, False): 1.304,
        (3, 1, 256, 256, True, False): 0.694,
        (3, 1, 256, 256, False, False): 0.510,
        (3, 2, 256, 512, False, False): 0.465,
        (1, 2, 256, 512, False, False): 1.997,
        (3, 1, 512, 512, True, False): 0.691,
        (3, 1, 512, 512, False, False): 0.539,
        (1, 1, 512, 16, False, True): 1.932,
        (7, 2, 3, 64, False, False): 1.709,
        (7, 2, 1, 64, False, False): 1.380,
        (1, 1, 512, 2, False, True): 0.866,
        (7, 2, 2, 64, False, False): 1.532,
        (1, 1, 512, 32, False, True): 1.394,
        (1, 1, 512, 10, False, True): 1.932,
        (1, 1, 512, 26, False, True): 1.813,
    },
}


def shape_key(ks, stride, cin, cout, residual=False, head=False):
    return (int(ks), int(stride), int(cin), int(cout), bool(residual), bool(head))


# ------------------------------------------------------------------------------ number formats
def _np(v):
    return v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def split_x3(v):
    """fp16x3's (hi, lo) pair of f32 values, as f64 hi + lo: hi = fp16(v), lo = fp16(v - hi)."""
    v32 = _np(v).astype(np.float32)
    hi = v32.astype(np.float16)
    lo = (v32 - hi.astype(np.float32)).astype(np.float16)
    return torch.from_numpy(hi.astype(np.float64) + lo.astype(np.float64))


def store(v, mode):
    """f64 values rounded to the mode's activation storage (numpy rounds f64 -> fp16 once)."""
    if mode == "fp16":
        return torch.from_numpy(_np(v).astype(np.float16).astype(np.float64))
    if mode == "fp32":
        return torch.from_numpy(_np(v).astype(np.float32).astype(np.float64))
    return split_x3(v)


def store_term(ref, mode):
    a = ref.abs()
    if mode == "fp16":
        return 2.0 ** -11 * a + 2.0 ** -25
    if mode == "fp32":
        return 2.0 ** -24 * a
    return 2.0 ** -22 * a + 2.0 ** -25


def stem_input(x, mode):
    """The stem's input as its kernel converts the f32 frame: fp16 rounds it, fp16x3 splits it."""
    x = torch.as_tensor(_np(x).astype(np.float32))
    if mode == "fp16":
        return torch.from_numpy(x.numpy().astype(np.float16).astype(np.float64))
    if mode == "fp16x3":
        return split_x3(x)
    return x.double()


def fold(state, keys, mode):
    """(w (Cout, Cin, ks, ks), bias (Cout)) in f64 of conv `keys` = (conv prefix, bn prefix)."""
    ck, bk = keys
    w = np.asarray(state[ck + ".weight"], np.float64)
    g, b, mu, var = (np.asarray(state[f"{bk}.{n}"], np.float64) for n in ("weight", "bias", "running_mean", "running_var"))
    scale = g / np.sqrt(var + 1e-5)
    w32 = (w * scale[:, None, None, None]).astype(np.float32)
    bias = (b - mu * scale).astype(np.float32)
    if mode == "fp16":
        w32 = w32.astype(np.float16)
    return torch.from_numpy(w32.astype(np.float64)), torch.from_numpy(bias.astype(np.float64))


# ------------------------------------------------------------------------------ one launch
class Ref:
    """ref (the exact f64 value), bound and q's denominator of one output map of a launch."""

    def __init__(self, ref, bound, den, K, exact=False):
        self.ref, self.bound, self.den, self.K, self.exact = ref, bound, den, K, exact


def _acc_bound(S, K, mode):
    if mode == "fp16x3":
        return (3 * K + 2) * U_ACC * S + 2 * 2.0 ** -22 * S
    return (K + 2) * U_ACC * S


def conv_launch(mode, x, w, b, res=None, relu=True, stride=1, maxpool=False, _raw=False):
    """Reference of conv(x, w) + b (+ res) (ReLU) (max pool) from the launch's true inputs (f64)."""
    ks = w.shape[-1]
    pad = ks // 2
    K = w.shape[1] * ks * ks
    bb = b.view(1, -1, 1, 1)
    with torch.no_grad():
        pre = F.conv2d(x, w, stride=stride, padding=pad) + bb
        S = F.conv2d(x.abs(), w.abs(), stride=stride, padding=pad) + bb.abs()
        V = F.conv2d((x * x).float(), (w * w).float(), stride=stride, padding=pad).double()
        if res is not None:
            pre = pre + res
            S = S + res.abs()
        exact = F.relu(pre) if relu else pre
        if _raw:
            return exact, S, V, K
        ref = exact
        bound = _acc_bound(S, K, mode) + store_term(ref, mode)
        den = np.sqrt(K) * 2.0 ** -24 * V.sqrt() + store_term(ref, mode)
        if maxpool:
            ref, bound, den = (F.max_pool2d(t, 3, 2, 1) for t in (ref, bound, den))
    return Ref(ref, bound, den, K)


def maxpool_launch(x):
    """The max pool alone (fp32 mode): exact."""
    ref = F.max_pool2d(x, 3, 2, 1)
    return Ref(ref, torch.zeros_like(ref), torch.zeros_like(ref), 0, exact=True)


def head_launch(mode, x, fcw, fcb, in_bound=None):
    """Reference of fc(mean over H x W of x) -> (B, 2K) f32.  in_bound: a bound on |x - true x| per
    element, carried through (the head fused behind a conv)."""
    B, C, H, W = x.shape
    K = H * W + C
    fcw, fcb = torch.as_tensor(fcw, dtype=torch.float64), torch.as_tensor(fcb, dtype=torch.float64)
    with torch.no_grad():
        exact = x.mean((2, 3)) @ fcw.T + fcb
        S = x.abs().mean((2, 3)) @ fcw.abs().T + fcb.abs()
        V = ((x * x).sum((2, 3)) / (H * W) ** 2) @ (fcw * fcw).T
        ref = exact
        bound = (K + 2 + (mode == "fp16x3")) * U_ACC * S + store_term(ref, "fp32")
        if in_bound is not None:
            bound = bound + in_bound.mean((2, 3)) @ fcw.abs().T
        den = np.sqrt(K) * 2.0 ** -24 * V.sqrt() + store_term(ref, "fp32")
    return Ref(ref, bound, den, K)


def launch_refs(info, state, mode):
    """{"out": Ref, "out2": Ref} of a tapped launch (KeypointCNN.tap's dict) from its own inputs."""
    m = info["maps"]
    out = {}
    if info["conv"] is None and info["maxpool"]:
        out["out"] = maxpool_launch(m["in"])
    elif info["conv"] is None:
        out["out"] = head_launch(mode, m["in"], state["resnet.fc.weight"], state["resnet.fc.bias"])
    else:
        x = stem_input(m["in"], mode) if info["ks"] == 7 else m["in"]
        w, b = fold(state, info["conv"], mode)
        res = m["res"] if info["residual"] else None
        r = conv_launch(mode, x, w, b, res, info["relu"], info["stride"], info["maxpool"])
        if info["head"]:  # the head fused behind the conv: y from the conv's rounded output
            r = head_launch(mode, r.ref, state["resnet.fc.weight"], state["resnet.fc.bias"], in_bound=r.bound)
            r.den = None  # (rigorous check only)
        out["out"] = r
        if info["conv2"] is not None:
            w2, b2 = fold(state, info["conv2"], mode)
            out["out2"] = conv_launch(mode, x, w2, b2, None, False, info["stride"])
    return out


# ------------------------------------------------------------------------------ the checks
def check(gpu, r):
    """(ok, worst |err| / bound, index of the worst element, per-frame max q) of a map against its Ref.
    ok: every element within its bound (an exact launch: equal).  Elements with err = 0 count as
    ratio 0 (bound and denominator may be 0 there)."""
    gpu = torch.as_tensor(gpu, dtype=torch.float64)
    assert gpu.shape == r.ref.shape, (gpu.shape, r.ref.shape)
    err = (gpu - r.ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    if r.exact:
        ratio = torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))
    else:
        ratio = torch.where(err > 0, err / r.bound, torch.zeros_like(err))
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
    ok = bool((err <= r.bound).all())
    if r.exact or r.den is None:
        q = torch.zeros(gpu.shape[0], dtype=torch.float64)
    else:
        q = torch.where(err > 0, err / r.den, torch.zeros_like(err)).flatten(1).max(1).values
    return ok, float(ratio.flatten()[worst]), idx, q


def q_cap(mode, key):
    """The largest q a GPU launch of this shape may show: Q_FACTOR x the CPU f32 yardstick.  A head
    of another width than 16 has as few as 2 outputs per frame, a thin sample of q: its yardstick is
    the mode's largest head row over all measured widths (K = 64 + 512 whatever the width)."""
    if key[5] and key[3] != 16:
        return Q_FACTOR * max(v for k, v in Q_CPU[mode].items() if k[5])
    return Q_FACTOR * Q_CPU[mode][key]


def tap_keys(info):
    """Shape keys of a tapped launch's outputs: {"out": key, "out2": key}."""
    if info["conv"] is None:
        return {"out": shape_key(1, 1, info["Cin"], info["Cout"], head=True)} if info["head"] else {}
    keys = {"out": shape_key(info["ks"], info["stride"], info["Cin"], info["Cout"], info["residual"])}
    if info["conv2"] is not None:
        keys["out2"] = shape_key(1, info["stride"], info["Cin"], info["Cout"])
    return keys


# ------------------------------------------------------------------------------ the f64 oracle's launches
def oracle_launches(state, x):
    """The forward of oracle.resnet_ref restated launch by launch in f64 (exact, nothing rounded):
    a list of dicts {name, keys, keys2, x, res, relu, stride, maxpool, head} with each launch's
    true f64 inputs -- the stand-in activations of test_layer_ref.py and of measure_q_cpu."""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    L = []

    def run(name, keys, xin, res=None, relu=True, stride=1, maxpool=False, keys2=None):
        L.append(dict(name=name, keys=keys, keys2=keys2, x=xin, res=res, relu=relu, stride=stride, maxpool=maxpool,
                      head=False))
        w, b = fold(state, keys, "fp32")
        out = conv_launch("fp32", xin, w, b, res, relu, stride, _raw=True)[0]
        return F.max_pool2d(out, 3, 2, 1) if maxpool else out

    h = run("stem", ("resnet.conv1", "resnet.bn1"), x, stride=2, maxpool=True)
    for li in range(1, 5):
        for bi in range(2):
            p = f"resnet.layer{li}.{bi}"
            if li > 1 and bi == 0:
                ds = (p + ".downsample.0", p + ".downsample.1")
                o = run(f"layer{li}.{bi}.conv1+ds", (p + ".conv1", p + ".bn1"), h, stride=2, keys2=ds)
                w2, b2 = fold(state, ds, "fp32")
                idn = conv_launch("fp32", h, w2, b2, None, False, 2, _raw=True)[0]
            else:
                o = run(f"layer{li}.{bi}.conv1", (p + ".conv1", p + ".bn1"), h)
                idn = h
            h = run(f"layer{li}.{bi}.conv2", (p + ".conv2", p + ".bn2"), o, res=idn)
    L.append(dict(name="head", keys=None, keys2=None, x=h, res=None, relu=False, stride=1, maxpool=False, head=True))
    return L


def cpu_f32(l, state, mode):
    """The same launch in torch's CPU f32 arithmetic: launch l's inputs and the folded weights in the
    mode's formats (all exact in f32), f32 conv2d / mean + linear, the result stored in the mode's
    format: {"out": map, "out2": map}."""
    x = (stem_input(l["x"], mode) if l["name"] == "stem" else store(l["x"], mode)).float()
    with torch.no_grad():
        if l["head"]:
            fw = torch.as_tensor(np.asarray(state["resnet.fc.weight"], np.float32))
            fb = torch.as_tensor(np.asarray(state["resnet.fc.bias"], np.float32))
            return {"out": F.linear(x.mean((2, 3)), fw, fb).double()}
        out = {}
        for o, keys, res, relu, mp in (("out", l["keys"], l["res"], l["relu"], l["maxpool"]),
                                       ("out2", l["keys2"], None, False, False)):
            if keys is None:
                continue
            w, b = fold(state, keys, mode)
            v = F.conv2d(x, w.float(), b.float(), stride=l["stride"], padding=w.shape[-1] // 2)
            if res is not None:
                v = v + store(res, mode).float()
            v = F.relu(v) if relu else v
            out[o] = store((F.max_pool2d(v, 3, 2, 1) if mp else v).double(), mode)
        return out


def fmaf_chain_f32(l, state, block=32, blocked=True):
    """Launch l's conv (3x3, fp32 mode) as sequential f32 fmaf chains in the fp32 kernels' order
    (channel blocks of `block`, the 9 taps of a block, the block's channels): what a chain of
    dependent v_mfma_f32_16x16x4_f32 computes.  blocked (the kernels' form): one chain per channel
    block and the block sums added up in f32; else ONE chain over the whole K (their form before the
    single-launch checks).  The product and the add are done in f64 and rounded to f32 once per term
    (a 48-bit product is exact in f64)."""
    x = store(l["x"], "fp32").float()
    w, b = fold(state, l["keys"], "fp32")
    cout, cin = w.shape[:2]
    cols = F.unfold(x, 3, padding=1, stride=l["stride"]).numpy()  # (B, cin * 9, L), rows (ci, tap)
    idx = np.arange(cin * 9).reshape(cin, 9)
    order = np.concatenate([idx[c:c + block, t] for c in range(0, cin, block) for t in range(9)])
    wm = w.numpy().reshape(cout, cin * 9)
    acc = np.zeros((x.shape[0], cout, cols.shape[2]), np.float32)
    tot = np.zeros_like(acc)
    for i, k in enumerate(order):
        acc = (acc.astype(np.float64) + wm[None, :, k, None] * cols[:, None, k, :].astype(np.float64)).astype(np.float32)
        if blocked and (i + 1) % (9 * block) == 0:
            tot, acc = tot + acc, np.zeros_like(acc)
    acc = tot + acc
    acc = acc + b.numpy().astype(np.float32)[None, :, None]
    if l["res"] is not None:
        acc = acc + store(l["res"], "fp32").numpy().astype(np.float32).reshape(acc.shape)
    acc = np.maximum(acc, 0) if l["relu"] else acc
    ho = (x.shape[2] - 1) // l["stride"] + 1
    return torch.from_numpy(acc.astype(np.float64).reshape(x.shape[0], cout, ho, -1))


def oracle_refs(l, state, mode):
    """launch_refs for an oracle launch (inputs rounded to the mode's storage first, as a real
    launch's inputs are): ({"out": Ref, "out2": Ref}, {"out": key, "out2": key})."""
    x = stem_input(l["x"], mode) if l["name"] == "stem" else store(l["x"], mode)
    if l["head"]:
        return ({"out": head_launch(mode, x, state["resnet.fc.weight"], state["resnet.fc.bias"])},
                {"out": shape_key(1, 1, x.shape[1], np.asarray(state["resnet.fc.weight"]).shape[0], head=True)})
    res = None if l["res"] is None else store(l["res"], mode)
    w, b = fold(state, l["keys"], mode)
    refs = {"out": conv_launch(mode, x, w, b, res, l["relu"], l["stride"], l["maxpool"])}
    keys = {"out": shape_key(w.shape[-1], l["stride"], w.shape[1], w.shape[0], res is not None)}
    if l["keys2"] is not None:
        w2, b2 = fold(state, l["keys2"], mode)
        refs["out2"] = conv_launch(mode, x, w2, b2, None, False, l["stride"])
        keys["out2"] = shape_key(1, l["stride"], w2.shape[1], w2.shape[0])
    return refs, keys


# (seed, in_ch, n_kp) of the models whose stem and head alone are measured: the channel and keypoint
# counts between the library's limits (tests/test_detector_shapes_gpu.py runs them on the GPU)
SHAPE_MODELS = ((0, 1, 1), (1, 2, 16), (2, 3, 5), (3, 4, 13))


def measure_q_cpu(B=3):
    """{mode: {shape key: largest per-frame q of cpu_f32}} over every launch of the oracle's forward
    (the 4-channel model, seed 0, and the 3-channel one, seed 2, on synthetic_frames(6, B)), then the
    stem and the head of SHAPE_MODELS for the keys those two do not have (the 1- and 2-channel stems,
    the heads of 2, 10, 26 and 32 outputs; a key of the first two models keeps their row); also prints
    the largest |err| / bound of cpu_f32 per mode."""
    from perseus_amd import synth

    table = {m: {} for m in MODES}
    worst = {m: 0.0 for m in MODES}
    base = set()
    for seed, in_ch, n_kp in ((0, 4, 8), (2, 3, 8)) + SHAPE_MODELS:
        extra = (seed, in_ch, n_kp) in SHAPE_MODELS
        state = synth.synthetic_state_dict(seed, in_ch, n_kp)
        x = synth.synthetic_frames(6, B)[:, :in_ch].copy()
        for l in oracle_launches(state, x):
            if extra and not (l["name"] == "stem" or l["head"]):
                continue
            for mode in MODES:
                refs, keys = oracle_refs(l, state, mode)
                got = cpu_f32(l, state, mode)
                for o, r in refs.items():
                    ok, ratio, _, q = check(got[o], r)
                    worst[mode] = max(worst[mode], ratio)
                    if extra:
                        print(f"model {(seed, in_ch, n_kp)} {mode} {l['name']}: |err|/bound {ratio:.3f} q "
                              f"{float(q.max()):.3f} non-zero {float((got[o] != 0).double().mean()):.2f}")
                        if keys[o] in base:
                            continue
                    else:
                        base.add(keys[o])
                    table[mode][keys[o]] = max(table[mode].get(keys[o], 0.0), float(q.max()))
    print("largest |err| / bound of the CPU f32 launches:", worst)
    return table


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for m, t in measure_q_cpu().items():
        print(f'    "{m}": {{')
        for k, v in t.items():
            print(f"        {k}: {v:.3f},")
        print("    },")
