"""pa_trajectory_linearize (traj_all_kernel) at the shapes where its work split changes: factor
counts on both sides of a 64-factor wave and a 256-factor projection unit, a trajectory boundary
inside a dynamics block, odd unit counts.  Every element of every output against the f64 oracle;
every output inside a larger allocation whose padding must stay untouched (canaries); each
optional output NULL in turn and all Jacobians NULL (the error-only path), outputs on an 8-byte
(not 16-byte) boundary (wave_flush's scalar path and odd tail) and nvalid masks, each bit for bit
against the all-outputs launch."""
import numpy as np
import pytest
import torch

from oracle import factors_ref as F
from oracle import resnet_ref as R
from perseus_amd import _lib, pipeline

pytestmark = pytest.mark.gpu
ATOL = 1e-9
KCAL = np.array([280.0, 280.0, 0.0, 128.0, 128.0])
DT = 1.0 / 12.0
PAD = 64
SENT64 = 0x7FF4DEADBEEF5A5A  # a NaN payload no kernel produces
SENT32 = 0x5A5A5A5A
# (T, L, K, velocity frame): dynamics / projection factor counts in the comments
SHAPES = [(1, 2, 1, "world"),    # 1 / 2: smallest
          (16, 5, 8, "world"),   # 64 / 640: one exact dynamics wave; two projection units and a half
          (13, 6, 5, "body"),    # 65 / 390: a full wave plus a tail of 1
          (9, 8, 9, "world"),    # 63 / 648: just under a full wave
          (2, 33, 4, "body"),    # 64 / 264: a trajectory boundary inside a block, L > 24
          (3, 44, 3, "world"),   # 129 / 396: two full waves plus a tail of 1
          (64, 2, 16, "world")]  # 64 / 2048: eight exact projection units, odd unit count
UNALIGNED = [(13, 6, 5), (16, 5, 8)]
SP, SD, SC = np.array([2.0, 3.0]), np.array([0.1, 0.2, 0.05, 0.3, 0.15, 0.25]), np.array([0.5, 0.25, 1.0])

# per-factor elements of each output (0: per projection factor, 1: per dynamics / const-vel factor)
WIDTH = {"r_proj": (0, 2), "j_proj": (0, 12), "err_proj": (0, 1), "status": (0, 1), "r_dyn": (1, 6),
         "j_dyn0": (1, 36), "j_dyn1": (1, 18), "j_dyn2": (1, 18), "j_dyn3": (1, 36), "err_dyn": (1, 1),
         "r_cv": (1, 3), "j_cv0": (1, 9), "j_cv1": (1, 9), "err_cv": (1, 1)}
JACS = ("j_proj", "j_dyn0", "j_dyn1", "j_dyn2", "j_dyn3", "j_cv0", "j_cv1")
OPTIONAL = JACS + ("err_proj", "err_dyn", "err_cv", "status")


def _problem(T, L, nk, seed):
    rng = np.random.default_rng(seed)
    Fn = T * L
    behind = min(5, Fn - 1)
    poses = np.zeros((Fn, 12))
    for f in range(Fn):
        Rm, _ = F.pose_exp(np.concatenate([0.4 * rng.standard_normal(3), np.zeros(3)]))
        t = np.array([0.05 * rng.standard_normal(), 0.05 * rng.standard_normal(), 0.3 + 0.2 * rng.random()])
        if f == behind:
            t[2] = -0.3  # every corner behind the camera: cheirality
        poses[f] = F.pack((Rm, t))
    corners = 0.0175 * rng.choice([-1.0, 1.0], (nk, 3)) * rng.uniform(0.5, 1.0, (nk, 3))
    return dict(poses=poses, vels=rng.standard_normal((Fn, 3)), angvels=rng.standard_normal((Fn, 3)),
                y=rng.uniform(-1, 1, (Fn, 2 * nk)).astype(np.float32), corners=corners, behind=behind)


def _oracle(p, T, L, nk, vf):
    """Unwhitened reference in the device's layout (Jacobians column-major per factor)."""
    z = R.denormalize_f32(p["y"], 256, 256).astype(np.float64).reshape(-1, 2)
    rp, Jp, st = F.projection_batch(np.repeat(p["poses"], nk, axis=0), np.tile(p["corners"], (T * L, 1)), z, KCAL)
    idx = np.array([t * L + l for t in range(T) for l in range(L - 1)], dtype=np.int64)
    rd, J0, J1, J2, J3 = F.dynamics_batch(p["poses"][idx], p["angvels"][idx], p["vels"][idx], p["poses"][idx + 1],
                                          DT, vf)
    m = len(idx)
    eye = np.broadcast_to(np.eye(3), (m, 3, 3))
    ref = dict(r_proj=rp, j_proj=Jp, status=st, r_dyn=rd, j_dyn0=J0, j_dyn1=J1, j_dyn2=J2, j_dyn3=J3,
               r_cv=p["vels"][idx + 1] - p["vels"][idx], j_cv0=-eye, j_cv1=eye)
    return {k: (np.ascontiguousarray(v.transpose(0, 2, 1)) if k in JACS else v) for k, v in ref.items()}


class Problem:
    """One shape: inputs staged once per whitening, the oracle computed once."""

    def __init__(self, T, L, nk, vf):
        self.T, self.L, self.nk, self.vf = T, L, nk, vf
        self.p = _problem(T, L, nk, seed=100 * T + L)
        self.ref = _oracle(self.p, T, L, nk, vf)
        self.count = (T * L * nk, T * (L - 1))
        self.staged = {}

    def args(self, whiten, nvalid=None):
        key = (whiten, None if nvalid is None else tuple(nvalid.tolist()))
        if key not in self.staged:
            p = self.p
            sig = dict(proj_sigmas=SP, dyn_sigmas=SD, cv_sigmas=SC) if whiten else {}
            self.staged[key] = pipeline.prepare_trajectories(
                torch.as_tensor(p["y"], device="cuda"), p["poses"], p["vels"], p["angvels"], p["corners"], KCAL,
                T=self.T, L=self.L, dt=DT, vel_frame=self.vf, nvalid=nvalid, **sig)
        return self.staged[key][0]

    def launch(self, whiten=True, null=(), shift=(), nvalid=None):
        """Launch into fresh sentinel-filled allocations; outputs in `null` get a NULL pointer, those
        in `shift` start 8 bytes later.  Checks the canaries; returns {name: flat tensor}."""
        a = _lib.TrajArgs.from_buffer_copy(self.args(whiten, nvalid))
        bufs, views = {}, {}
        for name, (kind, per) in WIDTH.items():
            if name in null:
                setattr(a, name, None)
                continue
            n, sh = self.count[kind] * per, int(name in shift)
            i32 = name == "status"
            buf = torch.full((PAD + sh + n + PAD,), SENT32 if i32 else SENT64, dtype=torch.int32 if i32 else torch.int64,
                             device="cuda")
            bufs[name] = (buf, PAD + sh, n)
            setattr(a, name, buf.data_ptr() + (PAD + sh) * buf.element_size())
        pipeline.launch(a, torch.device("cuda", torch.cuda.current_device()))
        torch.cuda.synchronize()
        for name, (buf, lo, n) in bufs.items():
            sent = SENT32 if name == "status" else SENT64
            assert bool((buf[:lo] == sent).all()) and bool((buf[lo + n:] == sent).all()), f"{name}: padding written"
            views[name] = buf[lo:lo + n]
            assert not bool((views[name] == sent).any()), f"{name}: element not written"
        return views


_CACHE = {}


def _prob(shape):
    if shape not in _CACHE:  # the oracle runs once per shape, for every test of this file
        _CACHE[shape] = Problem(*shape)
    return _CACHE[shape]


def _f64(v):
    return v.view(torch.float64).cpu().numpy()


def _same(a, b, what):
    assert torch.equal(a, b), what  # integer views: bit for bit


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
@pytest.mark.parametrize("whiten", [False, True], ids=["raw", "whitened"])
def test_every_element_vs_oracle(shape, whiten):
    P = _prob(shape)
    out = P.launch(whiten)
    ref, nk = P.ref, P.nk
    st = out["status"].cpu().numpy()
    np.testing.assert_array_equal(st, ref["status"])
    assert st.sum() == nk and st[P.p["behind"] * nk:(P.p["behind"] + 1) * nk].all()
    ok = st == 0
    scale = {"proj": 1.0 / SP, "dyn": 1.0 / SD, "cv": 1.0 / SC} if whiten else {"proj": np.ones(2), "dyn": np.ones(6),
                                                                             "cv": np.ones(3)}
    for name, (kind, per) in WIDTH.items():
        if name == "status":
            continue
        fam = name.split("_")[1][:4].rstrip("0123")
        got = _f64(out[name]).reshape(P.count[kind], -1)
        if name.startswith("err"):  # 0.5 |r|^2 of the launch's own (whitened) residual
            r = _f64(out["r_" + fam]).reshape(P.count[kind], -1)
            want = 0.5 * (r ** 2).sum(1)
            m = ok if fam == "proj" else slice(None)
            np.testing.assert_allclose(got[:, 0][m], want[m], rtol=1e-14, atol=0, err_msg=name)
            if fam == "proj":
                assert np.isnan(got[~ok]).all()
            continue
        s = scale[fam]
        want = ref[name] * (s if name.startswith("r_") else s[None, None, :])  # column-major: rows last
        want = want.reshape(P.count[kind], -1)
        if fam == "proj":
            assert np.isnan(got[~ok]).all(), name
            got, want = got[ok], want[ok]
        if fam == "cv":
            np.testing.assert_array_equal(got, want, err_msg=name)  # differences and +-1 / sigma: exact
        else:
            np.testing.assert_allclose(got, want, atol=ATOL, rtol=0 if name.startswith("r_") else 1e-12, err_msg=name)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def test_optional_outputs_null(shape):
    P = _prob(shape)
    base = P.launch()
    for null in [(k,) for k in OPTIONAL] + [JACS]:
        out = P.launch(null=null)
        assert set(out) == set(WIDTH) - set(null)
        for name, v in out.items():
            _same(v, base[name], f"{name} with {null} NULL")


@pytest.mark.parametrize("shape", UNALIGNED, ids=lambda s: "x".join(map(str, s)))
def test_outputs_on_8_byte_boundary(shape):
    P = _prob(next(s for s in SHAPES if s[:3] == shape))
    base = P.launch()
    for k in WIDTH:
        if k == "status":
            continue
        out = P.launch(shift=(k,))
        for name, v in out.items():
            _same(v, base[name], f"{name} with {k} offset by 8 bytes")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def test_nvalid_masks_rows(shape):
    P = _prob(shape)
    T, L, nk = P.T, P.L, P.nk
    base = P.launch()
    choices = [0, 1, L - 1, L]
    nv = np.array([choices[(t + 1) % 4] for t in range(T)], np.int32)  # T = 1: 1 = L - 1
    out = P.launch(nvalid=torch.as_tensor(nv, device="cuda"))
    masked = np.repeat(np.array([l < L - nv[t] for t in range(T) for l in range(L)]), nk)
    assert masked.any() and (T == 1 or not masked.all())
    mk = torch.as_tensor(masked, device="cuda")
    st = out["status"]
    assert bool((st[mk] == 2).all())
    _same(st[~mk], base["status"][~mk], "status outside the mask")
    for name, per in (("r_proj", 2), ("j_proj", 12), ("err_proj", 1)):
        v, b = out[name].reshape(-1, per), base[name].reshape(-1, per)
        assert bool((v[mk] == 0).all()), f"{name}: masked rows are +0.0"
        _same(v[~mk], b[~mk], f"{name} outside the mask")
    for name in WIDTH:
        if name != "status" and not name.endswith("proj"):
            _same(out[name], base[name], name)
