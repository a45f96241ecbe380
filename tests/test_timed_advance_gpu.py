"""pa_window_advance_t (window_advance_t_kernel) on the device, through
pipeline.window_advance(..., dt_new=, mask_new=), against timed_ref.window_advance_t: every moved
element and both rings exact, the predicted pose within 1e-12; both rings, each ring alone, the
smallest window (L = 2) and windows longer than the kernel's 256-thread workgroup (L = 258: one
further ring round of one element; L = 600: two further rounds).  With the rings absent, or
present at the nominal dt, the window is bit for bit pa_window_advance_n's."""
import numpy as np
import pytest
import torch

import timed_ref as TR
from oracle import factors_ref as F
from perseus_amd import _lib, pipeline

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = 1.0 / 30.0
NK = 8
CORE = ("y", "pose", "angvel", "vel")


def _window(T, L, seed, rings):
    rng = np.random.default_rng(seed)
    pose = np.array([[F.pack(F.pose_exp(np.concatenate([0.5 * rng.standard_normal(3), 0.1 * rng.standard_normal(3)])))
                      for _ in range(L)] for _ in range(T)])
    win = dict(y=rng.uniform(-1, 1, (T, L, 2 * NK)).astype(np.float32), pose=pose,
               angvel=0.5 * rng.standard_normal((T, L, 3)), vel=0.05 * rng.standard_normal((T, L, 3)))
    if rings in ("both", "dt"):
        win["dt"] = np.exp(rng.uniform(np.log(1.0 / 240.0), np.log(0.5), (T, L - 1)))
    if rings in ("both", "mask"):
        win["mask"] = rng.integers(-2 ** 31, 2 ** 31, (T, L)).astype(np.int32)  # all 32 bits are only moved
    new = dict(y=rng.uniform(-1, 1, (T, 2 * NK)).astype(np.float32),
               dt=np.exp(rng.uniform(np.log(1.0 / 240.0), np.log(0.5), T)) if "dt" in win else None,
               mask=rng.integers(-2 ** 31, 2 ** 31, T).astype(np.int32) if "mask" in win else None)
    return win, new


def _dev(win):
    return {k: torch.as_tensor(v, device=DEV).contiguous() for k, v in win.items()}


def _t(a):
    return None if a is None else torch.as_tensor(a, device=DEV)


@pytest.mark.parametrize("vf", ["world", "body"])
@pytest.mark.parametrize("L,rings", [(2, "both"), (3, "both"), (6, "both"), (6, "dt"), (6, "mask"), (258, "both"),
                                     (600, "both"), (600, "mask")])
def test_window_advance_t_vs_reference(L, rings, vf):
    T = 3
    win, new = _window(T, L, 17 * L + len(rings), rings)
    nvalid = np.array([0, L - 1, L], np.int32)
    d, nv = _dev(win), _t(nvalid)
    keep = (_t(new["dt"]), _t(new["mask"]))
    pipeline.window_advance(_t(new["y"]), d, dt=DT, vel_frame=vf, nvalid=nv, dt_new=keep[0], mask_new=keep[1])
    torch.cuda.synchronize()
    ref = TR.window_advance_t(win, new["y"], new["dt"], new["mask"], DT, vf)
    got = {k: v.cpu().numpy() for k, v in d.items()}
    assert set(got) == set(ref)
    for k in ("y", "angvel", "vel", "dt", "mask"):  # moved, carried or landed: never recomputed
        if k in ref:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(got["pose"][:, :-1], ref["pose"][:, :-1])
    np.testing.assert_allclose(got["pose"][:, -1], ref["pose"][:, -1], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(nv.cpu().numpy(), np.minimum(nvalid + 1, L))
    if "dt" in win:  # the new frame was predicted with its trajectory's dt_new, not with dt
        other = TR.window_advance_t({k: win[k] for k in CORE}, new["y"], None, None, DT, vf)
        assert np.abs(other["pose"][:, -1] - ref["pose"][:, -1]).max() > 1e-6


@pytest.mark.parametrize("L", [2, 6, 300])
def test_rings_absent_or_nominal_are_pa_window_advance_n(L):
    T = 3
    win, new = _window(T, L, L, "both")
    core = {k: win[k] for k in CORE}
    a = _dev(core)
    na = torch.zeros(T, dtype=torch.int32, device=DEV)
    pipeline.window_advance(_t(new["y"]), a, dt=DT, nvalid=na)  # pa_window_advance_n
    # the dt ring at the nominal dt_new (whatever the ring holds, it is only moved), and the mask ring
    b = _dev(win)
    nb = torch.zeros(T, dtype=torch.int32, device=DEV)
    keep = (_t(np.full(T, DT)), _t(new["mask"]))
    pipeline.window_advance(_t(new["y"]), b, dt=0.5, nvalid=nb, dt_new=keep[0], mask_new=keep[1])
    # the mask ring alone: the prediction uses dt
    c = _dev({**core, "mask": win["mask"]})
    pipeline.window_advance(_t(new["y"]), c, dt=DT, mask_new=keep[1])
    # no ring at all, through the new entry point
    e = _dev(core)
    ne = torch.zeros(T, dtype=torch.int32, device=DEV)
    yn = _t(new["y"])
    _lib.check(_lib.lib().pa_window_advance_t(T, L, NK, yn.data_ptr(), e["y"].data_ptr(), e["pose"].data_ptr(),
                                              e["angvel"].data_ptr(), e["vel"].data_ptr(), ne.data_ptr(), None, None, None,
                                              None, DT, _lib.VEL_WORLD, _lib.stream_of(torch.device(DEV, 0))),
               "pa_window_advance_t")
    torch.cuda.synchronize()
    for other, what in ((b, "nominal dt ring"), (c, "mask ring alone"), (e, "no ring")):
        for k in CORE:
            assert torch.equal(a[k].view(torch.int32 if k == "y" else torch.int64),
                               other[k].view(torch.int32 if k == "y" else torch.int64)), (what, k)
    assert torch.equal(na, nb) and torch.equal(na, ne)


def test_window_advance_wants_each_ring_with_its_new_element():
    win, new = _window(2, 4, 1, "both")
    d = _dev(win)
    with pytest.raises(ValueError, match="dt_new"):
        pipeline.window_advance(_t(new["y"]), d, dt=DT, mask_new=_t(new["mask"]))
    with pytest.raises(ValueError, match="mask_new"):
        pipeline.window_advance(_t(new["y"]), d, dt=DT, dt_new=_t(new["dt"]))
