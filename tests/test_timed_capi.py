"""The real-timestamp fields of pa_traj_args (dt_pair, kp_mask, dt_new, mask_new) and
pa_window_advance_t through ctypes without a GPU (as test_prior_capi.py): what the entry points
reject returns PA_EINVAL with a message before any launch, so the (never dereferenced) pointers
here are made-up addresses."""
import ctypes as C
import os
import subprocess

import pytest

from perseus_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
NEW = ("dt_pair", "kp_mask", "dt_new", "mask_new")


def _args(**kw):
    """A pa_traj_args that passes every entry point's checks; the four new fields NULL unless given."""
    a = _lib.TrajArgs()
    a.T, a.L, a.n_kp, a.H, a.W, a.dt = 3, 6, 8, 256, 256, 0.1
    for name, typ in _lib.TrajArgs._fields_:
        if typ is C.c_void_p and name not in NEW:
            setattr(a, name, FAKE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _tick(a):
    L_ = _lib.lib()
    return L_.pa_window_pose_tick(C.byref(a), FAKE, 1e-2, FAKE, FAKE, FAKE, None), L_.pa_last_error()


def _tick_prior(a):
    L_ = _lib.lib()
    return L_.pa_window_pose_tick_prior(C.byref(a), FAKE, 1e-2, FAKE, FAKE, FAKE, FAKE, FAKE, None), L_.pa_last_error()


def _pre(a):
    L_ = _lib.lib()
    return L_.pa_window_pose_tick_pre(C.byref(a), 1e-2, FAKE, 1 << 40, None), L_.pa_last_error()


def _pre_prior(a):
    L_ = _lib.lib()
    return L_.pa_window_pose_tick_pre_prior(C.byref(a), 1e-2, FAKE, 1 << 40, FAKE, FAKE, None), L_.pa_last_error()


ADVANCING = [(_tick, b"pose tick:"), (_tick_prior, b"pose tick:"), (_pre, b"pose tick pre:"),
             (_pre_prior, b"pose tick pre:")]


@pytest.mark.parametrize("call,prefix", ADVANCING)
@pytest.mark.parametrize("given,needle", [(("dt_pair",), b"dt_pair and dt_new"), (("dt_new",), b"dt_pair and dt_new"),
                                          (("kp_mask",), b"kp_mask and mask_new"),
                                          (("mask_new",), b"kp_mask and mask_new"),
                                          (("dt_pair", "dt_new", "kp_mask"), b"kp_mask and mask_new"),
                                          (("kp_mask", "mask_new", "dt_new"), b"dt_pair and dt_new")])
def test_advancing_entry_points_want_each_ring_with_its_new_element(call, prefix, given, needle):
    rc, msg = call(_args(**{k: FAKE for k in given}))
    assert rc == -1, (rc, msg)
    assert msg.startswith(prefix) and needle in msg and b"together" in msg, msg


@pytest.mark.parametrize("call,prefix", ADVANCING)
def test_advancing_entry_points_keep_their_own_checks(call, prefix):
    for kw in (dict(), dict(dt_pair=FAKE, dt_new=FAKE), dict(kp_mask=FAKE, mask_new=FAKE)):
        a = _args(**kw)
        a.L = 25
        rc, msg = call(a)
        assert rc == -1 and b"L 25" in msg, (rc, msg)
        a = _args(**kw)
        a.T = 0  # nothing to do
        rc, msg = call(a)
        assert rc == 0, msg


def test_non_advancing_entry_points_ignore_the_new_pair():
    """_reduce and _post do not advance: a ring without its _new element passes their checks
    (here up to the next one, the workspace size)."""
    L_ = _lib.lib()
    a = _args(dt_pair=FAKE, kp_mask=FAKE)
    assert L_.pa_window_pose_tick_reduce(C.byref(a), 1e-2, FAKE, 8, None) == -1
    assert b"workspace" in L_.pa_last_error()
    assert L_.pa_window_pose_tick_post(C.byref(a), FAKE, FAKE, 8, FAKE, FAKE, FAKE, None) == -1
    assert b"workspace" in L_.pa_last_error()


def test_linearize_rejects_a_mask_with_more_than_32_keypoints():
    L_ = _lib.lib()
    a = _args(kp_mask=FAKE)
    a.n_kp = 33
    assert L_.pa_trajectory_linearize(C.byref(a), None) == -1
    msg = L_.pa_last_error()
    assert b"kp_mask" in msg and b"33" in msg, msg


def _advance_t(dt_pair=None, kp_mask=None, dt_new=None, mask_new=None, T=3, L=6, n_kp=8):
    L_ = _lib.lib()
    rc = L_.pa_window_advance_t(T, L, n_kp, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, dt_pair, kp_mask, dt_new, mask_new,
                                0.1, 0, None)
    return rc, L_.pa_last_error()


@pytest.mark.parametrize("kw,needle", [(dict(dt_pair=FAKE), b"dt_pair and dt_new"), (dict(dt_new=FAKE), b"dt_pair and dt_new"),
                                       (dict(kp_mask=FAKE), b"kp_mask and mask_new"),
                                       (dict(mask_new=FAKE), b"kp_mask and mask_new"),
                                       (dict(n_kp=33, kp_mask=FAKE, mask_new=FAKE), b"n_kp=33")])
def test_window_advance_t_rejects(kw, needle):
    rc, msg = _advance_t(**kw)
    assert rc == -1 and needle in msg, (rc, msg)


def test_window_advance_t_no_trajectories_is_a_no_op():
    for kw in (dict(), dict(dt_pair=FAKE, dt_new=FAKE), dict(kp_mask=FAKE, mask_new=FAKE)):
        rc, msg = _advance_t(T=0, **kw)
        assert rc == 0, msg


def test_dyn_linearize_dt_checks():
    L_ = _lib.lib()
    assert L_.pa_dyn_linearize_dt(0, *[None] * 5, 0, *[None] * 7, None) == 0
    assert L_.pa_dyn_linearize_dt(4, FAKE, FAKE, FAKE, FAKE, None, 0, None, FAKE, *[None] * 5, None) == -1
    assert b"null" in L_.pa_last_error()
    assert L_.pa_dyn_linearize_dt(4, FAKE, FAKE, FAKE, FAKE, FAKE, 7, None, FAKE, *[None] * 5, None) == -1
    assert b"vel_frame" in L_.pa_last_error()


def test_new_fields_stand_before_nvalid_at_the_c_compilers_offsets(tmp_path):
    """The four fields stand in the header's order between err_cv and nvalid (the struct still
    ends in nvalid, robust_proj, robust_proj_k, which test_robust_capi.py pins), and the ctypes
    mirror has the C compiler's offsets for them and for the three they moved (and its size)."""
    names = [f[0] for f in _lib.TrajArgs._fields_]
    assert names[-8:] == ["err_cv", *NEW, "nvalid", "robust_proj", "robust_proj_k"]
    src = tmp_path / "off.c"
    moved = NEW + ("nvalid", "robust_proj", "robust_proj_k")
    body = "".join(f'  printf("%zu\\n", offsetof(pa_traj_args, {n}));\n' for n in moved)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "perseus_amd.h"\nint main(void){\n'
                   + body + '  printf("%zu\\n", sizeof(pa_traj_args));\n  return 0;\n}\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [getattr(_lib.TrajArgs, n).offset for n in moved] + [C.sizeof(_lib.TrajArgs)]
    assert got == want
    assert all(getattr(_lib.TrajArgs(), n) is None for n in NEW)  # zero-initialised = none
