"""The fields of the constant-velocity factor on the angular velocity (pa_traj_args.isig_cw, r_cw,
err_cw) and its three sibling entry points through ctypes without a GPU (as test_timed_capi.py):
what the entry points reject returns PA_EINVAL with a message before any launch, so the (never
dereferenced) pointers here are made-up addresses."""
import ctypes as C
import os
import subprocess

import pytest

from perseus_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
CW = ("isig_cw", "r_cw", "err_cw")
TIMED = ("dt_pair", "kp_mask", "dt_new", "mask_new")


def _args(**kw):
    """A pa_traj_args that passes every entry point's checks with the factor off (its three
    fields and the timestamp fields NULL unless given)."""
    a = _lib.TrajArgs()
    a.T, a.L, a.n_kp, a.H, a.W, a.dt = 3, 6, 8, 256, 256, 0.1
    for name, typ in _lib.TrajArgs._fields_:
        if typ is C.c_void_p and name not in CW + TIMED:
            setattr(a, name, FAKE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _params():
    return _lib.LMParams(10, 1e-3, 10.0, 10.0, 1e-12, 1e12, 1e-6, 1e-9)


def _lm(a):
    L_ = _lib.lib()
    p = _params()
    rc = L_.pa_trajectory_lm_solve(C.byref(a), C.byref(p), FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, 1 << 40, None)
    return rc, L_.pa_last_error()


def _wlm(a):
    L_ = _lib.lib()
    p = _params()
    rc = L_.pa_window_lm_solve(C.byref(a), C.byref(p), 1, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, 1 << 40, None)
    return rc, L_.pa_last_error()


def _tick(a):
    L_ = _lib.lib()
    return L_.pa_window_pose_tick(C.byref(a), FAKE, 1e-2, FAKE, FAKE, FAKE, None), L_.pa_last_error()


def _pre(a):
    L_ = _lib.lib()
    return L_.pa_window_pose_tick_pre(C.byref(a), 1e-2, FAKE, 1 << 40, None), L_.pa_last_error()


def _reduce(a):
    L_ = _lib.lib()
    return L_.pa_window_pose_tick_reduce_prior(C.byref(a), 1e-2, FAKE, 1 << 40, FAKE, FAKE, None), L_.pa_last_error()


def _post(a):
    L_ = _lib.lib()
    return L_.pa_window_pose_tick_post(C.byref(a), FAKE, FAKE, 1 << 40, FAKE, FAKE, FAKE, None), L_.pa_last_error()


def _lin(a):
    L_ = _lib.lib()
    return L_.pa_trajectory_linearize(C.byref(a), None), L_.pa_last_error()


def test_new_fields_at_the_c_compilers_offsets(tmp_path):
    """isig_cw directly after isig_cv; r_cw, err_cw after err_dyn and before r_cv; nothing at or
    after err_cv (test_timed_capi.py / test_robust_capi.py pin the last eight names); the ctypes
    mirror has gcc's offsets for the new fields, every field they moved, and the size."""
    names = [f[0] for f in _lib.TrajArgs._fields_]
    assert names[names.index("isig_cv") + 1] == "isig_cw"
    i = names.index("err_dyn")
    assert names[i + 1:i + 4] == ["r_cw", "err_cw", "r_cv"]
    assert names[-8:] == ["err_cv", *TIMED, "nvalid", "robust_proj", "robust_proj_k"]
    moved = names[names.index("isig_cw"):]
    src = tmp_path / "off.c"
    body = "".join(f'  printf("%zu\\n", offsetof(pa_traj_args, {n}));\n' for n in moved)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "perseus_amd.h"\nint main(void){\n'
                   + body + '  printf("%zu\\n", sizeof(pa_traj_args));\n  return 0;\n}\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [getattr(_lib.TrajArgs, n).offset for n in moved] + [C.sizeof(_lib.TrajArgs)]
    assert got == want
    assert all(getattr(_lib.TrajArgs(), n) is None for n in CW)  # zero-initialised = off


@pytest.mark.parametrize("call", [_lm, _wlm, _tick, _pre, _reduce, _post])
def test_on_needs_isig_cw(call):
    rc, msg = call(_args(r_cw=FAKE, err_cw=FAKE))
    assert rc == -1 and b"isig_cw" in msg, (rc, msg)


@pytest.mark.parametrize("call", [_lm, _wlm])
def test_lm_on_needs_err_cw(call):
    rc, msg = call(_args(r_cw=FAKE, isig_cw=FAKE))
    assert rc == -1 and b"err_cw" in msg, (rc, msg)


@pytest.mark.parametrize("call", [_lin, _tick, _pre, _reduce, _post])
def test_err_cw_without_the_switch(call):
    rc, msg = call(_args(err_cw=FAKE, isig_cw=FAKE))
    assert rc == -1 and b"err_cw" in msg and b"r_cw" in msg, (rc, msg)


@pytest.mark.parametrize("call,needle", [(_lm, b"L 25"), (_wlm, b"L 25"), (_tick, b"L 25"), (_pre, b"L 25"),
                                         (_reduce, b"L 25"), (_post, b"L 25")])
def test_older_checks_come_first(call, needle):
    """An inconsistent factor AND an older error: the older message (the existing C-ABI tests
    fill every pointer and expect theirs)."""
    a = _args(r_cw=FAKE)
    a.L = 25
    rc, msg = call(a)
    assert rc == -1 and needle in msg and b"cw" not in msg, (rc, msg)


def test_off_demands_neither():
    """Factor off (r_cw NULL): LM does not ask for isig_cw / err_cw -- it passes every check up
    to the workspace size, which is the last one before the factor's."""
    L_ = _lib.lib()
    a, p = _args(), _params()
    rc = L_.pa_trajectory_lm_solve(C.byref(a), C.byref(p), FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, 8, None)
    assert rc == -1 and b"workspace" in L_.pa_last_error()
    a = _args(isig_cw=FAKE)  # a whitening alone switches nothing on
    rc = L_.pa_trajectory_lm_solve(C.byref(a), C.byref(p), FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, 8, None)
    assert rc == -1 and b"workspace" in L_.pa_last_error()


@pytest.mark.parametrize("call", [_lin, _lm, _wlm, _tick, _pre, _reduce, _post])
def test_no_trajectories_is_a_no_op(call):
    for kw in (dict(), dict(r_cw=FAKE), dict(r_cw=FAKE, isig_cw=FAKE, err_cw=FAKE)):
        a = _args(**kw)
        a.T = 0
        rc, msg = call(a)
        assert rc == 0, msg


def _gn_cw(T=3, L=6, r_cw=FAKE, isig_cw=FAKE, pi=None, pg=None, ws_bytes=1 << 40):
    L_ = _lib.lib()
    rc = L_.pa_trajectory_gn_step_cw(T, L, 8, *[FAKE] * 11, r_cw, isig_cw, 1e-2, None, None, None, FAKE, FAKE, FAKE,
                                     ws_bytes, pi, pg, None)
    return rc, L_.pa_last_error()


def _marg_cw(T=3, L=6, r_cw=FAKE, isig_cw=FAKE, pi=None, pg=None, ws_bytes=1 << 40):
    L_ = _lib.lib()
    rc = L_.pa_trajectory_marginals_cw(T, L, 8, *[FAKE] * 11, r_cw, isig_cw, 1e-9, FAKE, None, None, FAKE, FAKE,
                                       ws_bytes, pi, pg, None)
    return rc, L_.pa_last_error()


def _mz_cw(T=3, L=6, r_cw=FAKE, isig_cw=FAKE, pi=None, pg=None, lam=1e-2):
    L_ = _lib.lib()
    rc = L_.pa_window_marginalize_cw(T, L, 8, *[FAKE] * 11, pi, pg, r_cw, isig_cw, lam, None, None, None,
                                     *[FAKE] * 9, None)
    return rc, L_.pa_last_error()


SIBLINGS = [(_gn_cw, b"gn:"), (_marg_cw, b"marginals:"), (_mz_cw, b"marginalize:")]


def test_the_three_siblings_are_exported():
    L_ = _lib.lib()
    for name in ("pa_trajectory_gn_step_cw", "pa_trajectory_marginals_cw", "pa_window_marginalize_cw"):
        assert hasattr(L_, name) and name in _lib._SIGS


@pytest.mark.parametrize("call,prefix", SIBLINGS)
def test_siblings_reject(call, prefix):
    rc, msg = call(isig_cw=None)
    assert rc == -1 and msg.startswith(prefix) and b"isig_cw" in msg, (rc, msg)
    rc, msg = call(pi=FAKE)  # the prior pair is given together or not at all, as in the _prior parents
    assert rc == -1 and msg.startswith(prefix) and b"together" in msg, (rc, msg)
    rc, msg = call(isig_cw=None, pi=FAKE)  # the older check first
    assert rc == -1 and b"together" in msg, (rc, msg)
    for kw in (dict(), dict(isig_cw=None), dict(r_cw=None, isig_cw=None)):
        rc, msg = call(T=0, **kw)
        assert rc == 0, msg


def test_sibling_workspaces_are_the_parents():
    rc, msg = _gn_cw(ws_bytes=8)
    assert rc == -1 and b"workspace" in msg
    rc, msg = _marg_cw(ws_bytes=8)
    assert rc == -1 and b"workspace" in msg
