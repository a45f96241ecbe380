"""pa_trajectory_lm_prior_solve / pa_window_lm_prior_solve / pa_trajectory_lm_prior_workspace through
ctypes without a GPU (as test_lm_capi.py): validation returns PA_EINVAL with an "lm:" message before
any launch, so the (never dereferenced) pointers here are made-up addresses."""
import ctypes as C
import os
import subprocess

import pytest

from perseus_amd import _lib

FAKE = 0x1000  # a non-null, 16-byte aligned address: validation never reads through it
POINTERS = ("y", "pose", "vel", "angvel", "corners", "K", "isig_proj", "isig_dyn", "isig_cv", "r_proj", "j_proj",
            "err_proj", "status", "r_dyn", "j_dyn0", "j_dyn1", "j_dyn2", "j_dyn3", "err_dyn", "r_cv", "j_cv0", "j_cv1",
            "err_cv")
PRIOR_IN = ("info", "eta", "xbar_pose", "xbar_angvel", "xbar_vel")
TAIL = (*(FAKE,) * 5, None, FAKE, 1 << 40, None)


def _args(T=3, L=6, n_kp=8, **over):
    a = _lib.TrajArgs()
    a.T, a.L, a.n_kp, a.H, a.W = T, L, n_kp, 256, 256
    a.dt = 1.0 / 30.0
    for k in POINTERS:
        setattr(a, k, FAKE)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _params(**over):
    p = dict(max_iters=10, lambda0=1e-3, lambda_up=10.0, lambda_down=10.0, lambda_min=1e-12, lambda_max=1e12,
             rel_tol=1e-6, abs_tol=1e-9)
    p.update(over)
    return _lib.LMParams(*(p[k] for k, _ in _lib.LMParams._fields_))


def _prior(**over):
    p = _lib.LMPrior(*(FAKE,) * 7)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _both(a, p, prior, tail=TAIL):
    """(rc, message) of the trajectory and the window entry point on the same arguments."""
    L = _lib.lib()
    pp = None if prior is None else C.byref(prior)
    out = [(L.pa_trajectory_lm_prior_solve(C.byref(a), C.byref(p), pp, *tail), L.pa_last_error())]
    out.append((L.pa_window_lm_prior_solve(C.byref(a), C.byref(p), 1, pp, *tail), L.pa_last_error()))
    return out


def test_lm_prior_struct_layout_matches_header(tmp_path):
    """The ctypes mirror of pa_lm_prior has the C compiler's field offsets."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [f[0] for f in _lib.LMPrior._fields_]
    assert names == [*PRIOR_IN, "grad", "err"]
    src = tmp_path / "off.c"
    body = "".join(f'  printf("%zu\\n", offsetof(pa_lm_prior, {n}));\n' for n in names)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "perseus_amd.h"\nint main(void){\n'
                   + body + '  printf("%zu\\n", sizeof(pa_lm_prior));\n  return 0;\n}\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [getattr(_lib.LMPrior, n).offset for n in names] + [C.sizeof(_lib.LMPrior)]


@pytest.mark.parametrize("field", [*PRIOR_IN, "grad"])
def test_null_field_of_a_non_null_prior(field):
    for rc, msg in _both(_args(), _params(), _prior(**{field: None})):
        assert rc == -1, (rc, msg)
        assert msg.startswith(b"lm:") and b"prior" in msg and (field.split("_")[0]).encode() in msg, msg


def test_err_output_is_optional():
    """prior->err may be NULL: with everything else in place the call gets as far as the workspace check."""
    need = _lib.lib().pa_trajectory_lm_prior_workspace(3, 6, 8, 10)
    tail = (*(FAKE,) * 5, None, FAKE, need - 1, None)
    for rc, msg in _both(_args(), _params(), _prior(err=None), tail):
        assert rc == -1 and b"workspace %d < %d" % (need - 1, need) in msg, msg


def test_null_prior_accepts_the_parents_workspace_size():
    """prior = NULL is the parent: its workspace size is enough (one byte less is not), while a
    prior needs pa_trajectory_lm_prior_workspace.  (T = 3 passes every check up to the launch, so
    the accepted sizes are probed from below: the first size that is not rejected is never sent.)"""
    L = _lib.lib()
    parent = L.pa_trajectory_lm_workspace(3, 6, 8, 10)
    need = L.pa_trajectory_lm_prior_workspace(3, 6, 8, 10)
    assert need > parent
    tail = (*(FAKE,) * 5, None, FAKE, parent - 1, None)
    for rc, msg in _both(_args(), _params(), None, tail):
        assert rc == -1 and b"workspace %d < %d" % (parent - 1, parent) in msg, msg
    tail = (*(FAKE,) * 5, None, FAKE, parent, None)  # enough without a prior, not with one
    for rc, msg in _both(_args(), _params(), _prior(), tail):
        assert rc == -1 and b"workspace %d < %d" % (parent, need) in msg, msg


def test_the_parents_checks_hold_with_a_prior():
    for a, p, needle in ((_args(L=25), _params(), b"L 25"), (_args(n_kp=17), _params(), b"n_kp 17"),
                         (_args(), _params(max_iters=0), b"max_iters 0"), (_args(isig_cv=None), _params(), b"isig_cv"),
                         (_args(j_dyn2=None), _params(), b"factor output j_dyn2 ")):
        for prior in (None, _prior()):
            for rc, msg in _both(a, p, prior):
                assert rc == -1 and msg.startswith(b"lm:") and needle in msg, msg


def test_prior_workspace_at_least_the_parents_and_zero_outside_the_limits():
    L = _lib.lib()
    f, g = L.pa_trajectory_lm_prior_workspace, L.pa_trajectory_lm_workspace
    for shape in ((1, 2, 1, 1), (3, 6, 8, 10), (2, 24, 16, 30), (257, 3, 5, 8), (1000, 24, 8, 10)):
        T = shape[0]
        assert f(*shape) >= g(*shape) + T * 13 * 8, shape  # set 1's gradient (T, 12) and the err slots (T)
        assert f(*shape) % 16 == 0
    assert f(0, 6, 8, 10) == 0 and f(3, 1, 8, 10) == 0 and f(3, 25, 8, 10) == 0 and f(3, 6, 17, 10) == 0
    assert f(3, 6, 0, 10) == 0 and f(3, 6, 8, 0) == 0


def test_no_trajectories_is_a_no_op():
    tail = (*(FAKE,) * 5, None, None, 0, None)
    for prior in (None, _prior()):
        for rc, msg in _both(_args(T=0), _params(), prior, tail):
            assert rc == 0, msg
