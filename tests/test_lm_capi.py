"""pa_trajectory_lm_solve / pa_trajectory_lm_workspace through ctypes without a GPU (as
test_capi.py): every argument outside the entry point's limits returns PA_EINVAL with a message
before any launch, so the (never dereferenced) pointers here are made-up addresses."""
import ctypes as C

import pytest

from perseus_amd import _lib

FAKE = 0x1000  # a non-null, 16-byte aligned address: validation never reads through it
POINTERS = ("y", "pose", "vel", "angvel", "corners", "K", "isig_proj", "isig_dyn", "isig_cv", "r_proj", "j_proj",
            "err_proj", "status", "r_dyn", "j_dyn0", "j_dyn1", "j_dyn2", "j_dyn3", "err_dyn", "r_cv", "j_cv0", "j_cv1",
            "err_cv")
FACTOR_OUT = POINTERS[9:]


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


def _solve(a, p, ws_bytes=1 << 40, outs=(FAKE,) * 5, ws=FAKE):
    L = _lib.lib()
    rc = L.pa_trajectory_lm_solve(C.byref(a), C.byref(p), *outs, None, ws, ws_bytes, None)
    return rc, L.pa_last_error()


def _rejected(a, p, needle, **kw):
    rc, msg = _solve(a, p, **kw)
    assert rc == -1, (rc, msg)
    assert msg.startswith(b"lm:") and needle in msg, msg


def test_lm_params_struct_layout_matches_header(tmp_path):
    """The ctypes mirror of pa_lm_params has the C compiler's field offsets."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [f[0] for f in _lib.LMParams._fields_]
    src = tmp_path / "off.c"
    body = "".join(f'  printf("%zu\\n", offsetof(pa_lm_params, {n}));\n' for n in names)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "perseus_amd.h"\nint main(void){\n'
                   + body + '  printf("%zu\\n", sizeof(pa_lm_params));\n  return 0;\n}\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [getattr(_lib.LMParams, n).offset for n in names] + [C.sizeof(_lib.LMParams)]


@pytest.mark.parametrize("L", [1, 25])
def test_window_length_outside_the_solver_range(L):
    _rejected(_args(L=L), _params(), b"L %d" % L)


def test_too_many_keypoints():
    _rejected(_args(n_kp=17), _params(), b"n_kp 17")


def test_max_iters_zero():
    _rejected(_args(), _params(max_iters=0), b"max_iters 0")


@pytest.mark.parametrize("up", [1.0, 0.5])
def test_lambda_up_not_above_one(up):
    _rejected(_args(), _params(lambda_up=up), b"lambda_up")


@pytest.mark.parametrize("bad", [dict(lambda0=0.0), dict(lambda_down=1.0), dict(lambda_min=1.0, lambda_max=0.5),
                                 dict(rel_tol=-1.0), dict(abs_tol=float("nan")), dict(lambda0=float("nan"))])
def test_other_bad_parameters(bad):
    _rejected(_args(), _params(**bad), b"tol" if "tol" in next(iter(bad)) else b"lambda")


@pytest.mark.parametrize("field", ["isig_proj", "isig_dyn", "isig_cv"])
def test_missing_whitening_sigma(field):
    _rejected(_args(**{field: None}), _params(), field.encode())


@pytest.mark.parametrize("field", FACTOR_OUT)
def test_missing_factor_output_or_jacobian(field):
    _rejected(_args(**{field: None}), _params(), b"factor output " + field.encode() + b" ")


@pytest.mark.parametrize("field", ["y", "pose", "vel", "angvel", "corners", "K"])
def test_missing_state_or_model_pointer(field):
    _rejected(_args(**{field: None}), _params(), b"null state / model pointer")


def test_null_args_params_and_outputs():
    L = _lib.lib()
    assert L.pa_trajectory_lm_solve(None, C.byref(_params()), *(FAKE,) * 5, None, FAKE, 1 << 40, None) == -1
    assert L.pa_trajectory_lm_solve(C.byref(_args()), None, *(FAKE,) * 5, None, FAKE, 1 << 40, None) == -1
    for i in range(5):
        outs = tuple(None if j == i else FAKE for j in range(5))
        _rejected(_args(), _params(), b"output", outs=outs)


def test_workspace_too_small_or_missing():
    need = _lib.lib().pa_trajectory_lm_workspace(3, 6, 8, 10)
    _rejected(_args(), _params(), b"workspace %d < %d" % (need - 1, need), ws_bytes=need - 1)
    _rejected(_args(), _params(), b"workspace", ws=None)
    _rejected(_args(), _params(), b"aligned", ws=FAKE + 8)


def test_window_solve_and_reduce_check_their_arguments():
    """pa_window_lm_solve takes pa_trajectory_lm_solve's checks; pa_window_pose_tick_reduce the
    split tick's."""
    L = _lib.lib()
    tail = (*(FAKE,) * 5, None, FAKE, 1 << 40, None)
    assert L.pa_window_lm_solve(None, C.byref(_params()), 1, *tail) == -1
    assert L.pa_window_lm_solve(C.byref(_args(L=25)), C.byref(_params()), 1, *tail) == -1
    assert b"L 25" in L.pa_last_error()
    assert L.pa_window_lm_solve(C.byref(_args(isig_dyn=None)), C.byref(_params()), 0, *tail) == -1
    assert b"isig_dyn" in L.pa_last_error()
    need = L.pa_trajectory_lm_workspace(3, 6, 8, 10)
    assert L.pa_window_lm_solve(C.byref(_args()), C.byref(_params()), 1, *(FAKE,) * 5, None, FAKE, need - 1, None) == -1
    assert L.pa_window_lm_solve(C.byref(_args(T=0)), C.byref(_params()), 1, *(FAKE,) * 5, None, None, 0, None) == 0
    assert L.pa_window_pose_tick_reduce(None, 1e-2, FAKE, 1 << 40, None) == -1
    a = _args(nvalid=FAKE)
    assert L.pa_window_pose_tick_reduce(C.byref(a), -1.0, FAKE, 1 << 40, None) == -1
    assert b"lambda" in L.pa_last_error()
    assert L.pa_window_pose_tick_reduce(C.byref(a), 1e-2, FAKE, L.pa_window_pose_tick_workspace(3, 6) - 1, None) == -1
    assert b"workspace" in L.pa_last_error()
    assert L.pa_window_pose_tick_reduce(C.byref(_args(nvalid=None)), 1e-2, FAKE, 1 << 40, None) == -1
    assert L.pa_window_pose_tick_reduce(C.byref(_args(L=25, nvalid=FAKE)), 1e-2, FAKE, 1 << 40, None) == -1


def test_no_trajectories_is_a_no_op():
    rc, _ = _solve(_args(T=0), _params(), ws_bytes=0, ws=None)
    assert rc == 0


def test_workspace_positive_and_monotone():
    f = _lib.lib().pa_trajectory_lm_workspace
    assert f(1, 2, 1, 1) > 0
    sizes_T = [f(T, 6, 8, 10) for T in (1, 2, 3, 64, 257, 1000)]
    assert all(a < b for a, b in zip(sizes_T, sizes_T[1:]))
    sizes_it = [f(3, 6, 8, k) for k in (1, 2, 8, 9, 30, 100)]
    assert all(a <= b for a, b in zip(sizes_it, sizes_it[1:])) and sizes_it[0] < sizes_it[-1]
    assert f(3, 24, 16, 10) > f(3, 6, 8, 10)
    # shapes the solve rejects need no workspace
    assert f(0, 6, 8, 10) == 0 and f(3, 1, 8, 10) == 0 and f(3, 25, 8, 10) == 0 and f(3, 6, 17, 10) == 0
    assert f(3, 6, 8, 0) == 0
