"""The robust noise model arguments (pa_traj_args.robust_proj / robust_proj_k and
pa_proj_linearize_robust's robust_kind / robust_k) through ctypes without a GPU, as test_capi.py
and test_lm_capi.py: a kind outside PA_ROBUST_NONE / HUBER / CAUCHY, or a kind != 0 with k not a
positive finite number, returns PA_EINVAL with a message naming the field before any launch, so
the (never dereferenced) pointers here are made-up addresses.  k is ignored when the kind is 0."""
import ctypes as C

import pytest

from perseus_amd import _lib
from test_lm_capi import FAKE, _args, _params  # tests/ is on sys.path (rootdir conftest)

NAN = float("nan")
BAD = [(7, 1.0, b"robust_proj 7"), (-1, 1.0, b"robust_proj -1"), (1, 0.0, b"robust_proj_k 0"),
       (1, -1.0, b"robust_proj_k -1"), (1, NAN, b"robust_proj_k nan"), (2, float("inf"), b"robust_proj_k inf"),
       (2, 0.0, b"robust_proj_k 0")]


def _linearize(a):
    L = _lib.lib()
    return L.pa_trajectory_linearize(C.byref(a), None), L.pa_last_error()


def _lm(a, ws_bytes=1 << 40):
    L = _lib.lib()
    rc = L.pa_trajectory_lm_solve(C.byref(a), C.byref(_params()), *(FAKE,) * 5, None, FAKE, ws_bytes, None)
    return rc, L.pa_last_error()


def _window_lm(a):
    L = _lib.lib()
    rc = L.pa_window_lm_solve(C.byref(a), C.byref(_params()), 1, *(FAKE,) * 5, None, FAKE, 1 << 40, None)
    return rc, L.pa_last_error()


def _pre(a):
    L = _lib.lib()
    return L.pa_window_pose_tick_pre(C.byref(a), 1e-2, FAKE, 1 << 40, None), L.pa_last_error()


def _reduce(a):
    L = _lib.lib()
    return L.pa_window_pose_tick_reduce(C.byref(a), 1e-2, FAKE, 1 << 40, None), L.pa_last_error()


def _post(a):
    L = _lib.lib()
    return L.pa_window_pose_tick_post(C.byref(a), FAKE, FAKE, 1 << 40, FAKE, FAKE, FAKE, None), L.pa_last_error()


def _tick(a):
    L = _lib.lib()
    return L.pa_window_pose_tick(C.byref(a), FAKE, 1e-2, FAKE, FAKE, FAKE, None), L.pa_last_error()


ENTRY_POINTS = [_linearize, _lm, _window_lm, _pre, _reduce, _post, _tick]


def test_library_exports_the_robust_entry_point():
    assert hasattr(_lib.lib(), "pa_proj_linearize_robust")
    assert (_lib.ROBUST_NONE, _lib.ROBUST_HUBER, _lib.ROBUST_CAUCHY) == (0, 1, 2)


def test_zero_initialised_args_mean_off():
    a = _lib.TrajArgs()
    assert a.robust_proj == 0 and a.robust_proj_k == 0.0
    names = [f[0] for f in _lib.TrajArgs._fields_]
    assert names[-3:] == ["nvalid", "robust_proj", "robust_proj_k"]  # appended, as nvalid was


@pytest.mark.parametrize("call", ENTRY_POINTS, ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("kind,k,needle", BAD)
def test_bad_kind_or_k_is_rejected_before_any_launch(call, kind, k, needle):
    rc, msg = call(_args(nvalid=FAKE, robust_proj=kind, robust_proj_k=k))
    assert rc == -1, (rc, msg)
    assert needle in msg, msg


@pytest.mark.parametrize("k", [NAN, 0.0, -1.0])
def test_k_is_ignored_when_off(k):
    """kind 0 passes the robust check whatever k holds, and the call then fails on its next
    argument check, as it did before the fields existed."""
    rc, msg = _linearize(_args(y=None, robust_proj_k=k))
    assert rc == -1 and b"null input pointer" in msg, msg
    need = _lib.lib().pa_trajectory_lm_workspace(3, 6, 8, 10)
    rc, msg = _lm(_args(robust_proj_k=k), ws_bytes=need - 1)
    assert rc == -1 and b"workspace %d < %d" % (need - 1, need) in msg, msg
    rc, msg = _pre(_args(nvalid=None, robust_proj_k=k))
    assert rc == -1 and b"null window / model pointer" in msg, msg


@pytest.mark.parametrize("kind,k", [(1, 1.345), (2, 1.0)])
def test_valid_robust_arguments_pass_the_check(kind, k):
    rc, msg = _linearize(_args(y=None, robust_proj=kind, robust_proj_k=k))
    assert rc == -1 and b"null input pointer" in msg, msg
    rc, msg = _lm(_args(isig_cv=None, robust_proj=kind, robust_proj_k=k))
    assert rc == -1 and b"isig_cv" in msg, msg
    rc, msg = _pre(_args(nvalid=None, robust_proj=kind, robust_proj_k=k))
    assert rc == -1 and b"null window / model pointer" in msg, msg


def _proj(kind, k, n=4, tbody=FAKE):
    L = _lib.lib()
    rc = L.pa_proj_linearize_robust(n, tbody, FAKE, FAKE, FAKE, 0, None, 0, None, kind, k, FAKE, FAKE, FAKE, FAKE,
                                    None)
    return rc, L.pa_last_error()


@pytest.mark.parametrize("kind,k,needle", [(7, 1.0, b"robust_kind 7"), (1, 0.0, b"robust_k 0"),
                                           (1, -1.0, b"robust_k -1"), (2, NAN, b"robust_k nan")])
def test_proj_linearize_robust_checks_its_arguments(kind, k, needle):
    rc, msg = _proj(kind, k)
    assert rc == -1 and needle in msg, msg


def test_proj_linearize_robust_keeps_the_plain_checks():
    rc, msg = _proj(0, NAN, tbody=None)
    assert rc == -1 and b"null pointer" in msg, msg
    rc, msg = _proj(1, 1.345, tbody=None)
    assert rc == -1 and b"null pointer" in msg, msg
    assert _proj(1, 1.345, n=0)[0] == 0  # nothing to do
    assert _proj(1, 1.345, n=-1)[0] == -1


def test_python_robust_code():
    assert _lib.robust_code(None) == (0, 0.0)
    assert _lib.robust_code(("huber", 1.345)) == (1, 1.345)
    assert _lib.robust_code(("cauchy", 1)) == (2, 1.0)
    with pytest.raises(ValueError, match="robust kind"):
        _lib.robust_code(("tukey", 1.0))


def test_noise_model_classes():
    from perseus_amd.smoother import noiseModel

    h = noiseModel.mEstimator.Huber.Create(1.345)
    c = noiseModel.mEstimator.Cauchy.Create(2.0)
    assert h.weight(1.0) == 1.0 and h.weight(2.69) == 0.5 and h.loss(1.0) == 0.5
    assert h.loss(2.69) == 1.345 * (2.69 - 0.5 * 1.345)
    assert c.weight(2.0) == 0.5 and abs(c.loss(2.0) - 2.0 * 0.6931471805599453) < 1e-15
    nm = noiseModel.Robust.Create(h, noiseModel.Isotropic.Sigma(2, 60.0))
    assert nm.sigmas().tolist() == [60.0, 60.0] and nm.robust() is h
    assert _lib.robust_code(nm.robust()) == (1, 1.345)
    for bad in (0.0, -1.0, NAN):
        with pytest.raises(ValueError, match="positive finite"):
            noiseModel.mEstimator.Cauchy.Create(bad)
