"""pa_trajectory_marginals / pa_trajectory_marginals_workspace through ctypes without a GPU (as
test_lm_capi.py): every argument outside the entry point's limits returns PA_EINVAL with a
message before any launch, so the (never dereferenced) pointers here are made-up addresses."""
import pytest

from perseus_amd import _lib

FAKE = 0x1000  # a non-null address: validation never reads through it
FACTORS = ("r_proj", "j_proj", "status", "r_dyn", "j_dyn0", "j_dyn1", "j_dyn2", "j_dyn3", "r_cv", "j_cv0", "j_cv1")


def _call(T=3, L=6, n_kp=8, lam=1e-3, cov=FAKE, cross=None, cov_newest=None, info=FAKE, ws=FAKE, ws_bytes=1 << 40,
          **factors):
    ptrs = [factors.get(k, FAKE) for k in FACTORS]
    L_ = _lib.lib()
    rc = L_.pa_trajectory_marginals(T, L, n_kp, *ptrs, lam, cov, cross, cov_newest, info, ws, ws_bytes, None)
    return rc, L_.pa_last_error()


def _rejected(needle, **kw):
    rc, msg = _call(**kw)
    assert rc == -1, (rc, msg)
    assert msg.startswith(b"marginals:") and needle in msg, msg


def test_workspace_size():
    f = _lib.lib().pa_trajectory_marginals_workspace
    assert f(0, 24) == 0
    for T, L in ((1, 2), (3, 24), (257, 5), (1000, 24)):
        n = f(T, L)
        assert n > 0 and n % 8 == 0, (T, L, n)
    assert f(3, 24) < f(4, 24) and f(3, 23) < f(3, 24)


def test_window_of_one_frame():
    _rejected(b"L 1", L=1)


def test_too_many_keypoints():
    _rejected(b"n_kp 17", n_kp=17)


def test_negative_lambda():
    _rejected(b"lambda -1", lam=-1.0)


def test_nothing_to_compute():
    _rejected(b"cov", cov=None, cov_newest=None)


def test_cross_needs_cov():
    _rejected(b"cross", cov=None, cross=FAKE, cov_newest=FAKE)


def test_workspace_too_small_or_missing():
    need = _lib.lib().pa_trajectory_marginals_workspace(3, 6)
    _rejected(b"workspace %d < %d" % (need - 1, need), ws_bytes=need - 1)
    _rejected(b"workspace", ws=None)


def test_info_is_required():
    _rejected(b"info", info=None)


@pytest.mark.parametrize("field", FACTORS[3:])
def test_missing_pair_factor(field):
    _rejected(b"dynamics / constant-velocity", **{field: None})


@pytest.mark.parametrize("field", ["r_proj", "j_proj"])
def test_missing_projection_factor(field):
    _rejected(b"projection", **{field: None})


def test_no_trajectories_is_a_no_op():
    rc, _ = _call(T=0, cov=None, info=None, ws=None, ws_bytes=0)
    assert rc == 0
