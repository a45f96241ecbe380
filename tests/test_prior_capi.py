"""The fixed-lag marginalization entry points through ctypes without a GPU (as
test_marginals_capi.py): every argument outside an entry point's limits returns PA_EINVAL with a
message before any launch, so the (never dereferenced) pointers here are made-up addresses."""
import ctypes as C

import pytest

from perseus_amd import _lib

FAKE = 0x1000  # a non-null address: validation never reads through it
FACTORS = ("r_proj", "j_proj", "status", "r_dyn", "j_dyn0", "j_dyn1", "j_dyn2", "j_dyn3", "r_cv", "j_cv0", "j_cv1")
MARG_TAIL = ("delta", "gn_info", "nvalid", "pose", "angvel", "vel", "info_out", "eta_out", "xbar_pose_out",
             "xbar_angvel_out", "xbar_vel_out", "minfo")
LIN_PTRS = ("info", "eta", "xbar_pose", "xbar_angvel", "xbar_vel", "pose", "angvel", "vel", "grad_out", "err_out")


def _marg(T=3, L=6, n_kp=8, lam=1e-3, prior_info_in=FAKE, prior_grad_in=FAKE, **kw):
    ptrs = [kw.get(k, FAKE) for k in FACTORS]
    tail = [kw.get(k, FAKE) for k in MARG_TAIL]
    L_ = _lib.lib()
    rc = L_.pa_window_marginalize(T, L, n_kp, *ptrs, prior_info_in, prior_grad_in, lam, *tail, None)
    return rc, L_.pa_last_error()


def _lin(T=3, L=6, frame=1, **kw):
    L_ = _lib.lib()
    rc = L_.pa_window_prior_linearize(T, L, frame, *[kw.get(k, FAKE) for k in LIN_PTRS], None)
    return rc, L_.pa_last_error()


def _rejected(call, prefix, needle, **kw):
    rc, msg = call(**kw)
    assert rc == -1, (rc, msg)
    assert msg.startswith(prefix) and needle in msg, msg


# ---------------------------------------------------------------- pa_window_marginalize
@pytest.mark.parametrize("kw,needle", [(dict(T=-1), b"T -1"), (dict(L=1), b"L 1"), (dict(n_kp=17), b"n_kp 17"),
                                       (dict(n_kp=-1), b"n_kp -1"), (dict(lam=-1.0), b"lambda -1")])
def test_marginalize_limits(kw, needle):
    _rejected(_marg, b"marginalize:", needle, **kw)


@pytest.mark.parametrize("field", FACTORS[3:])
def test_marginalize_missing_pair_factor(field):
    _rejected(_marg, b"marginalize:", b"dynamics / constant-velocity", **{field: None})


@pytest.mark.parametrize("field", ["r_proj", "j_proj"])
def test_marginalize_missing_projection_factor(field):
    _rejected(_marg, b"marginalize:", b"projection", **{field: None})
    rc, msg = _marg(T=0, n_kp=0, **{field: None})  # (n_kp = 0 needs none; T = 0 launches nothing)
    assert rc == 0, msg


def test_marginalize_prior_pair_goes_together():
    _rejected(_marg, b"marginalize:", b"together", prior_info_in=None)
    _rejected(_marg, b"marginalize:", b"together", prior_grad_in=None)


@pytest.mark.parametrize("field", MARG_TAIL[3:])
def test_marginalize_missing_window_or_output(field):
    _rejected(_marg, b"marginalize:", b"null", **{field: None})


def test_marginalize_no_trajectories_is_a_no_op():
    rc, msg = _marg(T=0, **{k: None for k in FACTORS + MARG_TAIL}, prior_info_in=None, prior_grad_in=None)
    assert rc == 0, msg


# ---------------------------------------------------------------- pa_window_prior_linearize
@pytest.mark.parametrize("kw,needle", [(dict(T=-1), b"T -1"), (dict(L=1), b"L 1"), (dict(frame=-1), b"frame -1"),
                                       (dict(frame=6), b"frame 6")])
def test_prior_linearize_limits(kw, needle):
    _rejected(_lin, b"prior linearize:", needle, **kw)


@pytest.mark.parametrize("field", LIN_PTRS[:-1])
def test_prior_linearize_missing_pointer(field):
    _rejected(_lin, b"prior linearize:", b"null", **{field: None})


def test_prior_linearize_no_trajectories_is_a_no_op():
    rc, msg = _lin(T=0, **{k: None for k in LIN_PTRS})
    assert rc == 0, msg


# ---------------------------------------------------------------- the _prior siblings
def _gn_prior(prior_info=FAKE, prior_grad=FAKE, T=3):
    L_ = _lib.lib()
    rc = L_.pa_trajectory_gn_step_prior(T, 6, 8, *[FAKE] * 11, 1e-3, None, None, None, FAKE, FAKE, FAKE, 1 << 40,
                                        prior_info, prior_grad, None)
    return rc, L_.pa_last_error()


def _marginals_prior(prior_info=FAKE, prior_grad=FAKE, T=3):
    L_ = _lib.lib()
    rc = L_.pa_trajectory_marginals_prior(T, 6, 8, *[FAKE] * 11, 1e-3, FAKE, None, None, FAKE, FAKE, 1 << 40,
                                          prior_info, prior_grad, None)
    return rc, L_.pa_last_error()


@pytest.mark.parametrize("call,prefix", [(_gn_prior, b"gn:"), (_marginals_prior, b"marginals:")])
def test_sibling_prior_pair_goes_together(call, prefix):
    _rejected(call, prefix, b"together", prior_info=None)
    _rejected(call, prefix, b"together", prior_grad=None)
    rc, msg = call(T=0)
    assert rc == 0, msg


# ---------------------------------------------------------------- the tick siblings
def _tick_args():
    """A pa_traj_args that passes pose_tick_check (made-up addresses, never dereferenced)."""
    a = _lib.TrajArgs()
    a.T, a.L, a.n_kp, a.H, a.W, a.dt = 3, 6, 8, 256, 256, 0.1
    for name, typ in _lib.TrajArgs._fields_:
        if typ is C.c_void_p:
            setattr(a, name, FAKE)
    return a


def _tick_prior(a, pi, pg):
    L_ = _lib.lib()
    return L_.pa_window_pose_tick_prior(C.byref(a), FAKE, 1e-2, FAKE, FAKE, FAKE, pi, pg, None), L_.pa_last_error()


def _pre_prior(a, pi, pg):
    L_ = _lib.lib()
    return L_.pa_window_pose_tick_pre_prior(C.byref(a), 1e-2, FAKE, 1 << 40, pi, pg, None), L_.pa_last_error()


def _reduce_prior(a, pi, pg):
    L_ = _lib.lib()
    return L_.pa_window_pose_tick_reduce_prior(C.byref(a), 1e-2, FAKE, 1 << 40, pi, pg, None), L_.pa_last_error()


@pytest.mark.parametrize("call,prefix", [(_tick_prior, b"pose tick:"), (_pre_prior, b"pose tick pre:"),
                                         (_reduce_prior, b"pose tick reduce:")])
def test_tick_sibling_prior_pair_goes_together(call, prefix):
    for pi, pg in ((FAKE, None), (None, FAKE)):
        rc, msg = call(_tick_args(), pi, pg)
        assert rc == -1 and msg.startswith(prefix) and b"together" in msg, (rc, msg)
    a = _tick_args()
    a.L = 25  # the parents' checks come first, unchanged
    rc, msg = call(a, FAKE, FAKE)
    assert rc == -1 and b"L 25" in msg, (rc, msg)
    a = _tick_args()
    a.T = 0
    rc, msg = call(a, FAKE, None)
    assert rc == 0, msg


def test_traj_args_and_lm_take_no_prior():
    """The prior travels beside pa_traj_args (the _prior siblings), never inside it, and the
    Levenberg-Marquardt entry points have no sibling: they cannot be handed a prior."""
    assert not any(n.startswith("prior") for n, _ in _lib.TrajArgs._fields_)
    L_ = _lib.lib()
    for name in ("pa_trajectory_lm_solve_prior", "pa_window_lm_solve_prior"):
        assert not hasattr(L_, name)
