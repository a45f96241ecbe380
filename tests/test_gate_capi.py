"""pa_window_predict and pa_keypoint_gate through ctypes without a GPU (as test_timed_capi.py):
what the entry points reject returns PA_EINVAL with a message before any launch, so the (never
dereferenced) pointers here are made-up addresses."""
import ctypes as C
import os
import subprocess

import pytest

from perseus_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000


def _predict(T=3, L=6, Q=2, pose=FAKE, angvel=FAKE, vel=FAKE, cov=FAKE, cross=FAKE, cov_info=FAKE, q_diag=FAKE,
             tau=FAKE, vel_frame=0, pose_out=FAKE, cov_out=FAKE):
    L_ = _lib.lib()
    rc = L_.pa_window_predict(T, L, Q, pose, angvel, vel, cov, cross, cov_info, q_diag, tau, vel_frame, pose_out,
                              cov_out, None)
    return rc, L_.pa_last_error()


def _gate(T=3, n_kp=8, y_new=FAKE, pose_pred=FAKE, pose_stride=12, cov_pred=FAKE, corners=FAKE, K=FAKE, tcam=None,
          isig_proj=FAKE, chi2=13.816, min_pass=4, nvalid=None, min_frames=3, mask=FAKE, mask_stride=1, d2=None,
          zhat=None, ginfo=FAKE):
    L_ = _lib.lib()
    rc = L_.pa_keypoint_gate(T, n_kp, 256, 256, y_new, pose_pred, pose_stride, cov_pred, corners, K, tcam, isig_proj,
                             chi2, min_pass, nvalid, min_frames, mask, mask_stride, d2, zhat, ginfo, None)
    return rc, L_.pa_last_error()


def test_symbols_resolve_and_constants():
    L_ = _lib.lib()
    assert L_.pa_window_predict and L_.pa_keypoint_gate
    assert (_lib.GATE_APPLIED, _lib.GATE_FEW, _lib.GATE_NOCOV, _lib.GATE_YOUNG) == (0, 1, 2, 3)
    hdr = open(os.path.join(ROOT, "include", "perseus_amd.h")).read()
    for name, val in (("APPLIED", 0), ("FEW", 1), ("NOCOV", 2), ("YOUNG", 3)):
        assert f"#define PA_GATE_{name} {val}\n" in hdr


@pytest.mark.parametrize("kw,needle", [
    (dict(T=-1), b"T=-1"), (dict(Q=0), b"Q=0"), (dict(L=1), b"L=1"),
    (dict(cov=None), b"cov and cross"), (dict(cross=None), b"cov and cross"),
    (dict(cov=None, cross=None), b"cov_out needs"),
    (dict(L=2), b"L >= 3"),
    (dict(vel_frame=7), b"vel_frame"),
    (dict(pose=None), b"null"), (dict(angvel=None), b"null"), (dict(vel=None), b"null"), (dict(tau=None), b"null"),
    (dict(pose_out=None), b"null"),
])
def test_predict_rejects(kw, needle):
    rc, msg = _predict(**kw)
    assert rc == -1 and needle in msg, (rc, msg)
    assert msg.startswith(b"window predict:") or needle == b"vel_frame", msg  # (vel_frame: factors.py's own words)


def test_predict_optional_pointers_and_no_op():
    # T = 0 is a no-op whatever the pointers; the optional ones do not matter to the checks
    assert _predict(T=0, pose=None, angvel=None, vel=None, tau=None, pose_out=None, cov=None, cross=None,
                    cov_out=None)[0] == 0
    assert _predict(T=0)[0] == 0
    # the pose-only form at L = 2 passes every check up to the launch: rejected only for a reason
    # that comes after them (here: none is left, so T = 0 stands in for the launch)
    assert _predict(T=0, L=2, cov=None, cross=None, cov_out=None, cov_info=None, q_diag=None)[0] == 0


@pytest.mark.parametrize("kw,needle", [
    (dict(T=-1), b"T=-1"), (dict(n_kp=0), b"n_kp=0"), (dict(n_kp=33), b"n_kp=33"),
    (dict(chi2=0.0), b"chi2"), (dict(chi2=-1.0), b"chi2"), (dict(chi2=float("inf")), b"chi2"),
    (dict(chi2=float("nan")), b"chi2"),
    (dict(min_pass=-1), b"min_pass=-1"), (dict(pose_stride=11), b"pose_stride=11"),
    (dict(mask_stride=0), b"mask_stride=0"),
    (dict(y_new=None), b"null"), (dict(pose_pred=None), b"null"), (dict(cov_pred=None), b"null"),
    (dict(corners=None), b"null"), (dict(K=None), b"null"), (dict(isig_proj=None), b"null"),
    (dict(mask=None), b"null"), (dict(ginfo=None), b"null"),
])
def test_gate_rejects(kw, needle):
    rc, msg = _gate(**kw)
    assert rc == -1 and msg.startswith(b"keypoint gate:") and needle in msg, (rc, msg)


def test_gate_no_trajectories_is_a_no_op():
    assert _gate(T=0)[0] == 0
    assert _gate(T=0, y_new=None, pose_pred=None, cov_pred=None, corners=None, K=None, isig_proj=None, mask=None,
                 ginfo=None, pose_stride=72, mask_stride=6)[0] == 0
    assert _gate(T=0, n_kp=33)[0] == -1  # the shape checks come first


def test_traj_args_has_the_size_it_had(tmp_path):
    """pa_traj_args is untouched: the ctypes mirror's size is the C compiler's, and the value it had
    before the two entry points were appended to the header."""
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "perseus_amd.h"\nint main(void){\n'
                   '  printf("%zu\\n", sizeof(pa_traj_args));\n  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = int(subprocess.check_output([str(exe)]).split()[0])
    assert got == C.sizeof(_lib.TrajArgs) == 312
