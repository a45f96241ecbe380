"""TEST HELPER (not a test): references for pa_trajectory_marginals (include/perseus_amd.h).

`dense`: Sigma = np.linalg.inv(H + lam I) with H = A^T A from oracle.gn_ref.stack over a dict of
whitened factors (the device's own, as test_gn_gpu.py feeds the step's oracle), cut into the
diagonal blocks Sigma_{l,l} and the super-diagonal blocks Sigma_{l,l+1} (frame l on rows).

`recursion`: the block recursion the kernel runs (csrc/gn_marginals.hip), restated in numpy on
the blocks D_l, E_l of H:
    forward   S_0 = D_0 + lam I,  M_l = S_l^-1,  G_l = M_l E_l,  S_{l+1} = D_{l+1} + lam I - E_l^T G_l
    backward  Sigma_{L-1} = M_{L-1},  P_l = G_l Sigma_{l+1},
              Sigma_{l,l+1} = -P_l,  Sigma_l = M_l + P_l G_l^T
with every Sigma_l symmetrized as the kernel does.

`scaled_err`: the comparison's metric, per entry |got_ij - ref_ij| / sqrt(ref_ii ref_jj) with the
diagonals of the two frames' own marginal blocks (a correlation-scale error: variances in one
block span 1e-9 .. 1e9 at lam = 1e-9, where the unconstrained angular velocity sits at 1 / lam).
"""
from __future__ import annotations

import numpy as np

from oracle import gn_ref as G

NV = G.NV


def normal_matrices(f: dict, T: int, L: int, K: int):
    """H_t = A^T A per trajectory, (T, 12 L, 12 L)."""
    return np.stack([A.T @ A for A, _ in G.stack(f, T, L, K)])


def dense(f: dict, T: int, L: int, K: int, lam: float):
    """(cov (T, L, 12, 12), cross (T, L-1, 12, 12)) from the dense inverse."""
    cov, cross = [], []
    for H in normal_matrices(f, T, L, K):
        S = np.linalg.inv(H + lam * np.eye(H.shape[0]))
        D, E = G.blocks(S, L)
        cov.append(D)
        cross.append(E)
    return np.stack(cov), np.stack(cross)


def recursion(f: dict, T: int, L: int, K: int, lam: float):
    """The kernel's recursion in numpy: (cov, cross) as `dense`."""
    cov, cross = np.zeros((T, L, NV, NV)), np.zeros((T, L - 1, NV, NV))
    eye = lam * np.eye(NV)
    for t, H in enumerate(normal_matrices(f, T, L, K)):
        D, E = G.blocks(H, L)
        M, Gl = [], []
        S = D[0] + eye
        for l in range(L):
            M.append(np.linalg.inv(S))
            if l + 1 < L:
                Gl.append(M[l] @ E[l])
                S = D[l + 1] + eye - E[l].T @ Gl[l]
        sig = 0.5 * (M[L - 1] + M[L - 1].T)
        cov[t, L - 1] = sig
        for l in range(L - 2, -1, -1):
            P = Gl[l] @ sig
            cross[t, l] = -P
            u = M[l] + P @ Gl[l].T
            sig = 0.5 * (u + u.T)
            cov[t, l] = sig
    return cov, cross


def scaled_err(got_cov, got_cross, ref_cov, ref_cross):
    """Worst |delta_ij| / sqrt(ref_ii ref_jj) over (the cov blocks, the cross blocks); got_cross
    may be None (then the second figure is 0)."""
    ref_cov = np.asarray(ref_cov)
    T, L = ref_cov.shape[:2]
    sd = np.sqrt(np.einsum("tlii->tli", ref_cov))  # (T, L, 12)
    e_cov = np.abs(np.asarray(got_cov).reshape(T, L, NV, NV) - ref_cov) / (sd[..., :, None] * sd[..., None, :])
    e_cross = 0.0
    if got_cross is not None:
        d = np.abs(np.asarray(got_cross).reshape(T, L - 1, NV, NV) - np.asarray(ref_cross))
        e_cross = float((d / (sd[:, :-1, :, None] * sd[:, 1:, None, :])).max())
    return float(e_cov.max()), e_cross
