"""The Matern-5/2 product kernel for the numpy oracle, as a test helper (not a conftest).

The committed oracle knows 'matern32' and 'se'; any other kernel name falls through to Matern-3/2 there.  This module
restates its three kernel-specific functions -- `matern32`, `matern32_c0_and_s`, `_kernel_param_grads` -- with a
'matern52' branch written from the definition (no reference to the HIP code) and delegates every other name to the
originals.  `patch(monkeypatch)` / the `patched()` context manager put them into `oracle.lcgp_oracle` for the duration
of a test, after which `OracleLCGP(kernel='matern52')` is the Matern-5/2 model in every form the oracle has.

Definition (the reference's Matern-3/2 convention carried over, no sqrt(5) factor):

    C0 = prod_j (1 + S_j + S_j^2 / 3) exp(-sum_j S_j),      S_j = |x1_j - x2_j| / ell_j
    C  = scale ((1 - nt) C0 + nt [x1 is x2]),               nt = lnug / (1 + lnug)
    dC0/d ell_j = C0 S_j^2 (1 + S_j) / ((3 + 3 S_j + S_j^2) ell_j)

which is the textbook Matern-5/2 at lengthscale sqrt(5) ell_j per dimension.
"""
import contextlib

import numpy as np
import scipy.linalg as sla

from oracle import lcgp_oracle as orc

F64 = np.float64
_ORIG = dict(matern32=orc.matern32, matern32_c0_and_s=orc.matern32_c0_and_s, _kernel_param_grads=orc._kernel_param_grads)


def c0_matern52(a, b):
    """prod_j (1 + S_j + S_j^2 / 3) exp(-sum_j S_j) for inputs already divided by ell: (n1, d), (n2, d) -> (n1, n2)."""
    s = np.abs(np.asarray(a, F64)[:, None, :] - np.asarray(b, F64)[None, :, :])
    return np.prod(1.0 + s + s * s / 3.0, axis=2) * np.exp(-s.sum(axis=2))


def matern32(x1, x2, llmb, llmb0, lnug, diag_only=False, kernel='matern32'):
    if kernel != 'matern52':
        return _ORIG['matern32'](x1, x2, llmb, llmb0, lnug, diag_only, kernel)
    x1 = np.asarray(x1, F64)
    x2 = np.asarray(x2, F64)
    assert x1.ndim == 2 and x2.ndim == 2 and x1.shape[1] == x2.shape[1]
    llmb = np.asarray(llmb, F64).reshape(-1)
    if diag_only:
        assert np.all(np.abs(x1 - x2) <= (1e-6 + 1e-6 * np.abs(x2)))
        return float(llmb0) * np.ones(x1.shape[0], F64)
    c0 = c0_matern52(x1 / llmb, x2 / llmb)
    nt = lnug / (1.0 + lnug)
    same = (x1.shape == x2.shape) and bool(np.all(x1 == x2))
    c = (1.0 - nt) * c0 + (nt * np.eye(x1.shape[0]) if same else 0.0)
    return float(llmb0) * c


def matern32_c0_and_s(x, ell, kernel='matern32'):
    if kernel != 'matern52':
        return _ORIG['matern32_c0_and_s'](x, ell, kernel)
    a = x / ell
    s_all = np.abs(a.T[:, :, None] - a.T[:, None, :])            # (d, n, n)
    return c0_matern52(a, a), s_all


def _kernel_param_grads(low, c0, s_all, z, dk, ell, scale, nug, sr=None, kernel='matern32'):
    if kernel != 'matern52':
        return _ORIG['_kernel_param_grads'](low, c0, s_all, z, dk, ell, scale, nug, sr, kernel)
    n = low.shape[0]
    ainv = sla.cho_solve((low, True), np.eye(n))
    gmat = 0.5 * dk * ainv - 0.5 * np.outer(z, z)
    if sr is not None:
        gmat = gmat * sr[:, None] * sr[None, :]
    nt = nug / (1.0 + nug)
    g_ell = np.empty(len(ell), F64)
    for j in range(len(ell)):
        sj = s_all[j]
        w = sj * sj * (1.0 + sj) / ((3.0 + 3.0 * sj + sj * sj) * ell[j])
        g_ell[j] = np.sum(gmat * (scale * (1.0 - nt) * c0 * w))
    tr_g = np.trace(gmat)
    g_c0 = np.sum(gmat * c0)
    g_scale = (1.0 - nt) * g_c0 + nt * tr_g
    g_nug = scale * (tr_g - g_c0) / (1.0 + nug) ** 2
    return g_ell, g_scale, g_nug


def patch(monkeypatch):
    """Puts the three functions into oracle.lcgp_oracle until the test ends (pytest's monkeypatch undoes it)."""
    monkeypatch.setattr(orc, 'matern32', matern32)
    monkeypatch.setattr(orc, 'matern32_c0_and_s', matern32_c0_and_s)
    monkeypatch.setattr(orc, '_kernel_param_grads', _kernel_param_grads)


@contextlib.contextmanager
def patched():
    """The same as a context manager, for code outside a test function."""
    saved = {k: getattr(orc, k) for k in _ORIG}
    orc.matern32, orc.matern32_c0_and_s, orc._kernel_param_grads = matern32, matern32_c0_and_s, _kernel_param_grads
    try:
        yield orc
    finally:
        for k, v in saved.items():
            setattr(orc, k, v)


def kernel_matrix(x1s, x2s, ell, scale, nug, same=False):
    """C (with the nugget term on the diagonal when `same`) for STANDARDISED inputs: what the brute-force checks build."""
    c0 = c0_matern52(np.asarray(x1s, F64) / ell, np.asarray(x2s, F64) / ell)
    nt = nug / (1.0 + nug)
    c = (1.0 - nt) * c0
    if same:
        c = c + nt * np.eye(c.shape[0])
    return scale * c
