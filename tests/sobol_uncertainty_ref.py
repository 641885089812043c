"""float64 numpy restatement of what the emulator's own uncertainty adds to the closed-form Sobol variances, and of the exact
box-integrated posterior variance (LCGP.sobol_indices(uncertainty=True), LCGP.integrated_variance, lcgp_sobol_matrix_pairs),
written from the formulas of DESIGN.md 4.23 on top of tests/sobol_ref.py and tests/marginal_ref.py.

  matrix_sums         for one component and a dense symmetric weight Q (n, n): sum Q (M_u - M_0) for the 2 d + 1 subsets, S0 =
                      sum Q M_0, and the sizes of what they add up, sum |Q| (M_u + M_0) and sum |Q| M_0
  component           for one component from its theta row and a dense A^-1: the sums, S0, C_u = E[V_u] - V_u(mean), the
                      integrated variance IV, the variance of the box mean, the prior terms and the size
  dense_ainv          A^-1 of one component on the host, by a Cholesky solve and by an explicit inverse

Shared by the CPU tests (tests/test_sobol_uncertainty_host.py) and the GPU tests (tests/test_gpu_sobol_uncertainty.py)."""
import numpy as np
import scipy.linalg as sla

from tests import marginal_ref as mref
from tests import sobol_ref as ref


def matrix_sums(kernel, x, ell, box, Q):
    """x (n, d), ell (d), box (2, d) standardised, Q (n, n): (sums (2 d + 1), S0, size (2 d + 1), size0); the subsets in the
    order of sobol_ref.subset_products: {l}, all but l, all"""
    x, box, ell, Q = (np.asarray(a, np.float64) for a in (x, box, ell, Q))
    lo, hi = box[0], box[1]
    a = mref.I1(kernel, x, lo[None, :], hi[None, :], ell[None, :])                                  # (n, d)
    J = ref.pair_integral(kernel, lo, hi, x[:, None, :], ell[None, None, :], x[None, :, :], ell[None, None, :])
    M, M0 = ref.subset_products(J, a[:, None, :] * a[None, :, :])
    sums = np.einsum('ij,iju->u', Q, M - M0[..., None])
    size = np.einsum('ij,iju->u', np.abs(Q), M + M0[..., None])
    return sums, float(np.sum(Q * M0)), size, float(np.sum(np.abs(Q) * M0))


def prior_products(kernel, ell, box):
    """(P (2 d + 1), P0): prod over the inputs NOT in u of the double average I2_l, and prod over all inputs"""
    box = np.asarray(box, np.float64)
    d = box.shape[1]
    i2 = mref.I2(kernel, box[1] - box[0], np.asarray(ell, np.float64))
    P = np.ones(2 * d + 1)
    for l in range(d):
        P[l] = np.prod(np.delete(i2, l))
        P[d + l] = i2[l]
    return P, float(np.prod(i2))


def component(kernel, x, sr, th, ainv, box):
    """th = (ell[d], scale, nug, D, ...) the component's theta row, ainv (n, n) dense symmetric A^-1, sr (n).  Returns a dict:
    c = scale (1 - nt); Q = D c^2 sr sr^T o A^-1; sums, s0, size, size0 of matrix_sums; prior (2 d + 1) = c prod_{l not in u} I2_l;
    C (2 d + 1) = c (prod_{l not in u} I2_l - prod_l I2_l) - sums; IV = c - s0 - sums[all]; overall_var = c prod_l I2_l - s0"""
    x = np.asarray(x, np.float64)
    d = x.shape[1]
    ell, scale, nug, D = np.asarray(th[:d], np.float64), th[d], th[d + 1], th[d + 2]
    c = scale * (1.0 - nug / (1.0 + nug))
    v = c * np.asarray(sr, np.float64) * np.sqrt(D)
    Q = v[:, None] * v[None, :] * np.asarray(ainv, np.float64)
    sums, s0, size, size0 = matrix_sums(kernel, x, ell, box, Q)
    P, P0 = prior_products(kernel, ell, box)
    return dict(c=c, Q=Q, sums=sums, s0=s0, size=size, size0=size0, prior=c * P, C=c * (P - P0) - sums, IV=c - s0 - sums[2 * d],
                overall_var=c * P0 - s0)


def covariance_matrix(kernel, x, ell, scale, nug):
    """C = scale ((1 - nt) prod_l kappa(|x_il - x_jl| / ell_l) + nt I) over the standardised training inputs"""
    x = np.asarray(x, np.float64)
    nt = nug / (1.0 + nug)
    c0 = np.prod(mref.kappa(kernel, np.abs(x[:, None, :] - x[None, :, :]) / np.asarray(ell, np.float64)), axis=2)
    return scale * ((1.0 - nt) * c0 + nt * np.eye(x.shape[0]))


def dense_ainv(kernel, x, sr, th):
    """A = I + D (C o sr sr^T) of one component: (A^-1 by a Cholesky solve, A^-1 by an explicit inverse, the factor L)"""
    d = np.asarray(x).shape[1]
    sr = np.asarray(sr, np.float64)
    A = np.eye(len(sr)) + th[d + 2] * covariance_matrix(kernel, x, th[:d], th[d], th[d + 1]) * sr[:, None] * sr[None, :]
    low = np.linalg.cholesky(A)
    by_solve = sla.cho_solve((low, True), np.eye(len(sr)))
    return 0.5 * (by_solve + by_solve.T), np.linalg.inv(A), low
