"""float64 numpy restatement of the box-averaged predictions (LCGP.predict_marginal / main_effects, lcgp_predict_marginal) for
one component, written from the formulas of DESIGN.md 4.11, and the quadrature they are checked against.

  F, G, Fc            int_0^b kappa, int_0^b u kappa(u) du, int_b^inf kappa of the 1-D kernel factor kappa(u), u = |t - x| / ell
  I1, I2              the single and the double average of the factor over [lo, hi]
  marginal_rows       the averaged cross-covariance rows Xbar (n0, n) and the averaged priors (n0)
  latent_marginal     ghat, gvar (n0) of one component
  continuous_cov      the posterior covariance of the continuous surface over a set of points (no nugget on its diagonal)
  gauss_legendre      nodes and weights of the uniform measure on an interval; tensor_rule: their tensor product

Shared by the CPU tests (tests/test_marginal_host.py) and the GPU tests (tests/test_gpu_marginal.py)."""
import numpy as np
import scipy.linalg as sla
from scipy.special import erf, erfc

SERIES_BELOW = 0.5          # the closed forms of the Matern pair cancel for small b (G ~ b^2 / 2 from O(1) terms)
SERIES_TERMS = 20           # (b^20 / 20! < 1e-24 below 1/2)
ROOT_HALF_PI = np.sqrt(0.5 * np.pi)


def kappa(kernel, u):
    """the 1-D factor of the product kernel at scaled distance u >= 0"""
    if kernel == 'matern32':
        return (1.0 + u) * np.exp(-u)
    if kernel == 'se':
        return np.exp(-0.5 * u * u)
    assert kernel == 'matern52'
    return (1.0 + u + u * u / 3.0) * np.exp(-u)


def _series(kernel, b):
    """F, G from kappa(u) = sum_m f(m) (-u)^m / m!,  f(m) = 1 - m (Matern-3/2),  (m - 1)(m - 3) / 3 (Matern-5/2)"""
    t, sf, sg = np.ones_like(b), np.zeros_like(b), np.zeros_like(b)
    for m in range(SERIES_TERMS):
        f = 1.0 - m if kernel == 'matern32' else (m - 1.0) * (m - 3.0) / 3.0
        sf = sf + t * f / (m + 1.0)
        sg = sg + t * f / (m + 2.0)
        t = t * (-b / (m + 1.0))
    return b * sf, b * b * sg


def _closed(kernel, b):
    e, em = np.exp(-b), -np.expm1(-b)
    if kernel == 'matern32':
        return 2.0 * em - b * e, 3.0 * em - b * (3.0 + b) * e
    return (8.0 / 3.0) * em - b * (5.0 + b) / 3.0 * e, 5.0 * em - b * (5.0 + b * (2.0 + b / 3.0)) * e


def _FG(kernel, b):
    b = np.asarray(b, np.float64)
    if kernel == 'se':
        return ROOT_HALF_PI * erf(b * np.sqrt(0.5)), -np.expm1(-0.5 * b * b)
    small = b < SERIES_BELOW
    Fs, Gs = _series(kernel, np.where(small, b, 0.0))
    Fc_, Gc = _closed(kernel, np.where(small, 1.0, b))
    return np.where(small, Fs, Fc_), np.where(small, Gs, Gc)


def F(kernel, b):
    return _FG(kernel, b)[0]


def G(kernel, b):
    return _FG(kernel, b)[1]


def Fc(kernel, b):
    b = np.asarray(b, np.float64)
    if kernel == 'matern32':
        return (2.0 + b) * np.exp(-b)
    if kernel == 'se':
        return ROOT_HALF_PI * erfc(b * np.sqrt(0.5))
    return (8.0 + b * (5.0 + b)) / 3.0 * np.exp(-b)


def I1(kernel, x, lo, hi, ell):
    """(1 / w) int_lo^hi kappa(|t - x| / ell) dt, x inside the box, on its edge or outside (arrays broadcast).  Outside, once
    the nearer end is more than one length scale away, the difference is taken between the tails: the F saturate there"""
    x, lo, hi, ell = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (x, lo, hi, ell)))
    a1, a2 = x - lo, hi - x
    b1, b2 = np.abs(a1) / ell, np.abs(a2) / ell
    inside = (a1 >= 0.0) & (a2 >= 0.0)
    bn, bf = np.minimum(b1, b2), np.maximum(b1, b2)
    r = np.where(inside, F(kernel, b1) + F(kernel, b2),
                 np.where(bn > 1.0, Fc(kernel, bn) - Fc(kernel, bf), F(kernel, bf) - F(kernel, bn)))
    return ell / (hi - lo) * r


def I2(kernel, w, ell):
    """(1 / w^2) int int kappa(|t - t'| / ell) dt dt' over [0, w]^2 = 2 ell [w F(a) - ell G(a)] / w^2, a = w / ell"""
    a = np.asarray(w, np.float64) / np.asarray(ell, np.float64)
    Fa, Ga = _FG(kernel, a)
    return 2.0 * (Fa / a - Ga / (a * a))


def marginal_rows(x0s, mask, box, x, sr, th, kernel):
    """Xbar (n0, n) and prior (n0) of one component: th = its theta row (ell[d], scale, nug, ...), mask (n0, d) True =
    integrated, box (2, d) = [lo; hi], all in standardised inputs.  A row with an empty mask keeps the prior `scale`"""
    d = x.shape[1]
    ell, scale, nug = th[:d], th[d], th[d + 1]
    nt = nug / (1.0 + nug)
    mask = np.asarray(mask, bool)
    x0z = np.where(mask, 0.0, x0s)
    fac = kappa(kernel, np.abs(x0z[:, None, :] - x[None, :, :]) / ell)                  # (n0, n, d)
    avg = I1(kernel, x, box[0][None, :], box[1][None, :], ell[None, :])               # (n, d)
    fac = np.where(mask[:, None, :], avg[None, :, :], fac)
    X = scale * (1.0 - nt) * np.prod(fac, axis=2) * sr[None, :]
    dbl = I2(kernel, box[1] - box[0], ell)                                              # (d)
    prior = scale * (1.0 - nt) * np.prod(np.where(mask, dbl[None, :], 1.0), axis=1)
    return X, np.where(mask.any(axis=1), prior, scale)


def latent_marginal(x0s, mask, box, x, sr, th, low, z, kernel):
    """ghat, gvar (n0): Xbar z and prior - D |L^-1 Xbar^T|^2, low the Cholesky factor of A = I + D (C o sr sr^T)"""
    d = x.shape[1]
    X, prior = marginal_rows(x0s, mask, box, x, sr, th, kernel)
    u = sla.solve_triangular(low, X.T, lower=True)
    return X @ z, prior - th[d + 2] * np.sum(u * u, axis=0)


def continuous_cov(pts, x, sr, th, low, kernel):
    """(m, m) posterior covariance of the continuous surface over pts, and its posterior mean weights' rows X (m, n): the
    prior is scale (1 - nt) prod kappa, also on the diagonal (no nugget there)"""
    d = x.shape[1]
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    c = scale * (1.0 - nug / (1.0 + nug))
    X = c * np.prod(kappa(kernel, np.abs(pts[:, None, :] - x[None, :, :]) / ell), axis=2) * sr[None, :]
    K = c * np.prod(kappa(kernel, np.abs(pts[:, None, :] - pts[None, :, :]) / ell), axis=2)
    u = sla.solve_triangular(low, X.T, lower=True)
    return K - D * (u.T @ u), X


def gauss_legendre(m, lo, hi):
    """m nodes on [lo, hi] and weights of the UNIFORM measure on it (they sum to 1)"""
    t, w = np.polynomial.legendre.leggauss(m)
    return lo + 0.5 * (hi - lo) * (t + 1.0), 0.5 * w


def tensor_rule(m, box, dims):
    """nodes (m^len(dims), len(dims)) and weights of the tensor rule over the dimensions `dims` of box (2, d)"""
    rules = [gauss_legendre(m, box[0][l], box[1][l]) for l in dims]
    nodes = np.stack([g.reshape(-1) for g in np.meshgrid(*[r[0] for r in rules], indexing='ij')], axis=1)
    wts = np.ones(1)
    for r in rules:
        wts = (wts[:, None] * r[1][None, :]).reshape(-1)
    return nodes, wts
