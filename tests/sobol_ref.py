"""float64 numpy restatement of the closed-form Sobol indices (LCGP.sobol_indices, lcgp_sobol_pairs), written from the formulas
of DESIGN.md 4.22, and the quadrature they are checked against.

  moments             m_n(gamma, L) = int_0^L tau^n e^(-gamma tau) dtau, n = 0 .. nmax, without a division by gamma where gamma L
                      is small
  pair_integral       (1 / w) int_lo^hi kappa(|t - u| / a) kappa(|t - v| / b) dt: the box average of the product of two 1-D
                      kernel factors with different centres and length scales
  pair_sums           for one pair of components: D_u for the 2 d + 1 subsets (each input alone, all but each input, all
                      inputs), the two box means, and sum |w_i| |w'_i'| (M_u + M_0), the size of what D_u adds up
  indices             first-order and total indices, variances and means of the outputs from the pair sums
  piecewise_gauss_legendre   nodes and weights of the uniform measure on an interval, split at given break points

Shared by the CPU tests (tests/test_sobol_host.py) and the GPU tests (tests/test_gpu_sobol.py)."""
import numpy as np
from scipy.special import erf, erfc

from tests import marginal_ref as mref

SERIES_BELOW = 4.0          # gamma L below it: the all-positive series; from it on the forward recurrence (amplification < 1)
SERIES_STOP = 1e-18         # a term below this share of the sum ends the series
ROOT_HALF_PI = np.sqrt(0.5 * np.pi)


def moments(gamma, L, nmax):
    """m_n(gamma, L), n = 0 .. nmax, stacked on a new first axis; gamma >= 0, L >= 0 (arrays broadcast)"""
    gamma, L = np.broadcast_arrays(np.asarray(gamma, np.float64), np.asarray(L, np.float64))
    x = gamma * L
    small = x < SERIES_BELOW
    xs = np.where(small, x, 0.0)
    es = np.exp(-xs)
    g = np.where(small, 1.0, gamma)
    eL = np.exp(-g * L)
    out = np.empty((nmax + 1,) + x.shape)
    big = -np.expm1(-g * L) / g
    for n in range(nmax + 1):
        # m_n = e^(-gamma L) L^(n + 1) sum_j (gamma L)^j / ((n + 1) (n + 2) .. (n + 1 + j)): no cancellation, exact at gamma = 0
        term = np.full(x.shape, 1.0 / (n + 1.0))
        s = term.copy()
        for j in range(1, 200):
            term = term * xs / (n + 1.0 + j)
            s = s + term
            if np.all(term <= SERIES_STOP * s):
                break
        if n > 0:
            big = (n * big - L ** n * eL) / g
        out[n] = np.where(small, es * L ** (n + 1) * s, big)
    return out


def _poly(kernel, s0, al):
    """the coefficients in tau of P(s0 + al tau), P(s) = 1 + s (Matern-3/2), 1 + s + s^2 / 3 (Matern-5/2)"""
    if kernel == 'matern32':
        return [1.0 + s0, al]
    return [1.0 + s0 + s0 * s0 / 3.0, al * (1.0 + 2.0 * s0 / 3.0), al * al / 3.0]


def _pair_se(lo, hi, u, a, v, b):
    s2 = a * a + b * b
    pref = np.exp(-0.5 * (u - v) ** 2 / s2)
    sig = a * b / np.sqrt(s2)
    mu = (u * b * b + v * a * a) / s2
    z1, z2 = (mu - lo) / sig, (hi - mu) / sig              # the scaled distances of the centre to the two ends
    b1, b2 = np.abs(z1), np.abs(z2)
    inside = (z1 >= 0.0) & (z2 >= 0.0)
    bn, bf = np.minimum(b1, b2), np.maximum(b1, b2)
    F = lambda t: ROOT_HALF_PI * erf(t * np.sqrt(0.5))     # noqa: E731
    Fc = lambda t: ROOT_HALF_PI * erfc(t * np.sqrt(0.5))   # noqa: E731
    r = np.where(inside, F(b1) + F(b2), np.where(bn > 1.0, Fc(bn) - Fc(bf), F(bf) - F(bn)))
    return pref * sig * r / (hi - lo)


def pair_integral(kernel, lo, hi, u, a, v, b):
    """(1 / (hi - lo)) int_lo^hi kappa(|t - u| / a) kappa(|t - v| / b) dt (arrays broadcast).  SE: the product of two Gaussians
    is a Gaussian.  Matern: the centres ordered, the box split at those inside it, each of the three segments anchored at the
    end where the exponent is largest and integrated as e^(-s0a - s0b) sum_n q_n m_n(|c|, L)"""
    lo, hi, u, a, v, b = np.broadcast_arrays(*(np.asarray(t, np.float64) for t in (lo, hi, u, a, v, b)))
    if kernel == 'se':
        return _pair_se(lo, hi, u, a, v, b)
    assert kernel in ('matern32', 'matern52')
    swap = u > v
    u, v, a, b = np.where(swap, v, u), np.where(swap, u, v), np.where(swap, b, a), np.where(swap, a, b)
    cu, cv = np.clip(u, lo, hi), np.clip(v, lo, hi)
    nmax = 2 if kernel == 'matern32' else 4
    total = np.zeros(u.shape)
    for p, r, su, sv, at_r in ((lo, cu, -1.0, -1.0, np.ones(u.shape, bool)), (cu, cv, 1.0, -1.0, b < a),
                               (cv, hi, 1.0, 1.0, np.zeros(u.shape, bool))):
        L = r - p
        t0, e = np.where(at_r, r, p), np.where(at_r, -1.0, 1.0)
        s0a, s0b = np.abs(t0 - u) / a, np.abs(t0 - v) / b
        al, be = e * su / a, e * sv / b
        pa, pb = _poly(kernel, s0a, al), _poly(kernel, s0b, be)
        m = moments(al + be, L, nmax)
        seg = np.zeros(u.shape)
        for i, ca in enumerate(pa):
            for j, cb in enumerate(pb):
                seg = seg + ca * cb * m[i + j]
        total = total + np.exp(-s0a - s0b) * seg
    return total / (hi - lo)


def subset_products(J, A):
    """J, A (..., d): the factors of the integrated and of the averaged form per input -> (M (..., 2 d + 1), M0 (...)): M_u for
    u = {l} (l = 0 .. d - 1), all but l, all; M0 = prod A"""
    d = J.shape[-1]
    M = np.empty(J.shape[:-1] + (2 * d + 1,))
    for l in range(d):
        others = [m for m in range(d) if m != l]
        M[..., l] = J[..., l] * np.prod(A[..., others], axis=-1)
        M[..., d + l] = A[..., l] * np.prod(J[..., others], axis=-1)
    M[..., 2 * d] = np.prod(J, axis=-1)
    return M, np.prod(A, axis=-1)


def pair_sums(kernel, x, w1, ell1, w2, ell2, box):
    """one pair of components (weights w (n), length scales ell (d)) over the inputs x (n, d) and box (2, d), standardised:
    D (2 d + 1) = sum_ii' w1_i w2_i' (M_u - M_0), the means (m1, m2), and size (2 d + 1) = sum |w1_i| |w2_i'| (M_u + M_0)"""
    x, box = np.asarray(x, np.float64), np.asarray(box, np.float64)
    lo, hi = box[0], box[1]
    a1 = mref.I1(kernel, x, lo[None, :], hi[None, :], np.asarray(ell1)[None, :])            # (n, d)
    a2 = mref.I1(kernel, x, lo[None, :], hi[None, :], np.asarray(ell2)[None, :])
    J = pair_integral(kernel, lo, hi, x[:, None, :], np.asarray(ell1)[None, None, :], x[None, :, :], np.asarray(ell2)[None, None, :])
    A = a1[:, None, :] * a2[None, :, :]
    M, M0 = subset_products(J, A)
    ww = np.asarray(w1)[:, None] * np.asarray(w2)[None, :]
    D = np.einsum('ij,iju->u', ww, M - M0[..., None])
    size = np.einsum('ij,iju->u', np.abs(ww), M + M0[..., None])
    return D, (np.asarray(w1) @ np.prod(a1, axis=1), np.asarray(w2) @ np.prod(a2, axis=1)), size


def indices(D, means, W, scale, offset):
    """D (q, q, 2 d + 1) symmetric in its first two axes, means (q), the output map (W (q, p), scale (p), offset (p)) ->
    dict(first, total, variance, mean, first_variance, closed_variance)"""
    d = (D.shape[-1] - 1) // 2
    V = np.einsum('ka,la,klu->au', W, W, D) * (scale ** 2)[:, None]
    var = V[:, 2 * d]
    with np.errstate(divide='ignore', invalid='ignore'):
        first = np.where(var[:, None] == 0.0, np.nan, V[:, :d] / var[:, None])
        total = np.where(var[:, None] == 0.0, np.nan, 1.0 - V[:, d:2 * d] / var[:, None])
    return dict(first=first, total=total, variance=var, mean=offset + scale * (W.T @ means), first_variance=V[:, :d],
                closed_variance=V[:, d:2 * d])


def piecewise_gauss_legendre(m, lo, hi, breaks=(), max_len=None):
    """nodes and weights of the UNIFORM measure on [lo, hi] (they sum to 1): m Gauss-Legendre nodes on every piece between
    consecutive break points inside (lo, hi), pieces longer than max_len cut into equal parts no longer than it"""
    pts = np.unique(np.concatenate([[lo, hi], [t for t in np.asarray(breaks, np.float64).reshape(-1) if lo < t < hi]]))
    nodes, wts = [], []
    for p, r in zip(pts[:-1], pts[1:]):
        parts = 1 if max_len is None else max(1, int(np.ceil((r - p) / max_len)))
        cuts = np.linspace(p, r, parts + 1)
        for a, b in zip(cuts[:-1], cuts[1:]):
            t, w = mref.gauss_legendre(m, a, b)
            nodes.append(t)
            wts.append(w * (b - a) / (hi - lo))
    return np.concatenate(nodes), np.concatenate(wts)
