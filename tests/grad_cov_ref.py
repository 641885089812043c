"""float64 numpy restatement of the posterior covariance of the latent gradient (LCGP.predict_grad_cov, lcgp_predict_gradcov)
for one component, written from the formulas of DESIGN.md 4.10, by two routes:

  latent_grad_cov     the closed form: the prior term from the kernel's curvature at zero distance, the data term from the
                      rows P = L^-1 (d_l X)^T as tests/test_predict_hess_host.latent_hessians forms them
  stencil_grad_cov    a mixed central difference of the posterior covariance FUNCTION Sigma(x, x') at pairs of distinct
                      points (only off-diagonal entries of a joint covariance, so no nugget term enters); it knows nothing of
                      h, psi or kappa

Shared by the CPU tests (tests/test_grad_cov_host.py) and the GPU tests (tests/_grad_cov_gpu_worker.py)."""
import numpy as np
import scipy.linalg as sla

from tests.test_predict_hess_host import _cross

KAPPA = {'matern32': 1.0, 'se': 1.0, 'matern52': 1.0 / 3.0}        # -f''(0) of the 1-D factor


def _h(s, kernel):
    a = np.abs(s)
    if kernel == 'matern32':
        return s / (1.0 + a)
    if kernel == 'se':
        return s
    assert kernel == 'matern52'
    return s * (1.0 + a) / (3.0 + 3.0 * a + a * a)


def latent_mean_grad(x0s, x, sr, th, z, kernel):
    """dghat (n0, d): sum_j d_l c(i, j) sr_j z_j"""
    d = x.shape[1]
    ell, scale, nug = th[:d], th[d], th[d + 1]
    c = _cross(x0s, x, ell, scale, nug, kernel)
    s = (x0s[:, None, :] - x[None, :, :]) / ell
    dc = -c[:, :, None] * _h(s, kernel) / ell
    return np.einsum('ijl,j->il', dc, sr * z)


def latent_grad_cov(x0s, x, sr, th, low, kernel):
    """Gamma (n0, d, d) = delta_lm c(0) kappa / ell_l^2 - D P_il . P_im with respect to the standardised x0s; c(0) is the
    kernel between two DISTINCT inputs at zero distance (the continuous part of the prior variance, without the nugget)"""
    n0, d = x0s.shape
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    c = _cross(x0s, x, ell, scale, nug, kernel)
    s = (x0s[:, None, :] - x[None, :, :]) / ell
    dc = -c[:, :, None] * _h(s, kernel) / ell                       # (n0, n, d)
    dX = (dc * sr[None, :, None]).transpose(0, 2, 1).reshape(n0 * d, -1)        # row i d + l
    P = sla.solve_triangular(low, dX.T, lower=True).T.reshape(n0, d, -1)
    c_zero = _cross(x0s[:1], np.repeat(x0s[:1], 2, axis=0), ell, scale, nug, kernel)[0, 0]   # (1 x 2: never "the same set")
    prior = np.diag(c_zero * KAPPA[kernel] / ell ** 2)
    return prior[None, :, :] - D * np.einsum('ilj,imj->ilm', P, P)


def posterior_cov_pairs(xa, xb, x, sr, th, low, kernel):
    """Sigma(xa_i, xb_i) (n0) for pairs of distinct points: c(xa_i, xb_i) - D X(xa_i) A^-1 X(xb_i)^T"""
    d = x.shape[1]
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    assert not np.any(np.all(xa == xb, axis=1))
    prior = np.array([_cross(xa[i:i + 1], np.stack([xb[i], xb[i]]), ell, scale, nug, kernel)[0, 0] for i in range(xa.shape[0])])
    ua = sla.solve_triangular(low, (_cross(xa, x, ell, scale, nug, kernel) * sr[None, :]).T, lower=True)
    ub = sla.solve_triangular(low, (_cross(xb, x, ell, scale, nug, kernel) * sr[None, :]).T, lower=True)
    return prior - D * np.sum(ua * ub, axis=0)


def stencil(sigma, x0s, h):
    """Gamma[i, l, m] ~ [S(x + h e_l, x + 2h e_m) - S(x + h e_l, x - 2h e_m) - S(x - h e_l, x + 2h e_m) + S(x - h e_l, x - 2h e_m)]
    / (8 h^2) for sigma(xa, xb) -> the covariance of the pairs (xa_i, xb_i)"""
    n0, d = x0s.shape
    out = np.zeros((n0, d, d))
    for l in range(d):
        el = np.zeros(d)
        el[l] = h
        for m in range(d):
            em = np.zeros(d)
            em[m] = 2.0 * h
            out[:, l, m] = (sigma(x0s + el, x0s + em) - sigma(x0s + el, x0s - em)
                            - sigma(x0s - el, x0s + em) + sigma(x0s - el, x0s - em)) / (8.0 * h * h)
    return out


def stencil_grad_cov(x0s, x, sr, th, low, kernel, h):
    return stencil(lambda a, b: posterior_cov_pairs(a, b, x, sr, th, low, kernel), x0s, h)
