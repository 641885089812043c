"""float64 numpy restatement of the exact box ALC (LCGP.integrated_variance_reduction, lcgp_box_alc), written from the formulas
of DESIGN.md 4.26 on top of tests/sobol_ref.py and tests/marginal_ref.py: how much the box-integrated posterior variance of one
latent component drops if the simulator ran r more times at a candidate.

  cross_rows          the candidates' cross-covariance rows X_c as variance_reduction forms them (nugget entry at `match`)
  terms               for one component and a dense A^-1: the three terms of the numerator, den, R, size and gvar
  augmented           the training set with one candidate taken in (a new row, or r more replicates of a matched input)
  output_map          R (q, n_cand) -> Delta (p, n_cand)

Shared by the CPU tests (tests/test_box_alc_host.py) and the GPU tests (tests/test_gpu_box_alc.py)."""
import numpy as np

from tests import marginal_ref as mref
from tests import sobol_ref as ref


def _kernel_rows(kernel, xa, xb, ell):
    """prod_l kappa(|xa_l - xb_l| / ell_l): (len(xa), len(xb))"""
    return np.prod(mref.kappa(kernel, np.abs(xa[:, None, :] - xb[None, :, :]) / ell), axis=2)


def cross_rows(kernel, x, sr, th, xc, match=None):
    """X_c (n_cand, n) = c r(x_c) o sr, plus scale nt sr_i at column i = match[c] where match[c] >= 0 (the rep path's
    candidate that IS unique input i)"""
    x, xc, sr = (np.asarray(a, np.float64) for a in (x, xc, sr))
    d = x.shape[1]
    ell, scale, nug = np.asarray(th[:d], np.float64), th[d], th[d + 1]
    nt = nug / (1.0 + nug)
    X = scale * (1.0 - nt) * _kernel_rows(kernel, xc, x, ell) * sr[None, :]
    if match is not None:
        for j, i in enumerate(match):
            if i >= 0:
                X[j, i] += scale * nt * sr[i]
    return X


def terms(kernel, x, sr, th, ainv, box, xc, match=None, r=1):
    """th = (ell[d], scale, nug, D, ...) the component's theta row, ainv (n, n) dense symmetric A^-1, sr (n), box (2, d) and xc
    (n_cand, d) standardised.  Returns a dict of (n_cand,) arrays:
        t0 = c^2 m_cc        t1 = 2 c b_c . m_c        t2 = b_c^T M b_c        b_c = D c sr o (A^-1 X_c^T)
        gvar = scale - D X_c A^-1 X_c^T       den = max(gvar, 0) + 1 / (D r)
        R = (t0 - t1 + t2) / den              size = (t0 + 2 c |b_c| . m_c + |b_c|^T M |b_c|) / den
    and c = scale (1 - nt)."""
    x, xc, sr, box, ainv = (np.asarray(a, np.float64) for a in (x, xc, sr, box, ainv))
    d = x.shape[1]
    ell, scale, nug, D = np.asarray(th[:d], np.float64), th[d], th[d + 1], th[d + 2]
    c = scale * (1.0 - nug / (1.0 + nug))
    lo, hi = box[0], box[1]
    e3 = ell[None, None, :]
    M = np.prod(ref.pair_integral(kernel, lo, hi, x[:, None, :], e3, x[None, :, :], e3), axis=2)            # (n, n)
    mc = np.prod(ref.pair_integral(kernel, lo, hi, xc[:, None, :], e3, x[None, :, :], e3), axis=2)          # (n_cand, n)
    mcc = np.prod(ref.pair_integral(kernel, lo, hi, xc, ell[None, :], xc, ell[None, :]), axis=1)            # (n_cand,)
    X = cross_rows(kernel, x, sr, th, xc, match)
    V = X @ ainv
    b = D * c * sr[None, :] * V
    gvar = scale - D * np.sum(X * V, axis=1)
    den = np.maximum(gvar, 0.0) + 1.0 / (D * r)
    t0 = c * c * mcc
    t1 = 2.0 * c * np.sum(b * mc, axis=1)
    t2 = np.einsum('ci,ij,cj->c', b, M, b)
    ab = np.abs(b)
    size = (t0 + 2.0 * c * np.sum(ab * mc, axis=1) + np.einsum('ci,ij,cj->c', ab, M, ab)) / den
    return dict(c=c, t0=t0, t1=t1, t2=t2, gvar=gvar, den=den, R=(t0 - t1 + t2) / den, size=size)


def augmented(x, sr, xc_row, match_i, r):
    """(x', sr') after r runs at the candidate: r more replicates of unique input match_i (sr' = sqrt(sr^2 + r) there), or a
    new row with sr = sqrt(r)"""
    x, sr = np.asarray(x, np.float64), np.asarray(sr, np.float64)
    if match_i is not None and match_i >= 0:
        s2 = sr.copy()
        s2[match_i] = np.sqrt(sr[match_i] ** 2 + r)
        return x, s2
    return np.vstack([x, np.asarray(xc_row, np.float64)[None, :]]), np.r_[sr, np.sqrt(float(r))]


def output_map(R, W, scale, outputs=None):
    """Delta_a(c) = scale_a^2 sum_k W[k, a]^2 R_k(c): R (q, n_cand), W (q, p), scale (p)"""
    delta = (np.asarray(W) ** 2).T @ np.asarray(R) * (np.asarray(scale) ** 2)[:, None]
    return delta if outputs is None else delta[list(outputs)]
