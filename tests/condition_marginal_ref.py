"""float64 numpy restatement of the box averages on a conditioned view and of the covariance between two box-averaged rows
(lcgp_condition_predict_marginal), for one component, built on tests/marginal_ref.py:

  row_prior           prior_k(i, r): the prior covariance of the averages of row i and of the reference row r
  marginal_cov        gcov (n0): prior_k(i, r) - D Ubar_i . Ubar_r of the fitted model
  augmented           the component's training set augmented by a view's runs: (xa, sa, Cholesky factor, z)
  view_marginal       ghat', gvar'[, gcov'] by the rank-m correction of the closed form (what the device computes)
  MargCondOracleEngine  a numpy stand-in of HotPathEngine.predict_marginal_block(x0s, mask, box, state, ref)

Shared by the CPU tests (tests/test_condition_marginal_host.py) and the GPU tests (tests/test_gpu_condition_marginal.py)."""
import numpy as np
import scipy.linalg as sla
import torch

from tests import marginal_ref as mref
from tests.test_condition_host import CondOracleEngine
from tests.test_predict_hess_host import _cross


def row_prior(x0s, mask, xr, mr, box, th, kernel):
    """(n0) scale (1 - nt) prod_l f_l: kappa between the kept values, I1 at the kept value where one row integrates l, I2
    where both do.  No nugget term, also for two rows with empty masks at the same input"""
    d = len(xr)
    ell, scale, nug = th[:d], th[d], th[d + 1]
    mask, mr = np.asarray(mask, bool), np.asarray(mr, bool)
    x0z, xrz = np.where(mask, 0.0, x0s), np.where(mr, 0.0, xr)
    lo, hi = box[0][None, :], box[1][None, :]
    both_kept = mref.kappa(kernel, np.abs(x0z - xrz[None, :]) / ell)
    i_kept = mref.I1(kernel, x0z, lo, hi, ell[None, :])                   # l integrated in r
    r_kept = mref.I1(kernel, xrz[None, :], lo, hi, ell[None, :])          # l integrated in i
    dbl = mref.I2(kernel, box[1] - box[0], ell)[None, :]
    f = np.where(mask, np.where(mr[None, :], dbl, r_kept), np.where(mr[None, :], i_kept, both_kept))
    return scale * (1.0 - nug / (1.0 + nug)) * np.prod(f, axis=1)


def marginal_cov(x0s, mask, xr, mr, box, x, sr, th, low, kernel):
    """gcov (n0) of the fitted model: the posterior covariance of every row's average with the reference row's"""
    d = x.shape[1]
    Xi = mref.marginal_rows(x0s, mask, box, x, sr, th, kernel)[0]
    Xr = mref.marginal_rows(xr[None, :], np.asarray(mr, bool)[None, :], box, x, sr, th, kernel)[0]
    ui, ur = sla.solve_triangular(low, Xi.T, lower=True), sla.solve_triangular(low, Xr.T, lower=True)
    return row_prior(x0s, mask, xr, mr, box, th, kernel) - th[d + 2] * (ui.T @ ur)[:, 0]


def augmented(th, x, s, Y, kernel, xn_s, snew, ycol):
    """(xa, sa, low, z) of one component on the training set augmented by the new columns (tests/test_condition_host.
    dense_augmented's matrices): low the Cholesky factor of A = I + D (C o sa sa^T), z = A^-1 b"""
    xa, sa, Ya = np.vstack([x, xn_s]), np.r_[s, snew], np.hstack([Y, ycol])
    d = x.shape[1]
    ell, scale, nug, D, psi = th[:d], th[d], th[d + 1], th[d + 2], th[d + 3:]
    Cm = _cross(xa, xa, ell, scale, nug, kernel)
    Cm[np.arange(len(xa)), np.arange(len(xa))] = scale
    low = np.linalg.cholesky(np.eye(len(xa)) + D * Cm * np.outer(sa, sa))
    z = sla.solve_triangular(low.T, sla.solve_triangular(low, Ya.T @ psi, lower=True), lower=False)
    return xa, sa, low, z


def _widened(x0s, mask, box, x, sr, th, low, kernel, xn, Un, LS):
    """Xbar (n0, n), Ubar (n0, n), Tbar (n0, m) and the priors (n0) of masked rows on a view"""
    d = x.shape[1]
    X, prior = mref.marginal_rows(x0s, mask, box, x, sr, th, kernel)
    U = sla.solve_triangular(low, X.T, lower=True).T
    Cx = mref.marginal_rows(x0s, mask, box, xn, np.ones(len(xn)), th, kernel)[0]           # no sr, no nugget
    T = sla.solve_triangular(LS, (Cx - th[d + 2] * U @ Un.T).T, lower=True).T
    return X, U, T, prior


def view_marginal(th, low, z, x, sr, kernel, xn, Un, LS, v, x0s, mask, box, rrow=None):
    """ghat', gvar' (n0) of one component by the rank-m correction (closed_form_predict with both row kernels masked), and with
    rrow = (xr, mr) gcov' = prior(i, r) - D Ubar_i . Ubar_r - Tbar_i . Tbar_r as a third result"""
    d = x.shape[1]
    D = th[d + 2]
    X, U, T, prior = _widened(x0s, mask, box, x, sr, th, low, kernel, xn, Un, LS)
    out = (X @ z + T @ v, prior - D * np.sum(U * U, axis=1) - np.sum(T * T, axis=1))
    if rrow is None:
        return out
    xr, mr = np.asarray(rrow[0], np.float64), np.asarray(rrow[1], bool)
    _, Ur, Tr, _ = _widened(xr[None, :], mr[None, :], box, x, sr, th, low, kernel, xn, Un, LS)
    return out + (row_prior(x0s, mask, xr, mr, box, th, kernel) - D * (U @ Ur[0]) - T @ Tr[0],)


class MargCondOracleEngine(CondOracleEngine):
    """CondOracleEngine plus predict_marginal_block(x0s, mask, box, state=None, ref=None) in numpy float64"""

    def predict_marginal_block(self, x0s, mask, box, state=None, ref=None):
        x0s, mask, box = np.asarray(x0s, np.float64), np.asarray(mask, bool), np.asarray(box, np.float64)
        assert mask.shape == x0s.shape and box.shape == (2, self.d) and np.all(np.isfinite(x0s[~mask]))
        assert state is None or self.is_current(state['theta'])
        sr = np.ones(self.n) if self.sr is None else self.sr
        rows = []
        for i, (th, low, z, b) in enumerate(self._state):
            if state is None:
                r = mref.latent_marginal(x0s, mask, box, self.x, sr, th, low, z, self.kernel)
                if ref is not None:
                    r = r + (marginal_cov(x0s, mask, np.asarray(ref[0], np.float64), ref[1], box, self.x, sr, th, low,
                                          self.kernel),)
            else:
                r = view_marginal(th, low, z, self.x, sr, self.kernel, state['xn'], *state['state'][i], x0s, mask, box, ref)
            rows.append(r)
        return torch.as_tensor(np.stack([[r[j] for r in rows] for j in range(len(rows[0]))]))

