"""float64 numpy restatement of the Sobol queries on a conditioned view (ConditionedLCGP.sobol_indices / integrated_variance,
lcgp_condition_sobol_matrix_pairs), written from the formulas of DESIGN.md 4.24 on top of tests/sobol_uncertainty_ref.py.

Over the N = n + m centres xa = [x; xn] the view's posterior covariance of the continuous surface is c prod kappa - r_a^T Q' r_a:

  q_prime             Q' (N, N) = c^2 ([[D sr sr^T o A^-1, 0], [0, 0]] + P P^T), P = [-D sr o (W^T T_n^T); L_S^-T], T_n = L_S^-1 U_n
  mean_vectors        z' = z - D W^T (U_n^T w) and w = L_S^-T v: the view's mean is X_0 z' + c^x(x0, xn) w
  component           the sums, S0, C_u, IV, overall_var of one component for a given Q' (tests/sobol_uncertainty_ref.component
                      with the matrix handed in)
  ViewSobolOracleEngine   a numpy stand-in of the engine methods the view's queries call

Shared by the CPU tests (tests/test_condition_sobol_host.py) and the GPU tests (tests/test_gpu_condition_sobol.py)."""
import numpy as np
import scipy.linalg as sla

from tests import sobol_uncertainty_ref as uref
from tests.condition_marginal_ref import MargCondOracleEngine
from tests.test_sobol_host import SobolOracleEngine
from tests.test_sobol_uncertainty_host import UncertaintyOracleEngine


def q_prime(ainv, wtun, lsinv, sr, D, c):
    """ainv (n, n) the dense symmetric A^-1, wtun = W^T U_n^T (n, m) (W = L^-1 of A = L L^T), lsinv (m, m) = L_S^-1 lower
    triangular, sr (n), D and c = scale (1 - nt) of the component.  Returns (Q' (N, N), P (N, m))"""
    ainv, wtun, lsinv, sr = (np.asarray(a, np.float64) for a in (ainv, wtun, lsinv, sr))
    n, m = wtun.shape
    P = np.vstack([-D * sr[:, None] * (wtun @ lsinv.T), lsinv.T])           # W^T T_n^T = W^T U_n^T L_S^-T
    Q = P @ P.T
    Q[:n, :n] += D * np.outer(sr, sr) * ainv
    return c * c * Q, P


def wt_un_t(low, Un):
    """W^T U_n^T (n, m) from the Cholesky factor of A: L^-T U_n^T"""
    return sla.solve_triangular(np.asarray(low, np.float64).T, np.asarray(Un, np.float64).T, lower=False)


def mean_vectors(low, z, Un, LS, v, D):
    """(z' (n), w (m)) of one component"""
    w = sla.solve_triangular(LS.T, v, lower=False)
    return z - D * sla.solve_triangular(low.T, Un.T @ w, lower=False), w


def component(kernel, xa, th, Q, box):
    """th = (ell[d], scale, nug, D, ...), Q (N, N) the dense weight over the centres xa (N, d), c^2 included.  Returns the dict of
    sobol_uncertainty_ref.component: sums, s0, size, size0, prior, C, IV, overall_var, c"""
    xa = np.asarray(xa, np.float64)
    d = xa.shape[1]
    ell, scale, nug = np.asarray(th[:d], np.float64), th[d], th[d + 1]
    c = scale * (1.0 - nug / (1.0 + nug))
    sums, s0, size, size0 = uref.matrix_sums(kernel, xa, ell, box, Q)
    P, P0 = uref.prior_products(kernel, ell, box)
    return dict(c=c, Q=Q, sums=sums, s0=s0, size=size, size0=size0, prior=c * P, C=c * (P - P0) - sums, IV=c - s0 - sums[2 * d],
                overall_var=c * P0 - s0)


def view_q_prime(th, low, x, sr, Un, LS):
    """Q' of one component of a stand-in view (its Cholesky factor low of A, U_n and L_S), and the centres' count n"""
    d = x.shape[1]
    scale, nug, D = th[d], th[d + 1], th[d + 2]
    c = scale * (1.0 - nug / (1.0 + nug))
    n, m = len(x), len(LS)
    ainv = sla.cho_solve((low, True), np.eye(n))
    lsinv = sla.solve_triangular(LS, np.eye(m), lower=True)
    return q_prime(0.5 * (ainv + ainv.T), wt_un_t(low, Un), lsinv, sr, D, c)[0]


class ViewSobolOracleEngine(MargCondOracleEngine):
    """MargCondOracleEngine plus sobol_pairs, sobol_matrix_sums and the two methods a view's Sobol queries call, in numpy
    float64: condition_mean_vectors(state) and condition_sobol_matrix_sums(state, v, ell, box, ks)"""
    sobol_pairs = SobolOracleEngine.sobol_pairs
    sobol_matrix_sums = UncertaintyOracleEngine.sobol_matrix_sums

    def condition_mean_vectors(self, state):
        assert self.is_current(state['theta'])
        zs, ws = [], []
        for i, (th, low, z, b) in enumerate(self._state):
            Un, LS, v = state['state'][i]
            zp, w = mean_vectors(low, z, Un, LS, v, th[self.d + 2])
            zs.append(zp)
            ws.append(w)
        return np.stack(zs), np.stack(ws)

    def condition_sobol_matrix_sums(self, state, v, ell, box, ks):
        assert self.is_current(state['theta'])
        v, ell, box = (np.asarray(a, np.float64) for a in (v, ell, box))
        n, d, m = self.n, self.d, state['m']
        assert v.shape == (len(self._state), n + m) and ell.shape == (len(self._state), d) and box.shape == (2, d)
        xa = np.vstack([self.x, state['xn']])
        sr = np.ones(n) if self.sr is None else self.sr
        sums, s0 = np.zeros((len(ks), 2 * d + 1)), np.zeros(len(ks))
        for r, k in enumerate(np.asarray(ks)):
            th, low = self._state[k][0], self._state[k][1]
            np.testing.assert_array_equal(ell[k], th[:d])
            Un, LS, _ = state['state'][k]
            # (the engine's v holds c sr on the training rows and c on the new ones, D inside the matrices)
            D = th[d + 2]
            ainv = sla.cho_solve((low, True), np.eye(n))
            lsinv = sla.solve_triangular(LS, np.eye(m), lower=True)
            Pt = np.vstack([-D * (wt_un_t(low, Un) @ lsinv.T), lsinv.T])
            E = Pt @ Pt.T
            E[:n, :n] += D * ainv
            sums[r], s0[r], _, _ = uref.matrix_sums(self.kernel, xa, ell[k], box, v[k][:, None] * v[k][None, :] * E)
        np.testing.assert_allclose(v[:, :n], v[:, n:n + 1] * sr[None, :], rtol=1e-15)
        return sums, s0
