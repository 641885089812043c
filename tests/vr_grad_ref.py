"""float64 numpy restatement of the integrated variance reduction R(c) and of its gradient with respect to the candidate
(include/lcgp_hip.h: lcgp_variance_reduction_grad), for the CPU and GPU tests of variance_reduction_grad.
Every candidate is a new input (no nugget term in its cross row).  Three kernels; per component."""
import numpy as np
import scipy.linalg as sla
import torch

from tests.test_variance_reduction_host import VrOracleEngine, closed_form


def kern3(xa, xb, ell, kernel):
    """correlation without nugget: the product kernels of the library on inputs divided by ell"""
    S = np.abs(xa[:, None, :] / ell - xb[None, :, :] / ell)
    if kernel == 'se':
        return np.exp(-0.5 * np.sum(S * S, axis=2))
    if kernel == 'matern52':
        return np.prod(1.0 + S + S * S / 3.0, axis=2) * np.exp(-np.sum(S, axis=2))
    assert kernel == 'matern32', kernel
    return np.prod(1.0 + S, axis=2) * np.exp(-np.sum(S, axis=2))


def dkern3(xa, xb, ell, kernel):
    """(na, nb, d): derivative of kern3(xa, xb) with respect to xa[:, l]"""
    k0 = kern3(xa, xb, ell, kernel)[:, :, None]
    s = xa[:, None, :] / ell - xb[None, :, :] / ell
    a = np.abs(s)
    if kernel == 'se':
        f = s
    elif kernel == 'matern52':
        f = s * (1.0 + a) / (3.0 + 3.0 * a + s * s)
    else:
        f = s / (1.0 + a)
    return -k0 * f / ell


def value_and_grad(th, low, x, s, kernel, xr, xc, w, r):
    """R (n_cand,) and dR (n_cand, d) of one component: theta row th = (ell_1..d, scale, nug, D, ...), low = chol(I + D (C o s s^T)),
    x / xr / xc standardised training inputs / reference points / candidates, s the replicate scaling, w the weights"""
    d = x.shape[1]
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    coff = scale * (1.0 - nug / (1.0 + nug))
    kc = coff * kern3(xc, x, ell, kernel)
    dkc = coff * dkern3(xc, x, ell, kernel)
    uc = sla.solve_triangular(low, (kc * s[None, :]).T, lower=True).T
    ur = sla.solve_triangular(low, (coff * kern3(xr, x, ell, kernel) * s[None, :]).T, lower=True).T
    h = scale - D * np.sum(uc * uc, axis=1)
    den = np.maximum(h, 0.0) + 1.0 / (D * r)
    sig = coff * kern3(xc, xr, ell, kernel) - D * uc @ ur.T          # (n_cand, n_ref)
    dcr = coff * dkern3(xc, xr, ell, kernel)
    N = (sig * sig) @ w
    S = sig * w[None, :]
    Q = sla.solve_triangular(low, (S @ ur).T, lower=True, trans='T').T    # (S U_ref) L^-1
    V = sla.solve_triangular(low, uc.T, lower=True, trans='T').T          # U_cand L^-1
    dh = -2.0 * D * np.einsum('cjl,j,cj->cl', dkc, s, V)
    dh[h <= 0.0] = 0.0
    dN = 2.0 * (np.einsum('ctl,ct->cl', dcr, S) - D * np.einsum('cjl,j,cj->cl', dkc, s, Q))
    return N / den, dN / den[:, None] - (N / den ** 2)[:, None] * dh


class VrGradOracleEngine(VrOracleEngine):
    """VrOracleEngine plus variance_reduction_grad_block in numpy (and the Matern-5/2 kernel in variance_reduction_block)"""
    grad_calls = None

    def variance_reduction_block(self, x_cand_s, x_ref_s, w, match, r):
        if self.kernel != 'matern52' or (match is not None and np.any(np.asarray(match) >= 0)):
            return super().variance_reduction_block(x_cand_s, x_ref_s, w, match, r)
        return self.variance_reduction_grad_block(x_cand_s, x_ref_s, w, r)[0]

    def variance_reduction_grad_block(self, x_cand_s, x_ref_s, w, r):
        if self.grad_calls is not None:
            self.grad_calls.append(x_ref_s is None)
        xc = np.asarray(x_cand_s, np.float64)
        xr = xc if x_ref_s is None else np.asarray(x_ref_s, np.float64)
        s = np.ones(self.n) if self.sr is None else self.sr
        R = np.zeros((self.q_local, len(xc)))
        dR = np.zeros((self.q_local, len(xc), self.d))
        for i, (th, low, _, _) in enumerate(self._state):
            R[i], dR[i] = value_and_grad(th, low, self.x, s, self.kernel, xr, xc, np.asarray(w, np.float64), r)
            if self.kernel != 'matern52':       # the value in the arithmetic of variance_reduction_block: equal bit for bit
                R[i] = closed_form(th, low, self.x, s, self.kernel, xr, xc, np.asarray(w, np.float64), None, r)
        return torch.as_tensor(R), torch.as_tensor(dR)
