"""The objective of the fit as a differentiable torch float64 function of the flat CONSTRAINED parameter vector, for the
reference Hessian of LCGP.loss_hessian (a test helper, not a conftest).

`problem(o)` takes the constants of an OracleLCGP `o` (full or rep path, kernel 'matern32' / 'se' / 'matern52'); `objective(c,
prob)` restates oracle.nll_grad_full_chol / nll_grad_rep_chol on them with torch.linalg.cholesky:

    c = [ lLmb (q d) | lLmb0 (q) | lnugGPs (q) | lsigma2s (ns) ]          constrained values, the flat order of LCGP._get_flat
    f = sum_k [ 1/2 log det A_k - b_k^T (b_k - A_k^-1 b_k) / (2 D_k) ] + n/2 sum_a (t_a - 2 log std_a) + 1/2 sum_a ysq_a / sig_a^2
        - p/2 sum log r,            t = lsigma2s expanded over the error structure, sig_a = exp(t_a / 2) / std_a,
    A_k = I + D_k (C_k o s s^T),    b_k = sum_a phi_ak / sig_a Y_a,       (rep: Y = sqrt(r) o ybar, s = sqrt(r), f / n)

`hessian(c, prob)` is torch.autograd.functional.hessian of it; `value_and_grad(c, prob)` the value and the gradient.
tests/test_nll_hess_host.py ties value and gradient to the oracle (<= 1e-12 relative) and the Hessian to central differences
of the oracle's analytic gradient."""
import numpy as np
import torch

F64 = np.float64


def problem(o):
    """the constants of the objective of an OracleLCGP: a dict of numpy arrays and scalars"""
    rep = o.submethod == 'rep'
    if rep:
        sr = np.sqrt(np.asarray(o.r, F64))
        ybar_used = o.ybar_s if o.rep_standardize_ybar else o.ybar
        Y = ybar_used * sr[None, :]
        std = o.ybar_std[:, 0] if o.rep_standardize_ybar else np.ones(o.p, F64)
        x = o.x_unique_s
        sum_log_r = float(np.sum(np.log(o.r)))
    else:
        sr, Y, std, x, sum_log_r = None, o.y, np.ones(o.p, F64), o.x, 0.0
    return dict(x=np.asarray(x, F64), Y=np.asarray(Y, F64), sr=sr, std=np.asarray(std, F64), phi=np.asarray(o.phi, F64),
                D=np.asarray(o.diag_D, F64), es=[int(v) for v in o.diag_error_structure], n=int(o.n), d=int(o.d), p=int(o.p),
                q=int(o.q), rep=rep, sum_log_r=sum_log_r, kernel=o.kernel)


def flat_constrained(o):
    """the flat constrained vector of an OracleLCGP at its current parameters"""
    return np.concatenate([np.asarray(o.lLmb, F64).reshape(-1), np.asarray(o.lLmb0, F64), np.asarray(o.lnugGPs, F64),
                           np.asarray(o.lsigma2s, F64)])


def _c0(x, ell, kernel):
    s = torch.abs(x[:, None, :] - x[None, :, :]) / ell                 # (n, n, d)
    if kernel == 'se':
        return torch.exp(-0.5 * (s * s).sum(dim=2))
    if kernel == 'matern32':
        return torch.prod(1.0 + s, dim=2) * torch.exp(-s.sum(dim=2))
    assert kernel == 'matern52'
    return torch.prod(1.0 + s + s * s / 3.0, dim=2) * torch.exp(-s.sum(dim=2))


def objective(c, prob):
    """the objective (a 0-d float64 tensor) at the flat constrained vector c (a float64 tensor)"""
    n, d, p, q = prob['n'], prob['d'], prob['p'], prob['q']
    t64 = lambda a: torch.as_tensor(a, dtype=torch.float64)
    x, Y, std, phi, D = t64(prob['x']), t64(prob['Y']), t64(prob['std']), t64(prob['phi']), t64(prob['D'])
    s = torch.ones(n, dtype=torch.float64) if prob['sr'] is None else t64(prob['sr'])
    ell, scale, nug, ls2 = c[:q * d].reshape(q, d), c[q * d:q * d + q], c[q * d + q:q * d + 2 * q], c[q * d + 2 * q:]
    t = torch.repeat_interleave(ls2, torch.as_tensor(prob['es']))
    sig = torch.exp(0.5 * t) / std
    ysq = (Y * Y).sum(dim=1)
    f = 0.5 * (ysq / sig ** 2).sum() + n / 2.0 * (t - 2.0 * torch.log(std)).sum() - 0.5 * p * prob['sum_log_r']
    eye = torch.eye(n, dtype=torch.float64)
    for k in range(q):
        w = nug[k] / (1.0 + nug[k])
        C = scale[k] * ((1.0 - w) * _c0(x, ell[k], prob['kernel']) + w * eye)
        A = eye + D[k] * (C * s[:, None] * s[None, :])
        L = torch.linalg.cholesky(A)
        b = Y.T @ (phi[:, k] / sig)
        z = torch.cholesky_solve(b[:, None], L)[:, 0]
        f = f + torch.log(torch.diagonal(L)).sum() - (b @ (b - z)) / (2.0 * D[k])
    return f / n if prob['rep'] else f


def value_and_grad(c, prob):
    ct = torch.tensor(np.asarray(c, F64), requires_grad=True)
    f = objective(ct, prob)
    (g,) = torch.autograd.grad(f, ct)
    return float(f), g.numpy()


def hessian(c, prob):
    """(P, P) float64 numpy array: the autograd Hessian of objective() at c"""
    ct = torch.tensor(np.asarray(c, F64))
    return torch.autograd.functional.hessian(lambda v: objective(v, prob), ct).numpy()


def block_errors(H, Href, q, d):
    """max |H - Href| / max |Href| over the three block types separately -- the q dense (d + 2)^2 kernel blocks (and the zero
    cross-component kernel blocks with them), the kernel x noise border, the noise corner -- so that the large noise corner
    cannot hide a kernel block.  Flat order: lLmb (q d), lLmb0 (q), lnugGPs (q), lsigma2s."""
    nk = q * (d + 2)
    out = {}
    for name, (r, c) in dict(kernel=(slice(0, nk), slice(0, nk)), cross=(slice(0, nk), slice(nk, None)),
                             noise=(slice(nk, None), slice(nk, None))).items():
        out[name] = float(np.max(np.abs(H[r, c] - Href[r, c])) / np.max(np.abs(Href[r, c])))
    return out


def kernel_index(q, d):
    """(q, d + 2) int array: flat positions of component k's kernel parameters [ell_0 .. ell_{d-1}, scale, nug]"""
    idx = np.empty((q, d + 2), int)
    for k in range(q):
        idx[k, :d] = k * d + np.arange(d)
        idx[k, d] = q * d + k
        idx[k, d + 1] = q * d + q + k
    return idx
