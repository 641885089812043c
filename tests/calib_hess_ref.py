"""numpy restatements behind the tests of CalibrationTarget.loglik_hess / lcgp_calib_hess_rows, none of them used by the product:
  (i)  dense_hess: the Hessian of the p-space log density in the inputs straight from Sigma_i = Phi_s diag(gvar) Phi_s^T + Lambda,
       its first and second derivatives and r = t - Phi_s ghat (no Woodbury identity, no B);
  (ii) rows2: the second-order row formulas of include/lcgp_hip.h on top of calib_ref.rows, in np.float64 or np.longdouble, with
       the sum of the absolute values of each quantity's terms (what the GPU tests' tolerances are built from)."""
import numpy as np

from tests import calib_ref as ref


def tri_index(d):
    """(il, im): row-major over the lower triangle, entry (l, m <= l) at l (l + 1) / 2 + m"""
    return np.tril_indices(d)


def unpack_lower(packed, d):
    il, im = tri_index(d)
    full = np.empty(packed.shape[:-1] + (d, d), packed.dtype)
    full[..., il, im] = packed
    full[..., im, il] = packed
    return full


def dense_hess(phi_s, t, lam, ghat, gvar, dghat, dgvar, d2ghat, d2gvar, inv_range=None):
    """(i): (d2ll (n0, d, d), mag (n0, d, d)) from the latent predictions (q, n0), Jacobians (q, n0, d) and FULL Hessians
    (q, n0, d, d).  With a = Sigma^-1 r, mu_l = Phi_s dghat_l, S_l = Phi_s diag(dgvar_l) Phi_s^T and a_m = d a / d x_m =
    -Sigma^-1 (mu_m + S_m a):
        d2ll_lm = a_m.mu_l + a.mu_lm + a_m^T S_l a + 1/2 a^T S_lm a + 1/2 tr(Sigma^-1 S_m Sigma^-1 S_l) - 1/2 tr(Sigma^-1 S_lm)
    mag is the sum of the absolute values of these six terms (the GPU tests' error bound is built from it)."""
    q, n0, d = dghat.shape
    ir = np.ones(d) if inv_range is None else np.asarray(inv_range, np.float64)
    out, mag = np.zeros((n0, d, d)), np.zeros((n0, d, d))
    for i in range(n0):
        sig = phi_s @ (np.maximum(gvar[:, i], 0.0)[:, None] * phi_s.T) + lam
        si = np.linalg.inv(sig)
        si = 0.5 * (si + si.T)
        a = np.linalg.solve(sig, t - phi_s @ ghat[:, i])
        mu = phi_s @ dghat[:, i, :]                                                    # (|O|, d)
        S = [phi_s @ (dgvar[:, i, l][:, None] * phi_s.T) for l in range(d)]
        am = [-si @ (mu[:, m] + S[m] @ a) for m in range(d)]
        for l in range(d):
            for m in range(d):
                mu2 = phi_s @ d2ghat[:, i, l, m]
                S2 = phi_s @ (d2gvar[:, i, l, m][:, None] * phi_s.T)
                terms = np.array([am[m] @ mu[:, l], a @ mu2, am[m] @ S[l] @ a, 0.5 * a @ S2 @ a,
                                  0.5 * np.sum((si @ S[m] @ si) * S[l]), -0.5 * np.sum(si * S2)])
                out[i, l, m] = ir[l] * ir[m] * terms.sum()
                mag[i, l, m] = abs(ir[l] * ir[m]) * np.abs(terms).sum()
    return out, mag


def dense_B(phi_s, lam, gvar):
    """(n0, q, q): Phi_s^T Sigma_i^-1 Phi_s from the dense covariance"""
    return np.stack([phi_s.T @ np.linalg.solve(phi_s @ (np.maximum(gvar[:, i], 0.0)[:, None] * phi_s.T) + lam, phi_s)
                     for i in range(gvar.shape[1])])


def rows2(ghat, gvar, dghat, dgvar, d2ghat, d2gvar, M, b, c0, lognorm, inv_range=None, dtype=np.float64, order=None):
    """(ii): calib_ref.rows' dict plus B (n0, q, q) and d2ll (n0, d (d + 1) / 2), the packed lower triangle as
    lcgp_calib_hess_rows writes it, from PACKED latent Hessians (q, n0, tri); every operation in `dtype`.  order: a permutation of
    the components in which everything is evaluated (results are returned in the caller's order): the CPU tests evaluate the
    float64 restatement in reverse order and require it to stay inside the tolerance built from the forward order.
    B_abs = |M| + |R|^T |R| and d2ll_abs are the sums of the absolute values of the terms with s, v and B EXPANDED into their own
    terms (s_abs, v_abs, B_abs in the place of |s|, |v|, |B|): d2ll is a polynomial in s, v and B, each of them a sum that
    cancels, so, as the docstring of calib_ref.rows explains for v and dll, taking the computed s, v, B for exact atoms is no
    error bound.  Whether the expansion is right is checked on the CPU (tests/test_calibration_hess_host.py): were the reversed
    float64 evaluation to leave the tolerance, the expansion would be wrong, not the factor 4."""
    dt = dtype
    q, n0 = np.shape(ghat)
    if order is not None:
        o = np.asarray(order)
        inv = np.argsort(o)
        res = rows2(np.asarray(ghat)[o], np.asarray(gvar)[o], np.asarray(dghat)[o], np.asarray(dgvar)[o], np.asarray(d2ghat)[o],
                    np.asarray(d2gvar)[o], np.asarray(M)[np.ix_(o, o)], np.asarray(b)[o], c0, lognorm, inv_range, dt)
        for k in ('s', 's_abs', 'v', 'v_abs'):
            res[k] = res[k][inv]
        for k in ('B', 'B_abs'):
            res[k] = res[k][:, inv][:, :, inv]
        return res
    out = ref.rows(ghat, gvar, dghat, dgvar, M, b, c0, lognorm, inv_range, dt)
    ghat, gvar, M, dghat, dgvar, d2ghat, d2gvar = (np.asarray(a, np.float64).astype(dt)
                                                   for a in (ghat, gvar, M, dghat, dgvar, d2ghat, d2gvar))
    d = dghat.shape[2]
    tri = d * (d + 1) // 2
    il, im = tri_index(d)
    ir = np.ones(d, dt) if inv_range is None else np.asarray(inv_range, np.float64).astype(dt)
    scale = ir[il] * ir[im]
    half = dt(0.5)
    out.update({k: np.zeros((n0, q, q), dt) for k in ('B', 'B_abs')})
    out.update({k: np.zeros((n0, tri), dt) for k in ('d2ll', 'd2ll_abs')})
    aM = np.abs(M)
    for i in range(n0):
        h = np.sqrt(np.maximum(gvar[:, i], dt(0)))
        L = ref._cholesky(np.eye(q, dtype=dt) + h[:, None] * M * h[None, :], dt)
        R = ref._lower_solve(L, h[:, None] * M, dt)
        B = M - R.T @ R
        Ba = aM + np.abs(R).T @ np.abs(R)
        s, v, sa, va = out['s'][:, i], out['v'][:, i], out['s_abs'][:, i], out['v_abs'][:, i]
        P, V = dghat[:, i, :], dgvar[:, i, :]
        aP, aV = np.abs(P), np.abs(V)
        cross = P.T @ B @ (s[:, None] * V)
        full = (-(P.T @ B @ P) - cross - cross.T + V.T @ (half * B * B - (s[:, None] * s[None, :]) * B) @ V)
        across = aP.T @ Ba @ (sa[:, None] * aV)
        afull = aP.T @ Ba @ aP + across + across.T + aV.T @ (half * Ba * Ba + (sa[:, None] * sa[None, :]) * Ba) @ aV
        first = (s[:, None] * d2ghat[:, i, :] + v[:, None] * d2gvar[:, i, :]).sum(axis=0, dtype=dt)
        afirst = (sa[:, None] * np.abs(d2ghat[:, i, :]) + va[:, None] * np.abs(d2gvar[:, i, :])).sum(axis=0, dtype=dt)
        out['B'][i], out['B_abs'][i] = B, Ba
        out['d2ll'][i] = scale * (first + full[il, im])
        out['d2ll_abs'][i] = np.abs(scale) * (afirst + afull[il, im])
    return out


def row_tolerances2(ref64, refld):
    """calib_ref.row_tolerances (its rule, unchanged: 4 x max(error of the float64 restatement against the longdouble one,
    eps64 x the longdouble sum of absolute terms), elementwise) extended to B and d2ll.  Nothing of the code under test enters."""
    eps = np.finfo(np.float64).eps
    tol = ref.row_tolerances(ref64, refld)
    for k in ('B', 'd2ll'):
        err = np.abs(ref64[k].astype(np.longdouble) - refld[k])
        tol[k] = (4 * np.maximum(err, eps * refld[k + '_abs'])).astype(np.float64)
    return tol


def rows2_as_host_stub(blk, jac, hess, M, b, inv_range, c0, lognorm, want_sens, want_B):
    """rows2() behind the signature of LCGP._calib_hess_rows_device (CPU torch tensors in, numpy out): what the CPU tests install
    in place of the row kernels"""
    blk, jac, hess = blk.numpy(), jac.numpy(), hess.numpy()
    res = rows2(blk[0], blk[1], jac[0], jac[1], hess[0], hess[1], M.numpy(), b.numpy(), c0, lognorm, inv_range.numpy())
    return (res['ll'], res['dll'], res['d2ll'], (np.stack([res['s'], res['v']]) if want_sens else None),
            (res['B'] if want_B else None))


N0, D = 257, 6                                  # the synthetic block of tests/test_gpu_calibration.py
ROW_QS = (1, 2, 8, 9, 17, 64)
WIDE = dict(q=9, n0=5, d=40)


def hess_inputs(q, deficient):
    """tests/test_gpu_calibration._inputs(q, deficient) (its block of N0 = 257 rows, D = 6, rows 0..5 carrying gvar = 0 and
    -1e-18) plus packed latent Hessians d2ghat, d2gvar (q, N0, 21) drawn the same way"""
    from tests.test_gpu_calibration import _inputs
    inp = _inputs(q, deficient)
    rng = np.random.default_rng(7000 + 10 * q + deficient)
    tri = D * (D + 1) // 2
    inp['d2ghat'], inp['d2gvar'] = rng.standard_normal((q, N0, tri)), rng.standard_normal((q, N0, tri))
    return inp


def wide_inputs():
    """the one wide case, d = 40 at q = 9, n0 = 5 (the lanes stride over l in one pass of 64; tri = 820), drawn as _inputs
    draws: M of full rank, row 0 with gvar = 0, row 1 with -1e-18"""
    q, n0, d = WIDE['q'], WIDE['n0'], WIDE['d']
    rng = np.random.default_rng(4009)
    A = rng.standard_normal((q + 3, q)) / np.sqrt(q + 3)
    M = A.T @ A
    ghat, gvar = rng.standard_normal((q, n0)), rng.uniform(0.0, 1.0, (q, n0))
    gvar[:, 0], gvar[::2, 1] = 0.0, -1e-18
    tri = d * (d + 1) // 2
    return dict(ghat=ghat, gvar=gvar, dghat=rng.standard_normal((q, n0, d)), dgvar=rng.standard_normal((q, n0, d)),
                d2ghat=rng.standard_normal((q, n0, tri)), d2gvar=rng.standard_normal((q, n0, tri)), M=0.5 * (M + M.T),
                b=rng.standard_normal(q), c0=float(rng.uniform(1, 5)), lognorm=float(rng.standard_normal()),
                inv_range=rng.uniform(0.2, 4.0, d))


def rows2_of(inp, **kw):
    return rows2(inp['ghat'], inp['gvar'], inp['dghat'], inp['dgvar'], inp['d2ghat'], inp['d2gvar'], inp['M'], inp['b'], inp['c0'],
                 inp['lognorm'], inp['inv_range'], **kw)
