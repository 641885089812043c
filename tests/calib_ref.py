"""numpy restatements behind the calibration tests (LCGP.calibration / lcgp_calib_rows), none of them used by the product:
  (i)  dense_loglik: the log density in p-space from the dense covariance, its gradient from d Sigma = Phi_s diag(dgvar) Phi_s^T
       (no Woodbury identity anywhere);
  (ii) fold / rows: the q-space host preparation and the row formulas of include/lcgp_hip.h, in np.float64 or np.longdouble,
       with the sum of the absolute values of each quantity's terms (what the GPU tests' tolerances are built from)."""
import numpy as np

LOG2PI = float(np.log(2.0 * np.pi))


def observation(model, y_obs, obs_var, include_noise=True):
    """(obs mask, Phi_s (|O|, q), t (|O|,), Lambda (|O|, |O|)) of a model's output map, dense, float64"""
    W, noise, scale, offset = model._output_map()
    p = W.shape[1]
    y = np.asarray(y_obs, np.float64)
    obs = ~np.isnan(y)
    ov = np.asarray(obs_var, np.float64)
    if ov.ndim == 0:
        ov = np.full(p, float(ov))
    S = np.diag(ov) if ov.ndim == 1 else ov
    lam = S[np.ix_(obs, obs)] + (np.diag((scale ** 2 * noise)[obs]) if include_noise else 0.0)
    phi_s = (W[:, obs] * scale[obs][None, :]).T
    return obs, phi_s, (y - offset)[obs], lam


def dense_loglik(phi_s, t, lam, ghat, gvar, dghat=None, dgvar=None, inv_range=None):
    """(i): ll (n0,), the (n0, |O|, |O|) covariances and, with the latent Jacobians (q, n0, d), dll (n0, d); also the quadratic
    form and the log determinant per row (the GPU tests' error bound is built from them)"""
    n0 = ghat.shape[1]
    m = phi_s.shape[0]
    ll, quad, logdet = np.zeros(n0), np.zeros(n0), np.zeros(n0)
    cov = np.zeros((n0, m, m))
    dll = None if dghat is None else np.zeros((n0, dghat.shape[2]))
    for i in range(n0):
        sig = phi_s @ (np.maximum(gvar[:, i], 0.0)[:, None] * phi_s.T) + lam
        cov[i] = sig
        r = t - phi_s @ ghat[:, i]
        low = np.linalg.cholesky(sig)
        z = np.linalg.solve(low, r)
        quad[i], logdet[i] = z @ z, 2.0 * np.sum(np.log(np.diag(low)))
        ll[i] = -0.5 * (quad[i] + logdet[i] + m * LOG2PI)
        if dll is not None:
            a = np.linalg.solve(sig, r)
            si = np.linalg.inv(sig)
            for l in range(dll.shape[1]):
                dmean = phi_s @ dghat[:, i, l]
                dsig = phi_s @ (dgvar[:, i, l][:, None] * phi_s.T)
                dll[i, l] = a @ dmean + 0.5 * a @ dsig @ a - 0.5 * np.sum(si * dsig)
            if inv_range is not None:
                dll[i] *= inv_range
    return ll, cov, dll, quad, logdet


def fold(phi_s, t, lam):
    """(M, b, c0, lognorm) of the host preparation, float64, from the dense Lambda"""
    low = np.linalg.cholesky(lam)
    A = np.linalg.solve(low, phi_s)
    z = np.linalg.solve(low, t)
    M = A.T @ A
    return 0.5 * (M + M.T), A.T @ z, float(z @ z), 2.0 * float(np.sum(np.log(np.diag(low)))) + len(t) * LOG2PI


def _cholesky(K, dt):
    q = K.shape[0]
    L = np.zeros((q, q), dt)
    for j in range(q):
        c = K[j:, j] - (L[j:, :j] * L[j, :j][None, :]).sum(axis=1, dtype=dt)
        L[j, j] = np.sqrt(c[0])
        L[j + 1:, j] = c[1:] / L[j, j]
    return L


def _lower_solve(L, B, dt):
    X = np.zeros(B.shape, dt)
    cols = int(np.prod(B.shape[1:]))
    for j in range(L.shape[0]):
        X[j] = (B[j] - (L[j, :j, None] * X[:j].reshape(j, cols)).sum(axis=0, dtype=dt).reshape(B.shape[1:])) / L[j, j]
    return X


def _upper_solve(U, B, dt):
    q = U.shape[0]
    X = np.zeros(B.shape, dt)
    for j in range(q - 1, -1, -1):
        X[j] = (B[j] - np.sum(U[j, j + 1:] * X[j + 1:], dtype=dt)) / U[j, j]
    return X


def rows(ghat, gvar, dghat, dgvar, M, b, c0, lognorm, inv_range=None, dtype=np.float64):
    """(ii): the row formulas as include/lcgp_hip.h states them, every operation in `dtype`.  Returns a dict with ll (n0,),
    s, v (q, n0), dll (n0, d) (None without Jacobians) and, under the same names with the suffix `_abs`, the sum of the absolute
    values of the terms each quantity is the sum of.  v and dll are polynomials in s (v_k = 1/2 s_k^2 - 1/2 T_kk, dll = sum_k s_k
    dghat + v_k dgvar) and s_k is itself a sum that cancels, so their terms are those of the EXPANDED sums: (sum_i t_i)^2 has the
    terms t_i t_j, absolute sum s_abs^2, and s_k dghat the terms t_i dghat, absolute sum s_abs |dghat|.  Taking the computed s_k
    and v_k for exact atoms instead (terms 1/2 s_k^2, s_k dghat, v_k dgvar) is no error bound: the rounding of s, eps s_abs, enters
    v as |s_k| eps s_abs, which 1/2 eps s_k^2 does not cover when s_abs >> |s_k|.  Measured on the MI355X with those atoms, the
    kernel (whose largest errors over largest values, 1e-16 to 1.5e-15, equal the float64 numpy evaluation's) sat at up to
    3.7 x the tolerance in v (396 of 16448 entries at q = 64) and 1.9 x in dll, and so does float64 numpy with the components in
    reverse order (v at q = 17: 1.03 x); ll and s, plain sums, never exceeded 0.41 x."""
    dt = dtype
    ghat, gvar, M, b = (np.asarray(a, np.float64).astype(dt) for a in (ghat, gvar, M, b))
    c0, lognorm = dt(c0), dt(lognorm)
    q, n0 = ghat.shape
    grad = dghat is not None
    if grad:
        dghat, dgvar = np.asarray(dghat, np.float64).astype(dt), np.asarray(dgvar, np.float64).astype(dt)
        d = dghat.shape[2]
        ir = np.ones(d, dt) if inv_range is None else np.asarray(inv_range, np.float64).astype(dt)
    out = {k: np.zeros(n0, dt) for k in ('ll', 'll_abs')}
    out.update({k: np.zeros((q, n0), dt) for k in ('s', 's_abs', 'v', 'v_abs')})
    out.update({k: (np.zeros((n0, d), dt) if grad else None) for k in ('dll', 'dll_abs')})
    half, one, two = dt(0.5), dt(1), dt(2)
    for i in range(n0):
        g = ghat[:, i]
        h = np.sqrt(np.maximum(gvar[:, i], dt(0)))
        mg = M @ g
        w = b - mg
        K = np.eye(q, dtype=dt) + h[:, None] * M * h[None, :]
        L = _cholesky(K, dt)
        u = _lower_solve(L, h * w, dt)
        logs = np.log(np.diag(L))
        out['ll'][i] = -half * (c0 - two * (b @ g) + g @ mg - u @ u + two * np.sum(logs, dtype=dt) + lognorm)
        out['ll_abs'][i] = half * (abs(c0) + two * np.abs(b * g).sum() + np.abs(g[:, None] * M * g[None, :]).sum() + u @ u
                                   + two * np.abs(logs).sum() + abs(lognorm))
        a = h * _upper_solve(L.T, u, dt)
        s = w - M @ a
        R = _lower_solve(L, h[:, None] * M, dt)
        T = np.diag(M) - np.sum(R * R, axis=0, dtype=dt)
        v = half * s * s - half * T
        out['s'][:, i], out['v'][:, i] = s, v
        out['s_abs'][:, i] = np.abs(b) + np.abs(M) @ np.abs(g) + np.abs(M) @ np.abs(a)
        out['v_abs'][:, i] = half * out['s_abs'][:, i] ** 2 + half * (np.abs(np.diag(M)) + np.sum(R * R, axis=0, dtype=dt))
        if grad:
            terms = s[:, None] * dghat[:, i, :] + v[:, None] * dgvar[:, i, :]
            out['dll'][i] = ir * terms.sum(axis=0, dtype=dt)
            out['dll_abs'][i] = np.abs(ir) * (out['s_abs'][:, i, None] * np.abs(dghat[:, i, :])
                                              + out['v_abs'][:, i, None] * np.abs(dgvar[:, i, :])).sum(axis=0)
    return out


def row_tolerances(ref64, refld):
    """per quantity: 4 x max(error of the float64 evaluation against the longdouble one, eps64 x the sum of the absolute values
    of that quantity's terms in longdouble), elementwise; the factor 4 is for the kernel's different summation order.  Nothing of
    the code under test enters."""
    eps = np.finfo(np.float64).eps
    tol = {}
    for k in ('ll', 's', 'v', 'dll'):
        if refld[k] is None:
            continue
        err = np.abs(ref64[k].astype(np.longdouble) - refld[k])
        tol[k] = (4 * np.maximum(err, eps * refld[k + '_abs'])).astype(np.float64)
    return tol


def rows_as_host_stub(blk, jac, M, b, inv_range, c0, lognorm, want_sens):
    """rows() behind the signature of LCGP._calib_rows_device (CPU torch tensors in, numpy out): what the CPU tests install in
    place of the row kernel"""
    blk = blk.numpy()
    jac = None if jac is None else jac.numpy()
    res = rows(blk[0], blk[1], None if jac is None else jac[0], None if jac is None else jac[1], M.numpy(), b.numpy(), c0, lognorm,
               None if jac is None else inv_range.numpy())
    return res['ll'], res['dll'], (np.stack([res['s'], res['v']]) if want_sens else None)


# ---- the model-level cases of tests/test_gpu_calibration.py (shared with the CPU test of their precondition) ----
SPAN3 = np.array([5.0, 0.25, 1.0])                  # raw inputs = 1 + SPAN3 * synthetic inputs: a different range per dimension
MODEL_CASES = {
    'full-matern32-q3': dict(mode='full', kernel='matern32', p=5, q=3, seed=91),
    'rep-se-q3': dict(mode='rep', kernel='se', p=5, q=3, seed=92),
    'full-matern52-q17': dict(mode='full', kernel='matern52', p=20, q=17, seed=93),
    'rep-matern32-q17': dict(mode='rep', kernel='matern32', p=20, q=17, seed=94),
}


def model_case(name, dtype='float64', device='cuda:0', group=None):
    """(model at the case's parameters, raw training inputs x, y): n = 300 (full) or 150 unique inputs twice (rep), d = 3.
    Building the model and setting its parameters needs no GPU."""
    from lcgp_amd import LCGP, synth
    from oracle import lcgp_oracle as orc
    c = MODEL_CASES[name]
    if c['mode'] == 'full':
        x, y = synth.make_full(c['seed'], 300, 3, c['p'], c['q'])
    else:
        x, y = synth.make_rep(c['seed'], 150, 2, 3, c['p'], c['q'])
    x = 1.0 + SPAN3 * x
    kw = {} if group is None else {'process_group': group}
    m = LCGP(y=y, x=x, q=c['q'], submethod=c['mode'], kernel=c['kernel'], device=device, dtype=dtype, **kw)
    o = orc.OracleLCGP(y=y, x=x, q=c['q'], submethod=c['mode'])
    m._set_flat(synth.param_points(c['seed'], o.get_unconstrained())[1])
    return m, x, y


def case_observation(name, x, y, form='dense'):
    """(theta (17, 3) raw scale with two training inputs among its rows, y_obs (p,), obs_var) of a case: the observation is a
    training run's output plus a tenth of each output's spread; obs_var is a scalar, per-output variances or those plus a
    rank-2 discrepancy covariance"""
    rng = np.random.default_rng(MODEL_CASES[name]['seed'])
    p = y.shape[0]
    sd = y.std(axis=1)
    lo, hi = x.min(0), x.max(0)
    theta = lo + (hi - lo) * rng.uniform(0.05, 0.95, (17, x.shape[1]))
    theta[:2] = x[[3, 11]]
    y_obs = y[:, 7] + 0.1 * sd * rng.standard_normal(p)
    var = (sd * rng.uniform(0.05, 0.15, p)) ** 2
    B = 0.1 * sd[:, None] * rng.standard_normal((p, 2))
    obs_var = {'scalar': float(var.mean()), 'diag': var, 'dense': np.diag(var) + B @ B.T}[form]
    return theta, y_obs, obs_var


def cond_bound(model, y_obs, obs_var):
    """an upper bound of cond(Sigma_i) that holds at EVERY input and for every kernel: gvar_k lies in [0, prior variance of
    component k], so Sigma_i lies between Lambda and Phi_s diag(prior) Phi_s^T + Lambda in the positive-definite order"""
    obs, phi_s, t, lam = observation(model, y_obs, obs_var)
    prior = model.lLmb0.numpy().reshape(-1)
    top = np.linalg.eigvalsh(phi_s @ (prior[:, None] * phi_s.T) + lam)[-1]
    return top / np.linalg.eigvalsh(lam)[0]
