"""The Matern-5/2 product kernel (LCGP_KERNEL_MATERN52, `LCGP(..., kernel='matern52')`) through the C ABI, every query.

PARITY UNPINNED: the reference has no Matern-5/2 kernel (src/lcgp/covmat.py:5-55 holds Matern32 only).  The committed numpy
oracle cannot learn one, so these tests patch it with tests/matern52_oracle.py, which tests/test_matern52_oracle.py pins by
identities (closed-form gradient = finite differences = autograd, eigendecomposition form = Cholesky form, kernel value =
the textbook Matern-5/2 at lengthscale sqrt(5) ell).  Tolerances are those of the files whose cases are repeated here:
tests/test_gpu_se_kernel.py (NLL 1e-6 relative, gradient 1e-5 of max|g|, covariance matrix rtol 1e-13, predict rtol 1e-6 /
atol 1e-9, float32 against float64 2e-4 / 2e-2, fit 1e-3), tests/test_gpu_predict_grad.py (central differences 1e-6 of the
largest entry, float32 2e-3), tests/test_gpu_cv.py (1e-9), tests/test_gpu_variance_reduction.py and
tests/test_gpu_select_batch.py (1e-10 of the largest latent variance [times sum omega]; float32 2e-3).

The brute-force checks (leave-one-out, variance reduction, batch selection) refactorise the reduced / augmented data in
numpy with the helper's kernel; they are the only cover of the OP_VR epilogue and of the selection kernels for this kernel id,
where a site that only told Matern-3/2 from "anything else" would return squared-exponential numbers."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lcgp_amd import LCGP, Matern52, synth
from oracle import lcgp_oracle as orc
from tests import matern52_oracle as m52
from tests.test_gpu_variance_reduction import _free_port, _match, _points, _state
from tests.test_select_batch_host import omega_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NLL_RTOL = 1e-6
GRAD_RTOL = 1e-5
K = 'matern52'


@pytest.fixture(autouse=True)
def _oracle52(monkeypatch):
    m52.patch(monkeypatch)


def _check(m, o, pts):
    o.phi = m.phi.numpy().copy()
    for u in pts:
        v1, g1 = m.loss_and_grad(u)
        v2, g2 = o.loss_and_grad_unconstrained(u)
        print('matern52 NLL rel err %.3e, grad err %.3e of max|g|' % (abs(v1 - v2) / abs(v2), np.max(np.abs(g1 - g2)) / np.max(np.abs(g2))))
        assert abs(v1 - v2) <= NLL_RTOL * abs(v2), (v1, v2)
        assert np.max(np.abs(g1 - g2)) <= GRAD_RTOL * np.max(np.abs(g2)), np.max(np.abs(g1 - g2))


# ---- the cases of tests/test_gpu_se_kernel.py ----
def test_covariance_matrix():
    rng = np.random.default_rng(0)
    x1 = rng.standard_normal((70, 3))
    x2 = rng.standard_normal((45, 3))
    ell = [0.7, 1.3, 0.4]
    for a, b in ((x1, x2), (x1, x1)):
        got = Matern52(a, b, ell, 1.7, 3e-3).numpy()
        want = orc.matern32(a, b, ell, 1.7, 3e-3, kernel=K)
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-16)
        # neither of the other two kernels
        assert np.max(np.abs(got - orc.matern32(a, b, ell, 1.7, 3e-3))) > 1e-2
        assert np.max(np.abs(got - orc.matern32(a, b, ell, 1.7, 3e-3, kernel='se'))) > 1e-2
    np.testing.assert_allclose(Matern52(x1, x1, ell, 1.7, 3e-3, diag_only=True).numpy(), 1.7)
    # d > 32: the dimensions in chunks
    xa, xb = rng.standard_normal((70, 40)), rng.standard_normal((45, 40))
    ellw = rng.uniform(2.0, 6.0, 40)
    np.testing.assert_allclose(Matern52(xa, xb, ellw, 0.9, 1e-4).numpy(), orc.matern32(xa, xb, ellw, 0.9, 1e-4, kernel=K),
                               rtol=1e-13, atol=1e-16)


@pytest.mark.parametrize('n,d,p,q,kw', [
    (40, 1, 3, 3, {}),
    (65, 2, 4, 2, dict(robust_mean=False)),
    (200, 3, 6, 4, dict(diag_error_structure=[1, 2, 3])),
    (333, 6, 5, 5, {}),
    (300, 40, 4, 2, {}),                                        # d > 32: the wide gradient contraction
])
def test_full_path_matches_oracle(n, d, p, q, kw):
    x, y = synth.make_full(300 + n, n, d, p, q)
    m = LCGP(y=y, x=x, q=q, kernel=K, **kw)
    o = orc.OracleLCGP(y=y, x=x, q=q, kernel=K, **kw)
    _check(m, o, synth.param_points(n, o.get_unconstrained()))


@pytest.mark.parametrize('d', [10, 16])
def test_full_path_matches_oracle_in_the_other_dimension_buckets(d):
    x, y = synth.make_full(500 + d, 150, d, 4, 2)
    m = LCGP(y=y, x=x, q=2, kernel=K)
    o = orc.OracleLCGP(y=y, x=x, q=2, kernel=K)
    _check(m, o, synth.param_points(d, o.get_unconstrained()))


def test_rep_path_matches_oracle():
    x, y = synth.make_rep(270, 70, 3, 2, 4, 4)
    m = LCGP(y=y, x=x, submethod='rep', kernel=K)
    o = orc.OracleLCGP(y=y, x=x, submethod='rep', kernel=K)
    _check(m, o, synth.param_points(70, o.get_unconstrained()))


def test_differs_from_the_other_kernels_and_rejects_unknown_names():
    x, y = synth.make_full(5, 150, 3, 4, 3)
    a = LCGP(y=y, x=x, q=3, kernel=K)
    for other in ('matern32', 'se'):
        b = LCGP(y=y, x=x, q=3, kernel=other)
        assert abs(float(a.loss()) - float(b.loss())) > 1e-3 * abs(float(b.loss()))
    with pytest.raises(ValueError):
        LCGP(y=y, x=x, q=3, kernel='rbf')


def test_predict_matches_oracle():
    x, y = synth.make_full(31, 150, 3, 4, 3)
    m = LCGP(y=y, x=x, q=3, kernel=K)
    o = orc.OracleLCGP(y=y, x=x, q=3, kernel=K)
    o.phi = m.phi.numpy().copy()
    u = synth.param_points(31, o.get_unconstrained())[2]
    m._set_flat(u)
    o.set_unconstrained(u)
    for x0 in (np.random.default_rng(1).uniform(0, 1, (70, 3)), x):
        got = m.predict(x0, return_fullcov=True)
        want = o.predict(x0, return_fullcov=True)
        for g, w in zip(got, want):
            np.testing.assert_allclose(g.numpy(), w, rtol=1e-6, atol=1e-9)


def test_rep_predict_matches_oracle():
    x, y = synth.make_rep(33, 60, 3, 2, 4, 3)
    m = LCGP(y=y, x=x, q=3, submethod='rep', kernel=K)
    o = orc.OracleLCGP(y=y, x=x, q=3, submethod='rep', kernel=K)
    o.phi = m.phi.numpy().copy()
    u = synth.param_points(33, o.get_unconstrained())[1]
    m._set_flat(u)
    o.set_unconstrained(u)
    x0 = np.random.default_rng(2).uniform(0, 1, (50, 2))
    for g, w in zip(m.predict(x0), o.predict(x0)):
        np.testing.assert_allclose(g.numpy(), w, rtol=1e-6, atol=1e-9)


def test_float32_against_float64():
    x, y = synth.make_full(41, 700, 4, 6, 3)
    m64 = LCGP(y=y, x=x, q=3, kernel=K)
    m32 = LCGP(y=y, x=x, q=3, kernel=K, dtype='float32')
    u = m64._get_flat()
    v64, g64 = m64.loss_and_grad(u)
    v32, g32 = m32.loss_and_grad(u)
    print('matern52 float32: NLL %.3e, grad %.3e' % (abs(v32 - v64) / abs(v64), np.max(np.abs(g32 - g64)) / np.max(np.abs(g64))))
    assert abs(v32 - v64) <= 2e-4 * abs(v64)
    assert np.max(np.abs(g32 - g64)) <= 2e-2 * np.max(np.abs(g64))


def test_float32_wide_and_rep_against_float64():
    for mode, maker in (('full', lambda: synth.make_full(43, 300, 40, 4, 2)), ('rep', lambda: synth.make_rep(44, 100, 3, 3, 4, 2))):
        x, y = maker()
        m64 = LCGP(y=y, x=x, q=2, kernel=K, submethod=mode)
        m32 = LCGP(y=y, x=x, q=2, kernel=K, submethod=mode, dtype='float32')
        u = m64._get_flat()
        v64, g64 = m64.loss_and_grad(u)
        v32, g32 = m32.loss_and_grad(u)
        assert abs(v32 - v64) <= 2e-4 * abs(v64), mode
        assert np.max(np.abs(g32 - g64)) <= 2e-2 * np.max(np.abs(g64)), mode


def test_fit_reaches_the_oracle_optimum():
    x, y = synth.make_full(61, 120, 2, 4, 3)
    m = LCGP(y=y, x=x, q=3, kernel=K)
    o = orc.OracleLCGP(y=y, x=x, q=3, kernel=K)
    o.phi = m.phi.numpy().copy()
    m.fit()
    o.fit()
    assert abs(float(m.loss()) - o.loss()) <= 1e-3 * abs(o.loss())
    v_at, _ = o.loss_and_grad_unconstrained(m._get_flat())
    assert abs(float(m.loss()) - v_at) <= 1e-9 * abs(v_at)


# ---- float32 at the SoftClip bounds of the lengthscales ----
def test_float32_survives_collapsed_lengthscales():
    """tests/test_gpu_edge_cases.py::test_float32_survives_collapsed_lengthscales for this kernel: ten dimensions, every
    lengthscale at its lower bound 1e-6, the polynomial ~(1e12 / 3)^10 overflows float32 (a single factor stays finite, the
    product does not) beside an exponential that is zero.  The float32 engine itself has to cope (no float64 repeat)."""
    x, y = synth.make_full(323, 300, 10, 4, 2)
    m64 = LCGP(y=y, x=x, q=2, kernel=K)
    m32 = LCGP(y=y, x=x, q=2, kernel=K, dtype='float32')
    m32.float32_fallback = False
    u = m64._get_flat().copy()
    u[:20] = -40.0
    v64, g64 = m64.loss_and_grad(u)
    v32, g32 = m32.loss_and_grad(u)
    assert np.isfinite(v32) and np.all(np.isfinite(g32))
    assert abs(v32 - v64) <= 2e-4 * abs(v64)
    assert np.max(np.abs(g32 - g64)) <= 2e-2 * max(np.max(np.abs(g64)), 1e-300)
    o = orc.OracleLCGP(y=y, x=x, q=2, kernel=K)
    o.phi = m64.phi.numpy().copy()
    vo, go = o.loss_and_grad_unconstrained(u)
    assert abs(v64 - vo) <= 1e-6 * abs(vo) and np.max(np.abs(g64 - go)) <= 1e-5 * max(np.max(np.abs(go)), 1e-300)


@pytest.mark.parametrize('d,n', [(10, 300), (40, 200)])
@pytest.mark.parametrize('shift', [-40.0, 40.0])
def test_float32_at_the_lengthscale_bounds_behaves_as_matern32(d, n, shift):
    """lengthscales at the lower / upper bound, narrow and wide d: loss and gradient finite (or the point cleanly repeated in
    float64), never NaN, and whether float32 carried the point is what it is for Matern-3/2 there"""
    x, y = synth.make_full(325, n, d, 4, 2)
    res = {}
    for kernel in ('matern32', K):
        m = LCGP(y=y, x=x, q=2, kernel=kernel, dtype='float32')
        u = m._get_flat().copy()
        u[:2 * d] = shift
        v, g = m.loss_and_grad(u)
        assert np.isfinite(v) and np.all(np.isfinite(g)), kernel
        res[kernel] = (bool(m._last_eval_float64), int(m.float32_fallbacks))
    print('float32 at lengthscale shift %+g, d = %d: (repeated in float64, count) %r' % (shift, d, res))
    assert res[K] == res['matern32'], res


# ---- input gradients ----
def _post_model(mode, d, n=300, q=2, dtype='float64', seed=81, span=None, p=3):
    if mode == 'full':
        x, y = synth.make_full(seed, n, d, p, q)
    else:
        x, y = synth.make_rep(seed, n // 2, 3, d, p, q)
    if span is not None:
        x = 1.0 + span * x
    m = LCGP(y=y, x=x, q=q, submethod=mode, kernel=K, device='cuda:0', dtype=dtype)
    o = orc.OracleLCGP(y=y, x=x, q=q, submethod=mode)
    m._set_flat(synth.param_points(seed, o.get_unconstrained())[1])
    return m, np.asarray(x)


def _central_differences(m, x0, h):
    n0, d = x0.shape
    out = np.zeros((3, int(m.p), n0, d))
    for l in range(d):
        e = np.zeros_like(x0)
        e[:, l] = h[l]
        plus, minus = m.predict(x0 + e), m.predict(x0 - e)
        for w in range(3):
            out[w, :, :, l] = (plus[w].numpy() - minus[w].numpy()) / (2 * h[l])
    return out


@pytest.mark.parametrize('mode,d,dims', [('full', 3, None), ('rep', 3, None), ('full', 40, [0, 17, 33, 39]), ('rep', 6, None)])
def test_predict_grad_against_central_differences_and_autograd(mode, d, dims):
    """at new inputs AND at the training inputs themselves: the Matern-5/2 weight s (1 + |s|) / (3 + 3 |s| + s^2) goes to 0
    with s, so the surface has no kink there to step over (central differences straddle the training input)"""
    span = np.array([5.0, 0.25, 1.0]) if d == 3 else None
    m, x = _post_model(mode, d, span=span)
    lo, hi = x.min(0), x.max(0)
    xt = m.x_unique.numpy() if mode == 'rep' else x           # raw training inputs
    x0 = np.vstack([lo + (hi - lo) * np.random.default_rng(2).uniform(0.05, 0.95, (12, d)), xt[[0, 7, 11, 40, 101]]])
    got = [t.numpy() for t in m.predict_grad(x0)]
    h = 1e-5 * (hi - lo)
    if dims is None:
        fd, sel = _central_differences(m, x0, h), slice(None)
    else:                                   # wide d: the differences along a few dimensions (two predict calls each)
        fd = np.zeros((3, int(m.p), len(x0), len(dims)))
        for c, l in enumerate(dims):
            e = np.zeros_like(x0)
            e[:, l] = h[l]
            plus, minus = m.predict(x0 + e), m.predict(x0 - e)
            for w in range(3):
                fd[w, :, :, c] = (plus[w].numpy() - minus[w].numpy()) / (2 * h[l])
        sel = dims
    for g, f in zip(got, fd):
        assert g.shape == (int(m.p), len(x0), d)
        err = np.max(np.abs(g[:, :, sel] - f)) / np.max(np.abs(f))
        print('matern52 predict_grad %s d=%d: %.3e of the largest central difference' % (mode, d, err))
        assert err <= 1e-6, err
    # autograd through predict_differentiable: the same Jacobians contracted with ones
    xg = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
    outs = m.predict_differentiable(xg)
    for a, b in zip(outs, m.predict(x0)):
        assert torch.equal(a.detach(), b)
    for w in range(3):
        xg = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
        m.predict_differentiable(xg)[w].sum().backward()
        want = got[w].sum(axis=0)
        np.testing.assert_allclose(xg.grad.numpy(), want, rtol=1e-12, atol=1e-12 * np.max(np.abs(want)))


def test_predict_differentiable_gradcheck():
    m, x = _post_model('full', 2, n=120)
    x0 = np.vstack([np.random.default_rng(12).uniform(0.1, 0.9, (3, 2)), x[[5]]])
    xt = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
    for w in range(3):
        assert torch.autograd.gradcheck(lambda t: m.predict_differentiable(t)[w], (xt,), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_predict_grad_float32_against_float64():
    m64, x = _post_model('full', 4)
    m32, _ = _post_model('full', 4, dtype='float32')
    x0 = np.random.default_rng(10).uniform(0, 1, (150, 4))
    for a, b in zip(m32.predict_grad(x0), m64.predict_grad(x0)):
        err = np.max(np.abs(a.numpy() - b.numpy())) / np.max(np.abs(b.numpy()))
        assert err <= 2e-3, err


# ---- joint covariance and draws ----
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_joint_covariance_diagonals_and_sample(mode):
    m, x = _post_model(mode, 2, n=200)
    x0 = _points(x, 60, 3)
    yp, ypv, ycv = [t.numpy() for t in m.predict(x0)]
    lc = m.predict_latent_cov(x0).numpy()
    gv = m._ensure_aux().predict_block(m._standardise_x0(x0)[0])[1].cpu().numpy()
    np.testing.assert_allclose(np.diagonal(lc, axis1=1, axis2=2), gv, rtol=1e-9, atol=1e-12 * gv.max())
    jc = m.predict_jointcov(x0).numpy()
    np.testing.assert_allclose(np.diagonal(jc, axis1=1, axis2=2), ypv, rtol=1e-9, atol=1e-12 * np.max(ypv))
    jc0 = m.predict_jointcov(x0, include_noise=False).numpy()
    np.testing.assert_allclose(np.diagonal(jc0, axis1=1, axis2=2), ycv, rtol=1e-9, atol=1e-12 * np.max(ypv))
    # Sigma_k in float64 numpy with the helper's kernel: the GPU's matrix, and positive definite BEFORE the draw is asked for
    th, xs, s = _state(m)
    x0s = m._standardise_x0(x0)[0]
    d = xs.shape[1]
    for k in range(th.shape[0]):
        ell, scale, nug, D = th[k, :d], th[k, d], th[k, d + 1], th[k, d + 2]
        A = np.eye(len(xs)) + D * m52.kernel_matrix(xs, xs, ell, scale, nug, same=True) * np.outer(s, s)
        c = m52.kernel_matrix(x0s, xs, ell, scale, nug) * s[None, :]
        sig = m52.kernel_matrix(x0s, x0s, ell, scale, nug, same=True) - D * c @ np.linalg.solve(A, c.T)
        np.testing.assert_allclose(lc[k], sig, rtol=0, atol=1e-10 * scale)
        assert np.linalg.eigvalsh(sig).min() > 1e-8 * scale, 'the design must leave Sigma_k positive definite'
    draws = m.sample(x0, size=64, seed=5).numpy()               # default jitter
    assert draws.shape == (64, int(m.p), 60) and np.all(np.isfinite(draws))
    assert np.array_equal(draws, m.sample(x0, size=64, seed=5).numpy())
    # the draws scatter around ypred by a few standard deviations
    assert np.all(np.abs(draws.mean(axis=0) - yp) <= 6.0 * np.sqrt(ypv / 64))


# ---- leave-one-out / k-fold ----
def _latent_at(th, x, s, b, xt):
    """ghat, gvar of predict() at new standardised inputs xt for the data (x, s, b = Y^T psi), helper kernel, float64 numpy"""
    d = x.shape[1]
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    A = np.eye(len(x)) + D * m52.kernel_matrix(x, x, ell, scale, nug, same=True) * np.outer(s, s)
    c = m52.kernel_matrix(xt, x, ell, scale, nug) * s[None, :]
    sol = np.linalg.solve(A, np.column_stack([b, c.T]))
    return c @ sol[:, 0], scale - D * np.sum(c * sol[:, 1:].T, axis=1)


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_loo_and_folds_against_brute_force_refactorisation(mode):
    m, x = _post_model(mode, 2, n=330, q=3, p=4)
    eng = m._ensure_aux()
    th, xs, s = _state(m)
    n = len(xs)
    if mode == 'rep':
        yb = (m.ybar_s if m.rep_standardize_ybar else m.ybar).numpy()
        Y = yb * s[None, :]
    else:
        Y = m.y.numpy()
    blk = eng.loo_block().cpu().numpy()
    labels = np.random.default_rng(5).permutation(n) % 4
    _, ptr, idx = m._cv_labels(labels, 0)
    cvb = eng.cv_block(ptr, idx).cpu().numpy()
    d = xs.shape[1]
    for k in range(th.shape[0]):
        b = Y.T @ th[k, d + 3:]
        for rows, got in [([i], blk) for i in (0, n // 2, n - 1)] + [(np.flatnonzero(labels == 2), cvb)]:
            keep = np.setdiff1d(np.arange(n), rows)
            gh, gv = _latent_at(th[k], xs[keep], s[keep], b[keep], xs[rows])
            for w_, ref in enumerate((gh, gv)):
                scale = max(np.max(np.abs(got[w_, k])), 1e-300)
                err = np.max(np.abs(got[w_, k, rows] - ref)) / scale
                assert err <= 1e-9, (k, w_, len(rows), err)
    outs = [r.numpy() for r in m.predict_loo()]
    ref = m._outputs_rep(blk[0], blk[1]) if mode == 'rep' else m._outputs_full(blk[0], blk[1])
    for a, b_ in zip(outs, ref):
        assert a.shape == (int(m.p), n) and np.array_equal(a, b_.numpy())
    assert [r.shape for r in m.predict_cv(labels)] == [(int(m.p), n)] * 3


# ---- variance reduction and batch selection: brute force on the augmented data ----
def _gvar_at(th, x, s, xt):
    return _latent_at(th, x, s, np.zeros(len(x)), xt)[1]


def _augment(xt, rr, c, r):
    hit = np.flatnonzero(np.all(xt == c[None, :], axis=1))
    if len(hit):
        r2 = rr.copy()
        r2[hit[0]] += r
        return xt, r2
    return np.vstack([xt, c]), np.r_[rr, float(r)]


def _brute_R(th, xt, rr, xr_s, xc_s, w, r, cols):
    """(q, len(cols)): weighted drop of gvar over the reference points when r runs at candidate j join the data (xt, rr)"""
    out = np.zeros((th.shape[0], len(cols)))
    for k in range(th.shape[0]):
        before = w @ _gvar_at(th[k], xt, np.sqrt(rr), xr_s)
        for a, j in enumerate(cols):
            x2, r2 = _augment(xt, rr, xc_s[j], r)
            out[k, a] = before - w @ _gvar_at(th[k], x2, np.sqrt(r2), xr_s)
    return out


def _vr_model(mode, d, dtype='float64', n=480):
    if mode == 'full':
        x, y = synth.make_full(91, n, d, 4, 3)
    else:
        x, y = synth.make_rep(92, n // 3, 3, d, 4, 3)
    m = LCGP(y=y, x=x, q=3, submethod=mode, kernel=K, device='cuda:0', dtype=dtype)
    o = orc.OracleLCGP(y=y, x=x, q=3, submethod=mode)
    m._set_flat(synth.param_points(91, o.get_unconstrained())[1])
    return m, np.asarray(x)


@pytest.mark.parametrize('mode,d,n', [('full', 2, 480), ('rep', 2, 480), ('full', 6, 480), ('rep', 6, 480), ('full', 40, 360)])
def test_variance_reduction_against_brute_force(mode, d, n):
    m, x = _vr_model(mode, d, n=n)
    xc = _points(x, 150, 1)
    if mode == 'rep':
        xc = np.vstack([xc, m.x_unique.numpy()[[0, 7, 33]]])
    xr = _points(x, 230, 2)
    w = np.random.default_rng(3).random(len(xr))
    th, xt, s = _state(m)
    cols = [0, 1, 77, 149] + ([150, 152] if mode == 'rep' else [])
    for r in ((1, 3) if mode == 'rep' else (1,)):
        for ref, ww in ((None, None), (xr, w)):
            R = m.variance_reduction(xc, x_ref=ref, weights=ww, replicates=r, latent=True).numpy()
            xc_s = m._standardise_x0(xc)[0]
            xr_s = xc_s if ref is None else m._standardise_x0(ref)[0]
            wn = np.full(len(xr_s), 1.0 / len(xr_s)) if ww is None else ww / ww.sum()
            if mode == 'rep':
                assert np.sum(_match(m, xc_s) >= 0) == 3
            gv = m._ensure_aux().predict_block(xr_s)[1].cpu().numpy()
            assert np.all(np.isfinite(R)) and np.all(R >= -1e-12 * gv.max())
            bf = _brute_R(th, xt, s * s, xr_s, xc_s, wn, r, cols)
            err = np.max(np.abs(R[:, cols] - bf)) / gv.max()
            print('matern52 variance_reduction %s d=%d r=%d: %.3e of max gvar' % (mode, d, r, err))
            assert err <= 1e-10, (mode, d, r, err)


def test_variance_reduction_float32_against_float64():
    m64, x = _vr_model('full', 2)
    m32, _ = _vr_model('full', 2, dtype='float32')
    xc, xr = _points(x, 200, 10), _points(x, 150, 11)
    a = m64.variance_reduction(xc, x_ref=xr, latent=True).numpy()
    b = m32.variance_reduction(xc, x_ref=xr, latent=True).numpy()
    gv = m64._ensure_aux().predict_block(m64._standardise_x0(xr)[0])[1].cpu().numpy()
    assert np.all(np.isfinite(b))
    assert np.max(np.abs(a - b)) <= 2e-3 * gv.max(), np.max(np.abs(a - b)) / gv.max()


@pytest.mark.parametrize('mode,d,n', [('full', 2, 480), ('rep', 2, 480), ('full', 6, 480), ('full', 40, 360)])
def test_select_batch_against_brute_force_on_replayed_picks(mode, d, n):
    """every step's score row against a refactorisation of the data augmented by the picks the GPU made so far (the oracle
    replays the picks, so near-ties cannot make a case flaky); 1e-10 of max gvar * sum omega, as tests/test_gpu_select_batch.py"""
    m, x = _vr_model(mode, d, n=n)
    xc = _points(x, 40, 1)
    if mode == 'rep':
        xc = np.vstack([xc[:20], m.x_unique.numpy()[[0, 7, 33]], xc[20:]])
    xr = _points(x, 120, 2)
    w = np.random.default_rng(3).random(len(xr))
    size = 5
    th, xt, s = _state(m)
    om = omega_of(m)
    for r in ((1, 3) if mode == 'rep' else (1,)):
        for ref, ww in ((None, None), (xr, w)):
            idx, gain, scores = (t.numpy() for t in m.select_batch(xc, size, x_ref=ref, weights=ww, replicates=r, return_scores=True))
            xc_s = m._standardise_x0(xc)[0]
            xr_s = xc_s if ref is None else m._standardise_x0(ref)[0]
            wn = np.full(len(xr_s), 1.0 / len(xr_s)) if ww is None else ww / ww.sum()
            unit = m._ensure_aux().predict_block(xr_s)[1].cpu().numpy().max() * np.sum(om)
            assert len(set(idx.tolist())) == size
            x2, r2 = xt, s * s
            worst = 0.0
            for t in range(size):
                live = np.setdiff1d(np.arange(len(xc)), idx[:t])
                assert np.all(np.isneginf(scores[t, idx[:t]])) and np.all(np.isfinite(scores[t, live]))
                assert idx[t] == int(np.argmax(scores[t])) and gain[t] == scores[t, idx[t]]
                bf = om @ _brute_R(th, x2, r2, xr_s, xc_s, wn, r, live)
                worst = max(worst, np.max(np.abs(scores[t, live] - bf)) / unit)
                x2, r2 = _augment(x2, r2, xc_s[idx[t]], r)
            print('matern52 select_batch %s d=%d r=%d: worst %.3e of max gvar * sum omega' % (mode, d, r, worst))
            assert worst <= 1e-10, (mode, d, r, worst)


def test_select_batch_float32_on_replayed_picks():
    m64, x = _vr_model('full', 2)
    m32, _ = _vr_model('full', 2, dtype='float32')
    xc, xr = _points(x, 60, 10), _points(x, 100, 11)
    idx, gain, scores = (t.numpy() for t in m32.select_batch(xc, 4, x_ref=xr, return_scores=True))
    assert np.all(np.isfinite(gain)) and len(set(idx.tolist())) == 4
    # step 0 has no picks to replay: it is the float64 model's variance reduction
    om = omega_of(m64)
    R = m64.variance_reduction(xc, x_ref=xr, latent=True).numpy()
    unit = m64._ensure_aux().predict_block(m64._standardise_x0(xr)[0])[1].cpu().numpy().max() * np.sum(om)
    assert np.max(np.abs(scores[0] - om @ R)) <= 2e-3 * unit


# ---- two ranks ----
def test_two_ranks_reproduce_one_rank():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_m52_gpu_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, OMP_NUM_THREADS="4"))
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout
