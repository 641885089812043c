"""CPU tests of the input Hessians and the gradient covariance of a conditioned view (ConditionedLCGP.predict_hess /
predict_differentiable(order=2) / predict_grad_cov / active_subspace): a numpy stand-in of
HotPathEngine.condition_predict_hess_block / condition_grad_cov_block written from the closed form of include/lcgp_hip.h (the
derivative rows P, Q and the widened rows P' = [P | Q / sqrt(D)], the contraction over n + m columns), checked against brute
force (augment the training set, refactor, lcgp_predict_hess's and lcgp_predict_gradcov's formulas) and against central
differences of the closed-form view gradient; the host layer -- shapes, dtypes, exact symmetry, the raw-scale output map on
non-unit input ranges, latent=True, staleness, second-order autograd, active_subspace's assembly, two ranks -- through that
stand-in; and the symbols, argument checks and sizes of the new C entries (tests/test_gpu_condition_hess.py runs the same
through liblcgp_hip.so)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from tests import grad_cov_ref as gref
from tests.test_condition_grad_host import CondGradOracleEngine, closed_form_predict_grad
from tests.test_condition_host import KERNELS, _free_port, make_model, new_columns, patch_cond
from tests.test_grad_cov_host import GradCovOracleEngine
from tests.test_predict_hess_host import _cross, latent_hessians, pack_lower

HERE = os.path.dirname(os.path.abspath(__file__))


def _h_psi(s, kernel):
    a = np.abs(s)
    if kernel == 'matern32':
        return s / (1.0 + a), -(1.0 - a) / (1.0 + a)
    if kernel == 'se':
        return s, s * s - 1.0
    assert kernel == 'matern52'
    return s * (1.0 + a) / (3.0 + 3.0 * a + a * a), -(1.0 + a - a * a) / (3.0 + 3.0 * a + a * a)


def _second(x0, x, ell, c, kernel):
    """(h (n0, n, d), d2c (n0, n, d, d)) of the kernel values c: lcgp_predict_hess's h and d2_lm c"""
    d = x.shape[1]
    h, psi = _h_psi((x0[:, None, :] - x[None, :, :]) / ell, kernel)
    kap = h[:, :, :, None] * h[:, :, None, :]
    idx = np.arange(d)
    kap[:, :, idx, idx] = psi
    return h, c[:, :, None, None] * kap / (ell[:, None] * ell[None, :])


def closed_form_predict_hess(th, low, z, x, sr, kernel, xn, Un, LS, v, x0):
    """(d2ghat', d2gvar', Gamma') (n0, d, d) of one component in the closed form of include/lcgp_hip.h
    (lcgp_condition_predict_hess / lcgp_condition_predict_gradcov)"""
    n0, d = x0.shape
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    c = _cross(x0, x, ell, scale, nug, kernel)
    cx = _cross(x0, xn, ell, scale, nug, kernel)
    U0 = sla.solve_triangular(low, (c * sr[None, :]).T, lower=True).T
    T = sla.solve_triangular(LS, (cx - D * U0 @ Un.T).T, lower=True).T
    w = sla.solve_triangular(LS.T, v, lower=False)
    zp = z - D * sla.solve_triangular(low.T, Un.T @ w, lower=False)
    R = sla.solve_triangular(LS.T, T.T, lower=False).T
    Vp = sla.solve_triangular(low.T, (U0 - R @ Un).T, lower=False).T
    h, d2c = _second(x0, x, ell, c, kernel)
    hx, d2cx = _second(x0, xn, ell, cx, kernel)
    # the derivative rows, their factors -1 / ell_l left out: row i d + l
    dX = (c[:, :, None] * h * sr[None, :, None]).transpose(0, 2, 1).reshape(n0 * d, -1)
    dXn = (cx[:, :, None] * hx).transpose(0, 2, 1).reshape(n0 * d, -1)
    P = sla.solve_triangular(low, dX.T, lower=True).T
    Q = sla.solve_triangular(LS, (dXn - D * P @ Un.T).T, lower=True).T
    Pw = np.hstack([P, Q / np.sqrt(D)]).reshape(n0, d, -1)
    G = np.einsum('ilj,imj->ilm', Pw, Pw) / (ell[:, None] * ell[None, :])
    hm = np.einsum('ijlm,j->ilm', d2c, sr * zp) + np.einsum('ialm,a->ilm', d2cx, w)
    hv = -2.0 * (D * np.einsum('ijlm,ij->ilm', d2c, sr[None, :] * Vp) + np.einsum('ialm,ia->ilm', d2cx, R) + D * G)
    c_zero = _cross(x0[:1], np.repeat(x0[:1], 2, axis=0), ell, scale, nug, kernel)[0, 0]
    gamma = np.diag(c_zero * gref.KAPPA[kernel] / ell ** 2)[None, :, :] - D * G
    return hm, hv, gamma


class CondHessOracleEngine(CondGradOracleEngine):
    """CondGradOracleEngine plus condition_predict_hess_block / condition_grad_cov_block, in numpy float64"""
    grad_cov_block = GradCovOracleEngine.grad_cov_block        # (the base model's query beside the view's)

    def _second_order(self, state, x0s):
        assert self.is_current(state['theta'])
        x0 = np.asarray(x0s, np.float64)
        sr = np.ones(self.n) if self.sr is None else self.sr
        return [closed_form_predict_hess(th, low, z, self.x, sr, self.kernel, state['xn'], *state['state'][i], x0)
                for i, (th, low, z, b) in enumerate(self._state)]

    def condition_predict_hess_block(self, state, x0s):
        blk, jac = self.condition_predict_grad_block(state, x0s)
        res = self._second_order(state, x0s)
        hess = np.stack([np.stack([pack_lower(r[0]) for r in res]), np.stack([pack_lower(r[1]) for r in res])])
        return blk, jac, torch.as_tensor(hess)

    def condition_grad_cov_block(self, state, x0s, w=None, per_point=True):
        if w is None and not per_point:
            raise ValueError("condition_grad_cov_block: per_point=False needs weights")
        dghat = self.condition_predict_grad_block(state, x0s)[1][0]
        gamma = np.stack([pack_lower(r[2]) for r in self._second_order(state, x0s)])
        M = None if w is None else torch.as_tensor(np.einsum('i,kie->ke', np.asarray(w, np.float64), gamma))
        return dghat, (torch.as_tensor(gamma) if per_point else None), M


def hess_model(mode, kernel='matern32', d=2, **kw):
    m, x, y, xn, yn = make_model(mode, kernel, d, **kw)
    return patch_cond(m, CondHessOracleEngine), x, y, xn, yn


def _x0(x, d, n0=9, seed=3):
    """new inputs on the raw scale of make_model, two training inputs among them"""
    return np.vstack([-1.5 + 4.0 * np.random.default_rng(seed).uniform(0.05, 0.95, (n0, d)), x[:2]])


def brute_force_second_order(m, xn, yn, x0):
    """d2ghat, d2gvar, Gamma (q, n0, d, d) from first principles: the training set augmented by the new columns, A rebuilt and
    factorised, then tests/test_predict_hess_host.latent_hessians and tests/grad_cov_ref.latent_grad_cov on the augmented set"""
    eng = m._aux_engine
    s = np.ones(eng.n) if eng.sr is None else eng.sr
    xn_s, snew, ycol = new_columns(m, xn, yn)
    xa, sa, Ya = np.vstack([eng.x, xn_s]), np.r_[s, snew], np.hstack([eng.Y, ycol])
    x0s = m._standardise_x0(x0)[0]
    d = xa.shape[1]
    hm, hv, gm = [], [], []
    for th in eng._theta_last:
        ell, scale, nug, D, psi = th[:d], th[d], th[d + 1], th[d + 2], th[d + 3:]
        Cm = _cross(xa, xa, ell, scale, nug, eng.kernel)
        Cm[np.arange(len(xa)), np.arange(len(xa))] = scale
        low = np.linalg.cholesky(np.eye(len(xa)) + D * Cm * np.outer(sa, sa))
        res = latent_hessians(x0s, xa, sa, th, low, sla.cho_solve((low, True), Ya.T @ psi), eng.kernel)
        hm.append(res[4])
        hv.append(res[5])
        gm.append(gref.latent_grad_cov(x0s, xa, sa, th, low, eng.kernel))
    return np.stack(hm), np.stack(hv), np.stack(gm)


def clear_points(m, view, d, n0, h, seed=5):
    """n0 standardised points at least two steps h clear of every training AND view coordinate (the Matern-3/2 kinks)"""
    eng = m._aux_engine
    knots = np.vstack([eng.x, view._state['xn']])
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < n0:
        p = rng.uniform(0.05, 0.95, d)
        if np.min(np.abs(p[None, :] - knots)) >= 2.0 * h:
            pts.append(p)
    return np.array(pts)


@pytest.mark.parametrize('d', [1, 2])
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_closed_form_equals_brute_force_and_central_differences(mode, kernel, d):
    m, x, _, xn, yn = hess_model(mode, kernel, d)
    view = m.condition(xn, yn)
    # brute force on the augmented training set; training inputs and the view's own inputs among the new inputs
    x1 = np.vstack([_x0(x, d), view.x_new.numpy()[:2]])
    n1 = len(x1)
    got = list(view._latent_predict_hess(x1)[4:]) + [view.predict_grad_cov(x1, latent=True).numpy()]
    want = brute_force_second_order(m, xn, yn, x1)
    for name, a, b in zip(('d2ghat', 'd2gvar', 'gamma'), got, want):
        assert a.shape == b.shape == (2, n1, d, d)
        err = np.max(np.abs(a - b)) / np.max(np.abs(b))
        assert err <= 1e-10, (name, err)
    base = m._aux_engine.predict_hess_block(m._standardise_x0(x1)[0])[2].numpy()
    assert np.max(np.abs(pack_lower(got[0]) - base[0])) > 1e-3 * np.max(np.abs(base[0]))      # the new runs did something
    # central differences of the closed-form view gradient, per component, on the standardised scale
    eng, st = m._aux_engine, view._state
    sr = np.ones(eng.n) if eng.sr is None else eng.sr
    h = 1e-5
    x0s = clear_points(m, view, d, 7, h)
    assert np.min(np.abs(x0s[:, None, :] - np.vstack([eng.x, st['xn']])[None, :, :])) >= 2.0 * h
    for i, (th, low, z, b) in enumerate(eng._state):
        hm, hv, _ = closed_form_predict_hess(th, low, z, eng.x, sr, eng.kernel, st['xn'], *st['state'][i], x0s)

        def f(p):
            return closed_form_predict_grad(th, low, z, eng.x, sr, eng.kernel, st['xn'], *st['state'][i], p)
        for c in range(d):
            e = np.zeros(d)
            e[c] = h
            (mp, vp), (mm, vm) = f(x0s + e), f(x0s - e)
            assert np.max(np.abs(hm[:, :, c] - (mp - mm) / (2 * h))) <= 1e-6 * np.max(np.abs(hm)), (i, c)
            assert np.max(np.abs(hv[:, :, c] - (vp - vm) / (2 * h))) <= 1e-6 * np.max(np.abs(hv)), (i, c)


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_host_layer_shapes_dtypes_symmetry_output_map_and_latent(mode):
    m, x, _, xn, yn = hess_model(mode)
    view = m.condition(torch.as_tensor(xn), torch.as_tensor(yn))
    x0 = _x0(x, 2)
    res = view.predict_hess(torch.as_tensor(x0))
    assert len(res) == 3
    for a in res:
        assert isinstance(a, torch.Tensor) and a.dtype == torch.float64 and a.shape == (3, 11, 2, 2)
        assert a.device.type == 'cpu' and not a.requires_grad and torch.all(torch.isfinite(a))
        assert torch.equal(a, a.transpose(-1, -2))                                  # exact symmetry by host mirroring
    assert torch.equal(res[1], res[2]) and res[1] is not res[2]
    gh, gv, jm, jv, hm, hv = view._latent_predict_hess(x0)
    a, b, c, e = view.predict_grad(x0, latent=True)
    assert np.array_equal(gh, a.numpy()) and np.array_equal(gv, b.numpy())
    assert np.array_equal(jm, c.numpy()) and np.array_equal(jv, e.numpy())
    assert hm.shape == hv.shape == (2, 11, 2, 2)
    # the base model's output map and its division by the input ranges (4.0 in every dimension here)
    W, _, scale, _ = m._output_map()
    rng = (m.x_max.numpy() - m.x_min.numpy()).reshape(-1)
    assert np.all(rng > 3.0)
    rr = rng[:, None] * rng[None, :]
    want = np.einsum('ka,kilm->ailm', W, hm) * scale[:, None, None, None] / rr
    np.testing.assert_allclose(res[0].numpy(), want, rtol=1e-13)
    want = np.einsum('ka,kilm->ailm', W ** 2, hv) * (scale ** 2)[:, None, None, None] / rr
    np.testing.assert_allclose(res[2].numpy(), want, rtol=1e-13)
    # the gradient covariance: latent and through the output map
    G = view.predict_grad_cov(x0, latent=True)
    cov = view.predict_grad_cov(torch.as_tensor(x0))
    assert G.shape == (2, 11, 2, 2) and cov.shape == (3, 11, 2, 2) and G.dtype == cov.dtype == torch.float64
    assert torch.equal(G, G.transpose(-1, -2)) and torch.equal(cov, cov.transpose(-1, -2))
    want = np.einsum('ka,kilm->ailm', W ** 2, G.numpy()) * (scale ** 2)[:, None, None, None] / rr
    np.testing.assert_allclose(cov.numpy(), want, rtol=1e-13)
    # conditioning cannot add gradient uncertainty: Gamma_base - Gamma' is positive semidefinite
    Gb = m.predict_grad_cov(x0, latent=True).numpy()
    ev = np.linalg.eigvalsh(Gb - G.numpy())
    assert np.min(ev) >= -1e-12 * np.max(np.abs(Gb)) and np.max(ev) > 1e-6 * np.max(np.abs(Gb))
    # central differences of view.predict_grad on the raw scale, away from the training inputs
    h = 1e-5 * rng
    for c in range(2):
        e = np.zeros(2)
        e[c] = h[c]
        p, q = view.predict_grad(x0[:9] + e), view.predict_grad(x0[:9] - e)
        for j in (0, 2):
            fd = (p[j].numpy() - q[j].numpy()) / (2 * h[c])
            assert np.max(np.abs(res[j].numpy()[:, :9, :, c] - fd)) <= 1e-6 * np.max(np.abs(res[j].numpy())), (c, j)
    # the base model is only read: its own latents are not the view's
    m.predict_hess(x0)
    assert not np.array_equal(m.d2ghat.numpy(), hm)
    for call in (view.predict_hess, view.predict_grad_cov):
        with pytest.raises(ValueError, match='x0 must have shape'):
            call(np.zeros((3, 3)))


def test_queries_raise_when_the_view_is_stale():
    m, x, y, xn, yn = hess_model('full')
    view = m.condition(xn, yn)
    x0 = x[:3] + 0.01
    view.predict_hess(x0)
    view.active_subspace(x0)
    m._set_flat(m._get_flat() + 0.01)
    calls = (lambda: view.predict_hess(x0), lambda: view.predict_grad_cov(x0), lambda: view.predict_grad_cov(x0, latent=True),
             lambda: view.active_subspace(x0), lambda: view.predict_differentiable(torch.as_tensor(x0), order=2))
    for call in calls:
        with pytest.raises(RuntimeError, match='stale'):
            call()
    m.predict(x0)                                        # the workspace now holds another factorisation
    for call in calls:
        with pytest.raises(RuntimeError, match='stale'):
            call()
    v2 = m.condition(xn, yn)
    assert v2.predict_hess(x0)[0].shape == (3, 3, 2, 2) and v2.predict_grad_cov(x0).shape == (3, 3, 2, 2)


@pytest.mark.parametrize('kernel', ['se', 'matern52'])
def test_order_two_gradgradcheck_and_hessian(kernel):
    m, x, _, xn, yn = hess_model('full', kernel)
    view = m.condition(xn, yn)
    x0 = _x0(x, 2, 3)[:3]
    xt = torch.tensor(x0, dtype=torch.float64, requires_grad=True)

    def f(t):
        return view.predict_differentiable(t, order=2)
    outs = f(torch.as_tensor(x0))
    for a, b in zip(outs, view.predict(x0)):
        assert torch.equal(a, b)
    assert torch.autograd.gradcheck(f, (xt,), eps=1e-6, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradgradcheck(f, (xt,), eps=1e-6, atol=1e-5, rtol=1e-4)
    d2yp, _, d2ycv = view.predict_hess(x0)
    for j, want in ((0, d2yp), (1, d2ycv)):
        H = torch.autograd.functional.hessian(lambda t: f(t)[j].sum(), xt.detach())
        for i in range(3):
            np.testing.assert_allclose(H[i, :, i, :].numpy(), want[:, i].sum(dim=0).numpy(), rtol=1e-12, atol=1e-14)
            for k in range(3):
                if k != i:
                    assert torch.all(H[i, :, k, :] == 0)        # output row i depends on x0[i] alone
    # a first-order use of order=2 equals order=1
    (g2,) = torch.autograd.grad(f(xt)[0].sum(), xt)
    (g1,) = torch.autograd.grad(view.predict_differentiable(xt)[0].sum(), xt)
    assert torch.equal(g1, g2)


def test_order_one_still_refuses_double_backward_and_bad_orders_are_refused():
    m, x, _, xn, yn = hess_model('rep')
    view = m.condition(xn, yn)
    xt = torch.tensor(_x0(x, 2, 3)[:3], dtype=torch.float64, requires_grad=True)
    for f in (view.predict_differentiable, lambda t: view.predict_differentiable(t, order=1)):
        with pytest.raises(RuntimeError, match='double backward'):
            torch.autograd.grad(f(xt)[0].sum(), xt, create_graph=True)
    with pytest.raises(ValueError, match='order must be 1 or 2'):
        view.predict_differentiable(xt, order=3)
    (g,) = torch.autograd.grad(view.predict_differentiable(xt, order=2)[0].sum(), xt, create_graph=True)
    with pytest.raises(RuntimeError, match='triple'):              # (the Hessians are constants, not a graph)
        torch.autograd.grad(g.sum(), xt, create_graph=True)


@pytest.mark.parametrize('mode,kernel', [('full', 'matern32'), ('rep', 'se'), ('full', 'matern52')])
def test_active_subspace_is_the_weighted_sum_of_the_per_point_queries(mode, kernel):
    m, x, _, xn, yn = hess_model(mode, kernel)
    view = m.condition(xn, yn)
    x_ref = _x0(x, 2, 12, seed=9)
    rng = np.random.default_rng(4)
    for weights, outputs in ((None, None), (rng.uniform(0.1, 1.0, len(x_ref)), [2, 0])):
        res = view.active_subspace(x_ref, weights, outputs)
        w = np.full(len(x_ref), 1.0 / len(x_ref)) if weights is None else weights / weights.sum()
        sel = list(range(3)) if outputs is None else outputs
        g = view.predict_grad(x_ref)[0].numpy()[sel]
        cov = view.predict_grad_cov(x_ref).numpy()[sel]
        mean_part, cov_part = np.einsum('i,ail,aim->alm', w, g, g), np.einsum('i,ailm->alm', w, cov)
        big = np.max(np.abs(mean_part + cov_part))
        assert np.max(np.abs(res.mean_part.numpy() - mean_part)) <= 1e-11 * big
        assert np.max(np.abs(res.cov_part.numpy() - cov_part)) <= 1e-11 * big
        assert np.max(np.abs(res.matrix.numpy() - mean_part - cov_part)) <= 1e-11 * big
        assert res.matrix.shape == (len(sel), 2, 2) and torch.equal(res.matrix, res.matrix.transpose(-1, -2))
        assert torch.equal(res.activity, torch.diagonal(res.matrix, dim1=-2, dim2=-1))
        assert torch.all(res.eigenvalues[:, 0] >= res.eigenvalues[:, 1])
        # the new runs settle part of the ranking: the covariance part shrinks
        base = m.active_subspace(x_ref, weights, outputs)
        assert np.all(np.trace(res.cov_part.numpy(), axis1=1, axis2=2) < np.trace(base.cov_part.numpy(), axis1=1, axis2=2))
    for args, msg in (((x_ref, np.ones(3)), 'weights must have length'), ((x_ref, -np.ones(len(x_ref))), 'non-negative'),
                      ((x_ref, np.zeros(len(x_ref))), 'all be zero'), ((x_ref, None, [3]), 'outputs must be'),
                      ((np.zeros((4, 3)),), 'x_ref must have shape')):
        with pytest.raises(ValueError, match=msg):
            view.active_subspace(*args)


def test_two_ranks_gather_what_one_rank_computes():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_condition_hess_host_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


# ---- the C entries -------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ('lcgp_condition_predict_hess_scratch_bytes', 'lcgp_condition_predict_hess',
               'lcgp_condition_predict_gradcov_scratch_bytes', 'lcgp_condition_predict_gradcov')


def test_new_symbols_version_and_sizes():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() == 610
    for name in NEW_SYMBOLS:
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    from lcgp_amd.engine import HotPathEngine
    from lcgp_amd.lcgp import ConditionedLCGP
    assert all(hasattr(HotPathEngine, a) for a in ('condition_predict_hess_block', 'condition_grad_cov_block'))
    assert all(hasattr(ConditionedLCGP, a) for a in ('predict_hess', 'predict_grad_cov', 'active_subspace'))
    nb = C.c_size_t(0)

    def hs(m, n0, d=6, dtype=0, n=4096, q=8):
        assert lib.lcgp_condition_predict_hess_scratch_bytes(dtype, n, d, q, m, n0, C.byref(nb)) == 0, lib.lcgp_last_error()
        return nb.value

    def gs(m, n0, d=6, dtype=0, n=4096, q=8):
        assert lib.lcgp_condition_predict_gradcov_scratch_bytes(dtype, n, d, q, m, n0, C.byref(nb)) == 0, lib.lcgp_last_error()
        return nb.value

    def grad_sb(m, n0, dtype=0, n=4096, q=8):
        assert lib.lcgp_condition_predict_grad_scratch_bytes(dtype, n, q, m, n0, C.byref(nb)) == 0, lib.lcgp_last_error()
        return nb.value

    ms, n0s = (1, 64, 128, 129, 256, 1000, 1024), (1, 10, 21, 22, 127, 128, 129, 341)
    for dtype in (0, 1):
        for fn in (hs, gs):
            for a, b in zip(ms, ms[1:]):
                for n0 in n0s:
                    assert fn(a, n0, dtype=dtype) <= fn(b, n0, dtype=dtype)
            for m in ms:
                for a, b in zip(n0s, n0s[1:]):
                    assert fn(m, a, dtype=dtype) <= fn(m, b, dtype=dtype)
        for m in ms:
            for n0 in n0s:
                assert hs(m, n0, dtype=dtype) == grad_sb(m, n0, dtype) + gs(m, n0, dtype=dtype)
    # the documented sizes: q rows_pad (2 npad + 3 mpad) elements (P' of npad + mpad, DX of npad, two blocks of mpad), rows_pad =
    # n0 d padded to 64 below 128 rows and to 128 from there
    assert gs(1000, 341) == 8 * 2048 * (2 * 4096 + 3 * 1024) * 8 and gs(1000, 341, dtype=1) == gs(1000, 341) // 2
    assert gs(1, 10) == 8 * 64 * (2 * 4096 + 3 * 128) * 8 and gs(1, 22) == 8 * 256 * (2 * 4096 + 3 * 128) * 8
    assert gs(70, 130, d=1, n=333, q=3) == 3 * 256 * (2 * 384 + 3 * 128) * 8
    for fn in (lib.lcgp_condition_predict_hess_scratch_bytes, lib.lcgp_condition_predict_gradcov_scratch_bytes):
        for args, msg in (((0, 4096, 6, 8, 0, 1), b'm < 1'), ((0, 4096, 6, 8, 5, 0), b'n0 < 1'), ((2, 4096, 6, 8, 5, 1), b'dtype'),
                          ((0, 0, 6, 8, 5, 1), b'n, q_local'), ((0, 4096, 6, 0, 5, 1), b'n, q_local'),
                          ((0, 4096, 0, 8, 5, 1), b'd must be'), ((0, 4096, 127, 8, 5, 1), b'd must be'),
                          ((0, 4096, 6, 8, 5, 1 << 28), b'LCGP_HESS_MAX_ROWS')):
            assert fn(*args, C.byref(nb)) < 0
            assert msg in lib.lcgp_last_error(), (args, lib.lcgp_last_error())
        assert fn(0, 4096, 6, 8, 5, 1, None) < 0


def test_c_abi_argument_checks():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything
    big = 1 << 40

    def hess(dtype=0, kern=0, n=50, d=2, q=2, m=4, n0=3, x=dummy, theta=dummy, ws=dummy, state=dummy, xn=dummy, gstate=dummy,
             x0=dummy, scratch=dummy, nsc=big, outs=(dummy,) * 6, stride=0):
        return lib.lcgp_condition_predict_hess(None, dtype, kern, n, d, 3, q, x, None, theta, ws, state, m, xn, gstate, n0, x0,
                                               scratch, nsc, *outs, stride)

    def gcov(dtype=0, kern=0, n=50, d=2, q=2, m=4, n0=3, x=dummy, theta=dummy, ws=dummy, state=dummy, xn=dummy, gstate=dummy,
             x0=dummy, scratch=dummy, nsc=big, dghat=dummy, gamma=dummy, w=None, M=None, stride=0):
        return lib.lcgp_condition_predict_gradcov(None, dtype, kern, n, d, 3, q, x, None, theta, ws, state, m, xn, gstate, n0, x0,
                                                  scratch, nsc, dghat, gamma, w, M, stride)

    nb = C.c_size_t(0)
    common = [(dict(m=0), 'm < 1'), (dict(dtype=2), 'dtype'), (dict(d=0), 'd must be'), (dict(d=127), 'd must be'),
              (dict(n=0), 'n < 1'), (dict(q=0), 'q_local'), (dict(kern=3), 'kernel_id'), (dict(n0=0), 'n0 < 1'),
              (dict(n0=1 << 28), 'LCGP_HESS_MAX_ROWS'), (dict(stride=2), 'out_stride'), (dict(nsc=0), 'scratch is smaller')] + \
             [(dict([(k, None)]), 'NULL') for k in ('x', 'theta', 'ws', 'state', 'xn', 'gstate', 'x0', 'scratch')]
    assert lib.lcgp_condition_predict_hess_scratch_bytes(0, 50, 2, 2, 4, 3, C.byref(nb)) == 0
    for kw, msg in common + [(dict(nsc=nb.value - 1), 'scratch is smaller')] + \
            [(dict(outs=(dummy,) * i + (None,) + (dummy,) * (5 - i)), 'NULL') for i in range(6)]:
        assert hess(**kw) == -1, kw
        assert msg.encode() in lib.lcgp_last_error(), (kw, lib.lcgp_last_error())
    assert lib.lcgp_condition_predict_gradcov_scratch_bytes(0, 50, 2, 2, 4, 3, C.byref(nb)) == 0
    for kw, msg in common + [(dict(nsc=nb.value - 1), 'scratch is smaller'), (dict(dghat=None), 'NULL'),
                             (dict(gamma=None), 'gamma may only be NULL'), (dict(w=dummy), 'w and M go together'),
                             (dict(M=dummy), 'w and M go together')]:
        assert gcov(**kw) == -1, kw
        assert msg.encode() in lib.lcgp_last_error(), (kw, lib.lcgp_last_error())
