"""CPU tests of the input gradients and the calibration target of a conditioned view (ConditionedLCGP.predict_grad /
predict_differentiable / calibration): a numpy stand-in of HotPathEngine.condition_predict_grad_block written from the closed
form of include/lcgp_hip.h (w, z', R, U', V' and the contraction over n + m columns), checked against central differences of
the closed-form view prediction and against brute force (augment the training set, refactor, lcgp_predict_grad's formulas);
the host layer -- shapes, dtypes, the raw-scale output map on non-unit input ranges, latent=True, staleness, autograd, two
ranks -- through that stand-in; view.calibration against tests/calib_ref.py fed with the brute-force latents; and the symbols,
argument checks and sizes of the new C entries (tests/test_gpu_condition_grad.py runs the same through liblcgp_hip.so)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from tests import calib_ref as ref
from tests.test_condition_host import (KERNELS, CondOracleEngine, _free_port, closed_form_predict, make_model, new_columns,
                                       patch_cond)
from tests.test_predict_hess_host import _cross, latent_hessians

HERE = os.path.dirname(os.path.abspath(__file__))


def kernel_derivative(x0, x, ell, c, kernel):
    """(n0, n, d): d c(x0_i, x_j) / d x0_il for the kernel values c, lcgp_predict_grad's dc_l (0 at dx_l = 0)"""
    s = (x0[:, None, :] - x[None, :, :]) / ell
    a = np.abs(s)
    h = {'matern32': s / (1.0 + a), 'se': s, 'matern52': s * (1.0 + a) / (3.0 + 3.0 * a + a * a)}[kernel]
    return -c[:, :, None] * h / ell


def closed_form_predict_grad(th, low, z, x, sr, kernel, xn, Un, LS, v, x0):
    """(dghat', dgvar') (n0, d) of one component in the closed form of include/lcgp_hip.h (lcgp_condition_predict_grad)"""
    d = x.shape[1]
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    c = _cross(x0, x, ell, scale, nug, kernel)
    cx = _cross(x0, xn, ell, scale, nug, kernel)
    U0 = sla.solve_triangular(low, (c * sr[None, :]).T, lower=True).T
    T = sla.solve_triangular(LS, (cx - D * U0 @ Un.T).T, lower=True).T
    w = sla.solve_triangular(LS.T, v, lower=False)                               # L_S^-T v
    zp = z - D * sla.solve_triangular(low.T, Un.T @ w, lower=False)              # z - D W^T (U_n^T w),  W = L^-1
    R = sla.solve_triangular(LS.T, T.T, lower=False).T                           # T L_S^-1
    Vp = sla.solve_triangular(low.T, (U0 - R @ Un).T, lower=False).T             # U' W
    dc, dcx = kernel_derivative(x0, x, ell, c, kernel), kernel_derivative(x0, xn, ell, cx, kernel)
    jm = np.einsum('ijl,j->il', dc, sr * zp) + np.einsum('ial,a->il', dcx, w)
    jv = -2.0 * D * np.einsum('ijl,ij->il', dc, sr[None, :] * Vp) - 2.0 * np.einsum('ial,ia->il', dcx, R)
    return jm, jv


class CondGradOracleEngine(CondOracleEngine):
    """CondOracleEngine plus condition_predict_grad_block, in numpy float64"""
    device = torch.device('cpu')        # (where a several-rank calibration target puts the gathered blocks)

    def condition_predict_grad_block(self, state, x0s):
        blk = self.condition_predict_block(state, x0s)
        x0 = np.asarray(x0s, np.float64)
        sr = np.ones(self.n) if self.sr is None else self.sr
        jac = np.zeros((2, self.q_local) + x0.shape)
        for i, (th, low, z, b) in enumerate(self._state):
            jac[0, i], jac[1, i] = closed_form_predict_grad(th, low, z, self.x, sr, self.kernel, state['xn'], *state['state'][i], x0)
        return blk, torch.as_tensor(jac)


def grad_model(mode, kernel='matern32', d=2, **kw):
    m, x, y, xn, yn = make_model(mode, kernel, d, **kw)
    return patch_cond(m, CondGradOracleEngine), x, y, xn, yn


def _x0(x, d, n0=9, seed=3):
    """new inputs on the raw scale of make_model, two training inputs among them"""
    return np.vstack([-1.5 + 4.0 * np.random.default_rng(seed).uniform(0.05, 0.95, (n0, d)), x[:2]])


def brute_force_grad(m, xn, yn, x0):
    """ghat, gvar (q, n0) and dghat, dgvar (q, n0, d) from first principles: the training set augmented by the new columns, A
    rebuilt and factorised, lcgp_predict_grad's formulas on the augmented matrix (tests/test_predict_hess_host.latent_hessians)"""
    eng = m._aux_engine
    s = np.ones(eng.n) if eng.sr is None else eng.sr
    xn_s, snew, ycol = new_columns(m, xn, yn)
    xa, sa, Ya = np.vstack([eng.x, xn_s]), np.r_[s, snew], np.hstack([eng.Y, ycol])
    x0s = m._standardise_x0(x0)[0]
    d = xa.shape[1]
    out = []
    for th in eng._theta_last:
        ell, scale, nug, D, psi = th[:d], th[d], th[d + 1], th[d + 2], th[d + 3:]
        Cm = _cross(xa, xa, ell, scale, nug, eng.kernel)
        Cm[np.arange(len(xa)), np.arange(len(xa))] = scale
        low = np.linalg.cholesky(np.eye(len(xa)) + D * Cm * np.outer(sa, sa))
        out.append(latent_hessians(x0s, xa, sa, th, low, sla.cho_solve((low, True), Ya.T @ psi), eng.kernel)[:4])
    return [np.stack([o[i] for o in out]) for i in range(4)]


@pytest.mark.parametrize('d', [1, 3])
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_closed_form_equals_central_differences_and_brute_force(mode, kernel, d):
    m, x, _, xn, yn = grad_model(mode, kernel, d)
    x0 = _x0(x, d)[:9]                                      # (central differences: clear of the kinks at training inputs)
    view = m.condition(xn, yn)
    gh, gv, jm, jv = [t.numpy() for t in view.predict_grad(x0, latent=True)]
    assert gh.shape == gv.shape == (2, 9) and jm.shape == jv.shape == (2, 9, d)
    # central differences of the closed-form view prediction, per component, on the standardised scale
    eng, st = m._aux_engine, view._state
    sr = np.ones(eng.n) if eng.sr is None else eng.sr
    x0s = m._standardise_x0(x0)[0]
    h = 1e-5
    for i, (th, low, z, b) in enumerate(eng._state):
        def f(p):
            return closed_form_predict(th, low, z, eng.x, sr, eng.kernel, st['xn'], *st['state'][i], p)
        for l in range(d):
            e = np.zeros(d)
            e[l] = h
            (mp, vp), (mm, vm) = f(x0s + e), f(x0s - e)
            fm, fv = (mp - mm) / (2 * h), (vp - vm) / (2 * h)
            assert np.max(np.abs(jm[i, :, l] - fm)) <= 1e-6 * np.max(np.abs(jm[i])), (i, l)
            assert np.max(np.abs(jv[i, :, l] - fv)) <= 1e-6 * np.max(np.abs(jv[i])), (i, l)
    # brute force on the augmented training set, training inputs among the new inputs (same = 0: the continuous surface)
    x1 = np.vstack([_x0(x, d), view.x_new.numpy()[:2]])
    got = [t.numpy() for t in view.predict_grad(x1, latent=True)]
    want = brute_force_grad(m, xn, yn, x1)
    for a, b in zip(got, want):
        assert a.shape == b.shape
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-8 * np.max(np.abs(b)))
    base = m._aux_engine.predict_grad_block(m._standardise_x0(x1)[0])[1].numpy()
    assert np.max(np.abs(got[2] - base[0])) > 1e-3 * np.max(np.abs(base[0]))      # the new runs did something


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_host_layer_shapes_dtypes_output_map_and_range_scaling(mode):
    m, x, _, xn, yn = grad_model(mode)
    view = m.condition(torch.as_tensor(xn), torch.as_tensor(yn))
    x0 = _x0(x, 2)
    res = view.predict_grad(torch.as_tensor(x0))
    assert len(res) == 3
    for a in res:
        assert isinstance(a, torch.Tensor) and a.dtype == torch.float64 and a.shape == (3, 11, 2)
        assert a.device.type == 'cpu' and not a.requires_grad and torch.all(torch.isfinite(a))
    assert torch.equal(res[1], res[2]) and res[1] is not res[2]
    gh, gv, jm, jv = view.predict_grad(x0, latent=True)
    assert gh.shape == gv.shape == (2, 11) and jm.shape == jv.shape == (2, 11, 2) and jm.dtype == torch.float64
    a, b = view.predict(x0, latent=True)
    assert torch.equal(gh, a) and torch.equal(gv, b)
    # the base model's output map and its division by the input ranges (4.0 in every dimension here)
    W, _, scale, _ = m._output_map()
    rng = (m.x_max.numpy() - m.x_min.numpy()).reshape(-1)
    assert np.all(rng > 3.0)
    want = np.einsum('ka,kil->ail', W, jm.numpy()) * scale[:, None, None] / rng[None, None, :]
    np.testing.assert_allclose(res[0].numpy(), want, rtol=1e-13)
    want = np.einsum('ka,kil->ail', W ** 2, jv.numpy()) * (scale ** 2)[:, None, None] / rng[None, None, :]
    np.testing.assert_allclose(res[2].numpy(), want, rtol=1e-13)
    # central differences of view.predict on the raw scale, away from the training inputs
    h = 1e-5 * rng
    for l in range(2):
        e = np.zeros(2)
        e[l] = h[l]
        p, q = view.predict(x0[:9] + e), view.predict(x0[:9] - e)
        for k, j in ((0, 0), (2, 2)):
            fd = (p[k].numpy() - q[k].numpy()) / (2 * h[l])
            assert np.max(np.abs(res[j].numpy()[:, :9, l] - fd)) <= 1e-6 * np.max(np.abs(res[j].numpy())), (l, k)
    # the base model is only read: its own latent Jacobians are not the view's
    m.predict_grad(x0)
    assert not np.array_equal(m.dghat.numpy(), jm.numpy())
    with pytest.raises(ValueError, match='x0 must have shape'):
        view.predict_grad(np.zeros((3, 3)))


def test_queries_raise_when_the_view_is_stale():
    m, x, y, xn, yn = grad_model('full')
    m._calib_rows_device = ref.rows_as_host_stub
    view = m.condition(xn, yn)
    x0 = x[:3] + 0.01
    tgt = view.calibration(y[:, 2], 0.3)
    view.predict_grad(x0)
    tgt.loglik_grad(x0)
    m._set_flat(m._get_flat() + 0.01)
    calls = (lambda: view.predict_grad(x0), lambda: view.predict_grad(x0, latent=True),
             lambda: view.predict_differentiable(torch.as_tensor(x0)), lambda: view.calibration(y[:, 2], 0.3),
             lambda: tgt.loglik(x0), lambda: tgt.loglik_grad(x0), lambda: tgt.loglik_differentiable(torch.as_tensor(x0)))
    for call in calls:
        with pytest.raises(RuntimeError, match='stale'):
            call()
    m.predict(x0)                                        # the workspace now holds another factorisation
    for call in calls:
        with pytest.raises(RuntimeError, match='stale'):
            call()
    v2 = m.condition(xn, yn)
    assert v2.predict_grad(x0)[0].shape == (3, 3, 2) and v2.calibration(y[:, 2], 0.3).loglik(x0).shape == (3,)


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_predict_differentiable_first_order_and_no_double_backward(mode):
    m, x, _, xn, yn = grad_model(mode)
    view = m.condition(xn, yn)
    x0 = _x0(x, 2, 4)[:4]
    outs = view.predict_differentiable(torch.as_tensor(x0))
    for a, b in zip(outs, view.predict(x0)):
        assert not a.requires_grad and torch.equal(a, b)
    xt = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(view.predict_differentiable, (xt,), eps=1e-6, atol=1e-6, rtol=1e-5)
    dyp, _, dycv = view.predict_grad(x0)
    (g,) = torch.autograd.grad(view.predict_differentiable(xt)[0].sum(), xt)
    np.testing.assert_allclose(g.numpy(), dyp.sum(dim=0).numpy(), rtol=1e-13)
    (g,) = torch.autograd.grad(view.predict_differentiable(xt)[1].sum(), xt)
    np.testing.assert_allclose(g.numpy(), dycv.sum(dim=0).numpy(), rtol=1e-13)
    with pytest.raises(RuntimeError, match='double backward'):
        torch.autograd.grad(view.predict_differentiable(xt)[0].sum(), xt, create_graph=True)


# ---- calibration on the view ---------------------------------------------------------------------------------------------
def _observation(y, form, seed=3):
    rng = np.random.default_rng(seed)
    p = y.shape[0]
    sd = y.std(axis=1)
    y_obs = y[:, 5] + 0.1 * sd * rng.standard_normal(p)
    var = (sd * rng.uniform(0.05, 0.15, p)) ** 2
    B = 0.1 * sd[:, None] * rng.standard_normal((p, 2))
    return y_obs, {'scalar': float(var.mean()), 'diag': var, 'dense': np.diag(var) + B @ B.T}[form]


@pytest.mark.parametrize('form', ['scalar', 'diag', 'dense'])
@pytest.mark.parametrize('mode,kernel', [('full', 'matern32'), ('rep', 'se'), ('full', 'matern52')])
def test_view_calibration_equals_the_dense_density_of_the_augmented_latents(mode, kernel, form):
    m, x, y, xn, yn = grad_model(mode, kernel)
    m._calib_rows_device = ref.rows_as_host_stub
    view = m.condition(xn, yn)
    theta = np.vstack([_x0(x, 2), view.x_new.numpy()[:1]])
    gh, gv, jm, jv = brute_force_grad(m, xn, yn, theta)
    inv_range = 1.0 / (m.x_max.numpy() - m.x_min.numpy()).reshape(-1)
    for nan_at in ((), (1,)):
        y_obs, obs_var = _observation(y, form)
        y_obs[list(nan_at)] = np.nan
        tgt = view.calibration(y_obs, obs_var)
        assert tgt.model is m and list(np.flatnonzero(~tgt.observed)) == list(nan_at)
        _, phi_s, t, lam = ref.observation(m, y_obs, obs_var)
        want, _, dwant, _, _ = ref.dense_loglik(phi_s, t, lam, gh, gv, jm, jv, inv_range)
        ll = tgt.loglik(theta)
        assert ll.shape == (12,) and ll.dtype == torch.float64 and ll.device.type == 'cpu'
        np.testing.assert_allclose(ll.numpy(), want, rtol=1e-9, atol=1e-9)
        ll2, dll = tgt.loglik_grad(theta)
        assert torch.equal(ll2, ll) and dll.shape == (12, 2)
        np.testing.assert_allclose(dll.numpy(), dwant, rtol=0, atol=1e-7 * np.max(np.abs(dwant)))
        # the view's target is not the base model's
        assert np.max(np.abs(ll.numpy() - m.calibration(y_obs, obs_var).loglik(theta).numpy())) > 1e-6
    # the folding is the base model's code
    a, b = view.calibration(y_obs, obs_var), m.calibration(y_obs, obs_var)
    assert np.array_equal(a.M, b.M) and np.array_equal(a.b, b.b) and (a.c0, a.lognorm) == (b.c0, b.lognorm)
    assert view.calibration(y_obs, obs_var, include_noise=False).lognorm < a.lognorm


@pytest.mark.parametrize('mode,form', [('full', 'dense'), ('rep', 'diag')])
def test_view_loglik_grad_equals_central_differences_and_autograd(mode, form):
    m, x, y, xn, yn = grad_model(mode)
    m._calib_rows_device = ref.rows_as_host_stub
    view = m.condition(xn, yn)
    y_obs, obs_var = _observation(y, form)
    y_obs[2] = np.nan
    tgt = view.calibration(y_obs, obs_var)
    theta = _x0(x, 2)[:9]
    ll, dll, s, v = tgt.loglik_grad(theta, latent=True)
    assert dll.shape == (9, 2) and s.shape == v.shape == (2, 9)
    h = 1e-5 * (m.x_max.numpy() - m.x_min.numpy()).reshape(-1)
    fd = np.zeros((9, 2))
    for l in range(2):
        e = np.zeros(2)
        e[l] = h[l]
        fd[:, l] = (tgt.loglik(theta + e).numpy() - tgt.loglik(theta - e).numpy()) / (2 * h[l])
    assert np.max(np.abs(dll.numpy() - fd)) <= 1e-6 * np.max(np.abs(fd)), (np.max(np.abs(dll.numpy() - fd)), np.max(np.abs(fd)))
    tt = torch.tensor(theta[:4], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(tgt.loglik_differentiable, (tt,), eps=1e-6, atol=1e-6, rtol=1e-5)
    (g,) = torch.autograd.grad(tgt.loglik_differentiable(tt).sum(), tt)
    assert torch.equal(g, dll[:4])
    with pytest.raises(RuntimeError, match='double backward'):
        torch.autograd.grad(tgt.loglik_differentiable(tt).sum(), tt, create_graph=True)


def test_view_calibration_argument_errors_are_the_base_models():
    m, x, y, xn, yn = grad_model('full')
    view = m.condition(xn, yn)
    p = 3
    y_obs, dense = _observation(y, 'dense')
    for args, exc, msg in (((y_obs[:2], 1.0), ValueError, 'y_obs'), ((np.full(p, np.nan), 1.0), ValueError, 'no observed'),
                           ((np.where(np.arange(p) == 1, np.inf, y_obs), 1.0), ValueError, 'finite'),
                           ((y_obs, np.ones(p + 1)), ValueError, 'obs_var'), ((y_obs, -1.0), ValueError, 'non-negative'),
                           ((y_obs, dense + np.triu(np.full((p, p), 1e-3), 1)), ValueError, 'symmetric')):
        with pytest.raises(exc, match=msg):
            view.calibration(*args)
    with pytest.raises(np.linalg.LinAlgError):
        view.calibration(y_obs, 0.0, include_noise=False)
    with pytest.raises(np.linalg.LinAlgError):
        view.calibration(y_obs, np.full((p, p), 1.0) - np.diag([0.0, 0.0, 0.5]), include_noise=False)
    with pytest.raises(ValueError, match='theta'):
        view.calibration(y_obs, dense).loglik(np.zeros((3, 5)))


def test_two_ranks_gather_what_one_rank_computes():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_condition_grad_host_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


# ---- the C entries -------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ('lcgp_condition_grad_state_bytes', 'lcgp_condition_grad_prepare', 'lcgp_condition_predict_grad_scratch_bytes',
               'lcgp_condition_predict_grad')


def test_new_symbols_version_and_sizes():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() == 610
    for name in NEW_SYMBOLS:
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    from lcgp_amd.engine import HotPathEngine
    from lcgp_amd.lcgp import ConditionedLCGP
    assert hasattr(HotPathEngine, 'condition_predict_grad_block')
    assert all(hasattr(ConditionedLCGP, a) for a in ('predict_grad', 'predict_differentiable', 'calibration'))
    nb = C.c_size_t(0)

    def gs(m, dtype=0, n=4096, q=8):
        assert lib.lcgp_condition_grad_state_bytes(dtype, n, q, m, C.byref(nb)) == 0, lib.lcgp_last_error()
        return nb.value

    def sb(m, n0, dtype=0, n=4096, q=8):
        assert lib.lcgp_condition_predict_grad_scratch_bytes(dtype, n, q, m, n0, C.byref(nb)) == 0, lib.lcgp_last_error()
        return nb.value

    def cond_sb(m, n0, dtype=0, n=4096, q=8):
        assert lib.lcgp_condition_scratch_bytes(dtype, n, q, m, n0, C.byref(nb)) == 0, lib.lcgp_last_error()
        return nb.value

    ms, n0s = (1, 64, 128, 129, 256, 1000, 1024, 4096), (1, 64, 127, 128, 129, 1000, 2048)
    for dtype in (0, 1):
        for a, b in zip(ms, ms[1:]):
            assert gs(a, dtype) <= gs(b, dtype)
            for n0 in n0s:
                assert sb(a, n0, dtype) <= sb(b, n0, dtype)
        for m in ms:
            for a, b in zip(n0s, n0s[1:]):
                assert sb(m, a, dtype) <= sb(m, b, dtype)
            assert sb(m, 2048, dtype) <= cond_sb(m, 2048, dtype)            # a pass needs no more than lcgp_condition_predict's
    # the documented sizes: (mpad + 2 npad) doubles per component in either dtype; 2 n0pad (npad + mpad) elements
    assert gs(1000) == gs(1000, 1) == 8 * (1024 + 2 * 4096) * 8
    assert gs(1, n=333, q=3) == 3 * (128 + 2 * 384) * 8
    assert sb(1000, 2048) == 2 * 8 * 2048 * (4096 + 1024) * 8 and sb(1000, 2048, 1) == sb(1000, 2048) // 2
    for args, msg in (((0, 4096, 8, 0), b'm < 1'), ((2, 4096, 8, 5), b'dtype'), ((0, 0, 8, 5), b'n, q_local'),
                      ((0, 4096, 0, 5), b'n, q_local')):
        assert lib.lcgp_condition_grad_state_bytes(*args, C.byref(nb)) < 0
        assert msg in lib.lcgp_last_error()
    assert lib.lcgp_condition_grad_state_bytes(0, 4096, 8, 5, None) < 0
    for args, msg in (((0, 4096, 8, 0, 1), b'm < 1'), ((0, 4096, 8, 5, 0), b'n0 < 1'), ((2, 4096, 8, 5, 1), b'dtype'),
                      ((0, 0, 8, 5, 1), b'n, q_local')):
        assert lib.lcgp_condition_predict_grad_scratch_bytes(*args, C.byref(nb)) < 0
        assert msg in lib.lcgp_last_error()
    assert lib.lcgp_condition_predict_grad_scratch_bytes(0, 4096, 8, 5, 1, None) < 0


def test_c_abi_argument_checks():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything
    big = 1 << 40

    def prep(dtype=0, n=50, d=2, q=2, m=4, theta=dummy, ws=dummy, state=dummy, gstate=dummy):
        return lib.lcgp_condition_grad_prepare(None, dtype, n, d, 3, q, theta, ws, state, m, gstate)

    def pred(dtype=0, kern=0, n=50, d=2, q=2, m=4, n0=3, x=dummy, theta=dummy, ws=dummy, state=dummy, xn=dummy, gstate=dummy,
             x0=dummy, scratch=dummy, nsc=big, ghat=dummy, gvar=dummy, dghat=dummy, dgvar=dummy, stride=0):
        return lib.lcgp_condition_predict_grad(None, dtype, kern, n, d, 3, q, x, None, theta, ws, state, m, xn, gstate, n0, x0,
                                               scratch, nsc, ghat, gvar, dghat, dgvar, stride)

    nb = C.c_size_t(0)
    assert lib.lcgp_condition_predict_grad_scratch_bytes(0, 50, 2, 4, 3, C.byref(nb)) == 0
    need = nb.value
    common = [(dict(m=0), 'm < 1'), (dict(dtype=2), 'dtype'), (dict(d=0), 'd must be'), (dict(d=127), 'd must be'),
              (dict(n=0), 'n < 1'), (dict(q=0), 'q_local'), (dict(theta=None), 'NULL'), (dict(ws=None), 'NULL'),
              (dict(state=None), 'NULL'), (dict(gstate=None), 'NULL')]
    for kw, msg in common:
        assert prep(**kw) == -1, kw
        assert msg.encode() in lib.lcgp_last_error(), (kw, lib.lcgp_last_error())
    for kw, msg in common + [(dict(kern=3), 'kernel_id'), (dict(x=None), 'NULL'), (dict(xn=None), 'NULL'), (dict(n0=0), 'n0 < 1'),
                             (dict(x0=None), 'NULL'), (dict(scratch=None), 'NULL'), (dict(ghat=None), 'NULL'),
                             (dict(gvar=None), 'NULL'), (dict(dghat=None), 'NULL'), (dict(dgvar=None), 'NULL'),
                             (dict(stride=2), 'out_stride'), (dict(nsc=need - 1), 'scratch is smaller'),
                             (dict(nsc=0), 'scratch is smaller')]:
        assert pred(**kw) == -1, kw
        assert msg.encode() in lib.lcgp_last_error(), (kw, lib.lcgp_last_error())
