"""CPU tests of CalibrationTarget.loglik_hess and loglik_differentiable(order=2): the host layer -- the second-order latent mode,
the mirroring of the packed triangle, the raw-scale chain rule, NaN rows, the three forms of obs_var, full and rep paths, the
three kernels, the autograd wrapper, staleness, a view's target, two ranks -- through the numpy stand-ins of the engine
(tests/test_predict_hess_host.py, tests/test_condition_hess_host.py) with the row kernels replaced by their float64 numpy
restatements (tests/calib_ref.py, tests/calib_hess_ref.py), against the Hessian of the dense p-space density and central
differences of loglik_grad; the validity of the row kernel's tolerance on the GPU test's inputs; and the C entry's argument
checks (tests/test_gpu_calibration_hess.py runs the kernel itself on the GPU)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lcgp_amd import LCGP, synth
from oracle import lcgp_oracle as orc
from tests import calib_hess_ref as href
from tests import calib_ref as ref
from tests.test_calibration_host import LO, P, Q, SPAN, _observation, _theta
from tests.test_condition_hess_host import _free_port, clear_points, hess_model
from tests.test_predict_hess_host import assert_clear_of_kinks, patch_engine

HERE = os.path.dirname(os.path.abspath(__file__))


def _stubs(m):
    m._calib_rows_device = ref.rows_as_host_stub
    m._calib_hess_rows_device = href.rows2_as_host_stub
    return m


def _model(mode, kernel='matern32'):
    """(model through the stand-ins at set parameters, raw x, y): the shapes of tests/test_calibration_host.py, p = 5 outputs,
    q = 3 components, a different input range per dimension"""
    if mode == 'full':
        x, y = synth.make_full(75, 40, 2, P, Q)
    else:
        x, y = synth.make_rep(76, 16, 3, 2, P, Q)
    x = LO + SPAN * x
    m = _stubs(patch_engine(LCGP(y=y, x=x, q=Q, submethod=mode, kernel=kernel)))
    o = orc.OracleLCGP(y=y, x=x, q=Q, submethod=mode)               # (only for the shape of the parameter vector)
    m._set_flat(synth.param_points(75, o.get_unconstrained())[1])
    assert int(m.p) == P and int(m.q) == Q
    return m, x, y


def _inv_range(m):
    return 1.0 / (m.x_max.numpy() - m.x_min.numpy()).reshape(-1)


def _dense(m, src, theta, y_obs, obs_var, include_noise=True):
    """(d2ll (n0, d, d), B (n0, q, q)) of the dense p-space density fed with the stand-in's latents (src: the model or a view)"""
    ghat, gvar, dghat, dgvar, d2ghat, d2gvar = src._latent_predict_hess(theta)
    _, phi_s, t, lam = ref.observation(m, y_obs, obs_var, include_noise)
    want, _ = href.dense_hess(phi_s, t, lam, ghat, gvar, dghat, dgvar, d2ghat, d2gvar, _inv_range(m))
    return want, href.dense_B(phi_s, lam, gvar)


def _assert_hess(tgt, m, src, theta, y_obs, obs_var, include_noise=True):
    n0, d = theta.shape
    ll, dll, d2ll, s, v, B = tgt.loglik_hess(theta, latent=True)
    assert d2ll.shape == (n0, d, d) and d2ll.dtype == torch.float64 and d2ll.device.type == 'cpu'
    assert s.shape == v.shape == (Q, n0) and B.shape == (n0, Q, Q)
    assert torch.equal(d2ll, d2ll.transpose(-1, -2))                # EXACTLY symmetric
    for a, b in zip((ll, dll, s, v), tgt.loglik_grad(theta, latent=True)):
        assert np.array_equal(a.numpy(), b.numpy())                 # bitwise loglik_grad's
    plain = tgt.loglik_hess(theta)
    assert len(plain) == 3 and all(torch.equal(a, b) for a, b in zip(plain, (ll, dll, d2ll)))
    want, wantB = _dense(m, src, theta, y_obs, obs_var, include_noise)
    np.testing.assert_allclose(d2ll.numpy(), want, rtol=1e-9, atol=1e-9 * np.max(np.abs(want)))
    np.testing.assert_allclose(B.numpy(), wantB, rtol=1e-9, atol=1e-9 * np.max(np.abs(wantB)))


@pytest.mark.parametrize('form', ['scalar', 'diag', 'dense'])
@pytest.mark.parametrize('mode,kernel', [('full', 'matern32'), ('rep', 'matern32'), ('full', 'se'), ('rep', 'matern52')])
def test_loglik_hess_equals_the_hessian_of_the_dense_density(mode, kernel, form):
    m, x, y = _model(mode, kernel)
    y_obs, obs_var = _observation(y, form)
    theta = _theta()
    theta[:2] = x[[1, 6]]                                   # training inputs: the continuous surface, no nugget
    _assert_hess(m.calibration(y_obs, obs_var), m, m, theta, y_obs, obs_var)


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_nan_rows_also_fewer_observed_than_components_and_no_noise(mode):
    m, x, y = _model(mode)
    y_obs, obs_var = _observation(y, 'dense')
    theta = _theta()
    for keep in ([0, 1, 3, 4], [1, 3]):                     # |O| = 4, and |O| = 2 < q = 3
        yo = np.full(P, np.nan)
        yo[keep] = y_obs[keep]
        _assert_hess(m.calibration(yo, obs_var), m, m, theta, yo, obs_var)
    y_obs, var = _observation(y, 'diag')
    _assert_hess(m.calibration(y_obs, var, include_noise=False), m, m, theta, y_obs, var, include_noise=False)


def _central_differences_of_loglik_grad(tgt, theta, h):
    """(n0, d, d): [..., l, c] = d/dtheta[i, c] of loglik_grad's dll[..., l], every row perturbed at once"""
    out = np.zeros(theta.shape + (theta.shape[1],))
    for c in range(theta.shape[1]):
        e = np.zeros_like(theta)
        e[:, c] = h[c]
        out[..., c] = (tgt.loglik_grad(theta + e)[1].numpy() - tgt.loglik_grad(theta - e)[1].numpy()) / (2 * h[c])
    return out


@pytest.mark.parametrize('mode,kernel,form', [('full', 'matern32', 'dense'), ('rep', 'matern32', 'diag'), ('full', 'se', 'scalar'),
                                              ('full', 'matern52', 'dense')])
def test_loglik_hess_equals_central_differences_of_loglik_grad(mode, kernel, form):
    """step and bar of tests/test_predict_hess_host.py's central-difference test: 1e-5 of the range, 1e-6 of the largest entry"""
    m, x, y = _model(mode, kernel)
    y_obs, obs_var = _observation(y, form)
    y_obs[2] = np.nan
    theta = _theta(11)
    h = 1e-5 * SPAN
    if kernel == 'matern32':
        assert_clear_of_kinks(theta, x, h)
    tgt = m.calibration(y_obs, obs_var)
    d2ll = tgt.loglik_hess(theta)[2].numpy()
    fd = _central_differences_of_loglik_grad(tgt, theta, h)
    err = np.max(np.abs(d2ll - fd))
    print(mode, kernel, err / np.max(np.abs(fd)))
    assert err <= 1e-6 * np.max(np.abs(fd)), (err, np.max(np.abs(fd)))


def _autograd_checks(tgt, theta, loglik_hess):
    tt = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
    fn = lambda t: tgt.loglik_differentiable(t, order=2)            # noqa: E731
    out = fn(torch.as_tensor(theta))
    assert not out.requires_grad and torch.equal(out, tgt.loglik(theta))
    assert torch.autograd.gradcheck(fn, (tt,), eps=1e-6, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradgradcheck(fn, (tt,), eps=1e-6, atol=1e-5, rtol=1e-4)
    H = torch.autograd.functional.hessian(lambda t: fn(t).sum(), tt.detach())
    n0, d = theta.shape
    assert H.shape == (n0, d, n0, d)
    want = loglik_hess(theta)[2]
    for i in range(n0):
        for j in range(n0):
            blk = want[i] if i == j else torch.zeros(d, d, dtype=torch.float64)
            assert torch.equal(H[i, :, j, :], blk)                  # row i depends on theta[i] alone
    # a first-order use of order=2 equals order=1 and makes no Hessian pass
    (g2,) = torch.autograd.grad(fn(tt).sum(), tt)
    (g1,) = torch.autograd.grad(tgt.loglik_differentiable(tt).sum(), tt)
    assert torch.equal(g1, g2) and not g2.requires_grad and torch.equal(g1, tgt.loglik_grad(theta)[1])


@pytest.mark.parametrize('kernel', ['se', 'matern52'])
def test_order_two_gradgradcheck_and_hessian(kernel):
    m, x, y = _model('full', kernel)
    y_obs, obs_var = _observation(y, 'dense')
    tgt = m.calibration(y_obs, obs_var)
    _autograd_checks(tgt, _theta(4), tgt.loglik_hess)


def test_the_hessian_pass_runs_only_in_a_double_backward():
    m, x, y = _model('full')
    y_obs, obs_var = _observation(y, 'diag')
    tgt = m.calibration(y_obs, obs_var)
    calls = []
    stub = m._calib_hess_rows_device
    m._calib_hess_rows_device = lambda *a: calls.append(1) or stub(*a)
    tt = torch.tensor(_theta(3), dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(tgt.loglik_differentiable(tt, order=2).sum(), tt, create_graph=True)
    assert g.requires_grad and not calls
    (gg,) = torch.autograd.grad(g.pow(2).sum(), tt)
    assert len(calls) == 1 and gg.shape == tt.shape and torch.all(torch.isfinite(gg))


def test_order_one_still_refuses_double_backward_third_order_and_bad_orders_are_refused():
    m, x, y = _model('rep')
    y_obs, obs_var = _observation(y, 'dense')
    tgt = m.calibration(y_obs, obs_var)
    tt = torch.tensor(_theta(3), dtype=torch.float64, requires_grad=True)
    for f in (tgt.loglik_differentiable, lambda t: tgt.loglik_differentiable(t, order=1)):
        with pytest.raises(RuntimeError, match='double backward'):
            torch.autograd.grad(f(tt).sum(), tt, create_graph=True)
    (g,) = torch.autograd.grad(tgt.loglik_differentiable(tt, order=2).sum(), tt, create_graph=True)
    with pytest.raises(RuntimeError, match='triple backward'):
        torch.autograd.grad(g.pow(2).sum(), tt, create_graph=True)
    for bad in (0, 3, '2'):
        with pytest.raises(ValueError, match='order must be 1 or 2'):
            tgt.loglik_differentiable(tt, order=bad)


def test_target_goes_stale_when_the_parameters_change():
    m, x, y = _model('full')
    y_obs, obs_var = _observation(y, 'diag')
    tgt = m.calibration(y_obs, obs_var)
    theta = _theta(3)
    tgt.loglik_hess(theta)
    u = m._get_flat().copy()
    u[0] += 0.1
    m._set_flat(u)
    for call in (lambda: tgt.loglik_hess(theta), lambda: tgt.loglik_hess(theta, latent=True),
                 lambda: tgt.loglik_differentiable(torch.as_tensor(theta), order=2)):
        with pytest.raises(RuntimeError, match='stale'):
            call()
    assert m.calibration(y_obs, obs_var).loglik_hess(theta)[2].shape == (3, 2, 2)


# ---- a view's target ---------------------------------------------------------------------------------------------------------
def _view_target(mode, kernel='matern32'):
    m, x, y, xn, yn = hess_model(mode, kernel)
    _stubs(m)
    view = m.condition(xn, yn)
    y_obs = np.asarray(y)[:, 4] + 0.05
    obs_var = np.array([0.3, 0.2, 0.25])
    return m, view, view.calibration(y_obs, obs_var), x, xn, y_obs, obs_var


@pytest.mark.parametrize('mode,kernel', [('full', 'matern32'), ('rep', 'se'), ('full', 'matern52')])
def test_view_target_hessian_dense_density_and_central_differences(mode, kernel):
    m, view, tgt, x, xn, y_obs, obs_var = _view_target(mode, kernel)
    assert tgt._view is view and int(m.q) == 2
    h = 1e-5
    lo, span = m.x_min.numpy().reshape(-1), (m.x_max.numpy() - m.x_min.numpy()).reshape(-1)
    theta = np.vstack([lo + span * clear_points(m, view, 2, 7, h), x[:1], xn[:1]])
    n0 = len(theta)
    ll, dll, d2ll, s, v, B = tgt.loglik_hess(theta, latent=True)
    assert d2ll.shape == (n0, 2, 2) and B.shape == (n0, 2, 2) and torch.equal(d2ll, d2ll.transpose(-1, -2))
    for a, b in zip((ll, dll, s, v), tgt.loglik_grad(theta, latent=True)):
        assert np.array_equal(a.numpy(), b.numpy())
    want, wantB = _dense(m, view, theta, y_obs, obs_var)
    np.testing.assert_allclose(d2ll.numpy(), want, rtol=1e-9, atol=1e-9 * np.max(np.abs(want)))
    np.testing.assert_allclose(B.numpy(), wantB, rtol=1e-9, atol=1e-9 * np.max(np.abs(wantB)))
    # the view's latents, not the model's
    assert np.max(np.abs(d2ll.numpy() - m.calibration(y_obs, obs_var).loglik_hess(theta)[2].numpy())) > 1e-6 * np.max(np.abs(want))
    clear = theta[:7]                                       # (the last two rows sit on Matern-3/2's kinks)
    fd = _central_differences_of_loglik_grad(tgt, clear, h * span)
    err = np.max(np.abs(d2ll.numpy()[:7] - fd))
    assert err <= 1e-6 * np.max(np.abs(fd)), (err, np.max(np.abs(fd)))


def test_view_target_autograd_and_staleness():
    m, view, tgt, x, xn, y_obs, obs_var = _view_target('full', 'se')
    theta = x[:3] + 0.013
    _autograd_checks(tgt, theta, tgt.loglik_hess)
    u0 = m._get_flat().copy()
    m._set_flat(u0 + 0.01)
    for call in (lambda: tgt.loglik_hess(theta), lambda: tgt.loglik_differentiable(torch.as_tensor(theta), order=2)):
        with pytest.raises(RuntimeError, match='stale'):
            call()
    m.predict(theta)                                        # the workspace now holds another factorisation
    m._set_flat(u0)                                         # the target's own parameters again: its VIEW stays stale
    with pytest.raises(RuntimeError, match='stale'):
        tgt.loglik_hess(theta)


def test_two_ranks_gather_what_one_rank_computes():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_calibration_hess_host_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


# ---- the row kernel's tolerance --------------------------------------------------------------------------------------------
def _assert_reversed_inside(inp, q, what):
    r64, rld = href.rows2_of(inp), href.rows2_of(inp, dtype=np.longdouble)
    tol = href.row_tolerances2(r64, rld)
    rev = href.rows2_of(inp, order=np.arange(q)[::-1])
    for k in ('ll', 's', 'v', 'dll', 'B', 'd2ll'):
        err = np.abs(rev[k].astype(np.longdouble) - rld[k])
        print('%s %s: reversed float64 / tolerance %.3g' % (what, k, float(np.max(err / tol[k]))))
        assert np.all(err <= tol[k]), (what, k, float(np.max(err / tol[k])))
        assert np.all(np.abs(r64[k].astype(np.longdouble) - rld[k]) <= tol[k])


@pytest.mark.parametrize('deficient', [0, 1], ids=['full-rank', 'rank-deficient'])
@pytest.mark.parametrize('q', href.ROW_QS)
def test_the_row_tolerance_holds_for_float64_in_reverse_component_order(q, deficient):
    """the validity of tests/test_gpu_calibration_hess.py's tolerance on its own synthetic inputs: a float64 evaluation of the
    same formulas in ANOTHER summation order (the components reversed) must stay inside 4 x max(forward float64 error, eps x
    sum of absolute terms); if it does not, the term expansion of calib_hess_ref.rows2 is wrong"""
    _assert_reversed_inside(href.hess_inputs(q, deficient), q, 'q=%d deficient=%d' % (q, deficient))


def test_the_row_tolerance_holds_on_the_wide_case():
    _assert_reversed_inside(href.wide_inputs(), href.WIDE['q'], 'wide')


# ---- the C entry -------------------------------------------------------------------------------------------------------------
def test_new_symbol_version_and_c_abi_argument_checks():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() == 610
    assert hasattr(lib, 'lcgp_calib_hess_rows') and 'lcgp_calib_hess_rows' in _hip.SIGNATURES
    assert len(_hip.SIGNATURES['lcgp_calib_hess_rows'][1]) == 21
    p = C.c_void_p(16)              # never dereferenced: every call below is refused before it enqueues anything

    def call(q=3, d=2, n0=10, ghat=p, gvar=p, dghat=p, dgvar=p, d2ghat=p, d2gvar=p, stride=0, M=p, b=p, ll=p, dll=p, d2ll=p,
             sens=p, B=p):
        return lib.lcgp_calib_hess_rows(None, q, d, n0, ghat, gvar, dghat, dgvar, d2ghat, d2gvar, stride, M, b, 0.0, 0.0, None,
                                        ll, dll, d2ll, sens, B)

    for kw, word in (({'q': 0}, b'q must'), ({'q': 65}, b'q must'), ({'d': 0}, b'd must'), ({'d': 127}, b'd must'),
                     ({'n0': 0}, b'n0'), ({'d2ghat': None, 'd2gvar': None}, b'd2ll needs the Hessians'),
                     ({'d2ghat': None}, b'both'), ({'d2gvar': None}, b'both'),
                     ({'dghat': None, 'dgvar': None, 'dll': None}, b'd2ll needs the Jacobians'),
                     ({'stride': 9}, b'in_stride'), ({'stride': -1}, b'in_stride'), ({'ghat': None}, b'NULL'),
                     ({'M': None}, b'NULL'), ({'ll': None}, b'NULL'), ({'dghat': None}, b'd2ll needs the Jacobians'),
                     ({'dgvar': None, 'd2ll': None}, b'both')):
        assert call(**kw) < 0, kw
        assert word in lib.lcgp_last_error(), (kw, lib.lcgp_last_error())
