"""CPU tests of LCGP.calibration() / CalibrationTarget: the host layer -- folding the observation into q-space, NaN rows, the
three forms of obs_var, the raw-scale chain rule, full and rep paths, the autograd wrapper, staleness, argument errors --
through the numpy stand-in of the engine (tests/test_predict_grad_host.py) with the row kernel replaced by its float64 numpy
restatement (tests/calib_ref.py), against the dense p-space density built from the oracle's predict; and the C entry's
argument checks (tests/test_gpu_calibration.py runs the kernel itself on the GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

from lcgp_amd import LCGP, synth
from oracle import lcgp_oracle as orc
from tests import calib_ref as ref
from tests.test_predict_grad_host import patch_engine

LO, SPAN = np.array([1.0, -2.0]), np.array([3.0, 0.5])           # a non-unit input range, different per dimension
P, Q = 5, 3


def _pair(mode, kernel='matern32'):
    """(model through the stand-ins, oracle at the same parameters, raw x, y); p = 5 outputs, q = 3 components"""
    if mode == 'full':
        x, y = synth.make_full(75, 40, 2, P, Q)
    else:
        x, y = synth.make_rep(76, 16, 3, 2, P, Q)
    x = LO + SPAN * x
    m = patch_engine(LCGP(y=y, x=x, q=Q, submethod=mode, kernel=kernel))
    m._calib_rows_device = ref.rows_as_host_stub
    o = orc.OracleLCGP(y=y, x=x, q=Q, submethod=mode, kernel=kernel)
    o.phi = m.phi.numpy().copy()
    u = synth.param_points(75, o.get_unconstrained())[1]
    m._set_flat(u)
    o.set_unconstrained(u)
    assert int(m.p) == P and int(m.q) == Q
    return m, o, x, y


def _observation(y, form='dense', seed=3):
    rng = np.random.default_rng(seed)
    sd = y.std(axis=1)
    y_obs = y[:, 5] + 0.1 * sd * rng.standard_normal(P)
    var = (sd * rng.uniform(0.05, 0.15, P)) ** 2
    B = 0.1 * sd[:, None] * rng.standard_normal((P, 2))
    return y_obs, {'scalar': float(var.mean()), 'diag': var, 'dense': np.diag(var) + B @ B.T}[form]


def _theta(n0=9, seed=4):
    return LO + SPAN * np.random.default_rng(seed).uniform(0.05, 0.95, (n0, 2))


def _dense_from_oracle(m, o, theta, y_obs, obs_var, include_noise=True):
    """the p-space log density at the rows of theta: mean and covariance from the ORACLE's predict (on the full path its
    return_fullcov covariance, on the rep path its latent prediction through the output map)"""
    y = np.asarray(y_obs, float)
    obs = ~np.isnan(y)
    ov = np.asarray(obs_var, float)
    S = np.diag(np.full(P, float(ov))) if ov.ndim == 0 else (np.diag(ov) if ov.ndim == 1 else ov)
    S = S[np.ix_(obs, obs)]
    if m.submethod == 'full' and include_noise:
        ypred, _, _, cov = o.predict(theta, return_fullcov=True)
        out = np.zeros(theta.shape[0])
        for i in range(theta.shape[0]):
            sig = cov[i][np.ix_(obs, obs)] + S
            r = (y - ypred[:, i])[obs]
            out[i] = -0.5 * (r @ np.linalg.solve(sig, r) + np.linalg.slogdet(sig)[1] + obs.sum() * ref.LOG2PI)
        return out
    o.predict(theta)
    _, phi_s, t, lam = ref.observation(m, y_obs, obs_var, include_noise)
    return ref.dense_loglik(phi_s, t, lam, o.ghat, o.gvar)[0]


@pytest.mark.parametrize('form', ['scalar', 'diag', 'dense'])
@pytest.mark.parametrize('mode,kernel', [('full', 'matern32'), ('rep', 'matern32'), ('full', 'se')])
def test_loglik_equals_the_dense_density_of_the_oracle(mode, kernel, form):
    m, o, x, y = _pair(mode, kernel)
    y_obs, obs_var = _observation(y, form)
    theta = _theta()
    theta[:2] = x[[1, 6]]                                   # training inputs: the continuous surface, no nugget
    tgt = m.calibration(y_obs, obs_var)
    ll = tgt.loglik(theta)
    assert ll.shape == (9,) and ll.dtype == torch.float64 and ll.device.type == 'cpu'
    want = _dense_from_oracle(m, o, theta, y_obs, obs_var)
    np.testing.assert_allclose(ll.numpy(), want, rtol=1e-9, atol=1e-9)
    ll2, dll = tgt.loglik_grad(theta)
    assert np.array_equal(ll2.numpy(), ll.numpy()) and dll.shape == (9, 2)


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_nan_rows_are_dropped_also_fewer_observed_than_components(mode):
    m, o, x, y = _pair(mode)
    y_obs, obs_var = _observation(y, 'dense')
    theta = _theta()
    for keep in ([0, 1, 3, 4], [1, 3]):                     # |O| = 4, and |O| = 2 < q = 3
        yo = np.full(P, np.nan)
        yo[keep] = y_obs[keep]
        tgt = m.calibration(yo, obs_var)
        assert list(np.flatnonzero(tgt.observed)) == keep
        want = _dense_from_oracle(m, o, theta, yo, obs_var)
        np.testing.assert_allclose(tgt.loglik(theta).numpy(), want, rtol=1e-9, atol=1e-9)
        # entries of obs_var in the rows and columns of unobserved outputs are ignored, whatever they hold
        junk = obs_var.copy()
        drop = [a for a in range(P) if a not in keep]
        junk[drop, :] = np.nan
        junk[:, drop] = -7.0
        assert np.array_equal(m.calibration(yo, junk).loglik(theta).numpy(), tgt.loglik(theta).numpy())


def test_include_noise_false_and_diagonal_fast_path():
    m, o, x, y = _pair('full')
    y_obs, var = _observation(y, 'diag')
    theta = _theta()
    tgt = m.calibration(y_obs, var, include_noise=False)
    want = _dense_from_oracle(m, o, theta, y_obs, var, include_noise=False)
    np.testing.assert_allclose(tgt.loglik(theta).numpy(), want, rtol=1e-9, atol=1e-9)
    assert np.max(np.abs(want - _dense_from_oracle(m, o, theta, y_obs, var))) > 1e-3           # the noise term matters here
    # the diagonal path and the dense path fold to the same M, b, c0, lognorm
    a, b = m.calibration(y_obs, var), m.calibration(y_obs, np.diag(var))
    for u, v in ((a.M, b.M), (a.b, b.b), (a.c0, b.c0), (a.lognorm, b.lognorm)):
        np.testing.assert_allclose(u, v, rtol=1e-12)
    assert np.array_equal(a.M, a.M.T)
    _, phi_s, t, lam = ref.observation(m, y_obs, var)
    for u, v in zip((a.M, a.b, a.c0, a.lognorm), ref.fold(phi_s, t, lam)):
        np.testing.assert_allclose(u, v, rtol=1e-12)


def _central_differences(fn, theta, h):
    out = np.zeros(theta.shape)
    for l in range(theta.shape[1]):
        e = np.zeros_like(theta)
        e[:, l] = h[l]
        out[:, l] = (fn(theta + e) - fn(theta - e)) / (2 * h[l])
    return out


@pytest.mark.parametrize('mode,kernel,form', [('full', 'matern32', 'dense'), ('rep', 'matern32', 'diag'), ('full', 'se', 'scalar'),
                                              ('rep', 'matern32', 'dense')])
def test_loglik_grad_equals_central_differences_of_the_dense_density(mode, kernel, form):
    """the raw-scale chain rule with input ranges that differ per dimension; step 1e-5 of the range, 1e-6 of the largest entry"""
    m, o, x, y = _pair(mode, kernel)
    y_obs, obs_var = _observation(y, form)
    y_obs[2] = np.nan
    theta = _theta(11)
    tgt = m.calibration(y_obs, obs_var)
    ll, dll, s, v = tgt.loglik_grad(theta, latent=True)
    assert dll.shape == (11, 2) and s.shape == v.shape == (Q, 11) and dll.dtype == torch.float64
    fd = _central_differences(lambda th: _dense_from_oracle(m, o, th, y_obs, obs_var), theta, 1e-5 * SPAN)
    assert np.max(np.abs(dll.numpy() - fd)) <= 1e-6 * np.max(np.abs(fd)), (np.max(np.abs(dll.numpy() - fd)), np.max(np.abs(fd)))
    # s, v are the latent sensitivities: the dense gradient with unit Jacobians picks them out
    o.predict(theta)
    _, phi_s, t, lam = ref.observation(m, y_obs, obs_var)
    eye = np.zeros((Q, 11, Q))
    eye[np.arange(Q), :, np.arange(Q)] = 1.0
    want_s = ref.dense_loglik(phi_s, t, lam, o.ghat, o.gvar, eye, 0 * eye)[2]
    want_v = ref.dense_loglik(phi_s, t, lam, o.ghat, o.gvar, 0 * eye, eye)[2]
    np.testing.assert_allclose(s.numpy(), want_s.T, rtol=1e-7, atol=1e-7 * np.max(np.abs(want_s)))
    np.testing.assert_allclose(v.numpy(), want_v.T, rtol=1e-7, atol=1e-7 * np.max(np.abs(want_v)))


def test_loglik_differentiable_gradcheck_and_no_double_backward():
    m, o, x, y = _pair('full')
    y_obs, obs_var = _observation(y, 'dense')
    tgt = m.calibration(y_obs, obs_var)
    theta = _theta(4)
    out = tgt.loglik_differentiable(torch.as_tensor(theta))
    assert not out.requires_grad and torch.equal(out, tgt.loglik(theta))
    tt = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(tgt.loglik_differentiable, (tt,), eps=1e-6, atol=1e-6, rtol=1e-5)
    (g,) = torch.autograd.grad(tgt.loglik_differentiable(tt).sum(), tt)
    assert torch.equal(g, tgt.loglik_grad(theta)[1])
    with pytest.raises(RuntimeError, match='double backward'):
        torch.autograd.grad(tgt.loglik_differentiable(tt).sum(), tt, create_graph=True)


def test_target_goes_stale_when_the_parameters_change():
    m, o, x, y = _pair('full')
    y_obs, obs_var = _observation(y, 'diag')
    tgt = m.calibration(y_obs, obs_var)
    theta = _theta(3)
    tgt.loglik(theta)
    u = m._get_flat().copy()
    u[0] += 0.1
    m._set_flat(u)
    for call in (lambda: tgt.loglik(theta), lambda: tgt.loglik_grad(theta), lambda: tgt.loglik_differentiable(torch.as_tensor(theta))):
        with pytest.raises(RuntimeError, match='stale'):
            call()
    assert np.all(np.isfinite(m.calibration(y_obs, obs_var).loglik(theta).numpy()))


def test_argument_errors():
    m, o, x, y = _pair('full')
    y_obs, dense = _observation(y, 'dense')
    with pytest.raises(ValueError, match='y_obs'):
        m.calibration(y_obs[:4], 1.0)
    with pytest.raises(ValueError, match='y_obs'):
        m.calibration(y_obs[:, None], 1.0)
    with pytest.raises(ValueError, match='no observed'):
        m.calibration(np.full(P, np.nan), 1.0)
    with pytest.raises(ValueError, match='finite'):
        m.calibration(np.where(np.arange(P) == 1, np.inf, y_obs), 1.0)
    with pytest.raises(ValueError, match='obs_var'):
        m.calibration(y_obs, np.ones(P + 1))
    with pytest.raises(ValueError, match='obs_var'):
        m.calibration(y_obs, np.ones((P, P, 1)))
    with pytest.raises(ValueError, match='non-negative'):
        m.calibration(y_obs, -1.0)
    with pytest.raises(ValueError, match='non-negative'):
        m.calibration(y_obs, np.where(np.arange(P) == 2, -1e-3, 1.0))
    with pytest.raises(ValueError, match='non-negative'):
        m.calibration(y_obs, dense - 2 * np.diag(np.diag(dense)))
    skew = dense.copy()
    skew[0, 1] += 1e-3
    with pytest.raises(ValueError, match='symmetric'):
        m.calibration(y_obs, skew)
    with pytest.raises(np.linalg.LinAlgError):
        m.calibration(y_obs, 0.0, include_noise=False)
    indef = np.full((P, P), 1.0) + np.diag([0.0, 0, 0, 0, -0.5])
    with pytest.raises(np.linalg.LinAlgError):
        m.calibration(y_obs, indef, include_noise=False)
    tgt = m.calibration(y_obs, dense)
    with pytest.raises(ValueError, match='theta'):
        tgt.loglik(np.zeros((3, 5)))


def test_c_abi_argument_checks_of_the_row_entry():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() == 610
    assert hasattr(lib, 'lcgp_calib_rows') and 'lcgp_calib_rows' in _hip.SIGNATURES
    p = C.c_void_p(16)              # never dereferenced: every call below is refused before it enqueues anything

    def call(q=3, d=2, n0=10, ghat=p, gvar=p, dghat=p, dgvar=p, stride=0, M=p, b=p, ll=p, dll=p, sens=p):
        return lib.lcgp_calib_rows(None, q, d, n0, ghat, gvar, dghat, dgvar, stride, M, b, 0.0, 0.0, None, ll, dll, sens)

    for kw, word in (({'q': 0}, b'q must'), ({'q': 65}, b'q must'), ({'d': 0}, b'd must'), ({'d': 127}, b'd must'),
                     ({'n0': 0}, b'n0'), ({'ghat': None}, b'NULL'), ({'gvar': None}, b'NULL'), ({'M': None}, b'NULL'),
                     ({'b': None}, b'NULL'), ({'ll': None}, b'NULL'), ({'dghat': None}, b'both'), ({'dgvar': None}, b'both'),
                     ({'dghat': None, 'dgvar': None}, b'dll needs'), ({'stride': 9}, b'in_stride'), ({'stride': -1}, b'in_stride')):
        assert call(**kw) < 0, kw
        assert word in lib.lcgp_last_error(), (kw, lib.lcgp_last_error())


def test_precondition_of_the_gpu_comparison_every_covariance_is_well_conditioned():
    """tests/test_gpu_calibration.py bounds the error of the dense density by 64 p eps cond(Sigma_i) (...): asserted here, for its
    inputs, cond(Sigma_i) <= 1e6 at EVERY input (gvar between zero and the prior variance brackets Sigma_i)"""
    for name in ref.MODEL_CASES:
        m, x, y = ref.model_case(name)
        for form in ('scalar', 'diag', 'dense'):
            theta, y_obs, obs_var = ref.case_observation(name, x, y, form)
            assert ref.cond_bound(m, y_obs, obs_var) <= 1e6, (name, form, ref.cond_bound(m, y_obs, obs_var))
