"""CPU tests of the Sobol queries on a conditioned view (ConditionedLCGP.sobol_indices / integrated_variance):
the restatement of the view's covariance correction Q' (tests/condition_sobol_ref.py) against a dense inverse of the augmented
matrix and against quadrature of the view's own continuous posterior covariance, the host layer through a numpy stand-in of
the engine methods, two gloo ranks against one, and the argument checks of the new C entries (tests/test_gpu_condition_sobol.py
runs the same through liblcgp_hip.so on the GPU).

Bar of the restatement: 1e-10 of the prior term c prod_{l not in u} I2_l (IV: c; the variance of the box mean: c prod I2),
unless the dense route's own two ways to the inverse of the augmented matrix disagree by more than 1e-11 of it -- then ten times
that disagreement (the rule of tests/test_gpu_sobol_uncertainty.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla

from tests import condition_marginal_ref as cmref
from tests import condition_sobol_ref as cref
from tests import marginal_ref as mref
from tests import sobol_ref as ref
from tests import sobol_uncertainty_ref as uref
from tests.test_condition_host import _free_port, closed_form_begin, make_model, new_columns, patch_cond
from tests.test_predict_hess_host import _cross
from tests.test_sobol_uncertainty_host import _component

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = ('matern32', 'se', 'matern52')
END_TO_END_BAR = 1e-10
HOST_AGREES_WITHIN = 1e-11
PLUG = ('first', 'total', 'variance', 'mean', 'first_variance', 'closed_variance')
NEW = ('expected_variance', 'expected_first_variance', 'expected_closed_variance', 'first_expected', 'total_expected',
       'integrated_variance')


def view_model(mode, kernel='matern32', d=2, **kw):
    """tests.test_condition_host.make_model on the stand-in that answers the view's Sobol queries"""
    m, x, y, xn, yn = make_model(mode, kernel, d, **kw)
    return patch_cond(m, cref.ViewSobolOracleEngine), x, y, xn, yn


def _new_runs(mode, d, mnew, p=3, seed=29):
    """mnew new unique inputs on the raw scale of make_model; on the rep path with 1 to 3 replicates each, shuffled"""
    rng = np.random.default_rng(seed + d + mnew)
    xu = -1.5 + 4.0 * rng.uniform(0, 1, (mnew, d))
    if mode == 'rep':
        rows = np.repeat(np.arange(mnew), 1 + np.arange(mnew) % 3)
        xu = xu[rows[rng.permutation(len(rows))]]
    return xu, rng.standard_normal((p, len(xu))) + 0.3


@pytest.mark.parametrize('mnew', [1, 5])
@pytest.mark.parametrize('d', [1, 3])
@pytest.mark.parametrize('mode', ['full', 'rep'])
@pytest.mark.parametrize('kernel', KERNELS)
def test_q_prime_is_the_inverse_of_the_augmented_matrix(kernel, mode, d, mnew):
    """C_u, IV and the variance of the box mean from Q' = c^2 ([[D sr sr^T o A^-1, 0], [0, 0]] + P P^T), built from A^-1, U_n and
    L_S, against sobol_uncertainty_ref.component fed with a dense inverse of the augmented matrix; and the weights of the
    view's mean surface over the n + m centres, c sr z' and c w, against c sa z of that route"""
    m, x, y, _, _ = view_model(mode, kernel, d)
    xn, yn = _new_runs(mode, d, mnew)
    view = m.condition(xn, yn)
    assert view.m == mnew
    eng = m._aux_engine
    sr = np.ones(eng.n) if eng.sr is None else eng.sr
    xn_s, snew, ycol = new_columns(m, xn, yn)
    box = np.stack([np.full(d, 0.1), np.full(d, 0.9)])
    worst = 0.0
    for k, (th, low, z, b) in enumerate(eng._state):
        Un, LS, v = view._state['state'][k]
        xa, sa, _, za = cmref.augmented(th, eng.x, sr, eng.Y, kernel, xn_s, snew, ycol)
        got = cref.component(kernel, xa, th, cref.view_q_prime(th, low, eng.x, sr, Un, LS), box)
        by_solve, by_inverse, _ = uref.dense_ainv(kernel, xa, sa, th)
        a, bb = (uref.component(kernel, xa, sa, th, inv, box) for inv in (by_solve, by_inverse))
        _, p0 = uref.prior_products(kernel, th[:d], box)
        host = max(np.max(np.abs(a['C'] - bb['C']) / a['prior']), abs(a['IV'] - bb['IV']) / a['c'])
        bar = END_TO_END_BAR if host <= HOST_AGREES_WITHIN else 10.0 * host
        ratio = max(np.max(np.abs(got['C'] - a['C']) / a['prior']), abs(got['IV'] - a['IV']) / a['c'],
                    abs(got['overall_var'] - a['overall_var']) / (a['c'] * p0))
        worst = max(worst, ratio)
        assert np.all(np.abs(got['C'] - a['C']) <= bar * a['prior']), (k, np.abs(got['C'] - a['C']) / a['prior'])
        assert abs(got['IV'] - a['IV']) <= bar * a['c']
        assert abs(got['overall_var'] - a['overall_var']) <= bar * a['c'] * p0
        zp, w = cref.mean_vectors(low, z, Un, LS, v, th[d + 2])
        want = sa * za
        assert np.max(np.abs(np.r_[sr * zp, w] - want)) <= END_TO_END_BAR * np.max(np.abs(want))
    print('restatement', kernel, mode, d, mnew, 'worst ratio', worst)


def test_q_prime_against_quadrature_of_the_views_continuous_covariance():
    """IV and C_all at d = 2, n = 12, m = 3 against the view's continuous posterior covariance,
        cov'(t, t') = cov(t, t') - T(t) . T(t'),    T = (c^x(t, xn) - D U_0 U_n^T) L_S^-T
    (marginal_ref.continuous_cov for the fitted part), on the piecewise tensor Gauss-Legendre rule that breaks at the
    coordinates of the training AND the new inputs; the prior part of wt^T cov wt is replaced by its closed form as in
    tests/test_sobol_uncertainty_host.py.  Bar 4e-12 (c + size), as there"""
    kernel = 'matern52'
    x, sr, th, box, ainv, low = _component(kernel, 'rep')
    d = 2
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    xn = np.array([[0.22, 0.31], [0.71, 0.12], [0.95, 0.66]])                 # the last one outside the box
    r = np.array([1.0, 3.0, 2.0])
    Un, LS, _ = closed_form_begin(th, low, np.zeros(len(x)), x, sr, kernel, xn, np.zeros(3), r)
    got = cref.component(kernel, np.vstack([x, xn]), th, cref.view_q_prime(th, low, x, sr, Un, LS), box)
    rules = [ref.piecewise_gauss_legendre(8, box[0][l], box[1][l], np.r_[x[:, l], xn[:, l]]) for l in range(d)]
    g0, g1 = np.meshgrid(rules[0][0], rules[1][0], indexing='ij')
    pts = np.stack([g0.reshape(-1), g1.reshape(-1)], axis=1)
    wt = (rules[0][1][:, None] * rules[1][1][None, :]).reshape(-1)
    cov, X0 = mref.continuous_cov(pts, x, sr, th, low, kernel)
    U0 = sla.solve_triangular(low, X0.T, lower=True).T
    T = sla.solve_triangular(LS, (_cross(pts, xn, ell, scale, nug, kernel) - D * U0 @ Un.T).T, lower=True).T
    cov = cov - T @ T.T
    iv = wt @ np.diag(cov)
    prior_rule = got['c'] * np.prod([rr[1] @ mref.kappa(kernel, np.abs(rr[0][:, None] - rr[0][None, :]) / th[l]) @ rr[1]
                                    for l, rr in enumerate(rules)])
    _, p0 = uref.prior_products(kernel, th[:d], box)
    c_all = iv - (wt @ cov @ wt - prior_rule + got['c'] * p0)
    bar = 4e-12 * (got['c'] + got['size'][2 * d])
    print('quadrature on the view', 'IV', got['IV'], abs(got['IV'] - iv) / bar * 4e-12, 'C_all', got['C'][2 * d],
          abs(got['C'][2 * d] - c_all) / bar * 4e-12)
    assert abs(got['IV'] - iv) <= bar, (got['IV'], iv)
    assert abs(got['C'][2 * d] - c_all) <= bar, (got['C'][2 * d], c_all)
    base = uref.component(kernel, x, sr, th, ainv, box)
    assert 0.0 < got['IV'] < base['IV'] < got['c']


# ---- the host layer ----------------------------------------------------------------------------------------------------------
def _direct(m, view, bs):
    """(C (q, 2 d + 1), IV (q), overall_var (q)) of the view from the stand-in's own state"""
    eng = m._aux_engine
    sr = np.ones(eng.n) if eng.sr is None else eng.sr
    xa = np.vstack([eng.x, view._state['xn']])
    res = [cref.component(m.kernel, xa, s[0], cref.view_q_prime(s[0], s[1], eng.x, sr, *view._state['state'][k][:2]), bs)
           for k, s in enumerate(eng._state)]
    return np.stack([r['C'] for r in res]), np.array([r['IV'] for r in res]), np.array([r['overall_var'] for r in res])


@pytest.mark.parametrize('mode,kernel', [(mode, kernel) for mode in ('full', 'rep') for kernel in KERNELS])
def test_view_queries_assemble_the_engine_sums(mode, kernel):
    m, x, y, xn, yn = view_model(mode, kernel)
    view = m.condition(xn, yn)
    p, d, q = 3, 2, 2
    s0 = view.sobol_indices()
    s = view.sobol_indices(uncertainty=True)
    for name in PLUG:                                           # the plug-in fields do not move
        np.testing.assert_array_equal(getattr(s, name).numpy(), getattr(s0, name).numpy(), err_msg=name)
    for name in NEW:
        assert getattr(s0, name) is None, name
        assert getattr(s, name).dtype.is_floating_point
    assert s.first.shape == (p, d) and s.total.shape == (p, d) and s.variance.shape == (p,) and s.mean.shape == (p,)
    assert s.expected_variance.shape == (p,) and s.integrated_variance.shape == (p,)
    for name in ('first_variance', 'closed_variance', 'expected_first_variance', 'expected_closed_variance', 'first_expected',
                 'total_expected'):
        assert getattr(s, name).shape == (p, d), name
    bs = m._marginal_box(None)
    Cq, ivq, ovq = _direct(m, view, bs)
    W, _, scale, _ = m._output_map()
    corr = ((W ** 2).T @ Cq) * (scale ** 2)[:, None]
    V = np.concatenate([s.first_variance.numpy(), s.closed_variance.numpy(), s.variance.numpy()[:, None]], axis=1)
    E = np.concatenate([s.expected_first_variance.numpy(), s.expected_closed_variance.numpy(),
                        s.expected_variance.numpy()[:, None]], axis=1)
    np.testing.assert_allclose(E, V + corr, rtol=1e-12, atol=0)
    np.testing.assert_allclose(s.integrated_variance.numpy(), ((W ** 2).T @ ivq) * scale ** 2, rtol=1e-12)
    np.testing.assert_allclose(s.first_expected.numpy(), E[:, :d] / E[:, 2 * d:], rtol=1e-13)
    np.testing.assert_allclose(s.total_expected.numpy(), 1.0 - E[:, d:2 * d] / E[:, 2 * d:], rtol=1e-12, atol=1e-14)
    # the plug-in part is that of the view's own mean surface: its box mean and the variance of its box mean
    me = view.main_effects(grid=2)
    np.testing.assert_allclose(s.mean.numpy(), me.overall.numpy(), rtol=0, atol=1e-10 * np.max(np.abs(me.overall.numpy())))
    ov = me.overall_var.numpy()
    ev = s.expected_variance.numpy()
    np.testing.assert_allclose(s.integrated_variance.numpy() - (ev - s.variance.numpy()), ov, rtol=0, atol=1e-10 * np.max(ov))
    np.testing.assert_allclose(((W ** 2).T @ ovq) * scale ** 2, ov, rtol=0, atol=1e-10 * np.max(ov))
    # integrated_variance() is the same pass alone; outputs= and latent=
    np.testing.assert_array_equal(view.integrated_variance().numpy(), s.integrated_variance.numpy())
    np.testing.assert_array_equal(view.integrated_variance(outputs=[2, 0]).numpy(), s.integrated_variance.numpy()[[2, 0]])
    sel = view.sobol_indices(outputs=[2, 0], uncertainty=True)
    for name in PLUG + NEW:
        np.testing.assert_array_equal(getattr(sel, name).numpy(), getattr(s, name).numpy()[[2, 0]], err_msg=name)
    lat = view.sobol_indices(latent=True, uncertainty=True)
    assert lat.first.shape == (q, d)
    np.testing.assert_allclose(lat.expected_variance.numpy() - lat.variance.numpy(), Cq[:, 2 * d], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(lat.integrated_variance.numpy(), ivq, rtol=1e-12)
    np.testing.assert_array_equal(view.integrated_variance(latent=True).numpy(), lat.integrated_variance.numpy())
    assert view.integrated_variance(latent=True, outputs=1).shape == (1,)
    # conditioning cannot add uncertainty: IV, every C_u and the variance of the box mean against the base model's, per component
    Cb, ivb, ovb = m._sobol_matrix(bs)
    Cv, ivv, ovv = view._sobol_matrix(bs, *view._float64_state())
    c = m.lLmb0.numpy() * (1.0 - m.lnugGPs.numpy() / (1.0 + m.lnugGPs.numpy()))
    tol = 1e-12 * c
    assert np.all(ivv <= ivb + tol) and np.all(ovv <= ovb + tol)
    assert np.all(Cv <= Cb + tol[:, None]) and np.all(Cv >= -tol[:, None])
    assert np.all(ivv < ivb)                                    # and the new runs did settle something
    # a sub-box changes the answer, and the base model's own results are what they were
    xr = np.asarray(x)
    lo, hi = xr.min(axis=0), xr.max(axis=0)
    sub = np.stack([lo + 0.3 * (hi - lo), lo + 0.6 * (hi - lo)])
    got = view.integrated_variance(box=sub, latent=True).numpy()
    np.testing.assert_allclose(got, _direct(m, view, m._marginal_box(sub))[1], rtol=1e-12)
    assert not np.allclose(got, ivq, rtol=1e-3)
    np.testing.assert_array_equal(m._sobol_matrix(bs)[1], ivb)


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_view_equals_a_model_on_the_augmented_data(mode):
    """every latent field against sobol_ref / sobol_uncertainty_ref on the augmented training set at the same theta rows"""
    kernel = 'se'
    m, x, y, xn, yn = view_model(mode, kernel)
    view = m.condition(xn, yn)
    eng = m._aux_engine
    sr = np.ones(eng.n) if eng.sr is None else eng.sr
    xn_s, snew, ycol = new_columns(m, xn, yn)
    bs = m._marginal_box(None)
    d = 2
    lat = view.sobol_indices(latent=True, uncertainty=True)
    for k, (th, low, z, b) in enumerate(eng._state):
        xa, sa, _, za = cmref.augmented(th, eng.x, sr, eng.Y, kernel, xn_s, snew, ycol)
        c = th[d] * (1.0 - th[d + 1] / (1.0 + th[d + 1]))
        w = c * sa * za
        Dk, means, size = ref.pair_sums(kernel, xa, w, th[:d], w, th[:d], bs)
        a = uref.component(kernel, xa, sa, th, uref.dense_ainv(kernel, xa, sa, th)[0], bs)
        assert abs(lat.mean.numpy()[k] - means[0]) <= 1e-10 * np.sum(np.abs(w))
        got = np.r_[lat.first_variance.numpy()[k], lat.closed_variance.numpy()[k], lat.variance.numpy()[k]]
        assert np.all(np.abs(got - Dk) <= END_TO_END_BAR * size), np.abs(got - Dk) / size
        gotE = np.r_[lat.expected_first_variance.numpy()[k], lat.expected_closed_variance.numpy()[k], lat.expected_variance.numpy()[k]]
        assert np.all(np.abs(gotE - got - a['C']) <= END_TO_END_BAR * a['prior'])
        assert abs(lat.integrated_variance.numpy()[k] - a['IV']) <= END_TO_END_BAR * a['c']


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_a_single_input_explains_everything(mode):
    m, x, y, xn, yn = view_model(mode, 'matern32', d=1)
    s = m.condition(xn, yn).sobol_indices(uncertainty=True)
    for name in ('first', 'total', 'first_expected', 'total_expected'):
        np.testing.assert_allclose(getattr(s, name).numpy(), 1.0, rtol=0, atol=1e-12, err_msg=name)


def test_stale_view_and_bad_arguments():
    m, x, y, xn, yn = view_model('full')
    view = m.condition(xn, yn)
    xr = np.asarray(x)
    lo, hi = xr.min(axis=0), xr.max(axis=0)
    for call in (view.integrated_variance, view.sobol_indices):
        with pytest.raises(ValueError, match='upper > lower'):
            call(box=np.stack([hi, lo]))
        with pytest.raises(ValueError, match='outputs'):
            call(outputs=[3])
        with pytest.raises(ValueError, match='outputs'):
            call(outputs=[2], latent=True)
    with pytest.raises(ValueError, match='outputs'):
        m.sobol_indices(outputs=[2], latent=True, uncertainty=True)          # (what the model raises)
    view.integrated_variance()
    m._set_flat(m._get_flat() + 0.01)
    with pytest.raises(RuntimeError, match='stale'):
        view.integrated_variance()
    with pytest.raises(RuntimeError, match='stale'):
        view.sobol_indices(uncertainty=True)
    m.predict(x[:3] + 0.01)
    with pytest.raises(RuntimeError, match='stale'):
        view.sobol_indices()


def test_a_float32_view_builds_its_float64_state_once():
    """a float32 model: the view's own state is the float32 engine's; the Sobol queries build a companion state on the float64
    engine from the stored standardised outputs and counts, once, and agree with the float64 model's view (the stand-in computes
    in float64 either way)"""
    m32, x, y, xn, yn = view_model('rep', 'matern52', dtype='float32')
    m64, _, _, _, _ = view_model('rep', 'matern52')
    v32, v64 = m32.condition(xn, yn), m64.condition(xn, yn)
    assert not v32._float64 and v64._float64 and v32._companion is None
    a, b = v32.sobol_indices(uncertainty=True), v64.sobol_indices(uncertainty=True)
    comp = v32._companion
    assert comp is not None and v64._companion is None
    for name in PLUG + NEW:
        np.testing.assert_allclose(getattr(a, name).numpy(), getattr(b, name).numpy(), rtol=1e-9, atol=1e-12, err_msg=name)
    np.testing.assert_array_equal(v32.integrated_variance().numpy(), a.integrated_variance.numpy())
    assert v32._companion is comp
    v32.predict(x[:3] + 0.01)                                   # the view's other queries keep working
    # a view built without the outputs of its runs says so
    from lcgp_amd.lcgp import ConditionedLCGP
    bare = ConditionedLCGP(m32, v32.x_new, v32._engine, v32._state)
    with pytest.raises(RuntimeError, match='outputs of its new runs'):
        bare.integrated_variance()


def test_two_ranks_equal_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_condition_sobol_host_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


def test_c_abi_of_the_new_entries():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() == 610
    for name in ('lcgp_condition_sobol_matrix_pairs', 'lcgp_condition_sobol_scratch_bytes', 'lcgp_condition_grad_fetch'):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    nb = C.c_size_t(0)

    def a256(v):
        return (v + 255) // 256 * 256
    # n = 1000, m = 70: N = 1070 -> 17 x 17 tiles (Npad = 1088), npad = 1024, mpad = 128
    assert lib.lcgp_condition_sobol_scratch_bytes(1000, 3, 4, 70, 4, C.byref(nb)) == 0
    want = (a256(8 * 4 * 3 * 1070) + a256(8 * 4) + a256(8 * 17 * 17 * 8) + 256 + 2 * a256(8 * 128 * 1024) + a256(8 * 1088 * 128)
            + a256(8 * 1088 * 1088))
    assert nb.value == want, (nb.value, want)
    assert lib.lcgp_condition_sobol_scratch_bytes(1000, 127, 4, 70, 4, C.byref(nb)) < 0 and b'd must be' in lib.lcgp_last_error()
    assert lib.lcgp_condition_sobol_scratch_bytes(0, 3, 4, 70, 4, C.byref(nb)) < 0 and b'n < 1' in lib.lcgp_last_error()
    assert lib.lcgp_condition_sobol_scratch_bytes(1000, 3, 4, 0, 4, C.byref(nb)) < 0 and b'm < 1' in lib.lcgp_last_error()
    assert lib.lcgp_condition_sobol_scratch_bytes(1000, 3, 4, 70, 0, C.byref(nb)) < 0 and b'nks' in lib.lcgp_last_error()
    assert lib.lcgp_condition_sobol_scratch_bytes(1000, 3, 4, 70, 4, None) < 0 and b'NULL' in lib.lcgp_last_error()
    # the scratch of the model's entries is what it was
    assert lib.lcgp_sobol_matrix_scratch_bytes(1000, 3, 4, 4, C.byref(nb)) == 0 and nb.value == 8 * (4 * 3 * 1000 + 4 + 4 * 256 * 8)
    assert lib.lcgp_sobol_scratch_bytes(1000, 3, 4, 10, C.byref(nb)) == 0 and nb.value == 8 * (4 * 3 * 1000 + 4 + 10 * 256 * 7)
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything
    good = (C.c_int * 2)(0, 1)

    def call(dtype=_hip.F64, kern=0, n=100, d=2, p=3, q=2, theta=dummy, ws=dummy, state=dummy, m=5, xa=dummy, v=dummy, ell=dummy,
             box=dummy, ks=good, nks=2, scratch=dummy, nbytes=1 << 40, out=dummy):
        return lib.lcgp_condition_sobol_matrix_pairs(None, dtype, kern, n, d, p, q, theta, ws, state, m, xa, v, ell, box, ks, nks,
                                                     scratch, nbytes, out)

    assert call(dtype=_hip.F32) < 0 and b'float64' in lib.lcgp_last_error()
    assert call(kern=7) < 0 and b'kernel_id' in lib.lcgp_last_error()
    assert call(d=0) < 0 and b'd must be' in lib.lcgp_last_error()
    assert call(d=127) < 0 and b'd must be' in lib.lcgp_last_error()
    assert call(n=0) < 0 and b'n < 1' in lib.lcgp_last_error()
    assert call(q=0) < 0 and b'q_local' in lib.lcgp_last_error()
    assert call(m=0) < 0 and b'm < 1' in lib.lcgp_last_error()
    assert call(nks=0) < 0 and b'nks' in lib.lcgp_last_error()
    for arg in ('theta', 'ws', 'state', 'xa', 'v', 'ell', 'box', 'ks', 'scratch', 'out'):
        assert call(**{arg: None}) < 0 and b'NULL' in lib.lcgp_last_error(), arg
    assert call(ks=(C.c_int * 2)(0, 2)) < 0 and b'ks must' in lib.lcgp_last_error()
    assert call(ks=(C.c_int * 2)(-1, 1)) < 0 and b'ks must' in lib.lcgp_last_error()
    assert call(nbytes=1000) < 0 and b'scratch too small' in lib.lcgp_last_error()

    def fetch(n=100, q=2, m=5, gs=dummy, w=dummy, z=dummy):
        return lib.lcgp_condition_grad_fetch(None, n, q, m, gs, w, z)

    assert fetch(n=0) < 0 and fetch(q=0) < 0
    assert fetch(m=0) < 0 and b'm < 1' in lib.lcgp_last_error()
    for arg in ('gs', 'w', 'z'):
        assert fetch(**{arg: None}) < 0 and b'NULL' in lib.lcgp_last_error(), arg
