"""CPU tests of the expected Sobol variances and the exact integrated variance (LCGP.sobol_indices(uncertainty=True),
LCGP.integrated_variance): the restatement of tests/sobol_uncertainty_ref.py against quadrature of the
posterior covariance of the continuous surface (marginal_ref.continuous_cov), the signs and the order of the corrections, the
variance of the box mean against the box-averaged prediction, the host layer through a numpy stand-in of
HotPathEngine.sobol_matrix_sums, and the C entries of the library (tests/test_gpu_sobol_uncertainty.py runs the same through
liblcgp_hip.so on the GPU).  The pair integral and the other device functions are those of lcgp_sobol_pairs: their CPU tests are
in tests/test_sobol_host.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla

from tests import marginal_ref as mref
from tests import sobol_ref as ref
from tests import sobol_uncertainty_ref as uref
from tests.test_sobol_host import SobolOracleEngine, model_of as sobol_model_of

KERNELS = ('matern32', 'se', 'matern52')
PLUG = ('first', 'total', 'variance', 'mean', 'first_variance', 'closed_variance')
NEW = ('expected_variance', 'expected_first_variance', 'expected_closed_variance', 'first_expected', 'total_expected',
       'integrated_variance')


def _component(kernel, sr_kind, n=12, d=2, seed=5):
    """one component at n = 12, d = 2: inputs in the unit square, a box that leaves some of them outside, unit or replicate
    weights sr; returns (x, sr, th, box, ainv, low)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (n, d))
    sr = np.ones(n) if sr_kind == 'full' else np.sqrt(rng.integers(1, 4, n).astype(float))
    th = np.array([0.35, 0.8, 1.7, 0.02, 40.0])               # ell (2), scale, nug, D
    box = np.array([[0.1, 0.0], [0.9, 0.8]])
    ainv, _, low = uref.dense_ainv(kernel, x, sr, th)
    return x, sr, th, box, ainv, low


@pytest.mark.parametrize('sr_kind', ['full', 'rep'])
@pytest.mark.parametrize('kernel', KERNELS)
def test_restatement_against_quadrature_of_the_continuous_covariance(kernel, sr_kind):
    """IV and C_all at d = 2, n = 12 against continuous_cov on the piecewise tensor Gauss-Legendre rule that breaks at the
    training coordinates (8 nodes per piece: between breaks the integrands are analytic).
        IV    = sum_a wt_a cov[a, a]
        C_all = IV - wt^T cov wt
    The prior part of wt^T cov wt, c prod_l (w_l^T kappa_l w_l), has a kink along t = t' INSIDE every piece, which no tensor
    rule resolves; it is a product of 1-D sums, so it is taken out of the rule's value and its closed form c prod_l I2_l
    (tests/test_marginal_host.py checks it) put in its place.
    Bar 4e-12 (c + size): the pair integral is within 1e-12 relative of quadrature (tests/test_sobol_host.py), a subset
    product holds d = 2 of them, and the rule's own sum of as many terms rounds as much again; size = sum |Q| (M_u + M_0)."""
    x, sr, th, box, ainv, low = _component(kernel, sr_kind)
    got = uref.component(kernel, x, sr, th, ainv, box)
    d = 2
    rules = [ref.piecewise_gauss_legendre(8, box[0][l], box[1][l], x[:, l]) for l in range(d)]
    g0, g1 = np.meshgrid(rules[0][0], rules[1][0], indexing='ij')
    pts = np.stack([g0.reshape(-1), g1.reshape(-1)], axis=1)
    wt = (rules[0][1][:, None] * rules[1][1][None, :]).reshape(-1)
    cov, _ = mref.continuous_cov(pts, x, sr, th, low, kernel)
    iv = wt @ np.diag(cov)
    prior_rule = got['c'] * np.prod([r[1] @ mref.kappa(kernel, np.abs(r[0][:, None] - r[0][None, :]) / th[l]) @ r[1]
                                    for l, r in enumerate(rules)])
    _, p0 = uref.prior_products(kernel, th[:d], box)
    c_all = iv - (wt @ cov @ wt - prior_rule + got['c'] * p0)
    bar = 4e-12 * (got['c'] + got['size'][2 * d])
    print('quadrature', kernel, sr_kind, 'IV', got['IV'], abs(got['IV'] - iv) / bar * 4e-12, 'C_all', got['C'][2 * d],
          abs(got['C'][2 * d] - c_all) / bar * 4e-12)
    assert abs(got['IV'] - iv) <= bar, (got['IV'], iv)
    assert abs(got['C'][2 * d] - c_all) <= bar, (got['C'][2 * d], c_all)
    assert 0.0 < got['IV'] < got['c']


@pytest.mark.parametrize('sr_kind', ['full', 'rep'])
@pytest.mark.parametrize('kernel', KERNELS)
def test_corrections_are_nonnegative_and_ordered(kernel, sr_kind):
    """C_u is the expectation of a variance: C_u >= -1e-12 c; a subset explains no more than all inputs: C_{l} <= C_all and
    C_{~l} <= C_all"""
    for seed in (5, 6, 7):
        x, sr, th, box, ainv, low = _component(kernel, sr_kind, seed=seed)
        got = uref.component(kernel, x, sr, th, ainv, box)
        c, Cu = got['c'], got['C']
        assert np.all(Cu >= -1e-12 * c), Cu
        assert np.all(Cu[:4] <= Cu[4] + 1e-12 * c), Cu


@pytest.mark.parametrize('sr_kind', ['full', 'rep'])
@pytest.mark.parametrize('kernel', KERNELS)
def test_variance_of_the_box_mean_is_the_all_integrated_marginal_row(kernel, sr_kind):
    """c prod I2 - S0 against latent_marginal's variance of the row that integrates every input (a triangular solve, no
    A^-1): within 1e-12 of what either adds up, c prod I2 + sum |Q| M_0"""
    x, sr, th, box, ainv, low = _component(kernel, sr_kind)
    got = uref.component(kernel, x, sr, th, ainv, box)
    _, gvar = mref.latent_marginal(np.zeros((1, 2)), np.ones((1, 2), bool), box, x, sr, th, low, np.zeros(len(x)), kernel)
    size0 = got['size0']
    assert abs(got['overall_var'] - gvar[0]) <= 1e-12 * (got['c'] + size0), (got['overall_var'], gvar[0])
    # and IV - C_all is the same number: the total variance splits into the variance of the mean and the rest
    assert abs((got['IV'] - got['C'][4]) - got['overall_var']) <= 1e-12 * (got['c'] + size0)


# ---- the host layer ----------------------------------------------------------------------------------------------------------
class UncertaintyOracleEngine(SobolOracleEngine):
    """SobolOracleEngine plus sobol_matrix_sums, in numpy float64 from tests/sobol_uncertainty_ref.py"""

    def sobol_matrix_sums(self, x, v, ell, box, ks):
        x, v, ell, box = (np.asarray(a, np.float64) for a in (x, v, ell, box))
        n, d = x.shape
        assert v.shape == (len(self._state), n) and ell.shape == (len(self._state), d) and box.shape == (2, d)
        sums, s0 = np.zeros((len(ks), 2 * d + 1)), np.zeros(len(ks))
        for r, k in enumerate(np.asarray(ks)):
            th, low = self._state[k][0], self._state[k][1]
            np.testing.assert_array_equal(ell[k], th[:d])
            ainv = sla.cho_solve((low, True), np.eye(n))
            sums[r], s0[r], _, _ = uref.matrix_sums(self.kernel, x, ell[k], box, v[k][:, None] * v[k][None, :] * ainv)
        return sums, s0


def model_of(mode, kernel='matern32'):
    m, x = sobol_model_of(mode, kernel)
    make = m._make_engine

    def _make(dtype=None):
        e = make(dtype)
        if e is not None:
            e.__class__ = UncertaintyOracleEngine
        return e
    m._make_engine = _make
    m._engine = None
    m._invalidate()
    return m, x


def _direct(m, box=None):
    """(C (q, 2 d + 1), IV (q), overall_var (q)) from the stand-in's own state, through uref.component"""
    eng = m._ensure_aux()
    d = eng.d
    sr = np.ones(eng.n) if eng.sr is None else eng.sr
    bs = np.stack([np.zeros(d), np.ones(d)]) if box is None else m._marginal_box(box)
    res = [uref.component(m.kernel, eng.x, sr, s[0], sla.cho_solve((s[1], True), np.eye(eng.n)), bs) for s in eng._state]
    return np.stack([r['C'] for r in res]), np.array([r['IV'] for r in res]), np.array([r['overall_var'] for r in res])


@pytest.mark.parametrize('mode,kernel', [(mode, kernel) for mode in ('full', 'rep') for kernel in KERNELS])
def test_sobol_indices_with_uncertainty_assemble_the_matrix_sums(mode, kernel):
    m, x = model_of(mode, kernel)
    s0 = m.sobol_indices()
    s = m.sobol_indices(uncertainty=True)
    for name in PLUG:                                           # the plug-in fields do not move
        np.testing.assert_array_equal(getattr(s, name).numpy(), getattr(s0, name).numpy(), err_msg=name)
    for name in NEW:
        assert getattr(s0, name) is None, name
        assert getattr(s, name).dtype.is_floating_point
    assert s.expected_variance.shape == (3,) and s.integrated_variance.shape == (3,)
    for name in ('expected_first_variance', 'expected_closed_variance', 'first_expected', 'total_expected'):
        assert getattr(s, name).shape == (3, 2), name
    Cq, ivq, ovq = _direct(m)
    W, _, scale, _ = m._output_map()
    corr = ((W ** 2).T @ Cq) * (scale ** 2)[:, None]
    V = np.concatenate([s.first_variance.numpy(), s.closed_variance.numpy(), s.variance.numpy()[:, None]], axis=1)
    E = np.concatenate([s.expected_first_variance.numpy(), s.expected_closed_variance.numpy(),
                        s.expected_variance.numpy()[:, None]], axis=1)
    np.testing.assert_allclose(E, V + corr, rtol=1e-13, atol=0)
    np.testing.assert_allclose(s.integrated_variance.numpy(), ((W ** 2).T @ ivq) * scale ** 2, rtol=1e-13)
    np.testing.assert_allclose(s.first_expected.numpy(), E[:, :2] / E[:, 4:], rtol=1e-13)
    np.testing.assert_allclose(s.total_expected.numpy(), 1.0 - E[:, 2:4] / E[:, 4:], rtol=1e-12, atol=1e-14)
    ev = s.expected_variance.numpy()
    assert np.all(E >= V - 1e-12 * s.variance.numpy()[:, None])
    fe, te = s.first_expected.numpy(), s.total_expected.numpy()
    assert np.all(fe >= -1e-10) and np.all(fe <= te + 1e-10) and np.all(te <= 1.0 + 1e-10)
    # IV - (E[V] - V) is the variance of the box mean, main_effects().overall_var
    ov = m.main_effects(grid=2).overall_var.numpy()
    np.testing.assert_allclose(s.integrated_variance.numpy() - (ev - s.variance.numpy()), ov, rtol=0, atol=1e-10 * np.max(ov))
    np.testing.assert_allclose(((W ** 2).T @ ovq) * scale ** 2, ov, rtol=0, atol=1e-10 * np.max(ov))
    # integrated_variance() is the same pass alone
    np.testing.assert_array_equal(m.integrated_variance().numpy(), s.integrated_variance.numpy())
    np.testing.assert_array_equal(m.integrated_variance(outputs=[2, 0]).numpy(), s.integrated_variance.numpy()[[2, 0]])
    sel = m.sobol_indices(outputs=[2, 0], uncertainty=True)
    for name in PLUG + NEW:
        np.testing.assert_array_equal(getattr(sel, name).numpy(), getattr(s, name).numpy()[[2, 0]], err_msg=name)
    # latent: per component
    lat = m.sobol_indices(latent=True, uncertainty=True)
    np.testing.assert_allclose(lat.expected_variance.numpy() - lat.variance.numpy(), Cq[:, 4], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(lat.integrated_variance.numpy(), ivq, rtol=1e-13)
    np.testing.assert_array_equal(m.integrated_variance(latent=True).numpy(), lat.integrated_variance.numpy())
    assert m.integrated_variance(latent=True, outputs=1).shape == (1,)
    # a sub-box changes the answer
    xn = np.asarray(x)
    lo, hi = xn.min(axis=0), xn.max(axis=0)
    sub = np.stack([lo + 0.3 * (hi - lo), lo + 0.6 * (hi - lo)])
    got = m.integrated_variance(box=sub, latent=True).numpy()
    np.testing.assert_allclose(got, _direct(m, sub)[1], rtol=1e-12)
    assert not np.allclose(got, ivq, rtol=1e-3)


def test_integrated_variance_is_the_box_mean_of_predict_less_the_nugget_constant():
    """the box mean of predict()'s yconfvar at new inputs, by the piecewise tensor rule, exceeds integrated_variance() by
    scale_a^2 sum_k W_ka^2 scale_k nt_k"""
    m, x = model_of('full', 'se')
    xn = np.asarray(x)
    lo, hi = xn.min(axis=0), xn.max(axis=0)
    rules = [ref.piecewise_gauss_legendre(6, lo[l], hi[l], xn[:, l]) for l in range(2)]
    g0, g1 = np.meshgrid(rules[0][0], rules[1][0], indexing='ij')
    wt = (rules[0][1][:, None] * rules[1][1][None, :]).reshape(-1)
    yconfvar = m.predict(np.stack([g0.reshape(-1), g1.reshape(-1)], axis=1))[2].numpy()
    W, _, scale, _ = m._output_map()
    nug = m.lnugGPs.numpy()
    const = scale ** 2 * ((W ** 2).T @ (m.lLmb0.numpy() * nug / (1.0 + nug)))
    iv = m.integrated_variance().numpy()
    np.testing.assert_allclose(yconfvar @ wt - const, iv, rtol=0, atol=1e-9 * np.max(yconfvar))


def test_refuses_bad_arguments():
    m, x = model_of('full')
    xn = np.asarray(x)
    lo, hi = xn.min(axis=0), xn.max(axis=0)
    with pytest.raises(ValueError, match='upper > lower'):
        m.integrated_variance(box=np.stack([hi, lo]))
    with pytest.raises(ValueError, match='outputs'):
        m.integrated_variance(outputs=[3])
    with pytest.raises(ValueError, match='outputs'):
        m.sobol_indices(outputs=[2], latent=True, uncertainty=True)


def test_c_abi_of_the_matrix_entry():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() == 610
    for name in ('lcgp_sobol_matrix_pairs', 'lcgp_sobol_matrix_scratch_bytes', 'lcgp_sobol_pairs', 'lcgp_sobol_scratch_bytes'):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    nb = C.c_size_t(0)
    # n = 1000 -> 16 x 16 tiles; the table, the means, 2 d + 2 tile sums of min(nks, 64) components
    assert lib.lcgp_sobol_matrix_scratch_bytes(1000, 3, 4, 4, C.byref(nb)) == 0
    assert nb.value == 8 * (4 * 3 * 1000 + 4 + 4 * 256 * 8)
    assert lib.lcgp_sobol_matrix_scratch_bytes(1000, 3, 80, 80, C.byref(nb)) == 0
    assert nb.value == 8 * (80 * 3 * 1000 + 80 + 64 * 256 * 8)
    assert lib.lcgp_sobol_matrix_scratch_bytes(1000, 127, 4, 4, C.byref(nb)) < 0 and b'd must be' in lib.lcgp_last_error()
    assert lib.lcgp_sobol_matrix_scratch_bytes(0, 3, 4, 4, C.byref(nb)) < 0 and b'n < 1' in lib.lcgp_last_error()
    assert lib.lcgp_sobol_matrix_scratch_bytes(1000, 3, 4, 0, C.byref(nb)) < 0 and b'nks' in lib.lcgp_last_error()
    assert lib.lcgp_sobol_matrix_scratch_bytes(1000, 3, 4, 4, None) < 0 and b'NULL' in lib.lcgp_last_error()
    # the scratch of lcgp_sobol_pairs is what it was
    assert lib.lcgp_sobol_scratch_bytes(1000, 3, 4, 10, C.byref(nb)) == 0 and nb.value == 8 * (4 * 3 * 1000 + 4 + 10 * 256 * 7)
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything
    good = (C.c_int * 2)(0, 1)

    def call(dtype=_hip.F64, kern=0, n=100, d=2, p=3, q=2, x=dummy, v=dummy, ell=dummy, box=dummy, ws=dummy, ks=good, nks=2,
             scratch=dummy, out=dummy):
        return lib.lcgp_sobol_matrix_pairs(None, dtype, kern, n, d, p, q, x, v, ell, box, ws, ks, nks, scratch, out)

    assert call(dtype=_hip.F32) < 0 and b'float64' in lib.lcgp_last_error()
    assert call(kern=7) < 0 and b'kernel_id' in lib.lcgp_last_error()
    assert call(d=0) < 0 and b'd must be' in lib.lcgp_last_error()
    assert call(d=127) < 0 and b'd must be' in lib.lcgp_last_error()
    assert call(n=0) < 0 and b'n < 1' in lib.lcgp_last_error()
    assert call(q=0) < 0 and b'q_local' in lib.lcgp_last_error()
    assert call(nks=0) < 0 and b'nks' in lib.lcgp_last_error()
    for arg in ('x', 'v', 'ell', 'box', 'ws', 'ks', 'scratch', 'out'):
        assert call(**{arg: None}) < 0 and b'NULL' in lib.lcgp_last_error(), arg
    assert call(ks=(C.c_int * 2)(0, 2)) < 0 and b'ks must' in lib.lcgp_last_error()
    assert call(ks=(C.c_int * 2)(-1, 1)) < 0 and b'ks must' in lib.lcgp_last_error()
