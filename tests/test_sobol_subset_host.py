"""CPU tests of the closed variances of arbitrary input subsets (LCGP.sobol_subsets, sobol_indices(order=2), shapley_effects;
DESIGN.md 4.25): the restatement of tests/sobol_subset_ref.py against a piecewise tensor Gauss-Legendre rule over its own surface,
the device's subset product (lcgp_amd/csrc/sobol_subset.h) compiled for the host against the restatement, the host layer (mask
building, the order=2 algebra, the Shapley weights, the expectations, the argument checks) through a numpy stand-in of the
engine's three subset methods, and the C entries of the library (tests/test_gpu_sobol_subsets.py runs the same on the GPU)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

from lcgp_amd import LCGP, synth
from oracle import lcgp_oracle as orc
from tests import marginal_ref as mref
from tests import sobol_ref as ref
from tests import sobol_subset_ref as sref
from tests.test_sobol_host import patch_engine
from tests.test_sobol_uncertainty_host import UncertaintyOracleEngine, model_of as model_d2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ('matern32', 'se', 'matern52')
PLUG = ('first', 'total', 'variance', 'mean', 'first_variance', 'closed_variance')
EXPECTED = ('expected_variance', 'expected_first_variance', 'expected_closed_variance', 'first_expected', 'total_expected',
            'integrated_variance')


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', KERNELS)
def test_restatement_against_tensor_quadrature_of_its_own_surface(kernel):
    """d = 2, n = 12, two components: V^c_{0} and V^c_{01} of each component (the pair (k, k)) and their covariances between
    the components (the pair (0, 1)) against the piecewise tensor Gauss-Legendre rule split at the training coordinates, 12
    nodes per piece.  Bar 1e-12 of size = sum |w_i| |w'_i'| (M_u + M_0), what D_u adds up; the empty mask gives exactly 0"""
    rng = np.random.default_rng(5)
    n, d = 12, 2
    x = rng.uniform(0.0, 1.0, (n, d))
    box = np.array([[0.1, 0.0], [0.9, 0.8]])
    ell = np.array([[0.35, 0.8], [1.1, 0.25]])
    w = rng.standard_normal((2, n))
    masks = [0b01, 0b11, 0b00, 0b10]
    rules = [ref.piecewise_gauss_legendre(12, box[0][l], box[1][l], x[:, l]) for l in range(d)]
    w0, w1 = rules[0][1], rules[1][1]
    f = [np.einsum('i,ia,ib->ab', w[k], mref.kappa(kernel, np.abs(rules[0][0][None, :] - x[:, :1]) / ell[k, 0]),
                   mref.kappa(kernel, np.abs(rules[1][0][None, :] - x[:, 1:]) / ell[k, 1])) for k in range(2)]
    mean = [w0 @ fk @ w1 for fk in f]
    worst = 0.0
    for k, kp in ((0, 0), (1, 1), (0, 1)):
        D, mm, size = sref.subset_pair_sums(kernel, x, w[k], ell[k], w[kp], ell[kp], box, masks)
        assert D[2] == 0.0
        assert abs(mm[0] - mean[k]) <= 1e-12 * np.sum(np.abs(w[k])) and abs(mm[1] - mean[kp]) <= 1e-12 * np.sum(np.abs(w[kp]))
        want = {0b01: w0 @ ((f[k] @ w1 - mean[k]) * (f[kp] @ w1 - mean[kp])),
                0b10: ((w0 @ f[k] - mean[k]) * (w0 @ f[kp] - mean[kp])) @ w1,
                0b11: w0 @ ((f[k] - mean[k]) * (f[kp] - mean[kp])) @ w1}
        for s, mask in enumerate(masks):
            if mask:
                ratio = abs(D[s] - want[mask]) / size[s]
                print('restatement against quadrature', kernel, (k, kp), bin(mask), 'ratio', ratio)
                worst = max(worst, ratio)
                assert ratio <= 1e-12, (kernel, k, kp, mask, D[s], want[mask])
        # the classical subsets are the columns of the pair sums of tests/sobol_ref.py
        Dc, _, sizec = ref.pair_sums(kernel, x, w[k], ell[k], w[kp], ell[kp], box)
        got, _, _ = sref.subset_pair_sums(kernel, x, w[k], ell[k], w[kp], ell[kp], box, sref.classical_masks(d))
        assert np.all(np.abs(got - Dc) <= 1e-14 * sizec)
    print('restatement against quadrature', kernel, 'worst ratio', worst)


# ---- the device's subset product, compiled for the host --------------------------------------------------------------------
@pytest.fixture(scope='module')
def subset_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('subset') / 'sobol_subset_host')
    subprocess.run(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-I', os.path.join(ROOT, 'lcgp_amd', 'csrc'), '-o', exe,
                    os.path.join(ROOT, 'tests', 'native', 'sobol_subset_host.cpp')], check=True)
    return exe


@pytest.mark.parametrize('dd', [8, 16])
def test_device_subset_product_on_the_host_equals_the_restatement(subset_host, tmp_path, dd):
    """random J and A with zeros, denormals and products that underflow among them, dimensions beyond d neutral (1.0) as the
    kernel pads them, random masks plus the empty and the full one: m0, the product and the difference are BITWISE the
    restatement's (the same factors in the same order, nothing contracted); the empty mask gives exactly 0, also where m0 is
    a denormal or 0"""
    rng = np.random.default_rng(17 + dd)
    nrec = 4000
    d = rng.integers(1, dd + 1, nrec)
    J = 10.0 ** rng.uniform(-3.0, 0.0, (nrec, dd))
    A = 10.0 ** rng.uniform(-3.0, 0.0, (nrec, dd))
    special = np.array([0.0, 5e-324, 1e-310, 2.3e-308, 1e-200, 1e-160, 1.0])
    for arr in (J, A):
        hit = rng.random((nrec, dd)) < 0.15
        arr[hit] = rng.choice(special, int(hit.sum()))
    beyond = np.arange(dd)[None, :] >= d[:, None]
    J[beyond] = 1.0
    A[beyond] = 1.0
    full = (np.uint64(1) << d.astype(np.uint64)) - np.uint64(1)
    masks = rng.integers(0, 1 << 16, nrec).astype(np.uint64) & full
    masks[::7] = 0
    masks[3::7] = full[3::7]
    rec = np.zeros(nrec, dtype=[('mask', '<u8'), ('J', '<f8', dd), ('A', '<f8', dd)])
    rec['mask'], rec['J'], rec['A'] = masks, J, A
    fin, fout = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    rec.tofile(fin)
    subprocess.run([subset_host, str(dd), fin, fout], check=True)
    got = np.fromfile(fout, '<f8').reshape(nrec, 3)
    want_m0 = sref.subset_product(0, J, A)
    want_p = np.array([sref.subset_product(int(m), J[i], A[i]) for i, m in enumerate(masks)])
    np.testing.assert_array_equal(got[:, 0], want_m0)
    np.testing.assert_array_equal(got[:, 1], want_p)
    np.testing.assert_array_equal(got[:, 2], want_p - want_m0)
    assert np.all(got[masks == 0, 2] == 0.0) and np.any(want_m0 == 0.0) and np.any((want_m0 > 0.0) & (want_m0 < 2.3e-308))
    assert np.all(got[masks == full, 1] == np.array([sref.subset_product((1 << dd) - 1, J[i], A[i]) for i in np.flatnonzero(masks == full)]))


# ---- the host layer ----------------------------------------------------------------------------------------------------------
class SubsetOracleEngine(UncertaintyOracleEngine):
    """UncertaintyOracleEngine plus the subset methods, in numpy float64 from tests/sobol_subset_ref.py"""

    def sobol_subset_pairs(self, x, w, ell, box, pairs, masks):
        x, w, ell, box = (np.asarray(a, np.float64) for a in (x, w, ell, box))
        masks = np.asarray(masks)
        assert masks.dtype == np.uint64 and masks.ndim == 1 and not np.any(masks >> np.uint64(x.shape[1]))
        D, means = np.zeros((len(pairs), len(masks))), np.zeros(len(pairs))
        for r, (k, kp) in enumerate(np.asarray(pairs)):
            D[r], m, _ = sref.subset_pair_sums(self.kernel, x, w[k], ell[k], w[kp], ell[kp], box, masks)
            means[r] = m[0] if k == kp else 0.0
        self.calls = getattr(self, 'calls', []) + [('vec', len(masks))]
        return D, means

    def sobol_matrix_subset_sums(self, x, v, ell, box, ks, masks):
        x, v, ell, box = (np.asarray(a, np.float64) for a in (x, v, ell, box))
        n = x.shape[0]
        sums = np.zeros((len(ks), len(masks)))
        for r, k in enumerate(np.asarray(ks)):
            ainv = sla.cho_solve((self._state[k][1], True), np.eye(n))
            sums[r], _ = sref.subset_matrix_sums(self.kernel, x, ell[k], box, v[k][:, None] * v[k][None, :] * ainv, masks)
        self.calls = getattr(self, 'calls', []) + [('mat', len(masks))]
        return sums


def _with_subsets(m):
    make = m._make_engine

    def _make(dtype=None):
        e = make(dtype)
        if e is not None:
            e.__class__ = SubsetOracleEngine
        return e
    m._make_engine = _make
    m._engine = None
    m._invalidate()
    return m


def model_d3(kernel='matern32', mode='full'):
    """d = 3, p = 4 outputs, q = 2 components through the stand-in"""
    if mode == 'full':
        x, y = synth.make_full(91, 18, 3, 4, 2)
    else:
        x, y = synth.make_rep(92, 9, 2, 3, 4, 2)
    m = _with_subsets(patch_engine(LCGP(y=y, x=x, q=2, submethod=mode, kernel=kernel)))
    o = orc.OracleLCGP(y=y, x=x, q=2, submethod=mode)
    m._set_flat(synth.param_points(91, o.get_unconstrained())[1])
    return m, x


def _np(t):
    return t.numpy()


@pytest.mark.parametrize('mode,kernel', [('full', 'matern32'), ('rep', 'se'), ('full', 'matern52')])
def test_sobol_subsets_assemble_the_subset_sums(mode, kernel):
    m, _ = model_d3(kernel, mode)
    d = 3
    subsets = [(0,), (2, 0), (), (0, 1, 2), [1], (1, 2), (0, 2)]
    s = m.sobol_subsets(subsets, uncertainty=True)
    assert 'SobolSubsets' in repr(s) and s.subsets == [tuple(u) for u in subsets]
    assert s.closed_variance.shape == (4, 7) and s.closed.shape == (4, 7) and s.variance.shape == (4,) and s.mean.shape == (4,)
    base = m.sobol_indices(uncertainty=True)
    V = _np(base.variance)
    # the classical subsets are sobol_indices' fields, the full set is V, the empty one exactly 0, order inside a subset is free
    Vc = _np(s.closed_variance)
    np.testing.assert_allclose(Vc[:, 0], _np(base.first_variance)[:, 0], rtol=0, atol=1e-13 * V.max())
    np.testing.assert_allclose(Vc[:, 4], _np(base.first_variance)[:, 1], rtol=0, atol=1e-13 * V.max())
    np.testing.assert_allclose(Vc[:, 5], _np(base.closed_variance)[:, 0], rtol=0, atol=1e-13 * V.max())
    np.testing.assert_allclose(Vc[:, 3], V, rtol=1e-13)
    np.testing.assert_allclose(_np(s.variance), V, rtol=1e-13)
    np.testing.assert_allclose(_np(s.mean), _np(base.mean), rtol=1e-13)
    assert np.all(Vc[:, 2] == 0.0) and np.all(_np(s.closed)[:, 2] == 0.0)
    np.testing.assert_array_equal(Vc[:, 1], Vc[:, 6])
    np.testing.assert_array_equal(_np(s.closed), Vc / _np(s.variance)[:, None])
    np.testing.assert_array_equal(_np(s.closed)[:, 3], np.ones(4))
    # monotone under inclusion, with and without the emulator's uncertainty
    E = _np(s.expected_closed_variance)
    for arr in (Vc, E):
        assert np.all(arr[:, 0] <= arr[:, 1] + 1e-13 * V.max()) and np.all(arr[:, 1] <= arr[:, 3] + 1e-13 * V.max())
    # the expectations: sobol_indices(uncertainty=True)'s for the classical subsets, never below the plug-in values
    EV = _np(base.expected_variance)
    np.testing.assert_allclose(E[:, 0], _np(base.expected_first_variance)[:, 0], rtol=0, atol=1e-13 * EV.max())
    np.testing.assert_allclose(E[:, 5], _np(base.expected_closed_variance)[:, 0], rtol=0, atol=1e-13 * EV.max())
    np.testing.assert_allclose(_np(s.expected_variance), EV, rtol=1e-13)
    assert np.all(E >= Vc - 1e-13 * EV.max()) and np.all(E[:, 2] == 0.0)
    np.testing.assert_array_equal(_np(s.closed_expected), E / _np(s.expected_variance)[:, None])
    # without uncertainty: the same plug-in fields bitwise, the others None; outputs= and latent= select rows
    p = m.sobol_subsets(subsets)
    for name in ('closed_variance', 'closed', 'variance', 'mean'):
        np.testing.assert_array_equal(_np(getattr(p, name)), _np(getattr(s, name)))
    assert p.expected_closed_variance is None and p.closed_expected is None and p.expected_variance is None
    sel = m.sobol_subsets(subsets, outputs=[3, 1])
    np.testing.assert_array_equal(_np(sel.closed_variance), Vc[[3, 1]])
    lat = m.sobol_subsets([(0, 1)], latent=True, uncertainty=True)
    assert lat.closed_variance.shape == (2, 1) and lat.expected_closed_variance.shape == (2, 1)
    # one pass each: the caller's masks plus the full set
    eng = m._ensure_aux64()
    eng.calls = []
    m.sobol_subsets(subsets, uncertainty=True)
    assert eng.calls == [('vec', 8), ('mat', 8)]
    assert d == int(m.d)


@pytest.mark.parametrize('mode,kernel', [('full', 'se'), ('rep', 'matern32')])
def test_order_two_adds_the_interactions_and_leaves_order_one_bitwise(mode, kernel):
    m, _ = model_d3(kernel, mode)
    d = 3
    a, b = m.sobol_indices(uncertainty=True), m.sobol_indices(uncertainty=True, order=2)
    for name in PLUG + EXPECTED:
        np.testing.assert_array_equal(_np(getattr(a, name)), _np(getattr(b, name)), err_msg=name)
    for name in ('second', 'second_variance', 'expected_second_variance', 'second_expected'):
        assert getattr(a, name) is None and getattr(b, name).shape == (4, d, d), name
    one = m.sobol_indices(order=1)
    for name in PLUG:
        np.testing.assert_array_equal(_np(getattr(a, name)), _np(getattr(one, name)), err_msg=name)
    plain = m.sobol_indices(order=2)
    assert plain.expected_second_variance is None and plain.second_expected is None
    np.testing.assert_array_equal(_np(plain.second_variance), _np(b.second_variance))
    pairs = [(0, 1), (0, 2), (1, 2)]
    s = m.sobol_subsets(pairs, uncertainty=True)
    V, EV = _np(b.variance), _np(b.expected_variance)
    for (sv, sn, cv, fv, tot) in ((_np(b.second_variance), _np(b.second), _np(s.closed_variance), _np(b.first_variance), V),
                                  (_np(b.expected_second_variance), _np(b.second_expected), _np(s.expected_closed_variance),
                                   _np(b.expected_first_variance), EV)):
        assert np.all(np.isnan(sv[:, np.arange(d), np.arange(d)])) and np.all(np.isnan(sn[:, np.arange(d), np.arange(d)]))
        for c, (l, k) in enumerate(pairs):
            np.testing.assert_array_equal(sv[:, l, k], cv[:, c] - fv[:, l] - fv[:, k])
            np.testing.assert_array_equal(sv[:, k, l], sv[:, l, k])
            np.testing.assert_array_equal(sn[:, l, k], sv[:, l, k] / tot)
    # d = 3: V = sum V_l + sum V_lm + V_012, and the total of input 0 holds V_0, V_01, V_02 and V_012
    sv = _np(b.second_variance)
    v012 = V - _np(b.first_variance).sum(axis=1) - sv[:, 0, 1] - sv[:, 0, 2] - sv[:, 1, 2]
    total0 = (_np(b.first_variance)[:, 0] + sv[:, 0, 1] + sv[:, 0, 2] + v012) / V
    np.testing.assert_allclose(total0, _np(b.total)[:, 0], rtol=0, atol=1e-12)
    assert np.all(sv[:, [0, 0, 1], [1, 2, 2]] >= -1e-13 * V[:, None])
    eng = m._ensure_aux64()
    eng.calls = []
    m.sobol_indices(order=2)
    assert eng.calls == [('vec', 3)]


def test_order_two_at_d_2_is_what_the_first_order_indices_leave():
    m, _ = model_d2('full', 'matern52')
    m = _with_subsets(m)
    s = m.sobol_indices(order=2)
    first, second = _np(s.first), _np(s.second)
    assert second.shape == (3, 2, 2)
    np.testing.assert_allclose(second[:, 0, 1], 1.0 - first[:, 0] - first[:, 1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(second[:, 0, 1], _np(s.total)[:, 0] - first[:, 0], rtol=0, atol=1e-12)
    sh = m.shapley_effects()
    np.testing.assert_allclose(_np(sh.effects)[:, 0], _np(s.first_variance)[:, 0] + 0.5 * _np(s.second_variance)[:, 0, 1],
                               rtol=0, atol=1e-13 * _np(s.variance).max())


@pytest.mark.parametrize('mode,kernel', [('full', 'matern32'), ('rep', 'matern52')])
def test_shapley_effects_against_the_permutation_definition(mode, kernel):
    """d = 3: the 6 orderings; the effects add up to V; V_l <= effect_l <= V - V_~l"""
    m, _ = model_d3(kernel, mode)
    d = 3
    sh = m.shapley_effects(uncertainty=True)
    assert 'ShapleyEffects' in repr(sh) and sh.effects.shape == (4, d) and sh.shares.shape == (4, d) and sh.variance.shape == (4,)
    allsets = [tuple(l for l in range(d) if (s >> l) & 1) for s in range(1 << d)]
    assert len(list(itertools.permutations(range(d)))) == 6
    sub = m.sobol_subsets(allsets, uncertainty=True)
    base = m.sobol_indices(uncertainty=True)
    for eff, shares, var, closed, fv, cv in (
            (_np(sh.effects), _np(sh.shares), _np(sh.variance), _np(sub.closed_variance), _np(base.first_variance), _np(base.closed_variance)),
            (_np(sh.effects_expected), _np(sh.shares_expected), _np(sh.expected_variance), _np(sub.expected_closed_variance),
             _np(base.expected_first_variance), _np(base.expected_closed_variance))):
        want = sref.shapley_by_permutations(lambda mask: closed[:, mask], d)
        np.testing.assert_allclose(eff, want, rtol=0, atol=1e-14 * var.max())
        np.testing.assert_allclose(eff.sum(axis=1), var, rtol=1e-13)
        np.testing.assert_array_equal(var, closed[:, -1])
        np.testing.assert_array_equal(shares, eff / var[:, None])
        assert np.all(eff >= fv - 1e-13 * var[:, None]) and np.all(eff <= var[:, None] - cv + 1e-13 * var[:, None])
    plain = m.shapley_effects(outputs=[2], latent=False)
    np.testing.assert_array_equal(_np(plain.effects), _np(sh.effects)[[2]])
    assert plain.effects_expected is None and plain.shares_expected is None and plain.expected_variance is None
    assert m.shapley_effects(latent=True).effects.shape == (2, d)
    eng = m._ensure_aux64()
    eng.calls = []
    m.shapley_effects(uncertainty=True)
    assert eng.calls == [('vec', 8), ('mat', 8)]


def test_a_constant_output_has_nan_shares():
    m, _ = model_d3('se')
    m.phi[1, :] = 0.0
    m._invalidate()
    sh, s = m.shapley_effects(), m.sobol_subsets([(0, 1)])
    assert _np(sh.variance)[1] == 0.0 and np.all(np.isnan(_np(sh.shares)[1])) and np.all(_np(sh.effects)[1] == 0.0)
    assert np.all(np.isnan(_np(s.closed)[1])) and np.all(np.isfinite(_np(s.closed)[[0, 2, 3]]))
    assert np.all(np.isnan(_np(m.sobol_indices(order=2).second)[1]))


def test_refuses_bad_arguments():
    m, _ = model_d3()
    for bad in ([(3,)], [(0, -1)], [(0, 1), (1, 7)]):
        with pytest.raises(ValueError, match='outside'):
            m.sobol_subsets(bad)
    with pytest.raises(ValueError, match='repeats'):
        m.sobol_subsets([(0, 1, 0)])
    for bad in (3, [0, 1], 'ab'):
        with pytest.raises(ValueError, match='sequence of sequences'):
            m.sobol_subsets(bad)
    with pytest.raises(ValueError, match='outputs'):
        m.sobol_subsets([(0,)], outputs=[4])
    for bad in (0, 3, '2', 1.5, True):
        with pytest.raises(ValueError, match='order'):
            m.sobol_indices(order=bad)
    with pytest.raises(ValueError, match='outputs'):
        m.shapley_effects(outputs=[2], latent=True)
    # the limits, checked before anything is evaluated: d > 16 for subsets, d > 10 for Shapley effects
    x, y = synth.make_full(93, 30, 17, 3, 2)
    wide = LCGP(y=y, x=x, q=2)
    with pytest.raises(ValueError, match='16'):
        wide.sobol_subsets([(0,)])
    with pytest.raises(ValueError, match='16'):
        wide._subset_masks([()])
    x, y = synth.make_full(94, 30, 11, 3, 2)
    eleven = LCGP(y=y, x=x, q=2)
    with pytest.raises(ValueError, match='d = 11 > 10'):
        eleven.shapley_effects()
    assert eleven._subset_masks([(10, 0), ()])[1].tolist() == [1025, 0]


# ---- the C entries -----------------------------------------------------------------------------------------------------------
def test_c_abi_of_the_subset_entries():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() == 610
    for name in ('lcgp_sobol_subset_chunk', 'lcgp_sobol_subset_scratch_bytes', 'lcgp_sobol_subset_pairs',
                 'lcgp_sobol_matrix_subset_pairs', 'lcgp_condition_sobol_subset_scratch_bytes',
                 'lcgp_condition_sobol_matrix_subset_pairs'):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    assert lib.lcgp_sobol_subset_chunk(3) == 32 and lib.lcgp_sobol_subset_chunk(8) == 32
    assert lib.lcgp_sobol_subset_chunk(9) == 32 and lib.lcgp_sobol_subset_chunk(16) == 32
    assert lib.lcgp_sobol_subset_chunk(17) < 0 and b'16' in lib.lcgp_last_error()
    assert lib.lcgp_sobol_subset_chunk(0) < 0
    nb = C.c_size_t(0)
    # n = 1000 -> 16 x 16 tiles; the table, the means, chunk tile sums of min(npairs, 64) pairs, whatever nsub
    for nsub in (1, 8, 1000):
        assert lib.lcgp_sobol_subset_scratch_bytes(1000, 3, 4, 10, nsub, C.byref(nb)) == 0
        assert nb.value == 8 * (4 * 3 * 1000 + 4 + 10 * 256 * 32)
    assert lib.lcgp_sobol_subset_scratch_bytes(1000, 11, 12, 78, 5, C.byref(nb)) == 0
    assert nb.value == 8 * (12 * 11 * 1000 + 12 + 64 * 256 * 32)
    assert lib.lcgp_sobol_subset_scratch_bytes(1000, 17, 4, 10, 5, C.byref(nb)) < 0 and b'16' in lib.lcgp_last_error()
    assert lib.lcgp_sobol_subset_scratch_bytes(0, 3, 4, 10, 5, C.byref(nb)) < 0 and b'n < 1' in lib.lcgp_last_error()
    assert lib.lcgp_sobol_subset_scratch_bytes(1000, 3, 4, 10, 0, C.byref(nb)) < 0 and b'nsub' in lib.lcgp_last_error()
    assert lib.lcgp_sobol_subset_scratch_bytes(1000, 3, 4, 10, 5, None) < 0 and b'NULL' in lib.lcgp_last_error()
    # the existing formulas stay
    assert lib.lcgp_sobol_scratch_bytes(1000, 3, 4, 10, C.byref(nb)) == 0 and nb.value == 8 * (4 * 3 * 1000 + 4 + 10 * 256 * 7)
    plain, sub = C.c_size_t(0), C.c_size_t(0)
    assert lib.lcgp_condition_sobol_scratch_bytes(1000, 3, 2, 20, 2, C.byref(plain)) == 0
    assert lib.lcgp_condition_sobol_subset_scratch_bytes(1000, 3, 2, 20, 2, 9, C.byref(sub)) == 0
    assert sub.value - plain.value == 8 * 256 * (32 - 8)            # (16 x 16 tiles of the 1020 centres: 32 sums for 2 d + 2)
    assert lib.lcgp_condition_sobol_subset_scratch_bytes(1000, 17, 2, 20, 2, 9, C.byref(sub)) < 0 and b'16' in lib.lcgp_last_error()
    assert lib.lcgp_condition_sobol_subset_scratch_bytes(1000, 3, 2, 20, 2, 0, C.byref(sub)) < 0 and b'nsub' in lib.lcgp_last_error()
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything
    pairs = (C.c_int * 4)(0, 0, 0, 1)
    ks = (C.c_int * 2)(0, 1)
    good = (C.c_uint64 * 3)(0, 3, 1)

    def vec(kern=0, n=100, d=2, q=2, x=dummy, w=dummy, ell=dummy, box=dummy, pairs=pairs, npairs=2, masks=good, nsub=3,
            scratch=dummy, out=dummy):
        return lib.lcgp_sobol_subset_pairs(None, kern, n, d, q, x, w, ell, box, pairs, npairs, masks, nsub, scratch, out)

    def mat(dtype=_hip.F64, kern=0, n=100, d=2, p=3, q=2, x=dummy, v=dummy, ell=dummy, box=dummy, ws=dummy, ks=ks, nks=2,
            masks=good, nsub=3, scratch=dummy, out=dummy):
        return lib.lcgp_sobol_matrix_subset_pairs(None, dtype, kern, n, d, p, q, x, v, ell, box, ws, ks, nks, masks, nsub, scratch, out)

    def view(dtype=_hip.F64, kern=0, n=100, d=2, p=3, q=2, theta=dummy, ws=dummy, state=dummy, m=5, xa=dummy, v=dummy, ell=dummy,
             box=dummy, ks=ks, nks=2, masks=good, nsub=3, scratch=dummy, nbytes=1 << 40, out=dummy):
        return lib.lcgp_condition_sobol_matrix_subset_pairs(None, dtype, kern, n, d, p, q, theta, ws, state, m, xa, v, ell, box, ks,
                                                            nks, masks, nsub, scratch, nbytes, out)

    for call in (vec, mat, view):
        assert call(d=17) < 0 and b'16' in lib.lcgp_last_error(), call
        assert call(nsub=0) < 0 and b'nsub' in lib.lcgp_last_error(), call
        assert call(n=0) < 0 and b'n' in lib.lcgp_last_error(), call
        assert call(masks=None) < 0 and b'NULL' in lib.lcgp_last_error(), call
        assert call(masks=(C.c_uint64 * 3)(0, 4, 1)) < 0 and b'bit at or above d' in lib.lcgp_last_error(), call
        assert call(masks=(C.c_uint64 * 3)(0, 1 << 40, 1)) < 0 and b'bit at or above d' in lib.lcgp_last_error(), call
        assert call(kern=7) < 0 and b'kernel' in lib.lcgp_last_error(), call
        for arg in ('ell', 'box', 'scratch', 'out'):
            assert call(**{arg: None}) < 0 and b'NULL' in lib.lcgp_last_error(), (call, arg)
    assert vec(n=0) < 0 and b'n < 1' in lib.lcgp_last_error()
    for arg in ('x', 'w', 'pairs'):
        assert vec(**{arg: None}) < 0 and b'NULL' in lib.lcgp_last_error(), arg
    assert vec(pairs=(C.c_int * 4)(0, 0, 0, 2)) < 0 and b'pairs' in lib.lcgp_last_error()
    for call in (mat, view):
        assert call(dtype=_hip.F32) < 0 and b'float64 workspace' in lib.lcgp_last_error(), call
        assert call(ks=(C.c_int * 2)(0, 2)) < 0 and b'ks' in lib.lcgp_last_error(), call
        assert call(ks=None) < 0 and b'NULL' in lib.lcgp_last_error(), call
    for arg in ('x', 'v', 'ws'):
        assert mat(**{arg: None}) < 0 and b'NULL' in lib.lcgp_last_error(), arg
    for arg in ('theta', 'ws', 'state', 'xa', 'v'):
        assert view(**{arg: None}) < 0 and b'NULL' in lib.lcgp_last_error(), arg
    assert view(nbytes=64) < 0 and b'scratch too small' in lib.lcgp_last_error()
    assert view(m=0) < 0 and b'm < 1' in lib.lcgp_last_error()
