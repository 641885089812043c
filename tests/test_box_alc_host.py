"""CPU tests of the exact box ALC (LCGP.integrated_variance_reduction, lcgp_box_alc): the restatement of
tests/box_alc_ref.py against the integrated variance of the model with the candidate taken into the training set
(tests/sobol_uncertainty_ref.py) and against quadrature of the squared posterior covariance (marginal_ref.continuous_cov); the
host layer through a numpy stand-in of HotPathEngine.box_alc_block; the argument checks; the C entries of the library
(tests/test_gpu_box_alc.py runs the same through liblcgp_hip.so on the GPU).

The three terms of the closed form cancel (their absolute sum, `size`, is 6 to 353 c here where the gain is 5e-5 to 7e-3 of
c), so every bar is stated against c = scale (1 - nt), never against the gain."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla

from tests import box_alc_ref as bref
from tests import marginal_ref as mref
from tests import sobol_ref as ref
from tests import sobol_uncertainty_ref as uref
from tests.test_sobol_uncertainty_host import UncertaintyOracleEngine, model_of as uncertainty_model_of

KERNELS = ('matern32', 'se', 'matern52')
BOXES = {'default': np.array([[0.0, 0.0], [1.0, 1.0]]), 'sub': np.array([[0.1, 0.0], [0.9, 0.8]])}
TH = np.array([0.35, 0.8, 1.7, 0.02, 40.0])               # ell (2), scale, nug, D


def _component(kernel, sr_kind, n=12, d=2, seed=5):
    """one component at n = 12, d = 2 in the unit square, unit or replicate weights sr; six candidates: four in the square, one
    outside every box, and (rep) unique input 3 itself.  Returns (x, sr, ainv, low, xc, match)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (n, d))
    sr = np.ones(n) if sr_kind == 'full' else np.sqrt(rng.integers(1, 4, n).astype(float))
    ainv, _, low = uref.dense_ainv(kernel, x, sr, TH)
    xc = np.vstack([rng.uniform(0.0, 1.0, (4, d)), [[1.2, -0.1]]])
    match = np.full(len(xc), -1)
    if sr_kind == 'rep':
        xc, match = np.vstack([xc, x[3:4]]), np.r_[match, 3]
    return x, sr, ainv, low, xc, match


@pytest.mark.parametrize('box_name', ['default', 'sub'])
@pytest.mark.parametrize('sr_kind', ['full', 'rep'])
@pytest.mark.parametrize('kernel', KERNELS)
def test_restatement_is_the_drop_of_the_integrated_variance(kernel, sr_kind, box_name):
    """R(c) against IV(model) - IV(model with the candidate taken in), both through sobol_uncertainty_ref.component with a dense
    A^-1 of the n and of the n + 1 (rep, matched: n) inputs.  Bar 1e-11 c: either IV rounds at 1e-16 of c + sum |Q| (M + M_0),
    some hundred c, and A^-1 of the augmented model at its condition number times that."""
    box = BOXES[box_name]
    x, sr, ainv, _, xc, match = _component(kernel, sr_kind)
    iv0 = uref.component(kernel, x, sr, TH, ainv, box)['IV']
    worst = 0.0
    for r in ((1, 3) if sr_kind == 'rep' else (1,)):
        t = bref.terms(kernel, x, sr, TH, ainv, box, xc, match, r)
        for j in range(len(xc)):
            xa, sa = bref.augmented(x, sr, xc[j], match[j], r)
            iv1 = uref.component(kernel, xa, sa, TH, uref.dense_ainv(kernel, xa, sa, TH)[0], box)['IV']
            err = abs(t['R'][j] - (iv0 - iv1)) / t['c']
            worst = max(worst, err)
            assert err <= 1e-11, (kernel, sr_kind, r, j, t['R'][j], iv0 - iv1)
            assert t['R'][j] > 0.0 and t['size'][j] >= abs(t['R'][j])
    print('identity', kernel, sr_kind, box_name, 'worst |R - (IV - IV_aug)| / c', worst)


def _quadrature(kernel, x, sr, low, box, xc, r, rules):
    """sum_a wt_a cov(t_a, c)^2 / den over the tensor rule: cov of the continuous surface between a node and the candidate, den =
    cov(c, c) + scale nt + 1 / (D r) -- predict()'s latent variance at a new input plus the noise of r runs"""
    g0, g1 = np.meshgrid(rules[0][0], rules[1][0], indexing='ij')
    pts = np.stack([g0.reshape(-1), g1.reshape(-1)], axis=1)
    wt = (rules[0][1][:, None] * rules[1][1][None, :]).reshape(-1)
    scale, nug, D = TH[2], TH[3], TH[4]
    # continuous_cov's formula for the block between the nodes and the candidates only (the rule has up to 2e4 nodes)
    cc, Xc = mref.continuous_cov(xc, x, sr, TH, low, kernel)
    c = scale * (1.0 - nug / (1.0 + nug))
    Xp = c * np.prod(mref.kappa(kernel, np.abs(pts[:, None, :] - x[None, :, :]) / TH[:2]), axis=2) * sr[None, :]
    K = c * np.prod(mref.kappa(kernel, np.abs(pts[:, None, :] - xc[None, :, :]) / TH[:2]), axis=2)
    cross = K - D * (sla.solve_triangular(low, Xp.T, lower=True).T @ sla.solve_triangular(low, Xc.T, lower=True))
    den = np.maximum(np.diag(cc) + scale * nug / (1.0 + nug), 0.0) + 1.0 / (D * r)
    out = wt @ (cross ** 2) / den
    return out


@pytest.mark.parametrize('sr_kind', ['full', 'rep'])
@pytest.mark.parametrize('kernel', KERNELS)
def test_restatement_against_quadrature_of_the_squared_covariance(kernel, sr_kind):
    """R(c) = int Cov(f(x), run at c)^2 dmu / den for candidates that are new inputs (d = 2, the sub-box).  SE: the integrand is
    analytic, a 16-node-per-dimension tensor Gauss-Legendre rule (its difference to the 32-node rule is printed).  The Matern
    kernels have kinks at the training and candidate coordinates, where an unbroken rule stalls near 1e-8: the piecewise rule of
    tests/sobol_ref.py broken there, 8 nodes per piece.  Bar 1e-11 c: the rule adds up at most 1e4 positive terms below R (1e4 eps
    R, R <= c), the closed form rounds at eps size (size: some hundred c), and the pair integral itself is within 1e-12 relative of
    quadrature (tests/test_sobol_host.py)."""
    box = BOXES['sub']
    x, sr, ainv, low, xc, _ = _component(kernel, sr_kind)
    xc = xc[:5]                                   # the new inputs (the fifth lies outside the box)
    for r in ((1, 3) if sr_kind == 'rep' else (1,)):
        t = bref.terms(kernel, x, sr, TH, ainv, box, xc, None, r)
        if kernel == 'se':
            want = _quadrature(kernel, x, sr, low, box, xc, r, [mref.gauss_legendre(16, box[0][l], box[1][l]) for l in range(2)])
            fine = _quadrature(kernel, x, sr, low, box, xc, r, [mref.gauss_legendre(32, box[0][l], box[1][l]) for l in range(2)])
            print('quadrature se', sr_kind, r, '16 against 32 nodes', np.max(np.abs(want - fine)) / t['c'])
        else:
            rules = [ref.piecewise_gauss_legendre(8, box[0][l], box[1][l], np.r_[x[:, l], xc[:, l]]) for l in range(2)]
            want = _quadrature(kernel, x, sr, low, box, xc, r, rules)
        err = np.abs(t['R'] - want) / t['c']
        print('quadrature', kernel, sr_kind, r, 'worst |R - rule| / c', np.max(err), 'R / c', t['R'] / t['c'])
        assert np.all(err <= 1e-11), (kernel, sr_kind, r, err)
        np.testing.assert_allclose(t['den'], np.maximum(t['gvar'], 0.0) + 1.0 / (TH[4] * r), rtol=0, atol=0)


# ---- the host layer ----------------------------------------------------------------------------------------------------------
class BoxAlcOracleEngine(UncertaintyOracleEngine):
    """UncertaintyOracleEngine plus box_alc_block, in numpy float64 from tests/box_alc_ref.py"""
    calls = None

    def box_alc_block(self, x_cand_s, box_s, match, r):
        import torch
        if self.calls is not None:
            self.calls.append((np.array(box_s), None if match is None else np.array(match), r))
        sr = np.ones(self.n) if self.sr is None else self.sr
        out = np.zeros((len(self._state), len(x_cand_s)))
        for k, s in enumerate(self._state):
            ainv = sla.cho_solve((s[1], True), np.eye(self.n))
            out[k] = bref.terms(self.kernel, self.x, sr, s[0], ainv, box_s, x_cand_s, match, r)['R']
        return torch.as_tensor(out)


def model_of(mode, kernel='matern32'):
    m, x = uncertainty_model_of(mode, kernel)
    make = m._make_engine

    def _make(dtype=None):
        e = make(dtype)
        if e is not None:
            e.__class__ = BoxAlcOracleEngine
        return e
    m._make_engine = _make
    m._engine = None
    m._invalidate()
    return m, x


def _candidates(m, x, rng, k=5):
    xn = np.asarray(x)
    lo, hi = xn.min(axis=0), xn.max(axis=0)
    new = lo - 0.05 * (hi - lo) + 1.1 * (hi - lo) * rng.random((k, xn.shape[1]))
    if m.submethod == 'rep':
        return np.vstack([new[:3], m.x_unique.numpy()[[4, 11]], new[3:]])
    return new


@pytest.mark.parametrize('mode,kernel', [(mode, kernel) for mode in ('full', 'rep') for kernel in KERNELS])
def test_model_maps_the_latent_gains_to_the_outputs(mode, kernel):
    m, x = model_of(mode, kernel)
    xc = _candidates(m, x, np.random.default_rng(3))
    eng = m._ensure_aux64()
    eng.calls = []
    R = m.integrated_variance_reduction(xc, latent=True).numpy()
    assert R.shape == (int(m.q), len(xc)) and R.dtype == np.float64
    box_s, match, r = eng.calls[-1]
    np.testing.assert_array_equal(box_s, np.stack([np.zeros(2), np.ones(2)]))
    if mode == 'rep':
        assert list(match) == [-1, -1, -1, 4, 11, -1, -1] and r == 1
    else:
        assert match is None and r == 1
    W, _, scale, _ = m._output_map()
    delta = m.integrated_variance_reduction(xc).numpy()
    np.testing.assert_allclose(delta, bref.output_map(R, W, scale), rtol=1e-14, atol=0)
    np.testing.assert_array_equal(m.integrated_variance_reduction(xc, outputs=[2, 0]).numpy(), delta[[2, 0]])
    # every gain is positive here and below the integrated variance it is taken from
    iv = m.integrated_variance().numpy()
    assert np.all(delta > 0.0) and np.all(delta <= iv[:, None])
    assert np.all(R <= m.integrated_variance(latent=True).numpy()[:, None])
    # a sub-box reaches the engine standardised and changes the answer
    xn = np.asarray(x)
    lo, hi = xn.min(axis=0), xn.max(axis=0)
    sub = np.stack([lo + 0.3 * (hi - lo), lo + 0.6 * (hi - lo)])
    Rs = m.integrated_variance_reduction(xc, box=sub, latent=True).numpy()
    np.testing.assert_allclose(eng.calls[-1][0], np.array([[0.3, 0.3], [0.6, 0.6]]), rtol=1e-13)
    assert not np.allclose(Rs, R, rtol=1e-3)
    if mode == 'rep':
        R3 = m.integrated_variance_reduction(xc, replicates=3, latent=True).numpy()
        assert eng.calls[-1][2] == 3 and np.all(R3 > R)


def test_refuses_bad_arguments():
    m, x = model_of('full')
    xn = np.asarray(x)
    lo, hi = xn.min(axis=0), xn.max(axis=0)
    with pytest.raises(ValueError, match='x_cand must have shape'):
        m.integrated_variance_reduction(xn[:, :1])
    with pytest.raises(ValueError, match='upper > lower'):
        m.integrated_variance_reduction(xn[:3], box=np.stack([hi, lo]))
    with pytest.raises(ValueError, match='box must have shape'):
        m.integrated_variance_reduction(xn[:3], box=np.stack([lo, hi, hi]))
    with pytest.raises(ValueError, match='outputs'):
        m.integrated_variance_reduction(xn[:3], outputs=[3])
    with pytest.raises(ValueError, match='replicates must be 1 on the full path'):
        m.integrated_variance_reduction(xn[:3], replicates=2)
    with pytest.raises(ValueError, match='replicates must be an integer'):
        m.integrated_variance_reduction(xn[:3], replicates=0)


def test_c_abi_of_the_box_alc_entries():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() == 610
    for name in ('lcgp_box_alc', 'lcgp_box_alc_scratch_bytes'):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    assert len(_hip.SIGNATURES['lcgp_box_alc'][1]) == 22
    nb = C.c_size_t(0)
    # n = 1000 -> npad = 1024; 70 candidates -> slabs of 128 rows; per component npad^2 + 2 * 128 * npad + 3 * 128 doubles
    assert lib.lcgp_box_alc_scratch_bytes(_hip.F64, 1000, 3, 4, 70, C.byref(nb)) == 0
    assert nb.value == 8 * 4 * (1024 * 1024 + 2 * 128 * 1024 + 3 * 128)
    assert lib.lcgp_box_alc_scratch_bytes(_hip.F64, 1000, 3, 1, 2048, C.byref(nb)) == 0
    assert nb.value == 8 * (1024 * 1024 + 2 * 2048 * 1024 + 3 * 2048)
    assert lib.lcgp_box_alc_scratch_bytes(_hip.F32, 1000, 3, 4, 70, C.byref(nb)) < 0 and b'float64' in lib.lcgp_last_error()
    assert lib.lcgp_box_alc_scratch_bytes(_hip.F64, 1000, 127, 4, 70, C.byref(nb)) < 0 and b'd must be' in lib.lcgp_last_error()
    assert lib.lcgp_box_alc_scratch_bytes(_hip.F64, 0, 3, 4, 70, C.byref(nb)) < 0 and b'n < 1' in lib.lcgp_last_error()
    assert lib.lcgp_box_alc_scratch_bytes(_hip.F64, 1000, 3, 4, 0, C.byref(nb)) < 0 and b'n_cand' in lib.lcgp_last_error()
    assert lib.lcgp_box_alc_scratch_bytes(_hip.F64, 1000, 3, 4, 70, None) < 0 and b'NULL' in lib.lcgp_last_error()
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything

    def call(dtype=_hip.F64, kern=0, n=100, d=2, p=3, q=2, x=dummy, sr=None, theta=dummy, ws=dummy, k0=0, qg=2, box=dummy,
             n_cand=5, xc=dummy, match=None, r=1, scratch=dummy, out=dummy, stride=0):
        return lib.lcgp_box_alc(None, dtype, kern, n, d, p, q, x, sr, theta, ws, k0, qg, box, n_cand, xc, match, r, 1, scratch,
                                out, stride)

    assert call(dtype=_hip.F32) < 0 and b'float64' in lib.lcgp_last_error()
    assert call(kern=7) < 0 and b'kernel_id' in lib.lcgp_last_error()
    assert call(d=0) < 0 and b'd must be' in lib.lcgp_last_error()
    assert call(d=127) < 0 and b'd must be' in lib.lcgp_last_error()
    assert call(n=0) < 0 and b'n < 1' in lib.lcgp_last_error()
    assert call(n_cand=0) < 0 and b'n_cand' in lib.lcgp_last_error()
    assert call(n_cand=70000) < 0 and b'chunks' in lib.lcgp_last_error()
    assert call(q=0) < 0 and b'q_local' in lib.lcgp_last_error()
    assert call(k0=1) < 0 and b'k0 / q_group' in lib.lcgp_last_error()
    assert call(qg=0) < 0 and b'k0 / q_group' in lib.lcgp_last_error()
    assert call(r=0) < 0 and b'replicates' in lib.lcgp_last_error()
    assert call(stride=4) < 0 and b'out_stride' in lib.lcgp_last_error()
    for arg in ('x', 'theta', 'ws', 'box', 'xc', 'scratch', 'out'):
        assert call(**{arg: None}) < 0 and b'NULL' in lib.lcgp_last_error(), arg
