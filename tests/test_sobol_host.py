"""CPU tests of the closed-form Sobol indices (LCGP.sobol_indices): the pair integral of tests/sobol_ref.py against piecewise
Gauss-Legendre quadrature, its limit and symmetry, the restated assembly against a tensor quadrature of its own surface, the
host layer (shapes, outputs=, latent=, argument checks, NaN for a constant output, two gloo ranks against one) through a numpy
stand-in of HotPathEngine.sobol_pairs, and the C entries of the library (tests/test_gpu_sobol.py runs the same through
liblcgp_hip.so on the GPU)."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from lcgp_amd import dist as _dist
from tests import marginal_ref as mref
from tests import sobol_ref as ref
from tests.test_marginal_host import MargOracleEngine
from tests.test_predict_hess_host import _model

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = ('matern32', 'se', 'matern52')


class SobolOracleEngine(MargOracleEngine):
    """MargOracleEngine plus sobol_pairs, in numpy float64 from tests/sobol_ref.py"""

    def sobol_pairs(self, x, w, ell, box, pairs):
        x, w, ell, box = (np.asarray(a, np.float64) for a in (x, w, ell, box))
        n, d = x.shape
        assert w.shape == (w.shape[0], n) and ell.shape == (w.shape[0], d) and box.shape == (2, d)
        D, means = np.zeros((len(pairs), 2 * d + 1)), np.zeros(len(pairs))
        for r, (k, kp) in enumerate(np.asarray(pairs)):
            D[r], m, _ = ref.pair_sums(self.kernel, x, w[k], ell[k], w[kp], ell[kp], box)
            means[r] = m[0] if k == kp else 0.0
        return D, means


def patch_engine(model):
    """tests.test_marginal_host.patch_engine, installing SobolOracleEngine"""
    def _make(dtype=None):
        rank, world = _dist.rank_world(model._group)
        model._local_ks = _dist.local_components(model.q, rank, world)
        if not model._local_ks:
            return None
        if model.submethod == 'rep':
            sr = np.sqrt(model.r.numpy().astype(float))
            yb = (model.ybar_s if model.rep_standardize_ybar else model.ybar).numpy()
            return SobolOracleEngine(model.x_unique_s.numpy(), yb * sr[None, :], sr, len(model._local_ks),
                                     comp_ids=model._local_ks, q_total=model.q, kernel=model.kernel)
        return SobolOracleEngine(model.x.numpy(), model.y.numpy(), None, len(model._local_ks),
                                 comp_ids=model._local_ks, q_total=model.q, kernel=model.kernel)
    model._make_engine = _make
    model._engine = None
    model._invalidate()
    return model


def model_of(mode, kernel='matern32'):
    m, x = _model(mode, kernel)
    return patch_engine(m), x


# ---- the pair integral -------------------------------------------------------------------------------------------------------
LO, HI = 0.0, 1.0
# centres: equal, both inside (both orders), on the box's ends, one outside on either side, both outside on opposite sides, both
# outside on the same side.  The last two sit 0.03 and 0.01 from the box: at a = 0.01 box widths an SE factor ten or thirty
# length scales out is e^-50 .. e^-450, where the rounding of the scaled distance z itself moves the value by z^2 eps = 1e-13 per
# operation -- a property of the inputs in double precision, not of either way of integrating
CENTRES = ((0.3, 0.3), (0.2, 0.7), (0.9, 0.1), (0.0, 1.0), (-0.2, 0.5), (0.4, 1.3), (-0.3, 1.2), (-0.03, -0.01), (1.01, 1.03))


def _scales():
    """(a, b): a in {0.01, 1, 30} box widths with b = a, a (1 + 1e-12), a (1 + 1e-6), 2 a, and b across the other two values"""
    out = []
    for a in (0.01, 1.0, 30.0):
        out += [(a, a), (a, a * (1.0 + 1e-12)), (a, a * (1.0 + 1e-6)), (a, 2.0 * a)]
        out += [(a, b) for b in (0.01, 1.0, 30.0) if b != a]
    return out


@pytest.mark.parametrize('kernel', KERNELS)
def test_pair_integral_against_piecewise_gauss_legendre(kernel):
    """every (centres, length scales) of the fixed table: 40 nodes per piece, pieces split at the centres and no longer than
    2 min(a, b).  Bar 1e-12 relative (the recipe stays within 2e-14 of 40-digit quadrature; the margin covers the rule's own
    rounding: up to 4000 positive terms per integral)"""
    worst = 0.0
    for a, b in _scales():
        for u, v in CENTRES:
            t, wt = ref.piecewise_gauss_legendre(40, LO, HI, (u, v), 2.0 * min(a, b))
            want = np.sum(wt * mref.kappa(kernel, np.abs(t - u) / a) * mref.kappa(kernel, np.abs(t - v) / b))
            got = float(ref.pair_integral(kernel, LO, HI, u, a, v, b))
            if want == 0.0:                 # (SE, centres fifty and more length scales apart: e^-1250 underflows on both sides)
                assert 0.0 <= got < 1e-300 and kernel == 'se' and min(a, b) == 0.01, (kernel, a, b, u, v, got)
                continue
            err = abs(got - want) / want
            worst = max(worst, err)
            assert err <= 1e-12, (kernel, a, b, u, v, got, want, err)
    print('pair integral against quadrature', kernel, 'worst relative deviation', worst)


@pytest.mark.parametrize('kernel', KERNELS)
def test_pair_integral_tends_to_the_single_average(kernel):
    """b -> infinity: the second factor is 1 - O((w / b)^2) over the box, so J -> I1 of the first; at b = 1e9 box widths
    the difference is below rounding"""
    for a in (0.05, 1.0, 30.0):
        for u in (0.3, 0.0, -0.2, 1.4):
            for v in (0.5, -3.0):
                got = float(ref.pair_integral(kernel, LO, HI, u, a, v, 1e9))
                want = float(mref.I1(kernel, u, LO, HI, a))
                assert abs(got - want) <= 1e-13 * want, (kernel, a, u, v, got, want)
                got = float(ref.pair_integral(kernel, LO, HI, v, 1e9, u, a))
                assert abs(got - want) <= 1e-13 * want, (kernel, a, u, v, got, want)


@pytest.mark.parametrize('kernel', KERNELS)
def test_pair_integral_is_symmetric_in_its_two_factors(kernel):
    rng = np.random.default_rng(11)
    u, v = rng.uniform(-0.3, 1.3, (2, 200))
    a, b = 10.0 ** rng.uniform(-2.0, 1.5, (2, 200))
    b[:40] = a[:40]
    np.testing.assert_array_equal(ref.pair_integral(kernel, 0.2, 0.9, u, a, v, b), ref.pair_integral(kernel, 0.2, 0.9, v, b, u, a))


def test_moments_series_and_recurrence_meet_at_the_switch():
    """both routes on both sides of gamma L = 4, and the limit gamma = 0: m_n = L^(n + 1) / (n + 1)"""
    L = 0.7
    for x in (3.999999, 4.0, 4.000001):
        got = ref.moments(x / L, L, 4)
        t, wt = mref.gauss_legendre(40, 0.0, L)
        for n in range(5):
            want = L * np.sum(wt * t ** n * np.exp(-x / L * t))
            assert abs(got[n] - want) <= 1e-13 * want, (x, n)
    np.testing.assert_allclose(ref.moments(0.0, L, 4), [L ** (n + 1) / (n + 1) for n in range(5)], rtol=1e-15)
    np.testing.assert_array_equal(ref.moments(3.0, 0.0, 4), np.zeros(5))


def test_assembly_against_tensor_quadrature_of_its_own_surface():
    """two Matern-3/2 components at d = 2, n = 9: the mean, V, V_0 and V_1 of a mixed output from pair_sums against a piecewise
    tensor Gauss-Legendre rule (12 nodes per piece, pieces split at the training coordinates) over the surface itself"""
    rng = np.random.default_rng(3)
    n, d = 9, 2
    x = rng.uniform(0.0, 1.0, (n, d))
    box = np.array([[0.1, 0.0], [0.9, 0.8]])
    ell = np.array([[0.3, 0.7], [1.1, 0.2]])
    w = rng.standard_normal((2, n))
    mix = np.array([0.8, -1.3])
    D = np.zeros((2, 2, 2 * d + 1))
    means = np.zeros(2)
    for k in range(2):
        for kp in range(k, 2):
            D[k, kp], m, _ = ref.pair_sums('matern32', x, w[k], ell[k], w[kp], ell[kp], box)
            D[kp, k] = D[k, kp]
            if k == kp:
                means[k] = m[0]
    got = ref.indices(D, means, mix[:, None], np.ones(1), np.zeros(1))
    rules = [ref.piecewise_gauss_legendre(12, box[0][l], box[1][l], x[:, l]) for l in range(d)]

    def surface(t0, t1):
        f = 0.0
        for k in range(2):
            f = f + mix[k] * np.einsum('i,ia,ib->ab', w[k], mref.kappa('matern32', np.abs(t0[None, :] - x[:, :1]) / ell[k, 0]),
                                       mref.kappa('matern32', np.abs(t1[None, :] - x[:, 1:]) / ell[k, 1]))
        return f

    f = surface(rules[0][0], rules[1][0])
    w0, w1 = rules[0][1], rules[1][1]
    mean = w0 @ f @ w1
    V = w0 @ (f - mean) ** 2 @ w1
    V0 = w0 @ (f @ w1 - mean) ** 2
    V1 = ((w0 @ f) - mean) ** 2 @ w1
    scale = abs(mean) ** 2 + V
    assert abs(got['mean'][0] - mean) <= 1e-13 * abs(mean)
    for name, a, b in (('V', got['variance'][0], V), ('V_0', got['first_variance'][0, 0], V0), ('V_1', got['first_variance'][0, 1], V1),
                       ('V_~0', got['closed_variance'][0, 0], V1), ('V_~1', got['closed_variance'][0, 1], V0)):
        print('assembly', name, abs(a - b) / scale)
        assert abs(a - b) <= 1e-13 * scale, (name, a, b)


# ---- the host layer ----------------------------------------------------------------------------------------------------------
def _direct(m, box=None):
    """ref.indices from the stand-in's own state: what sobol_indices must assemble"""
    eng = m._ensure_aux()
    d, q = eng.d, int(m.q)
    sr = np.ones(eng.n) if eng.sr is None else eng.sr
    th = np.stack([s[0] for s in eng._state])
    w = np.stack([t[d] * (1.0 - t[d + 1] / (1.0 + t[d + 1])) * sr * s[2] for t, s in zip(th, eng._state)])
    bs = np.stack([np.zeros(d), np.ones(d)]) if box is None else m._marginal_box(box)
    D, means = np.zeros((q, q, 2 * d + 1)), np.zeros(q)
    for k in range(q):
        for kp in range(k, q):
            D[k, kp], mm, _ = ref.pair_sums(m.kernel, eng.x, w[k], th[k, :d], w[kp], th[kp, :d], bs)
            D[kp, k] = D[k, kp]
            if k == kp:
                means[k] = mm[0]
    W, _, scale, offset = m._output_map()
    return ref.indices(D, means, W, scale, offset), D, means


@pytest.mark.parametrize('mode,kernel', [(mode, kernel) for mode in ('full', 'rep') for kernel in KERNELS])
def test_sobol_indices_assemble_the_pair_sums(mode, kernel):
    m, x = model_of(mode, kernel)
    s = m.sobol_indices()
    assert 'SobolIndices' in repr(s)
    for name in ('first', 'total', 'first_variance', 'closed_variance'):
        assert getattr(s, name).shape == (3, 2) and getattr(s, name).dtype.is_floating_point
    assert s.variance.shape == (3,) and s.mean.shape == (3,)
    want, D, means = _direct(m)
    for name in ('first', 'total', 'variance', 'mean', 'first_variance', 'closed_variance'):
        np.testing.assert_allclose(getattr(s, name).numpy(), want[name], rtol=1e-13, atol=0, err_msg=name)
    first, total = s.first.numpy(), s.total.numpy()
    assert np.all(first >= -1e-10) and np.all(first <= total + 1e-10) and np.all(first.sum(axis=1) <= 1.0 + 1e-10)
    assert np.all(s.variance.numpy() > 0.0)
    # d = 2: what the two first-order terms leave is the one interaction, which both totals contain
    np.testing.assert_allclose(total[:, 0] - first[:, 0], total[:, 1] - first[:, 1], rtol=0, atol=1e-10)
    # the mean is main_effects().overall, the first-order variance that of the main effect's curve (piecewise Gauss-Legendre)
    np.testing.assert_allclose(s.mean.numpy(), m.main_effects(grid=2).overall.numpy(), rtol=1e-12)
    xn = np.asarray(x)
    lo, hi = xn.min(axis=0), xn.max(axis=0)
    for l in range(2):
        t, wt = ref.piecewise_gauss_legendre(8, lo[l], hi[l], xn[:, l])
        x0 = np.full((len(t), 2), np.nan)
        x0[:, l] = t
        curve = m.predict_marginal(x0, [1 - l])[0].numpy()
        vl = ((curve - (curve @ wt)[:, None]) ** 2) @ wt
        np.testing.assert_allclose(s.first_variance.numpy()[:, l], vl, rtol=0, atol=1e-9 * np.max(s.variance.numpy()))
    # outputs select rows, in the order given
    sel = m.sobol_indices(outputs=[2, 0])
    for name in ('first', 'total', 'variance', 'mean', 'first_variance', 'closed_variance'):
        np.testing.assert_array_equal(getattr(sel, name).numpy(), getattr(s, name).numpy()[[2, 0]])
    # latent: the components themselves, from the pairs k = k'
    lat = m.sobol_indices(latent=True)
    assert lat.first.shape == (2, 2) and lat.variance.shape == (2,)
    np.testing.assert_allclose(lat.variance.numpy(), D[[0, 1], [0, 1], 4], rtol=1e-14)
    np.testing.assert_allclose(lat.first.numpy(), D[[0, 1], [0, 1], :2] / D[[0, 1], [0, 1], 4:5], rtol=1e-14)
    np.testing.assert_allclose(lat.mean.numpy(), means, rtol=1e-14)
    assert m.sobol_indices(latent=True, outputs=1).first.shape == (1, 2)
    # a sub-box changes the answer; the default box is the training inputs' bounding box
    same = m.sobol_indices(box=np.stack([lo, hi]))
    np.testing.assert_allclose(same.first.numpy(), first, rtol=1e-12)
    sub = np.stack([lo + 0.3 * (hi - lo), lo + 0.6 * (hi - lo)])
    got = m.sobol_indices(box=sub)
    np.testing.assert_allclose(got.first.numpy(), _direct(m, sub)[0]['first'], rtol=1e-12)
    assert not np.allclose(got.first.numpy(), first, rtol=1e-3)


def test_sobol_indices_refuses_bad_arguments():
    m, x = model_of('full')
    xn = np.asarray(x)
    lo, hi = xn.min(axis=0), xn.max(axis=0)
    with pytest.raises(ValueError, match='box'):
        m.sobol_indices(box=np.stack([lo, hi, hi]))
    with pytest.raises(ValueError, match='upper > lower'):
        m.sobol_indices(box=np.stack([hi, lo]))
    with pytest.raises(ValueError, match='upper > lower'):
        m.sobol_indices(box=np.stack([lo, [np.nan, hi[1]]]))
    for bad in ([3], [-1], [0, 5]):
        with pytest.raises(ValueError, match='outputs'):
            m.sobol_indices(outputs=bad)
    with pytest.raises(ValueError, match='outputs'):
        m.sobol_indices(outputs=[2], latent=True)          # (q = 2 components)


def test_a_constant_output_has_nan_indices():
    """an output no component feeds is constant over the box: V is exactly 0 and its indices are NaN, the others stay finite"""
    m, x = model_of('full', 'se')
    m.phi[1, :] = 0.0
    m._invalidate()
    s = m.sobol_indices()
    assert s.variance.numpy()[1] == 0.0 and np.all(s.first_variance.numpy()[1] == 0.0)
    assert np.all(np.isnan(s.first.numpy()[1])) and np.all(np.isnan(s.total.numpy()[1]))
    assert np.all(np.isfinite(s.first.numpy()[[0, 2]])) and np.all(np.isfinite(s.total.numpy()[[0, 2]]))
    assert np.isfinite(s.mean.numpy()[1])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_equal_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_sobol_host_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


def test_c_abi_of_the_sobol_entry():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() == 610
    for name in ('lcgp_sobol_pairs', 'lcgp_sobol_scratch_bytes'):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    nb = C.c_size_t(0)
    # n = 1000 -> 16 x 16 tiles; the table, the means, the tile sums of min(npairs, 64) pairs
    assert lib.lcgp_sobol_scratch_bytes(1000, 3, 4, 10, C.byref(nb)) == 0
    assert nb.value == 8 * (4 * 3 * 1000 + 4 + 10 * 256 * 7)
    assert lib.lcgp_sobol_scratch_bytes(1000, 3, 12, 78, C.byref(nb)) == 0
    assert nb.value == 8 * (12 * 3 * 1000 + 12 + 64 * 256 * 7)
    assert lib.lcgp_sobol_scratch_bytes(1000, 127, 4, 10, C.byref(nb)) < 0 and b'd must be' in lib.lcgp_last_error()
    assert lib.lcgp_sobol_scratch_bytes(0, 3, 4, 10, C.byref(nb)) < 0 and b'n < 1' in lib.lcgp_last_error()
    assert lib.lcgp_sobol_scratch_bytes(1000, 3, 4, 0, C.byref(nb)) < 0 and b'npairs' in lib.lcgp_last_error()
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything
    good = (C.c_int * 4)(0, 0, 0, 1)

    def call(kern=0, n=100, d=2, q=2, x=dummy, w=dummy, ell=dummy, box=dummy, pairs=good, npairs=2, scratch=dummy, out=dummy):
        return lib.lcgp_sobol_pairs(None, kern, n, d, q, x, w, ell, box, pairs, npairs, scratch, out)

    assert call(kern=7) < 0 and b'kernel_id' in lib.lcgp_last_error()
    assert call(d=0) < 0 and b'd must be' in lib.lcgp_last_error()
    assert call(q=0) < 0 and b'q_all' in lib.lcgp_last_error()
    for arg in ('x', 'w', 'ell', 'box', 'pairs', 'scratch', 'out'):
        assert call(**{arg: None}) < 0 and b'NULL' in lib.lcgp_last_error(), arg
    assert call(pairs=(C.c_int * 4)(0, 0, 0, 2)) < 0 and b'pairs' in lib.lcgp_last_error()
    assert call(pairs=(C.c_int * 4)(0, -1, 0, 1)) < 0 and b'pairs' in lib.lcgp_last_error()
