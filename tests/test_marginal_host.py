"""CPU tests of the box-averaged predictions (LCGP.predict_marginal / main_effects): the closed forms of tests/marginal_ref.py
against scipy quadrature, the restatement against a tensor Gauss-Legendre rule over its own pointwise posterior, the host
layer (argument checks, mask forms, boxes, NaN under the mask, the layout of main_effects, two gloo ranks against one) through
a numpy stand-in of HotPathEngine.predict_marginal_block, and the C entries of the library (tests/test_gpu_marginal.py runs the
same through liblcgp_hip.so on the GPU)."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.integrate import quad

from lcgp_amd import LCGP, synth
from lcgp_amd import dist as _dist
from oracle import lcgp_oracle as orc
from tests import marginal_ref as ref
from tests.test_predict_grad_host import LO, SPAN
from tests.test_predict_hess_host import HessOracleEngine, _model

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = ('matern32', 'se', 'matern52')


class MargOracleEngine(HessOracleEngine):
    """HessOracleEngine plus predict_marginal_block, in numpy float64 from tests/marginal_ref.py"""

    def predict_marginal_block(self, x0s, mask, box):
        x0s, mask, box = np.asarray(x0s, np.float64), np.asarray(mask, bool), np.asarray(box, np.float64)
        assert mask.shape == x0s.shape and box.shape == (2, self.d) and np.all(np.isfinite(x0s[~mask]))
        sr = np.ones(self.n) if self.sr is None else self.sr
        res = [ref.latent_marginal(x0s, mask, box, self.x, sr, th, low, z, self.kernel) for th, low, z, b in self._state]
        return torch.as_tensor(np.stack([[r[0] for r in res], [r[1] for r in res]]))


def patch_engine(model):
    """tests.test_predict_hess_host.patch_engine, installing MargOracleEngine"""
    def _make(dtype=None):
        rank, world = _dist.rank_world(model._group)
        model._local_ks = _dist.local_components(model.q, rank, world)
        if not model._local_ks:
            return None
        if model.submethod == 'rep':
            sr = np.sqrt(model.r.numpy().astype(float))
            yb = (model.ybar_s if model.rep_standardize_ybar else model.ybar).numpy()
            return MargOracleEngine(model.x_unique_s.numpy(), yb * sr[None, :], sr, len(model._local_ks),
                                    comp_ids=model._local_ks, q_total=model.q, kernel=model.kernel)
        return MargOracleEngine(model.x.numpy(), model.y.numpy(), None, len(model._local_ks),
                                comp_ids=model._local_ks, q_total=model.q, kernel=model.kernel)
    model._make_engine = _make
    model._engine = None
    model._invalidate()
    return model


def model_of(mode, kernel='matern32'):
    m, x = _model(mode, kernel)
    return patch_engine(m), x


# ---- the closed forms -------------------------------------------------------------------------------------------------
BOX = (0.2, 0.9)
QUAD_BAR = 1e-11


def _ells():
    """both ends of the model's length-scale bounds (the SoftClip of lLmb) and two values between them"""
    m, _ = _model('full')
    tr = m.lLmb.transform
    assert (tr.low, tr.high) == (1e-6, 1e4)
    return (float(tr.low), 0.05, 3.0, float(tr.high))


def _quad_scaled(kernel, a, b):
    """int_a^b kappa(|s|) ds with break points at the kink and where the factor has decayed.  The integral is taken in the
    scaled variable s = (t - x) / ell: in t itself the integrand at ell = 1e-6 varies over 1e-6 around x = O(1), where the
    spacing of doubles (1e-16) is 1e-10 of that scale, and quad then agrees with the closed form to 2e-11 only (measured;
    its own error estimate, 1e-14, does not see this)"""
    pts = [s for s in (0.0, 1.0, -1.0, 8.0, -8.0, 40.0, -40.0) if a < s < b]
    return quad(lambda s: ref.kappa(kernel, abs(s)), a, b, points=pts or None, epsabs=0.0, epsrel=1e-13, limit=400)


@pytest.mark.parametrize('kernel', KERNELS)
def test_single_and_double_average_against_quad(kernel):
    """I1 at x inside the box, on both edges, outside on both sides and three length scales outside; I2 from the 1-D form
    (2 / w^2) int_0^w (w - r) kappa(r / ell) dr.  Bar 1e-11 relative; where the value underflows (ell = 1e-6, x outside:
    e^-1e5) both are exactly 0.  Measured worst relative deviation over all x: 8.9e-16 / 5.9e-16 / 3.4e-16 / 4.4e-16
    (Matern-3/2), 3.5e-16 / 6.2e-15 / 2.2e-16 / 2.2e-16 (SE), 5.0e-15 / 7.3e-16 / 2.2e-16 / 2.2e-16 (Matern-5/2) at ell = 1e-6 /
    0.05 / 3 / 1e4; quad's own estimate is 1e-14 to 9e-14 of the value throughout, the extreme ell included."""
    lo, hi = BOX
    w = hi - lo
    for ell in _ells():
        worst = 0.0
        for x in (0.5, lo, hi, -0.1, 1.3, lo - 3.0 * ell if ell < 1.0 else 0.1):
            want, est = _quad_scaled(kernel, (lo - x) / ell, (hi - x) / ell)
            want, est = want * ell / w, est * ell / w
            got = float(ref.I1(kernel, x, lo, hi, ell))
            assert est <= 1e-12 * abs(want)
            assert abs(got - want) <= QUAD_BAR * abs(want), (ell, x, got, want)
            if want != 0.0:
                worst = max(worst, abs(got - want) / abs(want))
        a = w / ell
        pts = [s for s in (1.0, 8.0, 40.0) if s < a]
        want, est = quad(lambda s: (a - s) * ref.kappa(kernel, s), 0.0, a, points=pts or None, epsabs=0.0, epsrel=1e-13, limit=400)
        want, est = 2.0 * want / (a * a), 2.0 * est / (a * a)
        got = float(ref.I2(kernel, w, ell))
        print('closed forms', kernel, ell, 'I1 worst', worst, 'I2', abs(got - want) / want, 'quad estimate', est / want)
        assert est <= 1e-12 * want
        assert abs(got - want) <= QUAD_BAR * want, (ell, got, want)
        assert 0.0 < got <= 1.0


@pytest.mark.parametrize('kernel', ['matern32', 'matern52'])
def test_series_and_closed_forms_meet_at_the_switch(kernel):
    """below b = 1/2 F and G come from the series of kappa, above from the closed forms: both routes on both sides of the switch
    (closed-form G at 0.3: value 0.04 from terms of size 1, 25 ulp), and the leading terms for small b"""
    b = np.linspace(0.3, 0.7, 41)
    Fs, Gs = ref._series(kernel, b)
    Fc_, Gc = ref._closed(kernel, b)
    assert np.max(np.abs(Fs - Fc_) / Fc_) <= 1e-14 and np.max(np.abs(Gs - Gc) / Gc) <= 2e-14
    for b in (1e-3, 1e-6, 1e-9):
        lead = 0.5 if kernel == 'matern32' else 1.0 / 6.0
        assert abs(ref.F(kernel, b) / b - 1.0 + lead * b * b / 3.0) <= 1e-15 + b ** 3
        assert abs(ref.G(kernel, b) / (b * b) - 0.5 + lead * b * b / 4.0) <= 1e-15 + b ** 3
    np.testing.assert_allclose(ref.F(kernel, 800.0) + ref.Fc(kernel, 800.0), 2.0 if kernel == 'matern32' else 8.0 / 3.0, rtol=1e-15)


# ---- the restatement against a quadrature of its own pointwise posterior ---------------------------------------------------
# Gauss-Legendre nodes per integrated dimension, fixed here on the CPU so that the rule's deviation from the closed form is
# below 1e-8 of the largest entry, and the deviation measured with it: worst over both components, every kept dimension, mean
# and variance 1.50e-10, held here rounded up (the variance with dimension 1 kept, length scales 0.34 / 0.60 / 0.48).  12 nodes reach rounding
# (2.0e-15), which would leave the GPU test that takes ten times this figure as its bar nothing but rounding to compare.
GL_NODES = 8
CPU_QUAD_DEV = 1.6e-10


def quadrature_model():
    """n = 60, d = 3, SE, q = 2 by the recipe of the GPU tests' models (synth.make_full and the perturbed initial parameters of
    seed 81, so the length scales are those of the GPU test's n = 300 model up to the spread of the inputs): x, sr and per
    component (theta row, Cholesky factor, z) in numpy float64"""
    x, y = synth.make_full(81, 60, 3, 3, 2)
    m = patch_engine(LCGP(y=y, x=x, q=2, kernel='se'))
    m._set_flat(synth.param_points(81, orc.OracleLCGP(y=y, x=x, q=2).get_unconstrained())[1])
    eng = m._ensure_aux()
    return eng.x, np.ones(eng.n), [(th, low, z) for th, low, z, b in eng._state]


QUAD_BOX = np.array([[0.1, 0.25, 0.0], [0.9, 1.0, 0.8]])       # training inputs lie outside it on both sides
QUAD_KEEP = np.array([0.15, 0.5, 0.85])                        # the values of the kept dimension


def quadrature_of(pointwise, m, keep_dim):
    """mean and variance of the box average over the dimensions other than keep_dim by the tensor rule: w^T ghat(nodes) and
    w^T Sigma w, from pointwise(pts) -> (ghat (m), Sigma (m, m)) with Sigma the CONTINUOUS posterior covariance"""
    dims = [l for l in range(3) if l != keep_dim]
    nodes, wts = ref.tensor_rule(m, QUAD_BOX, dims)
    mean, var = [], []
    for v in QUAD_KEEP:
        pts = np.empty((len(wts), 3))
        pts[:, dims] = nodes
        pts[:, keep_dim] = v
        gh, S = pointwise(pts)
        mean.append(wts @ gh)
        var.append(wts @ S @ wts)
    return np.array(mean), np.array(var)


def test_restatement_equals_gauss_legendre_over_its_own_posterior():
    """two of three dimensions integrated (each pair) and all three, SE, both components: the closed form against w^T ghat(nodes)
    and w^T Sigma w with GL_NODES nodes per dimension, relative to the largest entry"""
    x, sr, comps = quadrature_model()
    worst = 0.0
    for th, low, z in comps:
        def pointwise(pts):
            S, X = ref.continuous_cov(pts, x, sr, th, low, 'se')
            return X @ z, S

        print('length scales', th[:3])
        for keep in range(3):
            x0s = np.full((3, 3), np.nan)
            x0s[:, keep] = QUAD_KEEP
            mask = np.ones((3, 3), bool)
            mask[:, keep] = False
            gh, gv = ref.latent_marginal(x0s, mask, QUAD_BOX, x, sr, th, low, z, 'se')
            assert np.all(gv > 0.0) and np.all(gv < th[3])
            for nodes in (12, GL_NODES):
                mean, var = quadrature_of(pointwise, nodes, keep)
                em, ev = np.max(np.abs(mean - gh)) / np.max(np.abs(gh)), np.max(np.abs(var - gv)) / np.max(np.abs(gv))
                print('gauss-legendre', keep, nodes, 'mean', em, 'var', ev)
            worst = max(worst, em, ev)
        # all three integrated: the Bayesian-quadrature mean of the surface over the box, and its variance
        nodes, wts = ref.tensor_rule(GL_NODES, QUAD_BOX, [0, 1, 2])
        gh, S = pointwise(nodes)
        got = ref.latent_marginal(np.full((1, 3), np.nan), np.ones((1, 3), bool), QUAD_BOX, x, sr, th, low, z, 'se')
        em, ev = abs(wts @ gh - got[0][0]) / abs(got[0][0]), abs(wts @ S @ wts - got[1][0]) / abs(got[1][0])
        print('gauss-legendre all', GL_NODES, 'mean', em, 'var', ev)
        worst = max(worst, em, ev)
    print('worst', worst)
    assert worst <= CPU_QUAD_DEV < 1e-8, worst


# ---- the host layer --------------------------------------------------------------------------------------------------------
CASES = [(mode, kernel) for mode in ('full', 'rep') for kernel in KERNELS]


@pytest.mark.parametrize('mode,kernel', CASES)
def test_predict_marginal_is_the_restatement_through_the_output_map(mode, kernel):
    m, x = model_of(mode, kernel)
    rng = np.random.default_rng(5)
    x0 = LO + SPAN * rng.uniform(0.05, 0.95, (9, 2))
    mask = np.array([[False, False], [True, False], [False, True], [True, True]] * 2 + [[True, False]])
    ypred, yconfvar = [t.numpy() for t in m.predict_marginal(x0, mask)]
    assert ypred.shape == (3, 9) and yconfvar.shape == (3, 9) and ypred.dtype == np.float64
    gh, gv = [t.numpy() for t in m.predict_marginal(x0, mask, latent=True)]
    assert gh.shape == (2, 9) and gv.shape == (2, 9)
    eng = m._ensure_aux()
    sr = np.ones(eng.n) if eng.sr is None else eng.sr
    x0s = m._standardise_x0(x0)[0]
    box = np.stack([np.zeros(2), np.ones(2)])                       # the default: the training inputs' bounding box
    want = [ref.latent_marginal(x0s, mask, box, eng.x, sr, th, low, z, kernel) for th, low, z, b in eng._state]
    np.testing.assert_array_equal(gh, np.stack([r[0] for r in want]))
    np.testing.assert_array_equal(gv, np.stack([r[1] for r in want]))
    W, _, scale, offset = m._output_map()
    np.testing.assert_allclose(ypred, (W.T @ gh) * scale[:, None] + offset[:, None], rtol=1e-14, atol=0)
    np.testing.assert_allclose(yconfvar, ((W ** 2).T @ gv) * (scale ** 2)[:, None], rtol=1e-14, atol=0)
    assert np.all(yconfvar > 0.0)
    # rows that integrate nothing are predict() at new inputs
    yp, _, ycv = [t.numpy() for t in m.predict(x0[[0, 4]])]
    np.testing.assert_allclose(ypred[:, [0, 4]], yp, rtol=1e-12, atol=0)
    np.testing.assert_allclose(yconfvar[:, [0, 4]], ycv, rtol=1e-10, atol=0)
    # averaging shrinks the variance of the latent components below the pointwise one at the same kept inputs
    pointwise = m.predict_marginal(x0, [], latent=True)[1].numpy()
    assert np.all(gv[:, mask.any(axis=1)] < pointwise[:, mask.any(axis=1)])


def test_mask_forms_boxes_and_ignored_columns():
    m, x = model_of('full', 'matern52')
    rng = np.random.default_rng(6)
    x0 = LO + SPAN * rng.uniform(0.0, 1.0, (7, 2))
    base = [t.numpy() for t in m.predict_marginal(x0, [1])]
    mask = np.zeros((7, 2), bool)
    mask[:, 1] = True
    for form in ((1,), np.array([1]), [1, 1], mask, torch.as_tensor(mask).numpy()):
        got = [t.numpy() for t in m.predict_marginal(x0, form)]
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
    # a scalar index, a tensor x0
    got = [t.numpy() for t in m.predict_marginal(torch.as_tensor(x0), 1)]
    assert np.array_equal(got[0], base[0])
    # values under the mask are ignored: NaN, inf, anything
    for junk in (np.nan, np.inf, -7.0):
        x1 = x0.copy()
        x1[:, 1] = junk
        got = [t.numpy() for t in m.predict_marginal(x1, [1])]
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), junk
    # the default box is the training inputs' bounding box
    xn = np.asarray(x)
    got = [t.numpy() for t in m.predict_marginal(x0, [1], box=np.stack([xn.min(axis=0), xn.max(axis=0)]))]
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
    # a sub-box changes the answer, and only through the integrated dimension: the box of a kept dimension is never used
    sub = np.stack([xn.min(axis=0) + 0.3 * SPAN, xn.min(axis=0) + 0.6 * SPAN])
    a = m.predict_marginal(x0, [1], box=sub)[0].numpy()
    assert not np.allclose(a, base[0], rtol=1e-6)
    sub2 = sub.copy()
    sub2[:, 0] = [xn[:, 0].min() - 5.0, xn[:, 0].max() + 11.0]
    assert np.array_equal(m.predict_marginal(x0, [1], box=sub2)[0].numpy(), a)
    # a narrow box around a value approaches the pointwise prediction there
    v = xn.min(axis=0) + 0.5 * SPAN
    narrow = np.stack([v - 1e-7 * SPAN, v + 1e-7 * SPAN])
    xp = x0.copy()
    xp[:, 1] = v[1]
    # (the box's ends are rounded to 1e-16, 1e-9 of its width 2e-7: the bar is 1e-7 of the largest entry, the truncation 1e-14)
    want = m.predict(xp)[0].numpy()
    np.testing.assert_allclose(m.predict_marginal(x0, [1], box=narrow)[0].numpy(), want, rtol=0, atol=1e-7 * np.max(np.abs(want)))


def test_predict_marginal_refuses_bad_arguments():
    m, x = model_of('full')
    x0 = LO + SPAN * np.random.default_rng(7).uniform(0.0, 1.0, (5, 2))
    with pytest.raises(ValueError, match='shape'):
        m.predict_marginal(x0[:, :1], [0])
    for bad in ([2], [-1], [0, 5]):
        with pytest.raises(ValueError, match='indices'):
            m.predict_marginal(x0, bad)
    with pytest.raises(ValueError, match='indices'):
        m.predict_marginal(x0, [0.5])
    with pytest.raises(ValueError, match='boolean'):
        m.predict_marginal(x0, np.zeros((4, 2), bool))
    xn = np.asarray(x)
    lo, hi = xn.min(axis=0), xn.max(axis=0)
    with pytest.raises(ValueError, match='box'):
        m.predict_marginal(x0, [0], box=np.stack([lo, hi, hi]))
    with pytest.raises(ValueError, match='upper > lower'):
        m.predict_marginal(x0, [0], box=np.stack([lo, [hi[0], lo[1]]]))            # degenerate in dimension 1
    with pytest.raises(ValueError, match='upper > lower'):
        m.predict_marginal(x0, [0], box=np.stack([hi, lo]))
    with pytest.raises(ValueError, match='upper > lower'):
        m.predict_marginal(x0, [0], box=np.stack([lo, [np.nan, hi[1]]]))
    x1 = x0.copy()
    x1[2, 1] = np.nan
    with pytest.raises(ValueError, match='kept'):
        m.predict_marginal(x1, [0])
    m.predict_marginal(x1, [1])                                                    # (under the mask: fine)
    with pytest.raises(ValueError, match='grid'):
        m.main_effects(grid=0)
    with pytest.raises(ValueError, match='outputs'):
        m.main_effects(outputs=[3])


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_main_effects_layout(mode):
    m, x = model_of(mode, 'se')
    xn = np.asarray(x)
    lo, hi = xn.min(axis=0), xn.max(axis=0)
    G = 5
    me = m.main_effects(grid=G)
    assert me.grid.shape == (2, G) and me.mean.shape == (3, 2, G) and me.var.shape == (3, 2, G)
    assert me.overall.shape == (3,) and me.overall_var.shape == (3,) and me.effect.shape == (3, 2, G)
    np.testing.assert_allclose(me.grid.numpy(), np.stack([np.linspace(lo[l], hi[l], G) for l in range(2)]), rtol=1e-15)
    np.testing.assert_array_equal(me.effect.numpy(), me.mean.numpy() - me.overall.numpy()[:, None, None])
    # row (l, g) keeps only dimension l at grid value g; the last row integrates everything
    for l in range(2):
        x0 = np.full((G, 2), np.nan)
        x0[:, l] = me.grid.numpy()[l]
        yp, ycv = m.predict_marginal(x0, [1 - l])                  # (another batch size: the host products round differently)
        np.testing.assert_allclose(me.mean.numpy()[:, l], yp.numpy(), rtol=1e-13)
        np.testing.assert_allclose(me.var.numpy()[:, l], ycv.numpy(), rtol=1e-13)
    yp, ycv = m.predict_marginal(np.full((1, 2), np.nan), [0, 1])
    np.testing.assert_allclose(me.overall.numpy(), yp.numpy()[:, 0], rtol=1e-13)
    np.testing.assert_allclose(me.overall_var.numpy(), ycv.numpy()[:, 0], rtol=1e-13)
    # the same rows in one call: to the bit
    x0 = np.full((2 * G + 1, 2), np.nan)
    mask = np.ones((2 * G + 1, 2), bool)
    for l in range(2):
        x0[l * G:(l + 1) * G, l] = me.grid.numpy()[l]
        mask[l * G:(l + 1) * G, l] = False
    yp, ycv = m.predict_marginal(x0, mask)
    np.testing.assert_array_equal(me.mean.numpy(), yp.numpy()[:, :-1].reshape(3, 2, G))
    np.testing.assert_array_equal(me.var.numpy(), ycv.numpy()[:, :-1].reshape(3, 2, G))
    np.testing.assert_array_equal(me.overall.numpy(), yp.numpy()[:, -1])
    np.testing.assert_array_equal(me.overall_var.numpy(), ycv.numpy()[:, -1])
    assert np.all(me.overall_var.numpy() > 0.0) and np.all(me.overall_var.numpy() < np.min(me.var.numpy(), axis=(1, 2)))
    # the overall mean is the average of each main effect over its own input (Gauss-Legendre in one dimension)
    t, w = ref.gauss_legendre(24, 0.0, 1.0)
    for l in range(2):
        x0 = np.full((24, 2), np.nan)
        x0[:, l] = lo[l] + (hi[l] - lo[l]) * t
        yp = m.predict_marginal(x0, [1 - l])[0].numpy()
        np.testing.assert_allclose(yp @ w, me.overall.numpy(), rtol=1e-9)
    # outputs select rows; a sub-box moves the grid
    sel = m.main_effects(grid=G, outputs=[2, 0])
    np.testing.assert_array_equal(sel.mean.numpy(), me.mean.numpy()[[2, 0]])
    np.testing.assert_array_equal(sel.overall_var.numpy(), me.overall_var.numpy()[[2, 0]])
    sub = np.stack([lo + 0.25 * (hi - lo), lo + 0.5 * (hi - lo)])
    ms = m.main_effects(grid=3, box=sub)
    np.testing.assert_allclose(ms.grid.numpy(), np.stack([np.linspace(sub[0, l], sub[1, l], 3) for l in range(2)]), rtol=1e-15)
    assert 'MainEffects' in repr(ms)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_gather_what_one_rank_computes():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_marginal_host_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


def test_c_abi_of_the_marginal_entry():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() == 610
    for name in ('lcgp_predict_marginal', 'lcgp_predict_marginal_scratch_bytes'):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    assert len(_hip.SIGNATURES['lcgp_predict_marginal'][1]) == len(_hip.SIGNATURES['lcgp_predict'][1]) + 1
    nb, npred = C.c_size_t(0), C.c_size_t(0)
    # n = 1000 -> npad 1024; n0 = 100 -> 128 rows; q = 2: X and U as lcgp_predict, then the table and the double averages
    assert lib.lcgp_predict_marginal_scratch_bytes(0, 1000, 3, 2, 100, C.byref(nb)) == 0
    assert lib.lcgp_predict_scratch_bytes(0, 1000, 2, 100, C.byref(npred)) == 0
    assert nb.value == npred.value + 8 * 2 * 3 * (1024 + 1) == 2 * 2 * 128 * 1024 * 8 + 8 * 2 * 3 * 1025
    assert lib.lcgp_predict_marginal_scratch_bytes(1, 1000, 5, 2, 50, C.byref(nb)) == 0
    assert nb.value == 2 * 2 * 64 * 1024 * 4 + 8 * 2 * 5 * 1025
    assert lib.lcgp_predict_marginal_scratch_bytes(2, 1000, 3, 2, 100, C.byref(nb)) < 0
    assert b'dtype' in lib.lcgp_last_error()
    assert lib.lcgp_predict_marginal_scratch_bytes(0, 1000, 127, 2, 100, C.byref(nb)) < 0
    assert b'd must be' in lib.lcgp_last_error()
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything
    head = (dummy, None, dummy, dummy)                              # x, sr, theta, workspace

    def call(dtype=0, kern=0, d=2, n0=10, x0=dummy, mask=dummy, box=dummy, scratch=dummy, gh=dummy, gv=dummy, stride=0):
        return lib.lcgp_predict_marginal(None, dtype, kern, 100, d, 3, 1, *head, n0, x0, mask, box, scratch, gh, gv, stride)

    assert call(dtype=2) < 0 and b'dtype' in lib.lcgp_last_error()
    assert call(kern=7) < 0 and b'kernel_id' in lib.lcgp_last_error()
    assert call(d=127) < 0 and b'd must be' in lib.lcgp_last_error()
    assert call(n0=0) < 0 and b'n0' in lib.lcgp_last_error()
    for arg in ('x0', 'mask', 'box', 'scratch', 'gh', 'gv'):
        assert call(**{arg: None}) < 0 and b'NULL' in lib.lcgp_last_error(), arg
    assert call(stride=5) < 0 and b'out_stride' in lib.lcgp_last_error()
