"""CPU tests of the posterior covariance of the gradient and the active-subspace matrix (LCGP.predict_grad_cov /
active_subspace): the closed form of tests/grad_cov_ref.py against its own independent stencil, the host layer (unpacking,
output map, weights, eigen-decomposition) through a numpy stand-in of HotPathEngine.grad_cov_block, and the C entries of the
library (tests/test_gpu_grad_cov.py runs the same through liblcgp_hip.so on the GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

from lcgp_amd import LCGP, synth
from lcgp_amd import dist as _dist
from tests import grad_cov_ref as ref
from tests.test_predict_grad_host import LO, SPAN
from tests.test_predict_hess_host import HessOracleEngine, _model, assert_clear_of_kinks, pack_lower


class GradCovOracleEngine(HessOracleEngine):
    """HessOracleEngine plus grad_cov_block, in numpy float64 from tests/grad_cov_ref.py"""

    def grad_cov_block(self, x0s, w=None, per_point=True):
        x0s = np.asarray(x0s, np.float64)
        sr = np.ones(self.n) if self.sr is None else self.sr
        dghat = np.stack([ref.latent_mean_grad(x0s, self.x, sr, th, z, self.kernel) for th, low, z, b in self._state])
        gamma = np.stack([pack_lower(ref.latent_grad_cov(x0s, self.x, sr, th, low, self.kernel)) for th, low, z, b in self._state])
        M = None if w is None else torch.as_tensor(np.einsum('i,kie->ke', np.asarray(w, np.float64), gamma))
        return torch.as_tensor(dghat), (torch.as_tensor(gamma) if per_point else None), M


def patch_engine(model):
    """tests.test_predict_hess_host.patch_engine, installing GradCovOracleEngine"""
    def _make(dtype=None):
        rank, world = _dist.rank_world(model._group)
        model._local_ks = _dist.local_components(model.q, rank, world)
        if not model._local_ks:
            return None
        if model.submethod == 'rep':
            sr = np.sqrt(model.r.numpy().astype(float))
            yb = (model.ybar_s if model.rep_standardize_ybar else model.ybar).numpy()
            return GradCovOracleEngine(model.x_unique_s.numpy(), yb * sr[None, :], sr, len(model._local_ks),
                                       comp_ids=model._local_ks, q_total=model.q, kernel=model.kernel)
        return GradCovOracleEngine(model.x.numpy(), model.y.numpy(), None, len(model._local_ks),
                                   comp_ids=model._local_ks, q_total=model.q, kernel=model.kernel)
    model._make_engine = _make
    model._engine = None
    model._invalidate()
    return model


def model_of(mode, kernel='matern32'):
    m, x = _model(mode, kernel)
    return patch_engine(m), x


CASES = [(mode, kernel) for mode in ('full', 'rep') for kernel in ('matern32', 'se', 'matern52')]
H = 1e-4                                                           # of the standardised range
# 4 x the largest difference measured below (relative to the largest entry of Gamma), per kernel
STENCIL_BAR = {'matern32': 4 * 7.29e-4, 'se': 4 * 2.12e-7, 'matern52': 4 * 2.39e-7}


def _state(m):
    """(engine, sr) of the model's stand-in at the current parameters"""
    eng = m._ensure_aux()
    return eng, (np.ones(eng.n) if eng.sr is None else eng.sr)


@pytest.mark.parametrize('mode,kernel', CASES)
def test_closed_form_equals_the_stencil_of_the_posterior_covariance_function(mode, kernel):
    """The two routes of tests/grad_cov_ref.py agree: the closed form and the mixed difference of Sigma(x, x') at distinct
    points, h = 1e-4 of the standardised range, points at least two steps away from every training coordinate.  The stencil
    truncates at O(h) for Matern-3/2 (the |a|^3 term of the 1-D factor) and at O(h^2) for the other two.
    Measured max |closed - stencil| / max |closed| over full / rep and both components: Matern-3/2 7.29e-4, SE 2.12e-7,
    Matern-5/2 2.39e-7;
    the bars are 4 x that."""
    m, x = model_of(mode, kernel)
    eng, sr = _state(m)
    x0s = np.random.default_rng(4).uniform(0.05, 0.95, (11, 2))
    assert_clear_of_kinks(x0s, eng.x, 2 * H * np.ones(2))           # (the stencil reaches 2 h)
    for th, low, z, b in eng._state:
        closed = ref.latent_grad_cov(x0s, eng.x, sr, th, low, kernel)
        fd = ref.stencil_grad_cov(x0s, eng.x, sr, th, low, kernel, H)
        err = np.max(np.abs(closed - fd)) / np.max(np.abs(closed))
        print('stencil', mode, kernel, err)
        assert err <= STENCIL_BAR[kernel], err


@pytest.mark.parametrize('mode,kernel', CASES)
def test_predict_grad_cov_is_the_restatement_through_the_output_map(mode, kernel):
    m, x = model_of(mode, kernel)
    x0 = LO + SPAN * np.random.default_rng(5).uniform(0.05, 0.95, (9, 2))
    cov = m.predict_grad_cov(x0).numpy()
    assert cov.shape == (3, 9, 2, 2) and cov.dtype == np.float64
    assert np.array_equal(cov, np.swapaxes(cov, -1, -2))            # exactly symmetric
    eng, sr = _state(m)
    x0s, _ = m._standardise_x0(x0)
    G = np.stack([ref.latent_grad_cov(x0s, eng.x, sr, th, low, kernel) for th, low, z, b in eng._state])
    lat = m.predict_grad_cov(x0, latent=True).numpy()
    assert lat.shape == (2, 9, 2, 2)
    np.testing.assert_allclose(lat, G, rtol=1e-12, atol=1e-12 * np.max(np.abs(G)))
    W, _, scale, _ = m._output_map()
    rng = (m.x_max - m.x_min).numpy().reshape(-1)                   # the standardisation's range, not SPAN itself
    want = np.zeros_like(cov)
    for a in range(3):
        for k in range(2):
            want[a] += scale[a] ** 2 * W[k, a] ** 2 * G[k] / (rng[:, None] * rng[None, :])
    np.testing.assert_allclose(cov, want, rtol=1e-12, atol=1e-12 * np.max(np.abs(want)))
    np.testing.assert_array_equal(m.dghat.numpy(), m._latent_predict_grad(x0)[2])
    # positive semi-definite, and so is what the data took away from the prior
    d = 2
    for k, (th, low, z, b) in enumerate(eng._state):
        c_zero = th[d] * (1.0 - th[d + 1] / (1.0 + th[d + 1]))
        prior = np.diag(c_zero * ref.KAPPA[kernel] / th[:d] ** 2)
        for i in range(9):
            ev = np.linalg.eigvalsh(lat[k, i])
            assert ev[0] >= -1e-12 * ev[-1], (k, i, ev)
            gone = np.linalg.eigvalsh(prior - lat[k, i])
            assert gone[0] >= -1e-12 * np.max(np.diag(prior)), (k, i, gone)
    for a in range(3):
        for i in range(9):
            ev = np.linalg.eigvalsh(cov[a, i])
            assert ev[0] >= -1e-12 * ev[-1], (a, i, ev)


def _assembled(m, x_ref, w, outputs):
    """sum_i w_i (grad ypred grad ypred^T + predict_grad_cov) from the two per-point queries"""
    g = m.predict_grad(x_ref)[0].numpy()[outputs]
    cov = m.predict_grad_cov(x_ref).numpy()[outputs]
    mean_part = np.einsum('i,ail,aim->alm', w, g, g)
    cov_part = np.einsum('i,ailm->alm', w, cov)
    return mean_part, cov_part


@pytest.mark.parametrize('mode,kernel', CASES)
def test_active_subspace_is_the_weighted_sum_of_the_per_point_queries(mode, kernel):
    m, x = model_of(mode, kernel)
    rng = np.random.default_rng(6)
    x_ref = LO + SPAN * rng.uniform(0.0, 1.0, (37, 2))
    w = rng.uniform(0.0, 2.0, 37)
    w[3] = 0.0
    res = m.active_subspace(x_ref, weights=w)
    mat = res.matrix.numpy()
    assert mat.shape == (3, 2, 2) and res.activity.shape == (3, 2) and res.eigenvalues.shape == (3, 2)
    assert res.eigenvectors.shape == (3, 2, 2)
    np.testing.assert_array_equal(mat, res.mean_part.numpy() + res.cov_part.numpy())
    np.testing.assert_array_equal(mat, np.swapaxes(mat, -1, -2))
    mean_part, cov_part = _assembled(m, x_ref, w / w.sum(), [0, 1, 2])
    tol = 1e-12 * np.max(np.abs(mat))
    np.testing.assert_allclose(res.mean_part.numpy(), mean_part, rtol=0, atol=tol)
    np.testing.assert_allclose(res.cov_part.numpy(), cov_part, rtol=0, atol=tol)
    np.testing.assert_allclose(mat, mean_part + cov_part, rtol=0, atol=tol)
    np.testing.assert_array_equal(res.activity.numpy(), np.diagonal(mat, axis1=-2, axis2=-1))
    lam, V = res.eigenvalues.numpy(), res.eigenvectors.numpy()
    assert np.all(np.diff(lam, axis=1) <= 0)                        # descending
    np.testing.assert_allclose(np.einsum('alk,ak,amk->alm', V, lam, V), mat, rtol=0, atol=tol)
    for a in range(3):
        for c in range(2):
            assert V[a, np.argmax(np.abs(V[a, :, c])), c] > 0       # the sign convention
    # outputs select rows; uniform weights are the default
    sel = m.active_subspace(x_ref, weights=w, outputs=[2, 0])
    np.testing.assert_array_equal(sel.matrix.numpy(), mat[[2, 0]])
    uni = m.active_subspace(x_ref, weights=np.full(37, 0.25))
    dflt = m.active_subspace(x_ref)
    np.testing.assert_array_equal(uni.matrix.numpy(), dflt.matrix.numpy())


def test_active_subspace_refuses_bad_arguments():
    m, x = model_of('full')
    x_ref = LO + SPAN * np.random.default_rng(7).uniform(0.0, 1.0, (5, 2))
    with pytest.raises(ValueError, match='length'):
        m.active_subspace(x_ref, weights=np.ones(4))
    with pytest.raises(ValueError, match='non-negative'):
        m.active_subspace(x_ref, weights=[1, 1, -1, 1, 1])
    with pytest.raises(ValueError, match='all be zero'):
        m.active_subspace(x_ref, weights=np.zeros(5))
    with pytest.raises(ValueError, match='outputs'):
        m.active_subspace(x_ref, outputs=[3])
    with pytest.raises(ValueError, match='shape'):
        m.active_subspace(x_ref[:, :1])
    with pytest.raises(ValueError, match='shape'):
        m.predict_grad_cov(x_ref[:, :1])


def test_the_input_the_function_depends_on_has_the_largest_activity():
    """y from synth.make_full with d = 1; the model sees a second input column of noise the output ignores"""
    x1, y = synth.make_full(73, 40, 1, 3, 2)
    x = np.hstack([x1, np.random.default_rng(73).uniform(0.0, 1.0, (40, 1))])
    m = patch_engine(LCGP(y=y, x=x, q=2))
    m.fit()
    x_ref = np.random.default_rng(74).uniform(0.0, 1.0, (50, 2))
    res = m.active_subspace(x_ref)
    act = res.activity.numpy()
    print('activity', act)
    assert np.all(act[:, 0] > act[:, 1]), act
    assert np.all(np.abs(res.eigenvectors.numpy()[:, 0, 0]) > np.abs(res.eigenvectors.numpy()[:, 1, 0]))


def test_c_abi_of_the_gradient_covariance_entry():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() == 610
    for name in ('lcgp_predict_gradcov', 'lcgp_predict_gradcov_scratch_bytes'):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    nb, nh = C.c_size_t(0), C.c_size_t(0)
    # n = 1000 -> npad 1024; n0 d = 300 -> 384 rows of dX and of P; q = 2, float64: no X / U slabs
    assert lib.lcgp_predict_gradcov_scratch_bytes(0, 1000, 3, 2, 100, C.byref(nb)) == 0
    assert nb.value == 2 * 2 * 384 * 1024 * 8
    assert lib.lcgp_predict_hess_scratch_bytes(0, 1000, 3, 2, 100, C.byref(nh)) == 0
    assert nb.value < nh.value
    assert lib.lcgp_predict_gradcov_scratch_bytes(1, 1000, 1, 2, 50, C.byref(nb)) == 0
    assert nb.value == 2 * 2 * 64 * 1024 * 4
    assert lib.lcgp_predict_gradcov_scratch_bytes(2, 1000, 3, 2, 100, C.byref(nb)) < 0
    assert b'dtype' in lib.lcgp_last_error()
    assert lib.lcgp_predict_gradcov_scratch_bytes(0, 1000, 127, 2, 100, C.byref(nb)) < 0
    assert b'd must be' in lib.lcgp_last_error()
    assert lib.lcgp_predict_gradcov_scratch_bytes(0, 1000, 100, 2, 50000, C.byref(nb)) < 0
    assert b'n0 * d' in lib.lcgp_last_error()
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything
    head = (dummy, None, dummy, dummy)                              # x, sr, theta, workspace

    def call(dtype=0, kern=0, d=2, n0=10, x0=dummy, scratch=dummy, dghat=dummy, gamma=dummy, w=None, M=None, stride=0):
        return lib.lcgp_predict_gradcov(None, dtype, kern, 100, d, 3, 1, *head, n0, x0, scratch, dghat, gamma, w, M, stride)

    assert call(dtype=2) < 0 and b'dtype' in lib.lcgp_last_error()
    assert call(kern=7) < 0 and b'kernel_id' in lib.lcgp_last_error()
    assert call(d=127) < 0 and b'd must be' in lib.lcgp_last_error()
    assert call(n0=0) < 0 and b'n0' in lib.lcgp_last_error()
    assert call(d=100, n0=50000) < 0 and b'n0 * d' in lib.lcgp_last_error()
    assert call(x0=None) < 0 and b'NULL' in lib.lcgp_last_error()
    assert call(scratch=None) < 0 and b'NULL' in lib.lcgp_last_error()
    assert call(dghat=None) < 0 and b'NULL' in lib.lcgp_last_error()
    assert call(gamma=None) < 0 and b'NULL' in lib.lcgp_last_error()          # nothing to write at all
    assert call(w=dummy) < 0 and b'together' in lib.lcgp_last_error()
    assert call(M=dummy) < 0 and b'together' in lib.lcgp_last_error()
    assert call(stride=5) < 0 and b'out_stride' in lib.lcgp_last_error()
