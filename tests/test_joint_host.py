"""CPU tests of the joint posterior covariance and the correlated draws (LCGP.predict_latent_cov / predict_jointcov /
sample): the host layer -- output projection, output selection, rep scaling, seeding by GLOBAL component, error
agreement -- through a numpy stand-in of HotPathEngine.predict_cov / sample_latent, and the argument checks of the new
C entries (tests/test_gpu_joint.py runs the same through liblcgp_hip.so)."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from lcgp_amd import LCGP, synth
from lcgp_amd import dist as _dist
from oracle import lcgp_oracle as orc
from tests.helpers import OracleEngine


class JointOracleEngine(OracleEngine):
    """OracleEngine plus the two joint-covariance entries, in numpy"""

    def _sigma(self, x0s, same):
        x0s = np.asarray(x0s, np.float64)
        n0 = x0s.shape[0]
        sr = np.ones(self.n) if self.sr is None else self.sr
        out = np.zeros((self.q_local, n0, n0))
        for i, (th, low, z, b) in enumerate(self._state):
            d = self.d
            ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
            c00 = orc.matern32(x0s, x0s, ell, scale, nug, kernel=self.kernel)
            c = orc.matern32(x0s, self.x, ell, scale, nug, kernel=self.kernel)      # (the nugget iff x0 IS x, as `same`)
            u = sla.solve_triangular(low, (c * sr[None, :]).T, lower=True)
            out[i] = c00 - D * u.T @ u
        return out

    def predict_cov(self, x0s, same=False):
        return torch.as_tensor(self._sigma(x0s, same))

    def sample_latent(self, x0s, S, seeds, jitter=1e-10, same=False):
        sig = self._sigma(x0s, same)
        gh, _ = self.predict(np.asarray(x0s, np.float64), same)
        n0 = sig.shape[1]
        out = np.zeros((self.q_local, S, n0))
        for i, th in enumerate(self._state):
            low = np.linalg.cholesky(sig[i] + jitter * th[0][self.d] * np.eye(n0))
            eps = np.random.default_rng(seeds[i]).standard_normal((S, n0))
            out[i] = gh[i][None, :] + eps @ low.T
        return torch.as_tensor(out)


def _patch(model, engine_cls=JointOracleEngine):
    def _make(dtype=None):
        rank, world = _dist.rank_world(model._group)
        model._local_ks = _dist.local_components(model.q, rank, world)
        if model.submethod == 'rep':
            sr = np.sqrt(model.r.numpy().astype(float))
            yb = (model.ybar_s if model.rep_standardize_ybar else model.ybar).numpy()
            return engine_cls(model.x_unique_s.numpy(), yb * sr[None, :], sr, len(model._local_ks),
                              comp_ids=model._local_ks, q_total=model.q, kernel=model.kernel)
        return engine_cls(model.x.numpy(), model.y.numpy(), None, len(model._local_ks),
                          comp_ids=model._local_ks, q_total=model.q, kernel=model.kernel)
    model._make_engine = _make
    return model


def _model(mode, kernel='matern32', **kw):
    if mode == 'full':
        x, y = synth.make_full(41, 40, 2, 3, 3)
        m = _patch(LCGP(y=y, x=x, submethod=mode, kernel=kernel, **kw))
    else:
        x, y = synth.make_rep(42, 16, 3, 2, 4, 4)
        m = _patch(LCGP(y=y, x=x, submethod=mode, kernel=kernel, **kw))
    o = orc.OracleLCGP(y=y, x=x, submethod=mode)
    m._set_flat(synth.param_points(41, o.get_unconstrained())[1])
    return m, x


@pytest.mark.parametrize('mode,kw', [('full', {}), ('rep', {}), ('rep', {'rep_standardize_ybar': False}),
                                     ('full', {'kernel': 'se'})])
def test_diagonals_are_the_marginals_of_predict(mode, kw):
    m, x = _model(mode, **kw)
    x0 = np.vstack([np.random.default_rng(1).uniform(0, 1, (7, 2)), x[:3]])    # including training inputs
    ypred, ypredvar, yconfvar = [t.numpy() for t in m.predict(x0)]
    gvar = m.gvar.numpy()
    lc = m.predict_latent_cov(x0).numpy()
    assert lc.shape == (m.q, 10, 10)
    np.testing.assert_allclose(np.diagonal(lc, axis1=1, axis2=2), gvar, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(lc, np.transpose(lc, (0, 2, 1)), rtol=0, atol=1e-14)
    jc = m.predict_jointcov(x0).numpy()
    jc0 = m.predict_jointcov(x0, include_noise=False).numpy()
    assert jc.shape == (m.p, 10, 10)
    np.testing.assert_allclose(np.diagonal(jc, axis1=1, axis2=2), ypredvar, rtol=1e-12)
    np.testing.assert_allclose(np.diagonal(jc0, axis1=1, axis2=2), yconfvar, rtol=1e-12)
    off = ~np.eye(10, dtype=bool)
    np.testing.assert_allclose(jc[:, off], jc0[:, off], rtol=1e-14)       # the noise is white
    sel = m.predict_jointcov(x0, outputs=[2, 0]).numpy()
    np.testing.assert_array_equal(sel, jc[[2, 0]])


def test_training_set_as_x0_applies_the_nugget_as_predict_does():
    m, x = _model('full')
    lc = m.predict_latent_cov(x).numpy()
    m.predict(x)
    np.testing.assert_allclose(np.diagonal(lc, axis1=1, axis2=2), m.gvar.numpy(), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_sample_projects_seeds_by_global_component_and_scales(mode):
    m, x = _model(mode)
    x0 = np.random.default_rng(2).uniform(0, 1, (6, 2))
    s = m.sample(x0, size=5, seed=11).numpy()
    assert s.shape == (5, m.p, 6)
    np.testing.assert_array_equal(s, m.sample(x0, size=5, seed=11).numpy())
    assert not np.array_equal(s, m.sample(x0, size=5, seed=12).numpy())
    assert not np.array_equal(s, m.sample(x0, size=5, seed=11, include_noise=False).numpy())
    # restated: latent component k from default_rng((seed, k)), the observation noise from default_rng((seed, q))
    lc = m.predict_latent_cov(x0).numpy()
    m.predict(x0)
    gh = m.ghat.numpy()
    W, noise, scale, offset = m._output_map()
    g = np.stack([gh[k][None, :] + np.random.default_rng((11, k)).standard_normal((5, 6))
                  @ np.linalg.cholesky(lc[k] + 1e-10 * m.lLmb0.numpy()[k] * np.eye(6)).T for k in range(m.q)])
    ys = np.einsum('ka,ksi->sai', W, g) + np.sqrt(noise)[None, :, None] * \
        np.random.default_rng((11, m.q)).standard_normal((5, m.p, 6))
    np.testing.assert_allclose(s, ys * scale[None, :, None] + offset[None, :, None], rtol=1e-12, atol=1e-12)
    # the same map as predict(): the mean of the noise-free draws' generator is ypred
    ypred = m.predict(x0)[0].numpy()
    np.testing.assert_allclose(np.einsum('ka,ki->ai', W, gh) * scale[:, None] + offset[:, None], ypred, rtol=1e-12)


def test_jointcov_is_the_projection_of_the_latent_covariance():
    m, x = _model('rep')
    x0 = np.random.default_rng(4).uniform(0, 1, (5, 2))
    lc = m.predict_latent_cov(x0).numpy()
    W, noise, scale, _ = m._output_map()
    want = np.einsum('ka,kij->aij', W ** 2, lc) + noise[:, None, None] * np.eye(5)[None]
    want *= (scale ** 2)[:, None, None]
    np.testing.assert_allclose(m.predict_jointcov(x0).numpy(), want, rtol=1e-13)


def test_failed_factorisation_raises_naming_the_global_component_and_jitter():
    class Failing(JointOracleEngine):
        def sample_latent(self, x0s, S, seeds, jitter=1e-10, same=False):
            info = np.array([0, 3, 0], np.int32)
            err = np.linalg.LinAlgError('local')
            err.info = info
            raise err
    m, x = _model('full')
    m = _patch(m, Failing)
    m._engine = None
    with pytest.raises(np.linalg.LinAlgError, match=r"component\(s\) \[1\].*jitter=0"):
        m.sample(x[:4], size=2, seed=0, jitter=0.0)


def test_c_abi_argument_checks_of_the_joint_entries():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() >= 520
    nb = C.c_size_t(0)
    assert lib.lcgp_predict_cov_scratch_bytes(0, 1000, 2, 100, C.byref(nb)) == 0
    assert nb.value == 2 * 2 * 128 * 1024 * 8
    assert lib.lcgp_predict_cov_scratch_bytes(2, 1000, 2, 100, C.byref(nb)) < 0
    assert b'dtype' in lib.lcgp_last_error()
    assert lib.lcgp_sample_scratch_bytes(0, 100, 2, 0, C.byref(nb)) < 0
    assert b'S must be' in lib.lcgp_last_error()
    assert lib.lcgp_sample_scratch_bytes(0, 100, 2, 200, C.byref(nb)) == 0 and nb.value == 2 * 2 * 256 * 128 * 8
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything
    args = (None, 0, 0, 100, 2, 3, 1, dummy, None, dummy, dummy)
    assert lib.lcgp_predict_cov(*args, 0, dummy, 0, dummy, dummy, 0.0) < 0
    assert b'n0' in lib.lcgp_last_error()
    assert lib.lcgp_predict_cov(*args, 10, dummy, 0, dummy, dummy, -1.0) < 0
    assert b'jitter' in lib.lcgp_last_error()
    assert lib.lcgp_predict_cov(*args, 10, dummy, 0, dummy, dummy, float('nan')) < 0
    assert lib.lcgp_predict_cov(*args, 10, dummy, 95, dummy, dummy, 0.0) < 0
    assert b'same' in lib.lcgp_last_error()
    assert lib.lcgp_predict_cov(*args, 10, dummy, 0, None, dummy, 0.0) < 0
    assert b'NULL' in lib.lcgp_last_error()
    assert lib.lcgp_predict_cov(None, 0, 7, 100, 2, 3, 1, dummy, None, dummy, dummy, 10, dummy, 0, dummy, dummy, 0.0) < 0
    assert b'kernel_id' in lib.lcgp_last_error()
    assert lib.lcgp_sample_latent(None, 0, 10, 2, 3, 1, 0, dummy, dummy, dummy, 0, dummy, dummy) < 0
    assert b'S must be' in lib.lcgp_last_error()
    assert lib.lcgp_sample_latent(None, 0, 10, 2, 3, 1, 4, dummy, dummy, dummy, 5, dummy, dummy) < 0
    assert b'ldg' in lib.lcgp_last_error()
    assert lib.lcgp_sample_latent(None, 0, 10, 2, 3, 1, 4, dummy, None, dummy, 0, dummy, dummy) < 0
    assert b'NULL' in lib.lcgp_last_error()
