"""CPU tests of the joint posterior on a conditioned view (ConditionedLCGP.predict_latent_cov / predict_jointcov / sample):
the numpy stand-in of tests/test_condition_host.py extended by condition_predict_cov / condition_sample_latent in the closed
form of include/lcgp_hip.h, checked against brute force (augment the training set, refactor I + D (C o s s^T) on n + m points,
dense float64); the host layer -- output projection, noise, seeding, staleness, the gather over ranks -- through that stand-in;
the conditioning identity through the public API; and the symbols, argument checks and sizes of the new C entries
(tests/test_gpu_condition_joint.py runs the same through liblcgp_hip.so)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from tests.test_condition_host import (KERNELS, CondOracleEngine, _free_port, make_model, new_columns, patch_cond)
from tests.test_predict_hess_host import _cross

HERE = os.path.dirname(os.path.abspath(__file__))
JITTER = 1e-6       # of the draws below: with it the factor of a covariance known to 1e-9 is known to about 1e-6 (see there)


def _prior(x0, th, kernel):
    d = x0.shape[1]
    c = _cross(x0, x0, th[:d], th[d], th[d + 1], kernel)
    c[np.arange(len(x0)), np.arange(len(x0))] = th[d]               # the nugget on the diagonal
    return c


class JointCondOracleEngine(CondOracleEngine):
    """CondOracleEngine plus the joint covariance and the draws of the fitted model and of a view, in numpy float64"""

    def _parts(self, th, low, x0):
        d = self.d
        sr = np.ones(self.n) if self.sr is None else self.sr
        X0 = _cross(x0, self.x, th[:d], th[d], th[d + 1], self.kernel) * sr[None, :]
        return X0, sla.solve_triangular(low, X0.T, lower=True).T

    def _sigma(self, x0s, state=None):
        x0 = np.asarray(x0s, np.float64)
        out = np.zeros((self.q_local, len(x0), len(x0)))
        for i, (th, low, z, b) in enumerate(self._state):
            D = th[self.d + 2]
            _, U0 = self._parts(th, low, x0)
            out[i] = _prior(x0, th, self.kernel) - D * U0 @ U0.T
            if state is not None:
                Un, LS, v = state['state'][i]
                Sg = _cross(x0, state['xn'], th[:self.d], th[self.d], th[self.d + 1], self.kernel) - D * U0 @ Un.T
                T = sla.solve_triangular(LS, Sg.T, lower=True).T
                out[i] -= T @ T.T
        return out

    def _draws(self, sig, gh, S, seeds, jitter):
        n0 = sig.shape[1]
        out = np.zeros((self.q_local, S, n0))
        for i, st in enumerate(self._state):
            low = np.linalg.cholesky(sig[i] + jitter * st[0][self.d] * np.eye(n0))
            out[i] = gh[i][None, :] + np.random.default_rng(seeds[i]).standard_normal((S, n0)) @ low.T
        return torch.as_tensor(out)

    def predict_cov(self, x0s, same=False):
        assert not same
        return torch.as_tensor(self._sigma(x0s))

    def sample_latent(self, x0s, S, seeds, jitter=1e-10, same=False):
        assert not same
        return self._draws(self._sigma(x0s), self.predict(np.asarray(x0s, np.float64))[0], S, seeds, jitter)

    def condition_predict_cov(self, state, x0s):
        assert self.is_current(state['theta'])
        return torch.as_tensor(self._sigma(x0s, state))

    def condition_sample_latent(self, state, x0s, S, seeds, jitter=1e-10):
        gh = self.condition_predict_block(state, x0s)[0].numpy()
        return self._draws(self._sigma(x0s, state), gh, S, seeds, jitter)


def joint_model(mode, kernel='matern32', d=2, **kw):
    m, x, y, xn, yn = make_model(mode, kernel, d, **kw)
    return patch_cond(m, JointCondOracleEngine), x, xn, yn


def dense_joint(rows, x, s, Y, kernel, xn_s, snew, ycol, x0s):
    """(ghat, Sigma) (q, n0) / (q, n0, n0) from first principles in float64 numpy: the training set (x, s, Y) augmented by the
    new columns, A = I + D (C o s s^T) on the n + m points rebuilt and factorised at the theta rows, lcgp_predict_cov's formula
    with same = 0"""
    xa, sa, Ya = np.vstack([x, xn_s]), np.r_[s, snew], np.hstack([Y, ycol])
    d = xa.shape[1]
    gh, sig = [], []
    for th in rows:
        ell, scale, nug, D, psi = th[:d], th[d], th[d + 1], th[d + 2], th[d + 3:]
        low = np.linalg.cholesky(np.eye(len(xa)) + D * _prior(xa, th, kernel) * np.outer(sa, sa))
        u = sla.solve_triangular(low, (_cross(x0s, xa, ell, scale, nug, kernel) * sa[None, :]).T, lower=True)
        gh.append(u.T @ sla.solve_triangular(low, Ya.T @ psi, lower=True))
        sig.append(_prior(x0s, th, kernel) - D * u.T @ u)
    return np.stack(gh), np.stack(sig)


def dense_augmented_joint(m, xn, yn, x0):
    eng = m._aux_engine
    s = np.ones(eng.n) if eng.sr is None else eng.sr
    return dense_joint(eng._theta_last, eng.x, s, eng.Y, eng.kernel, *new_columns(m, xn, yn), m._standardise_x0(x0)[0])


def _x0(x, d, n=9):
    """new inputs on the model's raw scale, two training inputs among them"""
    return np.vstack([-1.5 + 4.0 * np.random.default_rng(3).uniform(0, 1, (n, d)), x[:2]])


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_view_joint_equals_brute_force_augmentation(mode, kernel):
    m, x, xn, yn = joint_model(mode, kernel)
    x0 = np.vstack([_x0(x, 2), xn[:1]])                 # ... and one of the view's own inputs
    view = m.condition(xn, yn)
    lc = view.predict_latent_cov(x0)
    assert lc.dtype == torch.float64 and tuple(lc.shape) == (2, 12, 12) and not lc.requires_grad
    lc = lc.numpy()
    rh, rs = dense_augmented_joint(m, xn, yn, x0)
    np.testing.assert_allclose(lc, rs, rtol=0, atol=1e-9 * np.max(np.abs(rs)))
    # the runs did something: the covariance of the base model is another one
    assert np.max(np.abs(lc - m.predict_latent_cov(x0).numpy())) > 1e-4 * np.max(np.abs(rs))
    # the outputs: the base model's map on the dense covariance
    W, noise, scale, offset = m._output_map()
    want = np.einsum('ka,kij->aij', W ** 2, rs)
    jc0 = view.predict_jointcov(x0, include_noise=False).numpy()
    jc = view.predict_jointcov(x0).numpy()
    assert jc.shape == (3, 12, 12)
    tol = 1e-9 * np.max(np.abs(want * (scale ** 2)[:, None, None]))
    np.testing.assert_allclose(jc0, want * (scale ** 2)[:, None, None], rtol=0, atol=tol)
    np.testing.assert_allclose(jc, (want + noise[:, None, None] * np.eye(12)[None]) * (scale ** 2)[:, None, None], rtol=0, atol=tol)
    np.testing.assert_array_equal(view.predict_jointcov(x0, outputs=[2, 0]).numpy(), jc[[2, 0]])
    np.testing.assert_array_equal(view.predict_jointcov(x0, outputs=1, include_noise=False).numpy(), jc0[[1]])
    # the draws: ghat' + eps L^T with L the factor of the DENSE covariance plus the jitter.  The view's covariance is the dense
    # one to 1e-9 of its largest entry; with the jitter its smallest eigenvalue is at least 1e-6 scale, so the factor moves by
    # about 1e-9 / sqrt(1e-6) = 1e-6 of that scale: bound 1e-5 of the largest draw
    s = view.sample(x0, size=4, seed=11, jitter=JITTER)
    assert s.dtype == torch.float64 and tuple(s.shape) == (4, 3, 12)
    rows = m._aux_engine._theta_last
    g = np.stack([rh[k][None, :] + np.random.default_rng((11, k)).standard_normal((4, 12))
                  @ np.linalg.cholesky(rs[k] + JITTER * rows[k][2] * np.eye(12)).T for k in range(2)])
    ys = np.einsum('ka,ksi->sai', W, g)
    ys0 = ys * scale[None, :, None] + offset[None, :, None]
    ys = (ys + np.sqrt(noise)[None, :, None] * np.random.default_rng((11, 2)).standard_normal((4, 3, 12))) \
        * scale[None, :, None] + offset[None, :, None]
    np.testing.assert_allclose(s.numpy(), ys, rtol=0, atol=1e-5 * np.max(np.abs(ys)))
    s0 = view.sample(x0, size=4, seed=11, include_noise=False, jitter=JITTER).numpy()
    np.testing.assert_allclose(s0, ys0, rtol=0, atol=1e-5 * np.max(np.abs(ys0)))
    np.testing.assert_array_equal(s.numpy(), view.sample(x0, size=4, seed=11, jitter=JITTER).numpy())
    assert not np.array_equal(s.numpy(), view.sample(x0, size=4, seed=12, jitter=JITTER).numpy())
    assert tuple(view.sample(x0).shape) == (1, 3, 12)                # defaults: one draw, a fresh seed


@pytest.mark.parametrize('mode,kw', [('full', {}), ('rep', {}), ('rep', {'rep_standardize_ybar': False})])
def test_diagonals_are_the_marginals_of_the_view(mode, kw):
    m, x, xn, yn = joint_model(mode, **kw)
    x0 = _x0(x, 2)
    view = m.condition(xn, yn)
    ypred, ypredvar, yconfvar = [t.numpy() for t in view.predict(x0)]
    gvar = view.predict(x0, latent=True)[1].numpy()
    lc = view.predict_latent_cov(x0).numpy()
    np.testing.assert_allclose(np.diagonal(lc, axis1=1, axis2=2), gvar, rtol=1e-12, atol=1e-14 * np.max(np.abs(lc)))
    np.testing.assert_allclose(np.diagonal(view.predict_jointcov(x0).numpy(), axis1=1, axis2=2), ypredvar, rtol=1e-12)
    np.testing.assert_allclose(np.diagonal(view.predict_jointcov(x0, include_noise=False).numpy(), axis1=1, axis2=2), yconfvar,
                               rtol=1e-11)


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_conditioning_identity_through_the_public_api(mode, kernel):
    """view.predict_latent_cov(x0) = Sigma(x0, x0) - Sigma(x0, xn) (Sigma(xn, xn) + diag tau)^-1 Sigma(xn, x0) with Sigma the BASE
    model's predict_latent_cov over [x0; xn] and tau_i = 1 / (D_k r_i)"""
    m, x, xn, yn = joint_model(mode, kernel)
    x0 = _x0(x, 2, 7)
    view = m.condition(xn, yn)
    xu = view.x_new.numpy()
    if mode == 'rep':
        r = np.array([np.sum(np.all(xn == u[None, :], axis=1)) for u in xu], float)
    else:
        r = np.ones(len(xu))
    big = m.predict_latent_cov(np.vstack([x0, xu])).numpy()
    got = view.predict_latent_cov(x0).numpy()
    n0 = len(x0)
    for k in range(2):
        D = float(m.diag_D[k])
        S = big[k][n0:, n0:] + np.diag(1.0 / (D * r))
        want = big[k][:n0, :n0] - big[k][:n0, n0:] @ np.linalg.solve(S, big[k][n0:, :n0])
        np.testing.assert_allclose(got[k], want, rtol=0, atol=1e-9 * np.max(np.abs(big[k])))


def test_errors_and_staleness():
    m, x, xn, yn = joint_model('full')
    view = m.condition(xn, yn)
    x0 = x[:3] + 0.01
    for size in (0, -2):
        with pytest.raises(ValueError, match='size must be >= 1'):
            view.sample(x0, size=size)
    for fn in (view.predict_latent_cov, view.predict_jointcov, view.sample):
        with pytest.raises(ValueError, match='x0 must have shape'):
            fn(np.zeros((3, 3)))
    before = [t.numpy().copy() for t in (m.predict_jointcov(x0), m.sample(x0, seed=0), *m.predict(x0))]
    view.predict_latent_cov(x0), view.predict_jointcov(x0), view.sample(x0, seed=3)
    after = [t.numpy() for t in (m.predict_jointcov(x0), m.sample(x0, seed=0), *m.predict(x0))]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))          # the base model is only read
    m._set_flat(m._get_flat() + 0.01)
    for fn in (view.predict_latent_cov, view.predict_jointcov, view.sample):
        with pytest.raises(RuntimeError, match='stale'):
            fn(x0)
    m.predict(x0)
    for fn in (view.predict_latent_cov, view.predict_jointcov, view.sample):
        with pytest.raises(RuntimeError, match='stale'):
            fn(x0)


def test_failed_factorisation_names_the_global_component_and_the_jitter():
    class Failing(JointCondOracleEngine):
        def condition_sample_latent(self, state, x0s, S, seeds, jitter=1e-10):
            err = np.linalg.LinAlgError('local')
            err.info = np.array([0, 3], np.int32)
            raise err
    m, x, _, xn, yn = make_model('full')
    view = patch_cond(m, Failing).condition(xn, yn)
    with pytest.raises(np.linalg.LinAlgError, match=r"component\(s\) \[1\].*jitter=0"):
        view.sample(x[:4] + 0.01, size=2, seed=0, jitter=0.0)


def test_view_on_the_float64_engine_of_a_float32_model():
    class F32Fails(JointCondOracleEngine):
        def condition_begin(self, xn_s, t, r=None):
            if self.dtype_name == 'float32':
                err = np.linalg.LinAlgError('S_k')
                err.info = np.array([0, 2])
                raise err
            return super().condition_begin(xn_s, t, r)
    m, x, _, xn, yn = make_model('full', dtype='float32')
    patch_cond(m, F32Fails)
    x0 = x[:4] + 0.01
    view = m.condition(xn, yn)
    assert view._engine is m._engine64 and view._engine is not m._aux_engine
    ref = joint_model('full')[0].condition(xn, yn)
    assert torch.equal(view.predict_latent_cov(x0), ref.predict_latent_cov(x0))
    assert torch.equal(view.predict_jointcov(x0), ref.predict_jointcov(x0))
    assert torch.equal(view.sample(x0, size=3, seed=4), ref.sample(x0, size=3, seed=4))


def test_two_ranks_draw_what_one_rank_draws():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_condition_joint_host_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


NEW_SYMBOLS = ('lcgp_condition_predict_cov_scratch_bytes', 'lcgp_condition_predict_cov')


def test_new_symbols_and_the_scratch_formula():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() == 610
    for name in NEW_SYMBOLS:
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    from lcgp_amd.engine import HotPathEngine
    assert hasattr(HotPathEngine, 'condition_predict_cov') and hasattr(HotPathEngine, 'condition_sample_latent')
    nb = C.c_size_t(0)

    def r256(v):
        return (v + 255) // 256 * 256

    # the header's formula: q n0pad K' esz + q X npad esz + 2 q X mpad esz + 2 roundup256(q n0 8), X = min(2048, pad(n0))
    n, q, n0, n0pad, X = 4096, 8, 2000, 2048, 2048
    for m, mpad in ((32, 128), (1024, 1024)):
        for dtype, esz in ((0, 8), (1, 4)):
            assert lib.lcgp_condition_predict_cov_scratch_bytes(dtype, n, q, m, n0, C.byref(nb)) == 0, lib.lcgp_last_error()
            assert nb.value == (q * n0pad * (n + mpad) * esz + q * X * n * esz + 2 * q * X * mpad * esz + 2 * r256(q * n0 * 8))
    # below 128 rows the row former works on 64
    assert lib.lcgp_condition_predict_cov_scratch_bytes(0, 333, 3, 70, 1, C.byref(nb)) == 0
    assert nb.value == 3 * 128 * (384 + 128) * 8 + 3 * 64 * 384 * 8 + 2 * 3 * 64 * 128 * 8 + 2 * 256
    for args, msg in (((0, 4096, 8, 0, 1), b'm < 1'), ((0, 4096, 8, 5, 0), b'n0 < 1'), ((2, 4096, 8, 5, 1), b'dtype'),
                      ((0, 0, 8, 5, 1), b'n < 1'), ((0, 4096, 0, 5, 1), b'q_local')):
        assert lib.lcgp_condition_predict_cov_scratch_bytes(*args, C.byref(nb)) < 0
        assert msg in lib.lcgp_last_error(), (args, lib.lcgp_last_error())
    assert lib.lcgp_condition_predict_cov_scratch_bytes(0, 4096, 8, 5, 1, None) < 0


def test_c_abi_argument_checks():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything
    nb = C.c_size_t(0)
    assert lib.lcgp_condition_predict_cov_scratch_bytes(0, 50, 2, 4, 3, C.byref(nb)) == 0
    need = nb.value

    def cov(dtype=0, kern=0, n=50, d=2, q=2, m=4, n0=3, x=dummy, theta=dummy, ws=dummy, state=dummy, xn=dummy, x0=dummy,
            scratch=dummy, nsc=1 << 40, cws=dummy, jitter=0.0):
        return lib.lcgp_condition_predict_cov(None, dtype, kern, n, d, 3, q, x, None, theta, ws, state, m, xn, n0, x0, scratch, nsc,
                                              cws, jitter)

    for kw, msg in [(dict(m=0), 'm < 1'), (dict(m=-3), 'm < 1'), (dict(n0=0), 'n0 < 1'), (dict(kern=3), 'kernel_id'),
                    (dict(dtype=2), 'dtype'), (dict(d=0), 'd must be'), (dict(n=0), 'n < 1'), (dict(q=0), 'q_local'),
                    (dict(x=None), 'NULL'), (dict(theta=None), 'NULL'), (dict(ws=None), 'NULL'), (dict(state=None), 'NULL'),
                    (dict(xn=None), 'NULL'), (dict(x0=None), 'NULL'), (dict(scratch=None), 'NULL'), (dict(cws=None), 'NULL'),
                    (dict(jitter=-1.0), 'jitter'), (dict(jitter=float('nan')), 'jitter'),
                    (dict(nsc=need - 1), 'scratch is smaller'), (dict(nsc=0), 'scratch is smaller')]:
        assert cov(**kw) == -1, kw
        assert msg.encode() in lib.lcgp_last_error(), (kw, lib.lcgp_last_error())
