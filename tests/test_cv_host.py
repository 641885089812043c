"""CPU tests of closed-form cross-validation (LCGP.predict_loo / predict_cv): the host layer -- fold-label parsing, the
output map, rep scaling, the gather over ranks, the float64 repeat of a float32 model -- through a numpy stand-in of
HotPathEngine.loo_block / cv_block written in the closed form of include/lcgp_hip.h, checked against brute force (drop the
inputs, refactor I + D (C o s s^T) on the rest, predict at them), and the argument checks of the new C entries
(tests/test_gpu_cv.py runs the same through liblcgp_hip.so)."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from lcgp_amd import LCGP, synth
from lcgp_amd import dist as _dist
from oracle import lcgp_oracle as orc
from tests.helpers import OracleEngine

HERE = os.path.dirname(os.path.abspath(__file__))


class CvOracleEngine(OracleEngine):
    """OracleEngine plus loo_block / cv_block in the closed form of include/lcgp_hip.h, in numpy"""
    dtype_name = 'float64'

    def _parts(self, i):
        th, low, z, b = self._state[i]
        s = np.ones(self.n) if self.sr is None else self.sr
        return self.fetch_matrix(2, i), b, z, th[self.d + 2], s

    def loo_block(self):
        out = np.zeros((2, self.q_local, self.n))
        for i in range(self.q_local):
            a, b, z, D, s = self._parts(i)
            aii = np.diag(a)
            out[0, i] = (b - z / aii) / (D * s)
            out[1, i] = (1.0 / aii - 1.0) / (D * s * s)
        return torch.as_tensor(out)

    def cv_block(self, fold_ptr, fold_idx, return_cov=False):
        out = np.zeros((2, self.q_local, self.n))
        covs = []
        info = np.zeros(self.q_local, np.int64)
        for f in range(len(fold_ptr) - 1):
            B = np.asarray(fold_idx[fold_ptr[f]:fold_ptr[f + 1]])
            assert len(B) >= 1 and np.all(np.diff(B) > 0)
            cov = np.zeros((self.q_local, len(B), len(B)))
            for i in range(self.q_local):
                a, b, z, D, s = self._parts(i)
                try:
                    low = np.linalg.cholesky(a[np.ix_(B, B)])
                except np.linalg.LinAlgError:
                    info[i] = 1
                    continue
                mi = np.linalg.inv(low).T @ np.linalg.inv(low)
                out[0, i, B] = (b[B] - mi @ z[B]) / (D * s[B])
                out[1, i, B] = (np.diag(mi) - 1.0) / (D * s[B] ** 2)
                cov[i] = (mi - np.eye(len(B))) / (D * np.outer(s[B], s[B]))
            covs.append(torch.as_tensor(cov))
        if np.any(info):
            err = np.linalg.LinAlgError('fold')
            err.info = info
            raise err
        return (torch.as_tensor(out), covs) if return_cov else torch.as_tensor(out)


def _kern(xa, xb, ell, kernel):
    S = np.abs(xa[:, None, :] / ell - xb[None, :, :] / ell)
    if kernel == 'se':
        return np.exp(-0.5 * np.sum(S * S, axis=2))
    return np.prod(1.0 + S, axis=2) * np.exp(-np.sum(S, axis=2))


def brute_force(eng, i, B):
    """(ghat_B, Sigma_B) of local component i from the model conditioned on every input outside B: refactor and predict"""
    th, _, _, b = eng._state[i]
    d, n = eng.d, eng.n
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    s = np.ones(n) if eng.sr is None else eng.sr
    B = np.asarray(B)
    R = np.setdiff1d(np.arange(n), B)
    nt = nug / (1.0 + nug)
    cbb = scale * ((1 - nt) * _kern(eng.x[B], eng.x[B], ell, eng.kernel) + nt * np.eye(len(B)))
    if len(R) == 0:
        return np.zeros(len(B)), cbb
    crr = scale * ((1 - nt) * _kern(eng.x[R], eng.x[R], ell, eng.kernel) + nt * np.eye(len(R)))
    A = np.eye(len(R)) + D * crr * np.outer(s[R], s[R])
    c = scale * (1 - nt) * _kern(eng.x[B], eng.x[R], ell, eng.kernel) * s[R][None, :]      # same = 0: no nugget
    return c @ np.linalg.solve(A, b[R]), cbb - D * c @ np.linalg.solve(A, c.T)


def _make_factory(model, engine_cls):
    def _make(dtype=None):
        rank, world = _dist.rank_world(model._group)
        model._local_ks = _dist.local_components(model.q, rank, world)
        if not model._local_ks:
            return None
        if model.submethod == 'rep':
            sr = np.sqrt(model.r.numpy().astype(float))
            yb = (model.ybar_s if model.rep_standardize_ybar else model.ybar).numpy()
            e = engine_cls(model.x_unique_s.numpy(), yb * sr[None, :], sr, len(model._local_ks),
                           comp_ids=model._local_ks, q_total=model.q, kernel=model.kernel)
        else:
            e = engine_cls(model.x.numpy(), model.y.numpy(), None, len(model._local_ks),
                           comp_ids=model._local_ks, q_total=model.q, kernel=model.kernel)
        e.dtype_name = dtype or model._dtype
        return e
    return _make


def patch_cv(model, engine_cls=CvOracleEngine):
    model._make_engine = _make_factory(model, engine_cls)
    return model


CASES = [('full', {}), ('rep', {}), ('rep', {'rep_standardize_ybar': False}), ('full', {'kernel': 'se'})]


def _model(mode, group=None, **kw):
    if mode == 'full':
        x, y = synth.make_full(41, 40, 2, 3, 3)
    else:
        x, y = synth.make_rep(42, 40, 3, 2, 4, 4)      # 40 unique inputs, replicated
    m = patch_cv(LCGP(y=y, x=x, submethod=mode, process_group=group, **kw))
    o = orc.OracleLCGP(y=y, x=x, submethod=mode)
    m._set_flat(synth.param_points(41, o.get_unconstrained())[1])
    return m, x


def _brute_latent(m, folds):
    eng = m._ensure_aux()
    q, n = len(m._local_ks), eng.n
    gh, gv = np.zeros((q, n)), np.zeros((q, n))
    for i in range(q):
        for B in folds:
            g, S = brute_force(eng, i, B)
            gh[i, B], gv[i, B] = g, np.diag(S)
    return gh, gv


def _outputs(m, gh, gv):
    res = m._outputs_rep(gh, gv) if m.submethod == 'rep' else m._outputs_full(gh, gv)
    return [r.numpy() for r in res]


@pytest.mark.parametrize('mode,kw', CASES)
def test_loo_at_every_input_equals_brute_force(mode, kw):
    m, _ = _model(mode, **kw)
    n = m._cv_n()
    assert n == 40
    out = [r.numpy() for r in m.predict_loo()]
    gh, gv = _brute_latent(m, [[i] for i in range(n)])
    ref = _outputs(m, gh, gv)
    for a, b in zip(out, ref):
        assert a.shape == (int(m.p), n)
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-11 * np.max(np.abs(b)))
    lat = m._aux_engine.loo_block().numpy()
    np.testing.assert_allclose(lat[0], gh, rtol=1e-9, atol=1e-11 * np.max(np.abs(gh)))
    np.testing.assert_allclose(lat[1], gv, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize('mode,kw', CASES)
def test_folds_and_their_latent_covariance_equal_brute_force(mode, kw):
    m, _ = _model(mode, **kw)
    n = m._cv_n()
    labels = np.random.default_rng(3).integers(0, 4, n) * 7 - 3      # arbitrary integer labels, unequal folds
    ypred, ypv, ycv, lat = m.predict_cv(labels, return_latent_cov=True)
    folds = [np.flatnonzero(labels == v) for v in np.unique(labels)]
    gh, gv = _brute_latent(m, folds)
    for a, b in zip((ypred, ypv, ycv), _outputs(m, gh, gv)):
        np.testing.assert_allclose(a.numpy(), b, rtol=1e-9, atol=1e-11 * np.max(np.abs(b)))
    eng = m._aux_engine
    assert len(lat) == len(folds)
    for f, B in enumerate(folds):
        assert lat[f].shape == (int(m.q), len(B), len(B))
        for k in range(int(m.q)):
            np.testing.assert_allclose(lat[f][k].numpy(), brute_force(eng, k, B)[1], rtol=1e-8, atol=1e-12)
    assert np.array_equal(m.cv_labels, labels)


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_singleton_folds_reproduce_loo_and_one_fold_gives_the_prior(mode):
    m, _ = _model(mode)
    n = m._cv_n()
    loo = [r.numpy() for r in m.predict_loo()]
    cv = [r.numpy() for r in m.predict_cv(np.arange(n)[::-1].copy())]
    for a, b in zip(loo, cv):
        np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-13)
    eng = m._aux_engine
    lat = m.predict_cv(1, return_latent_cov=True)[3][0].numpy()
    q = int(m.q)
    gh = m._aux_engine.cv_block(np.array([0, n]), np.arange(n))[0].numpy()
    assert np.max(np.abs(gh)) <= 1e-12 * max(1.0, np.max(np.abs(eng._state[0][3])))
    for k in range(q):
        th = eng._state[k][0]
        d = eng.d
        ell, scale, nug = th[:d], th[d], th[d + 1]
        nt = nug / (1 + nug)
        prior = scale * ((1 - nt) * _kern(eng.x, eng.x, ell, eng.kernel) + nt * np.eye(n))
        np.testing.assert_allclose(lat[k], prior, rtol=1e-8, atol=1e-10 * scale)


class _LooAsPredict(CvOracleEngine):
    """predict() answers the brute-force leave-one-out latent values, whatever x0 is"""
    def predict(self, x0s, same=False):
        gh, gv = np.zeros((self.q_local, self.n)), np.zeros((self.q_local, self.n))
        for i in range(self.q_local):
            for j in range(self.n):
                g, S = brute_force(self, i, [j])
                gh[i, j], gv[i, j] = g[0], S[0, 0]
        return gh, gv


@pytest.mark.parametrize('mode,kw', CASES[:3])
def test_output_map_is_that_of_predict_and_ghat_is_left_alone(mode, kw):
    m, x = _model(mode, **kw)
    patch_cv(m, _LooAsPredict)
    x0 = m.x_unique.numpy() if mode == 'rep' else x
    pred = [r.numpy() for r in m.predict(np.asarray(x0))]
    ghat, gvar = m.ghat, m.gvar
    loo = [r.numpy() for r in m.predict_loo()]
    for a, b in zip(loo, pred):
        np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-12 * np.max(np.abs(b)))
    m.predict_cv(5)
    assert m.ghat is ghat and m.gvar is gvar


def test_no_evaluation_between_predict_and_cross_validation():
    m, x = _model('full')
    m.predict(x[:5])
    calls = []
    eng = m._engine
    orig = eng.evaluate
    eng.evaluate = lambda rows: (calls.append(1), orig(rows))[1]
    m.predict_loo()
    m.predict_cv(4)
    assert calls == []


def test_fold_label_parsing_and_its_errors():
    m, _ = _model('full')
    n = m._cv_n()
    m.predict_cv(7, seed=11)
    assert np.array_equal(m.cv_labels, np.random.default_rng(11).permutation(n) % 7)
    m.predict_cv(np.full(n, 2.0))                    # integral floats: one fold
    assert np.all(m.cv_labels == 2)
    _, ptr, idx = m._cv_labels(np.array([1, 0] * (n // 2)), 0)
    assert list(ptr) == [0, n // 2, n] and list(idx[:3]) == [1, 3, 5]
    for bad, msg in ((0, 'number of folds'), (n + 1, 'number of folds'), (2.5, 'int F'), (True, 'int F'),
                     (np.zeros(n - 1, int), 'shape'), (np.full(n, 0.5), 'integers'), (np.array(['a'] * n), 'integers')):
        with pytest.raises(ValueError, match=msg):
            m.predict_cv(bad)
    mr, xr = _model('rep')
    assert len(xr) > mr._cv_n()
    with pytest.raises(ValueError, match='unique input'):
        mr.predict_cv(np.zeros(len(xr), int))


class _Float32Fails(CvOracleEngine):
    def cv_block(self, fold_ptr, fold_idx, return_cov=False):
        if self.dtype_name == 'float32':
            err = np.linalg.LinAlgError('fold')
            err.info = np.arange(1, self.q_local + 1)
            raise err
        return super().cv_block(fold_ptr, fold_idx, return_cov)


def test_float32_model_repeats_a_failed_fold_factorisation_in_float64():
    m, x = _model('full', dtype='float32')
    patch_cv(m, _Float32Fails)
    m.predict(x[:3])
    assert m._aux_engine.dtype_name == 'float32'
    out = [r.numpy() for r in m.predict_cv(4, seed=2)]
    assert m.float32_fallbacks == 1 and m._aux_engine.dtype_name == 'float64' and m._aux_valid
    ref, _ = _model('full')
    for a, b in zip(out, ref.predict_cv(4, seed=2)):
        np.testing.assert_allclose(a, b.numpy(), rtol=1e-12)
    # a float64 engine that fails too: LinAlgError, never NaNs; and without the fallback the float32 failure is raised
    m2, _ = _model('full', dtype='float32')
    patch_cv(m2, _Float32Fails)
    m2.float32_fallback = False
    with pytest.raises(np.linalg.LinAlgError, match='fold matrix'):
        m2.predict_cv(4)
    m3, _ = _model('full', dtype='float32')
    patch_cv(m3, _AlwaysFails)
    with pytest.raises(np.linalg.LinAlgError, match='float64 either'):
        m3.predict_cv(4)
    assert m3.float32_fallbacks == 1


class _AlwaysFails(CvOracleEngine):
    def cv_block(self, fold_ptr, fold_idx, return_cov=False):
        err = np.linalg.LinAlgError('fold')
        err.info = np.ones(self.q_local, np.int64)
        raise err


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_gather_what_one_rank_computes():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_cv_host_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


def test_c_abi_argument_checks_of_the_cross_validation_entries():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() >= 540
    nb = C.c_size_t(0)

    def folds(ptr, idx):
        a = np.ascontiguousarray(np.r_[ptr, idx].astype(np.int32))
        return a, C.c_void_p(a.ctypes.data)

    good, gp = folds([0, 3, 5], [0, 2, 4, 1, 3])
    assert lib.lcgp_cv_workspace_bytes(0, 5, 2, 3, 4, 2, gp, C.byref(nb)) == 0
    ref = C.c_size_t(0)
    assert lib.lcgp_workspace_bytes(0, 3, 2, 3, 8, C.byref(ref)) == 0 and nb.value == ref.value
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything
    cases = [(([0, 0, 5], [0, 1, 2, 3, 4]), 'empty fold'),
             (([0, 3, 5], [0, 2, 5, 1, 3]), 'out of range'),
             (([0, 3, 5], [0, 2, 4, 2, 3]), 'repeated'),
             (([0, 3, 5], [0, 4, 2, 1, 3]), 'sorted'),
             (([0, 3, 4], [0, 2, 4, 1, 3]), 'fold_ptr')]
    for (ptr, idx), msg in cases:
        a, p = folds(ptr, idx)
        assert lib.lcgp_cv_workspace_bytes(0, 5, 2, 3, 4, 2, p, C.byref(nb)) < 0
        assert msg.encode() in lib.lcgp_last_error(), (msg, lib.lcgp_last_error())
        assert lib.lcgp_cv_gather(None, 0, 5, 2, 3, 4, dummy, 2, p, dummy, dummy) < 0
        assert msg.encode() in lib.lcgp_last_error()
        assert lib.lcgp_cv_apply(None, 0, 5, 2, 3, 4, None, dummy, dummy, 2, p, dummy, dummy, dummy, dummy, 0) < 0
        assert msg.encode() in lib.lcgp_last_error()
    big, bp = folds(np.arange(9000), np.arange(8999))
    assert lib.lcgp_cv_workspace_bytes(0, 8999, 2, 3, 8, 8999, bp, C.byref(nb)) < 0
    assert b'65535' in lib.lcgp_last_error()
    assert lib.lcgp_cv_workspace_bytes(0, 5, 2, 3, 4, 0, gp, C.byref(nb)) < 0
    assert lib.lcgp_cv_workspace_bytes(0, 5, 2, 3, 4, 2, None, C.byref(nb)) < 0
    assert b'NULL' in lib.lcgp_last_error()
    assert lib.lcgp_cv_gather(None, 0, 5, 2, 3, 4, dummy, 2, gp, None, dummy) < 0
    assert b'NULL' in lib.lcgp_last_error()
    assert lib.lcgp_cv_apply(None, 0, 5, 2, 3, 4, None, dummy, dummy, 2, gp, dummy, dummy, None, dummy, 0) < 0
    assert b'NULL' in lib.lcgp_last_error()
    assert lib.lcgp_cv_apply(None, 0, 5, 2, 3, 4, None, dummy, dummy, 2, gp, dummy, dummy, dummy, dummy, 4) < 0
    assert b'out_stride' in lib.lcgp_last_error()
    assert lib.lcgp_cv_gather(None, 2, 5, 2, 3, 4, dummy, 2, gp, dummy, dummy) < 0
    assert b'dtype' in lib.lcgp_last_error()
    assert lib.lcgp_loo(None, 0, 5, 2, 3, 4, None, dummy, dummy, None, dummy, 0) < 0
    assert b'NULL' in lib.lcgp_last_error()
    assert lib.lcgp_loo(None, 0, 5, 2, 3, 4, None, dummy, dummy, dummy, dummy, 3) < 0
    assert b'out_stride' in lib.lcgp_last_error()
    assert lib.lcgp_loo(None, 0, 0, 2, 3, 4, None, dummy, dummy, dummy, dummy, 0) < 0
    assert b'n < 1' in lib.lcgp_last_error()
