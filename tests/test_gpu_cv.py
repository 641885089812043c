"""Closed-form cross-validation on the GPU (lcgp_loo; lcgp_cv_gather -> lcgp_potrf_logdet -> lcgp_potri -> lcgp_cv_apply)
against float64 numpy: the closed form on a numpy factorisation of A_k, brute force (drop the inputs, refactor, predict) and
a conditioned model run through the library's own predict_cov; identities (singleton folds = LOO, one fold = the prior),
bitwise-equal results on poisoned memory, float32 against float64, two ranks against one, and the headline shape."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from lcgp_amd import LCGP, synth, _hip
from lcgp_amd.engine import HotPathEngine
from oracle import lcgp_oracle as orc
from tests.test_cv_host import brute_force

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


class _Np:
    """float64 numpy state of a GPU model (what tests.test_cv_host.brute_force reads), computed from the model's own data"""

    def __init__(self, m):
        eng = m._ensure_aux()
        self.kernel = m.kernel
        self.x = (m.x_unique_s if m.submethod == 'rep' else m.x).numpy().astype(np.float64)
        self.n, self.d = self.x.shape
        if m.submethod == 'rep':
            self.sr = np.sqrt(m.r.numpy().astype(float))
            yb = (m.ybar_s if m.rep_standardize_ybar else m.ybar).numpy()
            self.Y = yb * self.sr[None, :]
        else:
            self.sr = None
            self.Y = m.y.numpy()
        th = eng._theta_last
        self._state = [(th[k], None, None, self.Y.T @ th[k, self.d + 3:]) for k in range(th.shape[0])]

    def closed_form(self, k, folds):
        """ghat / gvar of the closed form from a float64 numpy inverse of A_k"""
        th, _, _, b = self._state[k]
        d = self.d
        ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
        s = np.ones(self.n) if self.sr is None else self.sr
        C_ = orc.matern32(self.x, self.x, ell, scale, nug, kernel=self.kernel)
        a = np.linalg.inv(np.eye(self.n) + D * C_ * np.outer(s, s))
        z = a @ b
        gh, gv = np.zeros(self.n), np.zeros(self.n)
        for B in folds:
            mi = np.linalg.inv(a[np.ix_(B, B)])
            gh[B] = (b[B] - mi @ z[B]) / (D * s[B])
            gv[B] = (np.diag(mi) - 1.0) / (D * s[B] ** 2)
        return gh, gv


def _model(mode, kernel='matern32', q=3, dtype='float64', n=600):
    if mode == 'full':
        x, y = synth.make_full(71, n, 2, 4, q)
    else:
        x, y = synth.make_rep(72, n // 3, 3, 2, 4, q)
    m = LCGP(y=y, x=x, q=q, submethod=mode, kernel=kernel, device='cuda:0', dtype=dtype)
    o = orc.OracleLCGP(y=y, x=x, q=q, submethod=mode)
    m._set_flat(synth.param_points(71, o.get_unconstrained())[1])
    return m, x


def _close(a, b, rel):
    scale = max(np.max(np.abs(b)), 1e-300)
    assert np.max(np.abs(a - b)) <= rel * scale, (np.max(np.abs(a - b)), scale)


def _fold_labels(n, sizes, seed):
    lab = np.full(n, len(sizes))
    perm = np.random.default_rng(seed).permutation(n)
    lo = 0
    for f, m in enumerate(sizes):
        lab[perm[lo:lo + m]] = f
        lo += m
    return lab


@pytest.mark.parametrize('kernel', ['matern32', 'se'])
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_loo_and_folds_against_float64_numpy_and_brute_force(mode, kernel):
    m, _ = _model(mode, kernel)
    st = _Np(m)
    n = st.n
    blk = m._ensure_aux().loo_block().cpu().numpy()
    # fold sizes at and around the 64 / 128 tile edges, plus the rest as one more fold
    sizes = [1, 63, 64, 65, 127, 128, 129] if n >= 600 else [1, 63, 64, 65]
    labels = _fold_labels(n, sizes, 5)
    folds = [np.flatnonzero(labels == f) for f in range(len(sizes) + 1)]
    _, ptr, idx = m._cv_labels(labels, 0)
    cvb = m._ensure_aux().cv_block(ptr, idx).cpu().numpy()
    for k in range(int(m.q)):
        gh, gv = st.closed_form(k, [[i] for i in range(n)])
        _close(blk[0, k], gh, 1e-9)
        _close(blk[1, k], gv, 1e-9)
        for i in (0, n // 2, n - 1):
            g, S = brute_force(st, k, [i])
            _close(blk[:, k, i], np.array([g[0], S[0, 0]]), 1e-9)
        gh, gv = st.closed_form(k, folds)
        _close(cvb[0, k], gh, 1e-9)
        _close(cvb[1, k], gv, 1e-9)
        for B in (folds[2], folds[6] if len(folds) > 6 else folds[-1]):
            g, S = brute_force(st, k, B)
            _close(cvb[0, k, B], g, 1e-9)
            _close(cvb[1, k, B], np.diag(S), 1e-9)
    # the public surface: predict's map of the same latent values
    outs = [r.numpy() for r in m.predict_cv(labels)]
    ref = m._outputs_rep(cvb[0], cvb[1]) if mode == 'rep' else m._outputs_full(cvb[0], cvb[1])
    for a, b in zip(outs, ref):
        assert a.shape == (int(m.p), n) and np.array_equal(a, b.numpy())


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_singleton_folds_are_loo_and_one_fold_is_the_prior(mode):
    m, _ = _model(mode, n=300)
    n = m._cv_n()
    loo = m._ensure_aux().loo_block().cpu().numpy()
    cv = m._ensure_aux().cv_block(np.arange(n + 1), np.arange(n)).cpu().numpy()
    _close(cv[0], loo[0], 1e-11)
    _close(cv[1], loo[1], 1e-11)
    st = _Np(m)
    blk, covs = m._ensure_aux().cv_block(np.array([0, n]), np.arange(n), return_cov=True)
    assert np.max(np.abs(blk[0].cpu().numpy())) <= 1e-9 * np.max(np.abs(loo[0]))
    for k in range(int(m.q)):
        th = st._state[k][0]
        prior = orc.matern32(st.x, st.x, th[:st.d], th[st.d], th[st.d + 1], kernel=st.kernel)
        _close(covs[0][k].cpu().numpy(), prior, 1e-9)


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_fold_covariance_is_predict_latent_cov_of_the_conditioned_model(mode):
    m, _ = _model(mode, n=450)
    st = _Np(m)
    n = st.n
    labels = _fold_labels(n, [70, 140], 9)
    _, _, _, lat = m.predict_cv(labels, return_latent_cov=True)
    eng = m._ensure_aux()
    for f in (0, 1):
        B = np.flatnonzero(labels == f)
        R = np.setdiff1d(np.arange(n), B)
        # the conditioned model: the same theta rows (theta, D, psi) on the other inputs, through the library's own path
        cond = HotPathEngine(st.x[R], st.Y[:, R], None if st.sr is None else st.sr[R], eng.q_local, device='cuda:0',
                             kernel=m.kernel)
        cond.evaluate(eng._theta_last)
        ref = cond.predict_cov(st.x[B], same=False).cpu().numpy()
        _close(lat[f].numpy(), ref, 1e-9)
        gh = cond.predict_block(st.x[B], same=False).cpu().numpy()
        loc = eng.cv_block(*m._cv_labels(labels, 0)[1:]).cpu().numpy()
        _close(loc[0][:, B], gh[0], 1e-9)
        _close(loc[1][:, B], gh[1], 1e-9)


def test_bitwise_equal_on_poisoned_cv_workspace_and_outputs():
    m, _ = _model('full', n=400)
    eng = m._ensure_aux()
    n = eng.n
    labels = _fold_labels(n, [1, 64, 129], 3)
    _, ptr, idx = m._cv_labels(labels, 0)
    results = []
    for fill in (0x00, 0xFF, 0x5A):
        eng.cv_block(ptr, idx)                      # allocates the cached workspace
        eng._cv_ws[1].fill_(fill)
        out = eng.cv_block(ptr, idx)
        # lcgp_cv_apply once more into outputs filled with the same byte
        dst = torch.empty((2, eng.q_local, n), dtype=torch.float64, device=eng.device)
        dst.view(torch.uint8).fill_(fill)
        folds_host = np.ascontiguousarray(np.r_[ptr, idx].astype(np.int32))
        fd = torch.as_tensor(folds_host).to(eng.device)
        _hip.check(eng.lib.lcgp_cv_apply(eng._stream(), eng.dtype, n, eng.d, eng.p, eng.q_local, eng._p(eng.sr),
                                         eng._p(eng.theta_dev), eng._p(eng.workspace), len(ptr) - 1,
                                         C.c_void_p(folds_host.ctypes.data), eng._p(fd), eng._p(eng._cv_ws[1]),
                                         eng._p(dst[0]), eng._p(dst[1]), n), "lcgp_cv_apply")
        loo = eng.loo_block()
        results.append((out.cpu().numpy(), dst.cpu().numpy(), loo.cpu().numpy()))
    for r in results[1:]:
        for a, b in zip(r, results[0]):
            assert np.array_equal(a, b)
    assert np.array_equal(results[0][0], results[0][1])


def test_float32_model_within_bound_of_float64():
    m64, _ = _model('full', n=400)
    m32, _ = _model('full', n=400, dtype='float32')
    m32.phi = m64.phi.clone()
    for f in ('predict_loo', 'predict_cv'):
        args = () if f == 'predict_loo' else (8,)
        a = [r.numpy() for r in getattr(m64, f)(*args)]
        b = [r.numpy() for r in getattr(m32, f)(*args)]
        for x, y in zip(b, a):
            assert np.all(np.isfinite(x))
            # float32 factorisation of A (condition number up to ~1e3 here) and float32 kernel values: 1e-3 of the scale
            _close(x, y, 1e-3)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_reproduce_one_rank():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_cv_gpu_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


def test_headline_shape_loo_points_and_one_fold_against_brute_force():
    x, y, cfg = synth.make_config(3)
    m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0')
    m.loss_and_grad(m._get_flat())
    st = _Np(m)
    n = st.n
    assert (n, st.d, int(m.p), int(m.q)) == (4096, 6, 64, 8)
    loo = m._ensure_aux().loo_block().cpu().numpy()
    m.predict_cv(10, seed=1)
    lab = m.cv_labels
    _, ptr, idx = m._cv_labels(lab, 0)
    cv = m._ensure_aux().cv_block(ptr, idx).cpu().numpy()
    B = np.flatnonzero(lab == 3)
    k = 5
    g, S = brute_force(st, k, B)
    _close(cv[0, k, B], g, 1e-8)
    _close(cv[1, k, B], np.diag(S), 1e-8)
    for i in (0, 2047, 4095):
        g, S = brute_force(st, k, [i])
        _close(loo[:, k, i], np.array([g[0], S[0, 0]]), 1e-8)


def test_no_evaluation_between_predict_and_cross_validation():
    m, x = _model('full', n=300)
    m.predict(x[:10])
    eng = m._engine
    calls = []
    orig = eng.evaluate_partial
    eng.evaluate_partial = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    m.predict_loo()
    m.predict_cv(6)
    assert calls == []
