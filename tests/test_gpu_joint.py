"""Joint posterior covariance over new inputs and correlated draws on the GPU (lcgp_predict_cov, lcgp_potrf_logdet on the
cov workspace, lcgp_sample_latent): against predict()'s marginals, a float64 numpy restatement of
Sigma_k = C00_k - D_k (c0_k o sr) A_k^-1 (c0_k o sr)^T built from the oracle's kernel, the factor the cov workspace holds,
the statistics of the draws, and a two-rank job against one rank."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from lcgp_amd import LCGP, synth
from lcgp_amd.engine import HotPathEngine
from oracle import lcgp_oracle as orc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _restated_sigma(m, x0s, k):
    """float64 numpy: C00 - D (c0 o sr) A^-1 (c0 o sr)^T with A = I + D (C o sr sr^T), the oracle's kernel"""
    xtr = (m.x_unique_s if m.submethod == 'rep' else m.x).numpy()
    sr = np.sqrt(m.r.numpy().astype(float)) if m.submethod == 'rep' else np.ones(xtr.shape[0])
    ell, scale, nug = m.lLmb.numpy()[k], m.lLmb0.numpy()[k], m.lnugGPs.numpy()[k]
    D = m.diag_D.numpy()[k]
    C = orc.matern32(xtr, xtr, ell, scale, nug, kernel=m.kernel) * sr[:, None] * sr[None, :]
    A = np.eye(xtr.shape[0]) + D * C
    c0 = orc.matern32(x0s, xtr, ell, scale, nug, kernel=m.kernel) * sr[None, :]
    c00 = orc.matern32(x0s, x0s, ell, scale, nug, kernel=m.kernel)
    low = np.linalg.cholesky(A)
    import scipy.linalg as sla
    u = sla.solve_triangular(low, c0.T, lower=True)
    return c00 - D * (u.T @ u), scale


def _model(mode, kernel, q=3):
    if mode == 'full':
        x, y = synth.make_full(51, 1000, 2, 4, q)
    else:
        x, y = synth.make_rep(52, 250, 4, 2, 4, q)
    m = LCGP(y=y, x=x, q=q, submethod=mode, kernel=kernel, device='cuda:0')
    o = orc.OracleLCGP(y=y, x=x, q=q, submethod=mode)
    m._set_flat(synth.param_points(51, o.get_unconstrained())[1])
    return m, x


@pytest.mark.parametrize('kernel', ['matern32', 'se'])
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_latent_and_joint_covariance_against_predict_and_numpy(mode, kernel):
    m, x = _model(mode, kernel)
    rng = np.random.default_rng(7)
    xr = x if mode == 'full' else m.x_unique.numpy()
    for n0 in (50, 128, 200):
        # the first rows are training inputs (their cross covariance has no nugget: x0 is not the training set)
        x0 = np.vstack([xr[:5], rng.uniform(0, 1, (n0 - 5, 2))])
        ypred, ypredvar, yconfvar = [t.numpy() for t in m.predict(x0)]
        gvar = m.gvar.numpy()
        lc = m.predict_latent_cov(x0).numpy()
        assert lc.shape == (m.q, n0, n0)
        x0s, same = m._standardise_x0(x0)
        assert not same
        for k in range(m.q):
            want, scale = _restated_sigma(m, x0s, k)
            assert np.max(np.abs(np.diag(lc[k]) - gvar[k])) <= 1e-12 * scale
            assert np.max(np.abs(lc[k] - want)) <= 1e-10 * scale, (n0, k, np.max(np.abs(lc[k] - want)) / scale)
        jc = m.predict_jointcov(x0).numpy()
        jc0 = m.predict_jointcov(x0, include_noise=False).numpy()
        np.testing.assert_allclose(np.diagonal(jc, axis1=1, axis2=2), ypredvar, rtol=1e-12)
        np.testing.assert_allclose(np.diagonal(jc0, axis1=1, axis2=2), yconfvar, rtol=1e-12)


def test_training_set_as_x0_and_the_factor_of_the_cov_workspace():
    m, x = _model('full', 'matern32', q=2)
    lc = m.predict_latent_cov(x).numpy()
    m.predict(x)
    x0s, same = m._standardise_x0(x)
    assert same
    for k in range(m.q):
        want, scale = _restated_sigma(m, x0s, k)
        assert np.max(np.abs(np.diag(lc[k]) - m.gvar.numpy()[k])) <= 1e-12 * scale
        assert np.max(np.abs(lc[k] - want)) <= 1e-10 * scale
    # the factor lcgp_potrf_logdet leaves in the cov workspace: L L^T = Sigma_k + tau_k I
    x0 = np.random.default_rng(9).uniform(0, 1, (300, 2))
    jit = 1e-8
    m.sample(x0, size=3, seed=1, jitter=jit)
    eng = m._aux_engine
    L = np.tril(eng.fetch_cov(300).cpu().numpy())
    sig = m.predict_latent_cov(x0).numpy()
    for k in range(m.q):
        tau = jit * m.lLmb0.numpy()[k]
        want = sig[k] + tau * np.eye(300)
        assert np.max(np.abs(L[k] @ L[k].T - want)) <= 1e-12 * np.max(np.abs(want))


def test_headline_shape_one_component():
    x, y, cfg = synth.make_config(3)
    m = LCGP(y=y[:8], x=x, q=1, device='cuda:0')
    x0 = np.random.default_rng(11).uniform(0, 1, (2000, cfg['d']))
    lc = m.predict_latent_cov(x0).numpy()
    m.predict(x0)
    x0s, _ = m._standardise_x0(x0)
    want, scale = _restated_sigma(m, x0s, 0)
    assert np.max(np.abs(np.diag(lc[0]) - m.gvar.numpy()[0])) <= 1e-12 * scale
    assert np.max(np.abs(lc[0] - want)) <= 1e-10 * scale


def test_sample_shape_seeds_and_statistics():
    x, y = synth.make_full(53, 200, 2, 3, 2)
    m = LCGP(y=y, x=x, q=2, device='cuda:0')
    o = orc.OracleLCGP(y=y, x=x, q=2)
    m._set_flat(synth.param_points(53, o.get_unconstrained())[1])
    x0 = np.random.default_rng(12).uniform(0, 1, (6, 2))
    s = m.sample(x0, size=4000, seed=123).numpy()
    assert s.shape == (4000, m.p, 6) and np.all(np.isfinite(s))
    np.testing.assert_array_equal(s, m.sample(x0, size=4000, seed=123).numpy())
    assert not np.array_equal(s[:10], m.sample(x0, size=10, seed=124).numpy())
    ypred = m.predict(x0)[0].numpy()
    jc = m.predict_jointcov(x0).numpy()
    se = np.sqrt(np.diagonal(jc, axis1=1, axis2=2) / 4000)
    assert np.all(np.abs(s.mean(axis=0) - ypred) <= 5 * se)
    for a in range(m.p):
        emp = np.cov(s[:, a, :], rowvar=False)
        sd = np.sqrt(np.diag(jc[a]))
        assert np.max(np.abs(emp - jc[a]) / np.outer(sd, sd)) <= 0.1
    assert m.sample(x0, size=3, seed=1, include_noise=False).shape == (3, m.p, 6)


def test_not_positive_definite_raises_and_jitter_repairs():
    # engine level, nugget exactly 0 (the model's nugget is clipped away from 0): 32 copies of one new input make
    # Sigma_k exactly singular, its factorisation meets non-positive pivots
    x, y = synth.make_full(54, 200, 1, 2, 1)
    e = HotPathEngine(x, y, q_local=1, kernel='se')
    rows = np.zeros((1, 1 + 3 + 2))
    rows[0, :4] = [0.5, 1.3, 0.0, 2.0]
    rows[0, 4:] = [0.3, -0.2]
    e.evaluate(rows)
    x0 = np.vstack([np.full((32, 1), 0.4), np.random.default_rng(1).uniform(0, 1, (8, 1))])
    with pytest.raises(np.linalg.LinAlgError, match='jitter=0') as ei:
        e.sample_latent(x0, 5, [(0, 0)], jitter=0.0)
    assert ei.value.info[0] != 0
    g = e.sample_latent(x0, 5, [(0, 0)], jitter=1e-6).cpu().numpy()
    assert np.all(np.isfinite(g))
    np.testing.assert_allclose(g[0, :, :32], np.repeat(g[0, :, :1], 32, axis=1), rtol=0, atol=1e-2)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_draw_and_cover_what_one_rank_does():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_joint_gpu_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout
