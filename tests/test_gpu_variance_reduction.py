"""Integrated variance reduction on the GPU (lcgp_variance_reduction_prepare / lcgp_variance_reduction: OP_VR of the tile
kernel) against float64 numpy: the closed form on a numpy factorisation of A_k, brute force (augment the training set,
refactor, predict) and a HotPathEngine conditioned on the augmented data through its own predict_block; bitwise-equal
results on poisoned scratch, whatever the candidate chunking, and on two ranks; float32 against float64; the headline shape."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from lcgp_amd import LCGP, synth
from lcgp_amd import engine as engine_mod
from lcgp_amd.engine import HotPathEngine
from oracle import lcgp_oracle as orc
from tests.test_variance_reduction_host import closed_form, gvar_at

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _model(mode, kernel='matern32', q=3, dtype='float64', n=480, d=2, p=4):
    if mode == 'full':
        x, y = synth.make_full(91, n, d, p, q)
    else:
        x, y = synth.make_rep(92, n // 3, 3, d, p, q)
    m = LCGP(y=y, x=x, q=q, submethod=mode, kernel=kernel, device='cuda:0', dtype=dtype)
    o = orc.OracleLCGP(y=y, x=x, q=q, submethod=mode)
    m._set_flat(synth.param_points(91, o.get_unconstrained())[1])
    return m, np.asarray(x)


def _state(m):
    """theta rows, standardised training inputs and replicate scaling of the model's factorisation, in float64"""
    eng = m._ensure_aux()
    x = (m.x_unique_s if m.submethod == 'rep' else m.x).numpy().astype(np.float64)
    s = np.sqrt(m.r.numpy().astype(float)) if m.submethod == 'rep' else np.ones(len(x))
    return eng._theta_last.copy(), x, s


def _numpy_R(m, xr_s, xc_s, w, match, r):
    th, x, s = _state(m)
    d = x.shape[1]
    out = np.zeros((th.shape[0], len(xc_s)))
    for k in range(th.shape[0]):
        ell, scale, nug, D = th[k, :d], th[k, d], th[k, d + 1], th[k, d + 2]
        A = np.eye(len(x)) + D * orc.matern32(x, x, ell, scale, nug, kernel=m.kernel) * np.outer(s, s)
        out[k] = closed_form(th[k], np.linalg.cholesky(A), x, s, m.kernel, xr_s, xc_s, w, match, r)
    return out


def _points(x, k, seed):
    lo, hi = x.min(axis=0), x.max(axis=0)
    return lo + (hi - lo) * np.random.default_rng(seed).random((k, x.shape[1]))


def _match(m, xc_s):
    xt = m._x_train()
    return np.array([int(np.flatnonzero(np.all(xt == c[None, :], axis=1))[0]) if np.any(np.all(xt == c[None, :], axis=1)) else -1
                     for c in xc_s])


@pytest.mark.parametrize('mode,kernel,d', [('full', 'matern32', 2), ('rep', 'matern32', 2), ('full', 'se', 6), ('rep', 'se', 6),
                                           ('full', 'matern32', 40), ('rep', 'matern32', 6)])
def test_matches_float64_numpy(mode, kernel, d):
    m, x = _model(mode, kernel, d=d, n=360 if d == 40 else 480)
    xc = _points(x, 150, 1)
    if mode == 'rep':
        xc = np.vstack([xc, m.x_unique.numpy()[[0, 7, 33]]])
    xr = _points(x, 230, 2)
    w = np.random.default_rng(3).random(len(xr))
    for r in ((1, 3) if mode == 'rep' else (1,)):
        for ref, ww in ((None, None), (xr, w)):
            R = m.variance_reduction(xc, x_ref=ref, weights=ww, replicates=r, latent=True).numpy()
            xc_s = m._standardise_x0(xc)[0]
            xr_s = xc_s if ref is None else m._standardise_x0(ref)[0]
            wn = np.full(len(xr_s), 1.0 / len(xr_s)) if ww is None else ww / ww.sum()
            match = _match(m, xc_s) if mode == 'rep' else None
            if mode == 'rep':
                assert np.sum(match >= 0) == 3
            ref_R = _numpy_R(m, xr_s, xc_s, wn, match, r)
            gv = m._ensure_aux().predict_block(xr_s)[1].cpu().numpy()
            assert np.all(np.isfinite(R)) and np.all(R >= -1e-12 * gv.max())
            err = np.max(np.abs(R - ref_R)) / gv.max()
            assert err <= 1e-10, (mode, kernel, d, r, err)


def test_rep_matches_and_replicates_against_brute_force_and_a_conditioned_engine():
    m, x = _model('rep', 'matern32')
    th, xt, s = _state(m)
    xr = _points(x, 120, 4)
    xc = np.vstack([_points(x, 2, 5), m.x_unique.numpy()[[3, 50]]])
    r = 3
    R = m.variance_reduction(xc, x_ref=xr, replicates=r, latent=True).numpy()
    xr_s, xc_s = m._standardise_x0(xr)[0], m._standardise_x0(xc)[0]
    w = np.full(len(xr), 1.0 / len(xr))
    gv0 = m._ensure_aux().predict_block(xr_s)[1].cpu().numpy()
    scale = gv0.max()
    rr = s * s
    for j, c in enumerate(xc_s):
        hit = np.flatnonzero(np.all(xt == c[None, :], axis=1))
        if len(hit):
            x2, r2 = xt, rr.copy()
            r2[hit[0]] += r
        else:
            x2, r2 = np.vstack([xt, c]), np.r_[rr, r]
        # numpy brute force
        for k in range(th.shape[0]):
            bf = w @ (gvar_at(th[k], xt, s, m.kernel, xr_s) - gvar_at(th[k], x2, np.sqrt(r2), m.kernel, xr_s))
            assert abs(R[k, j] - bf) <= 1e-10 * scale, (j, k, R[k, j], bf)
        # the library's own predict on the augmented data
        aug = HotPathEngine(x2, np.zeros((int(m.p), len(x2))), np.sqrt(r2), q_local=th.shape[0], kernel=m.kernel)
        aug.evaluate(th)
        gv1 = aug.predict_block(xr_s)[1].cpu().numpy()
        np.testing.assert_allclose(R[:, j], (gv0 - gv1) @ w, rtol=0, atol=1e-10 * scale)


def test_full_path_against_a_conditioned_engine():
    m, x = _model('full', 'se', d=6)
    th, xt, _ = _state(m)
    xr = _points(x, 100, 6)
    xc = np.vstack([_points(x, 2, 7), x[[5]]])          # a training input too: a new row, no nugget in its cross row
    R = m.variance_reduction(xc, x_ref=xr, latent=True).numpy()
    xr_s, xc_s = m._standardise_x0(xr)[0], m._standardise_x0(xc)[0]
    gv0 = m._ensure_aux().predict_block(xr_s)[1].cpu().numpy()
    for j, c in enumerate(xc_s):
        aug = HotPathEngine(np.vstack([xt, c]), np.zeros((int(m.p), len(xt) + 1)), None, q_local=th.shape[0], kernel='se')
        aug.evaluate(th)
        gv1 = aug.predict_block(xr_s)[1].cpu().numpy()
        np.testing.assert_allclose(R[:, j], (gv0 - gv1).mean(axis=1), rtol=0, atol=1e-10 * gv0.max())


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_bitwise_on_poisoned_scratch_and_any_candidate_chunking(mode, monkeypatch):
    m, x = _model(mode)
    xc = _points(x, 300, 8)
    if mode == 'rep':
        xc = np.vstack([xc[:100], m.x_unique.numpy()[:40], xc[100:]])
    xr = _points(x, 200, 9)
    base_shared = m.variance_reduction(xc, latent=True).numpy()
    base_sep = m.variance_reduction(xc, x_ref=xr, latent=True).numpy()
    eng = m._ensure_aux()
    for v in (0x00, 0xFF, 0x5A):
        eng._scratch.fill_(v)
        assert np.array_equal(m.variance_reduction(xc, latent=True).numpy(), base_shared), v
        eng._scratch.fill_(v)
        assert np.array_equal(m.variance_reduction(xc, x_ref=xr, latent=True).numpy(), base_sep), v
    for chunk in (37, 128, 131):
        monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', chunk)
        eng._scratch.fill_(0x5A)
        assert np.array_equal(m.variance_reduction(xc, latent=True).numpy(), base_shared), chunk
        assert np.array_equal(m.variance_reduction(xc, x_ref=xr, latent=True).numpy(), base_sep), chunk


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_float32_against_float64(mode):
    m64, x = _model(mode)
    m32, _ = _model(mode, dtype='float32')
    xc = _points(x, 200, 10)
    xr = _points(x, 150, 11)
    a = m64.variance_reduction(xc, x_ref=xr, latent=True).numpy()
    b = m32.variance_reduction(xc, x_ref=xr, latent=True).numpy()
    gv = m64._ensure_aux().predict_block(m64._standardise_x0(xr)[0])[1].cpu().numpy()
    # float32 products (U from the float32 factor), double sums: stated tolerance 2e-3 of the largest latent variance
    assert np.all(np.isfinite(b))
    assert np.max(np.abs(a - b)) <= 2e-3 * gv.max(), np.max(np.abs(a - b)) / gv.max()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_reproduce_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_vr_gpu_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


def test_headline_shape_runs():
    x, y = synth.make_full(93, 4096, 6, 64, 8)
    m = LCGP(y=y, x=x, q=8, device='cuda:0')
    o = orc.OracleLCGP(y=y, x=x, q=8)
    m._set_flat(synth.param_points(93, o.get_unconstrained())[1])
    xc = _points(np.asarray(x), 2000, 12)
    R = m.variance_reduction(xc, latent=True).numpy()
    gv = m._ensure_aux().predict_block(m._standardise_x0(xc)[0])[1].cpu().numpy()
    assert R.shape == (8, 2000) and np.all(np.isfinite(R))
    assert np.all(R >= 0) and np.all(R <= gv.mean(axis=1)[:, None] + 1e-9 * gv.max())
    delta = m.variance_reduction(xc).numpy()
    assert delta.shape == (64, 2000) and np.all(np.isfinite(delta)) and np.all(delta >= 0)
