"""Gradient of the integrated variance reduction on the GPU (lcgp_variance_reduction_grad: OP_VG_P / OP_VG_G of the tile kernel,
vrg_sigma_kernel, pgrad_kernel with a matrix operand) against the float64 numpy closed form of tests/vr_grad_ref.py on a numpy
factorisation of A_k (tests/test_variance_reduction_grad_host.py ties that closed form to central differences); value bitwise
that of variance_reduction; bitwise-equal gradients on poisoned scratch, whatever the candidate chunking, and on two ranks;
float32 against float64; the headline shape against central differences of variance_reduction.

The bounds below are reasoned, not yet observed: no MI355X run of this file has been made."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from lcgp_amd import LCGP, synth
from lcgp_amd import engine as engine_mod
from oracle import lcgp_oracle as orc
from tests.vr_grad_ref import kern3, value_and_grad

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# max|dR - ref| / max|ref| per component against the float64 numpy closed form: predict_grad's bound
BOUND = 1e-10
# the headline shape against central differences (step FD_STEP of the range) of variance_reduction(latent=True): truncation
# (FD_STEP / lengthscale)^2 ~ 1e-6 at lengthscales of a tenth of the range, rounding 1e-10 (variance_reduction's accuracy) / FD_STEP
# = 1e-6, times five
FD_STEP = 1e-4
FD_BOUND = 1e-5


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
    eng = m._ensure_aux()
    x = (m.x_unique_s if m.submethod == 'rep' else m.x).numpy().astype(np.float64)
    s = np.sqrt(m.r.numpy().astype(float)) if m.submethod == 'rep' else np.ones(len(x))
    return eng._theta_last.copy(), x, s


def _numpy_ref(m, xr_s, xc_s, w, r):
    th, x, s = _state(m)
    d = x.shape[1]
    R = np.zeros((th.shape[0], len(xc_s)))
    dR = np.zeros((th.shape[0], len(xc_s), d))
    for k in range(th.shape[0]):
        ell, scale, nug, D = th[k, :d], th[k, d], th[k, d + 1], th[k, d + 2]
        # (the committed oracle knows two kernels: the training covariance is built here, for all three)
        nt = nug / (1.0 + nug)
        A = np.eye(len(x)) + D * scale * ((1.0 - nt) * kern3(x, x, ell, m.kernel) + nt * np.eye(len(x))) * np.outer(s, s)
        R[k], dR[k] = value_and_grad(th[k], np.linalg.cholesky(A), x, s, m.kernel, xr_s, xc_s, w, r)
    return R, dR


def _points(x, k, seed):
    lo, hi = x.min(axis=0), x.max(axis=0)
    return lo + (hi - lo) * np.random.default_rng(seed).random((k, x.shape[1]))


def _rng(m):
    return (m.x_max.numpy() - m.x_min.numpy()).reshape(-1)


@pytest.mark.parametrize('mode,kernel,d', [('full', 'matern32', 1), ('full', 'matern32', 2), ('rep', 'matern32', 2), ('full', 'se', 6),
                                           ('rep', 'se', 6), ('full', 'matern52', 2), ('rep', 'matern52', 6),
                                           ('full', 'matern32', 40), ('full', 'matern52', 40), ('rep', 'matern32', 6)])
def test_matches_float64_numpy(mode, kernel, d):
    m, x = _model(mode, kernel, d=d, n=360 if d == 40 else 480)
    xc = _points(x, 150, 1)
    xr = _points(x, 230, 2)
    w = np.random.default_rng(3).random(len(xr))
    worst = 0.0
    for r in ((1, 3) if mode == 'rep' else (1,)):
        for ref, ww in ((None, None), (xr, w)):
            R, dR = (a.numpy() for a in m.variance_reduction_grad(xc, x_ref=ref, weights=ww, replicates=r, latent=True))
            xc_s = m._standardise_x0(xc)[0]
            xr_s = xc_s if ref is None else m._standardise_x0(ref)[0]
            wn = np.full(len(xr_s), 1.0 / len(xr_s)) if ww is None else ww / ww.sum()
            ref_R, ref_dR = _numpy_ref(m, xr_s, xc_s, wn, r)
            ref_dR = ref_dR / _rng(m)[None, None, :]
            assert dR.shape == (3, len(xc), d) and np.all(np.isfinite(dR))
            assert np.array_equal(R, m.variance_reduction(xc, x_ref=ref, weights=ww, replicates=r, latent=True).numpy())
            for k in range(3):
                err = np.max(np.abs(dR[k] - ref_dR[k])) / np.max(np.abs(ref_dR[k]))
                errR = np.max(np.abs(R[k] - ref_R[k])) / np.max(np.abs(ref_R[k]))
                print('vr_grad err mode=%s kernel=%s d=%d r=%d shared=%s k=%d: dR %.3e R %.3e' % (mode, kernel, d, r, ref is None, k, err,
                                                                                                   errR))
                worst = max(worst, err)
    assert worst <= BOUND, (mode, kernel, d, worst)


def test_outputs_map_and_rep_match_gets_the_continuous_surface():
    m, x = _model('rep', 'matern32')
    xu = m.x_unique.numpy()
    xc = np.vstack([_points(x, 5, 4), xu[[3, 50]]])
    xr = _points(x, 60, 5)
    R, dR = (a.numpy() for a in m.variance_reduction_grad(xc, x_ref=xr, replicates=2, latent=True))
    Rv = m.variance_reduction(xc, x_ref=xr, replicates=2, latent=True).numpy()
    assert np.array_equal(R[:, :5], Rv[:, :5])
    assert not np.array_equal(R[:, 5:], Rv[:, 5:])          # the matched candidates: a new input there, not more replicates
    xr_s, xc_s = m._standardise_x0(xr)[0], m._standardise_x0(xc)[0]
    ref_R, ref_dR = _numpy_ref(m, xr_s, xc_s, np.full(60, 1.0 / 60), 2)
    assert np.max(np.abs(R - ref_R)) <= BOUND * np.max(np.abs(ref_R))
    assert np.max(np.abs(dR - ref_dR / _rng(m)[None, None, :])) <= BOUND * np.max(np.abs(ref_dR / _rng(m)[None, None, :]))
    W, _, scale, _ = m._output_map()
    g, dg = (a.numpy() for a in m.variance_reduction_grad(xc, x_ref=xr, replicates=2, outputs=[2, 0]))
    np.testing.assert_allclose(g, ((scale ** 2)[:, None] * ((W ** 2).T @ R))[[2, 0]], rtol=1e-13)
    np.testing.assert_allclose(dg, ((scale ** 2)[:, None, None] * np.einsum('ka,kcl->acl', W ** 2, dR))[[2, 0]], rtol=1e-12, atol=0)


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_bitwise_on_poisoned_scratch_and_any_candidate_chunking(mode, monkeypatch):
    m, x = _model(mode)
    xc = _points(x, 300, 8)
    xr = _points(x, 200, 9)
    base_shared = m.variance_reduction_grad(xc, latent=True)[1].numpy()
    base_sep = m.variance_reduction_grad(xc, x_ref=xr, latent=True)[1].numpy()
    eng = m._ensure_aux()
    for v in (0x00, 0xFF, 0x5A):
        eng._scratch.fill_(v)
        assert np.array_equal(m.variance_reduction_grad(xc, latent=True)[1].numpy(), base_shared), v
        eng._scratch.fill_(v)
        assert np.array_equal(m.variance_reduction_grad(xc, x_ref=xr, latent=True)[1].numpy(), base_sep), v
    for chunk in (37, 128, 131):
        monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', chunk)
        eng._scratch.fill_(0x5A)
        assert np.array_equal(m.variance_reduction_grad(xc, latent=True)[1].numpy(), base_shared), chunk
        assert np.array_equal(m.variance_reduction_grad(xc, x_ref=xr, latent=True)[1].numpy(), base_sep), chunk


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_float32_against_float64(mode):
    m64, x = _model(mode)
    m32, _ = _model(mode, dtype='float32')
    xc = _points(x, 200, 10)
    xr = _points(x, 150, 11)
    a = m64.variance_reduction_grad(xc, x_ref=xr, latent=True)[1].numpy()
    b = m32.variance_reduction_grad(xc, x_ref=xr, latent=True)[1].numpy()
    assert np.all(np.isfinite(b))
    err = np.max(np.abs(a - b)) / np.max(np.abs(a))
    print('vr_grad float32 vs float64 mode=%s: %.3e' % (mode, err))
    assert err <= 2e-3, err


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_reproduce_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_vr_grad_gpu_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


def test_headline_shape_against_central_differences():
    x, y = synth.make_full(93, 4096, 6, 64, 8)
    m = LCGP(y=y, x=x, q=8, device='cuda:0')
    o = orc.OracleLCGP(y=y, x=x, q=8)
    m._set_flat(synth.param_points(93, o.get_unconstrained())[1])
    xn = np.asarray(x)
    xc = _points(xn, 2000, 12)
    ghat, gvar = m.ghat, m.gvar
    R, dR = (a.numpy() for a in m.variance_reduction_grad(xc, latent=True))
    assert m.ghat is ghat and m.gvar is gvar
    assert R.shape == (8, 2000) and dR.shape == (8, 2000, 6) and np.all(np.isfinite(dR))
    assert np.array_equal(R, m.variance_reduction(xc, latent=True).numpy())
    delta, ddelta = m.variance_reduction_grad(xc)
    assert ddelta.shape == (64, 2000, 6) and np.all(np.isfinite(ddelta.numpy()))
    # central differences of variance_reduction at 8 sampled candidates, the reference set (the 2000 candidates) held fixed
    idx = np.random.default_rng(13).choice(2000, 8, replace=False)
    hstep = FD_STEP * (xn.max(axis=0) - xn.min(axis=0))
    fd = np.zeros((8, 8, 6))
    for l in range(6):
        e = np.zeros(6)
        e[l] = hstep[l]
        up = m.variance_reduction(xc[idx] + e, x_ref=xc, latent=True).numpy()
        dn = m.variance_reduction(xc[idx] - e, x_ref=xc, latent=True).numpy()
        fd[:, :, l] = (up - dn) / (2 * hstep[l])
    worst = 0.0
    for k in range(8):
        err = np.max(np.abs(dR[k, idx] - fd[k])) / np.max(np.abs(dR[k]))
        print('vr_grad headline k=%d: central-difference error %.3e of max|dR|' % (k, err))
        worst = max(worst, err)
    assert worst <= FD_BOUND, worst
