"""Input gradients of the prediction on the GPU (lcgp_predict_grad, LCGP.predict_grad / predict_differentiable): the latent
Jacobians against a float64 numpy restatement from the oracle's kernel and np.linalg solves, the output Jacobians against
central differences of the GPU predict(), ghat / gvar bitwise those of lcgp_predict, independence of the scratch content,
float32 against float64, two ranks against one, the headline shape, and gradcheck through torch.autograd."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from lcgp_amd import LCGP, synth
from lcgp_amd.engine import PREDICT_CHUNK
from oracle import lcgp_oracle as orc
from tests.test_predict_grad_host import latent_jacobians

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _model(mode, kernel, d, n=300, q=2, dtype='float64', seed=81, span=None):
    """n = 300 (full) / 150 unique inputs (rep): neither a multiple of 64; span: raw inputs = 1 + span * synthetic inputs"""
    if mode == 'full':
        x, y = synth.make_full(seed, n, d, 3, q)
    else:
        x, y = synth.make_rep(seed, n // 2, 3, d, 3, q)
    if span is not None:
        x = 1.0 + span * x
    m = LCGP(y=y, x=x, q=q, submethod=mode, kernel=kernel, device='cuda:0', dtype=dtype)
    o = orc.OracleLCGP(y=y, x=x, q=q, submethod=mode)
    m._set_flat(synth.param_points(seed, o.get_unconstrained())[1])
    return m, x


def _restated(m, eng, x0s):
    """(ghat, gvar, Jm, Jv) per local component, float64 numpy: A_k = I + D_k (C_k o sr sr^T) from the oracle's kernel,
    its Cholesky factor from np.linalg, z_k = A_k^-1 (Y^T psi_k) -- the engine's theta rows and inputs, nothing else"""
    x, Y = eng.x.cpu().numpy().astype(np.float64), eng.Y.cpu().numpy().astype(np.float64)
    sr = np.ones(eng.n) if eng.sr is None else eng.sr.cpu().numpy().astype(np.float64)
    d = eng.d
    res = []
    for th in eng._theta_last:
        ell, scale, nug, D, psi = th[:d], th[d], th[d + 1], th[d + 2], th[d + 3:]
        C = orc.matern32(x, x, ell, scale, nug, kernel=m.kernel) * sr[:, None] * sr[None, :]
        low = np.linalg.cholesky(np.eye(eng.n) + D * C)
        z = np.linalg.solve(low.T, np.linalg.solve(low, Y.T @ psi))
        res.append(latent_jacobians(x0s, x, sr, th, low, z, m.kernel))
    return res


@pytest.mark.parametrize('d', [1, 6, 40])
@pytest.mark.parametrize('kernel', ['matern32', 'se'])
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_latent_jacobians_against_numpy(mode, kernel, d):
    m, x = _model(mode, kernel, d)
    eng = m._ensure_aux()
    xtr = (m.x_unique_s if mode == 'rep' else m.x).numpy()
    rng = np.random.default_rng(d)
    sizes = (1, 63, 128, 200) + ((PREDICT_CHUNK + 52,) if (mode, kernel, d) == ('full', 'matern32', 6) else ())
    for n0 in sizes:
        x0s = rng.uniform(0, 1, (n0, d))
        if n0 > 3:
            x0s[:3] = xtr[[0, 7, 11]]                           # training inputs: no nugget, the continuous surface
        blk, jac = [t.cpu().numpy() for t in eng.predict_grad_block(x0s)]
        want = _restated(m, eng, x0s)
        for k, (gh, gv, jm, jv) in enumerate(want):
            for got, ref, what in ((blk[0, k], gh, 'ghat'), (blk[1, k], gv, 'gvar'), (jac[0, k], jm, 'dghat'),
                                   (jac[1, k], jv, 'dgvar')):
                err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
                # fp64 throughout; the GPU works from the explicit inverse factor W = L^-1 (error ~ cond(A) eps)
                assert err <= 1e-10, (what, n0, k, err)


def _central_differences(m, x0, h):
    n0, d = x0.shape
    out = np.zeros((3, int(m.p), n0, d))
    for l in range(d):
        e = np.zeros_like(x0)
        e[:, l] = h[l]
        plus, minus = m.predict(x0 + e), m.predict(x0 - e)
        for w in range(3):
            out[w, :, :, l] = (plus[w].numpy() - minus[w].numpy()) / (2 * h[l])
    return out


@pytest.mark.parametrize('kernel', ['matern32', 'se'])
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_predict_grad_against_central_differences_of_predict(mode, kernel):
    m, x = _model(mode, kernel, 3, span=np.array([5.0, 0.25, 1.0]))        # a non-unit input range, different per dimension
    lo, hi = x.min(0), x.max(0)
    x0 = lo + (hi - lo) * np.random.default_rng(2).uniform(0.05, 0.95, (17, 3))
    got = [t.numpy() for t in m.predict_grad(x0)]
    fd = _central_differences(m, x0, 1e-5 * (hi - lo))
    for g, f in zip(got, fd):
        assert g.shape == (3, 17, 3)
        assert np.max(np.abs(g - f)) <= 1e-6 * np.max(np.abs(f)), np.max(np.abs(g - f)) / np.max(np.abs(f))


def test_outputs_bitwise_predict_and_independent_of_scratch_content():
    m, x = _model('full', 'matern32', 6)
    eng = m._ensure_aux()
    x0s = np.random.default_rng(9).uniform(0, 1, (200, 6))
    ref = eng.predict_block(x0s, False).cpu().numpy()
    first = None
    for fill in (0x00, 0xFF, 0x5A):
        eng._scratch.fill_(fill)
        blk, jac = [t.cpu().numpy() for t in eng.predict_grad_block(x0s)]
        assert np.array_equal(blk, ref), fill
        if first is None:
            first = jac
        assert np.array_equal(jac, first), fill
        assert np.all(np.isfinite(jac))


def test_float32_model_against_float64():
    """float32 stores x, the factors, U and V in float32 (the contraction accumulates in double): the Jacobians carry the
    float32 factorisation's error (unit roundoff 6e-8) amplified by the conditioning of A, a well-conditioned small problem
    here; 2e-3 of the largest entry leaves margin over that, as the float32 gradient of the NLL is held to 1e-3
    (tests/test_gpu_edge_cases.py)"""
    m64, x = _model('full', 'matern32', 4)
    m32, _ = _model('full', 'matern32', 4, dtype='float32')
    x0 = np.random.default_rng(10).uniform(0, 1, (150, 4))
    for a, b in zip(m32.predict_grad(x0), m64.predict_grad(x0)):
        err = np.max(np.abs(a.numpy() - b.numpy())) / np.max(np.abs(b.numpy()))
        assert err <= 2e-3, err


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_equal_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_predict_grad_gpu_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


def test_headline_shape_against_central_differences():
    """n = 4096, d = 6, q = 8, n0 = 2000: the whole call, then central differences of predict() on a sample of rows"""
    x, y, cfg = synth.make_config(3)
    m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0')
    x0 = np.random.default_rng(11).uniform(0, 1, (2000, cfg['d']))
    dyp, dypv, dycv = [t.numpy() for t in m.predict_grad(x0)]
    assert dyp.shape == (cfg['p'], 2000, cfg['d']) and np.all(np.isfinite(dyp)) and np.all(np.isfinite(dycv))
    rows = [0, 517, 1999]
    fd = _central_differences(m, x0[rows], np.full(cfg['d'], 1e-5))
    for g, f in zip((dyp, dypv, dycv), fd):
        assert np.max(np.abs(g[:, rows] - f)) <= 1e-6 * np.max(np.abs(f)), np.max(np.abs(g[:, rows] - f)) / np.max(np.abs(f))


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_predict_differentiable_gradcheck(mode):
    m, x = _model(mode, 'matern32', 2, n=120)
    x0 = np.random.default_rng(12).uniform(0.1, 0.9, (4, 2))
    outs = m.predict_differentiable(torch.as_tensor(x0))
    for a, b in zip(outs, m.predict(x0)):
        assert torch.equal(a, b)
    for dev in ('cpu', 'cuda:0'):
        xt = torch.tensor(x0, dtype=torch.float64, device=dev, requires_grad=True)
        for w in range(3):
            assert torch.autograd.gradcheck(lambda t: m.predict_differentiable(t)[w], (xt,), eps=1e-6, atol=1e-6, rtol=1e-4)
        yp = m.predict_differentiable(xt)[0]
        assert yp.device == xt.device
        yp.sum().backward()
        assert xt.grad.device == xt.device and torch.all(torch.isfinite(xt.grad))
