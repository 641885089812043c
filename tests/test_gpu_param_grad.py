"""GPU tests of the parameter derivatives of the prediction (lcgp_predict_paramgrad, LCGP.predict_param_grad / predict_laplace):
the latent outputs against the float64 numpy restatement of tests/param_grad_ref.py (tied to autograd and to the oracle by
tests/test_param_grad_host.py), ghat / gvar against lcgp_predict, independence of the scratch content, of the grouping and of
the chunk size, two ranks against one, predict_param_grad against central differences of the GPU's own predict, and
predict_laplace end to end.

Observed on the MI355X, worst over every case of test_latent_outputs_against_numpy (largest entry per block as the scale): ghat
9.9e-14, gvar 1.2e-13, dghat 1.2e-13, dgvar 8.7e-15, dnoise 8.0e-14 -- inside the first-order bar of 1e-10 (LATENT_BAR).  ghat /
gvar against predict_block, scratch content, grouping and chunking: equal to the bit.  predict_param_grad against central
differences of predict: dypred 2.0e-7, dypredvar 2.4e-9, dyconfvar 5.0e-8 (bar 1e-6).  yparamvar against the dense quadratic
form: 9.5e-16 (bar 1e-11)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import lcgp_amd.engine as engine_mod
from lcgp_amd import LCGP, synth
from oracle import lcgp_oracle as orc
from tests import param_grad_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# float64: the project's first-order bar (the same W = L^-1, error ~ cond(A) eps), relative to the largest entry per block
LATENT_BAR = 1e-10
NAMES = ('ghat', 'gvar', 'dghat', 'dgvar', 'dnoise')


def _model(mode, kernel, d, n=300, q=2, p=3, dtype='float64', seed=81):
    """n = 300 (full) / 150 unique inputs (rep): neither a multiple of 64"""
    if mode == 'full':
        x, y = synth.make_full(seed, n, d, p, q)
    else:
        x, y = synth.make_rep(seed, n // 2, 3, d, p, q)
    m = LCGP(y=y, x=x, q=q, submethod=mode, kernel=kernel, device='cuda:0', dtype=dtype)
    o = orc.OracleLCGP(y=y, x=x, q=q, submethod=mode)
    m._set_flat(synth.param_points(seed, o.get_unconstrained())[1])
    return m, x


def _blocks(res):
    """the engine's (block, dk, dn) as the five numpy arrays of NAMES, component first"""
    blk, dk, dn = (t.cpu().numpy() for t in res)
    return blk[0], blk[1], dk[0], dk[1], dn


def _restated(eng, kernel, x0s, same):
    x, Y = eng.x.cpu().numpy(), eng.Y.cpu().numpy()
    sr = None if eng.sr is None else eng.sr.cpu().numpy()
    res = [ref.latent(x0s, same, x, Y, sr, th, kernel) for th in eng._theta_last]
    return [np.stack([r[i] for r in res]) for i in range(5)]


def _check(got, want, tag, worst):
    for g, w, what in zip(got, want, NAMES):
        assert g.shape == w.shape, what
        err = float(np.max(np.abs(g - w)) / np.max(np.abs(w)))
        worst[what] = max(worst.get(what, 0.0), err)
        assert err <= LATENT_BAR, (what, tag, err)


@pytest.mark.parametrize('d', [1, 6, 17])
@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_latent_outputs_against_numpy(monkeypatch, mode, kernel, d):
    """64- and 128-row tiles and a ragged last tile; d = 17 takes two dimension blocks of the row kernel (16 per block); one
    call with x0 the training set (the nugget entry), one with the chunk size forced below n0"""
    m, x = _model(mode, kernel, d)
    eng = m._ensure_aux()
    xtr = (m.x_unique_s if mode == 'rep' else m.x).numpy()
    rng = np.random.default_rng(d)
    worst = {}
    for n0 in (1, 63, 128, 200):
        x0s = rng.uniform(0, 1, (n0, d))
        if n0 > 3:
            x0s[:3] = xtr[[0, 7, 11]]
        _check(_blocks(eng.predict_paramgrad_block(x0s)), _restated(eng, kernel, x0s, False), n0, worst)
    _check(_blocks(eng.predict_paramgrad_block(xtr, same=True)), _restated(eng, kernel, xtr, True), 'same', worst)
    monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', 64)
    _check(_blocks(eng.predict_paramgrad_block(xtr, same=True)), _restated(eng, kernel, xtr, True), 'same, chunked', worst)
    print('worst', mode, kernel, d, ' '.join('%s %.1e' % kv for kv in worst.items()))


@pytest.mark.parametrize('mode,kernel,d', [('full', 'matern32', 6), ('rep', 'matern52', 17)])
def test_ghat_gvar_are_those_of_predict(mode, kernel, d):
    m, x = _model(mode, kernel, d)
    eng = m._ensure_aux()
    xtr = (m.x_unique_s if mode == 'rep' else m.x).numpy()
    for x0s, same in ((np.random.default_rng(2).uniform(0, 1, (63, d)), False), (np.random.default_rng(3).uniform(0, 1, (200, d)), False),
                      (xtr, True)):
        want = eng.predict_block(x0s, same).cpu().numpy()
        got = eng.predict_paramgrad_block(x0s, same)[0].cpu().numpy()
        for g, w in zip(got, want):
            err = float(np.max(np.abs(g - w)) / np.max(np.abs(w)))
            print('ghat / gvar against predict_block', mode, len(x0s), same, err)
            assert err <= 1e-13


@pytest.mark.parametrize('mode,kernel,d', [('full', 'matern52', 6), ('rep', 'matern32', 17)])
def test_result_does_not_depend_on_scratch_content_grouping_or_chunking(monkeypatch, mode, kernel, d):
    m, x = _model(mode, kernel, d)
    eng = m._ensure_aux()
    x0s = np.random.default_rng(9).uniform(0, 1, (200, d))
    want = _blocks(eng.predict_paramgrad_block(x0s))
    for fill in (0x00, 0xFF, 0x5A):                  # zeros, NaN (all bits set), 0x5A
        eng._scratch.fill_(fill)
        for g, w in zip(_blocks(eng.predict_paramgrad_block(x0s)), want):
            assert np.all(np.isfinite(g)) and np.array_equal(g, w), fill
    eng._scratch.fill_(0xFF)
    for g, w, what in zip(_blocks(eng.predict_paramgrad_block(x0s, q_group=1)), want, NAMES):      # one component per call
        assert np.array_equal(g, w), what
    monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', 128)                   # 128 + 72 rows against 200 at once
    for g, w, what in zip(_blocks(eng.predict_paramgrad_block(x0s)), want, NAMES):
        err = float(np.max(np.abs(g - w)) / np.max(np.abs(w)))
        print('chunked against unchunked', what, err)
        assert err <= 1e-13, what


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_reproduce_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_param_grad_gpu_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


_fd = {}


def _fd_case(mode):
    """(float64 model, u, x0, central differences of the GPU's own predict over the unconstrained vector), once per mode"""
    x, y = synth.make_full(7, 200, 2, 4, 3) if mode == 'full' else synth.make_rep(7, 66, 3, 2, 4, 3)
    m = LCGP(y=y, x=x, q=3, submethod=mode, device='cuda:0')
    u = synth.param_points(7, orc.OracleLCGP(y=y, x=x, q=3, submethod=mode).get_unconstrained())[1]
    x0 = x[:1] + (x[3:20] - x[:1]) * 0.61
    if mode not in _fd:
        fd = [np.empty((4, len(x0), len(u))) for _ in range(3)]
        for i in range(len(u)):
            h = 1e-5 * max(1.0, abs(u[i]))
            e = np.zeros_like(u)
            e[i] = h
            m._set_flat(u + e)
            up = [t.numpy() for t in m.predict(x0)]
            m._set_flat(u - e)
            dn = [t.numpy() for t in m.predict(x0)]
            for b in range(3):
                fd[b][:, :, i] = (up[b] - dn[b]) / (2.0 * h)
        for f in fd:
            f.setflags(write=False)
        _fd[mode] = fd
    m._set_flat(u)
    return m, u, x, y, x0, _fd[mode]


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_predict_param_grad_matches_central_differences_of_predict(mode):
    m, u, x, y, x0, fd = _fd_case(mode)
    got_u = [t.numpy() for t in m.predict_param_grad(x0)]
    jac = m._flat_jacobians()[0]
    got_c = [t.numpy() for t in m.predict_param_grad(x0, space='constrained')]
    for g, gc, f, what in zip(got_u, got_c, fd, ('dypred', 'dypredvar', 'dyconfvar')):
        err = float(np.max(np.abs(g - f)) / np.max(np.abs(f)))
        errc = float(np.max(np.abs(gc * jac - f)) / np.max(np.abs(f)))
        print(mode, what, 'against central differences: unconstrained %.2e constrained %.2e' % (err, errc))
        assert err <= 1e-6 and errc <= 1e-6, what
    # a float32 model gives the float64 answer
    m32 = LCGP(y=y, x=x, q=3, submethod=mode, device='cuda:0', dtype='float32')
    m32.phi, m32.g, m32.diag_D = m.phi.clone(), m.g.clone(), m.diag_D.clone()
    m32._set_flat(u)
    for a, b in zip(m32.predict_param_grad(x0), got_u):
        np.testing.assert_array_equal(a.numpy(), b)
    assert m32._dtype == 'float32' and not m32._float64_only


def test_predict_laplace_end_to_end():
    x, y = synth.make_full(3, 60, 2, 4, 2)
    m = LCGP(y=y, x=x, q=2, device='cuda:0')
    m.fit()
    x0 = x[:1] + (x[2:40] - x[:1]) * 0.43
    base = [t.numpy().copy() for t in m.predict(x0)]
    assert m._aux_valid
    yp, ypv, ycv, pv = (t.numpy() for t in m.predict_laplace(x0))
    assert np.all(pv >= 0) and pv.shape == base[0].shape
    np.testing.assert_array_equal(yp, base[0])
    np.testing.assert_array_equal(ypv, base[1] + pv)
    np.testing.assert_array_equal(ycv, base[2] + pv)
    J = m.predict_param_grad(x0)[0].numpy()
    want = np.einsum('aip,pq,aiq->ai', J, m.laplace().cov, J)
    err = float(np.max(np.abs(pv - want)) / np.max(np.abs(want)))
    print('yparamvar against the dense quadratic form: %.2e; largest share of ypredvar %.3f' % (err, float(np.max(pv / ypv))))
    assert err <= 1e-11
    zero = m.predict_laplace(x0, cov=np.zeros((J.shape[2], J.shape[2])))
    for got, w in zip(zero[:3], base):
        np.testing.assert_array_equal(got.numpy(), w)
    assert np.all(zero[3].numpy() == 0.0)
    for a, b in zip(m.predict(x0), base):             # the workspace is only read
        np.testing.assert_array_equal(a.numpy(), b)
