"""CPU tests of the gradient of the integrated variance reduction (LCGP.variance_reduction_grad /
variance_reduction_differentiable): the numpy closed form of tests/vr_grad_ref.py against central differences of the closed
form of R in tests/test_variance_reduction_host.py; the host layer -- standardisation (chain rule), the output map, the
every-candidate-is-new rule, autograd, the gather over ranks -- through a numpy stand-in of
HotPathEngine.variance_reduction_grad_block; and the argument checks and scratch size of the new C entries
(tests/test_gpu_variance_reduction_grad.py runs the same through liblcgp_hip.so)."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from lcgp_amd import LCGP, synth
from oracle import lcgp_oracle as orc
from tests import matern52_oracle as m52
from tests import test_variance_reduction_host as vrh
from tests.test_variance_reduction_host import closed_form, patch_vr
from tests.vr_grad_ref import VrGradOracleEngine, kern3, value_and_grad

HERE = os.path.dirname(os.path.abspath(__file__))


def _problem(kernel, rep, d, seed):
    """one component at random parameters: theta row, chol(I + D (C o s s^T)), inputs in the unit box, replicate scaling"""
    rng = np.random.default_rng(seed)
    n = 30
    x = rng.random((n, d))
    ell = 0.3 + rng.random(d)
    scale, nug, D = 1.7, 0.02, 40.0
    th = np.r_[ell, scale, nug, D]
    s = np.sqrt(rng.integers(1, 5, n).astype(float)) if rep else np.ones(n)
    nt = nug / (1.0 + nug)
    C0 = scale * ((1 - nt) * kern3(x, x, ell, kernel) + nt * np.eye(n))
    low = np.linalg.cholesky(np.eye(n) + D * C0 * np.outer(s, s))
    return th, low, x, s, rng


@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
@pytest.mark.parametrize('rep', [False, True])
@pytest.mark.parametrize('d', [1, 2, 6])
def test_closed_form_gradient_equals_central_differences_of_the_closed_form(kernel, rep, d, monkeypatch):
    # (the existing closed form knows two kernels: its correlation function is given the third)
    monkeypatch.setattr(vrh, '_kern', kern3)
    th, low, x, s, rng = _problem(kernel, rep, d, 100 + d)
    xc = rng.random((7, d))
    xc[0, 0] = x[3, 0]                              # a candidate coordinate equal to a training coordinate
    xr_w = rng.random((9, d))
    xr_w[2, d - 1] = xc[1, d - 1]                   # ... and one equal to a reference coordinate
    for r in (1, 3):
        for xr, w in ((xr_w, rng.random(9) + 0.1), (None, None)):
            ref = xc.copy() if xr is None else xr       # the default set: a COPY of the candidates, held constant
            ww = np.full(len(ref), 1.0 / len(ref)) if w is None else w / w.sum()
            R, dR = value_and_grad(th, low, x, s, kernel, ref, xc, ww, r)
            np.testing.assert_allclose(R, closed_form(th, low, x, s, kernel, ref, xc, ww, None, r), rtol=1e-12)
            fd = np.zeros_like(dR)
            h = 1e-6
            for l in range(d):
                e = np.zeros(d)
                e[l] = h
                fd[:, l] = (closed_form(th, low, x, s, kernel, ref, xc + e, ww, None, r)
                            - closed_form(th, low, x, s, kernel, ref, xc - e, ww, None, r)) / (2 * h)
            assert np.max(np.abs(dR - fd)) <= 1e-5 * np.max(np.abs(dR)), np.max(np.abs(dR - fd)) / np.max(np.abs(dR))


def _model(mode, kernel='matern32', group=None):
    """inputs with a different non-unit range per dimension: the chain rule through the standardisation counts"""
    if mode == 'full':
        x, y = synth.make_full(41, 40, 2, 3, 3)
    else:
        x, y = synth.make_rep(42, 40, 3, 2, 4, 4)
    x = np.asarray(x) * np.array([3.0, 0.25]) + np.array([-1.0, 5.0])
    m = patch_vr(LCGP(y=y, x=x, submethod=mode, kernel=kernel, process_group=group), VrGradOracleEngine)
    o = orc.OracleLCGP(y=y, x=x, submethod=mode)
    m._set_flat(synth.param_points(41, o.get_unconstrained())[1])
    return m, x


def _box(x, rng, k):
    lo, hi = x.min(axis=0), x.max(axis=0)
    return lo + (hi - lo) * rng.random((k, x.shape[1]))


@pytest.mark.parametrize('mode,kernel', [('full', 'matern32'), ('rep', 'matern32'), ('full', 'se'), ('rep', 'matern52')])
def test_public_gradient_equals_central_differences_of_variance_reduction(mode, kernel, monkeypatch):
    if kernel == 'matern52':
        m52.patch(monkeypatch)          # the committed oracle knows two kernels: the stand-in's factorisation needs the third
    m, x = _model(mode, kernel)
    rng = np.random.default_rng(5)
    xc, xr = _box(x, rng, 6), _box(x, rng, 9)
    w = rng.random(9) + 0.1
    r = 3 if mode == 'rep' else 1
    for kw in (dict(latent=True), dict(), dict(outputs=[2, 0])):
        gain, dgain = m.variance_reduction_grad(xc, x_ref=xr, weights=w, replicates=r, **kw)
        val = m.variance_reduction(xc, x_ref=xr, weights=w, replicates=r, **kw)
        assert gain.dtype == torch.float64 and dgain.dtype == torch.float64
        assert dgain.shape == tuple(gain.shape) + (2,)
        np.testing.assert_allclose(gain.numpy(), val.numpy(), rtol=1e-12)
        fd = np.zeros(dgain.shape)
        for l in range(2):
            e = np.zeros(2)
            e[l] = 1e-6 * (x[:, l].max() - x[:, l].min())
            fd[:, :, l] = (m.variance_reduction(xc + e, x_ref=xr, weights=w, replicates=r, **kw).numpy()
                           - m.variance_reduction(xc - e, x_ref=xr, weights=w, replicates=r, **kw).numpy()) / (2 * e[l])
        dg = dgain.numpy()
        assert np.max(np.abs(dg - fd)) <= 1e-5 * np.max(np.abs(dg)), np.max(np.abs(dg - fd)) / np.max(np.abs(dg))
    full = m.variance_reduction_grad(xc, x_ref=xr, weights=w, replicates=r)[1].numpy()
    np.testing.assert_array_equal(m.variance_reduction_grad(xc, x_ref=xr, weights=w, replicates=r, outputs=[2, 0])[1].numpy(), full[[2, 0]])


def test_value_equality_and_the_continuous_surface_at_a_matching_candidate():
    m, x = _model('rep')
    rng = np.random.default_rng(6)
    xu = m.x_unique.numpy()
    xc = np.vstack([_box(x, rng, 3), xu[[4, 17]]])
    xr = _box(x, rng, 8)
    R, dR = (a.numpy() for a in m.variance_reduction_grad(xc, x_ref=xr, replicates=2, latent=True))
    Rv = m.variance_reduction(xc, x_ref=xr, replicates=2, latent=True).numpy()
    np.testing.assert_array_equal(R[:, :3], Rv[:, :3])
    # at a unique training input: the value of a NEW input there (no nugget in its cross row), not more replicates of that input
    eng = m._aux_engine
    xs = m._standardise_x0(xc)[0]
    for i, (th, low, _, _) in enumerate(eng._state):
        new = closed_form(th, low, eng.x, eng.sr, 'matern32', m._standardise_x0(xr)[0], xs, np.full(8, 0.125), None, 2)
        np.testing.assert_allclose(R[i], new, rtol=1e-12)
    assert np.all(np.abs(R[:, 3:] - Rv[:, 3:]) > 1e-6 * np.abs(Rv[:, 3:]))
    # ... and the gradient is that surface's: central differences through the matching point
    for l in range(2):
        e = np.zeros(2)
        e[l] = 1e-6 * (x[:, l].max() - x[:, l].min())
        fd = (m.variance_reduction(xc[3:] + e, x_ref=xr, replicates=2, latent=True).numpy()
              - m.variance_reduction(xc[3:] - e, x_ref=xr, replicates=2, latent=True).numpy()) / (2 * e[l])
        assert np.max(np.abs(dR[:, 3:, l] - fd)) <= 1e-5 * np.max(np.abs(dR))
    # the full path: replicates must be 1, as in variance_reduction
    mf, xf = _model('full')
    with pytest.raises(ValueError, match='full path'):
        mf.variance_reduction_grad(xf[:3] + 0.01, replicates=2)
    with pytest.raises(ValueError, match='x_cand'):
        mf.variance_reduction_grad(np.zeros((3, 3)))


def test_autograd_gradcheck_no_double_backward_and_constant_reference_copy():
    m, x = _model('full')
    rng = np.random.default_rng(7)
    xr = _box(x, rng, 7)
    xc = torch.tensor(_box(x, rng, 4), requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: m.variance_reduction_differentiable(t, x_ref=xr), (xc,), eps=1e-6, atol=1e-7, rtol=1e-5,
                                    nondet_tol=0.0)
    assert torch.autograd.gradcheck(lambda t: m.variance_reduction_differentiable(t, x_ref=xr, latent=True, weights=np.arange(1.0, 8.0)),
                                    (xc,), eps=1e-6, atol=1e-7, rtol=1e-5)
    out = m.variance_reduction_differentiable(xc, x_ref=xr)
    assert out.shape == (int(m.p), 4) and out.requires_grad
    with pytest.raises(RuntimeError, match='first derivatives only'):
        torch.autograd.grad(out.sum(), xc, create_graph=True)
    # x_ref=None: the reference set is a COPY of the candidates -- the engine is told so, and nothing flows through the copy:
    # the gradient is the one with the same points passed as an explicit constant x_ref
    eng = m._aux_engine
    eng.grad_calls = []
    a = m.variance_reduction_differentiable(xc)
    (ga,) = torch.autograd.grad(a.sum(), xc)
    b = m.variance_reduction_differentiable(xc, x_ref=xc.detach().numpy().copy())
    (gb,) = torch.autograd.grad(b.sum(), xc)
    assert eng.grad_calls == [True, False]
    np.testing.assert_allclose(ga.numpy(), gb.numpy(), rtol=1e-12, atol=0)
    dg = m.variance_reduction_grad(xc.detach().numpy())[1]
    np.testing.assert_allclose(ga.numpy(), dg.sum(dim=0).numpy(), rtol=1e-12)
    # no preceding evaluation is spent and ghat / gvar stay
    m.predict(xr[:2])
    ghat, gvar = m.ghat, m.gvar
    m.variance_reduction_grad(xr[:3])
    assert m.ghat is ghat and m.gvar is gvar


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_gather_what_one_rank_computes():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_vr_grad_host_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


def test_c_abi_argument_checks_and_scratch_size():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() >= 590
    assert 'lcgp_variance_reduction_grad' in _hip.SIGNATURES and 'lcgp_variance_reduction_grad_scratch_bytes' in _hip.SIGNATURES
    nb = C.c_size_t(0)

    def sb(n, d, q, nr, nc, dtype=0):
        assert lib.lcgp_variance_reduction_grad_scratch_bytes(dtype, n, d, q, nr, nc, C.byref(nb)) == 0, lib.lcgp_last_error()
        return nb.value

    sizes = [sb(4096, 6, 8, 2000, nc) for nc in (1, 37, 64, 128, 131, 1000, 2048, 4096)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    vr = C.c_size_t(0)
    assert lib.lcgp_variance_reduction_scratch_bytes(0, 4096, 8, 2000, 2048, C.byref(vr)) == 0
    # beyond the variance reduction's own: S (n_cand x n_ref), G / V and Q (n_cand x n each), three (n_cand, d) double blocks
    extra = 8 * 8 * 2048 * (2048 + 2 * 4096) + 3 * 8 * 8 * 2048 * 6
    assert 0 <= sb(4096, 6, 8, 2000, 2048) - vr.value - extra <= 4096
    assert sb(4096, 6, 8, 2000, 2048, 1) < sb(4096, 6, 8, 2000, 2048)
    for args, msg in (((0, 4096, 6, 8, 0, 10), b'n_ref'), ((0, 4096, 6, 8, 10, 0), b'n_cand'), ((0, 4096, 127, 8, 10, 10), b'd must be'),
                      ((2, 4096, 6, 8, 10, 10), b'dtype'), ((0, 4096, 6, 8, 10, 70000), b'n_cand must be <=')):
        assert lib.lcgp_variance_reduction_grad_scratch_bytes(*args, C.byref(nb)) < 0, args
        assert msg in lib.lcgp_last_error(), (args, lib.lcgp_last_error())
    assert lib.lcgp_variance_reduction_grad_scratch_bytes(0, 4096, 6, 8, 10, 10, None) < 0

    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything

    def vg(n=50, d=2, nr=10, nc=4, row0=-1, r=1, xc=dummy, out_stride=0, dtype=0, kern=0, w=dummy, dout=dummy, xr=dummy):
        return lib.lcgp_variance_reduction_grad(None, dtype, kern, n, d, 3, 2, dummy, None, dummy, dummy, nr, xr, w, nc, xc, row0, r,
                                                dummy, dummy, out_stride, dout)

    cases = [(dict(nr=0), 'n_ref'), (dict(nc=0), 'n_cand'), (dict(nc=70000), 'n_cand must be <='), (dict(r=0), 'r must be'),
             (dict(d=127), 'd must be'), (dict(d=0), 'd must be'), (dict(dtype=2), 'dtype'), (dict(kern=3), 'kernel_id'),
             (dict(row0=-2), 'cand_row0'), (dict(row0=8, nc=4), 'cand_row0 + n_cand'), (dict(row0=0, xc=dummy), 'x_cand must be NULL'),
             (dict(xc=None), 'NULL'), (dict(w=None), 'NULL'), (dict(dout=None), 'NULL'), (dict(xr=None), 'NULL'),
             (dict(out_stride=3), 'out_stride')]
    for kw, msg in cases:
        assert vg(**kw) < 0, kw
        assert msg.encode() in lib.lcgp_last_error(), (kw, lib.lcgp_last_error())
