"""GPU tests of the Hessian of the objective in the parameters (lcgp_nll_hess, LCGP.loss_hessian / laplace) against the torch
autograd reference of tests/nll_hess_ref.py (tied to the oracle by tests/test_nll_hess_host.py).

Accuracy bound: 10 x max(eps_ref, 1e-12) = 1e-11 of the largest entry per block type, eps_ref ~ 2e-15 being the deviation of the
CPU closed form from autograd (tests/test_nll_hess_host.py) and the factor 10 covering the different summation order of tiles.
Observed on the MI355X (first run, the shapes below): kernel blocks <= 2.1e-15, border <= 6.6e-15, noise corner <= 8.6e-16.
The cases at d = 5 and d = 9 tie the block-pair and chunk arithmetic that d <= 2 never reaches end to end; entry by entry it is
checked stage-wise in tests/test_gpu_param_bounds.py."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from lcgp_amd import LCGP, _hip, synth
from oracle import lcgp_oracle as orc
from tests import matern52_oracle as m52
from tests import nll_hess_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BOUND = 10.0 * max(2.3e-15, 1e-12)
Q = 3

# (mode, kernel, n, d, diag_error_structure): n = 200 ragged last 64-tile; 128 exact tiles; 330 crosses a 128-tile edge
CASES = [('full', 'matern32', 200, 2, None), ('full', 'se', 200, 2, None), ('full', 'matern52', 200, 2, None),
         ('rep', 'matern32', 200, 2, None), ('full', 'matern32', 128, 2, None), ('full', 'matern32', 330, 2, None),
         ('full', 'matern32', 200, 1, None), ('full', 'matern32', 200, 2, [1, 3]),
         # two and three blocks of four dimensions, m = d + 2 = 7 and 11 (two chunks of j in the trace reduction)
         ('full', 'matern52', 130, 5, None), ('rep', 'se', 130, 9, None)]
_cache = {}


def _case(mode, kernel, n, d, es, dtype='float64'):
    """(model, flat unconstrained point, autograd Hessian in the constrained parameters): the reference is computed once per case"""
    key = (mode, kernel, n, d, None if es is None else tuple(es))
    x, y = synth.make_full(7, n, d, 4, Q) if mode == 'full' else synth.make_rep(7, n // 3, 3, d, 4, Q)
    kw = dict(q=Q, submethod=mode, kernel=kernel, diag_error_structure=es)
    m = LCGP(y=y, x=x, device='cuda:0', dtype=dtype, **kw)
    if key not in _cache:
        with m52.patched():
            o = orc.OracleLCGP(y=y, x=x, **kw)
            o.phi = m.phi.numpy().copy()
            u = synth.param_points(7, o.get_unconstrained())[1]
            o.set_unconstrained(u)
        H = ref.hessian(ref.flat_constrained(o), ref.problem(o))
        H.setflags(write=False)
        _cache[key] = (u, H)
    return (m,) + _cache[key]


@pytest.mark.parametrize('mode,kernel,n,d,es', CASES)
def test_constrained_hessian_matches_autograd(mode, kernel, n, d, es):
    m, u, Href = _case(mode, kernel, n, d, es)
    H = m.loss_hessian(u, space='constrained')
    assert H.shape == Href.shape and H.dtype == np.float64
    errs = ref.block_errors(H, Href, Q, d)
    print('max |H - H_ref| / max |H_ref| per block type:', errs)
    assert max(errs.values()) <= BOUND, errs
    np.testing.assert_array_equal(H, H.T)
    idx = ref.kernel_index(Q, d)
    for a in range(Q):
        for b in range(a):
            assert np.all(H[np.ix_(idx[a], idx[b])] == 0.0)


@pytest.mark.parametrize('mode,kernel,n,d,es', [CASES[0], CASES[3], CASES[7]])
def test_unconstrained_hessian_matches_central_differences_of_loss_and_grad(mode, kernel, n, d, es):
    m, u, _ = _case(mode, kernel, n, d, es)
    H = m.loss_hessian(u)
    fd = np.empty_like(H)
    for i in range(len(u)):
        h = 1e-5 * max(1.0, abs(u[i]))
        e = np.zeros_like(u)
        e[i] = h
        fd[:, i] = (m.loss_and_grad(u + e)[1] - m.loss_and_grad(u - e)[1]) / (2.0 * h)
    err = np.max(np.abs(H - fd)) / np.max(np.abs(fd))
    print('unconstrained Hessian vs central differences of loss_and_grad: %.2e' % err)
    assert err <= 1e-6
    np.testing.assert_array_equal(H, H.T)


def test_predict_is_untouched_and_the_workspace_stays_valid():
    m, u, _ = _case(*CASES[0])
    m.loss_and_grad(u)
    x0 = np.random.default_rng(1).uniform(0.05, 0.95, (17, 2))
    before = [t.numpy().copy() for t in m.predict(x0)]
    H = m.loss_hessian()
    assert m._aux_valid
    after = [t.numpy() for t in m.predict(x0)]
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(H, m.loss_hessian(u))          # reproducible bit for bit, evaluated at u or in place


@pytest.mark.parametrize('mode,kernel,n,d,es', [CASES[0], CASES[3]])
def test_result_does_not_depend_on_the_scratch_content_or_the_grouping(mode, kernel, n, d, es):
    m, u, _ = _case(mode, kernel, n, d, es)
    m.loss_and_grad(u)
    eng = m._aux_engine
    want = eng.nll_hess_block().cpu().numpy()
    for fill in (0, 0xFF, 0x5A):                     # zeros, NaN (all bits set), 0x5A
        eng._scratch.fill_(fill)
        np.testing.assert_array_equal(eng.nll_hess_block().cpu().numpy(), want)
    # one component per call (what the engine does when the free memory holds no more) against all three at once
    width = eng.lib.lcgp_nll_hess_width(eng.d, eng.p)
    out = torch.full((eng.q_local, width), float('nan'), dtype=torch.float64, device=eng.device)
    eng._scratch.fill_(0xFF)
    for k0 in range(eng.q_local):
        _hip.check(eng.lib.lcgp_nll_hess(eng._stream(), eng.dtype, eng.kernel_id, eng.n, eng.d, eng.p, eng.q_local, eng._p(eng.x),
                                         eng._p(eng.Y), eng._p(eng.sr), eng._p(eng.theta_dev), eng._p(eng.workspace), k0, 1,
                                         eng._p(eng._scratch), eng._p(out)), 'lcgp_nll_hess')
    np.testing.assert_array_equal(out.cpu().numpy(), want)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_reproduce_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_nll_hess_gpu_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


def test_float32_model_returns_the_float64_hessian_bitwise():
    m64, u, _ = _case(*CASES[0])
    m32 = _case(*CASES[0], dtype='float32')[0]
    m32.phi, m32.g, m32.diag_D = m64.phi.clone(), m64.g.clone(), m64.diag_D.clone()
    for space in ('constrained', 'unconstrained'):
        np.testing.assert_array_equal(m32.loss_hessian(u, space=space), m64.loss_hessian(u, space=space))
    assert m32._dtype == 'float32' and not m32._float64_only


def test_the_entry_refuses_float32():
    lib = _hip.load()
    dummy = C.c_void_p(16)          # never dereferenced: the call is refused before it enqueues anything
    rc = lib.lcgp_nll_hess(None, _hip.F32, 0, 100, 2, 3, 1, dummy, dummy, None, dummy, dummy, 0, 1, dummy, dummy)
    assert rc < 0 and b'float64 only' in lib.lcgp_last_error()


def test_laplace_after_fit():
    x, y = synth.make_full(3, 60, 2, 4, 2)
    m = LCGP(y=y, x=x, q=2, device='cuda:0')
    m.fit()
    res = m.laplace()
    print('eigenvalues %.3e .. %.3e' % (res.eigenvalues[0], res.eigenvalues[-1]))
    assert np.all(res.eigenvalues > 0)
    for se, par in zip(res.stderr, m.get_param()):
        assert tuple(se.shape) == tuple(par.shape) and bool(torch.all(torch.isfinite(se))) and bool(torch.all(se > 0))
    assert m._aux_valid
