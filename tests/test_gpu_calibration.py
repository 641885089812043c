"""The calibration target on the GPU (lcgp_calib_rows, LCGP.calibration): the row kernel alone on synthetic inputs against the
np.longdouble evaluation of the same formulas (both kernel paths, every edge the formulas have: gvar = 0 and slightly negative,
a rank-deficient M, rows in strided blocks, no gradient, no sensitivities), bitwise independence of how the rows are split and
of what the outputs held; then the model: the log likelihood against the dense p-space density from the GPU's own predict(),
its gradient against central differences of that density, a float32 model, two ranks against one, the headline shape."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from lcgp_amd import LCGP, _hip, synth
from lcgp_amd.engine import calib_rows_device
from tests import calib_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps
N0, D = 257, 6                                  # the synthetic block every smaller case is a part of
DEV = 'cuda:0'


def _inputs(q, deficient):
    """ghat, gvar (q, N0), dghat, dgvar (q, N0, D), M = A^T A (rank q // 2 when deficient), b, c0, lognorm, inv_range.  Rows
    0..5 carry the edges: gvar exactly 0 in every component (0), in some (1, 2), slightly negative (3, 4), ghat = 0 (5)."""
    rng = np.random.default_rng(1000 * q + deficient)
    r = max(1, q // 2) if deficient else q + 3
    A = rng.standard_normal((r, q)) / np.sqrt(r)
    M = A.T @ A
    M = 0.5 * (M + M.T)
    ghat, gvar = rng.standard_normal((q, N0)), rng.uniform(0.0, 1.0, (q, N0))
    gvar[:, 0] = 0.0
    gvar[::2, 1] = 0.0
    gvar[q // 2:, 2] = 0.0
    gvar[:, 3] = -1e-18
    gvar[::3, 4] = -1e-18
    ghat[:, 5] = 0.0
    dghat, dgvar = rng.standard_normal((q, N0, D)), rng.standard_normal((q, N0, D))
    return dict(ghat=ghat, gvar=gvar, dghat=dghat, dgvar=dgvar, M=M, b=rng.standard_normal(q), c0=float(rng.uniform(1, 5)),
                lognorm=float(rng.standard_normal()), inv_range=rng.uniform(0.2, 4.0, D))


_CACHE = {}


def _reference(q, deficient):
    """(inputs, float64 reference, longdouble reference, tolerances) of the whole synthetic block: computed once, only read"""
    key = (q, deficient)
    if key not in _CACHE:
        inp = _inputs(q, deficient)
        args = (inp['ghat'], inp['gvar'], inp['dghat'], inp['dgvar'], inp['M'], inp['b'], inp['c0'], inp['lognorm'], inp['inv_range'])
        r64, rld = ref.rows(*args), ref.rows(*args, dtype=np.longdouble)
        _CACHE[key] = (inp, r64, rld, ref.row_tolerances(r64, rld))
    return _CACHE[key]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float64)).to(DEV)


def _p(t, off=0):
    return C.c_void_p(0 if t is None else t.data_ptr() + 8 * off)


def _run(inp, q, n0, d, row0=0, grad=True, sens=True, fill=0x00, unit_range=False):
    """lcgp_calib_rows on rows row0 .. row0 + n0 of the block, read in place (in_stride = N0 > n0), with the first d input
    dimensions; outputs pre-filled with the byte `fill`.  Returns numpy (ll, dll, s, v)."""
    lib = _hip.load()
    dg, dv = inp['dghat'], inp['dgvar']
    if d != D:                                  # d < D: the Jacobians of the first d dimensions, packed
        dg, dv = dg[:, :, :d], dv[:, :, :d]
    t = {k: _dev(v) for k, v in (('ghat', inp['ghat']), ('gvar', inp['gvar']), ('dghat', dg), ('dgvar', dv), ('M', inp['M']),
                                 ('b', inp['b']), ('ir', inp['inv_range'][:d]))}
    ll = torch.empty(n0, dtype=torch.float64, device=DEV)
    dll = torch.empty((n0, d), dtype=torch.float64, device=DEV) if grad else None
    sv = torch.empty((2, q, n0), dtype=torch.float64, device=DEV) if sens else None
    for o in (ll, dll, sv):
        if o is not None:
            o.view(torch.uint8).fill_(fill)
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    _hip.check(lib.lcgp_calib_rows(st, q, d, n0, _p(t['ghat'], row0), _p(t['gvar'], row0),
                                   _p(t['dghat'] if grad else None, row0 * d), _p(t['dgvar'] if grad else None, row0 * d), N0,
                                   _p(t['M']), _p(t['b']), inp['c0'], inp['lognorm'], _p(None if unit_range else t['ir']),
                                   _p(ll), _p(dll), _p(sv)), 'lcgp_calib_rows')
    torch.cuda.synchronize()
    sv = None if sv is None else sv.cpu().numpy()
    return ll.cpu().numpy(), None if dll is None else dll.cpu().numpy(), None if sv is None else sv[0], None if sv is None else sv[1]


def _check(got, rld, tol, rows, d, what):
    ll, dll, s, v = got
    for name, g, want, t in (('ll', ll, rld['ll'][rows], tol['ll'][rows]), ('s', s, rld['s'][:, rows], tol['s'][:, rows]),
                             ('v', v, rld['v'][:, rows], tol['v'][:, rows]),
                             ('dll', dll, rld['dll'][rows, :d], tol['dll'][rows, :d])):
        if g is None:
            continue
        assert np.all(np.isfinite(g)), (what, name)
        err = np.abs(g.astype(np.longdouble) - want)
        worst = np.unravel_index(np.argmax(err / t), err.shape)
        print('%s %s: largest error / tolerance %.3g' % (what, name, float(err[worst] / t[worst])))
        assert np.all(err <= t), (what, name, worst, float(err[worst]), float(t[worst]))


@pytest.mark.parametrize('deficient', [False, True], ids=['full-rank', 'rank-deficient'])
@pytest.mark.parametrize('q', [1, 2, 8, 9, 17, 64])
def test_row_kernel_against_longdouble(q, deficient):
    inp, r64, rld, tol = _reference(q, int(deficient))
    for n0 in (1, 63, 64, 65, 257):
        for d in (1, 6):
            got = _run(inp, q, n0, d)
            _check(got, rld, tol, slice(0, n0), d, 'q=%d n0=%d d=%d' % (q, n0, d))
            if d == 1:
                continue
            # the no-gradient form (NULL Jacobians) and the form without sensitivities: the same bits in what remains
            ll0 = _run(inp, q, n0, d, grad=False, sens=False)[0]
            ll1, dll1, _, _ = _run(inp, q, n0, d, sens=False)
            ll2, _, s2, v2 = _run(inp, q, n0, d, grad=False)
            assert np.array_equal(ll0, got[0]) and np.array_equal(ll1, got[0]) and np.array_equal(ll2, got[0])
            assert np.array_equal(dll1, got[1]) and np.array_equal(s2, got[2]) and np.array_equal(v2, got[3])
    # inv_range = NULL means ones
    unit, ranged = _run(inp, q, 65, 6, unit_range=True), _run(inp, q, 65, 6)
    assert np.array_equal(unit[0], ranged[0]) and np.array_equal(inp['inv_range'][None, :] * unit[1], ranged[1])


@pytest.mark.parametrize('q', [1, 8, 9, 64])
def test_rows_are_bitwise_independent_of_the_split_and_of_the_outputs_content(q):
    inp = _reference(q, 0)[0]
    whole = _run(inp, q, N0, D, fill=0x00)
    for fill in (0xFF, 0x5A):
        again = _run(inp, q, N0, D, fill=fill)
        for a, b in zip(whole, again):
            assert np.array_equal(a, b), fill
    cut = 100
    first, second = _run(inp, q, cut, D, fill=0xFF), _run(inp, q, N0 - cut, D, row0=cut, fill=0x5A)
    assert np.array_equal(np.concatenate([first[0], second[0]]), whole[0])
    assert np.array_equal(np.concatenate([first[1], second[1]]), whole[1])
    for w in (2, 3):
        assert np.array_equal(np.concatenate([first[w], second[w]], axis=1), whole[w])


# ------------------------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------------------------
def _dense(m, theta, y_obs, obs_var):
    """(ll, cond, quad, logdet) per row of theta from the dense p-space density: mean and covariance from the GPU's own
    predict(theta, return_fullcov=True) plus Sigma_obs (full path), from the latent prediction through _output_map (rep)"""
    y = np.asarray(y_obs, float)
    obs = ~np.isnan(y)
    n0 = theta.shape[0]
    if m.submethod == 'full':
        ypred, _, _, cov = [t.numpy() for t in m.predict(theta, return_fullcov=True)]
        S = np.asarray(obs_var, float)
        S = S * np.eye(len(y)) if S.ndim == 0 else (np.diag(S) if S.ndim == 1 else S)
        sig = cov[:, obs][:, :, obs] + S[np.ix_(obs, obs)][None]
        res = (y[:, None] - ypred)[obs]
    else:
        ghat, gvar = m._latent_predict(theta)
        _, phi_s, t, lam = ref.observation(m, y_obs, obs_var)
        sig = np.einsum('ak,ki,bk->iab', phi_s, np.maximum(gvar, 0.0), phi_s) + lam[None]
        res = t[:, None] - phi_s @ ghat
    ll, cond, quad, logdet = (np.zeros(n0) for _ in range(4))
    for i in range(n0):
        low = np.linalg.cholesky(sig[i])
        z = np.linalg.solve(low, res[:, i])
        quad[i], logdet[i], cond[i] = z @ z, 2.0 * np.sum(np.log(np.diag(low))), np.linalg.cond(sig[i])
        ll[i] = -0.5 * (quad[i] + logdet[i] + obs.sum() * ref.LOG2PI)
    return ll, cond, quad, logdet


def _central_differences(fn, theta, h):
    out = np.zeros(theta.shape)
    for l in range(theta.shape[1]):
        e = np.zeros_like(theta)
        e[:, l] = h[l]
        out[:, l] = (fn(theta + e) - fn(theta - e)) / (2 * h[l])
    return out


@pytest.mark.parametrize('name', list(ref.MODEL_CASES))
def test_loglik_and_gradient_against_the_dense_density_of_predict(name):
    m, x, y = ref.model_case(name)
    p = int(m.p)
    for form, drop in (('dense', None), ('diag', 2), ('scalar', None)):
        theta, y_obs, obs_var = ref.case_observation(name, x, y, form)
        if drop is not None:
            y_obs = y_obs.copy()
            y_obs[drop] = np.nan
        tgt = m.calibration(y_obs, obs_var)
        ll = tgt.loglik(theta).numpy()
        want, cond, quad, logdet = _dense(m, theta, y_obs, obs_var)
        assert np.all(cond <= 1e6), cond.max()
        tol = 64 * p * EPS * cond * (np.abs(quad) + np.abs(logdet) + p)
        print('%s %s: largest loglik error / tolerance %.3g' % (name, form, np.max(np.abs(ll - want) / tol)))
        assert np.all(np.abs(ll - want) <= tol), (form, np.max(np.abs(ll - want) / tol))
        ll2, dll = [t.numpy() for t in tgt.loglik_grad(theta)]
        assert np.array_equal(ll2, ll)
        if form == 'scalar':
            continue
        fd = _central_differences(lambda th: _dense(m, th, y_obs, obs_var)[0], theta, 1e-5 * (x.max(0) - x.min(0)))
        err = np.max(np.abs(dll - fd)) / np.max(np.abs(fd))
        print('%s %s: gradient error %.3g of the largest entry' % (name, form, err))
        assert err <= 1e-6, (form, err)


def test_float32_model_row_kernel_on_its_own_latent_blocks():
    """a float32 model's engine writes ghat, gvar, dghat, dgvar in double: the float64 row kernel on them against the
    longdouble formulas fed with the same arrays, at the row kernel's tolerance"""
    name = 'full-matern32-q3'
    m, x, y = ref.model_case(name, dtype='float32')
    theta, y_obs, obs_var = ref.case_observation(name, x, y, 'dense')
    tgt = m.calibration(y_obs, obs_var)
    eng = m._ensure_aux()
    assert eng.dtype_name == 'float32'
    blk, jac = eng.predict_grad_block(m._x0_2d(theta, 'theta'))
    M, b, inv_range = tgt._device_consts(blk.device)
    ll, dll, sens = [t.cpu().numpy() for t in calib_rows_device(blk, jac, M, b, tgt.c0, tgt.lognorm, inv_range, True)]
    args = (blk[0].cpu().numpy(), blk[1].cpu().numpy(), jac[0].cpu().numpy(), jac[1].cpu().numpy(), tgt.M, tgt.b, tgt.c0,
            tgt.lognorm, inv_range.cpu().numpy())
    r64, rld = ref.rows(*args), ref.rows(*args, dtype=np.longdouble)
    _check((ll, dll, sens[0], sens[1]), rld, ref.row_tolerances(r64, rld), slice(0, 17), 3, 'float32 model')
    got = tgt.loglik_grad(theta, latent=True)
    for a, b_ in zip(got, (ll, dll, sens[0], sens[1])):
        assert np.array_equal(a.numpy(), b_)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_equal_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_calibration_gpu_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


def test_loglik_differentiable_on_the_device():
    name = 'rep-se-q3'
    m, x, y = ref.model_case(name)
    theta, y_obs, obs_var = ref.case_observation(name, x, y, 'diag')
    tgt = m.calibration(y_obs, obs_var)
    tt = torch.tensor(theta[:4], dtype=torch.float64, device=DEV, requires_grad=True)
    out = tgt.loglik_differentiable(tt)
    assert out.device == tt.device and torch.equal(out.cpu(), tgt.loglik(theta[:4]))
    out.sum().backward()
    assert tt.grad.device == tt.device and torch.equal(tt.grad.cpu(), tgt.loglik_grad(theta[:4])[1])
    with pytest.raises(RuntimeError, match='double backward'):
        torch.autograd.grad(tgt.loglik_differentiable(tt).sum(), tt, create_graph=True)


def test_headline_shape():
    """n = 4096, d = 6, p = 64, q = 8, n0 = 2000: the whole call, then central differences of the dense density on three rows"""
    x, y, cfg = synth.make_config(3)
    m = LCGP(y=y, x=x, q=cfg['q'], device=DEV)
    rng = np.random.default_rng(12)
    theta = rng.uniform(0, 1, (2000, cfg['d']))
    sd = y.std(axis=1)
    y_obs = y[:, 100] + 0.1 * sd * rng.standard_normal(cfg['p'])
    obs_var = (0.1 * sd) ** 2
    tgt = m.calibration(y_obs, obs_var)
    ll, dll = [t.numpy() for t in tgt.loglik_grad(theta)]
    assert ll.shape == (2000,) and dll.shape == (2000, cfg['d']) and np.all(np.isfinite(ll)) and np.all(np.isfinite(dll))
    assert np.array_equal(tgt.loglik(theta).numpy(), ll)
    rows = [0, 517, 1999]
    fd = _central_differences(lambda th: _dense(m, th, y_obs, obs_var)[0], theta[rows], 1e-5 * (x.max(0) - x.min(0)))
    err = np.max(np.abs(dll[rows] - fd)) / np.max(np.abs(fd))
    print('headline: gradient error %.3g of the largest entry' % err)
    assert err <= 1e-6, err
