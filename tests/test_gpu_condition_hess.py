"""Input Hessians and the gradient covariance of a conditioned view on the GPU (lcgp_condition_predict_hess /
lcgp_condition_predict_gradcov: the widened derivative rows P' = [P | Q / sqrt(D)], phess_cond_kernel, pgrad_cond_mean_kernel)
against dense float64 numpy on the augmented data and against a HotPathEngine built on the augmented data at the same theta
rows (its own predict_hess_block / grad_cov_block); central differences of the GPU view.predict_grad and gradgradcheck; the
device reduction M; float32; semantics (a far-away run, Gamma_base - Gamma' positive semidefinite); bitwise-equal results on
poisoned cond workspace, state, grad state and scratch, for one component against all, for any PREDICT_CHUNK and on two ranks;
the base model untouched; limits.

Shapes: n = 333 training inputs (no multiple of 64), q = 3, m in {1, 70, 150} (one short tile, across a 64 and a 128 boundary of
the second segment and of K'), n0 in {1, 130} (below and across 128 inputs and 32-row groups), d in {1, 6} (one partial 4 x 4
block; a full and a partial one), once d = 40 (WIDE; more than one 32-dimension chunk in pdx_kernel), once several passes
(PREDICT_CHUNK lowered), the three kernels, full and rep with 1 to 3 replicates.  Some rows of x0 equal training inputs and
some the view's own new inputs (same = 0: the continuous surface).

Bounds, float64: the rule of tests/test_gpu_condition.py -- per component and quantity 1e-10 of the largest |entry| of the dense
reference over the case's points.  Every case also measures the augmented engine (code this feature does not touch) against
the same dense reference: where the view exceeds the fixed bound, the admissible bound is 4 x the augmented engine's own error
on that case.  It is never derived from the view's numbers.  float32: against the float64 dense reference, bound 4 x the
error of the augmented engine of the same dtype on the same case.  Every case prints its figures before it asserts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from lcgp_amd import _hip
from lcgp_amd import engine as engine_mod
from lcgp_amd.engine import HotPathEngine
from tests import grad_cov_ref as gref
from tests.test_condition_host import new_columns
from tests.test_gpu_condition import CASES, _checksum, _engine_args, _filled, _model, _new_runs, _training
from tests.test_gpu_condition_grad import _box_model, _x0
from tests.test_gpu_variance_reduction import _free_port, _points
from tests.test_predict_hess_host import _cross, latent_hessians, pack_lower

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL64 = 1e-10
NAMES = ('ghat', 'gvar', 'dghat', 'dgvar', 'd2ghat', 'd2gvar', 'gamma')


def dense_second_order(m, xn, yn, x0s, step=16):
    """[ghat, gvar (q, n0), dghat, dgvar (q, n0, d), d2ghat, d2gvar, Gamma (q, n0, tri)] from first principles in float64
    numpy: the training set augmented by the new columns, A rebuilt and factorised at the theta rows, the formulas of
    lcgp_predict_hess and lcgp_predict_gradcov on the augmented matrix (same = 0), `step` points at a time"""
    x, s, Y = _training(m)
    xn_s, snew, ycol = new_columns(m, xn, yn)
    xa, sa, Ya = np.vstack([x, xn_s]), np.r_[s, snew], np.hstack([Y, ycol])
    d = xa.shape[1]
    out = [[] for _ in NAMES]
    for th in m._ensure_aux()._theta_last:
        ell, scale, nug, D, psi = th[:d], th[d], th[d + 1], th[d + 2], th[d + 3:]
        Cm = _cross(xa, xa, ell, scale, nug, m.kernel)
        Cm[np.arange(len(xa)), np.arange(len(xa))] = scale
        low = np.linalg.cholesky(np.eye(len(xa)) + D * Cm * np.outer(sa, sa))
        z = sla.cho_solve((low, True), Ya.T @ psi)
        parts = [[] for _ in NAMES]
        for lo in range(0, len(x0s), step):
            pts = x0s[lo:lo + step]
            res = list(latent_hessians(pts, xa, sa, th, low, z, m.kernel)) + [gref.latent_grad_cov(pts, xa, sa, th, low, m.kernel)]
            for acc, r, packed in zip(parts, res, (0, 0, 0, 0, 1, 1, 1)):
                acc.append(pack_lower(r) if packed else r)
        for acc, p in zip(out, parts):
            acc.append(np.concatenate(p))
    return [np.stack(o) for o in out]


def _augmented_engine(m, xn, yn, dtype='float64'):
    rows = m._ensure_aux()._theta_last.copy()
    x, s, Y = _training(m)
    xn_s, snew, ycol = new_columns(m, xn, yn)
    aug = HotPathEngine(np.vstack([x, xn_s]), np.hstack([Y, ycol]), None if m.submethod == 'full' else np.r_[s, snew],
                        q_local=len(rows), dtype=dtype, kernel=m.kernel)
    aug.evaluate(rows)
    return aug


def _engine_second_order(hess_block, grad_cov_block):
    """the seven quantities of NAMES as numpy arrays from the two block methods' results"""
    blk, jac, hess = [t.cpu().numpy() for t in hess_block]
    dghat, gamma, _ = grad_cov_block
    return [blk[0], blk[1], jac[0], jac[1], hess[0], hess[1], gamma.cpu().numpy()], dghat.cpu().numpy()


def _view_second_order(view, x0s):
    eng, st = view._engine, view._state
    return _engine_second_order(eng.condition_predict_hess_block(st, x0s), eng.condition_grad_cov_block(st, x0s))


def _errors(got, aug, dense, sl=slice(None)):
    """per quantity (view vs dense, augmented engine vs dense, view vs augmented engine), each the largest over the components
    of max |difference| / largest |entry| of the dense reference"""
    rows = []
    for g, a, r in zip(got, aug, dense):
        r = r[:, sl]
        assert g.shape == r.shape == a.shape and np.all(np.isfinite(g))
        unit = np.abs(r).reshape(len(r), -1).max(axis=1).reshape((-1,) + (1,) * (r.ndim - 1))
        rows.append([float(np.max(np.abs(u - v) / unit)) for u, v in ((g, r), (a, r), (g, a))])
    return rows


def _check(tag, got, aug, dense, sl=slice(None), floor=TOL64):
    bad = []
    for name, (ev, ea, ex) in zip(NAMES, _errors(got, aug, dense, sl)):
        bound = max(floor, 4 * ea)
        print('condition hess %s %s: view vs dense %.3e | augmented engine vs dense %.3e | view vs augmented engine %.3e | '
              'bound %.1e' % (tag, name, ev, ea, ex, bound))
        if not (ev <= bound and ex <= bound + ea):
            bad.append((name, ev, ea, ex, bound))
    assert not bad, (tag, bad)


def _case64(m, x, xn, yn, x0, sizes, tag):
    view = m.condition(xn, yn)
    x0s = m._standardise_x0(x0)[0]
    dense = dense_second_order(m, xn, yn, x0s)
    aug = _augmented_engine(m, xn, yn)
    for n0 in sizes:
        got, dghat = _view_second_order(view, x0s[:n0])
        ref, _ = _engine_second_order(aug.predict_hess_block(x0s[:n0]), aug.grad_cov_block(x0s[:n0]))
        _check('%s n0=%d' % (tag, n0), got, ref, dense, slice(0, n0))
        blk, jac = [t.cpu().numpy() for t in view._engine.condition_predict_grad_block(view._state, x0s[:n0])]
        assert np.array_equal(got[0], blk[0]) and np.array_equal(got[1], blk[1])
        assert np.array_equal(got[2], jac[0]) and np.array_equal(got[3], jac[1]) and np.array_equal(dghat, jac[0])
    return view


@pytest.mark.parametrize('mode,kernel,d,k', CASES)
def test_view_second_order_matches_dense_numpy_on_the_augmented_data(mode, kernel, d, k):
    m, x = _model(mode, kernel, d)
    xn, yn = _new_runs(m, x, k, 3)
    view = _case64(m, x, xn, yn, _x0(x, xn, 130), (1, 130), '%s %s d=%d m=%d' % (mode, kernel, d, k))
    # the host layer on the GPU engine: shapes, exact symmetry, the latent tensors are the engine's blocks mirrored
    x0 = _x0(x, xn, 130)[:7]
    res = view.predict_hess(x0)
    cov, G = view.predict_grad_cov(x0), view.predict_grad_cov(x0, latent=True)
    for a in res + (cov,):
        assert a.shape == (4, 7, d, d) and a.dtype == torch.float64 and torch.equal(a, a.transpose(-1, -2))
    assert G.shape == (3, 7, d, d) and torch.equal(res[1], res[2])
    got, _ = _view_second_order(view, m._standardise_x0(x0)[0])
    assert np.array_equal(pack_lower(G.numpy()), got[6]) and np.array_equal(pack_lower(view._latent_predict_hess(x0)[5]), got[5])


def test_wide_contraction_d_40():
    m, x = _model('rep', 'matern32', 40)
    xn, yn = _new_runs(m, x, 70, 4)
    _case64(m, x, xn, yn, _x0(x, xn, 40), (40,), 'rep matern32 d=40 m=70')


@pytest.mark.parametrize('d,kernel', [(6, 'matern32'), (40, 'se')])
def test_bitwise_independent_of_the_chunk_size(monkeypatch, d, kernel):
    """a pass takes max(128, PREDICT_CHUNK // d) new inputs and a last pass of fewer than 128 is moved back over its
    predecessor: one pass, 200 + 128 (overlapping), 128 + 128 + 128 (overlapping) for the 300 inputs here; the rows a moved-back
    pass repeats weigh zero in the device reduction"""
    m, x = _model('rep', kernel, d)
    xn, yn = _new_runs(m, x, 70, 4)
    view = m.condition(xn, yn)
    eng, st = view._engine, view._state
    x0s = np.random.default_rng(13).uniform(0, 1, (300, d))
    w = np.random.default_rng(14).uniform(0.1, 1.0, 300)
    monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', 400 * d)
    ref = [t.cpu().numpy() for t in eng.condition_predict_hess_block(st, x0s)]
    rg = [t.cpu().numpy() for t in eng.condition_grad_cov_block(st, x0s, w)]
    host = np.einsum('i,kie->ke', w, rg[1])
    err = np.max(np.abs(rg[2] - host)) / np.max(np.abs(host))
    print('condition grad cov d=%d: device reduction M against the host sum of the per-point Gamma: %.3e (bound 1e-13)' % (d, err))
    assert err <= 1e-13
    for chunk in (200 * d, 128 * d, 1):
        monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', chunk)
        for a, b in zip([t.cpu().numpy() for t in eng.condition_predict_hess_block(st, x0s)], ref):
            assert np.array_equal(a, b), chunk
        got = [t.cpu().numpy() for t in eng.condition_grad_cov_block(st, x0s, w)]
        assert np.array_equal(got[0], rg[0]) and np.array_equal(got[1], rg[1]), chunk
        errc = np.max(np.abs(got[2] - host)) / np.max(np.abs(host))
        assert errc <= 1e-13, (chunk, errc)
        # reduce-only equals the per-point call's M bit for bit
        dg, none, M = eng.condition_grad_cov_block(st, x0s, w, per_point=False)
        assert none is None and np.array_equal(M.cpu().numpy(), got[2]) and np.array_equal(dg.cpu().numpy(), rg[0]), chunk
    with pytest.raises(ValueError, match='per_point=False needs weights'):
        eng.condition_grad_cov_block(st, x0s, None, per_point=False)


@pytest.mark.parametrize('mode,kernel,d,k', [('full', 'se', 6, 70), ('rep', 'matern32', 6, 150)])
def test_float32_against_the_float64_dense_reference(mode, kernel, d, k):
    m64, x = _model(mode, kernel, d)
    m32, _ = _model(mode, kernel, d, dtype='float32')
    xn, yn = _new_runs(m64, x, k, 6)
    x0s = m64._standardise_x0(_x0(x, xn, 130))[0]
    dense = dense_second_order(m64, xn, yn, x0s)
    v32 = m32.condition(xn, yn)
    name = v32._engine.dtype_name
    print('condition hess float32 model: the view was built on the %s engine' % name)
    got, _ = _view_second_order(v32, x0s)
    aug = _augmented_engine(m64, xn, yn, dtype=name)
    ref, _ = _engine_second_order(aug.predict_hess_block(x0s), aug.grad_cov_block(x0s))
    assert all(g.dtype == np.float64 for g in got)
    # (no floor: the bound is 4 x the error of the augmented engine of the same dtype, measured here)
    _check('%s %s d=%d m=%d %s' % (mode, kernel, d, k, name), got, ref, dense, floor=0.0)


# ---- central differences and autograd -----------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,kernel', [('full', 'matern32'), ('rep', 'se'), ('full', 'matern52')])
def test_predict_hess_against_central_differences_of_the_views_predict_grad(mode, kernel):
    m, x = _box_model(mode, kernel)
    xn, yn = _new_runs(m, x, 70, 5)
    view = m.condition(xn, yn)
    lo, hi = x.min(0), x.max(0)
    h = 1e-5 * (hi - lo)
    knots = np.vstack([x, xn])
    rng, pts = np.random.default_rng(2), []
    while len(pts) < 17:                                  # at least two steps from every kink (training and view coordinates)
        p = lo + (hi - lo) * rng.uniform(0.05, 0.95, 3)
        if np.min(np.abs(p[None, :] - knots) / h) >= 2.0:
            pts.append(p)
    x0 = np.array(pts)
    got = [t.numpy() for t in view.predict_hess(x0)]
    for c in range(3):
        e = np.zeros_like(x0)
        e[:, c] = h[c]
        plus, minus = view.predict_grad(x0 + e), view.predict_grad(x0 - e)
        for w in range(3):
            fd = (plus[w].numpy() - minus[w].numpy()) / (2 * h[c])
            err, unit = np.max(np.abs(got[w][..., c] - fd)), np.max(np.abs(got[w]))
            print('condition hess central differences %s %s output %d dim %d: %.3e of the largest entry' % (mode, kernel, w, c, err / unit))
            assert got[w].shape == (4, 17, 3, 3) and err <= 1e-6 * unit, (w, c, err / unit)


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_order_two_gradgradcheck_on_a_gpu_tensor(mode):
    m, x = _model(mode, 'se', 2)
    xn, yn = _new_runs(m, x, 5, 6)
    view = m.condition(xn, yn)
    x0 = _points(x, 3, 12)
    for dev in ('cpu', 'cuda:0'):
        xt = torch.tensor(x0, dtype=torch.float64, device=dev, requires_grad=True)
        for w in (0, 2):
            f = lambda t: view.predict_differentiable(t, order=2)[w]      # noqa: E731
            assert torch.autograd.gradcheck(f, (xt,), eps=1e-6, atol=1e-6, rtol=1e-4)
            assert torch.autograd.gradgradcheck(f, (xt,), eps=1e-6, atol=1e-5, rtol=1e-3)
    H = torch.autograd.functional.hessian(lambda t: view.predict_differentiable(t, order=2)[0].sum(), xt.detach())
    assert H.device == xt.device
    want = view.predict_hess(x0)[0].sum(dim=0)
    for i in range(3):
        np.testing.assert_allclose(H[i, :, i, :].cpu().numpy(), want[i].numpy(), rtol=1e-12, atol=1e-14)
    with pytest.raises(RuntimeError, match='double backward'):
        torch.autograd.grad(view.predict_differentiable(xt, order=1)[0].sum(), xt, create_graph=True)


def test_active_subspace_is_its_assembly_from_the_per_point_queries():
    m, x = _box_model('rep', 'matern52')
    xn, yn = _new_runs(m, x, 70, 5)
    view = m.condition(xn, yn)
    x_ref = _points(x, 130, 21)
    w = np.random.default_rng(22).uniform(0.1, 1.0, 130)
    res = view.active_subspace(x_ref, w, outputs=[3, 1])
    w = w / w.sum()
    g, cov = view.predict_grad(x_ref)[0].numpy()[[3, 1]], view.predict_grad_cov(x_ref).numpy()[[3, 1]]
    mean_part, cov_part = np.einsum('i,ail,aim->alm', w, g, g), np.einsum('i,ailm->alm', w, cov)
    big = np.max(np.abs(mean_part + cov_part))
    errs = [np.max(np.abs(a.numpy() - b)) / big for a, b in ((res.mean_part, mean_part), (res.cov_part, cov_part),
                                                           (res.matrix, mean_part + cov_part))]
    print('condition active subspace: mean part %.3e, cov part %.3e, matrix %.3e (bound 1e-11)' % tuple(errs))
    assert max(errs) <= 1e-11
    base = m.active_subspace(x_ref, w, outputs=[3, 1])
    assert np.all(np.trace(res.cov_part.numpy(), axis1=1, axis2=2) < np.trace(base.cov_part.numpy(), axis1=1, axis2=2))


# ---- semantics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_a_far_away_run_changes_nothing_inside_the_data(mode):
    m, x = _model(mode, 'matern32', 6)
    _, yn = _new_runs(m, x, 3, 12)
    far = x.max(axis=0)[None, :] + 1e4 * (x.max(axis=0) - x.min(axis=0))[None, :]
    x0s = m._standardise_x0(_points(x, 130, 13))[0]
    got, _ = _view_second_order(m.condition(far, yn[:, :1]), x0s)
    eng = m._ensure_aux()
    base, _ = _engine_second_order(eng.predict_hess_block(x0s), eng.grad_cov_block(x0s))
    for name, g, b in zip(NAMES, got, base):
        err = np.max(np.abs(g - b) / np.abs(b).reshape(3, -1).max(axis=1).reshape((-1,) + (1,) * (b.ndim - 1)))
        print('condition hess far-away run %s %s: %.3e' % (mode, name, err))
        assert err <= TOL64, (name, err)


@pytest.mark.parametrize('mode,kernel,d,k', [('full', 'matern32', 6, 70), ('rep', 'se', 6, 150), ('rep', 'matern52', 1, 1)])
def test_conditioning_cannot_add_gradient_uncertainty(mode, kernel, d, k):
    m, x = _model(mode, kernel, d)
    xn, yn = _new_runs(m, x, k, 3)
    x0 = _x0(x, xn, 130)
    Gv = m.condition(xn, yn).predict_grad_cov(x0, latent=True).numpy()
    Gb = m.predict_grad_cov(x0, latent=True).numpy()
    ev = np.linalg.eigvalsh(Gb - Gv)
    low = np.min(ev) / np.max(np.abs(Gb))
    print('condition grad cov %s %s d=%d m=%d: smallest eigenvalue of Gamma_base - Gamma_view %.3e of the largest entry, largest '
          '%.3e' % (mode, kernel, d, k, low, np.max(ev) / np.max(np.abs(Gb))))
    assert low >= -1e-12 and np.max(ev) > 0


# ---- bitwise --------------------------------------------------------------------------------------------------------------
def _raw(eng, xn_s, t, r, x0s, fill, w=None):
    """(blk, jac, hess, lcgp_condition_predict_grad's blk and jac, dghat, gamma, M) through the C entries with buffers of this
    test's own, every one filled with `fill` before the call that uses it: the cond workspace, the state, the grad state and
    the scratch of the preparation and of every pass"""
    lib, dev, q, d = eng.lib, eng.device, eng.q_local, eng.d
    m, n0, tri = len(xn_s), len(x0s), eng.d * (eng.d + 1) // 2
    nb = eng._nbytes
    cws = _filled(nb("lcgp_workspace_bytes", eng.dtype, m, d, eng.p, q), fill, dev)
    state = _filled(nb("lcgp_condition_state_bytes", eng.dtype, eng.n, d, q, m), fill, dev)
    gstate = _filled(nb("lcgp_condition_grad_state_bytes", eng.dtype, eng.n, q, m), fill, dev)
    nsc = max(nb("lcgp_condition_scratch_bytes", eng.dtype, eng.n, q, m, 0),
              nb("lcgp_condition_predict_hess_scratch_bytes", eng.dtype, eng.n, d, q, m, n0))
    assert nb("lcgp_condition_predict_gradcov_scratch_bytes", eng.dtype, eng.n, d, q, m, n0) <= nsc
    scratch = _filled(nsc, fill, dev)
    xnd = torch.as_tensor(np.ascontiguousarray(xn_s)).to(dev, eng.tdtype).contiguous()
    x0d = torch.as_tensor(np.ascontiguousarray(x0s)).to(dev, eng.tdtype).contiguous()
    td = torch.as_tensor(np.ascontiguousarray(t)).to(dev)
    rd = None if r is None else torch.as_tensor(np.ascontiguousarray(r, np.float64)).to(dev)
    wd = None if w is None else torch.as_tensor(np.ascontiguousarray(w, np.float64)).to(dev)
    info = torch.zeros(q, dtype=torch.int32, device=dev)
    out, plain = [torch.empty((2, q, n0), dtype=torch.float64, device=dev) for _ in range(2)]
    jac, pjac = [torch.empty((2, q, n0, d), dtype=torch.float64, device=dev) for _ in range(2)]
    hess = torch.empty((2, q, n0, tri), dtype=torch.float64, device=dev)
    dghat = torch.empty((q, n0, d), dtype=torch.float64, device=dev)
    gamma = torch.empty((q, n0, tri), dtype=torch.float64, device=dev)
    M = None if w is None else torch.zeros((q, tri), dtype=torch.float64, device=dev)
    p = eng._p
    with torch.cuda.device(dev):
        st = eng._stream()
        common = (st, eng.dtype, eng.kernel_id, eng.n, d, eng.p, q, p(eng.x), p(eng.sr), p(eng.theta_dev), p(eng.workspace))
        _hip.check(lib.lcgp_condition_prepare(*common, m, p(xnd), p(td), p(rd), p(scratch), nsc, p(cws), p(state), p(info)),
                   "lcgp_condition_prepare")
        assert not np.any(info.cpu().numpy())
        _hip.check(lib.lcgp_condition_grad_prepare(st, eng.dtype, eng.n, d, eng.p, q, p(eng.theta_dev), p(eng.workspace), p(state), m,
                                                   p(gstate)), "lcgp_condition_grad_prepare")
        view = (p(state), m, p(xnd), p(gstate), n0, p(x0d), p(scratch), nsc)
        scratch.fill_(fill)
        _hip.check(lib.lcgp_condition_predict_grad(*common, *view, p(plain[0]), p(plain[1]), p(pjac[0]), p(pjac[1]), n0),
                   "lcgp_condition_predict_grad")
        scratch.fill_(fill)
        _hip.check(lib.lcgp_condition_predict_hess(*common, *view, p(out[0]), p(out[1]), p(jac[0]), p(jac[1]), p(hess[0]),
                                                   p(hess[1]), n0), "lcgp_condition_predict_hess")
        scratch.fill_(fill)
        _hip.check(lib.lcgp_condition_predict_gradcov(*common, *view, p(dghat), p(gamma), p(wd), p(M), n0),
                   "lcgp_condition_predict_gradcov")
        res = [out, jac, hess, plain, pjac, dghat, gamma] + ([] if M is None else [M])
        return [a.cpu().numpy() for a in res]


@pytest.mark.parametrize('mode,dtype', [('full', 'float64'), ('rep', 'float64'), ('rep', 'float32')])
def test_bitwise_on_poisoned_memory_and_one_component(mode, dtype):
    m, x = _model(mode, 'matern32', 6, dtype=dtype)
    xn, yn = _new_runs(m, x, 70, 7)
    x0s = m._standardise_x0(_x0(x, xn, 130, 8))[0]
    w = np.random.default_rng(9).uniform(0.1, 1.0, 130)
    eng, xn_s, t, r = _engine_args(m, xn, yn)
    ck0 = _checksum(eng)
    state = eng.condition_begin(xn_s, t, r)
    ref = [a.cpu().numpy() for a in eng.condition_predict_hess_block(state, x0s)]
    rg = [a.cpu().numpy() for a in eng.condition_grad_cov_block(state, x0s, w)]
    gblk, gjac = [a.cpu().numpy() for a in eng.condition_predict_grad_block(state, x0s)]
    assert np.array_equal(ref[0], gblk) and np.array_equal(ref[1], gjac) and np.array_equal(rg[0], gjac[0])
    assert all(np.all(np.isfinite(a)) for a in ref + rg)
    for fill in (0x00, 0xFF, 0x5A):
        blk, jac, hess, plain, pjac, dghat, gamma, M = _raw(eng, xn_s, t, r, x0s, fill, w)
        assert np.array_equal(blk, plain) and np.array_equal(jac, pjac) and np.array_equal(dghat, pjac[0]), fill
        assert np.array_equal(blk, ref[0]) and np.array_equal(jac, ref[1]) and np.array_equal(hess, ref[2]), fill
        assert np.array_equal(gamma, rg[1]) and np.array_equal(M, rg[2]), fill
    assert _checksum(eng) == ck0                       # the base workspace is only read
    # q_local = 1 against all components: an engine of its own holding component k alone
    xt, s, Y = _training(m)
    rows = eng._theta_last
    for k in range(len(rows)):
        solo = HotPathEngine(xt, Y, None if mode == 'full' else s, q_local=1, dtype=dtype, kernel=m.kernel)
        solo.evaluate(rows[k:k + 1])
        st1 = solo.condition_begin(xn_s, t[k:k + 1], r)
        for a, b in zip(solo.condition_predict_hess_block(st1, x0s), ref):
            assert np.array_equal(a.cpu().numpy()[:, 0], b[:, k]), k
        for a, b in zip(solo.condition_grad_cov_block(st1, x0s, w), rg):
            assert np.array_equal(a.cpu().numpy()[0], b[k]), k


def test_two_ranks_reproduce_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_condition_hess_gpu_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


# ---- the base model is only read ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_base_model_and_first_order_view_queries_untouched(mode):
    m, x = _model(mode, 'se', 6)
    xn, yn = _new_runs(m, x, 70, 10)
    x0 = _points(x, 130, 11)
    lg0 = m.loss_and_grad()
    p0 = [t.numpy().copy() for t in m.predict(x0)]
    h0 = [t.numpy().copy() for t in m.predict_hess(x0)]
    eng = m._ensure_aux()
    ck0 = _checksum(eng)
    view = m.condition(xn, yn)
    v0 = [t.numpy().copy() for t in view.predict(x0)]
    g0 = [t.numpy().copy() for t in view.predict_grad(x0)]
    a = [t.numpy() for t in view.predict_hess(x0)]
    b = [t.numpy() for t in view.predict_hess(x0[:50])]
    assert all(np.array_equal(u[:, :50], v) for u, v in zip(a, b))
    view.predict_grad_cov(x0)
    view.active_subspace(x0)
    assert _checksum(eng) == ck0 and m._ensure_aux() is eng
    assert all(np.array_equal(u, v.numpy()) for u, v in zip(v0, view.predict(x0)))
    assert all(np.array_equal(u, v.numpy()) for u, v in zip(g0, view.predict_grad(x0)))
    assert all(np.array_equal(u, v.numpy()) for u, v in zip(p0, m.predict(x0)))
    assert all(np.array_equal(u, v.numpy()) for u, v in zip(h0, m.predict_hess(x0)))
    assert np.max(np.abs(a[0] - h0[0])) > 0
    lg1 = m.loss_and_grad()
    assert lg0[0] == lg1[0] and np.array_equal(lg0[1], lg1[1])
    view.predict_hess(x0[:3])                            # the same parameters, factorised again: the view is still current
    m._set_flat(m._get_flat() + 0.01)
    for call in (lambda: view.predict_hess(x0), lambda: view.predict_grad_cov(x0), lambda: view.active_subspace(x0),
                 lambda: view.predict_differentiable(torch.as_tensor(x0), order=2)):
        with pytest.raises(RuntimeError, match='stale'):
            call()


# ---- limits ---------------------------------------------------------------------------------------------------------------
def test_limits_and_errors_are_the_models():
    m, x = _model('full', 'matern32', 2)
    xn, yn = _new_runs(m, x, 5, 6)
    view = m.condition(xn, yn)
    for call in (view.predict_hess, view.predict_grad_cov, view.active_subspace):
        with pytest.raises(ValueError, match='must have shape'):
            call(np.zeros((3, 3)))
    with pytest.raises(ValueError, match='order must be 1 or 2'):
        view.predict_differentiable(x[:3], order=3)
    with pytest.raises(ValueError, match='weights must have length'):
        view.active_subspace(x[:5], np.ones(3))
    with pytest.raises(ValueError, match='outputs must be'):
        view.active_subspace(x[:5], None, [4])
    eng, st = view._engine, view._state
    nb = C.c_size_t(0)
    assert eng.lib.lcgp_condition_predict_hess_scratch_bytes(eng.dtype, eng.n, 2, eng.q_local, 5, 1 << 28, C.byref(nb)) < 0
    assert b'LCGP_HESS_MAX_ROWS' in eng.lib.lcgp_last_error()
    # a scratch that is too small is refused before anything is enqueued
    d8 = torch.zeros(64, dtype=torch.float64, device=eng.device)
    p = eng._p
    gs = eng._condition_grad_state(st)
    rc = eng.lib.lcgp_condition_predict_gradcov(eng._stream(), eng.dtype, eng.kernel_id, eng.n, 2, eng.p, eng.q_local, p(eng.x),
                                                p(eng.sr), p(eng.theta_dev), p(eng.workspace), p(st['state']), 5, p(st['xn']),
                                                p(gs), 3, p(d8), p(d8), 64, p(d8), p(d8), None, None, 0)
    assert rc == -1 and b'scratch is smaller' in eng.lib.lcgp_last_error()
