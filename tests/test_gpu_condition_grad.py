"""Input gradients and the calibration target of a conditioned view on the GPU (lcgp_condition_grad_prepare /
lcgp_condition_predict_grad: OP_COND_U of the tile kernel, pgrad_cond_kernel) against dense float64 numpy on the augmented data
and against a HotPathEngine built on the augmented data at the same theta rows (its own predict_grad_block); central
differences of view.predict and gradcheck; float32 against float64; bitwise-equal results on poisoned cond workspace, state,
grad state and scratch, for any split of the rows, for one component against all and on two ranks; the base
model untouched; limits; calibration on the view.

Shapes: n = 333 training inputs (no multiple of 64), q = 3, m in {1, 70, 150} (one short tile, across a 64 and a 128
boundary), n0 in {1, 130}, d in {1, 6}, once d = 40 (the wide contraction) and once n0 = 2100 (two passes stitched through
out_stride), the three kernels, full and rep with 1 to 3 replicates.  Some rows of x0 equal training inputs and some the
view's own new inputs (same = 0: the gradient of the continuous surface).

Bounds, float64: the rule of tests/test_gpu_condition.py -- per component and quantity (ghat, gvar, dghat, dgvar) 1e-10 of the
largest |entry| of the dense reference over the case's points.  tau = 1 / D can make S ill-conditioned, so every case also
measures the augmented engine (code this feature does not touch) against the same dense reference: where the view exceeds the
fixed bound, the admissible bound is 4 x the augmented engine's own error on that case.  It is never derived from the view's
numbers.  float32 against float64: 2e-3 of the largest entry.  Every case prints its figures before it asserts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from lcgp_amd import LCGP, _hip, synth
from lcgp_amd import engine as engine_mod
from lcgp_amd.engine import HotPathEngine, calib_rows_device
from oracle import lcgp_oracle as orc
from tests.test_condition_grad_host import kernel_derivative
from tests.test_condition_host import new_columns
from tests.test_gpu_condition import CASES, N, _checksum, _engine_args, _filled, _model, _new_runs, _training
from tests.test_gpu_variance_reduction import _free_port, _points
from tests.test_predict_hess_host import _cross

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL64 = 1e-10
TOL32 = 2e-3
NAMES = ('ghat', 'gvar', 'dghat', 'dgvar')


def dense_grad_augmented(rows, x, s, Y, kernel, xn_s, snew, ycol, x0s):
    """(ghat, gvar (q, n0), dghat, dgvar (q, n0, d)) from first principles in float64 numpy: the training set (x, s, Y)
    augmented by the new columns, A = I + D (C o s s^T) rebuilt and factorised at the theta rows, lcgp_predict_grad's formulas
    (same = 0) on the augmented matrix"""
    xa, sa, Ya = np.vstack([x, xn_s]), np.r_[s, snew], np.hstack([Y, ycol])
    d = x.shape[1]
    out = [np.zeros((len(rows), len(x0s))) for _ in range(2)] + [np.zeros((len(rows), len(x0s), d)) for _ in range(2)]
    for i, th in enumerate(rows):
        ell, scale, nug, D, psi = th[:d], th[d], th[d + 1], th[d + 2], th[d + 3:]
        Cm = _cross(xa, xa, ell, scale, nug, kernel)
        Cm[np.arange(len(xa)), np.arange(len(xa))] = scale
        low = np.linalg.cholesky(np.eye(len(xa)) + D * Cm * np.outer(sa, sa))
        c = _cross(x0s, xa, ell, scale, nug, kernel)
        X = c * sa[None, :]
        u = sla.solve_triangular(low, X.T, lower=True)
        V = sla.solve_triangular(low.T, u, lower=False).T
        z = sla.cho_solve((low, True), Ya.T @ psi)
        dc = kernel_derivative(x0s, xa, ell, c, kernel)
        out[0][i], out[1][i] = X @ z, scale - D * np.sum(u * u, axis=0)
        out[2][i] = np.einsum('ijl,j->il', dc, sa * z)
        out[3][i] = -2.0 * D * np.einsum('ijl,ij->il', dc, sa[None, :] * V)
    return out


def _augmented_engine(m, xn, yn):
    eng = m._ensure_aux()
    rows = eng._theta_last.copy()
    x, s, Y = _training(m)
    xn_s, snew, ycol = new_columns(m, xn, yn)
    aug = HotPathEngine(np.vstack([x, xn_s]), np.hstack([Y, ycol]), None if m.submethod == 'full' else np.r_[s, snew],
                        q_local=len(rows), kernel=m.kernel)
    aug.evaluate(rows)
    return aug


def _x0(x, xn, n0, seed=2):
    """n0 new inputs inside the data's box; from five rows on, three of them are training inputs and up to two the view's own
    new inputs"""
    x0 = _points(x, max(n0, 5), seed)
    x0[:3] = x[[5, 17, 100]]
    x0[3:3 + min(2, len(xn))] = xn[:2]
    return x0[:n0]


def _check64(m, x, xn, yn, x0, tag):
    view = m.condition(xn, yn)
    got = [t.numpy() for t in view.predict_grad(x0, latent=True)]
    eng = m._ensure_aux()
    x0s = m._standardise_x0(x0)[0]
    dense = dense_grad_augmented(eng._theta_last, *_training(m), m.kernel, *new_columns(m, xn, yn), x0s)
    blk, jac = [t.cpu().numpy() for t in _augmented_engine(m, xn, yn).predict_grad_block(x0s)]
    aug = [blk[0], blk[1], jac[0], jac[1]]
    bad = []
    for name, g, a, r in zip(NAMES, got, aug, dense):
        assert g.shape == r.shape and np.all(np.isfinite(g)), name
        unit = np.abs(r).reshape(len(r), -1).max(axis=1).reshape((-1,) + (1,) * (r.ndim - 1))
        ev, ea, ex = [float(np.max(np.abs(u - v) / unit)) for u, v in ((g, r), (a, r), (g, a))]
        bound = max(TOL64, 4 * ea)
        print('condition grad %s %s: view vs dense %.3e | augmented engine vs dense %.3e | view vs augmented engine %.3e | '
              'bound %.1e' % (tag, name, ev, ea, ex, bound))
        if not (ev <= bound and ex <= bound + ea):
            bad.append((name, ev, ea, ex, bound))
    assert not bad, (tag, bad)
    return view, got


@pytest.mark.parametrize('mode,kernel,d,k', CASES)
def test_view_gradients_match_dense_numpy_on_the_augmented_data(mode, kernel, d, k):
    m, x = _model(mode, kernel, d)
    xn, yn = _new_runs(m, x, k, 3)
    x0 = _x0(x, xn, 130)
    for n0 in (1, 130):
        view, got = _check64(m, x, xn, yn, x0[:n0], '%s %s d=%d m=%d n0=%d' % (mode, kernel, d, k, n0))
        assert got[2].shape == (3, n0, d)
        a, b = [t.numpy() for t in view.predict(x0[:n0], latent=True)]
        assert np.array_equal(got[0], a) and np.array_equal(got[1], b)


def test_wide_contraction_d_40():
    m, x = _model('rep', 'matern32', 40)
    xn, yn = _new_runs(m, x, 70, 4)
    _check64(m, x, xn, yn, _x0(x, xn, 130), 'rep matern32 d=40 m=70 n0=130')


def test_two_passes_are_stitched_through_out_stride():
    m, x = _model('full', 'matern52', 6)
    xn, yn = _new_runs(m, x, 70, 4)
    x0 = _x0(x, xn, 2100, 5)
    assert engine_mod.PREDICT_CHUNK == 2048
    view, got = _check64(m, x, xn, yn, x0, 'full matern52 d=6 m=70 n0=2100')
    # the second pass (52 rows, 64-row tiles) wrote its own columns and nothing else
    tail = [t.numpy() for t in view.predict_grad(x0[2048:], latent=True)]
    for a, b in zip(got, tail):
        assert np.array_equal(a[:, 2048:], b)


# ---- central differences and autograd -----------------------------------------------------------------------------------
def _box_model(mode, kernel, d=3, dtype='float64'):
    """_model of tests/test_gpu_condition.py on a non-unit box, a different range per dimension"""
    span = np.array([5.0, 0.25, 1.0])[:d]
    if mode == 'full':
        x, y = synth.make_full(95, N, d, 4, 3)
    else:
        x, y = synth.make_rep(96, N, 2, d, 4, 3)
    x = 1.0 + span * np.asarray(x)
    m = LCGP(y=y, x=x, q=3, submethod=mode, kernel=kernel, device='cuda:0', dtype=dtype)
    m._set_flat(synth.param_points(95, orc.OracleLCGP(y=y, x=x, q=3, submethod=mode).get_unconstrained())[1])
    return m, x


@pytest.mark.parametrize('mode,kernel', [('full', 'matern32'), ('rep', 'se'), ('full', 'matern52')])
def test_predict_grad_against_central_differences_of_the_views_predict(mode, kernel):
    m, x = _box_model(mode, kernel)
    xn, yn = _new_runs(m, x, 70, 5)
    view = m.condition(xn, yn)
    lo, hi = x.min(0), x.max(0)
    x0 = lo + (hi - lo) * np.random.default_rng(2).uniform(0.05, 0.95, (17, 3))
    got = [t.numpy() for t in view.predict_grad(x0)]
    h = 1e-5 * (hi - lo)
    for l in range(3):
        e = np.zeros_like(x0)
        e[:, l] = h[l]
        plus, minus = view.predict(x0 + e), view.predict(x0 - e)
        for w in range(3):
            fd = (plus[w].numpy() - minus[w].numpy()) / (2 * h[l])
            err, unit = np.max(np.abs(got[w][:, :, l] - fd)), np.max(np.abs(got[w]))
            print('condition grad central differences %s %s output %d dim %d: %.3e of the largest entry' % (mode, kernel, w, l, err / unit))
            assert got[w].shape == (4, 17, 3) and err <= 1e-6 * unit, (w, l, err / unit)


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_predict_differentiable_gradcheck(mode):
    m, x = _model(mode, 'matern32', 2)
    xn, yn = _new_runs(m, x, 5, 6)
    view = m.condition(xn, yn)
    x0 = _points(x, 4, 12)
    for a, b in zip(view.predict_differentiable(torch.as_tensor(x0)), view.predict(x0)):
        assert torch.equal(a, b)
    for dev in ('cpu', 'cuda:0'):
        xt = torch.tensor(x0, dtype=torch.float64, device=dev, requires_grad=True)
        for w in range(3):
            assert torch.autograd.gradcheck(lambda t: view.predict_differentiable(t)[w], (xt,), eps=1e-6, atol=1e-6, rtol=1e-4)
        yp = view.predict_differentiable(xt)[0]
        assert yp.device == xt.device
        yp.sum().backward()
        assert xt.grad.device == xt.device and torch.all(torch.isfinite(xt.grad))
    with pytest.raises(RuntimeError, match='double backward'):
        torch.autograd.grad(view.predict_differentiable(xt)[0].sum(), xt, create_graph=True)


@pytest.mark.parametrize('mode,kernel,d,k', [('full', 'se', 6, 70), ('rep', 'matern32', 6, 150)])
def test_float32_against_float64(mode, kernel, d, k):
    m64, x = _model(mode, kernel, d)
    m32, _ = _model(mode, kernel, d, dtype='float32')
    xn, yn = _new_runs(m64, x, k, 6)
    x0 = _x0(x, xn, 130)
    a = [t.numpy() for t in m64.condition(xn, yn).predict_grad(x0, latent=True)]
    v32 = m32.condition(xn, yn)
    b = [t.numpy() for t in v32.predict_grad(x0, latent=True)]
    print('condition grad float32 model: the view was built on the %s engine' % v32._engine.dtype_name)
    for name, u, v in zip(NAMES[2:], a[2:], b[2:]):
        assert v.dtype == np.float64 and np.all(np.isfinite(v))
        err = np.max(np.abs(u - v) / np.abs(u).reshape(3, -1).max(axis=1)[:, None, None])
        print('condition grad float32 vs float64 %s %s m=%d %s: %.3e (bound %.1e)' % (mode, kernel, k, name, err, TOL32))
        assert err <= TOL32, (name, err)
    for u, v in zip(m64.condition(xn, yn).predict_grad(x0), v32.predict_grad(x0)):
        assert np.max(np.abs(u.numpy() - v.numpy())) <= TOL32 * np.max(np.abs(u.numpy()))


# ---- bitwise -----------------------------------------------------------------------------------------------------------
def _raw(eng, xn_s, t, r, x0s, fill, splits=None):
    """(blk (2, q, n0), jac (2, q, n0, d), lcgp_condition_predict's blk) through the C entries with buffers of this test's own,
    every one filled with `fill` before the call that uses it: the cond workspace, the state, the grad state, the scratch of
    the preparation and of every pass"""
    lib, dev, q, d = eng.lib, eng.device, eng.q_local, eng.d
    m, n0 = len(xn_s), len(x0s)
    splits = [(0, n0)] if splits is None else splits
    nb = eng._nbytes
    cws = _filled(nb("lcgp_workspace_bytes", eng.dtype, m, d, eng.p, q), fill, dev)
    state = _filled(nb("lcgp_condition_state_bytes", eng.dtype, eng.n, d, q, m), fill, dev)
    gstate = _filled(nb("lcgp_condition_grad_state_bytes", eng.dtype, eng.n, q, m), fill, dev)
    nsc = max([nb("lcgp_condition_scratch_bytes", eng.dtype, eng.n, q, m, 0)] +
              [nb("lcgp_condition_predict_grad_scratch_bytes", eng.dtype, eng.n, q, m, rows) for _, rows in splits])
    scratch = _filled(nsc, fill, dev)
    xnd = torch.as_tensor(np.ascontiguousarray(xn_s)).to(dev, eng.tdtype).contiguous()
    x0d = torch.as_tensor(np.ascontiguousarray(x0s)).to(dev, eng.tdtype).contiguous()
    td = torch.as_tensor(np.ascontiguousarray(t)).to(dev)
    rd = None if r is None else torch.as_tensor(np.ascontiguousarray(r, np.float64)).to(dev)
    info = torch.zeros(q, dtype=torch.int32, device=dev)
    out, plain = [torch.empty((2, q, n0), dtype=torch.float64, device=dev) for _ in range(2)]
    jac = torch.empty((2, q, n0, d), dtype=torch.float64, device=dev)
    p = eng._p
    with torch.cuda.device(dev):
        st = eng._stream()
        common = (st, eng.dtype, eng.kernel_id, eng.n, d, eng.p, q, p(eng.x), p(eng.sr), p(eng.theta_dev), p(eng.workspace))
        _hip.check(lib.lcgp_condition_prepare(*common, m, p(xnd), p(td), p(rd), p(scratch), nsc, p(cws), p(state), p(info)),
                   "lcgp_condition_prepare")
        assert not np.any(info.cpu().numpy())
        scratch.fill_(fill)
        _hip.check(lib.lcgp_condition_grad_prepare(st, eng.dtype, eng.n, d, eng.p, q, p(eng.theta_dev), p(eng.workspace), p(state), m,
                                                   p(gstate)), "lcgp_condition_grad_prepare")
        for lo, rows in splits:
            x0p = C.c_void_p(x0d.data_ptr() + lo * d * x0d.element_size())
            scratch.fill_(fill)
            _hip.check(lib.lcgp_condition_predict(*common, p(state), m, p(xnd), rows, x0p, p(scratch), nsc,
                                                  C.c_void_p(plain[0].data_ptr() + 8 * lo), C.c_void_p(plain[1].data_ptr() + 8 * lo),
                                                  n0), "lcgp_condition_predict")
            scratch.fill_(fill)
            _hip.check(lib.lcgp_condition_predict_grad(*common, p(state), m, p(xnd), p(gstate), rows, x0p, p(scratch), nsc,
                                                       C.c_void_p(out[0].data_ptr() + 8 * lo), C.c_void_p(out[1].data_ptr() + 8 * lo),
                                                       C.c_void_p(jac[0].data_ptr() + 8 * lo * d),
                                                       C.c_void_p(jac[1].data_ptr() + 8 * lo * d), n0), "lcgp_condition_predict_grad")
        return out.cpu().numpy(), jac.cpu().numpy(), plain.cpu().numpy()


@pytest.mark.parametrize('mode,dtype', [('full', 'float64'), ('rep', 'float64'), ('rep', 'float32')])
def test_bitwise_on_poisoned_memory_row_splits_and_one_component(mode, dtype):
    m, x = _model(mode, 'matern32', 6, dtype=dtype)
    xn, yn = _new_runs(m, x, 70, 7)
    x0s = m._standardise_x0(_x0(x, xn, 130, 8))[0]
    eng, xn_s, t, r = _engine_args(m, xn, yn)
    state = eng.condition_begin(xn_s, t, r)
    ref, rjac = [a.cpu().numpy() for a in eng.condition_predict_grad_block(state, x0s)]
    assert np.array_equal(ref, eng.condition_predict_block(state, x0s).cpu().numpy()) and 'grad' in state
    assert np.all(np.isfinite(rjac))
    for fill in (0x00, 0xFF, 0x5A):
        blk, jac, plain = _raw(eng, xn_s, t, r, x0s, fill)
        assert np.array_equal(blk, ref) and np.array_equal(blk, plain) and np.array_equal(jac, rjac), fill
    # n0 = 130 in one call against its rows split 64 + 66 and 127 + 3: U_0 and T take 64- or 128-row tiles by the padded row
    # count and add in the same order on both (tests/test_gpu_condition.py); R, U' and V' are formed on 64-row tiles whatever
    # the row count is
    a = _raw(eng, xn_s, t, r, x0s, 0x5A, splits=[(0, 64), (64, 66)])
    b = _raw(eng, xn_s, t, r, x0s, 0xFF, splits=[(0, 127), (127, 3)])
    c = _raw(eng, xn_s, t, r, x0s[:127], 0x00)
    for name, u, v, w_ in zip(('blk', 'jac', 'plain'), a, b, c):
        print('condition grad %s %s %s: 64 + 66 equals 127 + 3: %s, equals 127 alone: %s' % (mode, dtype, name, np.array_equal(u, v),
                                                                                             np.array_equal(u[:, :, :127], w_)))
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert all(np.array_equal(u[:, :, :127], v) for u, v in zip(a, c))
    print('condition grad %s %s: 130 rows in one call against 64 + 66: Jacobians equal %s, max difference %.3e'
          % (mode, dtype, np.array_equal(a[1], rjac), np.max(np.abs(a[1] - rjac))))
    assert np.array_equal(a[0], ref) and np.array_equal(a[0], a[2]) and np.array_equal(a[1], rjac)
    # and on 128-row tiles: 260 rows in one call against 130 + 130
    x1 = m._standardise_x0(_points(x, 260, 9))[0]
    a, b = _raw(eng, xn_s, t, r, x1, 0x5A), _raw(eng, xn_s, t, r, x1, 0x00, splits=[(0, 130), (130, 130)])
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    # q_local = 1 against all components: an engine of its own holding component k alone
    xt, s, Y = _training(m)
    rows = eng._theta_last
    for k in range(len(rows)):
        solo = HotPathEngine(xt, Y, None if mode == 'full' else s, q_local=1, dtype=dtype, kernel=m.kernel)
        solo.evaluate(rows[k:k + 1])
        blk, jac = [u.cpu().numpy() for u in solo.condition_predict_grad_block(solo.condition_begin(xn_s, t[k:k + 1], r), x0s)]
        assert np.array_equal(blk[:, 0], ref[:, k]) and np.array_equal(jac[:, 0], rjac[:, k]), k


def test_two_ranks_reproduce_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_condition_grad_gpu_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


# ---- the base model is only read ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_base_model_untouched(mode):
    m, x = _model(mode, 'se', 6)
    xn, yn = _new_runs(m, x, 70, 10)
    x0 = _points(x, 130, 11)
    lg0 = m.loss_and_grad()
    p0 = [t.numpy().copy() for t in m.predict(x0)]
    g0 = [t.numpy().copy() for t in m.predict_grad(x0)]
    eng = m._ensure_aux()
    ck0 = _checksum(eng)
    view = m.condition(xn, yn)
    v0 = [t.numpy().copy() for t in view.predict(x0)]
    a = [t.numpy() for t in view.predict_grad(x0)]
    b = [t.numpy() for t in view.predict_grad(x0[:50])]
    assert all(np.array_equal(u[:, :50], v) for u, v in zip(a, b))
    tgt = view.calibration(yn[:, 0], 0.3)
    tgt.loglik_grad(x0[:20])
    assert _checksum(eng) == ck0 and m._ensure_aux() is eng
    assert all(np.array_equal(u, v.numpy()) for u, v in zip(v0, view.predict(x0)))
    assert all(np.array_equal(u, v.numpy()) for u, v in zip(p0, m.predict(x0)))
    assert all(np.array_equal(u, v.numpy()) for u, v in zip(g0, m.predict_grad(x0)))
    assert np.max(np.abs(a[0] - g0[0])) > 0
    lg1 = m.loss_and_grad()
    assert lg0[0] == lg1[0] and np.array_equal(lg0[1], lg1[1])
    view.predict_grad(x0[:3])                            # the same parameters, factorised again: the view is still current


# ---- limits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_a_far_away_run_changes_nothing_inside_the_data(mode):
    m, x = _model(mode, 'matern32', 6)
    _, yn = _new_runs(m, x, 3, 12)
    far = x.max(axis=0)[None, :] + 1e4 * (x.max(axis=0) - x.min(axis=0))[None, :]
    x0 = _points(x, 130, 13)
    got = [t.numpy() for t in m.condition(far, yn[:, :1]).predict_grad(x0, latent=True)]
    blk, jac = [t.cpu().numpy() for t in m._ensure_aux().predict_grad_block(m._standardise_x0(x0)[0])]
    for name, g, b in zip(NAMES, got, (blk[0], blk[1], jac[0], jac[1])):
        err = np.max(np.abs(g - b) / np.abs(b).reshape(3, -1).max(axis=1).reshape((-1,) + (1,) * (b.ndim - 1)))
        print('condition grad far-away run %s %s: %.3e' % (mode, name, err))
        assert err <= TOL64, (name, err)


# ---- calibration on the view --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,kernel,form', [('full', 'matern32', 'dense'), ('rep', 'se', 'diag'), ('full', 'matern52', 'scalar')])
def test_view_calibration_against_the_augmented_engine_and_central_differences(mode, kernel, form):
    m, x = _box_model(mode, kernel)
    xn, yn = _new_runs(m, x, 70, 14)
    view = m.condition(xn, yn)
    rng = np.random.default_rng(15)
    sd = yn.std(axis=1)
    y_obs = yn[:, 3] + 0.1 * sd * rng.standard_normal(4)
    var = (sd * rng.uniform(0.2, 0.4, 4)) ** 2
    B = 0.1 * sd[:, None] * rng.standard_normal((4, 2))
    obs_var = {'scalar': float(var.mean()), 'diag': var, 'dense': np.diag(var) + B @ B.T}[form]
    if form == 'diag':
        y_obs[1] = np.nan
    tgt = view.calibration(y_obs, obs_var)
    lo, hi = x.min(0), x.max(0)
    theta = lo + (hi - lo) * rng.uniform(0.05, 0.95, (17, 3))
    theta[:2] = x[[3, 11]]
    theta[2] = xn[0]
    ll = tgt.loglik(theta)
    ll2, dll, s, v = tgt.loglik_grad(theta, latent=True)
    assert torch.equal(ll, ll2) and dll.shape == (17, 3) and s.shape == v.shape == (3, 17)
    # calib_rows_device on the augmented engine's predict_grad_block with the same M, b, c0, lognorm
    aug = _augmented_engine(m, xn, yn)
    blk, jac = aug.predict_grad_block(m._standardise_x0(theta)[0])
    dev = blk.device
    M, b, inv_range = [torch.as_tensor(np.ascontiguousarray(a, np.float64)).to(dev) for a in (tgt.M, tgt.b, 1.0 / (hi - lo))]
    want, dwant, _ = [None if u is None else u.cpu().numpy() for u in calib_rows_device(blk, jac, M, b, tgt.c0, tgt.lognorm, inv_range)]
    e1 = np.max(np.abs(ll.numpy() - want)) / np.max(np.abs(want))
    e2 = np.max(np.abs(dll.numpy() - dwant)) / np.max(np.abs(dwant))
    print('condition calibration %s %s %s: loglik %.3e, gradient %.3e against the augmented engine (bound 1e-9)' % (mode, kernel, form, e1, e2))
    assert e1 <= 1e-9 and e2 <= 1e-9
    # central differences of loglik, away from the training inputs
    h = 1e-5 * (hi - lo)
    fd = np.zeros((14, 3))
    for l in range(3):
        e = np.zeros(3)
        e[l] = h[l]
        fd[:, l] = (tgt.loglik(theta[3:] + e).numpy() - tgt.loglik(theta[3:] - e).numpy()) / (2 * h[l])
    e3 = np.max(np.abs(dll.numpy()[3:] - fd)) / np.max(np.abs(fd))
    print('condition calibration %s %s %s: gradient against central differences %.3e (bound 1e-6)' % (mode, kernel, form, e3))
    assert e3 <= 1e-6
    tt = torch.tensor(theta[3:7], dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(tgt.loglik_differentiable(tt).sum(), tt)
    assert torch.equal(g, dll[3:7])
    m._set_flat(m._get_flat() + 0.01)
    for call in (lambda: tgt.loglik(theta), lambda: tgt.loglik_grad(theta), lambda: view.predict_grad(theta)):
        with pytest.raises(RuntimeError, match='stale'):
            call()
