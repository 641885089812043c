"""CPU tests of the ALC gradient on a conditioned view (ConditionedLCGP.variance_reduction_grad /
variance_reduction_differentiable): a numpy stand-in of HotPathEngine.condition_variance_reduction_grad_block written from the
view formulas of include/lcgp_hip.h (widened rows, Q_n, Q', R_c, V'_c), checked against tests/vr_grad_ref.value_and_grad on the
augmented data and against central differences of the closed-form view R'; the host layer -- shapes, latent=, outputs=, the
weights, the raw-scale gradient, the every-candidate-is-new rule, every ValueError, staleness, autograd, the gather over ranks --
through that stand-in; and the symbols, argument checks and documented scratch size of the new C entries
(tests/test_gpu_condition_vr_grad.py runs them on the GPU)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from lcgp_amd import LCGP, synth
from oracle import lcgp_oracle as orc
from tests.test_condition_design_host import (DesignOracleEngine, KERNELS, _a256, _box, _pad, _std_args, augmented, vr_bytes)
from tests.test_condition_host import _free_port, patch_cond
from tests.vr_grad_ref import dkern3, kern3, value_and_grad

HERE = os.path.dirname(os.path.abspath(__file__))


def view_value_and_grad(th, low, x, sr, kernel, Un, LS, xn, xr, xc, w, r):
    """R' (n_cand,) and dR' (n_cand, d) of one component of a view, from the formulas of lcgp_condition_vr_grad: nothing of the
    augmented data is factorised -- low, U_n and L_S are the base model's factor and the view's state"""
    n, d = x.shape
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    coff = scale * (1.0 - nug / (1.0 + nug))

    def wide(xa):
        U = sla.solve_triangular(low, (coff * kern3(xa, x, ell, kernel) * sr[None, :]).T, lower=True).T
        T = sla.solve_triangular(LS, (coff * kern3(xa, xn, ell, kernel) - D * U @ Un.T).T, lower=True).T
        return np.hstack([U, T / np.sqrt(D)])
    wr, wc = wide(xr), wide(xc)
    sig = coff * kern3(xc, xr, ell, kernel) - D * wc @ wr.T             # Sigma'(t, c), (n_cand, n_ref)
    h = scale - D * np.sum(wc * wc, axis=1)
    den = np.maximum(h, 0.0) + 1.0 / (D * r)
    R = (sig * sig) @ w / den
    S = sig * w[None, :]
    t1 = np.einsum('ctl,ct->cl', coff * dkern3(xc, xr, ell, kernel), S)
    G = S @ wr                                                           # [G_U | G_T / sqrt(D)]
    Qn = sla.solve_triangular(LS, (np.sqrt(D) * G[:, n:]).T, lower=True, trans='T').T
    Qp = sla.solve_triangular(low, (G[:, :n] - Qn @ Un).T, lower=True, trans='T').T
    Rc = sla.solve_triangular(LS, (np.sqrt(D) * wc[:, n:]).T, lower=True, trans='T').T
    Vp = sla.solve_triangular(low, (wc[:, :n] - Rc @ Un).T, lower=True, trans='T').T
    dkc, dkn = coff * dkern3(xc, x, ell, kernel), coff * dkern3(xc, xn, ell, kernel)
    a1 = D * np.einsum('cjl,j,cj->cl', dkc, sr, Qp) + np.einsum('cal,ca->cl', dkn, Qn)
    dh = -2.0 * D * np.einsum('cjl,j,cj->cl', dkc, sr, Vp) - 2.0 * np.einsum('cal,ca->cl', dkn, Rc)
    dh[h <= 0.0] = 0.0
    return R, (2.0 * (t1 - a1) - R[:, None] * dh) / den[:, None]


class VrGradViewOracleEngine(DesignOracleEngine):
    """DesignOracleEngine plus condition_variance_reduction_grad_block in numpy; R' in the arithmetic of
    condition_variance_reduction_block (equal bit for bit away from matches)"""
    grad_calls = None

    def condition_variance_reduction_grad_block(self, state, x_cand_s, x_ref_s, w, r):
        assert self.is_current(state['theta'])
        if self.grad_calls is not None:
            self.grad_calls.append(x_ref_s is None)
        xc = np.asarray(x_cand_s, np.float64)
        xr = xc if x_ref_s is None else np.asarray(x_ref_s, np.float64)
        sr = np.ones(self.n) if self.sr is None else self.sr
        w = np.asarray(w, np.float64)
        dR = np.zeros((self.q_local, len(xc), self.x.shape[1]))
        for i, ((th, low, _, _), (Un, LS, _)) in enumerate(zip(self._state, state['state'])):
            _, dR[i] = view_value_and_grad(th, low, self.x, sr, self.kernel, Un, LS, state['xn'], xr, xc, w, r)
        R = self.condition_variance_reduction_block(state, x_cand_s, x_ref_s, w, None, r)
        return R, torch.as_tensor(dR)


def make_view_model(mode, kernel='matern32', d=2, m_new=5, group=None, q=2):
    """a model through the stand-in on non-unit input ranges and m_new new unique inputs (rep: 1 to 3 replicates each, shuffled)"""
    if mode == 'full':
        x, y = synth.make_full(81 + d, 30, d, 3, 2)
    else:
        x, y = synth.make_rep(82 + d, 14, 3, d, 3, 2)
    x = (-1.5 + 4.0 * np.asarray(x)) * (0.25 + np.arange(d))[None, :]
    m = patch_cond(LCGP(y=y, x=x, q=q, submethod=mode, kernel=kernel, process_group=group), VrGradViewOracleEngine)
    o = orc.OracleLCGP(y=y, x=x, q=q, submethod=mode)               # (only for the shape of the parameter vector)
    m._set_flat(synth.param_points(81, o.get_unconstrained())[1])
    rng = np.random.default_rng(17 + d + m_new)
    xn = _box(x, m_new, 40 + d + m_new)
    if mode == 'rep':
        xn = np.repeat(xn, 1 + np.arange(m_new) % 3, axis=0)
        xn = xn[rng.permutation(len(xn))]
    yn = rng.standard_normal((3, len(xn))) + 0.3
    return m, x, xn, yn


def _cands(m, x, view, k, seed):
    """raw-scale candidates: new points, a base training input and one of the view's own inputs, both given bitwise"""
    new = _box(x, k, seed)
    xt = m.x_unique.numpy() if m.submethod == 'rep' else x
    return np.vstack([new[:3], xt[4:5], view.x_new.numpy()[:1], new[3:]])


@pytest.mark.parametrize('m_new', [1, 7])
@pytest.mark.parametrize('d', [1, 2, 6])
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_view_gradient_equals_the_augmented_models_and_central_differences(mode, kernel, d, m_new):
    m, x, xn, yn = make_view_model(mode, kernel, d, m_new)
    view = m.condition(xn, yn)
    assert view.m == m_new
    xc, xr = _cands(m, x, view, 6, 3), _box(x, 9, 4)
    w = np.random.default_rng(5).random(9) + 0.1
    rows, xa, sa, lows = augmented(m, xn, yn)
    rng_x = x.max(axis=0) - x.min(axis=0)
    assert np.allclose(rng_x, (m.x_max - m.x_min).numpy().reshape(-1))
    for r in ((1, 3) if mode == 'rep' else (1,)):
        for ref, ww in ((None, None), (xr, w)):
            R, dR = (t.numpy() for t in view.variance_reduction_grad(xc, x_ref=ref, weights=ww, replicates=r, latent=True))
            assert R.shape == (2, len(xc)) and dR.shape == (2, len(xc), d)
            xr_s, xc_s, wn, _ = _std_args(m, xc, ref, ww)
            # (i) the gradient of a model built on the augmented data, per component at 1e-10 of max|ref|
            for k, (th, low) in enumerate(zip(rows, lows)):
                Rw, dRw = value_and_grad(th, low, xa, sa, m.kernel, xr_s, xc_s, wn, r)
                dRw = dRw / rng_x[None, :]
                assert np.max(np.abs(R[k] - Rw)) <= 1e-10 * np.max(np.abs(Rw)), (k, np.max(np.abs(R[k] - Rw)) / np.max(np.abs(Rw)))
                assert np.max(np.abs(dR[k] - dRw)) <= 1e-10 * np.max(np.abs(dRw)), \
                    (k, np.max(np.abs(dR[k] - dRw)) / np.max(np.abs(dRw)))
            # (ii) central differences of the closed-form view R' (x_ref held fixed: a copy of the candidates where it is None)
            held = xc.copy() if ref is None else ref
            fd = np.zeros_like(dR)
            for l in range(d):
                e = np.zeros(d)
                e[l] = 1e-5 * rng_x[l]
                fd[:, :, l] = (view.variance_reduction(xc + e, x_ref=held, weights=ww, replicates=r, latent=True).numpy()
                               - view.variance_reduction(xc - e, x_ref=held, weights=ww, replicates=r, latent=True).numpy()) / (2 * e[l])
            assert np.max(np.abs(dR - fd)) <= 1e-6 * np.max(np.abs(dR)), np.max(np.abs(dR - fd)) / np.max(np.abs(dR))


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_shapes_latent_outputs_weights_and_raw_scale(mode):
    m, x, xn, yn = make_view_model(mode)
    view = m.condition(xn, yn)
    xc, xr = _box(x, 6, 11), _box(x, 5, 12)
    w = np.array([1.0, 2.0, 0.0, 3.0, 4.0])
    R, dR = view.variance_reduction_grad(torch.as_tensor(xc), x_ref=torch.as_tensor(xr), weights=w, latent=True)
    for t in (R, dR):
        assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and not t.requires_grad
    assert R.shape == (2, 6) and dR.shape == (2, 6, 2)
    W, _, scale, _ = m._output_map()
    gain, dgain = view.variance_reduction_grad(xc, x_ref=xr, weights=w)
    assert gain.shape == (3, 6) and dgain.shape == (3, 6, 2)
    np.testing.assert_array_equal(gain.numpy(), (W ** 2).T @ R.numpy() * (scale ** 2)[:, None])
    np.testing.assert_allclose(dgain.numpy(), np.einsum('ka,kcl->acl', W ** 2, dR.numpy()) * (scale ** 2)[:, None, None], rtol=1e-14)
    g2, d2 = view.variance_reduction_grad(xc, x_ref=xr, weights=w, outputs=[2, 0])
    np.testing.assert_array_equal(g2.numpy(), gain.numpy()[[2, 0]])
    np.testing.assert_array_equal(d2.numpy(), dgain.numpy()[[2, 0]])
    # gain is the view's variance_reduction, bit for bit, in every form
    np.testing.assert_array_equal(R.numpy(), view.variance_reduction(xc, x_ref=xr, weights=w, latent=True).numpy())
    np.testing.assert_array_equal(gain.numpy(), view.variance_reduction(xc, x_ref=xr, weights=w).numpy())
    # weights are normalised; a zero weight drops its reference point
    keep = [0, 1, 3, 4]
    R3, dR3 = view.variance_reduction_grad(xc, x_ref=xr[keep], weights=10 * w[keep], latent=True)
    np.testing.assert_allclose(R3.numpy(), R.numpy(), rtol=1e-12)
    np.testing.assert_allclose(dR3.numpy(), dR.numpy(), rtol=1e-10, atol=1e-12 * np.max(np.abs(dR.numpy())))
    # the gradient is on the RAW input scale: the engine's (standardised) gradient divided by the input ranges
    eng = m._aux_engine
    xr_s, xc_s, wn, _ = _std_args(m, xc, xr, w)
    _, dstd = eng.condition_variance_reduction_grad_block(view._state, xc_s, xr_s, wn, 1)
    rng_x = (m.x_max - m.x_min).numpy().reshape(-1)
    assert np.max(np.abs(rng_x - 1.0)) > 0.5
    np.testing.assert_array_equal(dR.numpy(), dstd.numpy() / rng_x[None, None, :])
    # the view is not the base model, and the base model answers its own queries as before
    b0 = m.variance_reduction(xc, x_ref=xr, weights=w, latent=True).numpy()
    assert np.max(np.abs(R.numpy() - b0)) > 1e-4 * np.max(np.abs(b0))
    view.variance_reduction_grad(xc)
    assert m._aux_engine is eng and np.array_equal(m.variance_reduction(xc, x_ref=xr, weights=w, latent=True).numpy(), b0)


def test_rep_candidates_at_training_and_view_inputs_get_the_continuous_surface():
    m, x, xn, yn = make_view_model('rep')
    view = m.condition(xn, yn)
    xu = m.x_unique.numpy()
    xc = np.vstack([_box(x, 3, 13), xu[[4, 9]], view.x_new.numpy()[2:3]])
    xr = _box(x, 8, 14)
    # variance_reduction refuses the view's input and adds replicates at the base inputs ...
    with pytest.raises(ValueError, match='equals one of the new inputs'):
        view.variance_reduction(xc, x_ref=xr, replicates=2)
    Rv = view.variance_reduction(xc[:5], x_ref=xr, replicates=2, latent=True).numpy()
    # ... the gradient call takes every candidate as a new input
    R, dR = (t.numpy() for t in view.variance_reduction_grad(xc, x_ref=xr, replicates=2, latent=True))
    np.testing.assert_array_equal(R[:, :3], Rv[:, :3])
    assert np.all(np.abs(R[:, 3:5] - Rv[:, 3:5]) > 1e-6 * np.abs(Rv[:, 3:5]))
    rows, xa, sa, lows = augmented(m, xn, yn)
    xr_s, xc_s, wn, _ = _std_args(m, xc, xr, None)
    rng_x = (m.x_max - m.x_min).numpy().reshape(-1)
    for k, (th, low) in enumerate(zip(rows, lows)):
        Rw, dRw = value_and_grad(th, low, xa, sa, m.kernel, xr_s, xc_s, wn, 2)
        np.testing.assert_allclose(R[k], Rw, rtol=0, atol=1e-10 * np.max(np.abs(Rw)))
        np.testing.assert_allclose(dR[k], dRw / rng_x[None, :], rtol=0, atol=1e-10 * np.max(np.abs(dRw / rng_x[None, :])))
    # the surface is continuous through the three points: central differences of variance_reduction around them
    for l in range(2):
        e = np.zeros(2)
        e[l] = 1e-5 * rng_x[l]
        fd = (view.variance_reduction(xc[3:] + e, x_ref=xr, replicates=2, latent=True).numpy()
              - view.variance_reduction(xc[3:] - e, x_ref=xr, replicates=2, latent=True).numpy()) / (2 * e[l])
        assert np.max(np.abs(dR[:, 3:, l] - fd)) <= 1e-6 * np.max(np.abs(dR))
    # x_ref=None with such candidates: no ValueError either
    assert view.variance_reduction_grad(xc, replicates=3)[1].shape == (3, 6, 2)


def test_every_value_error_of_vr_arguments():
    m, x, xn, yn = make_view_model('full')
    view = m.condition(xn, yn)
    xc = x[:4] + 0.01
    for kw, msg in (({'x_cand': np.zeros((3, 3))}, 'x_cand'), ({'x_cand': np.zeros((0, 2))}, 'x_cand'), ({'x_ref': np.zeros((3, 1))}, 'x_ref'),
                    ({'weights': [1, 2, 3]}, 'length'), ({'weights': [1, -1, 1, 1]}, 'non-negative'),
                    ({'weights': [1, np.nan, 1, 1]}, 'finite'), ({'weights': [1, np.inf, 1, 1]}, 'finite'),
                    ({'weights': [0, 0, 0, 0]}, 'all be zero'), ({'outputs': [3]}, 'outputs'), ({'outputs': [-1]}, 'outputs'),
                    ({'replicates': 0}, 'replicates'), ({'replicates': 1.5}, 'replicates'), ({'replicates': True}, 'replicates'),
                    ({'replicates': 2}, 'full path')):
        args = dict(x_cand=xc)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            view.variance_reduction_grad(**args)
        with pytest.raises(ValueError, match=msg):
            view.variance_reduction_differentiable(**args)
    mr, xr_, xnr, ynr = make_view_model('rep')
    vr = mr.condition(xnr, ynr)
    with pytest.raises(ValueError, match='replicates'):
        vr.variance_reduction_grad(mr.x_unique.numpy()[:2], replicates=0)
    assert vr.variance_reduction_grad(mr.x_unique.numpy()[:2], replicates=2)[1].shape == (3, 2, 2)


def test_the_gradient_goes_stale_with_the_view():
    m, x, xn, yn = make_view_model('full')
    view = m.condition(xn, yn)
    xc = x[:4] + 0.01
    view.variance_reduction_grad(xc)
    u = m._get_flat().copy()
    m._set_flat(u + 0.01)
    calls = (lambda: view.variance_reduction_grad(xc), lambda: view.variance_reduction_differentiable(torch.as_tensor(xc)))
    for call in calls:
        with pytest.raises(RuntimeError, match='stale'):
            call()
    m.predict(xc)
    m._set_flat(u)
    for call in calls:
        with pytest.raises(RuntimeError, match='stale'):
            call()
    assert m.condition(xn, yn).variance_reduction_grad(xc)[1].shape == (3, 4, 2)


def test_autograd_gradcheck_no_double_backward_and_constant_reference_copy():
    m, x, xn, yn = make_view_model('full')
    view = m.condition(xn, yn)
    xr = _box(x, 7, 21)
    xc = torch.tensor(_box(x, 4, 22), requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: view.variance_reduction_differentiable(t, x_ref=xr), (xc,), eps=1e-6, atol=1e-7,
                                    rtol=1e-5, nondet_tol=0.0)
    assert torch.autograd.gradcheck(lambda t: view.variance_reduction_differentiable(t, x_ref=xr, latent=True,
                                                                                     weights=np.arange(1.0, 8.0)),
                                    (xc,), eps=1e-6, atol=1e-7, rtol=1e-5)
    out = view.variance_reduction_differentiable(xc, x_ref=xr)
    assert out.shape == (int(m.p), 4) and out.requires_grad and out.dtype == torch.float64
    np.testing.assert_array_equal(out.detach().numpy(), view.variance_reduction(xc.detach().numpy(), x_ref=xr).numpy())
    with pytest.raises(RuntimeError, match='first derivatives only'):
        torch.autograd.grad(out.sum(), xc, create_graph=True)
    # x_ref=None: the engine is told the reference set is the candidates', and nothing flows through that copy
    eng = m._aux_engine
    eng.grad_calls = []
    (ga,) = torch.autograd.grad(view.variance_reduction_differentiable(xc).sum(), xc)
    (gb,) = torch.autograd.grad(view.variance_reduction_differentiable(xc, x_ref=xc.detach().numpy().copy()).sum(), xc)
    assert eng.grad_calls == [True, False]
    np.testing.assert_allclose(ga.numpy(), gb.numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(ga.numpy(), view.variance_reduction_grad(xc.detach().numpy())[1].sum(dim=0).numpy(), rtol=1e-12)
    # a numpy candidate set is accepted (no gradient is asked for)
    assert view.variance_reduction_differentiable(xc.detach().numpy(), x_ref=xr).shape == (3, 4)


def test_two_ranks_gather_what_one_rank_computes():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_condition_vr_grad_host_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def vr_grad_bytes(esz, n, d, q, m, n_ref, n_cand):
    """lcgp_condition_vr_grad_scratch_bytes as include/lcgp_hip.h documents it (m = 0: lcgp_variance_reduction_grad_scratch_bytes)"""
    npad, mpad = -(-n // 128) * 128, -(-m // 128) * 128
    c, rp = _pad(n_cand), -(-n_ref // 128) * 128
    extra = _a256(q * c * rp * esz) + _a256(q * c * (npad + mpad) * esz) + _a256(q * c * npad * esz) + 3 * _a256(q * n_cand * d * 8) + \
        (_a256(q * c * npad * esz) if m else 0) + 2 * _a256(q * c * mpad * esz)
    return vr_bytes(esz, n, q, m, n_ref, n_cand) + extra


def test_new_symbols_version_and_documented_size():
    from lcgp_amd import _hip
    from lcgp_amd.engine import HotPathEngine
    from lcgp_amd.lcgp import ConditionedLCGP
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() == 610
    for name in ('lcgp_condition_vr_grad_scratch_bytes', 'lcgp_condition_vr_grad'):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    assert hasattr(HotPathEngine, 'condition_variance_reduction_grad_block')
    assert hasattr(ConditionedLCGP, 'variance_reduction_grad') and hasattr(ConditionedLCGP, 'variance_reduction_differentiable')
    nb = C.c_size_t(0)
    for dtype, esz in ((0, 8), (1, 4)):
        for m in (32, 1024):
            assert lib.lcgp_condition_vr_grad_scratch_bytes(dtype, 4096, 6, 8, m, 2000, 2000, C.byref(nb)) == 0
            assert nb.value == vr_grad_bytes(esz, 4096, 6, 8, m, 2000, 2000)
        # the same formula with no view columns is the fitted model's size: the layout is one
        assert lib.lcgp_variance_reduction_grad_scratch_bytes(dtype, 4096, 6, 8, 2000, 2000, C.byref(nb)) == 0
        assert nb.value == vr_grad_bytes(esz, 4096, 6, 8, 0, 2000, 2000)
    for args in ((333, 1, 3, 1, 1, 1), (333, 6, 3, 70, 130, 130), (333, 40, 3, 150, 130, 2100), (333, 6, 1, 150, 2100, 37)):
        assert lib.lcgp_condition_vr_grad_scratch_bytes(0, *args, C.byref(nb)) == 0
        assert nb.value == vr_grad_bytes(8, *args)
        assert lib.lcgp_variance_reduction_grad_scratch_bytes(1, args[0], args[1], args[2], args[4], args[5], C.byref(nb)) == 0
        assert nb.value == vr_grad_bytes(4, args[0], args[1], args[2], 0, args[4], args[5])
    for args, msg in (((0, 4096, 6, 8, 0, 10, 10), b'm < 1'), ((0, 4096, 6, 8, 5, 0, 10), b'n_ref'), ((0, 4096, 6, 8, 5, 10, 0), b'n_cand'),
                      ((0, 4096, 6, 8, 5, 10, 70000), b'n_cand must be <='), ((0, 4096, 127, 8, 5, 10, 10), b'd must be'),
                      ((2, 4096, 6, 8, 5, 10, 10), b'dtype'), ((0, 0, 6, 8, 5, 10, 10), b'n < 1'),
                      ((0, 4096, 6, 65536, 5, 10, 10), b'q_local')):
        assert lib.lcgp_condition_vr_grad_scratch_bytes(*args, C.byref(nb)) < 0, args
        assert msg in lib.lcgp_last_error(), (args, lib.lcgp_last_error())
    assert lib.lcgp_condition_vr_grad_scratch_bytes(0, 4096, 6, 8, 5, 10, 10, None) < 0


def test_c_abi_argument_checks():
    """every call below is refused on the host before anything is enqueued: the pointers are never dereferenced"""
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    dummy = C.c_void_p(16)
    big = 1 << 40
    nb = C.c_size_t(0)
    assert lib.lcgp_condition_vr_grad_scratch_bytes(0, 50, 2, 2, 4, 10, 4, C.byref(nb)) == 0
    need = nb.value

    def vg(dtype=0, kern=0, n=50, d=2, q=2, m=4, nr=10, nc=4, x=dummy, theta=dummy, ws=dummy, state=dummy, xn=dummy, xr=dummy,
           w=dummy, xc=dummy, row0=-1, r=1, scratch=dummy, nsc=big, out=dummy, stride=0, dout=dummy):
        return lib.lcgp_condition_vr_grad(None, dtype, kern, n, d, 3, q, x, None, theta, ws, state, m, xn, nr, xr, w, nc, xc, row0, r,
                                          scratch, nsc, out, stride, dout)

    cases = [(dict(m=0), 'm < 1'), (dict(dtype=2), 'dtype'), (dict(d=0), 'd must be'), (dict(d=127), 'd must be'),
             (dict(n=0), 'n < 1'), (dict(q=0), 'q_local'), (dict(q=65536), 'q_local'), (dict(nr=0), 'n_ref'), (dict(nc=0), 'n_cand'),
             (dict(nc=70000), 'n_cand must be <='), (dict(kern=3), 'kernel_id'), (dict(r=0), 'r must be'),
             (dict(row0=-2), 'cand_row0'), (dict(row0=8, nc=4, xc=None), 'cand_row0 + n_cand'),
             (dict(row0=0), 'x_cand must be NULL'), (dict(xc=None), 'NULL'), (dict(x=None), 'NULL'), (dict(theta=None), 'NULL'),
             (dict(ws=None), 'NULL'), (dict(state=None), 'NULL'), (dict(xn=None), 'NULL'), (dict(xr=None), 'NULL'),
             (dict(w=None), 'NULL'), (dict(scratch=None), 'NULL'), (dict(out=None), 'NULL'), (dict(dout=None), 'NULL'),
             (dict(stride=3), 'out_stride'), (dict(nsc=need - 1), 'scratch is smaller'), (dict(nsc=0), 'scratch is smaller')]
    for kw, msg in cases:
        assert vg(**kw) == -1, kw
        assert msg.encode() in lib.lcgp_last_error(), (kw, lib.lcgp_last_error())
