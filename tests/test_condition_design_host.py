"""CPU tests of the design queries on a conditioned view (ConditionedLCGP.variance_reduction / select_batch): a numpy stand-in
of HotPathEngine.condition_variance_reduction_block / condition_select_* written in the closed form of include/lcgp_hip.h
(the widened rows [U_a | T_a / sqrt(D)]), checked against brute force on the augmented data (refactor I + D (C o s s^T), the
closed form of the fitted model's variance reduction, dense rank-one updates pick by pick); the host layer -- the output map,
outputs=, weights=, latent=, every ValueError of the base methods, the rep path's refusal of a candidate that is one of the
view's inputs, staleness, the gather over ranks -- through that stand-in; the select / condition identity; and the symbols,
argument checks and documented sizes of the new C entries (tests/test_gpu_condition_design.py runs them on the GPU)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from tests import matern52_oracle as m52
from tests.test_condition_host import CondOracleEngine, _free_port, make_model, new_columns, patch_cond
from tests.test_predict_hess_host import _cross
from tests.test_select_batch_host import DenseState, SelectOracleEngine, omega_of, parts
from tests.test_variance_reduction_host import _kern, closed_form

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = ('matern32', 'se', 'matern52')


# ---- dense float64 references on any of the three kernels -------------------------------------------------------------------
def _cx(xa, xb, ell, scale, nug, kernel):
    """C^x(xa, xb): the kernel WITHOUT a nugget term, also where the two sets are one (tests.test_predict_hess_host._cross puts
    the nugget on the diagonal then, as the reference's covariance function does)"""
    if kernel == 'matern52':
        return m52.kernel_matrix(xa, xb, ell, scale, nug, same=False)
    return scale * (1.0 - nug / (1.0 + nug)) * _kern(xa, xb, ell, kernel)


def parts3(th, low, x, s, kernel, xr, xc, match):
    """test_select_batch_host.parts on all three kernels: D, scale, U_ref, U_cand, C^x(ref, cand), C^x(cand, cand)"""
    d = x.shape[1]
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    cc = _cx(xc, x, ell, scale, nug, kernel)
    if match is not None:
        for j, i in enumerate(match):
            if i >= 0:
                cc[j, i] += scale * nug / (1.0 + nug)
    uc = sla.solve_triangular(low, (cc * s[None, :]).T, lower=True).T
    ur = sla.solve_triangular(low, (_cx(xr, x, ell, scale, nug, kernel) * s[None, :]).T, lower=True).T
    return D, scale, ur, uc, _cx(xr, xc, ell, scale, nug, kernel), _cx(xc, xc, ell, scale, nug, kernel)


class DenseState3(DenseState):
    """test_select_batch_host.DenseState (its rows() and condition()) built with any of the three kernels"""

    def __init__(self, th, low, x, s, kernel, xr, xc, w, match, r):
        D, scale, ur, uc, crc, ccc = parts3(th, low, x, s, kernel, xr, xc, match)
        self.src = crc - D * ur @ uc.T
        self.scc = ccc - D * uc @ uc.T
        np.fill_diagonal(self.scc, scale - D * np.sum(uc * uc, axis=1))
        self.w, self.tau = np.asarray(w, np.float64), 1.0 / (D * r)


def closed_form3(th, low, x, s, kernel, xr, xc, w, match, r):
    """test_variance_reduction_host.closed_form with any of the three kernels"""
    return DenseState3(th, low, x, s, kernel, xr, xc, w, match, r).rows()


def _references_are_the_projects_own(kernel):
    """DenseState3 / closed_form3 against DenseState / closed_form on the two kernels those know (called by the ALC test)"""
    rng = np.random.default_rng(2)
    x, xr, xc = rng.random((12, 2)), rng.random((5, 2)), rng.random((4, 2))
    th = np.array([0.4, 0.7, 1.3, 0.05, 2.0])
    s = np.sqrt(rng.integers(1, 4, 12).astype(float))
    C0 = _cross(x, x, th[:2], th[2], th[3], kernel)
    np.fill_diagonal(C0, th[2])
    low = np.linalg.cholesky(np.eye(12) + th[4] * C0 * np.outer(s, s))
    w = rng.random(5)
    match = np.array([-1, 3, -1, -1])
    a, b = DenseState3(th, low, x, s, kernel, xr, xc, w, match, 2), DenseState(th, low, x, s, kernel, xr, xc, w, match, 2)
    np.testing.assert_allclose(a.src, b.src, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(a.scc, b.scc, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(closed_form3(th, low, x, s, kernel, xr, xc, w, match, 2),
                               closed_form(th, low, x, s, kernel, xr, xc, w, match, 2), rtol=1e-12)
    assert len(parts(th, low, x, s, kernel, xr, xc, match)) == 6


# ---- the stand-in engine ----------------------------------------------------------------------------------------------------
class _ViewState(DenseState):
    """DenseState's rows() / condition() on the posterior covariance of a conditioned view"""

    def __init__(self, src, scc, w, tau):
        self.src, self.scc, self.w, self.tau = src, scc, np.asarray(w, np.float64), tau


class DesignOracleEngine(CondOracleEngine, SelectOracleEngine):
    """CondOracleEngine plus the design queries on a view in the closed form of include/lcgp_hip.h, in float64 numpy: widened rows
    U^_a = [U_a | T_a / sqrt(D)], Sigma' = C - D U^_t . U^_c, gvar' = scale - D |U^_c|^2 (and the fitted model's
    variance_reduction_block / select_* of SelectOracleEngine, the parent's side of the select / condition identity)"""

    def _view_states(self, state, x_cand_s, x_ref_s, w, match, r):
        assert self.is_current(state['theta'])
        xc = np.asarray(x_cand_s, np.float64)
        xr = xc if x_ref_s is None else np.asarray(x_ref_s, np.float64)
        sr = np.ones(self.n) if self.sr is None else self.sr
        xn, out = state['xn'], []
        for (th, low, z, b), (Un, LS, v) in zip(self._state, state['state']):
            d = self.x.shape[1]
            ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]

            def wide(xa, mt):
                ca = _cx(xa, self.x, ell, scale, nug, self.kernel)
                if mt is not None:
                    for j, i in enumerate(mt):
                        if i >= 0:
                            ca[j, i] += scale * nug / (1.0 + nug)
                U = sla.solve_triangular(low, (ca * sr[None, :]).T, lower=True).T
                T = sla.solve_triangular(LS, (_cx(xa, xn, ell, scale, nug, self.kernel) - D * U @ Un.T).T, lower=True).T
                return np.hstack([U, T / np.sqrt(D)])
            wr, wc = wide(xr, None), wide(xc, match)
            src = _cx(xr, xc, ell, scale, nug, self.kernel) - D * wr @ wc.T
            scc = _cx(xc, xc, ell, scale, nug, self.kernel) - D * wc @ wc.T
            np.fill_diagonal(scc, scale - D * np.sum(wc * wc, axis=1))
            out.append(_ViewState(src, scc, w, 1.0 / (D * r)))
        return out

    def condition_variance_reduction_block(self, state, x_cand_s, x_ref_s, w, match, r):
        return torch.as_tensor(np.array([st.rows() for st in self._view_states(state, x_cand_s, x_ref_s, w, match, r)]))

    def condition_select_begin(self, state, x_cand_s, x_ref_s, w, match, r, size):
        self._sel = self._view_states(state, x_cand_s, x_ref_s, w, match, r)

    def condition_select_rows(self):
        return self.select_rows()

    def condition_select_condition(self, j):
        return self.select_condition(j)

    def condition_select_batch_block(self, state, x_cand_s, x_ref_s, w, match, r, size, omega):
        begin = self.select_begin
        self.select_begin = lambda xc, xr, w_, mt, r_, size_: self.condition_select_begin(state, xc, xr, w_, mt, r_, size_)
        try:
            return self.select_batch_block(x_cand_s, x_ref_s, w, match, r, size, omega)
        finally:
            self.select_begin = begin


def design_model(mode, kernel='matern32', d=2, group=None, **kw):
    m, x, y, xn, yn = make_model(mode, kernel, d, group, **kw)
    return patch_cond(m, DesignOracleEngine), x, y, xn, yn


def _box(x, k, seed):
    lo, hi = x.min(axis=0), x.max(axis=0)
    return lo + (hi - lo) * np.random.default_rng(seed).random((k, x.shape[1]))


def _cands(m, x, k, seed):
    """raw-scale candidates: new points, plus (rep path) two base training inputs given bitwise"""
    new = _box(x, k, seed)
    return np.vstack([new[:3], m.x_unique.numpy()[[4, 9]], new[3:]]) if m.submethod == 'rep' else new


def augmented(m, xn, yn):
    """theta rows, the augmented training set (inputs, sqrt(r)) and its dense float64 factors, one per component"""
    eng = m._aux_engine
    s = np.ones(eng.n) if eng.sr is None else eng.sr
    xn_s, snew, _ = new_columns(m, xn, yn)
    xa, sa = np.vstack([eng.x, xn_s]), np.r_[s, snew]
    rows, d = eng._theta_last, eng.x.shape[1]
    lows = []
    for th in rows:
        Cm = _cross(xa, xa, th[:d], th[d], th[d + 1], eng.kernel)
        np.fill_diagonal(Cm, th[d])
        lows.append(np.linalg.cholesky(np.eye(len(xa)) + th[d + 2] * Cm * np.outer(sa, sa)))
    return rows, xa, sa, lows


def _std_args(m, xc, xr, w):
    xc_s = m._standardise_x0(xc)[0]
    xr_s = xc_s if xr is None else m._standardise_x0(xr)[0]
    wn = np.full(len(xr_s), 1.0 / len(xr_s)) if w is None else np.asarray(w, float) / np.sum(w)
    match = None
    if m.submethod == 'rep':
        xt = m._x_train()
        match = np.array([int(np.flatnonzero(np.all(xt == c[None, :], axis=1))[0]) if np.any(np.all(xt == c[None, :], axis=1))
                          else -1 for c in xc_s])
    return xr_s, xc_s, wn, match


@pytest.mark.parametrize('d', [1, 6])
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_view_alc_equals_brute_force_on_the_augmented_data(mode, kernel, d):
    if kernel != 'matern52' and mode == 'full' and d == 1:
        _references_are_the_projects_own(kernel)
    m, x, _, xn, yn = design_model(mode, kernel, d)
    view = m.condition(xn, yn)
    xc, xr = _cands(m, x, 7, 3), _box(x, 9, 4)
    w = np.random.default_rng(5).random(9) + 0.1
    rows, xa, sa, lows = augmented(m, xn, yn)
    for r in ((1, 3) if mode == 'rep' else (1,)):
        for ref, ww in ((None, None), (xr, w)):
            R = view.variance_reduction(xc, x_ref=ref, weights=ww, replicates=r, latent=True).numpy()
            xr_s, xc_s, wn, match = _std_args(m, xc, ref, ww)
            if mode == 'rep':
                assert np.sum(match >= 0) == 2
            want = np.array([closed_form3(th, low, xa, sa, m.kernel, xr_s, xc_s, wn, match, r) for th, low in zip(rows, lows)])
            assert R.shape == want.shape == (2, len(xc))
            np.testing.assert_allclose(R, want, rtol=0, atol=1e-9 * np.max(np.abs(want)))
            # the new runs took variance away: the view's reduction is not the base model's
            base = m.variance_reduction(xc, x_ref=ref, weights=ww, replicates=r, latent=True).numpy()
            assert np.max(np.abs(R - base)) > 1e-4 * np.max(np.abs(base))


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_view_select_batch_equals_dense_states_on_the_augmented_data(mode, kernel):
    m, x, _, xn, yn = design_model(mode, kernel, 2)
    view = m.condition(xn, yn)
    xc, xr = _cands(m, x, 8, 6), _box(x, 9, 7)
    rows, xa, sa, lows = augmented(m, xn, yn)
    om = omega_of(m)
    size = 5
    for r in ((1, 3) if mode == 'rep' else (1,)):
        for ref in (None, xr):
            idx, gain, scores = (t.numpy() for t in view.select_batch(xc, size, x_ref=ref, replicates=r, return_scores=True))
            assert idx.dtype == np.int64 and idx.shape == (size,) and gain.shape == (size,) and scores.shape == (size, len(xc))
            assert len(set(idx.tolist())) == size
            xr_s, xc_s, wn, match = _std_args(m, xc, ref, None)
            states = [DenseState3(th, low, xa, sa, m.kernel, xr_s, xc_s, wn, match, r) for th, low in zip(rows, lows)]
            R0 = view.variance_reduction(xc, x_ref=ref, replicates=r, latent=True).numpy()
            np.testing.assert_allclose(scores[0], om @ R0, rtol=1e-12)
            for t in range(size):
                want = om @ np.array([st.rows() for st in states])
                live = np.setdiff1d(np.arange(len(xc)), idx[:t])
                assert np.all(np.isneginf(scores[t, idx[:t]]))
                np.testing.assert_allclose(scores[t, live], want[live], rtol=0, atol=1e-9 * np.max(np.abs(want)))
                assert idx[t] == np.argmax(scores[t]) and gain[t] == scores[t, idx[t]]
                for st in states:
                    st.condition(int(idx[t]))
            assert np.all(np.diff(gain) <= 1e-12 * gain[0])


@pytest.mark.parametrize('kernel', ['matern32', 'se'])
def test_select_condition_identity(kernel):
    """step t's score row of base.select_batch equals sum_k omega_k R'_k of the view conditioned on the first t picks (full
    path, r = 1; ALC ignores the outputs handed to condition()); candidates already picked are excluded.  The two kernels of
    SelectOracleEngine, the stand-in of the fitted model's select_batch (tests/test_gpu_condition_design.py: on the GPU)."""
    m, x, _, _, _ = design_model('full', kernel, 2)
    xc, xr = _box(x, 9, 8), _box(x, 11, 9)
    idx, _, scores = (t.numpy() for t in m.select_batch(xc, 4, x_ref=xr, return_scores=True))
    om = omega_of(m)
    y_any = np.random.default_rng(10).standard_normal((3, 4))
    for t in range(1, 4):
        R = m.condition(xc[idx[:t]], y_any[:, :t]).variance_reduction(xc, xr, latent=True).numpy()
        live = np.setdiff1d(np.arange(len(xc)), idx[:t])
        np.testing.assert_allclose((om @ R)[live], scores[t, live], rtol=0, atol=1e-10 * np.max(scores[0]))


# ---- the host layer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_output_map_outputs_weights_and_latent(mode):
    m, x, _, xn, yn = design_model(mode)
    view = m.condition(xn, yn)
    xc, xr = _cands(m, x, 6, 11), _box(x, 5, 12)
    w = np.array([1.0, 2.0, 0.0, 3.0, 4.0])
    R = view.variance_reduction(torch.as_tensor(xc), x_ref=torch.as_tensor(xr), weights=w, latent=True)
    assert isinstance(R, torch.Tensor) and R.dtype == torch.float64 and R.shape == (2, len(xc)) and not R.requires_grad
    W, _, scale, _ = m._output_map()
    full = view.variance_reduction(xc, x_ref=xr, weights=w)
    assert full.shape == (3, len(xc)) and full.dtype == torch.float64
    np.testing.assert_array_equal(full.numpy(), (W ** 2).T @ R.numpy() * (scale ** 2)[:, None])
    sub = view.variance_reduction(xc, x_ref=xr, weights=w, outputs=[2, 0])
    np.testing.assert_array_equal(sub.numpy(), full.numpy()[[2, 0]])
    # weights are normalised; a zero weight drops its reference point
    keep = [0, 1, 3, 4]
    np.testing.assert_allclose(view.variance_reduction(xc, x_ref=xr[keep], weights=10 * w[keep], latent=True).numpy(), R.numpy(),
                               rtol=1e-12)
    # select_batch: omega from the chosen outputs, gain = the picked entries, the same picks with and without scores
    idx, gain, scores = view.select_batch(xc, 3, x_ref=xr, weights=w, outputs=[1], return_scores=True)
    i2, g2 = view.select_batch(xc, 3, x_ref=xr, weights=w, outputs=[1])
    assert torch.equal(idx, i2) and torch.equal(gain, g2) and scores.shape == (3, len(xc))
    np.testing.assert_allclose(scores[0].numpy(), omega_of(m, [1]) @ R.numpy(), rtol=1e-12)
    # the base model is only read, and answers its own queries as before
    eng = m._aux_engine
    b0 = m.variance_reduction(xc, x_ref=xr, weights=w, latent=True).numpy()
    view.variance_reduction(xc, latent=True)
    assert m._aux_engine is eng and np.array_equal(m.variance_reduction(xc, x_ref=xr, weights=w, latent=True).numpy(), b0)


def test_every_value_error_of_the_base_methods():
    m, x, _, xn, yn = design_model('full')
    view = m.condition(xn, yn)
    xc = x[:4] + 0.01
    for kw, msg in (({'x_cand': np.zeros((3, 3))}, 'x_cand'), ({'x_ref': np.zeros((3, 1))}, 'x_ref'),
                    ({'weights': [1, 2, 3]}, 'length'), ({'weights': [1, -1, 1, 1]}, 'non-negative'),
                    ({'weights': [1, np.nan, 1, 1]}, 'finite'), ({'weights': [1, np.inf, 1, 1]}, 'finite'),
                    ({'weights': [0, 0, 0, 0]}, 'all be zero'), ({'outputs': [3]}, 'outputs'), ({'outputs': [-1]}, 'outputs'),
                    ({'replicates': 0}, 'replicates'), ({'replicates': 1.5}, 'replicates'), ({'replicates': 2}, 'full path')):
        args = dict(x_cand=xc)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            view.variance_reduction(**args)
        with pytest.raises(ValueError, match=msg):
            view.select_batch(size=2, **args)
    for size in (0, 5, 1.5, True):
        with pytest.raises(ValueError, match='size must be'):
            view.select_batch(xc, size)
    with pytest.raises(ValueError, match='duplicate rows'):
        view.select_batch(np.vstack([xc, xc[1:2]]), 2)
    mr, xr_, _, xnr, ynr = design_model('rep')
    vr = mr.condition(xnr, ynr)
    with pytest.raises(ValueError, match='replicates'):
        vr.variance_reduction(mr.x_unique.numpy()[:2], replicates=0)
    assert vr.variance_reduction(mr.x_unique.numpy()[:2], replicates=2).shape == (3, 2)


def test_rep_path_refuses_a_candidate_that_is_one_of_the_views_inputs():
    m, x, _, xn, yn = design_model('rep')
    view = m.condition(xn, yn)
    xc = np.vstack([_box(x, 3, 13), view.x_new.numpy()[2:3]])
    for call in (lambda: view.variance_reduction(xc), lambda: view.select_batch(xc, 2),
                 lambda: view.variance_reduction(xc, x_ref=_box(x, 4, 14), replicates=2)):
        with pytest.raises(ValueError, match='equals one of the new inputs.*refit'):
            call()
    # as a REFERENCE point it is a new input like any other
    assert view.variance_reduction(xc[:3], x_ref=xc).shape == (3, 3)
    # full path: such a candidate is one more new row with its own nugget -- the base model's rule -- and equals brute force
    mf, xf, _, xnf, ynf = design_model('full')
    vf = mf.condition(xnf, ynf)
    xcf = np.vstack([_box(xf, 3, 15), xnf[1:2]])
    R = vf.variance_reduction(xcf, latent=True).numpy()
    rows, xa, sa, lows = augmented(mf, xnf, ynf)
    xr_s, xc_s, wn, match = _std_args(mf, xcf, None, None)
    want = np.array([closed_form3(th, low, xa, sa, mf.kernel, xr_s, xc_s, wn, None, 1) for th, low in zip(rows, lows)])
    np.testing.assert_allclose(R, want, rtol=0, atol=1e-9 * np.max(np.abs(want)))


def test_design_queries_go_stale_with_the_view():
    m, x, _, xn, yn = design_model('full')
    view = m.condition(xn, yn)
    xc = x[:4] + 0.01
    view.variance_reduction(xc)
    u = m._get_flat().copy()
    m._set_flat(u + 0.01)
    for call in (lambda: view.variance_reduction(xc), lambda: view.select_batch(xc, 2)):
        with pytest.raises(RuntimeError, match='stale'):
            call()
    m.predict(xc)
    m._set_flat(u)
    for call in (lambda: view.variance_reduction(xc), lambda: view.select_batch(xc, 2)):
        with pytest.raises(RuntimeError, match='stale'):
            call()
    assert m.condition(xn, yn).select_batch(xc, 2)[0].shape == (2,)


def test_two_ranks_gather_what_one_rank_computes():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_condition_design_host_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ('lcgp_condition_vr_scratch_bytes', 'lcgp_condition_vr_prepare', 'lcgp_condition_vr',
               'lcgp_condition_select_scratch_bytes', 'lcgp_condition_select_begin', 'lcgp_condition_select_score',
               'lcgp_condition_select_condition', 'lcgp_condition_select_picks', 'lcgp_condition_select_state')


def _a256(v):
    return -(-v // 256) * 256


def _pad(v):
    return -(-v // 128) * 128 if v >= 128 else -(-v // 64) * 64


def vr_bytes(esz, n, q, m, n_ref, n_cand):
    """lcgp_condition_vr_scratch_bytes as include/lcgp_hip.h documents it (m = 0: lcgp_variance_reduction_scratch_bytes)"""
    npad, mpad = -(-n // 128) * 128, -(-m // 128) * 128
    kp = npad + mpad
    xr, xc = min(2048, _pad(n_ref)), min(2048, _pad(n_cand))
    ref = _a256(q * (-(-n_ref // 128) * 128 + 64) * kp * esz) + 2 * _a256(q * n_ref * 8) + _a256(q * xr * npad * esz) + \
        _a256(2 * q * xr * mpad * esz)
    cand = _a256(q * _pad(n_cand) * kp * esz) + 2 * _a256(q * n_cand * 8) + _a256(q * xc * npad * esz) + \
        _a256(2 * q * xc * mpad * esz) + _a256(q * -(-n_ref // 64) * (-(-n_cand // 64) * 64) * 8)
    return ref + cand


def select_bytes(esz, n, d, q, m, n_ref, n_cand, size):
    """lcgp_condition_select_scratch_bytes as include/lcgp_hip.h documents it (m = 0: lcgp_select_scratch_bytes)"""
    npad, mpad = -(-n // 128) * 128, -(-m // 128) * 128
    kp = npad + mpad
    xr = min(2048, max(_pad(n_ref), _pad(n_cand)))
    u = _a256(q * (-(-n_ref // 128) * 128 + 64) * kp * esz) + _a256(q * (_pad(n_cand) + 128) * kp * esz) + \
        _a256(q * xr * npad * esz) + _a256(2 * q * xr * mpad * esz)
    dbl = 2 * _a256(q * n_ref * 8) + 2 * _a256(q * n_cand * 8) + _a256(q * -(-n_ref // 64) * (-(-n_cand // 64) * 64) * 8) + \
        _a256(q * n_cand * 8) + _a256(q * size * n_cand * 8) + _a256(q * size * n_ref * 8) + \
        _a256(q * -(-n_ref // 32) * kp * 8) + _a256(q * kp * 8) + _a256(q * size * 8) + _a256(q * n_ref * d * 8) + \
        _a256(q * n_cand * d * 8) + _a256(n_ref * 8)
    return u + dbl + _a256(n_cand * 4) + _a256(size * 4)


def test_new_symbols_version_and_documented_sizes():
    from lcgp_amd import _hip
    from lcgp_amd.engine import HotPathEngine
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() == 610
    for name in NEW_SYMBOLS:
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    for name in ('condition_variance_reduction_block', 'condition_select_begin', 'condition_select_rows',
                 'condition_select_condition', 'condition_select_batch_block'):
        assert hasattr(HotPathEngine, name)
    nb = C.c_size_t(0)
    for dtype, esz in ((0, 8), (1, 4)):
        for m in (32, 1024):
            assert lib.lcgp_condition_vr_scratch_bytes(dtype, 4096, 8, m, 2000, 2000, C.byref(nb)) == 0
            assert nb.value == vr_bytes(esz, 4096, 8, m, 2000, 2000)
            assert lib.lcgp_condition_select_scratch_bytes(dtype, 4096, 6, 8, m, 2000, 2000, 32, C.byref(nb)) == 0
            assert nb.value == select_bytes(esz, 4096, 6, 8, m, 2000, 2000, 32)
        # the same formulas with no view columns are the fitted model's sizes: the layout is one
        assert lib.lcgp_variance_reduction_scratch_bytes(dtype, 4096, 8, 2000, 2000, C.byref(nb)) == 0
        assert nb.value == vr_bytes(esz, 4096, 8, 0, 2000, 2000)
        assert lib.lcgp_select_scratch_bytes(dtype, 4096, 6, 8, 2000, 2000, 32, C.byref(nb)) == 0
        assert nb.value == select_bytes(esz, 4096, 6, 8, 0, 2000, 2000, 32)
    # a scratch sized for n_cand serves calls with fewer candidates; odd sizes
    for args in ((333, 3, 1, 1, 1), (333, 3, 70, 130, 130), (333, 3, 150, 130, 2100), (4096, 8, 256, 5000, 2048)):
        assert lib.lcgp_condition_vr_scratch_bytes(0, *args, C.byref(nb)) == 0
        assert nb.value == vr_bytes(8, *args)
    for args, msg in (((0, 4096, 8, 0, 10, 10), b'm < 1'), ((0, 4096, 8, 5, 0, 10), b'n_ref'), ((0, 4096, 8, 5, 10, 0), b'n_cand'),
                      ((2, 4096, 8, 5, 10, 10), b'dtype'), ((0, 0, 8, 5, 10, 10), b'n < 1'), ((0, 4096, 65536, 5, 10, 10), b'q_local')):
        assert lib.lcgp_condition_vr_scratch_bytes(*args, C.byref(nb)) < 0
        assert msg in lib.lcgp_last_error(), (args, lib.lcgp_last_error())
    assert lib.lcgp_condition_vr_scratch_bytes(0, 4096, 8, 5, 10, 10, None) < 0
    for args, msg in (((0, 4096, 6, 8, 0, 10, 10, 2), b'm < 1'), ((0, 4096, 6, 8, 5, 0, 10, 2), b'n_ref'),
                      ((0, 4096, 6, 8, 5, 10, 10, 11), b'size'), ((0, 4096, 6, 8, 5, 10, 10, 0), b'size'),
                      ((0, 4096, 127, 8, 5, 10, 10, 2), b'd must be'), ((0, 4096, 6, 65536, 5, 10, 10, 2), b'q_local')):
        assert lib.lcgp_condition_select_scratch_bytes(*args, C.byref(nb)) < 0
        assert msg in lib.lcgp_last_error(), (args, lib.lcgp_last_error())
    assert lib.lcgp_condition_select_scratch_bytes(0, 4096, 6, 8, 5, 10, 10, 2, None) < 0


def test_c_abi_argument_checks():
    """every call below is refused on the host before anything is enqueued: the pointers are never dereferenced"""
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    dummy = C.c_void_p(16)
    big = 1 << 40
    nb = C.c_size_t(0)

    def need_vr(nc):
        assert lib.lcgp_condition_vr_scratch_bytes(0, 50, 2, 4, 10, nc, C.byref(nb)) == 0
        return nb.value
    assert lib.lcgp_condition_select_scratch_bytes(0, 50, 2, 2, 4, 10, 6, 3, C.byref(nb)) == 0
    need_sel = nb.value

    def prep(dtype=0, kern=0, n=50, d=2, q=2, m=4, nr=10, x=dummy, theta=dummy, ws=dummy, state=dummy, xn=dummy, xr=dummy,
             scratch=dummy, nsc=big):
        return lib.lcgp_condition_vr_prepare(None, dtype, kern, n, d, 3, q, x, None, theta, ws, state, m, xn, nr, xr, scratch, nsc)

    def vr(dtype=0, kern=0, n=50, d=2, q=2, m=4, nr=10, nc=4, x=dummy, theta=dummy, ws=dummy, state=dummy, xn=dummy, xr=dummy,
           w=dummy, xc=dummy, mh=None, md=None, row0=-1, r=1, scratch=dummy, nsc=big, out=dummy, stride=0):
        return lib.lcgp_condition_vr(None, dtype, kern, n, d, 3, q, x, None, theta, ws, state, m, xn, nr, xr, w, nc, xc, mh, md, row0,
                                     r, scratch, nsc, out, stride)

    def begin(dtype=0, kern=0, n=50, d=2, q=2, m=4, nr=10, nc=6, size=3, x=dummy, theta=dummy, ws=dummy, state=dummy, xn=dummy,
              xr=dummy, w=dummy, xc=dummy, mh=None, md=None, r=1, rows=2048, scratch=dummy, nsc=big):
        return lib.lcgp_condition_select_begin(None, dtype, kern, n, d, 3, q, x, None, theta, ws, state, m, xn, nr, xr, w, nc, xc,
                                               mh, md, r, size, rows, scratch, nsc)

    def score(dtype=0, n=50, d=2, q=2, m=4, nr=10, nc=6, size=3, step=0, omega=dummy, scratch=dummy, nsc=big):
        return lib.lcgp_condition_select_score(None, dtype, n, d, q, m, nr, nc, size, step, omega, scratch, nsc, None)

    def cond(dtype=0, kern=0, n=50, d=2, q=2, m=4, nr=10, nc=6, size=3, r=1, step=0, theta=dummy, pick=dummy, scratch=dummy, nsc=big):
        return lib.lcgp_condition_select_condition(None, dtype, kern, n, d, 3, q, theta, m, nr, nc, size, r, step, pick, scratch, nsc)

    def state(dtype=0, n=50, d=2, q=2, m=4, nr=10, nc=6, size=3, which=0, scratch=dummy, nsc=big, out=dummy):
        return lib.lcgp_condition_select_state(None, dtype, n, d, q, m, nr, nc, size, which, scratch, nsc, out)

    picks = C.c_void_p(0)

    def pk(dtype=0, n=50, d=2, q=2, m=4, nr=10, nc=6, size=3, scratch=dummy, nsc=big, out=C.byref(picks)):
        return lib.lcgp_condition_select_picks(dtype, n, d, q, m, nr, nc, size, scratch, nsc, out)

    def match(vals):
        a = np.ascontiguousarray(np.asarray(vals, np.int32))
        return a, C.c_void_p(a.ctypes.data)

    def refused(fn, cases):
        for kw, msg in cases:
            assert fn(**kw) == -1, (fn.__name__, kw)
            assert msg.encode() in lib.lcgp_last_error(), (fn.__name__, kw, lib.lcgp_last_error())

    common = [(dict(m=0), 'm < 1'), (dict(dtype=2), 'dtype'), (dict(d=0), 'd must be'), (dict(d=127), 'd must be'),
              (dict(n=0), 'n < 1'), (dict(q=0), 'q_local'), (dict(q=65536), 'q_local'), (dict(nr=0), 'n_ref'),
              (dict(scratch=None), 'NULL')]
    ptrs = [(dict(x=None), 'NULL'), (dict(theta=None), 'NULL'), (dict(ws=None), 'NULL'), (dict(state=None), 'NULL'),
            (dict(xn=None), 'NULL'), (dict(xr=None), 'NULL'), (dict(kern=3), 'kernel_id')]
    ok, okp = match([-1, 3, 49, -1])
    refused(prep, common + ptrs + [(dict(nsc=need_vr(1) - 1), 'scratch is smaller'), (dict(nsc=0), 'scratch is smaller')])
    refused(vr, common + ptrs + [(dict(nc=0), 'n_cand'), (dict(r=0), 'r must be'), (dict(row0=-2), 'cand_row0'),
                                 (dict(row0=8, nc=4, xc=None), 'cand_row0 + n_cand'),
                                 (dict(row0=0), 'x_cand and match must be NULL'), (dict(mh=okp, md=None), 'both'),
                                 (dict(xc=None), 'NULL'), (dict(w=None), 'NULL'), (dict(out=None), 'NULL'),
                                 (dict(stride=3), 'out_stride'), (dict(nsc=need_vr(4) - 1), 'scratch is smaller')])
    for vals in ([-1, 3, 50, -1], [-2, 0, 0, 0]):
        bad, bp = match(vals)
        assert vr(mh=bp, md=dummy) == -1 and b'match must be -1 or a training index' in lib.lcgp_last_error()
    sel_common = common + [(dict(nc=0), 'n_cand'), (dict(size=0), 'size'), (dict(size=7), 'size'),
                           (dict(nsc=need_sel - 1), 'scratch is smaller'), (dict(nsc=0), 'scratch is smaller')]
    refused(begin, sel_common + ptrs + [(dict(r=0), 'r must be'), (dict(rows=0), 'pass_rows'), (dict(rows=4096), 'pass_rows'),
                                        (dict(mh=okp, md=None), 'both'), (dict(xc=None), 'NULL'), (dict(w=None), 'NULL')])
    refused(score, sel_common + [(dict(step=-1), 'step'), (dict(step=3), 'step'), (dict(omega=None), 'NULL')])
    refused(cond, sel_common + [(dict(kern=3), 'kernel_id'), (dict(r=0), 'r must be'), (dict(step=3), 'step'),
                                (dict(theta=None), 'NULL'), (dict(pick=None), 'NULL')])
    refused(state, sel_common + [(dict(which=2), 'which'), (dict(out=None), 'NULL')])
    refused(pk, sel_common + [(dict(out=None), 'NULL')])
    assert pk() == 0 and picks.value is not None and 16 < picks.value < 16 + need_sel
