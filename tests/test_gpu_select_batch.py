"""Greedy batch design on the GPU (lcgp_select_begin / lcgp_select_score / lcgp_select_condition) against float64 numpy: a dense
posterior covariance over reference points and candidates from a numpy factorisation of A_k, conditioned by plain rank-one
updates on the picks the GPU made (the oracle REPLAYS the GPU's picks, so near-ties cannot make a case flaky and no case is
left out); a HotPathEngine built on the augmented data; bitwise-equal results on poisoned scratch, for any pass size of begin,
through the step-by-step host loop and on two ranks; float32 against float64 on replayed picks; the headline shape.

Tolerance, float64: the variance reduction's own figure (tests/test_gpu_variance_reduction.py: 1e-10 of the largest latent
variance per component) carried through the score sum_k omega_k R_k, i.e. 1e-10 * max gvar * sum_k omega_k absolute, for every
step's row.  Every test prints the worst error it saw relative to that bound before it asserts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lcgp_amd import LCGP, synth
from lcgp_amd import engine as engine_mod
from lcgp_amd.engine import HotPathEngine
from oracle import lcgp_oracle as orc
from tests.test_gpu_variance_reduction import _free_port, _match, _model, _points, _state
from tests.test_select_batch_host import DenseState, omega_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL64 = 1e-10           # of max gvar * sum omega
TOL32 = 2e-3            # the float32 figure of test_gpu_variance_reduction.test_float32_against_float64


def _args(m, xc, xr, w, r):
    xc_s = m._standardise_x0(xc)[0]
    xr_s = xc_s if xr is None else m._standardise_x0(xr)[0]
    wn = np.full(len(xr_s), 1.0 / len(xr_s)) if w is None else np.asarray(w, float) / np.sum(w)
    match = _match(m, xc_s) if m.submethod == 'rep' else None
    return xr_s, xc_s, wn, match


def _unit(m, xr_s, om):
    """the scale of the tolerance: the largest latent variance over the reference points times sum_k omega_k"""
    gv = m._ensure_aux().predict_block(xr_s)[1].cpu().numpy()
    return gv.max() * np.sum(om)


def _score(om, R, picked):
    s = np.zeros(R.shape[1])
    for k in range(len(om)):
        s = s + om[k] * R[k]
    s[list(picked)] = -np.inf
    return s


def oracle_rows(m, xr_s, xc_s, wn, match, r, idx, om):
    """(len(idx), n_cand): the dense numpy oracle's score rows, row t conditioned on idx[:t]"""
    th, x, s = _state(m)
    d = x.shape[1]
    states = []
    for k in range(th.shape[0]):
        ell, scale, nug, D = th[k, :d], th[k, d], th[k, d + 1], th[k, d + 2]
        A = np.eye(len(x)) + D * orc.matern32(x, x, ell, scale, nug, kernel=m.kernel) * np.outer(s, s)
        states.append(DenseState(th[k], np.linalg.cholesky(A), x, s, m.kernel, xr_s, xc_s, wn, match, r))
    out = np.empty((len(idx), len(xc_s)))
    for t in range(len(idx)):
        out[t] = _score(om, np.array([st.rows() for st in states]), idx[:t])
        for st in states:
            st.condition(int(idx[t]))
    return out


def check_against_oracle(m, xc, size, xr=None, w=None, r=1, tag=''):
    idx, gain, scores = (t.numpy() for t in m.select_batch(xc, size, x_ref=xr, weights=w, replicates=r, return_scores=True))
    xr_s, xc_s, wn, match = _args(m, xc, xr, w, r)
    om = omega_of(m)
    unit = _unit(m, xr_s, om)
    ref = oracle_rows(m, xr_s, xc_s, wn, match, r, idx, om)
    assert len(set(idx.tolist())) == size
    worst = 0.0
    for t in range(size):
        live = np.setdiff1d(np.arange(len(xc)), idx[:t])
        assert np.all(np.isneginf(scores[t, idx[:t]])) and np.all(np.isfinite(scores[t, live]))
        worst = max(worst, np.max(np.abs(scores[t, live] - ref[t, live])) / unit)
        assert idx[t] == int(np.argmax(scores[t])) and gain[t] == scores[t, idx[t]]       # np.argmax: the lowest index on ties
    print('select_batch %s: worst error over %d steps = %.3e of max gvar * sum omega (bound %.1e)' % (tag, size, worst, TOL64))
    assert worst <= TOL64, (tag, worst)
    for t in range(size):
        assert ref[t, idx[t]] >= np.max(ref[t]) - TOL64 * unit, (tag, t)
    assert np.all(np.diff(gain) <= TOL64 * unit), (tag, gain)
    return idx, gain, scores


@pytest.mark.parametrize('mode,kernel,d,n', [('full', 'matern32', 2, 480), ('rep', 'matern32', 2, 480), ('full', 'se', 6, 480),
                                             ('rep', 'se', 6, 480), ('full', 'matern32', 40, 360), ('full', 'matern32', 1, 333),
                                             ('rep', 'matern32', 6, 471)])
def test_every_step_matches_the_dense_oracle_on_replayed_picks(mode, kernel, d, n):
    m, x = _model(mode, kernel, d=d, n=n)
    xc = _points(x, 150, 1)
    if mode == 'rep':
        xc = np.vstack([xc[:70], m.x_unique.numpy()[[0, 7, 33]], xc[70:]])
    xr = _points(x, 230, 2)
    w = np.random.default_rng(3).random(len(xr))
    for r in ((1, 3) if mode == 'rep' else (1,)):
        check_against_oracle(m, xc, 12, None, None, r, '%s %s d=%d n=%d r=%d shared' % (mode, kernel, d, n, r))
        check_against_oracle(m, xc, 12, xr, w, r, '%s %s d=%d n=%d r=%d' % (mode, kernel, d, n, r))


def test_size_edges():
    m, x = _model('full')
    xc = _points(x, 9, 4)
    idx, _, _ = check_against_oracle(m, xc, 9, _points(x, 50, 5), None, 1, 'size = n_cand')
    assert sorted(idx.tolist()) == list(range(9))
    idx, gain, _ = check_against_oracle(m, xc[:1], 1, None, None, 1, 'n_cand = 1')
    assert idx.tolist() == [0]


def _host_loop(m, xc, size, xr, w, r, picks=None):
    """the step-by-step route (select_begin / select_rows / select_condition, a host synchronisation per step): score rows for
    its own argmax picks, or for the given ones"""
    xc_s, xr_s, wn, _, r, match = m._vr_arguments(xc, xr, w, None, r)
    eng, om = m._ensure_aux(), omega_of(m)
    eng.select_begin(xc_s, xr_s, wn, match, r, size)
    idx, rows = [], np.empty((size, len(xc)))
    for t in range(size):
        rows[t] = _score(om, eng.select_rows().cpu().numpy(), idx)
        idx.append(int(np.argmax(rows[t])) if picks is None else int(picks[t]))
        if t + 1 < size:
            eng.select_condition(idx[-1])
    return np.array(idx), rows


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_bitwise_step0_poisoned_scratch_pass_sizes_and_host_loop(mode, monkeypatch):
    m, x = _model(mode)
    xc = _points(x, 300, 8)
    if mode == 'rep':
        xc = np.vstack([xc[:100], m.x_unique.numpy()[:40], xc[100:]])
    xr = _points(x, 200, 9)
    r = 2 if mode == 'rep' else 1
    om = omega_of(m)
    for ref in (None, xr):
        base = [t.numpy() for t in m.select_batch(xc, 10, x_ref=ref, replicates=r, return_scores=True)]
        R0 = m.variance_reduction(xc, x_ref=ref, replicates=r, latent=True).numpy()
        assert np.array_equal(base[2][0], _score(om, R0, []))
        eng = m._ensure_aux()

        def same(tag):
            got = [t.numpy() for t in m.select_batch(xc, 10, x_ref=ref, replicates=r, return_scores=True)]
            for a, b in zip(got, base):
                assert np.array_equal(a, b), tag

        for v in (0x00, 0xFF, 0x5A):
            eng._scratch.fill_(v)
            same(v)
        for chunk in (37, 128, 2048):
            monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', chunk)
            eng._scratch.fill_(0x5A)
            same(chunk)
        monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', 2048)
        eng._scratch.fill_(0xFF)
        idx, rows = _host_loop(m, xc, 10, ref, None, r)
        assert np.array_equal(idx, base[0]) and np.array_equal(rows, base[2])


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_last_row_equals_the_variance_reduction_of_an_engine_on_the_augmented_data(mode):
    m, x = _model(mode, 'matern32' if mode == 'rep' else 'se', d=2 if mode == 'rep' else 6)
    th, xt, s = _state(m)
    xc = _points(x, 60, 13)
    if mode == 'rep':
        xc = np.vstack([m.x_unique.numpy()[[3, 50]], xc])
    xr = _points(x, 100, 14)
    r = 3 if mode == 'rep' else 1
    size = 6
    idx, gain, scores = (t.numpy() for t in m.select_batch(xc, size, x_ref=xr, replicates=r, return_scores=True))
    xr_s, xc_s, wn, match = _args(m, xc, xr, None, r)
    om = omega_of(m)
    unit = _unit(m, xr_s, om)
    x2, r2 = xt, s * s
    for j in idx[:size - 1]:
        hit = np.flatnonzero(np.all(x2 == xc_s[j][None, :], axis=1)) if mode == 'rep' else []
        if len(hit):
            r2 = r2.copy()
            r2[hit[0]] += r
        else:
            x2, r2 = np.vstack([x2, xc_s[j]]), np.r_[r2, r]
    aug = HotPathEngine(x2, np.zeros((int(m.p), len(x2))), np.sqrt(r2) if mode == 'rep' else None, q_local=th.shape[0],
                        kernel=m.kernel)
    aug.evaluate(th)
    live = np.setdiff1d(np.arange(len(xc)), idx[:size - 1])
    m2 = None if mode != 'rep' else np.array([int(np.flatnonzero(np.all(x2 == c[None, :], axis=1))[0])
                                              if np.any(np.all(x2 == c[None, :], axis=1)) else -1 for c in xc_s[live]])
    R = aug.variance_reduction_block(xc_s[live], xr_s, wn, m2, r).cpu().numpy()
    err = np.max(np.abs(_score(om, R, []) - scores[-1, live])) / unit
    print('select_batch %s: last row against the engine on the augmented data: %.3e (bound %.1e)' % (mode, err, TOL64))
    assert err <= TOL64


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_float32_against_float64_on_replayed_picks(mode):
    m64, x = _model(mode)
    m32, _ = _model(mode, dtype='float32')
    xc = _points(x, 200, 10)
    xr = _points(x, 150, 11)
    idx, _, s64 = (t.numpy() for t in m64.select_batch(xc, 12, x_ref=xr, return_scores=True))
    _, s32 = _host_loop(m32, xc, 12, xr, None, 1, picks=idx)
    om = omega_of(m64)
    unit = _unit(m64, m64._standardise_x0(xr)[0], om)
    worst = 0.0
    for t in range(12):
        live = np.setdiff1d(np.arange(len(xc)), idx[:t])
        assert np.all(np.isfinite(s32[t, live]))
        worst = max(worst, np.max(np.abs(s32[t, live] - s64[t, live])) / unit)
    print('select_batch %s float32: worst error over 12 steps = %.3e (bound %.1e)' % (mode, worst, TOL32))
    assert worst <= TOL32
    i32, g32 = m32.select_batch(xc, 12, x_ref=xr)
    assert len(set(i32.tolist())) == 12 and np.all(np.isfinite(g32.numpy()))


def test_two_ranks_reproduce_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_select_gpu_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


def test_headline_shape_runs_and_leaves_the_model_unchanged():
    x, y = synth.make_full(93, 4096, 6, 64, 8)
    m = LCGP(y=y, x=x, q=8, device='cuda:0')
    o = orc.OracleLCGP(y=y, x=x, q=8)
    m._set_flat(synth.param_points(93, o.get_unconstrained())[1])
    xn = np.asarray(x)
    xc = _points(xn, 2000, 12)
    before = [t.numpy().copy() for t in m.predict(xn[:50] + 0.01)]
    ghat, gvar = m.ghat, m.gvar
    eng = m._ensure_aux()
    th = eng._theta_last.copy()
    idx, gain, scores = (t.numpy() for t in m.select_batch(xc, 32, return_scores=True))
    assert idx.shape == (32,) and len(set(idx.tolist())) == 32 and np.all(np.isfinite(gain))
    assert np.all(np.isfinite(scores[~np.isneginf(scores)])) and np.sum(np.isneginf(scores)) == 31 * 32 // 2
    unit = _unit(m, m._standardise_x0(xc)[0], omega_of(m))
    assert np.all(np.diff(gain) <= TOL64 * unit)
    assert m.ghat is ghat and m.gvar is gvar and m._ensure_aux() is eng and np.array_equal(eng._theta_last, th)
    after = [t.numpy() for t in m.predict(xn[:50] + 0.01)]
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
