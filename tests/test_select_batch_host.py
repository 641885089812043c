"""CPU tests of the greedy batch design (LCGP.select_batch): the host layer -- argument checks, omega from the output map, the
loop over steps, the gather over ranks -- through a numpy stand-in of HotPathEngine.select_* that conditions the DENSE posterior
covariance over reference points and candidates pick by pick with plain rank-one updates, checked against brute force (augment
the training set with the picked rows, refactor, recompute the variance drop of every remaining candidate), the lazy recursion
of include/lcgp_hip.h in numpy against the dense one, and the argument checks and scratch size of the new C entries
(tests/test_gpu_select_batch.py runs the same through liblcgp_hip.so)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from tests.test_variance_reduction_host import (VrOracleEngine, _cands, _free_port, _kern, _model, _std, gvar_at, patch_vr)

HERE = os.path.dirname(os.path.abspath(__file__))


def parts(th, low, x, s, kernel, xr, xc, match):
    """coff, D, scale, U_ref, U_cand of one component as include/lcgp_hip.h defines them"""
    d = x.shape[1]
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    nt = nug / (1.0 + nug)
    coff = scale * (1 - nt)
    cc = coff * _kern(xc, x, ell, kernel)
    if match is not None:
        for j, m in enumerate(match):
            if m >= 0:
                cc[j, m] += scale * nt
    uc = sla.solve_triangular(low, (cc * s[None, :]).T, lower=True).T
    ur = sla.solve_triangular(low, (coff * _kern(xr, x, ell, kernel) * s[None, :]).T, lower=True).T
    return ell, coff, D, scale, ur, uc


class DenseState:
    """the posterior covariance Sigma(ref, cand) and Sigma(cand, cand) (diagonal: the candidates' own gvar) of one component,
    conditioned by rank-one updates of the dense matrices"""

    def __init__(self, th, low, x, s, kernel, xr, xc, w, match, r):
        ell, coff, D, scale, ur, uc = parts(th, low, x, s, kernel, xr, xc, match)
        self.src = coff * _kern(xr, xc, ell, kernel) - D * ur @ uc.T
        self.scc = coff * _kern(xc, xc, ell, kernel) - D * uc @ uc.T
        np.fill_diagonal(self.scc, scale - D * np.sum(uc * uc, axis=1))
        self.w, self.tau = np.asarray(w, np.float64), 1.0 / (D * r)

    def rows(self):
        return (self.w @ (self.src * self.src)) / (np.maximum(np.diag(self.scc), 0.0) + self.tau)

    def condition(self, j):
        den = max(self.scc[j, j], 0.0) + self.tau
        pc, sc = self.scc[:, j].copy(), self.src[:, j].copy()
        self.src -= np.outer(sc, pc) / den
        self.scc -= np.outer(pc, pc) / den


def lazy_rows(th, low, x, s, kernel, xr, xc, w, match, r, picks):
    """R after each of `picks` by the lazy recursion of include/lcgp_hip.h (what the kernels do), one component"""
    ell, coff, D, scale, ur, uc = parts(th, low, x, s, kernel, xr, xc, match)
    tau = 1.0 / (D * r)
    h = scale - D * np.sum(uc * uc, axis=1)
    N = w @ (coff * _kern(xr, xc, ell, kernel) - D * ur @ uc.T) ** 2
    V, Uh, out = [], [], [N / (np.maximum(h, 0) + tau)]
    for j in picks:
        pcol = coff * _kern(xc, xc[j:j + 1], ell, kernel)[:, 0] - D * uc @ uc[j] - sum(v * v[j] for v in V)
        scol = coff * _kern(xr, xc[j:j + 1], ell, kernel)[:, 0] - D * ur @ uc[j] - sum(u * v[j] for u, v in zip(Uh, V))
        den = max(h[j], 0) + tau
        v, u = pcol / np.sqrt(den), scol / np.sqrt(den)
        wu = w * u
        g = coff * _kern(xc, xr, ell, kernel) @ wu - D * uc @ (ur.T @ wu) - sum(vs * (us @ wu) for us, vs in zip(Uh, V))
        N = np.maximum(N - 2 * v * g + v * v * (u @ wu), 0)
        h = h - v * v
        V.append(v)
        Uh.append(u)
        out.append(N / (np.maximum(h, 0) + tau))
    return np.array(out)


class SelectOracleEngine(VrOracleEngine):
    """VrOracleEngine plus the select_* interface of HotPathEngine on dense numpy matrices"""

    def select_begin(self, x_cand_s, x_ref_s, w, match, r, size):
        xr = x_cand_s if x_ref_s is None else x_ref_s
        s = np.ones(self.n) if self.sr is None else self.sr
        self._sel = [DenseState(th, low, self.x, s, self.kernel, np.asarray(xr), np.asarray(x_cand_s), w, match, r)
                     for th, low, _, _ in self._state]

    def select_rows(self):
        return torch.as_tensor(np.array([st.rows() for st in self._sel]))

    def select_condition(self, j):
        for st in self._sel:
            st.condition(j)

    def select_batch_block(self, x_cand_s, x_ref_s, w, match, r, size, omega):
        self.select_begin(x_cand_s, x_ref_s, w, match, r, size)
        n_cand = len(x_cand_s)
        idx, scores, picked = np.zeros(size, np.int32), np.empty((size, n_cand)), np.zeros(n_cand, bool)
        for t in range(size):
            R = self.select_rows().numpy()
            sc = np.zeros(n_cand)
            for k in range(len(omega)):
                sc = sc + omega[k] * R[k]
            sc[picked] = -np.inf
            idx[t], scores[t] = np.argmax(sc), sc
            picked[idx[t]] = True
            if t + 1 < size:
                self.select_condition(int(idx[t]))
        return torch.as_tensor(idx), torch.as_tensor(scores)


def patch_select(m, engine_cls=SelectOracleEngine):
    patch_vr(m, engine_cls)
    m._engine = None
    m._u_last = None
    return m


def _sel_model(mode, **kw):
    m, x = _model(mode, **kw)
    return patch_select(m), x


def omega_of(m, outputs=None):
    W, _, scale, _ = m._output_map()
    outputs = list(range(int(m.p))) if outputs is None else outputs
    return np.mean((W[:, outputs] ** 2) * (scale[outputs] ** 2)[None, :], axis=1)


def brute_after_picks(m, xr_s, xc_s, w, r, picks):
    """(q, n_cand): the variance drop of every candidate for the model whose training set was augmented by r runs at each of
    `picks` (refactorised, same theta)"""
    eng = m._aux_engine
    rep = m.submethod == 'rep'
    x = eng.x
    rr = np.asarray(m.r.numpy(), np.float64) if rep else np.ones(len(x))

    def add(x, rr, c):
        hit = np.flatnonzero(np.all(x == c[None, :], axis=1)) if rep else []
        if len(hit):
            r2 = rr.copy()
            r2[hit[0]] += r
            return x, r2
        return np.vstack([x, c]), np.r_[rr, r]

    for j in picks:
        x, rr = add(x, rr, xc_s[j])
    out = np.zeros((len(eng._state), len(xc_s)))
    for i, (th, _, _, _) in enumerate(eng._state):
        before = w @ gvar_at(th, x, np.sqrt(rr), eng.kernel, xr_s)
        for j, c in enumerate(xc_s):
            if j in picks:
                continue
            x2, r2 = add(x, rr, c)
            out[i, j] = before - w @ gvar_at(th, x2, np.sqrt(r2), eng.kernel, xr_s)
    return out


CASES = [('full', {}), ('rep', {}), ('full', {'kernel': 'se'}), ('rep', {'kernel': 'se'})]


@pytest.mark.parametrize('mode,kw', CASES)
@pytest.mark.parametrize('explicit_ref', [False, True])
def test_every_step_equals_brute_force_on_the_augmented_training_set(mode, kw, explicit_ref):
    m, x = _sel_model(mode, **kw)
    rng = np.random.default_rng(15)
    xc = _cands(m, x, rng, 7)           # rep: two training inputs among them (matched candidates)
    xr = (x.min(axis=0) + (x.max(axis=0) - x.min(axis=0)) * rng.random((9, x.shape[1]))) if explicit_ref else None
    w = rng.random(9) + 0.1 if explicit_ref else None
    ww = np.full(len(xc), 1.0 / len(xc)) if w is None else w / w.sum()
    om = omega_of(m)
    size = 5
    for r in ((1, 3) if mode == 'rep' else (1,)):
        idx, gain, scores = (t.numpy() for t in m.select_batch(xc, size, x_ref=xr, weights=w, replicates=r, return_scores=True))
        assert idx.dtype == np.int64 and idx.shape == (size,) and gain.shape == (size,) and scores.shape == (size, len(xc))
        assert len(set(idx)) == size
        # step 0 is variance_reduction combined with omega
        R0 = m.variance_reduction(xc, x_ref=xr, weights=w, replicates=r, latent=True).numpy()
        np.testing.assert_allclose(scores[0], om @ R0, rtol=1e-12)
        for t in range(size):
            ref = om @ brute_after_picks(m, _std(m, xc if xr is None else xr), _std(m, xc), ww, r, list(idx[:t]))
            live = np.setdiff1d(np.arange(len(xc)), idx[:t])
            assert np.all(np.isneginf(scores[t, idx[:t]]))
            np.testing.assert_allclose(scores[t, live], ref[live], rtol=1e-7, atol=1e-11 * np.max(ref))
            assert idx[t] == np.argmax(scores[t]) and gain[t] == scores[t, idx[t]]
        assert np.all(np.diff(gain) <= 1e-12 * gain[0])


@pytest.mark.parametrize('mode,kw', CASES)
def test_lazy_recursion_equals_dense_rank_one_updates(mode, kw):
    m, x = _sel_model(mode, **kw)
    rng = np.random.default_rng(16)
    xc_s = _std(m, _cands(m, x, rng, 8))
    xr_s = _std(m, x.min(axis=0) + (x.max(axis=0) - x.min(axis=0)) * rng.random((11, x.shape[1])))
    w = rng.random(11)
    w /= w.sum()
    m.variance_reduction(_cands(m, x, rng, 2))       # (builds the engine)
    eng = m._aux_engine
    s = np.ones(eng.n) if eng.sr is None else eng.sr
    match = None
    if mode == 'rep':
        match = np.array([next((i for i in range(eng.n) if np.array_equal(eng.x[i], c)), -1) for c in xc_s], np.int32)
        assert np.sum(match >= 0) == 2
    r = 2 if mode == 'rep' else 1
    picks = [5, 0, 3, 7]
    for th, low, _, _ in eng._state:
        dense = DenseState(th, low, eng.x, s, eng.kernel, xr_s, xc_s, w, match, r)
        lazy = lazy_rows(th, low, eng.x, s, eng.kernel, xr_s, xc_s, w, match, r, picks)
        for t in range(len(picks) + 1):
            live = np.setdiff1d(np.arange(len(xc_s)), picks[:t])
            np.testing.assert_allclose(lazy[t][live], dense.rows()[live], rtol=1e-9, atol=1e-14 * np.max(lazy[0]))
            if t < len(picks):
                dense.condition(picks[t])


def test_output_subset_and_weights_change_omega_and_scores():
    m, x = _sel_model('full')
    xc = _cands(m, x, np.random.default_rng(17), 7)
    w = np.r_[5.0, np.ones(6)]
    for outputs in (None, [2, 0], [1]):
        idx, gain, scores = (t.numpy() for t in m.select_batch(xc, 3, weights=w, outputs=outputs, return_scores=True))
        R0 = m.variance_reduction(xc, weights=w, latent=True).numpy()
        np.testing.assert_allclose(scores[0], omega_of(m, outputs) @ R0, rtol=1e-12)
        d0 = m.variance_reduction(xc, weights=w, outputs=outputs).numpy()
        np.testing.assert_allclose(scores[0], d0.mean(axis=0), rtol=1e-12)
    two = m.select_batch(xc, 3)
    assert len(two) == 2 and two[0].dtype == torch.int64 and two[1].dtype == torch.float64


def test_size_limits_and_model_left_unchanged():
    m, x = _sel_model('full')
    xc = _cands(m, x, np.random.default_rng(18), 6)
    m.predict(xc[:2])
    ghat, gvar = m.ghat, m.gvar
    idx, gain = m.select_batch(xc, len(xc))
    assert sorted(idx.tolist()) == list(range(len(xc)))
    assert m.ghat is ghat and m.gvar is gvar
    i1, g1 = m.select_batch(xc[:1], 1)
    assert i1.tolist() == [0] and np.isfinite(g1.numpy()).all()


def test_argument_errors():
    m, x = _sel_model('full')
    xc = x[:4] + 0.01
    for kw, msg in (({'size': 0}, 'size'), ({'size': 5}, 'size'), ({'size': 1.5}, 'size'), ({'size': True}, 'size'),
                    ({'x_cand': np.vstack([xc, xc[1:2]])}, 'duplicate'),
                    ({'x_cand': np.zeros((3, 3))}, 'x_cand'),
                    ({'x_ref': np.zeros((3, 1))}, 'x_ref'),
                    ({'weights': [1, 2, 3]}, 'length'),
                    ({'weights': [1, -1, 1, 1]}, 'non-negative'),
                    ({'weights': [1, np.nan, 1, 1]}, 'finite'),
                    ({'weights': [0, 0, 0, 0]}, 'all be zero'),
                    ({'outputs': [3]}, 'outputs'),
                    ({'replicates': 0}, 'replicates'),
                    ({'replicates': 2}, 'full path')):
        args = dict(x_cand=xc, size=2)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            m.select_batch(**args)
    mr, _ = _sel_model('rep')
    idx, _ = mr.select_batch(mr.x_unique.numpy()[:3], 2, replicates=2)
    assert len(set(idx.tolist())) == 2


def test_two_ranks_pick_what_one_rank_picks():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_select_host_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


def test_c_abi_argument_checks_and_scratch_size():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() >= 560
    nb = C.c_size_t(0)

    def sb(n, q, nr, nc, size, dtype=0, d=6):
        assert lib.lcgp_select_scratch_bytes(dtype, n, d, q, nr, nc, size, C.byref(nb)) == 0, lib.lcgp_last_error()
        return nb.value

    # all candidates resident: at least the two U; linear in size (the history); no n_ref x n_cand or n_cand x n_cand matrix
    base = sb(4096, 8, 2000, 2000, 32)
    assert base >= 8 * 8 * (2000 + 2000) * 4096
    a, b, c = sb(4096, 8, 2000, 2000, 16), base, sb(4096, 8, 2000, 2000, 48)
    assert b > a and abs((c - b) - (b - a)) <= 4096
    big = sb(4096, 8, 20000, 20000, 32)
    assert big < 8 * 8 * (20000 + 20000) * 4096 * 1.2 and big < 0.5 * 8 * 8 * 20000 * 20000
    assert sb(4096, 8, 2000, 2000, 32, 1) < base
    for kw, msg in ((dict(nr=0), b'n_ref'), (dict(nc=0), b'n_cand'), (dict(size=0), b'size'), (dict(size=11), b'size'),
                    (dict(d=0), b'd must be'), (dict(dtype=2), b'dtype')):
        a_ = dict(dtype=0, n=100, d=3, q=2, nr=10, nc=10, size=4)
        a_.update(kw)
        assert lib.lcgp_select_scratch_bytes(a_['dtype'], a_['n'], a_['d'], a_['q'], a_['nr'], a_['nc'], a_['size'], C.byref(nb)) < 0
        assert msg in lib.lcgp_last_error(), (kw, lib.lcgp_last_error())
    assert lib.lcgp_select_scratch_bytes(0, 100, 3, 2, 10, 10, 4, None) < 0

    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything

    def begin(n=50, d=2, nr=10, nc=4, size=2, mh=None, md=None, r=1, xc=dummy, w=dummy, rows=2048, dtype=0):
        return lib.lcgp_select_begin(None, dtype, 0, n, d, 3, 2, dummy, None, dummy, dummy, nr, dummy, w, nc, xc, mh, md, r, size,
                                     rows, dummy)

    ok = np.ascontiguousarray(np.array([-1, 3, 49, -1], np.int32))
    okp = C.c_void_p(ok.ctypes.data)
    for kw, msg in ((dict(nr=0), 'n_ref'), (dict(nc=0), 'n_cand'), (dict(size=0), 'size'), (dict(size=5), 'size'),
                    (dict(r=0), 'r must be'), (dict(d=127), 'd must be'), (dict(dtype=2), 'dtype'), (dict(rows=0), 'pass_rows'),
                    (dict(rows=4096), 'pass_rows'), (dict(mh=okp, md=None), 'both'), (dict(xc=None), 'NULL'), (dict(w=None), 'NULL')):
        assert begin(**kw) < 0, kw
        assert msg.encode() in lib.lcgp_last_error(), (kw, lib.lcgp_last_error())
    bad = np.ascontiguousarray(np.array([-1, 3, 50, -1], np.int32))
    assert begin(mh=C.c_void_p(bad.ctypes.data), md=dummy) < 0
    assert b'match must be -1 or a training index' in lib.lcgp_last_error()

    def cond(step=0, size=2, pick=dummy, r=1, nc=4):
        return lib.lcgp_select_condition(None, 0, 0, 50, 2, 3, 2, dummy, 10, nc, size, r, step, pick, dummy)

    for kw, msg in ((dict(step=-1), 'step'), (dict(step=2), 'step'), (dict(pick=None), 'NULL'), (dict(r=0), 'r must be'),
                    (dict(size=9), 'size')):
        assert cond(**kw) < 0, kw
        assert msg.encode() in lib.lcgp_last_error(), (kw, lib.lcgp_last_error())
    assert lib.lcgp_select_score(None, 0, 50, 2, 2, 10, 4, 2, 2, dummy, dummy, None) < 0
    assert b'step' in lib.lcgp_last_error()
    assert lib.lcgp_select_score(None, 0, 50, 2, 2, 10, 4, 2, 0, None, dummy, None) < 0
    assert b'NULL' in lib.lcgp_last_error()
    assert lib.lcgp_select_state(None, 0, 50, 2, 2, 10, 4, 2, 2, dummy, dummy) < 0
    assert b'which' in lib.lcgp_last_error()
