"""CPU tests of the integrated variance reduction (LCGP.variance_reduction): the host layer -- standardisation, rep-path
matching of candidates to training inputs, weights, the output map, the gather over ranks -- through a numpy stand-in of
HotPathEngine.variance_reduction_block written in the closed form of include/lcgp_hip.h, checked against brute force
(augment the training set with the candidate, refactor I + D (C o s s^T), predict at the reference points), and the argument
checks and scratch size of the new C entries (tests/test_gpu_variance_reduction.py runs the same through liblcgp_hip.so)."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from lcgp_amd import LCGP, synth
from oracle import lcgp_oracle as orc
from tests.test_cv_host import _make_factory
from tests.test_joint_host import JointOracleEngine

HERE = os.path.dirname(os.path.abspath(__file__))


def _kern(xa, xb, ell, kernel):
    S = np.abs(xa[:, None, :] / ell - xb[None, :, :] / ell)
    if kernel == 'se':
        return np.exp(-0.5 * np.sum(S * S, axis=2))
    return np.prod(1.0 + S, axis=2) * np.exp(-np.sum(S, axis=2))


def closed_form(th, low, x, s, kernel, xr, xc, w, match, r):
    """R(c) of one component in the closed form of include/lcgp_hip.h"""
    d = x.shape[1]
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    nt = nug / (1.0 + nug)
    cc = scale * (1 - nt) * _kern(xc, x, ell, kernel)
    if match is not None:
        for j, m in enumerate(match):
            if m >= 0:
                cc[j, m] += scale * nt
    uc = sla.solve_triangular(low, (cc * s[None, :]).T, lower=True).T
    ur = sla.solve_triangular(low, (scale * (1 - nt) * _kern(xr, x, ell, kernel) * s[None, :]).T, lower=True).T
    gh = scale - D * np.sum(uc * uc, axis=1)
    sig = scale * (1 - nt) * _kern(xr, xc, ell, kernel) - D * ur @ uc.T
    return (w @ (sig * sig)) / (np.maximum(gh, 0.0) + 1.0 / (D * r))


class VrOracleEngine(JointOracleEngine):
    """OracleEngine plus variance_reduction_block in the closed form of include/lcgp_hip.h, in numpy"""
    dtype_name = 'float64'
    calls = None

    def variance_reduction_block(self, x_cand_s, x_ref_s, w, match, r):
        if self.calls is not None:
            self.calls.append((x_ref_s is None, None if match is None else np.array(match)))
        xr = x_cand_s if x_ref_s is None else x_ref_s
        s = np.ones(self.n) if self.sr is None else self.sr
        out = np.zeros((self.q_local, len(x_cand_s)))
        for i, (th, low, _, _) in enumerate(self._state):
            out[i] = closed_form(th, low, self.x, s, self.kernel, np.asarray(xr), np.asarray(x_cand_s), np.asarray(w), match, r)
        return torch.as_tensor(out)


def patch_vr(model, engine_cls=VrOracleEngine):
    model._make_engine = _make_factory(model, engine_cls)
    return model


def gvar_at(th, x, s, kernel, xt):
    """predict()'s latent variance at new inputs xt of the model with training inputs x and replicate scaling s"""
    d = x.shape[1]
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    nt = nug / (1.0 + nug)
    C0 = scale * ((1 - nt) * _kern(x, x, ell, kernel) + nt * np.eye(len(x)))
    A = np.eye(len(x)) + D * C0 * np.outer(s, s)
    c = scale * (1 - nt) * _kern(xt, x, ell, kernel) * s[None, :]
    return scale - D * np.sum(c * np.linalg.solve(A, c.T).T, axis=1)


def brute_force(m, xr_s, xc_s, w, r):
    """(q, n_cand): the weighted sum of gvar_k over the reference points before minus after adding r runs at each candidate
    to the training set (refactorised, same theta)"""
    eng = m._aux_engine
    rep = m.submethod == 'rep'
    x = eng.x
    rr = np.asarray(m.r.numpy(), np.float64) if rep else np.ones(len(x))
    out = np.zeros((len(eng._state), len(xc_s)))
    for i, (th, _, _, _) in enumerate(eng._state):
        before = w @ gvar_at(th, x, np.sqrt(rr), eng.kernel, xr_s)
        for j, c in enumerate(xc_s):
            hit = np.flatnonzero(np.all(x == c[None, :], axis=1)) if rep else []
            if len(hit):
                r2 = rr.copy()
                r2[hit[0]] += r
                after = gvar_at(th, x, np.sqrt(r2), eng.kernel, xr_s)
            else:
                after = gvar_at(th, np.vstack([x, c]), np.sqrt(np.r_[rr, r]), eng.kernel, xr_s)
            out[i, j] = before - w @ after
    return out


def _model(mode, group=None, q=None, **kw):
    if mode == 'full':
        x, y = synth.make_full(41, 40, 2, 3, 3)
    else:
        x, y = synth.make_rep(42, 40, 3, 2, 4, 4)      # 40 unique inputs, replicated
    extra = {} if q is None else {'q': q}
    m = patch_vr(LCGP(y=y, x=x, submethod=mode, process_group=group, **extra, **kw))
    o = orc.OracleLCGP(y=y, x=x, submethod=mode, **extra)
    m._set_flat(synth.param_points(41, o.get_unconstrained())[1])
    return m, np.asarray(x)


def _std(m, x):
    return m._standardise_x0(x)[0]


def _cands(m, x, rng, k=6):
    """raw-scale candidates: new points, plus (rep path) training inputs given bitwise"""
    lo, hi = x.min(axis=0), x.max(axis=0)
    new = lo + (hi - lo) * rng.random((k, x.shape[1]))
    if m.submethod == 'rep':
        return np.vstack([new[:3], m.x_unique.numpy()[[4, 17]], new[3:]])
    return new


CASES = [('full', {}), ('rep', {}), ('full', {'kernel': 'se'}), ('rep', {'kernel': 'se'})]


@pytest.mark.parametrize('mode,kw', CASES)
@pytest.mark.parametrize('explicit_ref', [False, True])
def test_latent_reduction_equals_brute_force_augmentation(mode, kw, explicit_ref):
    m, x = _model(mode, **kw)
    rng = np.random.default_rng(5)
    xc = _cands(m, x, rng)
    xr = (x.min(axis=0) + (x.max(axis=0) - x.min(axis=0)) * rng.random((9, x.shape[1]))) if explicit_ref else None
    w = rng.random(len(xr if explicit_ref else xc)) + 0.1 if explicit_ref else None
    for r in ((1, 3) if mode == 'rep' else (1,)):
        R = m.variance_reduction(xc, x_ref=xr, weights=w, replicates=r, latent=True).numpy()
        ww = np.full(len(xc), 1.0 / len(xc)) if w is None else w / w.sum()
        ref = brute_force(m, _std(m, xc if xr is None else xr), _std(m, xc), ww, r)
        assert R.shape == (int(m.q), len(xc))
        np.testing.assert_allclose(R, ref, rtol=1e-8, atol=1e-12 * np.max(np.abs(ref)))
    if mode == 'rep':
        # the two training inputs among the candidates were matched, the others not
        eng = m._aux_engine
        eng.calls = []
        m.variance_reduction(xc)
        match = eng.calls[0][1]
        assert list(match) == [-1, -1, -1, 4, 17, -1, -1, -1]


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_output_map_and_output_subset(mode):
    m, x = _model(mode)
    xc = _cands(m, x, np.random.default_rng(6))
    R = m.variance_reduction(xc, latent=True).numpy()
    W, _, scale, _ = m._output_map()
    full = m.variance_reduction(xc).numpy()
    assert full.shape == (int(m.p), len(xc))
    np.testing.assert_allclose(full, (scale ** 2)[:, None] * ((W ** 2).T @ R), rtol=1e-13)
    sub = m.variance_reduction(xc, outputs=[2, 0]).numpy()
    np.testing.assert_array_equal(sub, full[[2, 0]])


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_identities(mode):
    m, x = _model(mode)
    rng = np.random.default_rng(7)
    xc = _cands(m, x, rng)
    xr = x.min(axis=0) + (x.max(axis=0) - x.min(axis=0)) * rng.random((11, x.shape[1]))
    w = rng.random(11)
    w /= w.sum()
    R = m.variance_reduction(xc, x_ref=xr, weights=w, latent=True).numpy()
    assert np.all(R >= 0)
    gv = m._aux_engine.predict(_std(m, xr))[1]
    assert np.all(R <= (gv @ w)[:, None] * (1 + 1e-12))
    # one reference point at the candidate itself: Sigma(c, c)^2 / (Sigma^h(c, c) + 1 / D), where Sigma^h(c, c) is predict()'s
    # gvar at c and the numerator's Sigma(c, c) lacks the nugget (c as a reference point is a new input).  (Candidates that
    # replicate a training input are left out here: predict() has no nugget in their cross row, their own row has it.)
    eng = m._aux_engine
    for j in range(len(xc)):
        if mode == 'rep' and np.any(np.all(eng.x == _std(m, xc[j:j + 1]), axis=1)):
            continue
        one = m.variance_reduction(xc[j:j + 1], x_ref=xc[j:j + 1], latent=True).numpy()[:, 0]
        gh = eng.predict(_std(m, xc[j:j + 1]))[1][:, 0]
        for i, (th, _, _, _) in enumerate(eng._state):
            d = eng.d
            scale, nug, D = th[d], th[d + 1], th[d + 2]
            num = gh[i] - scale * nug / (1 + nug)
            np.testing.assert_allclose(one[i], num * num / (max(gh[i], 0.0) + 1.0 / D), rtol=1e-10)


def test_full_path_equals_the_formula_on_predict_latent_cov_of_the_union():
    m, x = _model('full')
    rng = np.random.default_rng(8)
    xc = _cands(m, x, rng, 5)
    xr = np.vstack([x[:3], x.min(axis=0) + (x.max(axis=0) - x.min(axis=0)) * rng.random((4, x.shape[1]))])
    w = rng.random(len(xr))
    R = m.variance_reduction(xc, x_ref=xr, weights=w, latent=True).numpy()
    cov = m.predict_latent_cov(np.vstack([xr, xc])).numpy()
    nr = len(xr)
    D = np.array([st[0][m._aux_engine.d + 2] for st in m._aux_engine._state])
    sig = cov[:, :nr, nr:]
    den = np.maximum(np.diagonal(cov, axis1=1, axis2=2)[:, nr:], 0.0) + 1.0 / D[:, None]
    ref = np.einsum('t,ktc->kc', w / w.sum(), sig * sig) / den
    np.testing.assert_allclose(R, ref, rtol=1e-9, atol=1e-13)


def test_shared_reference_set_and_no_evaluation_after_predict():
    m, x = _model('full')
    xc = _cands(m, x, np.random.default_rng(9))
    m.predict(xc[:2])
    ghat, gvar = m.ghat, m.gvar
    eng = m._engine
    calls = []
    orig = eng.evaluate
    eng.evaluate = lambda rows: (calls.append(1), orig(rows))[1]
    eng.calls = []
    a = m.variance_reduction(xc).numpy()
    b = m.variance_reduction(xc, x_ref=xc).numpy()
    assert calls == []
    assert eng.calls[0][0] and not eng.calls[1][0]          # default x_ref: the engine is told the sets are one
    np.testing.assert_allclose(a, b, rtol=1e-13)
    assert m.ghat is ghat and m.gvar is gvar


def test_argument_errors():
    m, x = _model('full')
    xc = x[:4] + 0.01
    for kw, msg in (({'x_cand': np.zeros((3, 3))}, 'x_cand'),
                    ({'x_ref': np.zeros((3, 1))}, 'x_ref'),
                    ({'weights': [1, 2, 3]}, 'length'),
                    ({'weights': [1, -1, 1, 1]}, 'non-negative'),
                    ({'weights': [1, np.nan, 1, 1]}, 'finite'),
                    ({'weights': [1, np.inf, 1, 1]}, 'finite'),
                    ({'weights': [0, 0, 0, 0]}, 'all be zero'),
                    ({'outputs': [3]}, 'outputs'),
                    ({'outputs': [-1]}, 'outputs'),
                    ({'replicates': 0}, 'replicates'),
                    ({'replicates': 1.5}, 'replicates'),
                    ({'replicates': 2}, 'full path')):
        args = dict(x_cand=xc)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            m.variance_reduction(**args)
    mr, _ = _model('rep')
    with pytest.raises(ValueError, match='replicates'):
        mr.variance_reduction(mr.x_unique.numpy()[:2], replicates=0)
    assert mr.variance_reduction(mr.x_unique.numpy()[:2], replicates=2).shape == (int(mr.p), 2)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_gather_what_one_rank_computes():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_vr_host_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


def test_c_abi_argument_checks_and_scratch_size():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() >= 550
    nb = C.c_size_t(0)

    def sb(n, q, nr, nc, dtype=0):
        assert lib.lcgp_variance_reduction_scratch_bytes(dtype, n, q, nr, nc, C.byref(nb)) == 0, lib.lcgp_last_error()
        return nb.value

    # linear in n_cand at fixed n_ref (whole X work areas: n_cand multiples of 2048), and the n_ref x n_cand matrix is not formed
    a, b, c = sb(4096, 8, 5000, 2048), sb(4096, 8, 5000, 4096), sb(4096, 8, 5000, 6144)
    assert b > a and abs((c - b) - (b - a)) <= 4096
    big = sb(4096, 8, 20000, 20000)
    assert big < 0.5 * 8 * 8 * 20000 * 20000
    assert sb(4096, 8, 20000, 20000, 1) < big
    assert lib.lcgp_variance_reduction_scratch_bytes(0, 4096, 8, 0, 10, C.byref(nb)) < 0
    assert b'n_ref' in lib.lcgp_last_error()
    assert lib.lcgp_variance_reduction_scratch_bytes(0, 4096, 8, 10, 0, C.byref(nb)) < 0
    assert b'n_cand' in lib.lcgp_last_error()
    assert lib.lcgp_variance_reduction_scratch_bytes(0, 4096, 8, 10, 10, None) < 0

    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything

    def vr(n=50, d=2, nr=10, nc=4, mh=None, md=None, row0=-1, r=1, xc=dummy, out_stride=0, dtype=0, w=dummy):
        return lib.lcgp_variance_reduction(None, dtype, 0, n, d, 3, 2, dummy, None, dummy, dummy, nr, dummy, w, nc, xc, mh, md,
                                           row0, r, dummy, dummy, out_stride)

    def match(vals):
        a = np.ascontiguousarray(np.asarray(vals, np.int32))
        return a, C.c_void_p(a.ctypes.data)

    ok, okp = match([-1, 3, 49, -1])
    cases = [(dict(nr=0), 'n_ref'), (dict(nc=0), 'n_cand'), (dict(r=0), 'r must be'), (dict(d=127), 'd must be'),
             (dict(d=0), 'd must be'), (dict(dtype=2), 'dtype'), (dict(row0=-2), 'cand_row0'),
             (dict(row0=8, nc=4), 'cand_row0 + n_cand'), (dict(row0=0, xc=dummy), 'x_cand and match must be NULL'),
             (dict(mh=okp, md=None), 'both'), (dict(xc=None), 'NULL'), (dict(w=None), 'NULL'), (dict(out_stride=3), 'out_stride')]
    for kw, msg in cases:
        assert vr(**kw) < 0, kw
        assert msg.encode() in lib.lcgp_last_error(), (kw, lib.lcgp_last_error())
    for vals in ([-1, 3, 50, -1], [-2, 0, 0, 0]):
        bad, bp = match(vals)
        assert vr(mh=bp, md=dummy) < 0
        assert b'match must be -1 or a training index' in lib.lcgp_last_error()
    assert lib.lcgp_variance_reduction_prepare(None, 0, 0, 50, 2, 3, 2, dummy, None, dummy, dummy, 0, dummy, dummy) < 0
    assert b'n_ref' in lib.lcgp_last_error()
    assert lib.lcgp_variance_reduction_prepare(None, 0, 0, 50, 2, 3, 2, dummy, None, dummy, dummy, 5, None, dummy) < 0
    assert b'NULL' in lib.lcgp_last_error()
    assert lib.lcgp_variance_reduction_prepare(None, 0, 0, 50, 127, 3, 2, dummy, None, dummy, dummy, 5, dummy, dummy) < 0
    assert b'd must be' in lib.lcgp_last_error()
