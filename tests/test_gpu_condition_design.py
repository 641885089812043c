"""Design queries on a conditioned view on the GPU (lcgp_condition_vr_* / lcgp_condition_select_*: the base model's kernels on
rows widened to K' = npad + mpad) against a HotPathEngine built on the augmented data at the same theta rows (its own
variance_reduction_block / select_*: the code of the fitted model) and against dense float64 numpy on the augmented data
(tests/test_condition_design_host.closed_form3 / DenseState3: the project's closed_form and DenseState on all three kernels); the select / condition identity;
bitwise-equal results on poisoned scratch, for one component against all, for any split of the candidates, for any pass size of
begin and on two ranks; the base model and the view's predict untouched; float32 against float64; the public API.

Shapes: n = 333 training inputs (no multiple of 64), q = 3, m in {1, 70, 150} (K' = 512, 512, 640; m = 1 leaves 127 padded tail
columns), n_ref and n_cand in {1, 130} and once n_cand = 2100 (two passes of the row former), d in {1, 6}, the three kernels,
full and rep with replicates 1 and 3 and candidates that are base training inputs, select size 5.

Bounds, float64: the project's figure for a variance reduction (tests/test_gpu_variance_reduction.py), per component 1e-10 of the
largest gvar of the BASE model over the case's reference points; through the score 1e-10 * max gvar * sum omega
(tests/test_gpu_select_batch.py).  tau = 1 / D can make S ill-conditioned, so every case also measures the augmented engine
against the same dense oracle: where the view exceeds the fixed bound, the admissible bound is 4 x the augmented engine's own
error on that case (the rule of tests/test_gpu_condition.py); it is never derived from the view's numbers.  float32 against
float64: 2e-3 of the same units.  Every case prints its figures before it asserts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lcgp_amd import engine as engine_mod
from lcgp_amd.engine import HotPathEngine
from tests.test_condition_design_host import DenseState3, closed_form3
from tests.test_condition_host import new_columns
from tests.test_gpu_condition import _engine_args, _model, _new_runs, _training
from tests.test_gpu_variance_reduction import _free_port, _match, _points
from tests.test_predict_hess_host import _cross
from tests.test_select_batch_host import omega_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL64 = 1e-10
TOL32 = 2e-3
CASES = [('full', 'matern32', 1, 1), ('full', 'se', 6, 70), ('full', 'matern52', 6, 150), ('rep', 'matern32', 6, 70),
         ('rep', 'se', 1, 150), ('rep', 'matern52', 1, 1)]


class Augmented:
    """the two references of a case: the training set augmented by the new runs, factorised densely in float64 numpy at the
    theta rows of the model's factorisation, and a HotPathEngine built on it and evaluated at the same rows"""

    def __init__(self, m, xn, yn):
        eng = m._ensure_aux()
        self.rows = eng._theta_last.copy()
        x, s, Y = _training(m)
        xn_s, snew, ycol = new_columns(m, xn, yn)
        self.x, self.s, self.kernel = np.vstack([x, xn_s]), np.r_[s, snew], m.kernel
        d = x.shape[1]
        self.low = []
        for th in self.rows:
            Cm = _cross(self.x, self.x, th[:d], th[d], th[d + 1], m.kernel)
            np.fill_diagonal(Cm, th[d])
            self.low.append(np.linalg.cholesky(np.eye(len(self.x)) + th[d + 2] * Cm * np.outer(self.s, self.s)))
        self.engine = HotPathEngine(self.x, np.hstack([Y, ycol]), None if m.submethod == 'full' else self.s,
                                    q_local=len(self.rows), kernel=m.kernel)
        self.engine.evaluate(self.rows)

    def dense_R(self, xr_s, xc_s, w, match, r):
        return np.array([closed_form3(th, low, self.x, self.s, self.kernel, xr_s, xc_s, w, match, r)
                         for th, low in zip(self.rows, self.low)])

    def dense_states(self, xr_s, xc_s, w, match, r):
        return [DenseState3(th, low, self.x, self.s, self.kernel, xr_s, xc_s, w, match, r) for th, low in zip(self.rows, self.low)]


def _candidates(m, x, k, seed):
    """k candidates inside the data's box; on the rep path (k >= 100) three of them are base training inputs"""
    xc = _points(x, k, seed)
    if m.submethod == 'rep' and k >= 100:
        xc[[70, 71, 72]] = m.x_unique.numpy()[[0, 7, 33]]
    return xc


def _args(m, xc, xr, w):
    xc_s = m._standardise_x0(xc)[0]
    xr_s = xc_s if xr is None else m._standardise_x0(xr)[0]
    wn = np.full(len(xr_s), 1.0 / len(xr_s)) if w is None else np.asarray(w, float) / np.sum(w)
    match = _match(m, xc_s) if m.submethod == 'rep' else None
    return xr_s, xc_s, wn, match


def _gv_unit(m, xr_s):
    """(q, 1): the largest gvar of the base model over the reference points, per component"""
    return m._ensure_aux().predict_block(xr_s)[1].cpu().numpy().max(axis=1)[:, None]


def _check_R(m, view, aug, xc, xr, w, r, tag):
    R = view.variance_reduction(xc, x_ref=xr, weights=w, replicates=r, latent=True).numpy()
    xr_s, xc_s, wn, match = _args(m, xc, xr, w)
    dense = aug.dense_R(xr_s, xc_s, wn, match, r)
    eng_R = aug.engine.variance_reduction_block(xc_s, xr_s, wn, match, r).cpu().numpy()
    unit = _gv_unit(m, xr_s)
    ev = float(np.max(np.abs(R - dense) / unit))
    ea = float(np.max(np.abs(eng_R - dense) / unit))
    xv = float(np.max(np.abs(R - eng_R) / unit))
    bound = max(TOL64, 4 * ea)
    print('view ALC %s: view vs dense %.3e | augmented engine vs dense %.3e | view vs augmented engine %.3e | bound %.1e'
          % (tag, ev, ea, xv, bound))
    assert R.shape == dense.shape and np.all(np.isfinite(R)) and np.all(R >= -TOL64 * unit)
    assert ev <= bound, (tag, ev, bound)
    assert xv <= bound + ea, (tag, xv)
    return R


@pytest.mark.parametrize('mode,kernel,d,k', CASES)
def test_variance_reduction_matches_the_augmented_engine_and_dense_numpy(mode, kernel, d, k):
    m, x = _model(mode, kernel, d)
    xn, yn = _new_runs(m, x, k, 3)
    view = m.condition(xn, yn)
    aug = Augmented(m, xn, yn)
    xc, xr = _candidates(m, x, 130, 21), _points(x, 130, 22)
    w = np.random.default_rng(23).random(130) + 0.05
    if mode == 'rep':
        assert np.sum(_match(m, m._standardise_x0(xc)[0]) >= 0) == 3
    for r in ((1, 3) if mode == 'rep' else (1,)):
        for n_ref in (1, 130):
            for n_cand in (1, 130):
                _check_R(m, view, aug, xc[:n_cand], xr[:n_ref], w[:n_ref], r,
                         '%s %s d=%d m=%d r=%d n_ref=%d n_cand=%d' % (mode, kernel, d, k, r, n_ref, n_cand))
        _check_R(m, view, aug, xc, None, None, r, '%s %s d=%d m=%d r=%d shared' % (mode, kernel, d, k, r))


def test_variance_reduction_over_two_passes_of_the_row_former():
    m, x = _model('full', 'matern52', 6)
    xn, yn = _new_runs(m, x, 70, 4)
    view = m.condition(xn, yn)
    aug = Augmented(m, xn, yn)
    xc, xr = _points(x, 2100, 24), _points(x, 130, 25)
    assert engine_mod.PREDICT_CHUNK == 2048
    R = _check_R(m, view, aug, xc, xr, None, 1, 'full matern52 d=6 m=70 n_ref=130 n_cand=2100')
    # the candidates in two calls of other sizes: bitwise
    a = view.variance_reduction(xc[:1000], x_ref=xr, latent=True).numpy()
    b = view.variance_reduction(xc[1000:], x_ref=xr, latent=True).numpy()
    assert np.array_equal(np.hstack([a, b]), R)
    # 2100 reference points: the reference set takes two passes too
    _check_R(m, view, aug, xc[:130], xc, None, 1, 'full matern52 d=6 m=70 n_ref=2100 n_cand=130')


# ---- select_batch ------------------------------------------------------------------------------------------------------
def _score(om, R, picked):
    s = np.zeros(R.shape[1])
    for k in range(len(om)):
        s = s + om[k] * R[k]
    s[list(picked)] = -np.inf
    return s


def _replay(m, aug, xr_s, xc_s, wn, match, r, idx, om):
    """(dense oracle, augmented engine): score rows (len(idx), n_cand) each, row t conditioned on the given picks idx[:t]"""
    states = aug.dense_states(xr_s, xc_s, wn, match, r)
    dense, eng_rows = np.empty((len(idx), len(xc_s))), np.empty((len(idx), len(xc_s)))
    e = aug.engine
    e.select_begin(xc_s, xr_s, wn, match, r, len(idx))
    for t in range(len(idx)):
        dense[t] = _score(om, np.array([st.rows() for st in states]), idx[:t])
        eng_rows[t] = _score(om, e.select_rows().cpu().numpy(), idx[:t])
        if t + 1 < len(idx):
            for st in states:
                st.condition(int(idx[t]))
            e.select_condition(int(idx[t]))
    return dense, eng_rows


def _check_select(m, view, aug, xc, size, xr, w, r, tag):
    idx, gain, scores = (t.numpy() for t in view.select_batch(xc, size, x_ref=xr, weights=w, replicates=r, return_scores=True))
    xr_s, xc_s, wn, match = _args(m, xc, xr, w)
    om = omega_of(m)
    unit = float(_gv_unit(m, xr_s).max() * np.sum(om))
    dense, eng_rows = _replay(m, aug, xr_s, xc_s, wn, match, r, idx, om)
    assert idx.dtype == np.int64 and len(set(idx.tolist())) == size and scores.shape == (size, len(xc))
    ev = ea = xv = 0.0
    for t in range(size):
        live = np.setdiff1d(np.arange(len(xc)), idx[:t])
        assert np.all(np.isneginf(scores[t, idx[:t]])) and np.all(np.isfinite(scores[t, live]))
        ev = max(ev, np.max(np.abs(scores[t, live] - dense[t, live])) / unit)
        ea = max(ea, np.max(np.abs(eng_rows[t, live] - dense[t, live])) / unit)
        xv = max(xv, np.max(np.abs(scores[t, live] - eng_rows[t, live])) / unit)
        assert idx[t] == int(np.argmax(scores[t])) and gain[t] == scores[t, idx[t]]
    bound = max(TOL64, 4 * ea)
    print('view select_batch %s: over %d steps view vs dense %.3e | augmented engine vs dense %.3e | view vs augmented engine %.3e '
          '| bound %.1e (units of max gvar * sum omega); gain %s' % (tag, size, ev, ea, xv, bound, gain.tolist()))
    assert ev <= bound, (tag, ev, bound)
    assert xv <= bound + ea, (tag, xv)
    assert np.all(np.diff(gain) <= bound * unit), (tag, gain)
    return idx, gain, scores


@pytest.mark.parametrize('mode,kernel,d,k', CASES)
def test_select_batch_every_step_on_replayed_picks(mode, kernel, d, k):
    m, x = _model(mode, kernel, d)
    xn, yn = _new_runs(m, x, k, 5)
    view = m.condition(xn, yn)
    aug = Augmented(m, xn, yn)
    xc, xr = _candidates(m, x, 130, 26), _points(x, 130, 27)
    w = np.random.default_rng(28).random(130) + 0.05
    for r in ((1, 3) if mode == 'rep' else (1,)):
        tag = '%s %s d=%d m=%d r=%d' % (mode, kernel, d, k, r)
        _check_select(m, view, aug, xc, 5, xr, w, r, tag + ' n_ref=130')
        _check_select(m, view, aug, xc, 5, xr[:1], None, r, tag + ' n_ref=1')
        _check_select(m, view, aug, xc, 5, None, None, r, tag + ' shared')


def test_select_batch_over_two_passes_and_size_edges():
    m, x = _model('full', 'matern52', 6)
    xn, yn = _new_runs(m, x, 70, 6)
    view = m.condition(xn, yn)
    aug = Augmented(m, xn, yn)
    xc, xr = _points(x, 2100, 29), _points(x, 130, 30)
    _check_select(m, view, aug, xc, 5, xr, None, 1, 'full matern52 d=6 m=70 n_cand=2100')
    idx, _, _ = _check_select(m, view, aug, xc[:5], 5, xr, None, 1, 'size = n_cand = 5')
    assert sorted(idx.tolist()) == list(range(5))
    idx, _, _ = _check_select(m, view, aug, xc[:1], 1, xr[:1], None, 1, 'n_cand = n_ref = 1')
    assert idx.tolist() == [0]


@pytest.mark.parametrize('kernel,d', [('matern32', 6), ('se', 1)])
def test_select_condition_identity(kernel, d):
    """step t's score row of base.select_batch equals sum_k omega_k R'_k of the view conditioned on the first t picks (full
    path, r = 1, any outputs: ALC ignores them).  The bound's fallback is 4 x the error of base.select_batch -- the code of the
    fitted model -- against the dense oracle replaying its picks."""
    from tests.test_gpu_select_batch import oracle_rows
    m, x = _model('full', kernel, d)
    xc, xr = _points(x, 130, 31), _points(x, 130, 32)
    idx, gain, scores = (t.numpy() for t in m.select_batch(xc, 4, x_ref=xr, return_scores=True))
    xr_s, xc_s, wn, _ = _args(m, xc, xr, None)
    om = omega_of(m)
    unit = float(_gv_unit(m, xr_s).max() * np.sum(om))
    dense = oracle_rows(m, xr_s, xc_s, wn, None, 1, idx, om)
    y_any = np.random.default_rng(33).standard_normal((int(m.p), 4))
    for t in range(1, 4):
        view = m.condition(xc[idx[:t]], y_any[:, :t])
        R = view.variance_reduction(xc, x_ref=xr, latent=True).numpy()
        live = np.setdiff1d(np.arange(len(xc)), idx[:t])
        got = _score(om, R, [])
        ev = np.max(np.abs(got[live] - scores[t, live])) / unit
        ea = np.max(np.abs(scores[t, live] - dense[t, live])) / unit
        bound = max(TOL64, 4 * ea)
        print('select / condition identity %s d=%d step %d: view vs select_batch row %.3e | select_batch vs dense %.3e | bound %.1e'
              % (kernel, d, t, ev, ea, bound))
        assert ev <= bound, (t, ev, bound)


# ---- bitwise -----------------------------------------------------------------------------------------------------------
def _view_state(m, xn, yn):
    eng, xn_s, t, r = _engine_args(m, xn, yn)
    return eng, eng.condition_begin(xn_s, t, r), xn_s, t, r


def _host_loop(eng, state, xc_s, xr_s, wn, match, r, size, om, picks=None):
    """the step-by-step route on a view: score rows for its own argmax picks, or for the given ones"""
    eng.condition_select_begin(state, xc_s, xr_s, wn, match, r, size)
    idx, rows = [], np.empty((size, len(xc_s)))
    for t in range(size):
        rows[t] = _score(om, eng.condition_select_rows().cpu().numpy(), idx)
        idx.append(int(np.argmax(rows[t])) if picks is None else int(picks[t]))
        if t + 1 < size:
            eng.condition_select_condition(idx[-1])
    return np.array(idx), rows


@pytest.mark.parametrize('mode,dtype', [('full', 'float64'), ('rep', 'float64'), ('rep', 'float32')])
def test_bitwise_poisoned_scratch_splits_pass_rows_and_one_component(mode, dtype, monkeypatch):
    m, x = _model(mode, 'matern32', 6, dtype=dtype)
    xn, yn = _new_runs(m, x, 70, 7)
    xc, xr = _candidates(m, x, 130, 34), _points(x, 130, 35)
    r = 2 if mode == 'rep' else 1
    eng, state, xn_s, tt, rr = _view_state(m, xn, yn)
    xr_s, xc_s, wn, match = _args(m, xc, xr, None)
    om = omega_of(m)
    for ref in (xr_s, None):
        wr = wn if ref is not None else np.full(130, 1.0 / 130)
        R = eng.condition_variance_reduction_block(state, xc_s, ref, wr, match, r).cpu().numpy()
        idx, sc = [t.cpu().numpy() for t in eng.condition_select_batch_block(state, xc_s, ref, wr, match, r, 5, om)]
        assert np.array_equal(sc[0], _score(om, R, []))              # step 0 IS the view's variance reduction
        for fill in (0xFF, 0x00, 0x5A):                              # 0xFF: NaN in both dtypes
            eng._scratch.fill_(fill)
            assert np.array_equal(eng.condition_variance_reduction_block(state, xc_s, ref, wr, match, r).cpu().numpy(), R), fill
            eng._scratch.fill_(fill)
            got = [t.cpu().numpy() for t in eng.condition_select_batch_block(state, xc_s, ref, wr, match, r, 5, om)]
            assert np.array_equal(got[0], idx) and np.array_equal(got[1], sc), fill
        if ref is not None:
            # candidates split 130 = 64 + 66 over two calls
            eng._scratch.fill_(0xFF)
            a = eng.condition_variance_reduction_block(state, xc_s[:64], ref, wr, None if match is None else match[:64], r)
            b = eng.condition_variance_reduction_block(state, xc_s[64:], ref, wr, None if match is None else match[64:], r)
            assert np.array_equal(np.hstack([a.cpu().numpy(), b.cpu().numpy()]), R)
        # pass_rows of begin: 64 against 2048, and the step-by-step host loop
        monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', 64)
        eng._scratch.fill_(0x5A)
        got = [t.cpu().numpy() for t in eng.condition_select_batch_block(state, xc_s, ref, wr, match, r, 5, om)]
        assert np.array_equal(got[0], idx) and np.array_equal(got[1], sc)
        assert np.array_equal(eng.condition_variance_reduction_block(state, xc_s, ref, wr, match, r).cpu().numpy(), R)
        monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', 2048)
        eng._scratch.fill_(0xFF)
        hi, hrows = _host_loop(eng, state, xc_s, ref, wr, match, r, 5, om)
        assert np.array_equal(hi, idx) and np.array_equal(hrows, sc)
    # the view's gvar' (the h of step 0) is bitwise condition_predict_block's gvar where the row has no match
    eng.condition_select_begin(state, xc_s, xr_s, wn, match, r, 5)
    sel = eng._sel
    h = torch.empty((eng.q_local, 130), dtype=torch.float64, device=eng.device)
    from lcgp_amd import _hip
    _hip.check(eng.lib.lcgp_condition_select_state(eng._stream(), *sel['dims'], 1, *sel['scs'], eng._p(h)), 'state')
    h = h.cpu().numpy()
    gv = eng.condition_predict_block(state, xc_s)[1].cpu().numpy()
    free = np.ones(130, bool) if match is None else match < 0
    assert np.array_equal(h[:, free], gv[:, free]) and free.sum() >= 127
    # q_local = 1 against all components: an engine of its own holding component k alone
    R = eng.condition_variance_reduction_block(state, xc_s, xr_s, wn, match, r).cpu().numpy()
    idx, sc = [t.cpu().numpy() for t in eng.condition_select_batch_block(state, xc_s, xr_s, wn, match, r, 5, om)]
    xt, s, Y = _training(m)
    rows = eng._theta_last
    one = np.ones(1)
    for k in range(len(rows)):
        solo = HotPathEngine(xt, Y, None if mode == 'full' else s, q_local=1, dtype=dtype, kernel=m.kernel)
        solo.evaluate(rows[k:k + 1])
        st = solo.condition_begin(xn_s, tt[k:k + 1], rr)
        assert np.array_equal(solo.condition_variance_reduction_block(st, xc_s, xr_s, wn, match, r).cpu().numpy()[0], R[k]), k
        # its state after the picks of the full run: R_k of every step
        _, solo_rows = _host_loop(solo, st, xc_s, xr_s, wn, match, r, 5, one, picks=idx)
        eng.condition_select_begin(state, xc_s, xr_s, wn, match, r, 5)
        for t in range(5):
            assert np.array_equal(eng.condition_select_rows().cpu().numpy()[k][np.setdiff1d(np.arange(130), idx[:t])],
                                  solo_rows[t][np.setdiff1d(np.arange(130), idx[:t])]), (k, t)
            if t + 1 < 5:
                eng.condition_select_condition(int(idx[t]))


def test_two_ranks_reproduce_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_condition_design_gpu_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


# ---- the base model and the view's predict are only read ------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_base_model_and_view_predict_untouched(mode):
    m, x = _model(mode, 'se', 6)
    xn, yn = _new_runs(m, x, 70, 10)
    xc, xr, x0 = _candidates(m, x, 130, 36), _points(x, 130, 37), _points(x, 130, 38)
    r = 3 if mode == 'rep' else 1

    def base_queries():
        out = [t.numpy().copy() for t in m.predict(x0)]
        out.append(m.variance_reduction(xc, x_ref=xr, replicates=r, latent=True).numpy().copy())
        out += [t.numpy().copy() for t in m.select_batch(xc, 5, x_ref=xr, replicates=r, return_scores=True)]
        return out
    before = base_queries()
    eng = m._ensure_aux()
    view = m.condition(xn, yn)
    p0 = [t.numpy().copy() for t in view.predict(x0, latent=True)]
    R = view.variance_reduction(xc, x_ref=xr, replicates=r, latent=True).numpy()
    view.select_batch(xc, 5, x_ref=xr, replicates=r)
    p1 = [t.numpy() for t in view.predict(x0, latent=True)]
    assert all(np.array_equal(a, b) for a, b in zip(p0, p1))
    assert m._ensure_aux() is eng
    after = base_queries()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    # the new runs took variance away: the view's reduction differs from the base model's and is never larger in total
    assert np.max(np.abs(R - before[3])) > 0
    assert np.array_equal(view.variance_reduction(xc, x_ref=xr, replicates=r, latent=True).numpy(), R)


@pytest.mark.parametrize('mode,kernel,d,k', [('full', 'se', 6, 70), ('rep', 'matern32', 6, 150)])
def test_float32_against_float64(mode, kernel, d, k):
    m64, x = _model(mode, kernel, d)
    m32, _ = _model(mode, kernel, d, dtype='float32')
    xn, yn = _new_runs(m64, x, k, 6)
    xc, xr = _candidates(m64, x, 130, 39), _points(x, 130, 40)
    r = 3 if mode == 'rep' else 1
    v64, v32 = m64.condition(xn, yn), m32.condition(xn, yn)
    print('view design float32 model: the view was built on the %s engine' % v32._engine.dtype_name)
    a = v64.variance_reduction(xc, x_ref=xr, replicates=r, latent=True).numpy()
    b = v32.variance_reduction(xc, x_ref=xr, replicates=r, latent=True).numpy()
    xr_s, xc_s, wn, match = _args(m64, xc, xr, None)
    unit = _gv_unit(m64, xr_s)
    ev = np.max(np.abs(a - b) / unit)
    # select: the float32 view replays the float64 view's picks
    om = omega_of(m64)
    idx, _, s64 = (t.numpy() for t in v64.select_batch(xc, 5, x_ref=xr, replicates=r, return_scores=True))
    _, s32 = _host_loop(v32._engine, v32._state, xc_s, xr_s, wn, match, r, 5, om, picks=idx)
    es = 0.0
    for t in range(5):
        live = np.setdiff1d(np.arange(130), idx[:t])
        assert np.all(np.isfinite(s32[t, live]))
        es = max(es, np.max(np.abs(s32[t, live] - s64[t, live])) / (unit.max() * np.sum(om)))
    print('view design float32 vs float64 %s %s m=%d: ALC %.3e, select rows %.3e (bound %.1e)' % (mode, kernel, k, ev, es, TOL32))
    assert b.dtype == np.float64 and np.all(np.isfinite(b))
    assert ev <= TOL32 and es <= TOL32
    i32, g32 = v32.select_batch(xc, 5, x_ref=xr, replicates=r)
    assert len(set(i32.tolist())) == 5 and np.all(np.isfinite(g32.numpy()))


# ---- public API ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_public_api_shapes_dtypes_staleness_and_the_rep_refusal(mode):
    m, x = _model(mode, 'matern32', 2)
    xn, yn = _new_runs(m, x, 5, 14)
    view = m.condition(xn, yn)
    xc, xr = _points(x, 9, 41), _points(x, 7, 42)
    delta = view.variance_reduction(torch.as_tensor(xc), x_ref=torch.as_tensor(xr), weights=np.arange(1.0, 8.0), outputs=[0, 2])
    ref = m.variance_reduction(xc, x_ref=xr, weights=np.arange(1.0, 8.0), outputs=[0, 2])
    assert isinstance(delta, torch.Tensor) and delta.dtype == ref.dtype == torch.float64 and delta.shape == ref.shape == (2, 9)
    assert delta.device == ref.device and not delta.requires_grad and torch.all(torch.isfinite(delta)) and torch.all(delta >= 0)
    R = view.variance_reduction(xc, x_ref=xr, weights=np.arange(1.0, 8.0), latent=True).numpy()
    W, _, scale, _ = m._output_map()
    np.testing.assert_array_equal(delta.numpy(), (W[:, [0, 2]] ** 2).T @ R * (scale[[0, 2]] ** 2)[:, None])
    assert R.shape == (3, 9)
    idx, gain = view.select_batch(xc, 4, x_ref=xr)
    i2, g2, sc = view.select_batch(xc, 4, x_ref=xr, return_scores=True)
    assert idx.dtype == torch.int64 and idx.shape == (4,) and gain.dtype == torch.float64 and gain.shape == (4,)
    assert sc.shape == (4, 9) and torch.equal(idx, i2) and torch.equal(gain, g2)
    with pytest.raises(ValueError, match='size must be'):
        view.select_batch(xc, 10)
    with pytest.raises(ValueError, match='duplicate rows'):
        view.select_batch(np.vstack([xc, xc[:1]]), 2)
    with pytest.raises(ValueError, match='x_cand must have shape'):
        view.variance_reduction(xc[:, :1])
    xu = view.x_new.numpy()
    again = np.vstack([xc[:3], xu[1:2]])
    if mode == 'rep':
        for call in (lambda: view.variance_reduction(again), lambda: view.select_batch(again, 2)):
            with pytest.raises(ValueError, match='refit'):
                call()
        assert view.variance_reduction(np.vstack([xc[:3], m.x_unique.numpy()[4:5]]), replicates=2).shape == (4, 4)
    else:
        assert view.variance_reduction(again).shape == (4, 4)      # one more new row with its own nugget
        with pytest.raises(ValueError, match='replicates must be 1'):
            view.variance_reduction(xc, replicates=2)
    m._set_flat(m._get_flat() + 0.01)
    for call in (lambda: view.variance_reduction(xc), lambda: view.select_batch(xc, 2)):
        with pytest.raises(RuntimeError, match='stale'):
            call()
    m.predict(xc)
    with pytest.raises(RuntimeError, match='stale'):
        view.variance_reduction(xc)
    assert m.condition(xn, yn).select_batch(xc, 2)[0].shape == (2,)
