"""Box averages on a conditioned view and the covariance of every row's average with a reference row's on the GPU
(lcgp_condition_predict_marginal: the masked cross_kernel instance against the view's inputs, marg_refrow_kernel,
marg_refcov_kernel) against the float64 numpy restatement on the augmented data (tests/condition_marginal_ref.py), with the
augmented HotPathEngine's own figures beside them; the bitwise properties that guard the unchanged paths; NaN under either
row's mask; a Gauss-Legendre rule over the GPU's own pointwise queries on the view; float32; main_effects end to end.

Shapes: n = 300 (full) / 150 x 2 (rep), q = 2, d in {3, 34} (34 straddles the 32-dimension chunk), m in {1, 70}, n0 in {1, 70, 130}
(64- and 128-row tiles), the mask mix of tests/test_gpu_marginal.py.

Units, float64 (tests/test_gpu_condition.py): per component the largest latent variance of the BASE model over 130 points for
gvar and gcov, the largest |ghat| of the restatement for ghat; bar 1e-10, fixed.  float32 against the float64 restatement: the
base model's rows 4 x 5.81e-6 of the largest entry (tests/test_gpu_marginal.py; gcov in units of the largest variance entry, a
covariance being bounded by the variances), the view 2e-3 of the units above (tests/test_gpu_condition.py).  Every case prints
its figures before it asserts.

Measured on an MI355X, worst over the 18 float64 cases, view / augmented engine: ghat' 3.4e-13 / 3.3e-13, gvar' 9.7e-15 / 9.9e-15,
gcov' 5.5e-15 / 6.4e-15; gcov of the fitted model 6.0e-15.  float32: the model's rows ghat 5.81e-6, gvar 1.6e-6, gcov 1.4e-6; the view
ghat' 1.2e-5, gvar' 1.1e-6, gcov' 9.9e-7.  Gauss-Legendre over the view's own pointwise queries: mean 2.0e-10, variance 8.7e-11,
covariance 2.8e-10 (bar 1.6e-9)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lcgp_amd.engine as engine_mod
from lcgp_amd import _hip
from lcgp_amd.engine import HotPathEngine
from tests import condition_marginal_ref as cref
from tests import marginal_ref as ref
from tests.test_condition_host import new_columns
from tests.test_gpu_condition import _engine_args, _new_runs, _training
from tests.test_gpu_marginal import F32_BAR, QUAD_BOX, QUAD_KEEP, _boxes, _free_port, _model, _rows
from tests.test_gpu_variance_reduction import _points
from tests.test_marginal_host import CPU_QUAD_DEV, GL_NODES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL64 = 1e-10
TOL32 = 2e-3


def _ref_row(d, seed=1):
    """a reference row that keeps some dimensions and integrates others (across the 32-dimension chunk when d > 32)"""
    rng = np.random.default_rng(seed + d)
    xr, mr = rng.uniform(0.0, 1.0, d), np.arange(d) % 3 == 1
    xr[mr] = np.nan
    return xr, mr


def _restate(m, xn, yn, x0s, mask, box, row):
    """per component (ghat, gvar, gcov) of the model (xn = None) or of the model on the augmented data, float64 numpy"""
    eng = m._ensure_aux()
    x, s, Y = _training(m)
    out = []
    for th in np.asarray(eng._theta_last):
        new = (np.zeros((0, x.shape[1])), np.zeros(0), np.zeros((Y.shape[0], 0))) if xn is None else new_columns(m, xn, yn)
        xa, sa, low, z = cref.augmented(th, x, s, Y, m.kernel, *new)
        gh, gv = ref.latent_marginal(x0s, mask, box, xa, sa, th, low, z, m.kernel)
        out.append((gh, gv, cref.marginal_cov(x0s, mask, np.where(row[1], 0.0, row[0]), row[1], box, xa, sa, th, low, m.kernel)))
    return out


def _units(m, want, x):
    """(uh, uv) per component: max |ghat| of the restatement; the largest gvar of the base model over 130 points"""
    base = m._ensure_aux().predict_block(m._standardise_x0(_points(x, 130, 2))[0]).cpu().numpy()
    return np.array([np.max(np.abs(w[0])) for w in want]), base[1].max(axis=1)


def _errors(got, want, uh, uv):
    return [max(float(np.max(np.abs(got[j, k] - w[j]))) / (uh[k] if j == 0 else uv[k]) for k, w in enumerate(want)) for j in range(3)]


CASES = [('full', 'matern32', 3, 1), ('full', 'se', 34, 70), ('rep', 'matern52', 3, 70), ('rep', 'matern32', 34, 1),
         ('full', 'matern52', 34, 70), ('rep', 'se', 3, 70)]


@pytest.mark.parametrize('mode,kernel,d,k', CASES)
def test_view_and_covariance_against_the_restatement_on_the_augmented_data(mode, kernel, d, k):
    """ghat', gvar' and gcov' of the view, and gcov of the model, against dense float64 numpy; beside them the augmented engine's
    own predict_marginal_block (its ghat, gvar and gcov, the latter through the same new kernel on other data)"""
    m, x = _model(mode, kernel, d)
    x = np.asarray(x)
    eng = m._ensure_aux()
    xn, yn = _new_runs(m, x, k, 3)
    view = m.condition(xn, yn)
    rows = eng._theta_last.copy()
    xt, s, Y = _training(m)
    xn_s, snew, ycol = new_columns(m, xn, yn)
    aug = HotPathEngine(np.vstack([xt, xn_s]), np.hstack([Y, ycol]), None if mode == 'full' else np.r_[s, snew],
                        q_local=len(rows), kernel=kernel)
    aug.evaluate(rows)
    x0s, mask = _rows(d, n0=130)
    row = _ref_row(d)
    box = _boxes(d)[1]
    for n0 in (1, 70, 130):
        sl = slice(4, 5) if n0 == 1 else slice(0, n0)                     # (row 4: a random mask)
        a, b = x0s[sl], mask[sl]
        want_v, want_m = _restate(m, xn, yn, a, b, box, row), _restate(m, None, None, a, b, box, row)
        uh, uv = _units(m, want_v, x)
        got_v = eng.predict_marginal_block(a, b, box, state=view._state, ref=row).cpu().numpy()
        got_m = eng.predict_marginal_block(a, b, box, ref=row).cpu().numpy()
        got_a = aug.predict_marginal_block(a, b, box, ref=row).cpu().numpy()
        assert got_v.shape == got_m.shape == (3, 2, n0)
        ev, em, ea = _errors(got_v, want_v, uh, uv), _errors(got_m, want_m, uh, uv), _errors(got_a, want_v, uh, uv)
        print('condition marginal %s %s d=%d m=%d n0=%d: view ghat %.3e gvar %.3e gcov %.3e | model ghat %.3e gvar %.3e gcov %.3e | '
              'augmented engine ghat %.3e gvar %.3e gcov %.3e' % ((mode, kernel, d, k, n0) + tuple(ev) + tuple(em) + tuple(ea)))
        assert np.all(np.isfinite(got_v)) and np.all(np.isfinite(got_m))
        assert max(ev) <= TOL64 and max(em) <= TOL64, (ev, em)
        # the first two rows do not depend on the reference row
        assert np.array_equal(got_m[:2], eng.predict_marginal_block(a, b, box).cpu().numpy())
        assert np.array_equal(got_v[:2], eng.predict_marginal_block(a, b, box, state=view._state).cpu().numpy())


@pytest.mark.parametrize('kernel,k', [('se', 70), ('matern52', 1)])
def test_float32_against_the_float64_restatement(kernel, k):
    d = 3
    m32, x = _model('full', kernel, d, dtype='float32')
    m64, _ = _model('full', kernel, d)
    x = np.asarray(x)
    xn, yn = _new_runs(m64, x, k, 5)
    x0s, mask = _rows(d)
    row = _ref_row(d)
    box = _boxes(d)[1]
    want_v, want_m = _restate(m64, xn, yn, x0s, mask, box, row), _restate(m64, None, None, x0s, mask, box, row)
    uh, uv = _units(m64, want_v, x)
    e32 = m32._ensure_aux()
    got_m = e32.predict_marginal_block(x0s, mask, box, ref=row).cpu().numpy()
    # the base model's rows: relative to the largest entry, the covariance to the largest variance entry
    em = [max(float(np.max(np.abs(got_m[j, c] - w[j]))) / np.max(np.abs(w[min(j, 1)])) for c, w in enumerate(want_m)) for j in range(3)]
    v32 = m32.condition(xn, yn)
    lo, span = m32.x_min.numpy().reshape(-1), (m32.x_max - m32.x_min).numpy().reshape(-1)
    raw = lambda t: lo + span * t                                # noqa: E731
    res = v32.predict_marginal(raw(np.where(mask, 0.0, x0s)), mask, box=raw(box), latent=True,
                               cov_with=(raw(np.where(row[1], 0.0, row[0])), row[1]))
    got_v = np.stack([t.numpy() for t in res])
    ev = _errors(got_v, want_v, uh, uv)
    print('condition marginal float32 %s m=%d (view on the %s engine): model ghat %.3e gvar %.3e gcov %.3e (bar %.2e) | view ghat '
          '%.3e gvar %.3e gcov %.3e (bar %.1e)' % ((kernel, k, v32._engine.dtype_name) + tuple(em) + (F32_BAR,) + tuple(ev) + (TOL32,)))
    assert got_v.dtype == np.float64 and np.all(np.isfinite(got_v))
    assert max(em) <= F32_BAR, em
    assert max(ev) <= TOL32, ev


# ---- bitwise ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_rows_with_an_empty_mask_are_bitwise_condition_predict_block(dtype):
    d = 34
    m, x = _model('rep', 'se', d, dtype=dtype)
    eng, xn_s, t, r = _engine_args(m, *_new_runs(m, np.asarray(x), 70, 7))
    state = eng.condition_begin(xn_s, t, r)
    x0s, mask = _rows(d)
    empty = ~mask.any(axis=1)
    plain = eng.condition_predict_block(state, np.where(mask, 0.5, x0s)).cpu().numpy()
    got = eng.predict_marginal_block(x0s, mask, _boxes(d)[1], state=state).cpu().numpy()
    assert np.array_equal(got[:, :, empty], plain[:, :, empty])
    assert not np.array_equal(got[:, :, ~empty], plain[:, :, ~empty])
    for n0 in (70, 200):                                           # no row integrates anything: 64-row and 128-row tiles
        x0 = np.random.default_rng(4).uniform(0, 1, (n0, d))
        got = eng.predict_marginal_block(x0, np.zeros((n0, d), bool), _boxes(d)[1], state=state, ref=_ref_row(d)).cpu().numpy()
        assert np.array_equal(got[:2], eng.condition_predict_block(state, x0).cpu().numpy())


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_bitwise_independent_of_scratch_content_chunk_size_and_q_local(monkeypatch, dtype):
    """300 rows: one pass, 200 + 128 (moved back), 128 + 128 + 128; three scratch fills; an engine of its own per component"""
    d = 34
    m, x = _model('rep', 'matern32', d, dtype=dtype)
    eng, xn_s, t, r = _engine_args(m, *_new_runs(m, np.asarray(x), 70, 8))
    state = eng.condition_begin(xn_s, t, r)
    x0s, mask = _rows(d, n0=300)
    box, row = _boxes(d)[1], _ref_row(d)
    want_v = eng.predict_marginal_block(x0s, mask, box, state=state, ref=row).cpu().numpy()
    want_m = eng.predict_marginal_block(x0s, mask, box, ref=row).cpu().numpy()
    plain = eng.predict_marginal_block(x0s, mask, box).cpu().numpy()
    assert np.all(np.isfinite(want_v)) and np.all(np.isfinite(want_m)) and want_v.shape == (3, 2, 300)
    assert np.array_equal(want_m[:2], plain)                        # the reference row changes nothing in ghat and gvar
    for fill in (0x00, 0xFF, 0x5A):
        eng._scratch.fill_(fill)
        assert np.array_equal(eng.predict_marginal_block(x0s, mask, box, state=state, ref=row).cpu().numpy(), want_v), fill
        eng._scratch.fill_(fill)
        assert np.array_equal(eng.predict_marginal_block(x0s, mask, box, ref=row).cpu().numpy(), want_m), fill
    # q_local = 1 against all components
    xt, s, Y = _training(m)
    rows = eng._theta_last
    for k in range(len(rows)):
        solo = HotPathEngine(xt, Y, s, q_local=1, dtype=dtype, kernel=m.kernel)
        solo.evaluate(rows[k:k + 1])
        got = solo.predict_marginal_block(x0s, mask, box, state=solo.condition_begin(xn_s, t[k:k + 1], r), ref=row).cpu().numpy()
        assert np.array_equal(got[:, 0], want_v[:, k]), k
        assert np.array_equal(solo.predict_marginal_block(x0s, mask, box, ref=row).cpu().numpy()[:, 0], want_m[:, k]), k
    for chunk in (200, 128, 1):
        monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', chunk)
        eng._scratch.fill_(0x5A)
        assert np.array_equal(eng.predict_marginal_block(x0s, mask, box, state=state, ref=row).cpu().numpy(), want_v), chunk
        assert np.array_equal(eng.predict_marginal_block(x0s, mask, box, ref=row).cpu().numpy(), want_m), chunk
        assert np.array_equal(eng.predict_marginal_block(x0s, mask, box).cpu().numpy(), plain), chunk


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_values_under_either_rows_mask_are_never_loaded(dtype):
    """the library itself gets NaN, 0 or 1e30 under the masks of the rows and of the reference row (the engine would upload zeros)"""
    import ctypes as C
    d, n0 = 34, 70
    m, x = _model('full', 'matern52', d, dtype=dtype)
    eng, xn_s, t, r = _engine_args(m, *_new_runs(m, np.asarray(x), 70, 9))
    state = eng.condition_begin(xn_s, t, r)
    x0s, mask = _rows(d)
    box, (xr, mr) = _boxes(d)[1], _ref_row(d)
    want = eng.predict_marginal_block(x0s, mask, box, state=state, ref=(xr, mr)).cpu().numpy()
    md = torch.as_tensor(mask.astype(np.uint8)).to(eng.device)
    mrd = torch.as_tensor(mr.astype(np.uint8)).to(eng.device)
    bd = torch.as_tensor(box).to(eng.device)
    mm, view, kp = eng._view_args(state)
    nsc = eng._scratch.numel()
    head = (eng._stream(), eng.dtype, eng.kernel_id, eng.n, d, eng.p, eng.q_local, eng._p(eng.x), eng._p(eng.sr),
            eng._p(eng.theta_dev), eng._p(eng.workspace)) + view
    for junk in (np.nan, 0.0, 1e30):
        x0d = torch.as_tensor(np.where(mask, junk, x0s)).to(eng.device, eng.tdtype).contiguous()
        xrd = torch.as_tensor(np.where(mr, junk, xr)[None, :]).to(eng.device, eng.tdtype).contiguous()
        wide = torch.full((eng.q_local, kp), np.nan, dtype=eng.tdtype, device=eng.device)
        one = torch.full((2, eng.q_local, 1), np.nan, dtype=torch.float64, device=eng.device)
        out = torch.full((3, eng.q_local, n0), np.nan, dtype=torch.float64, device=eng.device)
        with torch.cuda.device(eng.device):
            _hip.check(eng.lib.lcgp_condition_predict_marginal(
                *head, 1, eng._p(xrd), eng._p(mrd), eng._p(bd), eng._p(eng._scratch), nsc, eng._p(one[0]), eng._p(one[1]), 1,
                0, eng._p(wide), None, None, None, None), 'lcgp_condition_predict_marginal')
            _hip.check(eng.lib.lcgp_condition_predict_marginal(
                *head, n0, eng._p(x0d), eng._p(md), eng._p(bd), eng._p(eng._scratch), nsc, eng._p(out[0]), eng._p(out[1]), n0,
                0, None, eng._p(wide), eng._p(xrd), eng._p(mrd), C.c_void_p(out[2].data_ptr())),
                'lcgp_condition_predict_marginal')
        assert np.array_equal(out.cpu().numpy(), want), junk


def test_two_ranks_equal_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_condition_marginal_gpu_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


# ---- the GPU's own pointwise queries under the Gauss-Legendre rule -------------------------------------------------------------
def test_gauss_legendre_over_the_views_own_pointwise_queries():
    """SE, d = 3, m = 5 new runs of which one lies outside the box: two dimensions integrated (each pair).  Mean from
    view.predict()'s latents at the nodes, variance w^T Sigma' w from view.predict_latent_cov minus nt_k scale_k sum w_i^2 (that
    matrix carries the nugget on its diagonal), covariance with the overall row w_i^T Sigma' w_r from the off-diagonal block of
    the same matrix over the nodes of both rows.  Bar: ten times the deviation of the rule the CPU test recorded.  Nothing of the
    closed forms enters the reference."""
    m, x = _model('full', 'se', 3)
    lo, span = m.x_min.numpy().reshape(-1), (m.x_max - m.x_min).numpy().reshape(-1)
    to_raw = lambda s: lo + span * s                             # noqa: E731
    xn_s = np.array([[0.3, 0.6, 0.2], [0.7, 0.4, 0.5], [0.5, 0.9, 0.7], [0.15, 0.3, 0.1], [1.05, 0.1, 0.9]])
    view = m.condition(to_raw(xn_s), np.random.default_rng(11).standard_normal((3, 5)) + 0.3)
    th = np.asarray(m._ensure_aux()._theta_last)
    nugget = th[:, 3] * th[:, 4] / (1.0 + th[:, 4])             # nt_k scale_k
    an, aw = ref.tensor_rule(GL_NODES, QUAD_BOX, [0, 1, 2])
    worst = 0.0
    for keep in range(3):
        dims = [l for l in range(3) if l != keep]
        nodes, wts = ref.tensor_rule(GL_NODES, QUAD_BOX, dims)
        k = len(wts)
        x0s = np.full((3, 3), np.nan)
        x0s[:, keep] = QUAD_KEEP
        mask = np.ones((3, 3), bool)
        mask[:, keep] = False
        gh, gv, gc = [t.numpy() for t in view.predict_marginal(to_raw(np.where(mask, 0.0, x0s)), mask, box=to_raw(QUAD_BOX),
                                                               latent=True, cov_with=(np.full(3, np.nan), [0, 1, 2]))]
        mean, var, cov = np.empty((2, 3)), np.empty((2, 3)), np.empty((2, 3))
        for i, v in enumerate(QUAD_KEEP):
            pts = np.empty((k, 3))
            pts[:, dims] = nodes
            pts[:, keep] = v
            both = to_raw(np.vstack([pts, an]))
            mean[:, i] = view.predict(both[:k], latent=True)[0].numpy() @ wts
            S = view.predict_latent_cov(both).numpy()
            var[:, i] = np.einsum('i,kij,j->k', wts, S[:, :k, :k], wts) - nugget * np.sum(wts * wts)
            cov[:, i] = np.einsum('i,kij,j->k', wts, S[:, :k, k:], aw)
        em, ev, ec = (np.max(np.abs(mean - gh)) / np.max(np.abs(gh)), np.max(np.abs(var - gv)) / np.max(np.abs(gv)),
                      np.max(np.abs(cov - gc)) / np.max(np.abs(gc)))
        print('gauss-legendre on the view', keep, 'mean', em, 'var', ev, 'cov', ec)
        worst = max(worst, em, ev, ec)
    assert worst <= 10.0 * CPU_QUAD_DEV, worst


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_main_effects_end_to_end_on_model_and_view():
    """n = 300, d = 3, p = 3, q = 2, SE: the five old fields of main_effects equal predict_marginal of the same rows to the bit,
    with and without effect_var; effect_var is var + overall_var - 2 ycov of predict_marginal(cov_with = the overall row)"""
    m, x = _model('full', 'se', 3)
    x = np.asarray(x)
    xn, yn = _new_runs(m, x, 70, 6)
    G = 9
    for q in (m, m.condition(xn, yn)):
        plain, me = q.main_effects(grid=G), q.main_effects(grid=G, effect_var=True)
        assert plain.effect_var is None and me.effect_var.shape == (3, 3, G) and me.mean.shape == (3, 3, G)
        x0 = np.full((3 * G + 1, 3), np.nan)
        mask = np.ones((3 * G + 1, 3), bool)
        for l in range(3):
            x0[l * G:(l + 1) * G, l] = me.grid.numpy()[l]
            mask[l * G:(l + 1) * G, l] = False
        yp, ycv = [t.numpy() for t in q.predict_marginal(x0, mask)]
        yp3, ycv3, ycov = [t.numpy() for t in q.predict_marginal(x0, mask, cov_with=(x0[-1], mask[-1]))]
        assert np.array_equal(yp, yp3) and np.array_equal(ycv, ycv3) and ycov.shape == (3, 3 * G + 1)
        for e in (plain, me):
            assert np.array_equal(e.mean.numpy(), yp[:, :-1].reshape(3, 3, G))
            assert np.array_equal(e.var.numpy(), ycv[:, :-1].reshape(3, 3, G))
            assert np.array_equal(e.overall.numpy(), yp[:, -1]) and np.array_equal(e.overall_var.numpy(), ycv[:, -1])
            assert np.array_equal(e.effect.numpy(), e.mean.numpy() - e.overall.numpy()[:, None, None])
            np.testing.assert_allclose(e.grid.numpy(), np.stack([np.linspace(x[:, l].min(), x[:, l].max(), G) for l in range(3)]),
                                       rtol=1e-14)
        ev = me.effect_var.numpy()
        assert np.array_equal(ev, (ycv[:, :-1] + ycv[:, -1:] - 2.0 * ycov[:, :-1]).reshape(3, 3, G))
        assert np.all(ev >= -1e-12 * np.max(ycv)) and np.all(ev < me.var.numpy() + me.overall_var.numpy()[:, None, None])
        # the overall row's covariance with itself is its variance (the same sums in another order)
        np.testing.assert_allclose(ycov[:, -1], ycv[:, -1], rtol=1e-9)
        print('main effects', 'view' if q is not m else 'model', 'effect_var / var: min %.3e max %.3e'
              % (np.min(ev / me.var.numpy()), np.max(ev / me.var.numpy())))
