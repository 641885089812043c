"""Joint covariance and draws of a conditioned view on the GPU (lcgp_condition_predict_cov: the widened rows of DESIGN 4.14 into
OP_PRED_COV with K = K', then the unchanged lcgp_potrf_logdet / lcgp_sample_latent) against dense float64 numpy on the augmented
data (tests/test_condition_joint_host.dense_joint) and against a HotPathEngine built on the augmented data at the same theta
rows (its own predict_cov); the diagonals against the view's marginals; the factor and the draws; bitwise-equal results on
poisoned scratch and cov workspace, for one component against all and on two ranks; the base model and the view's other queries
untouched; float32 against float64; a far-away run.

Shapes: those of tests/test_gpu_condition.py -- n = 333, q = 3, the six full / rep x kernel cases with d in {1, 6} and m in
{1, 70, 150} (m = 1: 127 zero tail columns; m = 150: two column tiles), n0 in {1, 130} (n0 = 1: the slab is padded to 128 rows,
the row former works on 64; n0 = 130: a ragged n0pad = 256) and once 2100 (two blocks of the row former, the second of 52 rows).
Rows 1 .. 3 of x0 are training inputs and row 4 is one of the view's inputs (n0 = 130, 2100).

Bounds, float64, per component k in units of scale_k (tests/test_gpu_joint.py's figures): the covariance against dense numpy
1e-10, its diagonal against view.predict(latent=True)'s gvar' 1e-12, the diagonals of predict_jointcov against view.predict's
ypredvar / yconfvar rtol 1e-12, symmetry exact.  tau = 1 / D can make S ill-conditioned, so every case also measures the
augmented engine's predict_cov (the parent's code) against the same dense result: where the view exceeds 1e-10 the admissible
bound is 4 x the augmented engine's own error on that case (the project's fallback rule, tests/test_gpu_condition.py); it is never
derived from the view's numbers.  float32 against float64: 2e-3 of scale_k, tests/test_gpu_condition.py's figure (the base
model's float32 joint covariance is held to stage-wise bounds in tests/test_gpu_joint_bounds.py, not to one figure).  Every case
prints its figures before it asserts.

There is no case of a jitter too small for a float32 view: at these shapes (n0 = 6 and 130 with a view input among the rows, m in
{1, 70, 150}) view.sample at the default jitter 1e-10 factorises in float32, as the base model's does, so the public API gives no
LinAlgError to assert and none was constructed; tests/test_condition_joint_host.py drives that route through a stand-in, and
tests/test_gpu_joint.py the info words of the unchanged factorisation."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lcgp_amd import _hip
from lcgp_amd.engine import HotPathEngine
from tests.test_condition_host import new_columns
from tests.test_condition_joint_host import dense_joint
from tests.test_gpu_condition import CASES, _engine_args, _filled, _model, _new_runs, _training
from tests.test_gpu_variance_reduction import _free_port, _points
from tests.test_predict_hess_host import _cross

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL64 = 1e-10
TOL_DIAG = 1e-12
TOL32 = 2e-3


def _x0(m, x, xn, n0, seed):
    """n0 new inputs inside the data's box; from 5 rows on, rows 1 .. 3 are training inputs and row 4 one of the new runs"""
    x0 = _points(x, n0, seed)
    if n0 >= 5:
        xt = m.x_unique.numpy() if m.submethod == 'rep' else x
        x0[1:4] = xt[[0, 7, 100]]
        x0[4] = xn[0]
    return x0


def _scales(m):
    eng = m._ensure_aux()
    return eng._theta_last[:, eng.d].copy()


def _dense_and_augmented(m, xn, yn, x0):
    """(ghat, Sigma) dense, and Sigma of an engine built on the augmented data, at the theta rows of the model's factorisation"""
    eng = m._ensure_aux()
    rows = eng._theta_last.copy()
    x, s, Y = _training(m)
    xn_s, snew, ycol = new_columns(m, xn, yn)
    x0s = m._standardise_x0(x0)[0]
    gh, sig = dense_joint(rows, x, s, Y, m.kernel, xn_s, snew, ycol, x0s)
    aug = HotPathEngine(np.vstack([x, xn_s]), np.hstack([Y, ycol]), None if m.submethod == 'full' else np.r_[s, snew],
                        q_local=len(rows), kernel=m.kernel)
    aug.evaluate(rows)
    return gh, sig, aug.predict_cov(x0s).cpu().numpy()


def _check64(m, x, xn, yn, x0, tag):
    view = m.condition(xn, yn)
    lc = view.predict_latent_cov(x0)
    n0 = len(x0)
    assert lc.dtype == torch.float64 and tuple(lc.shape) == (3, n0, n0)
    lc = lc.numpy()
    _, dense, aug = _dense_and_augmented(m, xn, yn, x0)
    unit = _scales(m)[:, None, None]
    ev = float(np.max(np.abs(lc - dense) / unit))
    ea = float(np.max(np.abs(aug - dense) / unit))
    bound = max(TOL64, 4 * ea)
    gv = view.predict(x0, latent=True)[1].numpy()
    ed = float(np.max(np.abs(np.diagonal(lc, axis1=1, axis2=2) - gv) / unit[:, :, 0]))
    print('condition joint %s: view vs dense %.3e | augmented engine vs dense %.3e | bound %.1e | diagonal vs gvar\' %.3e'
          % (tag, ev, ea, bound, ed))
    assert np.all(np.isfinite(lc))
    assert np.array_equal(lc, np.transpose(lc, (0, 2, 1)))
    assert ev <= bound, (tag, ev, ea, bound)
    assert ed <= TOL_DIAG, (tag, ed)
    return view, lc


@pytest.mark.parametrize('mode,kernel,d,k', CASES)
def test_view_covariance_matches_dense_numpy_and_the_marginals(mode, kernel, d, k):
    m, x = _model(mode, kernel, d)
    xn, yn = _new_runs(m, x, k, 3)
    for n0 in (1, 130):
        x0 = _x0(m, x, xn, n0, 2)
        view, lc = _check64(m, x, xn, yn, x0, '%s %s d=%d m=%d n0=%d' % (mode, kernel, d, k, n0))
        assert view.m == k
        ypred, ypredvar, yconfvar = [t.numpy() for t in view.predict(x0)]
        jc = view.predict_jointcov(x0).numpy()
        jc0 = view.predict_jointcov(x0, include_noise=False).numpy()
        assert jc.shape == (4, n0, n0)
        d1, d0 = np.diagonal(jc, axis1=1, axis2=2), np.diagonal(jc0, axis1=1, axis2=2)
        print('condition joint %s %s n0=%d: jointcov diagonal vs ypredvar %.3e, vs yconfvar %.3e (relative)'
              % (mode, kernel, n0, np.max(np.abs(d1 - ypredvar) / ypredvar), np.max(np.abs(d0 - yconfvar) / yconfvar)))
        np.testing.assert_allclose(d1, ypredvar, rtol=1e-12)
        np.testing.assert_allclose(d0, yconfvar, rtol=1e-12)
        assert np.array_equal(view.predict_jointcov(x0, outputs=[2, 0]).numpy(), jc[[2, 0]])


def test_two_blocks_of_the_row_former():
    m, x = _model('full', 'matern52', 6)
    xn, yn = _new_runs(m, x, 70, 4)
    x0 = _x0(m, x, xn, 2100, 5)
    view, lc = _check64(m, x, xn, yn, x0, 'full matern52 d=6 m=70 n0=2100')
    # the second block (52 rows) against the same rows on their own: the rows of a block do not depend on the block
    tail = view.predict_latent_cov(x0[2048:]).numpy()
    assert np.array_equal(lc[:, 2048:, 2048:], tail)


# ---- the factor and the draws ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_factor_in_the_cov_workspace_and_the_draws_from_it(mode):
    m, x = _model(mode, 'matern32', 6)
    xn, yn = _new_runs(m, x, 70, 5)
    x0 = _x0(m, x, xn, 130, 6)
    x0s = m._standardise_x0(x0)[0]
    view = m.condition(xn, yn)
    jit, seed, S = 1e-8, 21, 3
    s0 = view.sample(x0, size=S, seed=seed, include_noise=False, jitter=jit).numpy()
    eng = view._engine
    L = np.tril(eng.fetch_cov(130).cpu().numpy())           # the factor lcgp_potrf_logdet left: L L^T = Sigma' + tau I
    sig = view.predict_latent_cov(x0).numpy()
    scale = _scales(m)
    for k in range(3):
        want = sig[k] + jit * scale[k] * np.eye(130)
        e = np.max(np.abs(L[k] @ L[k].T - want)) / np.max(np.abs(want))
        print('condition joint factor %s k=%d: |L L^T - (Sigma\' + tau I)| / max %.3e' % (mode, k, e))
        assert e <= 1e-12
    # the latent draws: ghat' + L eps on the host from that factor and the same normals; a draw is a sum of at most 130 products
    # in double, so the device's order of summation moves it by at most 130 x 2^-53 x sum |L| |eps|: bound 1e-12 of the
    # largest |L| row sum times the largest normal
    gh = view.predict(x0, latent=True)[0].numpy()
    g = eng.condition_sample_latent(view._state, x0s, S, [(seed, k) for k in range(3)], jit).cpu().numpy()
    for k in range(3):
        eps = np.random.default_rng((seed, k)).standard_normal((S, 130))
        want = gh[k][None, :] + eps @ L[k].T
        tol = 1e-12 * np.max(np.sum(np.abs(L[k]), axis=1)) * np.max(np.abs(eps))
        print('condition joint draws %s k=%d: max difference %.3e (bound %.3e)' % (mode, k, np.max(np.abs(g[k] - want)), tol))
        assert np.max(np.abs(g[k] - want)) <= tol
    W, noise, sc, offset = m._output_map()
    np.testing.assert_allclose(s0, np.einsum('ka,ksi->sai', W, g) * sc[None, :, None] + offset[None, :, None], rtol=1e-12)


def test_sample_shape_seeds_and_statistics():
    m, x = _model('full', 'matern32', 2)
    xn, yn = _new_runs(m, x, 70, 8)
    view = m.condition(xn, yn)
    x0 = _points(x, 6, 12)
    s = view.sample(x0, size=4000, seed=123).numpy()
    assert s.shape == (4000, 4, 6) and np.all(np.isfinite(s))
    np.testing.assert_array_equal(s, view.sample(x0, size=4000, seed=123).numpy())
    assert not np.array_equal(s[:10], view.sample(x0, size=10, seed=124).numpy())
    ypred = view.predict(x0)[0].numpy()
    jc = view.predict_jointcov(x0).numpy()
    se = np.sqrt(np.diagonal(jc, axis1=1, axis2=2) / 4000)
    assert np.all(np.abs(s.mean(axis=0) - ypred) <= 5 * se)
    for a in range(4):
        emp = np.cov(s[:, a, :], rowvar=False)
        sd = np.sqrt(np.diag(jc[a]))
        assert np.max(np.abs(emp - jc[a]) / np.outer(sd, sd)) <= 0.1
    assert view.sample(x0, size=3, seed=1, include_noise=False).shape == (3, 4, 6)
    with pytest.raises(ValueError, match='size must be >= 1'):
        view.sample(x0, size=0)


# ---- bitwise ---------------------------------------------------------------------------------------------------------------
def _raw_cov(eng, state, x0s, fill, jitter=0.0):
    """(q_local, n0, n0) through the C entry with a scratch and a cov workspace of this test's own, both filled with `fill`"""
    lib, dev, q, d = eng.lib, eng.device, eng.q_local, eng.d
    m, n0 = state['m'], len(x0s)
    nsc = eng._nbytes("lcgp_condition_predict_cov_scratch_bytes", eng.dtype, eng.n, q, m, n0)
    scratch = _filled(nsc, fill, dev)
    cws = _filled(eng._nbytes("lcgp_workspace_bytes", eng.dtype, n0, d, eng.p, q), fill, dev)
    x0d = torch.as_tensor(np.ascontiguousarray(x0s)).to(dev, eng.tdtype).contiguous()
    out = torch.empty((q, n0, n0), dtype=eng.tdtype, device=dev)
    p = eng._p
    with torch.cuda.device(dev):
        st = eng._stream()
        _hip.check(lib.lcgp_condition_predict_cov(st, eng.dtype, eng.kernel_id, eng.n, d, eng.p, q, p(eng.x), p(eng.sr),
                                                  p(eng.theta_dev), p(eng.workspace), p(state['state']), m, p(state['xn']), n0,
                                                  p(x0d), p(scratch), nsc, p(cws), float(jitter)), "lcgp_condition_predict_cov")
        for k in range(q):
            _hip.check(lib.lcgp_fetch_matrix(st, eng.dtype, n0, d, eng.p, q, p(cws), 0, k, p(out[k])), "lcgp_fetch_matrix")
        # the padding of the matrix slot holds the identity, whatever the memory held: what the factorisation expects
        n0pad = -(-n0 // 128) * 128
        slot = cws[:q * n0pad * n0pad * out.element_size()].view(eng.tdtype).view(q, n0pad, n0pad)
        low = torch.tril(slot)
        pad = low[:, n0:, :]
        eye = torch.eye(n0pad, dtype=eng.tdtype, device=dev)[n0:, :]
        assert bool(torch.all(pad == eye[None])), 'padding rows of the matrix slot'
        return out.to(torch.float64).cpu().numpy()


@pytest.mark.parametrize('mode,dtype', [('full', 'float64'), ('rep', 'float64'), ('rep', 'float32')])
def test_bitwise_on_poisoned_memory_and_one_component(mode, dtype):
    m, x = _model(mode, 'matern32', 6, dtype=dtype)
    xn, yn = _new_runs(m, x, 70, 7)
    eng, xn_s, t, r = _engine_args(m, xn, yn)
    state = eng.condition_begin(xn_s, t, r)
    x0 = _x0(m, x, xn, 130, 8)
    x0s = m._standardise_x0(x0)[0]
    ref = eng.condition_predict_cov(state, x0s).cpu().numpy()
    lc = m.condition(xn, yn).predict_latent_cov(x0).numpy()
    # the model's r is this test's to rounding (on the rep path the test squares sqrt(r)); the covariance does not depend on t
    np.testing.assert_allclose(lc, ref, rtol=0, atol=1e-12 * np.max(np.abs(ref)))
    for fill in (0x00, 0xFF, 0x5A):
        assert np.array_equal(_raw_cov(eng, state, x0s, fill), ref), fill
        # n0 = 1: the slab's rows 64 .. 127 lie behind the row former's one block of 64
        one = _raw_cov(eng, state, x0s[:1], fill)
        assert np.array_equal(one, eng.condition_predict_cov(state, x0s[:1]).cpu().numpy()), fill
    # q_local = 1 against all components: an engine of its own holding component k alone
    xt, s, Y = _training(m)
    rows = eng._theta_last
    for k in range(len(rows)):
        solo = HotPathEngine(xt, Y, None if mode == 'full' else s, q_local=1, dtype=dtype, kernel=m.kernel)
        solo.evaluate(rows[k:k + 1])
        got = solo.condition_predict_cov(solo.condition_begin(xn_s, t[k:k + 1], r), x0s).cpu().numpy()
        assert np.array_equal(got[0], ref[k]), k


def test_bitwise_on_poisoned_memory_two_blocks():
    """n0 = 2100: the second block of the row former is 52 rows padded to 64, the slab 2176 rows -- rows 2112 .. 2175 are the
    entry's to zero"""
    m, x = _model('full', 'matern52', 6)
    xn, yn = _new_runs(m, x, 70, 4)
    eng, xn_s, t, r = _engine_args(m, xn, yn)
    state = eng.condition_begin(xn_s, t, r)
    x0s = m._standardise_x0(_x0(m, x, xn, 2100, 5))[0]
    ref = eng.condition_predict_cov(state, x0s).cpu().numpy()
    assert np.all(np.isfinite(ref))
    for fill in (0xFF, 0x5A):
        assert np.array_equal(_raw_cov(eng, state, x0s, fill), ref), fill


def test_two_ranks_reproduce_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_condition_joint_gpu_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_base_model_and_the_views_other_queries_untouched(mode):
    m, x = _model(mode, 'se', 6)
    xn, yn = _new_runs(m, x, 70, 10)
    x0 = _x0(m, x, xn, 130, 11)
    cand = _points(x, 40, 12)
    view = m.condition(xn, yn)

    def snapshot():
        return [t.numpy().copy() for t in (m.predict_jointcov(x0[:50]), m.sample(x0[:50], seed=0), *m.predict(x0), *view.predict(x0),
                                           view.variance_reduction(cand))]
    before = snapshot()
    lc = view.predict_latent_cov(x0).numpy()
    view.predict_jointcov(x0)
    view.sample(x0, size=5, seed=3, jitter=1e-8)
    after = snapshot()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert np.array_equal(view.predict_latent_cov(x0).numpy(), lc)
    m._set_flat(m._get_flat() + 0.01)
    for fn in (view.predict_latent_cov, view.predict_jointcov, view.sample):
        with pytest.raises(RuntimeError, match='stale'):
            fn(x0)


# ---- float32 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,kernel,d,k', [('full', 'se', 6, 70), ('rep', 'matern32', 6, 150)])
def test_float32_against_float64(mode, kernel, d, k):
    m64, x = _model(mode, kernel, d)
    m32, _ = _model(mode, kernel, d, dtype='float32')
    xn, yn = _new_runs(m64, x, k, 6)
    x0 = _x0(m64, x, xn, 130, 2)
    a = m64.condition(xn, yn).predict_latent_cov(x0).numpy()
    v32 = m32.condition(xn, yn)
    b = v32.predict_latent_cov(x0)
    assert b.dtype == torch.float64
    b = b.numpy()
    print('condition joint float32 model: the view was built on the %s engine' % v32._engine.dtype_name)
    e = float(np.max(np.abs(a - b) / _scales(m64)[:, None, None]))
    print('condition joint float32 vs float64 %s %s m=%d: %.3e of scale_k (bound %.1e)' % (mode, kernel, k, e, TOL32))
    assert np.all(np.isfinite(b)) and e <= TOL32
    # draws in float32: the jitter that the base model's float32 draws take (tests/test_gpu_joint_bounds.py)
    s = v32.sample(x0, size=4, seed=2, jitter=1e-3).numpy()
    assert s.shape == (4, 4, 130) and np.all(np.isfinite(s))


# ---- limits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_a_far_away_run_changes_nothing_inside_the_data(mode):
    """One run 1e4 ranges outside the data.  Where every kernel value between it and the training inputs and x0 underflows to
    exactly 0 in double (checked on the host from the theta rows), U_n, Sigma_0n and T are exact zeros, the m tail columns of the
    widened rows are zeros, and the product over K' adds exact zeros to the base model's sums in the base model's order: the
    difference is exactly 0.  Otherwise the 1e-10 bound holds."""
    m, x = _model(mode, 'matern32', 6)
    eng = m._ensure_aux()
    far = x.max(axis=0)[None, :] + 1e4 * (x.max(axis=0) - x.min(axis=0))[None, :]
    x0 = _points(x, 130, 13)
    yn = np.random.default_rng(12).standard_normal((4, 1)) + 0.2
    vf = m.condition(far, yn)
    got = vf.predict_latent_cov(x0).numpy()
    base = m.predict_latent_cov(x0).numpy()
    x0s, far_s = m._standardise_x0(x0)[0], m._standardise_x0(far)[0]
    rows, d = eng._theta_last, eng.d
    xt = _training(m)[0]
    underflow = all(np.all(_cross(np.vstack([xt, x0s]), far_s, th[:d], th[d], th[d + 1], 'matern32') == 0.0) for th in rows)
    e = float(np.max(np.abs(got - base) / _scales(m)[:, None, None]))
    print('condition joint far-away run %s: kernel values underflow to 0: %s; difference %.3e of scale_k' % (mode, underflow, e))
    if underflow:
        assert np.array_equal(got, base)
    else:
        assert e <= TOL64
