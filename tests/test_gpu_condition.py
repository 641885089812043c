"""Conditioning on new runs on the GPU (lcgp_condition_prepare / lcgp_condition_predict: OP_COND_CROSS of the tile kernel)
against a HotPathEngine built on the augmented data at the same theta rows (its own predict_block) and against dense float64
numpy (tests/test_condition_host.dense_augmented); bitwise-equal results on poisoned scratch, state and cond workspace, for one
component against all, for any split of the rows on one tile size and on two ranks; the base model untouched; limits; the
public API.

Shapes: n = 333 training inputs (no multiple of 64), m in {1, 70, 150} (one short tile, across a 64 and a 128 boundary), n0 in
{1, 130} and once 2100 (two passes stitched through out_stride), d in {1, 6}, the three kernels, full and rep with 1 to 3
replicates, float64 and float32.

Bounds, float64: the project's figure for a conditioned posterior (tests/test_gpu_variance_reduction.py,
test_gpu_select_batch.py), per component 1e-10 of the largest latent variance for gvar -- taken as the largest gvar of the BASE
model over the case's 130 new inputs -- and 1e-10 of max |ghat| of the dense oracle over them for ghat.  tau = 1 / D can make S
ill-conditioned, so every case also measures the augmented engine (the parent's code) against the same dense oracle: where the
view exceeds the fixed bound, the admissible bound is 4 x the augmented engine's own error on that case (two extra triangular
products).  It is never derived from the view's numbers.  float32 against float64: 2e-3 of the same units
(test_gpu_select_batch.py).  Every case prints its figures before it asserts.

There is no case of a float64 S that is not positive definite: its condition number is bounded by 1 + m scale D, about 1e8 at
the ceiling of the scale, and no valid input reaches 1e16 (tests/test_condition_host.py shows it on the CPU stand-in)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lcgp_amd import LCGP, _hip, synth
from lcgp_amd import engine as engine_mod
from lcgp_amd.engine import HotPathEngine
from lcgp_amd.lcgp import ConditionedLCGP
from oracle import lcgp_oracle as orc
from tests.test_condition_host import dense_augmented, new_columns
from tests.test_gpu_variance_reduction import _free_port, _points

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL64 = 1e-10
TOL32 = 2e-3
N = 333


def _model(mode, kernel='matern32', d=2, q=3, dtype='float64', p=4):
    if mode == 'full':
        x, y = synth.make_full(95, N, d, p, q)
    else:
        x, y = synth.make_rep(96, N, 2, d, p, q)        # 333 unique inputs, two replicates each
    m = LCGP(y=y, x=x, q=q, submethod=mode, kernel=kernel, device='cuda:0', dtype=dtype)
    o = orc.OracleLCGP(y=y, x=x, q=q, submethod=mode)
    m._set_flat(synth.param_points(95, o.get_unconstrained())[1])
    return m, np.asarray(x)


def _new_runs(m, x, k, seed):
    """k new unique inputs inside the data's box and outputs for them: one run each on the full path, 1 to 3 replicates in
    shuffled order on the rep path"""
    rng = np.random.default_rng(seed)
    xu = _points(x, k, seed)
    if m.submethod == 'rep':
        xu = xu[rng.permutation(np.repeat(np.arange(k), 1 + np.arange(k) % 3))]
    return xu, rng.standard_normal((int(m.p), len(xu))) + 0.2


def _training(m):
    """the engine's training set in float64: standardised inputs, sqrt(r), Y"""
    if m.submethod == 'rep':
        s = np.sqrt(m.r.numpy().astype(float))
        yb = (m.ybar_s if m.rep_standardize_ybar else m.ybar).numpy()
        return m.x_unique_s.numpy(), s, yb * s[None, :]
    return m.x.numpy(), np.ones(int(m.n)), m.y.numpy()


def _references(m, xn, yn, x0):
    """(dense oracle, augmented engine): ghat, gvar (q, n0) each, at the theta rows of the model's factorisation"""
    eng = m._ensure_aux()
    rows = eng._theta_last.copy()
    x, s, Y = _training(m)
    xn_s, snew, ycol = new_columns(m, xn, yn)
    x0s = m._standardise_x0(x0)[0]
    dense = dense_augmented(rows, x, s, Y, m.kernel, xn_s, snew, ycol, x0s)
    aug = HotPathEngine(np.vstack([x, xn_s]), np.hstack([Y, ycol]), None if m.submethod == 'full' else np.r_[s, snew],
                        q_local=len(rows), kernel=m.kernel)
    aug.evaluate(rows)
    blk = aug.predict_block(x0s).cpu().numpy()
    return dense, (blk[0], blk[1])


def _check64(m, x, xn, yn, x0, tag):
    """the view at x0 against both references, in the units of the docstring: per component the largest gvar of the base model
    and the largest |ghat| of the dense oracle over the 130 points _points(x, 130, 2)"""
    view = m.condition(xn, yn)
    gh, gv = [t.numpy() for t in view.predict(x0, latent=True)]
    (dh, dv), (ah, av) = _references(m, xn, yn, x0)
    pts = _points(x, 130, 2)
    pts_s = m._standardise_x0(pts)[0]
    base = m._ensure_aux().predict_block(pts_s).cpu().numpy()
    ph = dense_augmented(m._ensure_aux()._theta_last, *_training(m), m.kernel, *new_columns(m, xn, yn), pts_s)[0]
    uv, uh = base[1].max(axis=1)[:, None], np.abs(ph).max(axis=1)[:, None]

    def err(a, b, unit):
        return float(np.max(np.abs(a - b) / unit))
    ev, eh = err(gv, dv, uv), err(gh, dh, uh)               # the view against the dense oracle
    av_, ah_ = err(av, dv, uv), err(ah, dh, uh)             # the augmented engine against the dense oracle
    xv, xh = err(gv, av, uv), err(gh, ah, uh)               # the view against the augmented engine
    bv, bh = max(TOL64, 4 * av_), max(TOL64, 4 * ah_)
    print('condition %s: view vs dense gvar %.3e ghat %.3e | augmented engine vs dense gvar %.3e ghat %.3e | view vs augmented '
          'engine gvar %.3e ghat %.3e | bounds %.1e %.1e' % (tag, ev, eh, av_, ah_, xv, xh, bv, bh))
    assert np.all(np.isfinite(gh)) and np.all(np.isfinite(gv))
    assert ev <= bv and eh <= bh, (tag, ev, eh, bv, bh)
    assert xv <= bv + av_ and xh <= bh + ah_, (tag, xv, xh)
    return view, gh, gv


CASES = [('full', 'matern32', 1, 1), ('full', 'se', 6, 70), ('full', 'matern52', 6, 150), ('rep', 'matern32', 6, 70),
         ('rep', 'se', 1, 150), ('rep', 'matern52', 1, 1)]


@pytest.mark.parametrize('mode,kernel,d,k', CASES)
def test_view_matches_the_augmented_engine_and_dense_numpy(mode, kernel, d, k):
    m, x = _model(mode, kernel, d)
    xn, yn = _new_runs(m, x, k, 3)
    x0 = _points(x, 130, 2)
    for n0 in (1, 130):
        view, gh, gv = _check64(m, x, xn, yn, x0[:n0], '%s %s d=%d m=%d n0=%d' % (mode, kernel, d, k, n0))
        assert view.m == k and gh.shape == (3, n0)


def test_two_passes_are_stitched_through_out_stride():
    m, x = _model('full', 'matern52', 6)
    xn, yn = _new_runs(m, x, 70, 4)
    x0 = _points(x, 2100, 5)
    assert engine_mod.PREDICT_CHUNK == 2048
    view, gh, gv = _check64(m, x, xn, yn, x0, 'full matern52 d=6 m=70 n0=2100')
    # the second pass (52 rows, 64-row tiles) wrote its own columns and nothing else
    tail = [t.numpy() for t in view.predict(x0[2048:], latent=True)]
    assert np.array_equal(gh[:, 2048:], tail[0]) and np.array_equal(gv[:, 2048:], tail[1])


@pytest.mark.parametrize('mode,kernel,d,k', [('full', 'se', 6, 70), ('rep', 'matern32', 6, 150)])
def test_float32_against_float64(mode, kernel, d, k):
    m64, x = _model(mode, kernel, d)
    m32, _ = _model(mode, kernel, d, dtype='float32')
    xn, yn = _new_runs(m64, x, k, 6)
    x0 = _points(x, 130, 2)
    a = [t.numpy() for t in m64.condition(xn, yn).predict(x0, latent=True)]
    v32 = m32.condition(xn, yn)
    b = [t.numpy() for t in v32.predict(x0, latent=True)]
    assert b[0].dtype == np.float64
    print('condition float32 model: the view was built on the %s engine' % v32._engine.dtype_name)
    base = m64._ensure_aux().predict_block(m64._standardise_x0(x0)[0]).cpu().numpy()
    eh = np.max(np.abs(a[0] - b[0]) / np.abs(a[0]).max(axis=1)[:, None])
    ev = np.max(np.abs(a[1] - b[1]) / base[1].max(axis=1)[:, None])
    print('condition float32 vs float64 %s %s m=%d: ghat %.3e gvar %.3e (bound %.1e)' % (mode, kernel, k, eh, ev, TOL32))
    assert np.all(np.isfinite(b[0])) and np.all(np.isfinite(b[1]))
    assert eh <= TOL32 and ev <= TOL32


# ---- bitwise -----------------------------------------------------------------------------------------------------------
def _filled(nbytes, fill, device):
    return torch.full((int(nbytes),), fill, dtype=torch.uint8, device=device)


def _raw(eng, xn_s, t, r, x0s, fill, splits=None):
    """(2, q_local, n0) through the C entries with buffers of this test's own, every one filled with `fill` before the call
    that uses it: the cond workspace, the state, the scratch of the preparation and of every prediction pass"""
    lib, dev, q, d = eng.lib, eng.device, eng.q_local, eng.d
    m, n0 = len(xn_s), len(x0s)
    splits = [(0, n0)] if splits is None else splits
    nb = eng._nbytes
    cws = _filled(nb("lcgp_workspace_bytes", eng.dtype, m, d, eng.p, q), fill, dev)
    state = _filled(nb("lcgp_condition_state_bytes", eng.dtype, eng.n, d, q, m), fill, dev)
    nsc = max([nb("lcgp_condition_scratch_bytes", eng.dtype, eng.n, q, m, 0)] +
              [nb("lcgp_condition_scratch_bytes", eng.dtype, eng.n, q, m, rows) for _, rows in splits])
    scratch = _filled(nsc, fill, dev)
    xnd = torch.as_tensor(np.ascontiguousarray(xn_s)).to(dev, eng.tdtype).contiguous()
    x0d = torch.as_tensor(np.ascontiguousarray(x0s)).to(dev, eng.tdtype).contiguous()
    td = torch.as_tensor(np.ascontiguousarray(t)).to(dev)
    rd = None if r is None else torch.as_tensor(np.ascontiguousarray(r, np.float64)).to(dev)
    info = torch.zeros(q, dtype=torch.int32, device=dev)
    out = torch.empty((2, q, n0), dtype=torch.float64, device=dev)
    p = eng._p
    with torch.cuda.device(dev):
        st = eng._stream()
        _hip.check(lib.lcgp_condition_prepare(st, eng.dtype, eng.kernel_id, eng.n, d, eng.p, q, p(eng.x), p(eng.sr), p(eng.theta_dev),
                                              p(eng.workspace), m, p(xnd), p(td), p(rd), p(scratch), nsc, p(cws), p(state), p(info)),
                   "lcgp_condition_prepare")
        assert not np.any(info.cpu().numpy())
        for lo, rows in splits:
            scratch.fill_(fill)
            _hip.check(lib.lcgp_condition_predict(st, eng.dtype, eng.kernel_id, eng.n, d, eng.p, q, p(eng.x), p(eng.sr),
                                                  p(eng.theta_dev), p(eng.workspace), p(state), m, p(xnd), rows,
                                                  C.c_void_p(x0d.data_ptr() + lo * d * x0d.element_size()), p(scratch), nsc,
                                                  C.c_void_p(out[0].data_ptr() + 8 * lo), C.c_void_p(out[1].data_ptr() + 8 * lo),
                                                  n0), "lcgp_condition_predict")
        return out.cpu().numpy()


def _engine_args(m, xn, yn):
    eng = m._ensure_aux()
    xn_s, snew, ycol = new_columns(m, xn, yn)
    rows = eng._theta_last
    d = eng.d
    t = (rows[:, d + 3:] @ (ycol / snew[None, :])) / rows[:, d + 2][:, None]
    return eng, xn_s, t, (snew * snew if m.submethod == 'rep' else None)


@pytest.mark.parametrize('mode,dtype', [('full', 'float64'), ('rep', 'float64'), ('rep', 'float32')])
def test_bitwise_on_poisoned_memory_row_splits_and_one_component(mode, dtype):
    m, x = _model(mode, 'matern32', 6, dtype=dtype)
    xn, yn = _new_runs(m, x, 70, 7)
    x0 = _points(x, 130, 8)
    x0s = m._standardise_x0(x0)[0]
    eng, xn_s, t, r = _engine_args(m, xn, yn)
    ref = eng.condition_predict_block(eng.condition_begin(xn_s, t, r), x0s).cpu().numpy()
    gh, gv = [a.numpy() for a in m.condition(xn, yn).predict(x0, latent=True)]
    # the model's t and r are this test's (t to rounding: on the rep path the test divides the sqrt(r) back out of the columns)
    np.testing.assert_allclose(gh, ref[0], rtol=0, atol=1e-12 * np.max(np.abs(ref[0])))
    np.testing.assert_allclose(gv, ref[1], rtol=0, atol=1e-12 * np.max(np.abs(ref[1])))
    for fill in (0x00, 0xFF, 0x5A):
        assert np.array_equal(_raw(eng, xn_s, t, r, x0s, fill), ref), fill
    # n0 = 130 in one call against its rows split 64 + 66, and against other splits.  A pass below 128 rows forms U_0 and T on
    # 64-row tiles, one call of 130 rows pads to 256 and takes 128-row tiles; both tile sizes add an element's k terms in the
    # same order (ascending k, four per MFMA, one accumulator), and the stages a wave skips on a triangular tile hold zeros
    a = _raw(eng, xn_s, t, r, x0s, 0x5A, splits=[(0, 64), (64, 66)])
    b = _raw(eng, xn_s, t, r, x0s, 0xFF, splits=[(0, 127), (127, 3)])
    c = _raw(eng, xn_s, t, r, x0s[:127], 0x00)
    assert np.array_equal(a, b) and np.array_equal(a[:, :, :127], c)
    print('condition %s %s: 130 rows in one call (128-row tiles) against 64 + 66 (64-row tiles): equal %s, max difference %.3e'
          % (mode, dtype, np.array_equal(a, ref), np.max(np.abs(a - ref))))
    assert np.array_equal(a, ref)
    # and on 128-row tiles: 260 rows in one call against 130 + 130
    x1 = m._standardise_x0(_points(x, 260, 9))[0]
    assert np.array_equal(_raw(eng, xn_s, t, r, x1, 0x5A), _raw(eng, xn_s, t, r, x1, 0x00, splits=[(0, 130), (130, 130)]))
    # q_local = 1 against all components: an engine of its own holding component k alone
    xt, s, Y = _training(m)
    rows = eng._theta_last
    for k in range(len(rows)):
        solo = HotPathEngine(xt, Y, None if mode == 'full' else s, q_local=1, dtype=dtype, kernel=m.kernel)
        solo.evaluate(rows[k:k + 1])
        got = solo.condition_predict_block(solo.condition_begin(xn_s, t[k:k + 1], r), x0s).cpu().numpy()
        assert np.array_equal(got[:, 0], ref[:, k]), k


def test_two_ranks_reproduce_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_condition_gpu_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


# ---- the base model is only read ----------------------------------------------------------------------------------------
def _checksum(eng):
    import hashlib
    h = hashlib.sha256()
    for k in range(eng.q_local):
        for which in (0, 1, 2):
            h.update(eng.fetch_matrix(which, k).tobytes())
        for which in (0, 1):
            h.update(eng.fetch_vector(which, k).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_base_model_untouched(mode):
    m, x = _model(mode, 'se', 6)
    xn, yn = _new_runs(m, x, 70, 10)
    x0 = _points(x, 130, 11)
    lg0 = m.loss_and_grad()
    p0 = [t.numpy().copy() for t in m.predict(x0)]
    eng = m._ensure_aux()
    ck0 = _checksum(eng)
    view = m.condition(xn, yn)
    a = [t.numpy() for t in view.predict(x0)]
    b = [t.numpy() for t in view.predict(x0[:50])]
    assert all(np.array_equal(u[:, :50], v) for u, v in zip(a, b))
    assert _checksum(eng) == ck0 and m._ensure_aux() is eng
    p1 = [t.numpy() for t in m.predict(x0)]
    assert all(np.array_equal(u, v) for u, v in zip(p0, p1))
    assert np.max(np.abs(a[0] - p0[0])) > 0
    lg1 = m.loss_and_grad()
    assert lg0[0] == lg1[0] and np.array_equal(lg0[1], lg1[1])
    view.predict(x0[:3])                                 # the same parameters, factorised again: the view is still current


# ---- limits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_variance_at_the_new_inputs_and_a_far_away_run(mode):
    m, x = _model(mode, 'matern32', 6)
    xn, yn = _new_runs(m, x, 70, 12)
    eng = m._ensure_aux()
    rows = eng._theta_last
    d = eng.d
    scale, nug, D = rows[:, d][:, None], rows[:, d + 1][:, None], rows[:, d + 2][:, None]
    view = m.condition(xn, yn)
    xu = view.x_new.numpy()
    r = np.array([np.sum(np.all(xn == u[None, :], axis=1)) for u in xu], float)[None, :]
    _, gv1 = [t.numpy() for t in view.predict(xu, latent=True)]
    gv0 = eng.predict_block(m._standardise_x0(xu)[0])[1].cpu().numpy()
    tau = 1.0 / (D * r)
    # conditioning on input i alone already gives a - c^2 / (a + tau), a = gvar_i, c = a less the nugget's share (the cross
    # covariance of the continuous surface has none); more inputs only lower it.  That is at most tau + 2 scale nt.
    c = gv0 - scale * nug / (1.0 + nug)
    one = gv0 - c * c / (gv0 + tau)
    print('condition limits %s: max gvar after / before %.3e, max gvar after / tau %.3e' % (mode, np.max(gv1 / gv0), np.max(gv1 / tau)))
    assert np.all(gv1 < gv0) and np.all(gv1 <= one + TOL64 * scale) and np.all(gv1 <= tau + 2 * scale * nug / (1 + nug))
    # one run far outside the data changes nothing inside it
    far = x.max(axis=0)[None, :] + 1e4 * (x.max(axis=0) - x.min(axis=0))[None, :]
    x0 = _points(x, 130, 13)
    vf = m.condition(far, yn[:, :1])
    gh, gv = [t.numpy() for t in vf.predict(x0, latent=True)]
    base = eng.predict_block(m._standardise_x0(x0)[0]).cpu().numpy()
    eh = np.max(np.abs(gh - base[0]) / np.abs(base[0]).max(axis=1)[:, None])
    ev = np.max(np.abs(gv - base[1]) / base[1].max(axis=1)[:, None])
    print('condition far-away run %s: ghat %.3e gvar %.3e' % (mode, eh, ev))
    assert eh <= TOL64 and ev <= TOL64


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_info_word_of_a_non_positive_definite_s_reaches_the_engines_error(dtype):
    """The route of the info word through the real library: factorisation -> copy_stats_kernel -> the LinAlgError of
    condition_begin with .info per local component.  No valid input makes S indefinite in float64 (module docstring), so the
    engine is handed what the public API cannot produce: a NEGATIVE replicate count, tau_2 = 1 / (D r_2) far below -S_22."""
    m, x = _model('rep', 'matern32', 2, dtype=dtype)
    xn, yn = _new_runs(m, x, 5, 16)
    x0s = m._standardise_x0(_points(x, 9, 17))[0]
    eng, xn_s, t, r = _engine_args(m, xn, yn)
    good = eng.condition_predict_block(eng.condition_begin(xn_s, t, r), x0s).cpu().numpy()
    base = eng.predict_block(x0s).cpu().numpy()
    bad = r.copy()
    bad[2] = -1e-9
    with pytest.raises(np.linalg.LinAlgError, match='not numerically positive definite') as ei:
        eng.condition_begin(xn_s, t, bad)
    info = np.asarray(ei.value.info)
    print('condition %s: info words of S with a negative count at input 2: %s' % (dtype, info.tolist()))
    assert info.shape == (eng.q_local,) and np.all(info == 3)         # 1 + the first failing pivot, every component
    # nothing of the model was harmed, and the next preparation in the same cond workspace is the first one's bitwise
    assert np.array_equal(eng.predict_block(x0s).cpu().numpy(), base)
    assert np.array_equal(eng.condition_predict_block(eng.condition_begin(xn_s, t, r), x0s).cpu().numpy(), good)


# ---- public API ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_public_api_shapes_dtypes_and_staleness(mode):
    m, x = _model(mode, 'matern32', 2)
    xn, yn = _new_runs(m, x, 5, 14)
    view = m.condition(torch.as_tensor(xn), torch.as_tensor(yn))
    assert isinstance(view, ConditionedLCGP) and view.base is m and view.m == 5 and tuple(view.x_new.shape) == (5, 2)
    assert repr(view).startswith('ConditionedLCGP(m=5')
    x0 = _points(x, 9, 15)
    res, ref = view.predict(x0), m.predict(x0)
    assert len(res) == 3
    for a, b in zip(res, ref):
        assert isinstance(a, torch.Tensor) and a.dtype == b.dtype == torch.float64 and a.shape == b.shape == (4, 9)
        assert a.device == b.device and not a.requires_grad and torch.all(torch.isfinite(a))
    assert torch.all(res[2] <= ref[2] * (1 + 1e-12))          # conditioning never raises the confidence variance
    gh, gv = view.predict(x0, latent=True)
    assert gh.shape == gv.shape == (3, 9) and gh.dtype == gv.dtype == torch.float64
    for a, b in zip(m._outputs(gh.numpy(), gv.numpy()), res):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match='equals a training input'):
        m.condition(np.vstack([xn[:2], x[3:4]]), yn[:, :3])
    m._set_flat(m._get_flat() + 0.01)
    with pytest.raises(RuntimeError, match='stale'):
        view.predict(x0)
    m.predict(x0)
    with pytest.raises(RuntimeError, match='stale'):
        view.predict(x0)
    assert m.condition(xn, yn).predict(x0)[0].shape == (4, 9)
