"""The ALC gradient on a conditioned view on the GPU (lcgp_condition_vr_grad: lcgp_variance_reduction_grad's launches on rows
widened to K' = npad + mpad, R_c / Q_n on the state's dense L_S^-1, and pgrad_cond_mat_kernel's contraction over the n + m columns)
against dense float64 numpy on the augmented data (tests/vr_grad_ref.value_and_grad on tests/test_gpu_condition_design.Augmented's
factorisation) and against a HotPathEngine built on the augmented data at the same theta rows (its own
variance_reduction_grad_block: the code of the fitted model); R' bitwise the view's variance_reduction; central differences of
view.variance_reduction; float32 against float64; bitwise-equal results on poisoned scratch, for any split of the candidates, any
PREDICT_CHUNK, one component against all and on two ranks; the base model, the view and the workspace untouched; the public
API and gradcheck.

Shapes: n = 333 training inputs (npad 384, no multiple of 64), q = 3, m in {1, 70, 150} (K' = 512, 512, 640; m = 1 leaves 127
padded tail columns), n_ref and n_cand in {1, 130}, once n_cand = 2100 and once n_ref = 2100 (two passes), d in {1, 6, 40} (40: the
wide instance over two dimension chunks), the three kernels, full and rep with replicates 1 and 3, candidates equal to base
training inputs and to one of the view's inputs among them, an explicit reference set and the shared one.

Bounds, float64: the unit is the largest |entry| of the dense reference, per component; the fixed bound is the project's figure
for the gradient of the fitted model, 1e-10 (tests/test_gpu_variance_reduction_grad.py).  Every case also measures the augmented
engine -- the parent's code -- against the same dense reference: where the view exceeds the fixed bound, the admissible bound is
4 x the augmented engine's own error on that case (the rule of tests/test_gpu_condition.py); it is never derived from the view's
numbers.  Central differences: the yardstick is the same difference quotient taken on the augmented engine against that engine's
own analytic gradient, bound 4 x that figure.  float32 against float64: 2e-3 of max|dR'|.  Every case prints its figures before
it asserts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lcgp_amd import engine as engine_mod
from lcgp_amd.engine import HotPathEngine
from tests.test_gpu_condition import _checksum, _model, _new_runs, _training
from tests.test_gpu_condition_design import Augmented, _view_state
from tests.test_gpu_variance_reduction import _free_port, _points
from tests.vr_grad_ref import value_and_grad

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL64 = 1e-10
TOL32 = 2e-3
CASES = [('full', 'matern32', 1, 1), ('full', 'se', 6, 70), ('full', 'matern52', 6, 150), ('rep', 'matern32', 6, 70),
         ('rep', 'se', 1, 150), ('rep', 'matern52', 1, 1), ('full', 'matern32', 40, 70), ('rep', 'matern52', 40, 1),
         ('full', 'se', 40, 150)]


def _rng(m):
    return (m.x_max.numpy() - m.x_min.numpy()).reshape(-1)


def _train_raw(m, x):
    return m.x_unique.numpy() if m.submethod == 'rep' else x


def _candidates(m, x, view, k, seed):
    """k candidates inside the data's box; from 100 on, two of them are base training inputs and one is an input of the view,
    all given bitwise: new inputs like any other to the gradient"""
    xc = _points(x, k, seed)
    if k >= 100:
        xc[[70, 71]] = _train_raw(m, x)[[0, 33]]
        xc[72] = view.x_new.numpy()[0]
    return xc


def _args(m, xc, xr, w):
    xc_s = m._standardise_x0(xc)[0]
    xr_s = None if xr is None else m._standardise_x0(xr)[0]
    n_ref = len(xc_s) if xr is None else len(xr_s)
    wn = np.full(n_ref, 1.0 / n_ref) if w is None else np.asarray(w, float) / np.sum(w)
    return xr_s, xc_s, wn


def _dense(aug, xr_s, xc_s, wn, r):
    ref = xc_s if xr_s is None else xr_s
    both = [value_and_grad(th, low, aug.x, aug.s, aug.kernel, ref, xc_s, wn, r) for th, low in zip(aug.rows, aug.low)]
    return np.array([b[0] for b in both]), np.array([b[1] for b in both])


def _check(m, view, aug, xc, xr, w, r, tag):
    """the view's (R', dR') against both references; returns the three figures of dR'"""
    R, dR = (t.numpy() for t in view.variance_reduction_grad(xc, x_ref=xr, weights=w, replicates=r, latent=True))
    xr_s, xc_s, wn = _args(m, xc, xr, w)
    dense_R, dense_dR = _dense(aug, xr_s, xc_s, wn, r)
    eng_R, eng_dR = (t.cpu().numpy() for t in aug.engine.variance_reduction_grad_block(xc_s, xr_s, wn, r))
    rng = _rng(m)
    dense_dR, eng_dR = dense_dR / rng[None, None, :], eng_dR / rng[None, None, :]
    assert R.shape == dense_R.shape and dR.shape == dense_dR.shape and np.all(np.isfinite(R)) and np.all(np.isfinite(dR))
    uR = np.max(np.abs(dense_R), axis=1)[:, None]
    uD = np.max(np.abs(dense_dR), axis=(1, 2))[:, None, None]
    figs = []
    for name, a, b_eng, dense, unit in (('R', R, eng_R, dense_R, uR), ('dR', dR, eng_dR, dense_dR, uD)):
        ev = float(np.max(np.abs(a - dense) / unit))
        ea = float(np.max(np.abs(b_eng - dense) / unit))
        xv = float(np.max(np.abs(a - b_eng) / unit))
        bound = max(TOL64, 4 * ea)
        print('view ALC gradient %s %s: view vs dense %.3e | augmented engine vs dense %.3e | view vs augmented engine %.3e | '
              'bound %.1e' % (tag, name, ev, ea, xv, bound))
        figs.append((name, ev, ea, xv, bound))
    for name, ev, ea, xv, bound in figs:
        assert ev <= bound, (tag, name, ev, bound)
        assert xv <= bound + ea, (tag, name, xv)
    return R, dR


@pytest.mark.parametrize('mode,kernel,d,k', CASES)
def test_gradient_matches_the_augmented_engine_and_dense_numpy(mode, kernel, d, k):
    m, x = _model(mode, kernel, d)
    xn, yn = _new_runs(m, x, k, 3)
    view = m.condition(xn, yn)
    aug = Augmented(m, xn, yn)
    xc, xr = _candidates(m, x, view, 130, 21), _points(x, 130, 22)
    w = np.random.default_rng(23).random(130) + 0.05
    for r in ((1, 3) if mode == 'rep' else (1,)):
        for n_ref in (1, 130):
            for n_cand in (1, 130):
                _check(m, view, aug, xc[:n_cand], xr[:n_ref], w[:n_ref], r,
                       '%s %s d=%d m=%d r=%d n_ref=%d n_cand=%d' % (mode, kernel, d, k, r, n_ref, n_cand))
        R, _ = _check(m, view, aug, xc, None, None, r, '%s %s d=%d m=%d r=%d shared' % (mode, kernel, d, k, r))
        # R' is the view's variance_reduction bit for bit where no candidate matches (full: no candidate ever does; rep: the
        # shared set holds candidates variance_reduction matches or refuses, the free ones go against an explicit set)
        if mode == 'full':
            assert np.array_equal(R, view.variance_reduction(xc, latent=True).numpy())
        Rv = view.variance_reduction(xc[:70], x_ref=xr, weights=w, replicates=r, latent=True).numpy()
        assert np.array_equal(view.variance_reduction_grad(xc[:70], x_ref=xr, weights=w, replicates=r, latent=True)[0].numpy(), Rv)


def test_gradient_over_two_passes_of_either_set():
    m, x = _model('full', 'matern52', 6)
    xn, yn = _new_runs(m, x, 70, 4)
    view = m.condition(xn, yn)
    aug = Augmented(m, xn, yn)
    xc, xr = _points(x, 2100, 24), _points(x, 130, 25)
    assert engine_mod.PREDICT_CHUNK == 2048
    R, dR = _check(m, view, aug, xc, xr, None, 1, 'full matern52 d=6 m=70 n_ref=130 n_cand=2100')
    assert np.array_equal(R, view.variance_reduction(xc, x_ref=xr, latent=True).numpy())
    # the candidates in two calls of other sizes: bitwise
    a = view.variance_reduction_grad(xc[:1000], x_ref=xr, latent=True)
    b = view.variance_reduction_grad(xc[1000:], x_ref=xr, latent=True)
    assert np.array_equal(np.hstack([a[0].numpy(), b[0].numpy()]), R)
    assert np.array_equal(np.concatenate([a[1].numpy(), b[1].numpy()], axis=1), dR)
    # 2100 reference points: the reference set takes two passes too
    _check(m, view, aug, xc[:130], xc, None, 1, 'full matern52 d=6 m=70 n_ref=2100 n_cand=130')


@pytest.mark.parametrize('mode,kernel,k,r', [('full', 'se', 70, 1), ('rep', 'matern32', 150, 3)])
def test_central_differences_of_the_views_variance_reduction(mode, kernel, k, r):
    m, x = _model(mode, kernel, 6)
    xn, yn = _new_runs(m, x, k, 5)
    view = m.condition(xn, yn)
    aug = Augmented(m, xn, yn)
    xc, xr = _candidates(m, x, view, 130, 26), _points(x, 130, 27)
    idx = np.r_[np.random.default_rng(28).choice(70, 5, replace=False), 70, 71, 72]      # 8 sampled candidates
    xr_s, xc_s, wn = _args(m, xc, xr, None)
    rng = _rng(m)
    _, dR = (t.numpy() for t in view.variance_reduction_grad(xc, x_ref=xr, replicates=r, latent=True))
    eng_dR = aug.engine.variance_reduction_grad_block(xc_s, xr_s, wn, r)[1].cpu().numpy()
    fd_v, fd_a = np.zeros((3, 8, 6)), np.zeros((3, 8, 6))
    for l in range(6):
        e, es = np.zeros(6), np.zeros(6)
        e[l], es[l] = 1e-5 * rng[l], 1e-5
        fd_v[:, :, l] = (view.variance_reduction(xc[idx] + e, x_ref=xr, replicates=r, latent=True).numpy()
                         - view.variance_reduction(xc[idx] - e, x_ref=xr, replicates=r, latent=True).numpy()) / (2 * e[l])
        fd_a[:, :, l] = (aug.engine.variance_reduction_block(xc_s[idx] + es, xr_s, wn, None, r).cpu().numpy()
                         - aug.engine.variance_reduction_block(xc_s[idx] - es, xr_s, wn, None, r).cpu().numpy()) / (2 * es[l])
    unit = np.max(np.abs(eng_dR), axis=(1, 2))[:, None, None]
    ev = float(np.max(np.abs(dR[:, idx] * rng[None, None, :] - fd_v * rng[None, None, :]) / unit))
    ea = float(np.max(np.abs(eng_dR[:, idx] - fd_a) / unit))
    print('view ALC gradient central differences %s %s m=%d r=%d: view %.3e | augmented engine (yardstick) %.3e | bound %.3e'
          % (mode, kernel, k, r, ev, ea, 4 * ea))
    assert ev <= 4 * ea, (ev, ea)


@pytest.mark.parametrize('mode,kernel,d,k', [('full', 'se', 6, 70), ('rep', 'matern32', 6, 150), ('full', 'matern52', 40, 1)])
def test_float32_against_float64(mode, kernel, d, k):
    m64, x = _model(mode, kernel, d)
    m32, _ = _model(mode, kernel, d, dtype='float32')
    xn, yn = _new_runs(m64, x, k, 6)
    r = 3 if mode == 'rep' else 1
    v64, v32 = m64.condition(xn, yn), m32.condition(xn, yn)
    print('view ALC gradient float32 model: the view was built on the %s engine' % v32._engine.dtype_name)
    xc, xr = _candidates(m64, x, v64, 130, 39), _points(x, 130, 40)
    for ref in (xr, None):
        a = v64.variance_reduction_grad(xc, x_ref=ref, replicates=r, latent=True)[1].numpy()
        b = v32.variance_reduction_grad(xc, x_ref=ref, replicates=r, latent=True)[1].numpy()
        err = np.max(np.abs(a - b)) / np.max(np.abs(a))
        print('view ALC gradient float32 vs float64 %s %s d=%d m=%d shared=%s: %.3e (bound %.1e)'
              % (mode, kernel, d, k, ref is None, err, TOL32))
        assert b.dtype == np.float64 and np.all(np.isfinite(b))
        assert err <= TOL32, err


# ---- bitwise -----------------------------------------------------------------------------------------------------------
def _both(pair):
    return [t.cpu().numpy() for t in pair]


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('mode,dtype', [('full', 'float64'), ('rep', 'float64'), ('rep', 'float32')])
def test_bitwise_poisoned_scratch_splits_chunks_and_one_component(mode, dtype, monkeypatch):
    m, x = _model(mode, 'matern32', 6, dtype=dtype)
    xn, yn = _new_runs(m, x, 70, 7)
    r = 2 if mode == 'rep' else 1
    eng, state, xn_s, tt, rr = _view_state(m, xn, yn)
    view = m.condition(xn, yn)
    xc, xr = _candidates(m, x, view, 130, 34), _points(x, 130, 35)
    xr_s, xc_s, wn = _args(m, xc, xr, None)
    for ref in (xr_s, None):
        base = _both(eng.condition_variance_reduction_grad_block(state, xc_s, ref, wn, r))
        assert base[0].shape == (3, 130) and base[1].shape == (3, 130, 6) and np.all(np.isfinite(base[1]))
        # R' is bitwise the view's variance reduction without a match
        assert np.array_equal(base[0], eng.condition_variance_reduction_block(state, xc_s, ref, wn, None, r).cpu().numpy())
        for fill in (0x00, 0xFF, 0x5A):                              # 0xFF: NaN in both dtypes
            eng._scratch.fill_(fill)
            assert _same(_both(eng.condition_variance_reduction_grad_block(state, xc_s, ref, wn, r)), base), fill
        if ref is not None:
            for cut in (64, 127):                                    # 130 = 64 + 66 = 127 + 3 over two calls
                eng._scratch.fill_(0xFF)
                a = _both(eng.condition_variance_reduction_grad_block(state, xc_s[:cut], ref, wn, r))
                b = _both(eng.condition_variance_reduction_grad_block(state, xc_s[cut:], ref, wn, r))
                assert np.array_equal(np.hstack([a[0], b[0]]), base[0]), cut
                assert np.array_equal(np.concatenate([a[1], b[1]], axis=1), base[1]), cut
        for chunk in (37, 128, 131):
            monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', chunk)
            eng._scratch.fill_(0x5A)
            assert _same(_both(eng.condition_variance_reduction_grad_block(state, xc_s, ref, wn, r)), base), chunk
        monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', 2048)
    # q_local = 1 against all components: an engine of its own holding component k alone
    base = _both(eng.condition_variance_reduction_grad_block(state, xc_s, xr_s, wn, r))
    xt, s, Y = _training(m)
    rows = eng._theta_last
    for k in range(len(rows)):
        solo = HotPathEngine(xt, Y, None if mode == 'full' else s, q_local=1, dtype=dtype, kernel=m.kernel)
        solo.evaluate(rows[k:k + 1])
        st = solo.condition_begin(xn_s, tt[k:k + 1], rr)
        got = _both(solo.condition_variance_reduction_grad_block(st, xc_s, xr_s, wn, r))
        assert np.array_equal(got[0][0], base[0][k]) and np.array_equal(got[1][0], base[1][k]), k


def test_two_ranks_reproduce_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_condition_vr_grad_gpu_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


# ---- the base model, the view and the workspace are only read -------------------------------------------------------------
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_base_model_view_and_workspace_untouched(mode):
    m, x = _model(mode, 'se', 6)
    xn, yn = _new_runs(m, x, 70, 10)
    r = 3 if mode == 'rep' else 1
    view = m.condition(xn, yn)
    xc, xr, x0 = _candidates(m, x, view, 130, 36), _points(x, 130, 37), _points(x, 130, 38)
    free = np.r_[0:70, 73:130]

    def queries():
        out = [t.numpy().copy() for t in m.predict(x0)]
        out.append(m.variance_reduction(xc, x_ref=xr, replicates=r, latent=True).numpy().copy())
        out += [t.numpy().copy() for t in m.variance_reduction_grad(xc, x_ref=xr, replicates=r, latent=True)]
        out += [t.numpy().copy() for t in m.select_batch(xc, 5, x_ref=xr, replicates=r, return_scores=True)]
        out += [t.numpy().copy() for t in view.predict(x0, latent=True)]
        out.append(view.variance_reduction(xc[free], x_ref=xr, replicates=r, latent=True).numpy().copy())
        out += [t.numpy().copy() for t in view.predict_grad(x0, latent=True)]
        return out
    before = queries()
    eng = m._ensure_aux()
    ck0 = _checksum(eng)
    R, dR = (t.numpy() for t in view.variance_reduction_grad(xc, x_ref=xr, replicates=r, latent=True))
    view.variance_reduction_grad(xc, replicates=r)
    view.variance_reduction_differentiable(torch.as_tensor(xc), x_ref=xr, replicates=r)
    assert _checksum(eng) == ck0 and m._ensure_aux() is eng
    after = queries()
    assert len(before) == len(after) == 16 and all(np.array_equal(a, b) for a, b in zip(before, after))
    # the new runs took variance away: the view's gradient is not the base model's
    assert np.max(np.abs(dR - before[5])) > 1e-6 * np.max(np.abs(before[5]))
    assert np.array_equal(R[:, free], before[11])


# ---- public API ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_public_api_gradcheck_staleness_and_the_continuous_surface(mode):
    m, x = _model(mode, 'matern32', 2)
    xn, yn = _new_runs(m, x, 5, 14)
    view = m.condition(xn, yn)
    r = 2 if mode == 'rep' else 1
    xc, xr = _points(x, 9, 41), _points(x, 7, 42)
    xc[3], xc[4] = _train_raw(m, x)[4], view.x_new.numpy()[1]           # new inputs like any other: no ValueError on either path
    w = np.arange(1.0, 8.0)
    gain, dgain = view.variance_reduction_grad(torch.as_tensor(xc), x_ref=torch.as_tensor(xr), weights=w, outputs=[0, 2], replicates=r)
    for t in (gain, dgain):
        assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.device.type == 'cpu' and not t.requires_grad
        assert torch.all(torch.isfinite(t))
    assert gain.shape == (2, 9) and dgain.shape == (2, 9, 2)
    R, dR = (t.numpy() for t in view.variance_reduction_grad(xc, x_ref=xr, weights=w, replicates=r, latent=True))
    assert R.shape == (3, 9) and dR.shape == (3, 9, 2)
    W, _, scale, _ = m._output_map()
    np.testing.assert_array_equal(gain.numpy(), (W[:, [0, 2]] ** 2).T @ R * (scale[[0, 2]] ** 2)[:, None])
    np.testing.assert_allclose(dgain.numpy(), np.einsum('ka,kcl->acl', W[:, [0, 2]] ** 2, dR) * (scale[[0, 2]] ** 2)[:, None, None],
                               rtol=1e-13)
    free = [0, 1, 2, 5, 6, 7, 8]
    assert np.array_equal(gain.numpy()[:, free],
                          view.variance_reduction(xc[free], x_ref=xr, weights=w, outputs=[0, 2], replicates=r).numpy())
    if mode == 'rep':
        with pytest.raises(ValueError, match='refit'):
            view.variance_reduction(xc, x_ref=xr, replicates=r)
    else:
        with pytest.raises(ValueError, match='replicates must be 1'):
            view.variance_reduction_grad(xc, replicates=2)
    with pytest.raises(ValueError, match='x_cand must have shape'):
        view.variance_reduction_grad(xc[:, :1])
    for dev in ('cpu', 'cuda:0'):
        xt = torch.tensor(xc[:4], dtype=torch.float64, device=dev, requires_grad=True)
        assert torch.autograd.gradcheck(lambda t: view.variance_reduction_differentiable(t, x_ref=xr, weights=w, replicates=r), (xt,),
                                        eps=1e-6, atol=1e-6, rtol=1e-4)
        out = view.variance_reduction_differentiable(xt, x_ref=xr, latent=True, replicates=r)
        assert out.device == xt.device and out.shape == (3, 4) and out.requires_grad
        with pytest.raises(RuntimeError, match='first derivatives only'):
            torch.autograd.grad(out.sum(), xt, create_graph=True)
        out = view.variance_reduction_differentiable(xt, x_ref=xr, latent=True, replicates=r)
        out.sum().backward()
        assert xt.grad.device == xt.device and xt.grad.shape == (4, 2)
    m._set_flat(m._get_flat() + 0.01)
    for call in (lambda: view.variance_reduction_grad(xc), lambda: view.variance_reduction_differentiable(torch.as_tensor(xc))):
        with pytest.raises(RuntimeError, match='stale'):
            call()
    m.predict(xc)
    with pytest.raises(RuntimeError, match='stale'):
        view.variance_reduction_grad(xc)
    assert m.condition(xn, yn).variance_reduction_grad(xc, replicates=r)[1].shape == (int(m.p), 9, 2)
