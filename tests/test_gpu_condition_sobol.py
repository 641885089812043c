"""Sobol indices and the integrated variance on a conditioned view on the GPU (lcgp_condition_sobol_matrix_pairs,
ConditionedLCGP.sobol_indices / integrated_variance): every matrix-weighted sum and S0 of the pass against the
float64 numpy restatement fed with Q' built from the engine's own A^-1 and L^-1 (fetch_matrix) and the state's U_n and L_S^-1,
with a scratch full of 0xFF; the view's C_u, IV and plug-in sums end to end against dense numpy on the augmented data, beside an
engine built on the augmented data; a float32 model; identities with the view's main_effects() and predict_marginal();
monotonicity against the base model; two ranks against one.

Bars.  Pass parity: |dev - ref| <= 1e-12 sum |Q'| (M_u + M_0) (S0: sum |Q'| M_0), the size of what a sum adds up, from the
reference.  End to end: |dev - ref| <= 1e-10 c prod_{l not in u} I2_l, the prior term of C_u (IV: c), and for the mean part 1e-10
sum |w_i| |w'_i'| (M_u + M_0), unless the host's own two ways to the inverse of the augmented matrix disagree by more than 1e-11 of
the prior term -- then ten times that disagreement (tests/test_gpu_sobol_uncertainty.py).  Every case prints its figures before it
asserts.  Largest ratios measured on an MI355X: see profiles/sobol_checks.txt."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lcgp_amd.engine import HotPathEngine
from tests import condition_marginal_ref as cmref
from tests import condition_sobol_ref as cref
from tests import sobol_ref as ref
from tests import sobol_uncertainty_ref as uref
from tests.test_condition_host import new_columns
from tests.test_gpu_condition import _new_runs, _training
from tests.test_gpu_sobol import _boxes, _free_port, _model

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PARITY_BAR = 1e-12
END_TO_END_BAR = 1e-10
HOST_AGREES_WITHIN = 1e-11
PLUG = ('first', 'total', 'variance', 'mean', 'first_variance', 'closed_variance')
NEW = ('expected_variance', 'expected_first_variance', 'expected_closed_variance', 'first_expected', 'total_expected',
       'integrated_variance')


def _consts(m):
    """(sr (n), c (q), D (q), theta rows (q, d + 3)) of the model at its constrained parameters"""
    n = int(m.n)
    sr = np.sqrt(m.r.numpy().astype(np.float64)) if m.submethod == 'rep' else np.ones(n)
    ell, scale, nug, D = m.lLmb.numpy(), m.lLmb0.numpy(), m.lnugGPs.numpy(), m.diag_D.numpy().astype(np.float64).reshape(-1)
    return sr, scale * (1.0 - nug / (1.0 + nug)), D, np.concatenate([ell, scale[:, None], nug[:, None], D[:, None]], axis=1)


def _state_parts(eng, state, k):
    """(U_n (m, n), L_S^-1 (m, m)) of local component k out of the view's float64 device state"""
    n, m, q = eng.n, state['m'], eng.q_local
    npad, mpad = -(-n // 128) * 128, -(-m // 128) * 128
    flat = state['state'].view(torch.float64)
    U = flat[:q * mpad * npad].view(q, mpad, npad)[k, :m, :n].cpu().numpy()
    off = -(-(q * mpad * npad * 8) // 256) * 256 // 8
    Wi = flat[off:off + q * mpad * mpad].view(q, mpad, mpad)[k, :m, :m].cpu().numpy()
    assert np.array_equal(Wi, np.tril(Wi))
    return U, Wi


def _q_prime_from_device(eng, state, k, sr, D, c):
    ainv = eng.fetch_matrix(2, k)
    assert np.array_equal(ainv, ainv.T)
    W = np.tril(eng.fetch_matrix(1, k))
    Un, lsinv = _state_parts(eng, state, k)
    return cref.q_prime(ainv, W.T @ Un.T, lsinv, sr, D, c)[0]


def _parity(m, view, what, boxes):
    """every sum and S0 of every component against the restatement fed with Q' from the device's own matrices; twice, the second
    time on a scratch full of 0xFF, bitwise; a subset of ks in another order, bitwise.  Returns the worst ratio"""
    eng, state = view._float64_state()
    sr, c, D, th = _consts(m)
    n, d, q, mn = int(m.n), int(m.d), int(m.q), view.m
    ell = m.lLmb.numpy()
    xa = np.vstack([np.asarray(m._x_train(), np.float64), m._standardise_x0(view.x_new.numpy())[0]])
    v = c[:, None] * np.concatenate([np.broadcast_to(sr, (q, n)), np.ones((q, mn))], axis=1)
    Qp = [_q_prime_from_device(eng, state, k, sr, D[k], c[k]) for k in range(q)]
    worst = 0.0
    for box in boxes:
        first, first0 = eng.condition_sobol_matrix_sums(state, v, ell, box, np.arange(q))      # (allocates the scratch)
        eng._scratch.fill_(0xFF)                                                                 # every double a NaN
        sums, s0 = eng.condition_sobol_matrix_sums(state, v, ell, box, np.arange(q))
        assert sums.shape == (q, 2 * d + 1) and s0.shape == (q,) and np.all(np.isfinite(sums)) and np.all(np.isfinite(s0))
        assert np.array_equal(first, sums) and np.array_equal(first0, s0)
        for k in range(q):
            want, want0, size, size0 = uref.matrix_sums(m.kernel, xa, ell[k], box, Qp[k])
            ratio = max(np.max(np.abs(sums[k] - want) / size), abs(s0[k] - want0) / size0)
            print('view matrix sums', what, 'sub-box' if box[0][0] > 0 else 'default', k, 'ratio', ratio)
            worst = max(worst, ratio)
            assert np.all(np.abs(sums[k] - want) <= PARITY_BAR * size), (what, k, np.abs(sums[k] - want) / size)
            assert abs(s0[k] - want0) <= PARITY_BAR * size0, (what, k, abs(s0[k] - want0) / size0)
        if q > 1:
            eng._scratch.fill_(0x5A)
            part, part0 = eng.condition_sobol_matrix_sums(state, v, ell, box, [q - 1, 0])
            assert np.array_equal(part, sums[[q - 1, 0]]) and np.array_equal(part0, s0[[q - 1, 0]])
    print('view matrix sums', what, 'worst ratio', worst)
    return worst


@pytest.mark.parametrize('mode', ['full', 'rep'])
@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_pass_against_numpy(kernel, mode):
    """the base model of tests/test_gpu_sobol.py (n = 150, d = 3, p = 6, q = 3).  m = 1: N = 151, the new input alone in the last
    ragged tile's 23rd row.  m = 70: N = 220, four tiles a side, the boundary n = 150 inside tile 2 and inside its diagonal tile
    (rep: replicated rows in x_new, counts above 1)"""
    m, x = _model(mode, kernel, 3)
    x = np.asarray(x)
    for mn, boxes in ((1, _boxes(3)[:1]), (70, _boxes(3)[1:])):
        xn, yn = _new_runs(m, x, mn, 3)
        view = m.condition(xn, yn)
        assert view.m == mn
        _parity(m, view, '%s %s m=%d' % (kernel, mode, mn), boxes)


def test_pass_with_the_boundary_on_a_tile_edge():
    """n = 128, m = 64: three full tiles a side, nothing ragged, the boundary between tiles 1 and 2"""
    m, x = _model('full', 'matern32', 3, n=128)
    xn, yn = _new_runs(m, np.asarray(x), 64, 5)
    _parity(m, m.condition(xn, yn), 'n=128 m=64', _boxes(3))


def test_pass_with_more_new_inputs_than_training_inputs():
    """n = 70, m = 150 (mpad = 256 where every other case has 128; npad = 128): the rows of P and the k loop of E are longer than
    the training block, N = 220"""
    m, x = _model('rep', 'se', 3, n=70, p=3, q=2)
    xn, yn = _new_runs(m, np.asarray(x), 150, 6)
    _parity(m, m.condition(xn, yn), 'n=70 m=150', _boxes(3)[:1])


@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
@pytest.mark.parametrize('d', [11, 18])
def test_pass_in_more_dimensions(kernel, d):
    """d = 11: the 16-wide instance; d = 18: the kernel that recomputes.  n = 70, m = 20 (N = 90: two tiles a side, the boundary
    inside the second one), q = 2"""
    m, x = _model('full', kernel, d, n=70, p=4, q=2)
    xn, yn = _new_runs(m, np.asarray(x), 20, 4)
    _parity(m, m.condition(xn, yn), '%s d=%d' % (kernel, d), _boxes(d)[:1])


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(mode, kernel, dtype='float64'):
    """model (n = 150, d = 3, q = 3), its view on 70 new inputs, and the dense float64 numpy route on the augmented data at the
    theta rows of the float64 factorisation: per component uref.component by a Cholesky solve and by an explicit inverse, the
    weights c sa z, and per pair k <= k' the pair sums with their sizes.  Computed once per case and shared, never changed"""
    m, x = _model(mode, kernel, 3, dtype=dtype)
    xn, yn = _new_runs(m, np.asarray(x), 70, 3)
    view = m.condition(xn, yn)
    eng64 = m._ensure_aux64()
    rows = np.asarray(eng64._theta_last, np.float64).copy()
    xt, s, Y = _training(m)
    xn_s, snew, ycol = new_columns(m, xn, yn)
    bs = m._marginal_box(None)
    d, q = 3, int(m.q)
    comp, w = [], []
    for th in rows:
        xa, sa, _, za = cmref.augmented(th, xt, s, Y, kernel, xn_s, snew, ycol)
        by_solve, by_inverse, _ = uref.dense_ainv(kernel, xa, sa, th)
        comp.append(tuple(uref.component(kernel, xa, sa, th, inv, bs) for inv in (by_solve, by_inverse)))
        w.append(th[d] * (1.0 - th[d + 1] / (1.0 + th[d + 1])) * sa * za)
    pairs = {(k, kp): ref.pair_sums(kernel, xa, w[k], rows[k][:d], w[kp], rows[kp][:d], bs) for k in range(q) for kp in range(k, q)}
    return dict(m=m, view=view, x=np.asarray(x), xn=xn, yn=yn, rows=rows, xa=xa, sa=sa, comp=comp, w=np.stack(w), pairs=pairs, bs=bs,
                new=(xn_s, snew, ycol), training=(xt, s, Y))


def _bar(a, b):
    host = max(np.max(np.abs(a['C'] - b['C']) / a['prior']), abs(a['IV'] - b['IV']) / a['c'])
    return (END_TO_END_BAR if host <= HOST_AGREES_WITHIN else 10.0 * host), host


def _augmented_engine(case):
    """an engine on the augmented data at the same theta rows, evaluated: the route without the view's queries"""
    m = case['m']
    xt, s, Y = case['training']
    xn_s, snew, ycol = case['new']
    aug = HotPathEngine(np.vstack([xt, xn_s]), np.hstack([Y, ycol]), None if m.submethod == 'full' else np.r_[s, snew],
                        q_local=len(case['rows']), kernel=m.kernel)
    aug.evaluate(case['rows'])
    return aug


def _augmented_results(case, latent):
    """(SobolIndices, C, IV) of the augmented engine through the model's own host arithmetic"""
    m, aug, xa, sa, bs = case['m'], _augmented_engine(case), case['xa'], case['sa'], case['bs']
    q = int(m.q)
    sr, c, D, th = _consts(m)
    z = np.stack([aug.fetch_vector(1, k) for k in range(q)])
    w = c[:, None] * sa[None, :] * z

    def local_sums(loc, c_, Dk, sr_, ell):
        v = (c_[loc] * np.sqrt(Dk[loc]))[:, None] * sa[None, :]
        return aug.sobol_matrix_sums(xa, v, ell[loc], bs, np.arange(len(loc)))

    V, mean = m._sobol_mean(aug, xa, w, bs, latent)
    mat = m._sobol_matrix(bs, aug, local_sums)
    rows = list(range(q if latent else int(m.p)))
    return m._sobol_result(V, mean, rows, latent, lambda: mat), mat[0], mat[1]


@pytest.mark.parametrize('mode', ['full', 'rep'])
@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_view_against_dense_numpy_on_the_augmented_data(kernel, mode):
    case = _case(mode, kernel)
    m, view, bs = case['m'], case['view'], case['bs']
    d, q = 3, int(m.q)
    Cv, IVv, _ = view._sobol_matrix(bs, *view._float64_state())
    assert np.array_equal(view.integrated_variance(latent=True).numpy(), IVv)
    lat = view.sobol_indices(latent=True)
    _, Ca, IVa = _augmented_results(case, True)
    worst = dict(view=0.0, aug=0.0, host=0.0, mean=0.0)
    for k in range(q):
        a, b = case['comp'][k]
        bar, host = _bar(a, b)
        rv = max(np.max(np.abs(Cv[k] - a['C']) / a['prior']), abs(IVv[k] - a['IV']) / a['c'])
        ra = max(np.max(np.abs(Ca[k] - a['C']) / a['prior']), abs(IVa[k] - a['IV']) / a['c'])
        Dk, means, size = case['pairs'][(k, k)]
        got = np.r_[lat.first_variance.numpy()[k], lat.closed_variance.numpy()[k], lat.variance.numpy()[k]]
        rm = max(np.max(np.abs(got - Dk) / size), abs(lat.mean.numpy()[k] - means[0]) / np.sum(np.abs(case['w'][k])))
        print('view end to end', kernel, mode, k, 'view', rv, 'augmented engine', ra, 'host, two ways', host, 'bar', bar, 'mean part', rm)
        for name, r in (('view', rv), ('aug', ra), ('host', host), ('mean', rm)):
            worst[name] = max(worst[name], r)
        assert np.all(np.abs(Cv[k] - a['C']) <= bar * a['prior']), (k, np.abs(Cv[k] - a['C']) / a['prior'])
        assert abs(IVv[k] - a['IV']) <= bar * a['c'], (k, abs(IVv[k] - a['IV']) / a['c'])
        assert np.all(np.abs(got - Dk) <= bar * size), (k, np.abs(got - Dk) / size)
        assert abs(lat.mean.numpy()[k] - means[0]) <= bar * np.sum(np.abs(case['w'][k]))
        assert np.all(Cv[k] >= -1e-12 * a['c']) and np.all(Cv[k][:2 * d] <= Cv[k][2 * d] + 1e-12 * a['c'])
    print('view end to end', kernel, mode, 'worst', worst)


def _field_bars(case, latent):
    """per field of SobolIndices(uncertainty=True) the absolute bar 1e-10 x the size of what the field adds up, from the dense
    reference: V_u: scale_a^2 sum_kk' |W_ka| |W_k'a| size[k, k']; E[V_u]: that plus scale_a^2 sum_k W_ka^2 prior_u[k]; IV: scale_a^2
    sum_k W_ka^2 c_k; mean: |offset_a| + scale_a sum_k |W_ka| sum |w_k|; an index N / Dn: (bar_N + |index| bar_Dn) / Dn"""
    m = case['m']
    d, q = 3, int(m.q)
    size = np.zeros((q, q, 2 * d + 1))
    for (k, kp), (_, _, sz) in case['pairs'].items():
        size[k, kp] = size[kp, k] = sz
    prior = np.stack([case['comp'][k][0]['prior'] for k in range(q)])
    cc = np.array([case['comp'][k][0]['c'] for k in range(q)])
    wabs = np.sum(np.abs(case['w']), axis=1)
    if latent:
        sv, sp, sc, sm = size[np.arange(q), np.arange(q)], prior, cc, wabs
    else:
        W, _, scale, offset = m._output_map()
        sv = np.einsum('ka,la,klu->au', np.abs(W), np.abs(W), size) * (scale ** 2)[:, None]
        sp = ((W ** 2).T @ prior) * (scale ** 2)[:, None]
        sc = ((W ** 2).T @ cc) * scale ** 2
        sm = np.abs(offset) + np.abs(scale) * (np.abs(W).T @ wabs)
    host = max(_bar(*case['comp'][k])[0] for k in range(q))
    return host * sv, host * (sv + sp), host * sc, host * sm


@pytest.mark.parametrize('latent', [False, True])
@pytest.mark.parametrize('mode,kernel', [('full', 'matern32'), ('rep', 'se'), ('full', 'matern52')])
def test_every_field_against_a_model_on_the_augmented_data(mode, kernel, latent):
    """every field of sobol_indices(uncertainty=True) of the view against the same fields assembled, by the model's own host
    arithmetic at the same parameters, basis and standardisation, from an engine built and evaluated on the augmented data"""
    case = _case(mode, kernel)
    view = case['view']
    d = 3
    got = view.sobol_indices(latent=latent, uncertainty=True)
    want, _, _ = _augmented_results(case, latent)
    bv, be, bi, bm = _field_bars(case, latent)
    g = {name: getattr(got, name).numpy() for name in PLUG + NEW}
    w = {name: getattr(want, name).numpy() for name in PLUG + NEW}
    checks = [('first_variance', bv[:, :d]), ('closed_variance', bv[:, d:2 * d]), ('variance', bv[:, 2 * d]), ('mean', bm),
              ('expected_first_variance', be[:, :d]), ('expected_closed_variance', be[:, d:2 * d]),
              ('expected_variance', be[:, 2 * d]), ('integrated_variance', bi)]
    V, EV = w['variance'][:, None], w['expected_variance'][:, None]
    checks += [('first', (bv[:, :d] + np.abs(w['first']) * bv[:, 2 * d:]) / V),
               ('total', (bv[:, d:2 * d] + np.abs(1.0 - w['total']) * bv[:, 2 * d:]) / V),
               ('first_expected', (be[:, :d] + np.abs(w['first_expected']) * be[:, 2 * d:]) / EV),
               ('total_expected', (be[:, d:2 * d] + np.abs(1.0 - w['total_expected']) * be[:, 2 * d:]) / EV)]
    for name, bar in checks:
        ratio = np.max(np.abs(g[name] - w[name]) / bar)
        print('view against augmented model', mode, kernel, 'latent' if latent else 'outputs', name, 'ratio of the bar', ratio)
        assert g[name].shape == w[name].shape and np.all(np.abs(g[name] - w[name]) <= bar), (name, ratio)


def test_float32_model_against_the_float64_models_view():
    """a float32 model: its view lives on the float32 engine, the Sobol queries on a float64 companion state built from the stored
    outputs and counts.  The parameters are those of the float64 model, so the difference is that of the companion state: the
    end-to-end bar, against the same dense reference"""
    c32, c64 = _case('rep', 'matern52', 'float32'), _case('rep', 'matern52')
    v32, v64 = c32['view'], c64['view']
    assert not v32._float64 and v64._float64 and v32._engine.dtype_name == 'float32'
    d, q = 3, 3
    a, b = v32.sobol_indices(latent=True, uncertainty=True), v64.sobol_indices(latent=True, uncertainty=True)
    assert v32._companion is not None and v32._float64_state()[0].dtype_name == 'float64'
    np.testing.assert_allclose(c32['rows'], c64['rows'], rtol=1e-14, atol=0)
    for k in range(q):
        ref_a, ref_b = c64['comp'][k]
        bar, _ = _bar(ref_a, ref_b)
        size = c64['pairs'][(k, k)][2]
        for name, sl in (('first_variance', slice(0, d)), ('closed_variance', slice(d, 2 * d)), ('variance', 2 * d)):
            dv = np.abs(getattr(a, name).numpy()[k] - getattr(b, name).numpy()[k])
            de = np.abs(getattr(a, 'expected_' + name).numpy()[k] - getattr(b, 'expected_' + name).numpy()[k])
            print('float32 view', k, name, np.max(dv / size[sl]), np.max(de / (size[sl] + ref_a['prior'][sl])))
            assert np.all(dv <= bar * size[sl]) and np.all(de <= bar * (size[sl] + ref_a['prior'][sl])), (k, name)
        div = abs(a.integrated_variance.numpy()[k] - b.integrated_variance.numpy()[k])
        print('float32 view', k, 'IV', div / ref_a['c'])
        assert div <= bar * ref_a['c']
    np.testing.assert_array_equal(v32.integrated_variance(latent=True).numpy(), a.integrated_variance.numpy())


@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_identities_on_the_view(kernel):
    case = _case('full', kernel)
    m, view, bs = case['m'], case['view'], case['bs']
    d, p = 3, int(m.p)
    base_before = m.sobol_indices(uncertainty=True)
    s0 = view.sobol_indices()
    s = view.sobol_indices(uncertainty=True)
    for name in PLUG:
        assert np.array_equal(getattr(s, name).numpy(), getattr(s0, name).numpy()), name
    for name in NEW:
        assert getattr(s0, name) is None, name
    V, ev, iv = s.variance.numpy(), s.expected_variance.numpy(), s.integrated_variance.numpy()
    assert s.expected_first_variance.shape == (p, d) and ev.shape == (p,) and iv.shape == (p,)
    assert np.array_equal(view.integrated_variance().numpy(), iv)
    assert np.array_equal(view.integrated_variance(outputs=[4, 1]).numpy(), iv[[4, 1]])
    # IV - (E[V] - V) is the variance of the box mean; .mean is the box mean; V_l is the variance of the main effect's curve
    me = view.main_effects(grid=2)
    ov = me.overall_var.numpy()
    print('view overall_var', kernel, np.max(np.abs(iv - (ev - V) - ov) / ov))
    assert np.all(np.abs(iv - (ev - V) - ov) <= 1e-10 * ov)
    overall = view.main_effects().overall.numpy()
    print('view mean against main_effects', kernel, np.max(np.abs(s.mean.numpy() - overall) / V))
    assert np.all(np.abs(s.mean.numpy() - overall) <= 1e-10 * V)
    # (as tests/test_gpu_sobol.py for the model: piecewise Gauss-Legendre, 8 nodes per piece, split at the coordinates of the
    # training inputs and of the view's inputs; both within 1e-10 of V)
    xt = np.asarray(case['x'])
    lo, hi = xt.min(axis=0), xt.max(axis=0)
    for l in range(d):
        t, wt = ref.piecewise_gauss_legendre(8, lo[l], hi[l], np.r_[xt[:, l], case['xn'][:, l]])
        x0 = np.full((len(t), d), np.nan)
        x0[:, l] = t
        curve = view.predict_marginal(x0, [j for j in range(d) if j != l])[0].numpy()
        vl = ((curve - (curve @ wt)[:, None]) ** 2) @ wt
        got = s.first_variance.numpy()[:, l]
        print('view V_l against the marginal curve', kernel, l, np.max(np.abs(got - vl) / V))
        assert np.all(np.abs(got - vl) <= 1e-10 * V)
    # conditioning cannot add uncertainty, per component; C_u >= 0
    Cb, ivb, ovb = m._sobol_matrix(bs)
    Cv, ivv, ovv = view._sobol_matrix(bs, *view._float64_state())
    _, c, _, _ = _consts(m)
    tol = 1e-12 * c
    assert np.all(ivv <= ivb + tol) and np.all(ovv <= ovb + tol)
    assert np.all(Cv <= Cb + tol[:, None]) and np.all(Cv >= -tol[:, None])
    # the base model's own answers are bitwise what they were
    base_after = m.sobol_indices(uncertainty=True)
    for name in PLUG + NEW:
        assert np.array_equal(getattr(base_before, name).numpy(), getattr(base_after, name).numpy()), name


@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_a_single_input_explains_everything(kernel):
    m, x = _model('full', kernel, 1, n=50, p=3, q=2)
    xn, yn = _new_runs(m, np.asarray(x), 7, 3)
    s = m.condition(xn, yn).sobol_indices(uncertainty=True)
    for name in ('first', 'total', 'first_expected', 'total_expected'):
        np.testing.assert_allclose(getattr(s, name).numpy(), 1.0, rtol=0, atol=1e-12, err_msg=name)


def test_stale_view_raises():
    m, x = _model('full', 'matern32', 3, n=70, p=3, q=2)
    xn, yn = _new_runs(m, np.asarray(x), 5, 3)
    view = m.condition(xn, yn)
    view.integrated_variance()
    m._set_flat(m._get_flat() + 0.01)
    with pytest.raises(RuntimeError, match='stale'):
        view.integrated_variance()
    with pytest.raises(RuntimeError, match='stale'):
        view.sobol_indices(uncertainty=True)


def test_two_ranks_equal_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_condition_sobol_gpu_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout
