"""Closed variances of arbitrary input subsets on the GPU (lcgp_sobol_subset_pairs, lcgp_sobol_matrix_subset_pairs,
lcgp_condition_sobol_matrix_subset_pairs; LCGP.sobol_subsets, sobol_indices(order=2), shapley_effects): every D_u
against the float64 numpy restatement of tests/sobol_subset_ref.py with a scratch full of 0xFF, at d = 3 (all 8 masks), d = 6 (all
64 masks and more: several chunks) and d = 11 (the 16-wide instance); the matrix-weighted sums against the restatement fed with
the engine's own A^-1; V^c_{01} end to end against a tensor rule over predict_marginal; the d = 2 identities; a conditioned view
against an engine on the augmented data; determinism; two ranks against one.

Bars (the project's own).  Parity: |dev - ref| <= 1e-12 sum |w_i| |w'_i'| (M_u + M_0) (matrix-weighted:
sum |Q| (M_u + M_0)), the size of what a sum adds up, from the reference.  End to end: 1e-10 V.  Every case prints its figures
before it asserts.  Largest ratios measured on an MI355X: see profiles/sobol_checks.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import sobol_ref as ref
from tests import sobol_subset_ref as sref
from tests.test_gpu_sobol import _boxes, _free_port, _model, _weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PARITY_BAR = 1e-12
END_TO_END_BAR = 1e-10


def _chunk(d):
    from lcgp_amd import _hip
    return _hip.load().lcgp_sobol_subset_chunk(d)


def _parity(m, masks, what, boxes, alone=()):
    """every D_u of every pair k <= k' against the restatement, twice, the second time on a scratch full of 0xFF, bitwise; the
    classical masks among `masks` (the last 2 d + 1) against sobol_pairs' columns; the masks at the positions `alone` asked
    alone, bitwise.  Returns the worst ratio"""
    eng, x, w, ell = _weights(m)
    q, d = w.shape[0], x.shape[1]
    pairs = np.array([(k, kp) for k in range(q) for kp in range(k, q)])
    masks = np.asarray(masks, np.uint64)
    ncl = 2 * d + 1
    assert [int(s) for s in masks[-ncl:]] == sref.classical_masks(d)
    worst = 0.0
    for box in boxes:
        first, _ = eng.sobol_subset_pairs(x, w, ell, box, pairs, masks)          # (allocates the scratch)
        eng._scratch.fill_(0xFF)                                                 # every double a NaN
        D, means = eng.sobol_subset_pairs(x, w, ell, box, pairs, masks)
        assert D.shape == (len(pairs), len(masks)) and np.all(np.isfinite(D)) and np.all(np.isfinite(means))
        assert np.array_equal(first, D)
        assert np.all(D[:, masks == 0] == 0.0)
        classical, cmeans = eng.sobol_pairs(x, w, ell, box, pairs)
        for r, (k, kp) in enumerate(pairs):
            want, mm, size = sref.subset_pair_sums(m.kernel, x, w[k], ell[k], w[kp], ell[kp], box, masks)
            ratio = np.max(np.abs(D[r] - want) / size)
            rc = np.max(np.abs(D[r, -ncl:] - classical[r]) / size[-ncl:])
            print('subset sums', what, 'sub-box' if box[0][0] > 0 else 'default', (int(k), int(kp)), 'ratio', ratio,
                  'against sobol_pairs', rc)
            worst = max(worst, ratio, rc)
            assert np.all(np.abs(D[r] - want) <= PARITY_BAR * size), (what, k, kp, np.abs(D[r] - want) / size)
            assert np.all(np.abs(D[r, -ncl:] - classical[r]) <= PARITY_BAR * size[-ncl:]), (what, k, kp)
            assert means[r] == cmeans[r]
            if k == kp:
                assert abs(means[r] - mm[0]) <= PARITY_BAR * np.sum(np.abs(w[k])), (what, k)
        for s in alone:                          # a mask's sum depends neither on the other masks nor on its place
            eng._scratch.fill_(0x5A)
            one, _ = eng.sobol_subset_pairs(x, w, ell, box, pairs, masks[s:s + 1])
            assert np.array_equal(one[:, 0], D[:, s]), (what, s)
    print('subset sums', what, 'worst ratio', worst)
    return worst


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('mode', ['full', 'rep'])
@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_subset_sums_against_numpy(kernel, mode, dtype):
    """n = 150 (three ragged tiles a side), d = 3, q = 3: six pairs, all 8 masks (then the classical ones again, in
    lcgp_sobol_pairs' order), two boxes.  A float32 model hands over the weights of its float64 engine"""
    m, _ = _model(mode, kernel, 3, dtype=dtype)
    masks = list(range(8)) + sref.classical_masks(3)
    _parity(m, masks, '%s %s %s' % (kernel, mode, dtype), _boxes(3), alone=(5,))


@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
@pytest.mark.parametrize('d', [6, 11])
def test_subset_sums_over_several_chunks_and_in_more_dimensions(kernel, d):
    """n = 70 (two tiles a side, the second one ragged), q = 2.  d = 11: the 16-wide instance, 40 random masks and the 23
    classical ones: two chunks.  d = 6: all 64 masks, 40 random ones (repeats among them) and the 13 classical ones: four
    chunks, the last one ragged.  Five picked masks, from every chunk, asked alone equal their value from the big call"""
    m, _ = _model('full', kernel, d, n=70, p=4, q=2)
    rng = np.random.default_rng(100 + d)
    masks = [int(s) for s in rng.integers(0, 1 << d, 40)] + sref.classical_masks(d)
    if d == 6:
        masks = list(range(64)) + masks
        assert 64 > _chunk(6)
    assert len(masks) > _chunk(d)
    alone = (0, 7, _chunk(d) - 1, _chunk(d), len(masks) - 2)
    _parity(m, masks, '%s d=%d' % (kernel, d), _boxes(d), alone=alone)


@pytest.mark.parametrize('mode', ['full', 'rep'])
@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_matrix_weighted_subset_sums_against_numpy(kernel, mode):
    """d = 3, n = 150, all 8 masks: sum Q (M_u - M_0) of every component against the restatement fed with the engine's own A^-1
    (fetch_matrix(2, k)); C_u >= -1e-12 of its prior term; E[V^c_u] monotone under inclusion; the full mask reproduces
    sobol_indices(uncertainty=True).expected_variance within 1e-10 V"""
    from tests.test_gpu_sobol_uncertainty import _rows
    m, _ = _model(mode, kernel, 3)
    eng, x, v, ell, sr, th = _rows(m)
    q, d = 3, 3
    masks = np.arange(8, dtype=np.uint64)
    ainv = [eng.fetch_matrix(2, k) for k in range(q)]
    worst = 0.0
    for box in _boxes(d):
        first = eng.sobol_matrix_subset_sums(x, v, ell, box, np.arange(q), masks)
        eng._scratch.fill_(0xFF)
        sums = eng.sobol_matrix_subset_sums(x, v, ell, box, np.arange(q), masks)
        assert sums.shape == (q, 8) and np.all(np.isfinite(sums)) and np.array_equal(first, sums) and np.all(sums[:, 0] == 0.0)
        classical, _ = eng.sobol_matrix_sums(x, v, ell, box, np.arange(q))
        for k in range(q):
            want, size = sref.subset_matrix_sums(m.kernel, x, ell[k], box, v[k][:, None] * v[k][None, :] * ainv[k], masks)
            ratio = np.max(np.abs(sums[k] - want) / size)
            cl = [int(s) for s in sref.classical_masks(d)]
            rc = np.max(np.abs(sums[k][cl] - classical[k]) / size[cl])
            print('matrix subset sums', kernel, mode, 'sub-box' if box[0][0] > 0 else 'default', k, 'ratio', ratio,
                  'against sobol_matrix_sums', rc)
            worst = max(worst, ratio, rc)
            assert np.all(np.abs(sums[k] - want) <= PARITY_BAR * size), (k, np.abs(sums[k] - want) / size)
            assert np.all(np.abs(sums[k][cl] - classical[k]) <= PARITY_BAR * size[cl]), k
        part = eng.sobol_matrix_subset_sums(x, v, ell, box, [q - 1, 0], masks[[6, 1]])
        assert np.array_equal(part, sums[[q - 1, 0]][:, [6, 1]])
    print('matrix subset sums', kernel, mode, 'worst ratio', worst)
    bs = m._marginal_box(None)
    C = m._sobol_subset_matrix(bs, masks)
    c = th[:, d] * (1.0 - th[:, d + 1] / (1.0 + th[:, d + 1]))
    for k in range(q):
        P, _ = sref.prior_products(m.kernel, ell[k], bs, masks)
        print('C_u over its prior term, smallest over the masks but the empty one', kernel, mode, k, np.min((C[k] / (c[k] * P))[1:]))
        assert np.all(C[k] >= -1e-12 * c[k] * P), (k, C[k] / (c[k] * P))
    allsets = [tuple(l for l in range(d) if (s >> l) & 1) for s in range(8)]
    for latent in (True, False):
        s = m.sobol_subsets(allsets, latent=latent, uncertainty=True)
        base = m.sobol_indices(latent=latent, uncertainty=True)
        E, V, EV = s.expected_closed_variance.numpy(), base.variance.numpy(), base.expected_variance.numpy()
        gap = min(np.min((E[:, t] - E[:, u]) / V) for u in range(8) for t in range(8) if u & t == u and u != t)
        rel = np.max(np.abs(E[:, 7] - EV) / V)
        print('E[V^c_u] under inclusion', kernel, mode, latent, 'smallest gain / V', gap, 'full mask against expected_variance', rel)
        assert gap >= -END_TO_END_BAR
        assert rel <= END_TO_END_BAR and np.max(np.abs(s.expected_variance.numpy() - EV) / V) <= END_TO_END_BAR
        assert np.max(np.abs(s.variance.numpy() - V) / V) <= END_TO_END_BAR


def test_closed_variance_of_a_pair_against_tensor_quadrature_of_predict_marginal():
    """d = 3, n = 40, Matern-3/2: V^c_{01} against the variance of predict_marginal(x0, [2]) -- the surface with input 2
    integrated out, which enters no pair integral -- over the tensor piecewise rule in inputs 0 and 1 (6 nodes per piece, pieces
    split at the training coordinates).  Within 1e-10 V"""
    m, x = _model('full', 'matern32', 3, n=40, p=4, q=2)
    s = m.sobol_subsets([(0, 1)])
    xn = np.asarray(x)
    lo, hi = xn.min(axis=0), xn.max(axis=0)
    rules = [ref.piecewise_gauss_legendre(6, lo[l], hi[l], xn[:, l]) for l in range(2)]
    g0, g1 = np.meshgrid(rules[0][0], rules[1][0], indexing='ij')
    x0 = np.stack([g0.reshape(-1), g1.reshape(-1), np.full(g0.size, np.nan)], axis=1)
    f = m.predict_marginal(x0, [2])[0].numpy().reshape(4, len(rules[0][0]), len(rules[1][0]))
    w0, w1 = rules[0][1], rules[1][1]
    mean = np.einsum('i,aij,j->a', w0, f, w1)
    V01 = np.einsum('i,aij,j->a', w0, (f - mean[:, None, None]) ** 2, w1)
    V = s.variance.numpy()
    print('V^c_01 against the tensor rule over predict_marginal', np.abs(s.closed_variance.numpy()[:, 0] - V01) / V,
          'mean', np.abs(s.mean.numpy() - mean) / V)
    assert np.all(V > 0.0) and np.all(V01 < V)
    assert np.all(np.abs(s.closed_variance.numpy()[:, 0] - V01) <= END_TO_END_BAR * V)
    assert np.all(np.abs(s.mean.numpy() - mean) <= END_TO_END_BAR * V)


@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_two_inputs_share_their_one_interaction(kernel):
    """d = 2: second[0, 1] = 1 - first_0 - first_1, and the Shapley effect of an input is V_l plus half the interaction"""
    m, _ = _model('full', kernel, 2, n=70, p=4, q=2)
    s = m.sobol_indices(order=2, uncertainty=True)
    sh = m.shapley_effects(uncertainty=True)
    first, second, V = s.first.numpy(), s.second.numpy(), s.variance.numpy()
    print('d = 2', kernel, 'second - (1 - first_0 - first_1)', np.max(np.abs(second[:, 0, 1] - (1.0 - first[:, 0] - first[:, 1]))))
    assert np.all(np.abs(second[:, 0, 1] - (1.0 - first[:, 0] - first[:, 1])) <= END_TO_END_BAR)
    assert np.array_equal(second[:, 0, 1], second[:, 1, 0]) and np.all(np.isnan(second[:, [0, 1], [0, 1]]))
    for l in range(2):
        want = s.first_variance.numpy()[:, l] + 0.5 * s.second_variance.numpy()[:, 0, 1]
        print('d = 2', kernel, 'Shapley effect', l, np.max(np.abs(sh.effects.numpy()[:, l] - want) / V))
        assert np.all(np.abs(sh.effects.numpy()[:, l] - want) <= END_TO_END_BAR * V)
        want = s.expected_first_variance.numpy()[:, l] + 0.5 * s.expected_second_variance.numpy()[:, 0, 1]
        assert np.all(np.abs(sh.effects_expected.numpy()[:, l] - want) <= END_TO_END_BAR * V)
    assert np.all(np.abs(sh.effects.numpy().sum(axis=1) - V) <= END_TO_END_BAR * V)
    assert np.all(np.abs(sh.effects_expected.numpy().sum(axis=1) - s.expected_variance.numpy()) <= END_TO_END_BAR * V)
    assert np.all(sh.effects.numpy() >= s.first_variance.numpy() - END_TO_END_BAR * V[:, None])
    assert np.all(sh.effects.numpy() <= V[:, None] * s.total.numpy() + END_TO_END_BAR * V[:, None])


@pytest.mark.parametrize('mode,kernel', [('full', 'matern32'), ('rep', 'se'), ('full', 'matern52')])
def test_view_against_a_model_on_the_augmented_data(mode, kernel):
    """a view with m = 20 new runs: sobol_subsets(uncertainty=True) and shapley_effects() against the same host arithmetic on
    an engine built and evaluated on the augmented data at the same parameters, within 1e-10 V"""
    from lcgp_amd.engine import HotPathEngine
    from tests import condition_marginal_ref as cmref
    from tests.test_condition_host import new_columns
    from tests.test_gpu_condition import _new_runs, _training
    m, x = _model(mode, kernel, 3)
    xn, yn = _new_runs(m, np.asarray(x), 20, 3)
    view = m.condition(xn, yn)
    rows = np.asarray(m._ensure_aux64()._theta_last, np.float64).copy()
    xt, s, Y = _training(m)
    xn_s, snew, ycol = new_columns(m, xn, yn)
    xa, sa, _, _ = cmref.augmented(rows[0], xt, s, Y, kernel, xn_s, snew, ycol)
    aug = HotPathEngine(np.vstack([xt, xn_s]), np.hstack([Y, ycol]), None if mode == 'full' else np.r_[s, snew], q_local=len(rows),
                        kernel=m.kernel)
    aug.evaluate(rows)
    q, d = int(m.q), 3
    bs = m._marginal_box(None)
    scale, nug = m.lLmb0.numpy(), m.lnugGPs.numpy()
    c = scale * (1.0 - nug / (1.0 + nug))
    w = c[:, None] * sa[None, :] * np.stack([aug.fetch_vector(1, k) for k in range(q)])

    def matrix(masks):
        def local_sums(loc, c_, Dk, sr_, ell):
            return aug.sobol_matrix_subset_sums(xa, (c_[loc] * np.sqrt(Dk[loc]))[:, None] * sa[None, :], ell[loc], bs, np.arange(len(loc)), masks)
        return m._sobol_subset_matrix(bs, masks, aug, local_sums)

    ctx = (aug, xa, w, bs, matrix)
    subsets = [(0,), (0, 1), (), (1, 2), (0, 1, 2), (2,)]
    rows_all = list(range(int(m.p)))
    want = m._sobol_subsets_result(ctx, *m._subset_masks(subsets), rows_all, False, True)
    got = view.sobol_subsets(subsets, uncertainty=True)
    V = want.variance.numpy()
    assert np.all(V > 0.0) and got.subsets == want.subsets
    for name in ('closed_variance', 'variance', 'expected_closed_variance', 'expected_variance'):
        g, t = getattr(got, name).numpy(), getattr(want, name).numpy()
        ratio = np.max(np.abs(g - t) / (V if g.ndim == 1 else V[:, None]))
        print('view against augmented model', mode, kernel, name, 'ratio', ratio)
        assert g.shape == t.shape and ratio <= END_TO_END_BAR, name
    assert np.all(got.closed_variance.numpy()[:, 2] == 0.0)
    # the view has learnt something: its closed variances are not the base model's
    assert not np.allclose(got.closed_variance.numpy(), m.sobol_subsets(subsets).closed_variance.numpy(), rtol=1e-6)
    sh_want = m._shapley_result(ctx, rows_all, False, True)
    sh = view.shapley_effects(uncertainty=True)
    for name in ('effects', 'effects_expected', 'variance', 'expected_variance'):
        g, t = getattr(sh, name).numpy(), getattr(sh_want, name).numpy()
        ratio = np.max(np.abs(g - t) / (V if g.ndim == 1 else V[:, None]))
        print('view against augmented model', mode, kernel, 'Shapley', name, 'ratio', ratio)
        assert ratio <= END_TO_END_BAR, name
    assert np.all(np.abs(sh.effects.numpy().sum(axis=1) - sh.variance.numpy()) <= END_TO_END_BAR * V)
    # order=2 on the view: its pair masks are the same pass
    s2 = view.sobol_indices(order=2)
    cv = got.closed_variance.numpy()
    assert np.all(np.abs(s2.second_variance.numpy()[:, 0, 1] - (cv[:, 1] - cv[:, 0] - s2.first_variance.numpy()[:, 1])) <= END_TO_END_BAR * V)


def test_two_calls_agree_bitwise():
    m, _ = _model('rep', 'matern52', 3)
    subsets = [(0, 2), (1,), (), (0, 1, 2)]
    a, sa, ia = m.sobol_subsets(subsets, uncertainty=True), m.shapley_effects(uncertainty=True), m.sobol_indices(order=2, uncertainty=True)
    m._aux_engine._scratch.fill_(0x5A)
    b, sb, ib = m.sobol_subsets(subsets, uncertainty=True), m.shapley_effects(uncertainty=True), m.sobol_indices(order=2, uncertainty=True)
    for name in ('closed_variance', 'closed', 'variance', 'mean', 'expected_closed_variance', 'closed_expected', 'expected_variance'):
        assert np.array_equal(getattr(a, name).numpy(), getattr(b, name).numpy()), name
    for name in ('effects', 'shares', 'variance', 'effects_expected', 'shares_expected', 'expected_variance'):
        assert np.array_equal(getattr(sa, name).numpy(), getattr(sb, name).numpy()), name
    for name in ('second', 'second_variance', 'expected_second_variance', 'second_expected'):
        assert np.array_equal(getattr(ia, name).numpy(), getattr(ib, name).numpy(), equal_nan=True), name
    # order=1 is what it was: the same fields bitwise with and without the argument, the new ones None
    one, two = m.sobol_indices(), m.sobol_indices(order=2)
    for name in ('first', 'total', 'variance', 'mean', 'first_variance', 'closed_variance'):
        assert np.array_equal(getattr(one, name).numpy(), getattr(two, name).numpy()), name
    assert one.second is None and one.second_variance is None
    # the effects are in range and add up
    V = sa.variance.numpy()
    assert np.all(np.abs(sa.effects.numpy().sum(axis=1) - V) <= END_TO_END_BAR * V)
    assert np.all(sa.effects.numpy() >= ia.first_variance.numpy() - END_TO_END_BAR * V[:, None])
    assert np.all(sa.effects.numpy() <= (ia.total.numpy() + END_TO_END_BAR) * V[:, None])
    with pytest.raises(ValueError, match='repeats'):
        m.sobol_subsets([(1, 1)])


def test_two_ranks_equal_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_sobol_subsets_gpu_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout
