"""The exact box ALC on the GPU (lcgp_box_alc, HotPathEngine.box_alc_block, LCGP.integrated_variance_reduction):
every R_k(c) against the float64 numpy restatement of tests/box_alc_ref.py fed with the engine's own A^-1 (fetch_matrix(2, k)),
with a NaN-filled scratch, at n = 150 (three 64-tiles a side, the last one ragged), 70 candidates (two 64-row tiles) and d = 1, 3
and 18; bitwise equality across chunks, groups of components, scratch contents and ranks; the gain against
integrated_variance() - condition(c).integrated_variance() and against variance_reduction() on a Gauss-Legendre rule.

Bars.  Parity: |dev - ref| <= 1e-12 size, size = (c^2 m_cc + 2 c |b_c| . m_c + |b_c|^T M |b_c|) / den from the reference, the
project's parity bar for the Sobol sums -- the three terms cancel, so the bar is never stated against the gain.  End to end:
1e-10 of the prior term scale_a^2 sum_k W_ka^2 c_k, the project's end-to-end bar for the integrated variance; those tests first
assert, from the restatement, that every gain they check is at least 1e-6 of that term, so the bar checks four digits or more.
Largest ratios measured on an MI355X: profiles/box_alc_checks.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest

from lcgp_amd import engine as engine_module
from tests import box_alc_ref as bref
from tests import marginal_ref as mref
from tests.test_gpu_sobol import _boxes, _free_port, _model
from tests.test_gpu_sobol_uncertainty import _rows

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PARITY_BAR = 1e-12
END_TO_END_BAR = 1e-10
GAIN_AT_LEAST = 1e-6
N_CAND = 70


def _candidates_s(m, n_cand, seed=7):
    """(standardised candidates uniform in the training box widened by 10 %, match): on the rep path candidates 5 and 66 ARE
    unique inputs 9 and 140 (one in each 64-row tile of the candidates)"""
    rng = np.random.default_rng(seed)
    d = int(m.d)
    xc = -0.05 + 1.1 * rng.random((n_cand, d))
    if m.submethod != 'rep':
        return xc, None
    xt = np.asarray(m._x_train(), np.float64)
    match = np.full(n_cand, -1, np.int32)
    for j, i in ((5, 9), (n_cand - 4, 140)):
        xc[j], match[j] = xt[i], i
    return xc, match


def _parity(m, what, monkeypatch, r=1):
    """R of every component and candidate on both boxes against the restatement, the scratch full of NaN, and the bitwise
    equalities: chunks of 37 and of 70 rows, groups of one and of two components, scratch contents.  Returns the worst ratio"""
    eng, x, _, _, sr, th = _rows(m)
    q, d = th.shape[0], x.shape[1]
    ainv = [eng.fetch_matrix(2, k) for k in range(q)]
    xc, match = _candidates_s(m, N_CAND)
    worst = 0.0
    for box in _boxes(d):
        first = eng.box_alc_block(xc, box, match, r).cpu().numpy()               # (allocates the scratch)
        eng._scratch.fill_(0xFF)                                                 # every double a NaN
        R = eng.box_alc_block(xc, box, match, r).cpu().numpy()
        assert R.shape == (q, N_CAND) and np.all(np.isfinite(R))
        assert np.array_equal(first, R)
        for k in range(q):
            t = bref.terms(m.kernel, x, sr, th[k], ainv[k], box, xc, match, r)
            ratio = np.max(np.abs(R[k] - t['R']) / t['size'])
            print('box alc', what, 'sub-box' if box[0][0] > 0 else 'default', 'r', r, k, 'ratio', ratio,
                  'size / c', np.max(t['size']) / t['c'], 'smallest gain / c', np.min(t['R']) / t['c'])
            worst = max(worst, ratio)
            assert np.all(np.abs(R[k] - t['R']) <= PARITY_BAR * t['size']), (what, k, np.abs(R[k] - t['R']) / t['size'])
        with monkeypatch.context() as mp:
            mp.setattr(engine_module, 'PREDICT_CHUNK', 37)
            eng._scratch.fill_(0x5A)
            assert np.array_equal(eng.box_alc_block(xc, box, match, r).cpu().numpy(), R), 'chunks of 37 rows'
        for group in (1, 2):
            eng._scratch.fill_(0x00)
            assert np.array_equal(eng.box_alc_block(xc, box, match, r, q_group=group).cpu().numpy(), R), 'groups of %d' % group
    print('box alc', what, 'worst ratio', worst)
    return worst


@pytest.mark.parametrize('mode', ['full', 'rep'])
@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_box_alc_block_against_numpy(kernel, mode, monkeypatch):
    """n = 150, d = 3, p = 6, q = 3, 70 candidates, two boxes; rep: two candidates are unique inputs, and r = 3"""
    m, _ = _model(mode, kernel, 3)
    _parity(m, '%s %s' % (kernel, mode), monkeypatch, r=3 if mode == 'rep' else 1)


def test_box_alc_block_of_a_float32_model(monkeypatch):
    """a float32 model answers from its float64 engine and meets the same bar"""
    m, _ = _model('full', 'matern32', 3, dtype='float32')
    _parity(m, 'matern32 full float32', monkeypatch)


@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
@pytest.mark.parametrize('d', [1, 18])
def test_box_alc_block_in_one_and_in_many_dimensions(kernel, d, monkeypatch):
    m, _ = _model('full', kernel, d, p=4, q=2)
    _parity(m, '%s d=%d' % (kernel, d), monkeypatch)


def test_chunks_from_128_candidates_on_agree_bitwise(monkeypatch):
    """200 candidates: one pass on 128-row tiles against passes of 128 rows (the short last pass moved back over its
    predecessor) -- from 128 candidates on no pass runs on 64-row tiles, whose V sums in another order"""
    m, _ = _model('rep', 'matern52', 3)
    eng = m._ensure_aux64()
    xc, match = _candidates_s(m, 200)
    box = _boxes(3)[1]
    R = eng.box_alc_block(xc, box, match, 2).cpu().numpy()
    with monkeypatch.context() as mp:
        mp.setattr(engine_module, 'PREDICT_CHUNK', 100)
        eng._scratch.fill_(0xFF)
        assert np.array_equal(eng.box_alc_block(xc, box, match, 2, q_group=2).cpu().numpy(), R)


def _prior_term(m):
    """scale_a^2 sum_k W_ka^2 c_k per output: what the end-to-end bars are stated against"""
    W, _, scale, _ = m._output_map()
    scale_k, nug = m.lLmb0.numpy(), m.lnugGPs.numpy()
    return scale ** 2 * ((W ** 2).T @ (scale_k * (1.0 - nug / (1.0 + nug))))


def _restated_gain(m, xc_raw, box_s, replicates=1):
    """Delta (p, n_cand) from the restatement fed with the engine's A^-1, and the match it used"""
    eng, x, _, _, sr, th = _rows(m)
    xc = m._standardise_x0(xc_raw)[0]
    match = None
    if m.submethod == 'rep':
        lookup = {row.tobytes(): i for i, row in enumerate(np.ascontiguousarray(x))}
        match = np.array([lookup.get(row.tobytes(), -1) for row in np.ascontiguousarray(xc)], np.int32)
    R = np.stack([bref.terms(m.kernel, x, sr, th[k], eng.fetch_matrix(2, k), box_s, xc, match, replicates)['R']
                  for k in range(th.shape[0])])
    W, _, scale, _ = m._output_map()
    return bref.output_map(R, W, scale), match


@pytest.mark.parametrize('mode', ['full', 'rep'])
@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_gain_is_the_drop_of_integrated_variance_after_condition(kernel, mode):
    """integrated_variance_reduction(xc)[:, j] against integrated_variance() - condition(xc[j], .).integrated_variance() for 6
    candidates that are new inputs (a view refuses a training input), on the default box and on a raw-scale sub-box"""
    m, x = _model(mode, kernel, 3)
    xn = np.asarray(x)
    lo, hi = xn.min(axis=0), xn.max(axis=0)
    rng = np.random.default_rng(11)
    xc = lo - 0.05 * (hi - lo) + 1.1 * (hi - lo) * rng.random((6, 3))
    prior = _prior_term(m)
    for box in (None, np.stack([lo + 0.3 * (hi - lo), lo + 0.75 * (hi - lo)])):
        bs = m._marginal_box(box)
        want, match = _restated_gain(m, xc, bs)
        assert match is None or np.all(match < 0)
        assert np.all(want >= GAIN_AT_LEAST * prior[:, None]), np.min(want / prior[:, None])
        gain = m.integrated_variance_reduction(xc, box=box).numpy()
        assert gain.shape == (int(m.p), 6) and gain.dtype == np.float64
        iv = m.integrated_variance(box=box).numpy()
        worst = 0.0
        for j in range(6):
            after = m.condition(xc[j:j + 1], np.zeros((int(m.p), 1))).integrated_variance(box=box).numpy()
            ratio = np.max(np.abs(gain[:, j] - (iv - after)) / prior)
            worst = max(worst, ratio)
            assert np.all(np.abs(gain[:, j] - (iv - after)) <= END_TO_END_BAR * prior), (kernel, mode, j, ratio)
        print('gain against condition', kernel, mode, 'default' if box is None else 'sub-box', 'worst / prior', worst,
              'smallest gain / prior', np.min(want / prior[:, None]))
        assert np.all(gain <= iv[:, None])


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_gain_is_variance_reduction_on_a_gauss_legendre_rule(mode):
    """kernel = 'se', d = 2: with x_ref the 16 x 16 Gauss-Legendre nodes of the box and weights their weights, variance_reduction
    is the same integral by a rule exact to 1e-14 c (tests/test_box_alc_host.py).  Rep: candidates 1 and 4 ARE unique training
    inputs, with replicates 1 and 3 -- what a view refuses"""
    m, x = _model(mode, 'se', 2)
    xn = np.asarray(x)
    lo, hi = xn.min(axis=0), xn.max(axis=0)
    rng = np.random.default_rng(13)
    xc = lo - 0.05 * (hi - lo) + 1.1 * (hi - lo) * rng.random((6, 2))
    if mode == 'rep':
        xu = m.x_unique.numpy()
        xc[1], xc[4] = xu[9], xu[140]
    prior = _prior_term(m)
    for box in (None, np.stack([lo + 0.3 * (hi - lo), lo + 0.75 * (hi - lo)])):
        b = np.stack([lo, hi]) if box is None else box
        rules = [mref.gauss_legendre(16, b[0][l], b[1][l]) for l in range(2)]
        g0, g1 = np.meshgrid(rules[0][0], rules[1][0], indexing='ij')
        nodes = np.stack([g0.reshape(-1), g1.reshape(-1)], axis=1)
        wts = (rules[0][1][:, None] * rules[1][1][None, :]).reshape(-1)
        for r in ((1, 3) if mode == 'rep' else (1,)):
            want, match = _restated_gain(m, xc, m._marginal_box(box), r)
            if mode == 'rep':
                assert list(match) == [-1, 9, -1, -1, 140, -1]
            assert np.all(want >= GAIN_AT_LEAST * prior[:, None]), np.min(want / prior[:, None])
            gain = m.integrated_variance_reduction(xc, box=box, replicates=r).numpy()
            alc = m.variance_reduction(xc, x_ref=nodes, weights=wts, replicates=r).numpy()
            ratio = np.max(np.abs(gain - alc) / prior[:, None])
            print('gain against variance_reduction', mode, 'default' if box is None else 'sub-box', 'r', r, 'worst / prior', ratio,
                  'smallest gain / prior', np.min(want / prior[:, None]))
            assert np.all(np.abs(gain - alc) <= END_TO_END_BAR * prior[:, None]), (mode, r, ratio)


def test_latent_gains_map_to_the_outputs_and_stay_below_the_integrated_variance():
    m, x = _model('rep', 'matern32', 3)
    xn = np.asarray(x)
    lo, hi = xn.min(axis=0), xn.max(axis=0)
    xc = lo + (hi - lo) * np.random.default_rng(17).random((N_CAND, 3))
    R = m.integrated_variance_reduction(xc, latent=True).numpy()
    assert R.shape == (int(m.q), N_CAND)
    W, _, scale, _ = m._output_map()
    delta = m.integrated_variance_reduction(xc).numpy()
    np.testing.assert_allclose(delta, bref.output_map(R, W, scale), rtol=1e-14, atol=0)
    assert np.array_equal(m.integrated_variance_reduction(xc, outputs=[4, 1]).numpy(), delta[[4, 1]])
    assert np.all(R <= m.integrated_variance(latent=True).numpy()[:, None])
    assert np.all(delta <= m.integrated_variance().numpy()[:, None])
    assert np.all(m.integrated_variance_reduction(xc, replicates=2, latent=True).numpy() >= R)


def test_two_ranks_equal_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_box_alc_gpu_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout
