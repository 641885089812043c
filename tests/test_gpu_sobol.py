"""Closed-form Sobol indices on the GPU (lcgp_sobol_pairs, LCGP.sobol_indices): every pair sum D_u against the float64 numpy
restatement of tests/sobol_ref.py with a NaN-filled scratch, at d = 3 (the narrow kernel), d = 11 (its 16-wide instance) and
d = 18 (the recomputing kernel); the indices end to end against paths that enter no pair integral (main_effects,
predict_marginal, predict); d = 1; determinism; the range of the indices; two ranks against one.

Bar of the parity tests: |dev - ref| <= 1e-12 sum_ii' |w_i| |w'_i'| (M_u + M_0), the size of what a D_u adds up (from the
reference), so it does not loosen where an index is small.  Largest ratio |dev - ref| / that sum measured on an MI355X: see
profiles/sobol_checks.txt."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from lcgp_amd import LCGP, synth
from oracle import lcgp_oracle as orc
from tests import sobol_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PARITY_BAR = 1e-12
FIELDS = ('first', 'total', 'variance', 'mean', 'first_variance', 'closed_variance')


def _model(mode, kernel, d, n=150, p=6, q=3, dtype='float64', seed=83):
    """n = 150 inputs (full) / 150 unique inputs x 2 replicates (rep): not a multiple of 64, three tiles a side"""
    if mode == 'full':
        x, y = synth.make_full(seed, n, d, p, q)
    else:
        x, y = synth.make_rep(seed, n, 2, d, p, q)
    m = LCGP(y=y, x=x, q=q, submethod=mode, kernel=kernel, device='cuda:0', dtype=dtype)
    o = orc.OracleLCGP(y=y, x=x, q=q, submethod=mode)
    m._set_flat(synth.param_points(seed, o.get_unconstrained())[1])
    return m, x


def _weights(m):
    """(engine, x, w, ell) as sobol_indices hands them to the engine: the float64 engine's z, the constrained parameters"""
    eng = m._ensure_aux64()
    n, d, q = int(m.n), int(m.d), int(m.q)
    sr = np.sqrt(m.r.numpy().astype(np.float64)) if m.submethod == 'rep' else np.ones(n)
    z = np.stack([eng.fetch_vector(1, k) for k in range(q)])
    scale, nug = m.lLmb0.numpy(), m.lnugGPs.numpy()
    w = (scale * (1.0 - nug / (1.0 + nug)))[:, None] * sr[None, :] * z
    assert eng.dtype_name == 'float64' and w.shape == (q, n)
    return eng, np.asarray(m._x_train(), np.float64), w, m.lLmb.numpy()


def _boxes(d):
    """the default box and a sub-box that leaves training inputs outside on both sides"""
    return (np.stack([np.zeros(d), np.ones(d)]), np.stack([np.full(d, 0.3), np.full(d, 0.75)]))


def _parity(m, what):
    """every D_u of every pair k <= k' on both boxes against the restatement, the scratch full of NaN; returns the worst ratio"""
    eng, x, w, ell = _weights(m)
    q, d = w.shape[0], x.shape[1]
    pairs = np.array([(k, kp) for k in range(q) for kp in range(k, q)])
    worst = 0.0
    for box in _boxes(d):
        if box[0][0] > 0.0:
            assert np.any(x < box[0]) and np.any(x > box[1])
        first, _ = eng.sobol_pairs(x, w, ell, box, pairs)                 # (allocates the scratch)
        eng._scratch.fill_(0xFF)                                          # every double a NaN
        D, means = eng.sobol_pairs(x, w, ell, box, pairs)
        assert D.shape == (len(pairs), 2 * d + 1) and np.all(np.isfinite(D)) and np.all(np.isfinite(means))
        assert np.array_equal(first, D)
        for r, (k, kp) in enumerate(pairs):
            want, mm, size = ref.pair_sums(m.kernel, x, w[k], ell[k], w[kp], ell[kp], box)
            ratio = np.max(np.abs(D[r] - want) / size)
            print('pair sums', what, 'sub-box' if box[0][0] > 0 else 'default', (int(k), int(kp)), 'ratio', ratio)
            worst = max(worst, ratio)
            assert np.all(np.abs(D[r] - want) <= PARITY_BAR * size), (what, k, kp, np.abs(D[r] - want) / size)
            if k == kp:
                assert abs(means[r] - mm[0]) <= PARITY_BAR * np.sum(np.abs(w[k])), (what, k)
            else:
                assert means[r] == 0.0
    print('pair sums', what, 'worst ratio', worst)
    return worst


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('mode', ['full', 'rep'])
@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_pair_sums_against_numpy(kernel, mode, dtype):
    """n = 150, d = 3, p = 6, q = 3: six pairs, seven subsets, two boxes.  A float32 model hands over the weights of its
    float64 engine, so its sums meet the same bar"""
    m, _ = _model(mode, kernel, 3, dtype=dtype)
    _parity(m, '%s %s %s' % (kernel, mode, dtype))


@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
@pytest.mark.parametrize('d', [11, 18])
def test_pair_sums_in_more_dimensions(kernel, d):
    """d = 11: the 16-wide instance of the narrow kernel; d = 18: the kernel that recomputes (d^2 pair integrals per element).
    n = 70 (two tiles a side, the second one ragged), q = 2"""
    m, _ = _model('full', kernel, d, n=70, p=4, q=2)
    _parity(m, '%s d=%d' % (kernel, d))


@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_mean_and_first_order_variances_against_the_marginal_path(kernel):
    """.mean is main_effects().overall; V_l is the variance of predict_marginal's curve in input l, taken at piecewise
    Gauss-Legendre nodes split at the training coordinates, 8 nodes per piece.  Both within 1e-10 of V"""
    m, x = _model('full', kernel, 3)
    s = m.sobol_indices()
    V = s.variance.numpy()
    assert np.all(V > 0.0)
    overall = m.main_effects(grid=2).overall.numpy()
    print('mean against main_effects', kernel, np.max(np.abs(s.mean.numpy() - overall) / V))
    assert np.all(np.abs(s.mean.numpy() - overall) <= 1e-10 * V)
    xn = np.asarray(x)
    lo, hi = xn.min(axis=0), xn.max(axis=0)
    for l in range(3):
        t, wt = ref.piecewise_gauss_legendre(8, lo[l], hi[l], xn[:, l])
        assert len(t) == 8 * 149
        x0 = np.full((len(t), 3), np.nan)
        x0[:, l] = t
        curve = m.predict_marginal(x0, [c for c in range(3) if c != l])[0].numpy()
        vl = ((curve - (curve @ wt)[:, None]) ** 2) @ wt
        print('V_l against the marginal curve', kernel, l, np.max(np.abs(s.first_variance.numpy()[:, l] - vl) / V))
        assert np.all(np.abs(s.first_variance.numpy()[:, l] - vl) <= 1e-10 * V)


def test_total_variance_against_tensor_quadrature_of_predict():
    """d = 2, n = 40, Matern-3/2: V against the tensor piecewise rule (6 nodes per piece and dimension, pieces split at the
    training coordinates) over predict() itself.  No node is a training input, so predict is the continuous surface"""
    m, x = _model('full', 'matern32', 2, n=40, p=4, q=2)
    s = m.sobol_indices()
    xn = np.asarray(x)
    lo, hi = xn.min(axis=0), xn.max(axis=0)
    rules = [ref.piecewise_gauss_legendre(6, lo[l], hi[l], xn[:, l]) for l in range(2)]
    g0, g1 = np.meshgrid(rules[0][0], rules[1][0], indexing='ij')
    f = m.predict(np.stack([g0.reshape(-1), g1.reshape(-1)], axis=1))[0].numpy().reshape(4, len(rules[0][0]), len(rules[1][0]))
    w0, w1 = rules[0][1], rules[1][1]
    mean = np.einsum('i,aij,j->a', w0, f, w1)
    V = np.einsum('i,aij,j->a', w0, (f - mean[:, None, None]) ** 2, w1)
    print('V against the tensor rule', np.abs(s.variance.numpy() - V) / V, 'mean', np.abs(s.mean.numpy() - mean) / V)
    assert np.all(np.abs(s.variance.numpy() - V) <= 1e-10 * V)
    assert np.all(np.abs(s.mean.numpy() - mean) <= 1e-10 * V)


@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_a_single_input_explains_everything(kernel):
    m, _ = _model('full', kernel, 1, n=50, p=3, q=2)
    s = m.sobol_indices()
    np.testing.assert_allclose(s.first.numpy(), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(s.total.numpy(), 1.0, rtol=0, atol=1e-12)


def test_two_calls_agree_bitwise_and_the_indices_are_in_range():
    m, x = _model('rep', 'matern52', 3)
    a = m.sobol_indices()
    m._aux_engine._scratch.fill_(0x5A)
    b = m.sobol_indices()
    for name in FIELDS:
        assert np.array_equal(getattr(a, name).numpy(), getattr(b, name).numpy()), name
    first, total = a.first.numpy(), a.total.numpy()
    assert first.shape == (6, 3) and np.all(np.isfinite(first)) and np.all(np.isfinite(total))
    assert np.all(first >= -1e-10) and np.all(first <= total + 1e-10) and np.all(first.sum(axis=1) <= 1.0 + 1e-10)
    assert np.all(total <= 1.0 + 1e-10)
    lat = m.sobol_indices(latent=True, outputs=[2, 0])
    assert lat.first.shape == (2, 3)
    assert np.all(lat.first.numpy() >= -1e-10) and np.all(lat.first.numpy() <= lat.total.numpy() + 1e-10)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_equal_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_sobol_gpu_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout
