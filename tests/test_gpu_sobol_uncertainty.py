"""Expected Sobol variances and the exact integrated variance on the GPU (lcgp_sobol_matrix_pairs,
LCGP.sobol_indices(uncertainty=True), LCGP.integrated_variance): every matrix-weighted sum and S0 against the
float64 numpy restatement of tests/sobol_uncertainty_ref.py fed with the engine's own A^-1 (fetch_matrix(2, k): the lower
triangle mirrored), with a NaN-filled scratch, at d = 3 (the narrow kernel), d = 11 (its 16-wide instance) and d = 18 (the
recomputing kernel); the corrections C_u and IV end to end against a dense A^-1 built on the host; identities with
main_effects(); d = 1; determinism; two ranks against one.

Bar of the parity tests: |dev - ref| <= 1e-12 sum |Q| (M_u + M_0) (S0: sum |Q| M_0), the size of what a sum adds up, from the
reference.  End to end: |dev - ref| <= 1e-10 c prod_{l not in u} I2_l, the prior term of C_u (IV: c), unless the host's own two
ways to A^-1 disagree by more than 1e-11 of it -- then ten times that disagreement.  Largest ratios measured on an MI355X: see
profiles/sobol_checks.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import sobol_uncertainty_ref as uref
from tests.test_gpu_sobol import _boxes, _free_port, _model

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PARITY_BAR = 1e-12
END_TO_END_BAR = 1e-10
HOST_AGREES_WITHIN = 1e-11
PLUG = ('first', 'total', 'variance', 'mean', 'first_variance', 'closed_variance')
NEW = ('expected_variance', 'expected_first_variance', 'expected_closed_variance', 'first_expected', 'total_expected',
       'integrated_variance')


def _rows(m):
    """(engine, x, v, ell, sr, theta rows (q, d + 3)) as the model hands them to the engine: the float64 engine, the constrained
    parameters, v = c sr sqrt(D)"""
    eng = m._ensure_aux64()
    n, d, q = int(m.n), int(m.d), int(m.q)
    sr = np.sqrt(m.r.numpy().astype(np.float64)) if m.submethod == 'rep' else np.ones(n)
    ell, scale, nug, D = m.lLmb.numpy(), m.lLmb0.numpy(), m.lnugGPs.numpy(), m.diag_D.numpy().astype(np.float64).reshape(-1)
    c = scale * (1.0 - nug / (1.0 + nug))
    v = (c * np.sqrt(D))[:, None] * sr[None, :]
    assert eng.dtype_name == 'float64' and v.shape == (q, n)
    return eng, np.asarray(m._x_train(), np.float64), v, ell, sr, np.concatenate([ell, scale[:, None], nug[:, None], D[:, None]], axis=1)


def _parity(m, what):
    """every sum and S0 of every component on both boxes against the restatement fed with the engine's A^-1 (the lower
    triangle mirrored, which is what fetch_matrix returns), the scratch full of NaN; returns the worst ratio"""
    eng, x, v, ell, sr, th = _rows(m)
    q, d = v.shape[0], x.shape[1]
    ainv = [eng.fetch_matrix(2, k) for k in range(q)]
    for a in ainv:
        assert np.array_equal(a, a.T)
    worst = 0.0
    for box in _boxes(d):
        first, first0 = eng.sobol_matrix_sums(x, v, ell, box, np.arange(q))      # (allocates the scratch)
        eng._scratch.fill_(0xFF)                                                 # every double a NaN
        sums, s0 = eng.sobol_matrix_sums(x, v, ell, box, np.arange(q))
        assert sums.shape == (q, 2 * d + 1) and s0.shape == (q,) and np.all(np.isfinite(sums)) and np.all(np.isfinite(s0))
        assert np.array_equal(first, sums) and np.array_equal(first0, s0)
        for k in range(q):
            want, want0, size, size0 = uref.matrix_sums(m.kernel, x, ell[k], box, v[k][:, None] * v[k][None, :] * ainv[k])
            ratio = max(np.max(np.abs(sums[k] - want) / size), abs(s0[k] - want0) / size0)
            print('matrix sums', what, 'sub-box' if box[0][0] > 0 else 'default', k, 'ratio', ratio)
            worst = max(worst, ratio)
            assert np.all(np.abs(sums[k] - want) <= PARITY_BAR * size), (what, k, np.abs(sums[k] - want) / size)
            assert abs(s0[k] - want0) <= PARITY_BAR * size0, (what, k, abs(s0[k] - want0) / size0)
        if q > 1:                                                                # a subset of the components, in another order
            part, part0 = eng.sobol_matrix_sums(x, v, ell, box, [q - 1, 0])
            assert np.array_equal(part, sums[[q - 1, 0]]) and np.array_equal(part0, s0[[q - 1, 0]])
    print('matrix sums', what, 'worst ratio', worst)
    return worst


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('mode', ['full', 'rep'])
@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_matrix_sums_against_numpy(kernel, mode, dtype):
    """n = 150, d = 3, p = 6, q = 3: two full 64-tiles and a ragged one of 22 a side, so three diagonal tiles (mirrored reads) and
    three strictly lower ones; eight sums per component, two boxes.  A float32 model reads the A^-1 of its float64 engine"""
    m, _ = _model(mode, kernel, 3, dtype=dtype)
    _parity(m, '%s %s %s' % (kernel, mode, dtype))


@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
@pytest.mark.parametrize('d', [11, 18])
def test_matrix_sums_in_more_dimensions(kernel, d):
    """d = 11: the 16-wide instance of the narrow kernel; d = 18: the kernel that recomputes.  n = 70 (two tiles a side, the
    second one ragged), q = 2"""
    m, _ = _model('full', kernel, d, n=70, p=4, q=2)
    _parity(m, '%s d=%d' % (kernel, d))


@pytest.mark.parametrize('mode', ['full', 'rep'])
@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_corrections_and_integrated_variance_against_dense_numpy(kernel, mode):
    """C_u and IV of every component from the model against the restatement fed with an A^-1 built on the host from the
    constrained parameters and the training inputs, relative to the prior term c prod_{l not in u} I2_l (IV: c)"""
    m, _ = _model(mode, kernel, 3)
    eng, x, v, ell, sr, th = _rows(m)
    d, q = 3, int(m.q)
    bs = m._marginal_box(None)
    C, IV, _ = m._sobol_matrix(bs)
    iv_public = m.integrated_variance(latent=True).numpy()
    assert np.array_equal(iv_public, IV)
    worst, worst_host = 0.0, 0.0
    for k in range(q):
        by_solve, by_inverse, _ = uref.dense_ainv(m.kernel, x, sr, th[k])
        a, b = (uref.component(m.kernel, x, sr, th[k], inv, bs) for inv in (by_solve, by_inverse))
        host = max(np.max(np.abs(a['C'] - b['C']) / a['prior']), abs(a['IV'] - b['IV']) / a['c'])
        bar = END_TO_END_BAR if host <= HOST_AGREES_WITHIN else 10.0 * host
        ratio = max(np.max(np.abs(C[k] - a['C']) / a['prior']), abs(IV[k] - a['IV']) / a['c'])
        print('end to end', kernel, mode, k, 'ratio', ratio, 'host, two ways', host, 'bar', bar)
        worst, worst_host = max(worst, ratio), max(worst_host, host)
        assert np.all(np.abs(C[k] - a['C']) <= bar * a['prior']), (k, np.abs(C[k] - a['C']) / a['prior'])
        assert abs(IV[k] - a['IV']) <= bar * a['c'], (k, abs(IV[k] - a['IV']) / a['c'])
        assert np.all(C[k] >= -1e-12 * a['c']) and np.all(C[k][:2 * d] <= C[k][2 * d] + 1e-12 * a['c'])
    print('end to end', kernel, mode, 'worst ratio', worst, 'host, two ways', worst_host)


@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_identities_with_the_plug_in_fields_and_main_effects(kernel):
    m, _ = _model('full', kernel, 3)
    s0 = m.sobol_indices()
    s = m.sobol_indices(uncertainty=True)
    for name in PLUG:
        assert np.array_equal(getattr(s, name).numpy(), getattr(s0, name).numpy()), name
    for name in NEW:
        assert getattr(s0, name) is None, name
    V, ev, iv = s.variance.numpy(), s.expected_variance.numpy(), s.integrated_variance.numpy()
    assert s.expected_first_variance.shape == (6, 3) and ev.shape == (6,) and iv.shape == (6,)
    assert np.array_equal(m.integrated_variance().numpy(), iv)
    assert np.array_equal(m.integrated_variance(outputs=[4, 1]).numpy(), iv[[4, 1]])
    # the total variance of the surface splits into the variance of its box mean and the expected variance over the box:
    # IV - (E[V] - V) = c prod I2 - S0 mapped to the outputs = main_effects().overall_var
    ov = m.main_effects(grid=2).overall_var.numpy()
    _, _, ovk = m._sobol_matrix(m._marginal_box(None))
    mapped = m._latent_variance_to_rows(ovk, False)
    print('overall_var', kernel, np.max(np.abs(mapped - ov) / ov), np.max(np.abs(iv - (ev - V) - ov) / ov))
    assert np.all(np.abs(mapped - ov) <= 1e-10 * ov)
    assert np.all(np.abs(iv - (ev - V) - ov) <= 1e-10 * ov)
    assert np.all(ev >= V - 1e-12 * V)
    assert np.all(s.expected_first_variance.numpy() >= s.first_variance.numpy() - 1e-12 * V[:, None])
    assert np.all(s.expected_closed_variance.numpy() >= s.closed_variance.numpy() - 1e-12 * V[:, None])
    fe, te = s.first_expected.numpy(), s.total_expected.numpy()
    assert np.all(np.isfinite(fe)) and np.all(np.isfinite(te))
    assert np.all(fe >= -1e-10) and np.all(fe <= te + 1e-10) and np.all(te <= 1.0 + 1e-10)
    assert np.all(iv > 0.0)


@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_a_single_input_explains_everything_in_expectation(kernel):
    m, _ = _model('full', kernel, 1, n=50, p=3, q=2)
    s = m.sobol_indices(uncertainty=True)
    np.testing.assert_allclose(s.first_expected.numpy(), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(s.total_expected.numpy(), 1.0, rtol=0, atol=1e-12)


def test_two_calls_agree_bitwise():
    m, _ = _model('rep', 'matern52', 3)
    a = m.sobol_indices(uncertainty=True)
    iv = m.integrated_variance()
    m._aux_engine._scratch.fill_(0x5A)
    b = m.sobol_indices(uncertainty=True)
    for name in PLUG + NEW:
        assert np.array_equal(getattr(a, name).numpy(), getattr(b, name).numpy()), name
    m._aux_engine._scratch.fill_(0xA5)
    assert np.array_equal(m.integrated_variance().numpy(), iv.numpy())
    assert np.array_equal(iv.numpy(), a.integrated_variance.numpy())
    lat = m.sobol_indices(latent=True, outputs=[2, 0], uncertainty=True)
    assert lat.first_expected.shape == (2, 3) and lat.integrated_variance.shape == (2,)
    assert np.array_equal(lat.integrated_variance.numpy(), m.integrated_variance(latent=True).numpy()[[2, 0]])
    plain = m.sobol_indices(latent=True, outputs=[2, 0])
    for name in PLUG:
        assert np.array_equal(getattr(lat, name).numpy(), getattr(plain, name).numpy()), name
    for name in NEW:
        assert getattr(plain, name) is None, name


def test_two_ranks_equal_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_sobol_uncertainty_gpu_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout
