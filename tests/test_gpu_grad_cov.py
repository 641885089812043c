"""Posterior covariance of the gradient and active subspaces on the GPU (lcgp_predict_gradcov, LCGP.predict_grad_cov /
active_subspace): Gamma and dghat against the float64 numpy restatement of tests/grad_cov_ref.py, dghat bitwise that of
lcgp_predict_grad, independence of the scratch content and of the chunk size, two ranks against one, the device-side
weighted reduction, the off-diagonal stencil applied to the GPU's own predict_latent_cov, float32 against the float64
restatement, and active_subspace end to end.

Measured on an MI355X, worst relative deviation from the numpy restatement over every case of
test_gamma_and_dghat_against_numpy (largest entry as the scale): dghat 2.0e-14 / 1.9e-14 / 5.1e-14, Gamma 1.1e-15 / 4.0e-15 /
4.4e-15 (Matern-3/2 / SE / Matern-5/2) -- inside the first-order bar of 1e-10 (LATENT_BAR).  Weighted reduction against the host
sum of the per-point result: at most 9.3e-16 (bar 1e-13).  Stencil of the GPU's predict_latent_cov against Gamma: within 1 % of
the restatement's own stencil error (Matern-3/2 1.0e-2 absolute on entries up to 9.7, SE 2.3e-6, Matern-5/2 9.8e-7).
active_subspace end to end 6.1e-16 (bar 1e-11)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import lcgp_amd.engine as engine_mod
from lcgp_amd import LCGP, synth
from oracle import lcgp_oracle as orc
from tests import grad_cov_ref as ref
from tests import matern52_oracle as m52
from tests.test_predict_hess_host import pack_lower

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# float64: the project's first-order bar (the same W = L^-1, error ~ cond(A) eps), relative to the largest entry
LATENT_BAR = 1e-10


def _model(mode, kernel, d, n=300, q=2, dtype='float64', seed=81):
    """n = 300 (full) / 150 unique inputs (rep): neither a multiple of 64"""
    if mode == 'full':
        x, y = synth.make_full(seed, n, d, 3, q)
    else:
        x, y = synth.make_rep(seed, n // 2, 3, d, 3, q)
    m = LCGP(y=y, x=x, q=q, submethod=mode, kernel=kernel, device='cuda:0', dtype=dtype)
    o = orc.OracleLCGP(y=y, x=x, q=q, submethod=mode)
    m._set_flat(synth.param_points(seed, o.get_unconstrained())[1])
    return m, x


def _factors(m, eng):
    """(x, sr, [(theta row, Cholesky factor, z)]) in float64 numpy: A_k = I + D_k (C_k o sr sr^T) from the oracle's kernel, its
    factor from np.linalg, z_k = A_k^-1 (Y^T psi_k) -- the engine's theta rows and inputs, nothing else"""
    x, Y = eng.x.cpu().numpy().astype(np.float64), eng.Y.cpu().numpy().astype(np.float64)
    sr = np.ones(eng.n) if eng.sr is None else eng.sr.cpu().numpy().astype(np.float64)
    d = eng.d
    out = []
    for th in eng._theta_last:
        ell, scale, nug, D, psi = th[:d], th[d], th[d + 1], th[d + 2], th[d + 3:]
        if m.kernel == 'matern52':
            Cm = m52.kernel_matrix(x, x, ell, scale, nug, same=True)
        else:
            Cm = orc.matern32(x, x, ell, scale, nug, kernel=m.kernel)
        low = np.linalg.cholesky(np.eye(eng.n) + D * Cm * sr[:, None] * sr[None, :])
        z = np.linalg.solve(low.T, np.linalg.solve(low, Y.T @ psi))
        out.append((th, low, z))
    return x, sr, out


def _restated(m, fac, x0s, rows=64):
    """[(dghat (n0, d), packed Gamma (n0, tri))] per local component; x0s `rows` at a time (the n0 x n x d tensor)"""
    x, sr, comps = fac
    res = []
    for th, low, z in comps:
        jm = np.concatenate([ref.latent_mean_grad(x0s[lo:lo + rows], x, sr, th, z, m.kernel) for lo in range(0, len(x0s), rows)])
        G = np.concatenate([ref.latent_grad_cov(x0s[lo:lo + rows], x, sr, th, low, m.kernel) for lo in range(0, len(x0s), rows)])
        res.append((jm, pack_lower(G)))
    return res


@pytest.mark.parametrize('d', [1, 6, 40])
@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_gamma_and_dghat_against_numpy(mode, kernel, d):
    """64- and 128-row tiles of P, a ragged last tile, the wide-d path (d = 40), a single block of dimension pairs (d = 1) and
    several; n0 = 393 takes more than one pass at d = 6 and d = 40"""
    m, x = _model(mode, kernel, d)
    eng = m._ensure_aux()
    fac = _factors(m, eng)
    xtr = (m.x_unique_s if mode == 'rep' else m.x).numpy()
    rng = np.random.default_rng(d)
    for n0 in (1, 63, 128, 200, 393):
        x0s = rng.uniform(0, 1, (n0, d))
        if n0 > 3:
            x0s[:3] = xtr[[0, 7, 11]]                           # training inputs: no nugget, the continuous surface
        dghat, gamma, M = eng.grad_cov_block(x0s)
        assert M is None and gamma.shape == (eng.q_local, n0, d * (d + 1) // 2) and dghat.shape == (eng.q_local, n0, d)
        dghat, gamma = dghat.cpu().numpy(), gamma.cpu().numpy()
        for k, (jm, G) in enumerate(_restated(m, fac, x0s)):
            for got, want, what in ((dghat[k], jm, 'dghat'), (gamma[k], G, 'gamma')):
                err = np.max(np.abs(got - want)) / np.max(np.abs(want))
                print('latent', mode, kernel, d, n0, k, what, err)
                assert err <= LATENT_BAR, (what, n0, k, err)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_dghat_bitwise_predict_grad_and_independent_of_scratch_content(dtype):
    m, x = _model('full', 'matern52', 6, dtype=dtype)
    eng = m._ensure_aux()
    x0s = np.random.default_rng(9).uniform(0, 1, (200, 6))
    ref_jac = eng.predict_grad_block(x0s)[1][0].cpu().numpy()
    w = np.random.default_rng(10).uniform(0, 1, 200)
    eng.grad_cov_block(x0s)                                     # (grows the scratch to its size)
    first = None
    for fill in (0x00, 0xFF, 0x5A):
        eng._scratch.fill_(fill)
        got = [t.cpu().numpy() for t in eng.grad_cov_block(x0s, w)]
        assert np.array_equal(got[0], ref_jac), fill
        assert all(np.all(np.isfinite(g)) for g in got)
        if first is None:
            first = got
        for a, b in zip(got, first):
            assert np.array_equal(a, b), fill
    # the wide-d path of the contraction too
    m, x = _model('rep', 'matern32', 40, dtype=dtype)
    eng = m._ensure_aux()
    x0s = np.random.default_rng(11).uniform(0, 1, (70, 40))
    assert np.array_equal(eng.grad_cov_block(x0s)[0].cpu().numpy(), eng.predict_grad_block(x0s)[1][0].cpu().numpy())


@pytest.mark.parametrize('d,kernel', [(6, 'matern32'), (40, 'se')])
def test_per_point_results_bitwise_independent_of_the_chunk_size(monkeypatch, d, kernel):
    """a pass takes max(128, PREDICT_CHUNK // d) new inputs and a last pass of fewer than 128 is moved back over its
    predecessor: one pass, 200 + 193, 128 + 128 + 128 + 128 (the last overlapping) for the 393 inputs here.  The weighted sum
    changes its order of summation with the passes, so it is held to 1e-13 of its largest entry, not to the bit"""
    m, x = _model('rep', kernel, d)
    eng = m._ensure_aux()
    x0s = np.random.default_rng(13).uniform(0, 1, (393, d))
    w = np.random.default_rng(14).uniform(0, 1, 393)
    monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', 400 * d)
    want = [t.cpu().numpy() for t in eng.grad_cov_block(x0s, w)]
    for chunk in (200 * d, 128 * d, 1):
        monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', chunk)
        got = [t.cpu().numpy() for t in eng.grad_cov_block(x0s, w)]
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), chunk
        err = np.max(np.abs(got[2] - want[2])) / np.max(np.abs(want[2]))
        print('chunk', d, chunk, err)
        assert err <= 1e-13, (chunk, err)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_equal_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_grad_cov_gpu_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


@pytest.mark.parametrize('mode,kernel,d,dtype', [('full', 'matern32', 6, 'float64'), ('rep', 'matern52', 40, 'float64'),
                                                 ('full', 'se', 1, 'float64'), ('full', 'se', 6, 'float32')])
def test_weighted_reduction(monkeypatch, mode, kernel, d, dtype):
    """M = sum_i w_i Gamma[i] of the per-point call to 1e-13 of its largest entry, bitwise repeatable, and bitwise the same
    from a reduce-only call that never writes the per-point tensor; also over several passes with a moved-back last one"""
    m, x = _model(mode, kernel, d, dtype=dtype)
    eng = m._ensure_aux()
    rng = np.random.default_rng(15)
    for n0, chunk in ((1, None), (63, None), (393, None), (393, 128 * d)):
        if chunk is not None:
            monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', chunk)
        x0s, w = rng.uniform(0, 1, (n0, d)), rng.uniform(0, 1, n0)
        w[0] = 0.0 if n0 > 1 else 1.0
        plain = eng.grad_cov_block(x0s)[1].cpu().numpy()
        dghat, gamma, M = [t.cpu().numpy() for t in eng.grad_cov_block(x0s, w)]
        assert np.array_equal(gamma, plain)                     # the per-point result does not depend on the weights
        want = np.einsum('i,kie->ke', w, gamma)
        err = np.max(np.abs(M - want)) / np.max(np.abs(want))
        print('reduction', mode, kernel, d, dtype, n0, chunk, err)
        assert err <= 1e-13, (n0, chunk, err)
        again = eng.grad_cov_block(x0s, w)[2].cpu().numpy()
        assert np.array_equal(again, M)
        d2, none, M2 = eng.grad_cov_block(x0s, w, per_point=False)
        assert none is None and np.array_equal(M2.cpu().numpy(), M) and np.array_equal(d2.cpu().numpy(), dghat)
    with pytest.raises(ValueError, match='weights'):
        eng.grad_cov_block(x0s, None, per_point=False)


# float32 (x, the factor, dX and P in float32, the dot products and everything behind them in double) against the float64
# numpy restatement, relative to the largest entry: no bound can be derived (the float32 factorisation's error times the
# conditioning of A).  Measured on an MI355X on the well-conditioned n = 300 model below, worst of the two components:
# dghat 7.6e-7 / 8.7e-7 / 1.02e-6, Gamma 1.5e-7 / 4.5e-7 / 5.5e-7 (Matern-3/2 / SE / Matern-5/2); the bar is 4 x the worst of them (and never looser than 2e-2).
MEASURED_F32 = 1.03e-6
F32_BAR = 4 * MEASURED_F32


@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_float32_model_against_the_float64_restatement(kernel):
    assert F32_BAR <= 2e-2
    m32, x = _model('full', kernel, 4, dtype='float32')
    m64, _ = _model('full', kernel, 4)
    e32, e64 = m32._ensure_aux(), m64._ensure_aux()
    x0s = np.random.default_rng(10).uniform(0, 1, (150, 4))
    dghat, gamma, _ = [None if t is None else t.cpu().numpy() for t in e32.grad_cov_block(x0s)]
    errs = []
    for k, (jm, G) in enumerate(_restated(m64, _factors(m64, e64), x0s)):
        for got, want, what in ((dghat[k], jm, 'dghat'), (gamma[k], G, 'gamma')):
            errs.append(np.max(np.abs(got - want)) / np.max(np.abs(want)))
            print('float32', kernel, k, what, errs[-1])
    assert max(errs) <= F32_BAR, errs


@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_gamma_is_the_stencil_of_the_gpu_joint_covariance(kernel):
    """the mixed difference of tests/grad_cov_ref.stencil over OFF-diagonal entries of the GPU's own predict_latent_cov (a
    merged query that shares no launch with this one but the factor), at 8 points with d = 2.  The bar is 4 x the restatement's
    own |stencil - closed form| at the same h and points (the truncation error, measured on the reference, not on the code
    under test) plus a rounding floor of 1e-13 scale_k / h^2"""
    h = 1e-4
    m, x = _model('full', kernel, 2)
    eng = m._ensure_aux()
    fac = _factors(m, eng)
    xtr = fac[0]
    cand = np.random.default_rng(16).uniform(0.05, 0.95, (4000, 2))
    clear = np.flatnonzero(np.min(np.abs(cand[:, None, :] - xtr[None, :, :]), axis=(1, 2)) >= 4.0 * h)
    assert len(clear) >= 8
    x0s = cand[clear[:8]]
    lo, span = m.x_min.numpy().reshape(-1), (m.x_max - m.x_min).numpy().reshape(-1)
    to_raw = lambda s: lo + span * s                             # noqa: E731
    np.testing.assert_allclose(m._standardise_x0(to_raw(x0s))[0], x0s, rtol=0, atol=1e-15)
    gamma = m.predict_grad_cov(to_raw(x0s), latent=True).numpy()            # (q, 8, 2, 2)
    # every stencil point of every base point in one joint covariance: +-h e_l (4 points), +-2h e_m (4 points)
    offs = [s * h * e for e in np.eye(2) for s in (1.0, -1.0)] + [s * 2.0 * h * e for e in np.eye(2) for s in (1.0, -1.0)]
    pts = np.concatenate([x0s + o for o in offs])               # block b = the 8 base points shifted by offs[b]
    S = m.predict_latent_cov(to_raw(pts)).numpy()               # (q, 64, 64)
    index = {tuple(np.round(o / h).astype(int)): b for b, o in enumerate(offs)}
    base = np.arange(8)
    for k, (th, low, z) in enumerate(fac[2]):
        def sigma(xa, xb):
            ba = index[tuple(np.round((xa[0] - x0s[0]) / h).astype(int))]
            bb = index[tuple(np.round((xb[0] - x0s[0]) / h).astype(int))]
            assert ba != bb
            return S[k, 8 * ba + base, 8 * bb + base]
        fd_gpu = ref.stencil(sigma, x0s, h)
        closed = ref.latent_grad_cov(x0s, fac[0], fac[1], th, low, kernel)
        own = np.max(np.abs(ref.stencil_grad_cov(x0s, fac[0], fac[1], th, low, kernel, h) - closed))
        bar = 4.0 * own + 1e-13 * th[2] / h ** 2
        err = np.max(np.abs(fd_gpu - gamma[k]))
        print('stencil', kernel, k, 'err', err, 'reference stencil error', own, 'bar', bar, 'largest entry', np.max(np.abs(closed)))
        assert err <= bar, (k, err, bar)


def test_active_subspace_end_to_end():
    """n = 300, d = 6, p = 3, q = 2, 393 reference points: the device-side reduction against the assembly of the host test
    from the two per-point queries"""
    m, x = _model('full', 'matern32', 6)
    rng = np.random.default_rng(17)
    x_ref = rng.uniform(0, 1, (393, 6))
    w = rng.uniform(0, 1, 393)
    for weights in (None, w):
        res = m.active_subspace(x_ref, weights=weights)
        wn = np.full(393, 1.0 / 393) if weights is None else w / w.sum()
        g = m.predict_grad(x_ref)[0].numpy()
        cov = m.predict_grad_cov(x_ref).numpy()
        want = np.einsum('i,ail,aim->alm', wn, g, g) + np.einsum('i,ailm->alm', wn, cov)
        mat = res.matrix.numpy()
        assert mat.shape == (3, 6, 6)
        err = np.max(np.abs(mat - want)) / np.max(np.abs(want))
        print('active subspace', err, 'cov / mean', np.trace(res.cov_part.numpy()[0]) / np.trace(res.mean_part.numpy()[0]))
        assert err <= 1e-11, err
        assert np.array_equal(mat, res.mean_part.numpy() + res.cov_part.numpy())
        lam, V = res.eigenvalues.numpy(), res.eigenvectors.numpy()
        assert np.all(np.diff(lam, axis=1) <= 0) and np.all(lam[:, -1] >= -1e-12 * lam[:, 0])
        np.testing.assert_allclose(np.einsum('alk,ak,amk->alm', V, lam, V), mat, rtol=0, atol=1e-12 * np.max(np.abs(mat)))
