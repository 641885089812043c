"""Box-averaged predictions on the GPU (lcgp_predict_marginal, LCGP.predict_marginal / main_effects): ghat and gvar against the
float64 numpy restatement of tests/marginal_ref.py, rows with an empty mask bitwise those of lcgp_predict, NaN under the mask,
independence of the scratch content, of the chunk size and of the number of ranks, a Gauss-Legendre rule over the GPU's own
pointwise queries (predict and predict_latent_cov: no closed form enters), float32 against the float64 restatement, and
main_effects end to end.

Measured on an MI355X, worst deviation from the numpy restatement over every case of test_ghat_and_gvar_against_numpy (largest
entry as the scale): ghat 5.3e-14 / 4.0e-14 / 6.2e-14, gvar 7.9e-15 / 9.2e-15 / 4.0e-14 (Matern-3/2 / SE / Matern-5/2) -- inside
the first-order bar of 1e-10 (LATENT_BAR).  Gauss-Legendre over the GPU's own predict and predict_latent_cov (8 nodes per
dimension): mean 1.2e-11 / 7.9e-11 / 1.5e-10, variance 2.6e-12 / 8.6e-11 / 8.8e-11 with dimension 0 / 1 / 2 kept (bar 10 x the
CPU-recorded 1.6e-10).  main_effects().overall against the 1-D rule over each main effect: 1.3e-10 / 4.8e-13 / 3.1e-14 (same
bar).  float32 against the float64 restatement: ghat 5.81e-6, gvar 2.0e-6 (bar 4 x 5.81e-6).  Bitwise: empty-mask rows against
predict_block, NaN / 0 / 1e30 under the mask, three scratch fills, four chunk sizes, two ranks against one, main_effects against
predict_marginal on the same rows."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import lcgp_amd.engine as engine_mod
from lcgp_amd import LCGP, synth
from oracle import lcgp_oracle as orc
from tests import marginal_ref as ref
from tests import matern52_oracle as m52
from tests.test_marginal_host import CPU_QUAD_DEV, GL_NODES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# float64: the project's first-order bar (the same W = L^-1, error ~ cond(A) eps), relative to the largest entry
LATENT_BAR = 1e-10
N0 = 70                                        # rows per call: not a multiple of 64


def _model(mode, kernel, d, n=300, q=2, dtype='float64', seed=81):
    """n = 300 (full) / 150 unique inputs x 2 replicates (rep): neither a multiple of 64"""
    if mode == 'full':
        x, y = synth.make_full(seed, n, d, 3, q)
    else:
        x, y = synth.make_rep(seed, n // 2, 2, d, 3, q)
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


def _rows(d, n0=N0, seed=3):
    """x0s (NaN under the mask) and per-row masks: empty, a single dimension, all but one, all, and random ones; with d > 32
    the single and the kept dimensions walk across the boundary of the 32-dimension chunks (30 .. 33)"""
    rng = np.random.default_rng(seed + d)
    x0s = rng.uniform(0.0, 1.0, (n0, d))
    mask = np.zeros((n0, d), bool)
    edge = [l for l in (0, 30, 31, 32, 33, d - 1) if l < d]
    for i in range(n0):
        l = edge[(i // 5) % len(edge)]
        kind = i % 5
        if kind == 1:
            mask[i, l] = True
        elif kind == 2:
            mask[i] = True
            mask[i, l] = False
        elif kind == 3:
            mask[i] = True
        elif kind == 4:
            mask[i] = rng.uniform(0, 1, d) < 0.5
            if d > 32:
                mask[i, 31], mask[i, 32] = True, False            # (straddles the chunk boundary)
    x0s[mask] = np.nan
    return x0s, mask


def _boxes(d):
    """the default box and a sub-box that leaves training inputs outside on both sides"""
    return (np.stack([np.zeros(d), np.ones(d)]), np.stack([np.full(d, 0.3), np.full(d, 0.75)]))


def _restated(m, fac, x0s, mask, box):
    x, sr, comps = fac
    return [ref.latent_marginal(x0s, mask, box, x, sr, th, low, z, m.kernel) for th, low, z in comps]


@pytest.mark.parametrize('d', [3, 34])
@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_ghat_and_gvar_against_numpy(mode, kernel, d):
    """70 rows with every kind of mask, both boxes; d = 34 runs the 32-dimension chunk loop twice.  Measured worst deviation of
    the largest entry over all cases (MI355X): see MEASURED_F64 below"""
    m, x = _model(mode, kernel, d)
    eng = m._ensure_aux()
    fac = _factors(m, eng)
    x0s, mask = _rows(d)
    assert (~mask.any(axis=1)).sum() >= 10 and mask.all(axis=1).sum() >= 10
    for box in _boxes(d):
        xin = fac[0]
        if box[0][0] > 0.0:
            assert np.any(xin < box[0]) and np.any(xin > box[1])
        got = eng.predict_marginal_block(x0s, mask, box).cpu().numpy()
        assert got.shape == (2, eng.q_local, N0)
        for k, (gh, gv) in enumerate(_restated(m, fac, x0s, mask, box)):
            for h, want, what in ((0, gh, 'ghat'), (1, gv, 'gvar')):
                err = np.max(np.abs(got[h, k] - want)) / np.max(np.abs(want))
                print('latent', mode, kernel, d, 'sub-box' if box[0][0] > 0 else 'default', k, what, err)
                assert err <= LATENT_BAR, (what, k, err)
            assert np.all(got[1, k] > 0.0)


# worst figures the test above printed on an MI355X over its 12 cases, both boxes, both components (Matern-3/2 / SE / Matern-5/2):
# ghat 5.3e-14 / 4.0e-14 / 6.2e-14, gvar 7.9e-15 / 9.2e-15 / 4.0e-14
MEASURED_F64 = 6.2e-14


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('kernel,d', [('matern32', 3), ('se', 34), ('matern52', 34)])
def test_rows_with_an_empty_mask_are_bitwise_predict_block(dtype, kernel, d):
    m, x = _model('rep', kernel, d, dtype=dtype)
    eng = m._ensure_aux()
    x0s, mask = _rows(d)
    empty = ~mask.any(axis=1)
    plain = eng.predict_block(np.where(mask, 0.5, x0s), same=False).cpu().numpy()
    for box in _boxes(d):
        got = eng.predict_marginal_block(x0s, mask, box).cpu().numpy()
        assert np.array_equal(got[:, :, empty], plain[:, :, empty])
        assert not np.array_equal(got[:, :, ~empty], plain[:, :, ~empty])
    # no row integrates anything: the whole block, 64-row tiles and 128-row tiles
    for n0 in (N0, 200):
        x0 = np.random.default_rng(4).uniform(0, 1, (n0, d))
        got = eng.predict_marginal_block(x0, np.zeros((n0, d), bool), _boxes(d)[1])
        assert np.array_equal(got.cpu().numpy(), eng.predict_block(x0, same=False).cpu().numpy())


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_nan_under_the_mask_is_zeros_there_through_the_library(dtype):
    """the engine uploads zeros under the mask; here the library itself gets NaN there (its kernel must not load them)"""
    import torch
    from lcgp_amd import _hip
    d = 34
    m, x = _model('full', 'matern52', d, dtype=dtype)
    eng = m._ensure_aux()
    x0s, mask = _rows(d)
    box = _boxes(d)[1]
    want = eng.predict_marginal_block(x0s, mask, box).cpu().numpy()
    md = torch.as_tensor(mask.astype(np.uint8)).to(eng.device)
    bd = torch.as_tensor(box).to(eng.device)
    for junk in (np.nan, 0.0, 1e30):
        x0d = torch.as_tensor(np.where(mask, junk, x0s)).to(eng.device, eng.tdtype).contiguous()
        out = torch.full((2, eng.q_local, N0), np.nan, dtype=torch.float64, device=eng.device)
        _hip.check(eng.lib.lcgp_predict_marginal(
            eng._stream(), eng.dtype, eng.kernel_id, eng.n, d, eng.p, eng.q_local, eng._p(eng.x), eng._p(eng.sr),
            eng._p(eng.theta_dev), eng._p(eng.workspace), N0, eng._p(x0d), eng._p(md), eng._p(bd), eng._p(eng._scratch),
            eng._p(out[0]), eng._p(out[1]), N0), 'lcgp_predict_marginal')
        assert np.array_equal(out.cpu().numpy(), want), junk


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_bitwise_independent_of_scratch_content_and_chunk_size(monkeypatch, dtype):
    """a pass takes max(128, PREDICT_CHUNK) rows and a last pass of fewer than 128 is moved back over its predecessor: one
    pass, 200 + 128 (overlapping), 128 + 128 + 128 (overlapping) for the 300 rows here"""
    d = 34
    m, x = _model('rep', 'matern32', d, dtype=dtype)
    eng = m._ensure_aux()
    x0s, mask = _rows(d, n0=300)
    box = _boxes(d)[1]
    want = eng.predict_marginal_block(x0s, mask, box).cpu().numpy()
    assert np.all(np.isfinite(want))
    for fill in (0x00, 0xFF, 0x5A):
        eng._scratch.fill_(fill)
        assert np.array_equal(eng.predict_marginal_block(x0s, mask, box).cpu().numpy(), want), fill
    for chunk in (200, 128, 1):
        monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', chunk)
        eng._scratch.fill_(0x5A)
        assert np.array_equal(eng.predict_marginal_block(x0s, mask, box).cpu().numpy(), want), chunk
    # fewer than 128 rows are one pass whatever the chunk size
    a = eng.predict_marginal_block(x0s[:N0], mask[:N0], box).cpu().numpy()
    monkeypatch.setattr(engine_mod, 'PREDICT_CHUNK', 2048)
    assert np.array_equal(eng.predict_marginal_block(x0s[:N0], mask[:N0], box).cpu().numpy(), a)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_equal_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_marginal_gpu_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


QUAD_BOX = np.array([[0.1, 0.25, 0.0], [0.9, 1.0, 0.8]])
QUAD_KEEP = np.array([0.15, 0.5, 0.85])


def test_gauss_legendre_over_the_gpus_own_pointwise_queries():
    """SE, d = 3, two dimensions integrated (each pair): the tensor rule with the node count the CPU test fixed, mean from
    predict()'s latents at the nodes, variance w^T Sigma w from predict_latent_cov minus nt_k scale_k sum w_i^2 (that matrix
    carries the nugget on its diagonal, which no average over a set of positive measure sees).  Bar: ten times the deviation of
    the rule the CPU test recorded.  Nothing of the closed forms enters the reference."""
    m, x = _model('full', 'se', 3)
    eng = m._ensure_aux()
    lo, span = m.x_min.numpy().reshape(-1), (m.x_max - m.x_min).numpy().reshape(-1)
    to_raw = lambda s: lo + span * s                             # noqa: E731
    th = np.asarray(eng._theta_last)
    nugget = th[:, 3] * th[:, 4] / (1.0 + th[:, 4])             # nt_k scale_k
    worst = 0.0
    for keep in range(3):
        dims = [l for l in range(3) if l != keep]
        nodes, wts = ref.tensor_rule(GL_NODES, QUAD_BOX, dims)
        x0s = np.full((3, 3), np.nan)
        x0s[:, keep] = QUAD_KEEP
        mask = np.ones((3, 3), bool)
        mask[:, keep] = False
        gh, gv = [t.numpy() for t in m.predict_marginal(to_raw(np.where(mask, 0.0, x0s)), mask, box=to_raw(QUAD_BOX), latent=True)]
        mean, var = np.empty((2, 3)), np.empty((2, 3))
        for i, v in enumerate(QUAD_KEEP):
            pts = np.empty((len(wts), 3))
            pts[:, dims] = nodes
            pts[:, keep] = v
            mean[:, i] = m._latent_predict(to_raw(pts))[0] @ wts
            S = m.predict_latent_cov(to_raw(pts)).numpy()
            var[:, i] = np.einsum('i,kij,j->k', wts, S, wts) - nugget * np.sum(wts * wts)
        em, ev = np.max(np.abs(mean - gh)) / np.max(np.abs(gh)), np.max(np.abs(var - gv)) / np.max(np.abs(gv))
        print('gauss-legendre on the GPU', keep, 'mean', em, 'var', ev)
        worst = max(worst, em, ev)
    assert worst <= 10.0 * CPU_QUAD_DEV, worst


# float32 (x, the factor, the rows and U in float32; the table, the priors and the reductions in double) against the float64
# numpy restatement, relative to the largest entry: no bound can be derived (the float32 factorisation's error times the
# conditioning of A).  Measured on an MI355X on the n = 300 models below, worst of both components, boxes and kernels; the bar
# is 4 x that (and never looser than 2e-2).
# ghat 5.2e-6 / 1.4e-6 / 5.81e-6, gvar 1.5e-6 / 8.8e-7 / 2.0e-6 (Matern-3/2 / SE / Matern-5/2)
MEASURED_F32 = 5.81e-6
F32_BAR = 4 * MEASURED_F32


@pytest.mark.parametrize('kernel', ['matern32', 'se', 'matern52'])
def test_float32_model_against_the_float64_restatement(kernel):
    m32, x = _model('full', kernel, 3, dtype='float32')
    m64, _ = _model('full', kernel, 3)
    e32, e64 = m32._ensure_aux(), m64._ensure_aux()
    x0s, mask = _rows(3)
    errs = []
    for box in _boxes(3):
        got = e32.predict_marginal_block(x0s, mask, box).cpu().numpy()
        for k, (gh, gv) in enumerate(_restated(m64, _factors(m64, e64), x0s, mask, box)):
            for h, want, what in ((0, gh, 'ghat'), (1, gv, 'gvar')):
                errs.append(np.max(np.abs(got[h, k] - want)) / np.max(np.abs(want)))
                print('float32', kernel, k, what, errs[-1])
    assert F32_BAR <= 2e-2
    assert max(errs) <= F32_BAR, errs


def test_main_effects_end_to_end():
    """n = 300, d = 3, p = 3, q = 2, SE: main_effects against predict_marginal on the same rows, to the bit; and .overall
    against the Gauss-Legendre mean of each main effect over its own input (the rule and bar of the test above)"""
    m, x = _model('full', 'se', 3)
    G = 9
    lo, span = m.x_min.numpy().reshape(-1), (m.x_max - m.x_min).numpy().reshape(-1)
    quad_box = lo + span * QUAD_BOX                              # the box the rule's deviation was recorded on
    for box in (None, quad_box):
        me = m.main_effects(grid=G, box=box)
        assert me.mean.shape == (3, 3, G) and me.overall.shape == (3,)
        x0 = np.full((3 * G + 1, 3), np.nan)
        mask = np.ones((3 * G + 1, 3), bool)
        for l in range(3):
            x0[l * G:(l + 1) * G, l] = me.grid.numpy()[l]
            mask[l * G:(l + 1) * G, l] = False
        yp, ycv = [t.numpy() for t in m.predict_marginal(x0, mask, box=box)]
        assert np.array_equal(me.mean.numpy(), yp[:, :-1].reshape(3, 3, G))
        assert np.array_equal(me.var.numpy(), ycv[:, :-1].reshape(3, 3, G))
        assert np.array_equal(me.overall.numpy(), yp[:, -1]) and np.array_equal(me.overall_var.numpy(), ycv[:, -1])
        assert np.array_equal(me.effect.numpy(), me.mean.numpy() - me.overall.numpy()[:, None, None])
        assert np.all(me.var.numpy() > 0) and np.all(me.overall_var.numpy() < np.min(me.var.numpy(), axis=(1, 2)))
    # (me: on quad_box) the overall mean is the average of each main effect over its own input; largest entry: of the effects
    for l in range(3):
        t, w = ref.gauss_legendre(GL_NODES, quad_box[0][l], quad_box[1][l])
        xg = np.full((GL_NODES, 3), np.nan)
        xg[:, l] = t
        mg = np.ones((GL_NODES, 3), bool)
        mg[:, l] = False
        avg = m.predict_marginal(xg, mg, box=quad_box)[0].numpy() @ w
        err = np.max(np.abs(avg - me.overall.numpy())) / np.max(np.abs(me.mean.numpy()))
        print('main effects', l, err)
        assert err <= 10.0 * CPU_QUAD_DEV, (l, err)
