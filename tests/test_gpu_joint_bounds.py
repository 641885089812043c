"""Stage-wise componentwise bounds of the joint path on the GPU (tests/stage_bounds.py), every run on three fills.

The C entries are called directly: lcgp_predict_cov -> the cross covariance X and U = X W^T read back from its scratch
(do_predict_cov's layout: q slabs of X, n0pad x npad, then q slabs of U) and Sigma + tau I fetched from the cov
workspace -> lcgp_potrf_logdet on the cov workspace -> its factor L and info words -> lcgp_sample_latent.  Before each
run the cov workspace, both scratch buffers, `out` and the info / half_logdet words are filled with 0x00, 0xFF (NaN in
both precisions) and 0x5A bytes in turn: X, U, Sigma, the padding of the matrix slot, L, info and the draws must be
bitwise identical over the fills, every info word 0, and every check of the 0xFF run must pass:
    cross (X), u (U), sigma (Sigma + tau I), cov_factor (the fetched Sigma + tau I and L), draws.
The factor is held to check_cholesky_inverse_solve, not check_cholesky: the library solves each panel with the explicit
inverse of its 64 x 64 diagonal block, and on an ill-conditioned Sigma (one training point: Sigma is nearly the smooth
prior) that solve's residual exceeds check_cholesky's kappa-free bound (ratio ~2 at n = 1, n0 = 256).
The padding rows of the matrix slot must hold the identity, before and after the factorisation (lcgp_hip.h).

Jitter.  tau = jitter scale_k.  float64: 1e-8, small against the nugget term scale nt >= 1e-4 scale that keeps the
exact Sigma definite, large enough that a tau taken from the wrong place exceeds the bound.  float32: Sigma = C00 -
D U U^T cancels, and the stored Sigma differs from the exact one by up to C (npad + d + E) u (|C00| + |D| |U| |U|^T),
~2e-4 scale at npad = 768 and more at the headline size; the smallest eigenvalue of the exact Sigma can be as small as
the nugget term (1e-4 scale here), so the default 1e-10 is not definite in float32.  1e-3 clears that error at every
size below with a margin, and the headline configuration (npad = 4096, its own nugget) gets 1e-2.

Run with -s to see the worst ratio per case group, dtype and stage."""
import ctypes as C
from collections import defaultdict

import numpy as np
import pytest
import torch

from lcgp_amd import LCGP, _hip, synth
from lcgp_amd.engine import PREDICT_CHUNK, SAMPLE_CHUNK, HotPathEngine
from tests import stage_bounds as sb
from tests.test_gpu_stage_bounds import FILLS, _bits, _config_problem, _fetch, _filled, _problem

pytestmark = pytest.mark.gpu

JITTER = {"float64": 1e-8, "float32": 1e-3}
JITTER_HEADLINE = {"float64": 1e-8, "float32": 1e-2}

WORST = defaultdict(lambda: sb.Check(0.0, ()))       # (group, dtype, stage) -> worst Check over the group's cases


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst ratio |error| / bound per case group, dtype and stage of the joint path (<= 1 passes)")
    for key in sorted(WORST):
        c = WORST[key]
        print("  %-15s %-8s %-11s %.3e  at %s" % (key + (c.ratio, c.where)))


def _record(group, dtype, stage, c, where_extra=None):
    key = (group, dtype, stage)
    if c.ratio >= WORST[key].ratio:
        WORST[key] = sb.Check(c.ratio, (where_extra,) + tuple(c.where) if where_extra is not None else c.where)
    assert c.ratio <= 1.0, (group, dtype, stage, c, where_extra)


def _bytes(fn, *args):
    nbytes = C.c_size_t(0)
    _hip.check(fn(*args, C.byref(nbytes)), fn.__name__ if hasattr(fn, "__name__") else "bytes")
    return int(nbytes.value)


def _slot(eng, cws, n0):
    """(q_local, n0pad, n0pad) view of the matrix slot of the cov workspace (offset 0 of a workspace carved for n0)"""
    n0pad = sb._pad128(n0)
    return cws.view(eng.tdtype)[:eng.q_local * n0pad * n0pad].view(eng.q_local, n0pad, n0pad)


def _fetch_cov(eng, cws, n0):
    out = torch.empty((eng.q_local, n0, n0), dtype=eng.tdtype, device=eng.device)
    for k in range(eng.q_local):
        _hip.check(eng.lib.lcgp_fetch_matrix(eng._stream(), eng.dtype, n0, eng.d, eng.p, eng.q_local, eng._p(cws), 0, k,
                                             eng._p(out[k])), "lcgp_fetch_matrix")
    return out


def _run_joint(eng, fill, x0, same, jitter, eps, ghat):
    """lcgp_predict_cov -> lcgp_potrf_logdet -> lcgp_sample_latent on freshly filled memory; everything the checks read"""
    q, n0, S = eng.q_local, x0.shape[0], eps.shape[1]
    n0pad, npad = sb._pad128(n0), sb._pad128(eng.n)
    lib, dev = eng.lib, eng.device
    r = {}
    with torch.cuda.device(dev):
        st = eng._stream()
        cws = _filled((_bytes(lib.lcgp_workspace_bytes, eng.dtype, n0, eng.d, eng.p, q),), torch.uint8, fill, dev)
        scratch = _filled((_bytes(lib.lcgp_predict_cov_scratch_bytes, eng.dtype, eng.n, q, n0),), torch.uint8, fill, dev)
        x0d = torch.as_tensor(np.ascontiguousarray(x0, np.float64)).to(dev, eng.tdtype).contiguous()
        _hip.check(lib.lcgp_predict_cov(st, eng.dtype, eng.kernel_id, eng.n, eng.d, eng.p, q, eng._p(eng.x), eng._p(eng.sr),
                                        eng._p(eng.theta_dev), eng._p(eng.workspace), n0, eng._p(x0d), int(same),
                                        eng._p(scratch), eng._p(cws), float(jitter)), "lcgp_predict_cov")
        slab = n0pad * npad
        sc = scratch.view(eng.tdtype)
        r["X"] = sc[:q * slab].view(q, n0pad, npad)[:, :n0, :eng.n].clone()
        r["U"] = sc[q * slab:2 * q * slab].view(q, n0pad, npad)[:, :n0, :eng.n].clone()
        del scratch, sc
        r["sigma"] = _fetch_cov(eng, cws, n0)
        r["sigma_pad"] = torch.tril(_slot(eng, cws, n0))[:, n0:, :].clone()
        hl = _filled((q,), torch.float64, fill, dev)
        info = _filled((q,), torch.int32, fill, dev)
        _hip.check(lib.lcgp_potrf_logdet(st, eng.dtype, n0, eng.d, eng.p, q, eng._p(cws), eng._p(hl), eng._p(info), None, None),
                   "lcgp_potrf_logdet")
        r["info"] = info.clone()
        r["L"] = _fetch_cov(eng, cws, n0)
        r["L_pad"] = torch.tril(_slot(eng, cws, n0))[:, n0:, :].clone()
        sscr = _filled((_bytes(lib.lcgp_sample_scratch_bytes, eng.dtype, n0, q, S),), torch.uint8, fill, dev)
        out = _filled((q, S, n0), torch.float64, fill, dev)
        epsd = torch.as_tensor(np.ascontiguousarray(eps)).to(dev, eng.tdtype).contiguous()
        _hip.check(lib.lcgp_sample_latent(st, eng.dtype, n0, eng.d, eng.p, q, S, eng._p(cws), eng._p(epsd), eng._p(ghat), n0,
                                          eng._p(sscr), eng._p(out)), "lcgp_sample_latent")
        r["draws"] = out.clone()
    return r


def _poisoned(eng, x0, same, jitter, eps, ghat):
    base = _run_joint(eng, 0xFF, x0, same, jitter, eps, ghat)
    for f in FILLS:
        if f == 0xFF:
            continue
        other = _run_joint(eng, f, x0, same, jitter, eps, ghat)
        for key in base:
            assert torch.equal(_bits(other[key]), _bits(base[key])), ("fill 0x%02X changes" % f, key)
        del other
    return base


def _joint_case(group, eng, x, sr, th, kernel, dtype, x0, S, same=0, jitter=None, comps=None, seed=0):
    """the three-fill run at x0 and every check for the components `comps` (default: all)"""
    q, n0 = eng.q_local, x0.shape[0]
    jitter = JITTER[dtype] if jitter is None else jitter
    comps = range(q) if comps is None else comps
    eps = np.random.default_rng(seed).standard_normal((q, S, n0))
    ghat = eng.predict_block(x0, same)[0].contiguous()
    r = _poisoned(eng, x0, same, jitter, eps, ghat)
    assert torch.all(r["info"] == 0), (group, dtype, n0, r["info"])
    n0pad = sb._pad128(n0)
    ident = torch.eye(n0pad, dtype=eng.tdtype, device=eng.device)[n0:, :]
    for key in ("sigma_pad", "L_pad"):            # identity on the padding (lower tiles), exactly
        assert torch.equal(r[key], ident.expand_as(r[key])), (group, dtype, n0, key)
    for k in comps:
        tag = "n0=%d k%d" % (n0, k)
        W = _fetch(eng, 1, k, True)
        X, U, Sg, L = r["X"][k], r["U"][k], r["sigma"][k], r["L"][k]
        _record(group, dtype, "cross", sb.check_cov_cross(X, x0, x, sr, th[k], kernel, dtype, same), tag)
        _record(group, dtype, "u", sb.check_cov_u(U, X, W, dtype), tag)
        _record(group, dtype, "sigma", sb.check_sigma(Sg, U, x0, th[k], jitter, kernel, dtype), tag)
        _record(group, dtype, "cov_factor", sb.check_cholesky_inverse_solve(Sg, L, dtype), tag)
        _record(group, dtype, "draws", sb.check_draws(r["draws"][k], L, eps[k], ghat[k], dtype), tag)
        del W
    return r


def _engine(seed, n, d, q, dtype, kernel="matern32", rep=False):
    x, Y, sr, th = _problem(seed, n, d, 3, q, rep=rep)
    eng = HotPathEngine(x, Y, sr=sr, q_local=q, dtype=dtype, kernel=kernel)
    out = eng.evaluate(th)
    assert np.all(out[:, 2] == 0), out[:, 2]
    return eng, x, sr, th


def _x0(seed, n0, d):
    return np.random.default_rng(seed).uniform(-0.1, 1.1, (n0, d))


# ----------------------------------------------------------------------------------------------------------------------
BOUNDARY_N0 = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 255, 256, 257, 383, 384, 385, 1025)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", [1, 129, 700])
def test_tile_and_panel_boundaries_of_n0(dtype, n):
    """n0 at every 64 / 128-tile edge, n at 1, past one 128-tile and at several; q_local = 3 with its own theta each"""
    eng, x, sr, th = _engine(700 + n, n, 3, 3, dtype)
    for i, n0 in enumerate(BOUNDARY_N0):
        _joint_case("boundary", eng, x, sr, th, "matern32", dtype, _x0(800 + i, n0, 3), 5, seed=i)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_draw_counts(dtype):
    """S at the 128-row tiles of the draw product (eps padded to Spad = S rounded up to 128)"""
    eng, x, sr, th = _engine(901, 300, 3, 3, dtype)
    for n0 in (65, 257):
        for S in (1, 127, 128, 129, 300):
            _joint_case("draw_counts", eng, x, sr, th, "matern32", dtype, _x0(902 + S, n0, 3), S, seed=S)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("rep", [False, True], ids=["full", "rep"])
def test_training_set_as_x0(dtype, rep):
    """x0 = the engine's own inputs (the training set on the full path, x_unique on the rep path), same = 1: the nugget
    term is on the diagonal of the cross covariance too"""
    eng, x, sr, th = _engine(903, 257, 3, 3, dtype, rep=rep)
    _joint_case("training_x0", eng, x, sr, th, "matern32", dtype, x, 130, same=1)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_se_kernel_and_replicated_path(dtype):
    eng, x, sr, th = _engine(904, 500, 3, 3, dtype, kernel="se")
    _joint_case("se", eng, x, sr, th, "se", dtype, _x0(905, 257, 3), 129)
    eng, x, sr, th = _engine(906, 500, 3, 3, dtype, rep=True)
    _joint_case("rep", eng, x, sr, th, "matern32", dtype, _x0(907, 257, 3), 129)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_matern52_kernel(dtype):
    """Matern-5/2: one pass of the `boundary` case list (n = 129, every n0 of BOUNDARY_N0) and one of `training_x0` (n = 257,
    same = 1), q_local = 3; cross, u, sigma, cov_factor and draws of every component"""
    eng, x, sr, th = _engine(915, 129, 3, 3, dtype, kernel="matern52")
    for i, n0 in enumerate(BOUNDARY_N0):
        _joint_case("boundary_m52", eng, x, sr, th, "matern52", dtype, _x0(920 + i, n0, 3), 5, seed=i)
    eng, x, sr, th = _engine(916, 257, 3, 3, dtype, kernel="matern52")
    _joint_case("training_x0_m52", eng, x, sr, th, "matern52", dtype, x, 130, same=1)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_headline_configuration(dtype):
    """configs[2] (n = 4096, d = 6, q = 8) with its own data, standardisation and parameters, n0 = 2000, S = 128, every
    component"""
    m, eng, x, Y, th = _config_problem(3, dtype)
    out = eng.evaluate(th)
    assert np.all(out[:, 2] == 0), out[:, 2]
    lo, hi = x.min(axis=0), x.max(axis=0)
    x0 = lo + (hi - lo) * np.random.default_rng(908).uniform(0.0, 1.0, (2000, x.shape[1]))
    _joint_case("headline", eng, x, None, th, "matern32", dtype, x0, 128, jitter=JITTER_HEADLINE[dtype])
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_chunk_split_of_the_draws(dtype):
    """HotPathEngine.sample_latent with S = SAMPLE_CHUNK + 1: two lcgp_sample_latent calls.  The draws meet check_draws
    against eps regenerated from default_rng(seed), and the first SAMPLE_CHUNK equal an S = SAMPLE_CHUNK call bitwise."""
    eng, x, sr, th = _engine(909, 300, 3, 2, dtype)
    x0 = _x0(910, 65, 3)
    seeds = [(5, 0), (5, 1)]
    jit = JITTER[dtype]
    S = SAMPLE_CHUNK + 1
    g = eng.sample_latent(x0, S, seeds, jitter=jit)
    L = eng.fetch_cov(65)
    ghat = eng.predict_block(x0)[0]
    for k in range(2):
        eps = np.random.default_rng(seeds[k]).standard_normal((S, 65))
        _record("sample_chunks", dtype, "draws", sb.check_draws(g[k], L[k], eps, ghat[k], dtype), "S=%d k%d" % (S, k))
    g0 = eng.sample_latent(x0, SAMPLE_CHUNK, seeds, jitter=jit)
    assert torch.equal(_bits(g[:, :SAMPLE_CHUNK]), _bits(g0))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_predict_chunk_split_of_ghat(dtype):
    """n0 = PREDICT_CHUNK + 52: sample_latent computes ghat in two lcgp_predict calls, Sigma in one; the draws meet
    check_draws against predict()'s ghat"""
    eng, x, sr, th = _engine(911, 300, 3, 2, dtype)
    n0 = PREDICT_CHUNK + 52
    x0 = _x0(912, n0, 3)
    seeds = [(6, 0), (6, 1)]
    g = eng.sample_latent(x0, 16, seeds, jitter=JITTER[dtype])
    L = eng.fetch_cov(n0)
    ghat, _ = eng.predict(x0)
    for k in range(2):
        eps = np.random.default_rng(seeds[k]).standard_normal((16, n0))
        _record("ghat_chunks", dtype, "draws", sb.check_draws(g[k], L[k], eps, ghat[k], dtype), "k%d" % k)


def test_float32_model_diagonal_and_draws():
    """LCGP(dtype='float32'): diag(predict_latent_cov) against predict()'s gvar.  Both are scale - D |U_i|^2 from the same
    float32 X and W, reduced in different orders (the tile kernel, the predict reduction), each within
    C (npad + d + E_i) u (scale + |D| |U_i|^2) of the exact value; |D| |U_i|^2 = scale - gvar_i up to that error, so
        |diag - gvar| <= 2 C (npad + d + E_i) u (2 scale + |scale - gvar_i|)
    (E_i: the largest kernel magnification of row i).  sample() at jitter 1e-3 (see the module docstring) is finite."""
    x, y = synth.make_full(913, 600, 2, 4, 3)
    m = LCGP(y=y, x=x, q=3, dtype='float32')
    m.float32_fallback = False
    m._set_flat(synth.param_points(913, m._get_flat())[1])
    x0 = np.random.default_rng(914).uniform(0, 1, (300, 2))
    lc = m.predict_latent_cov(x0).numpy()
    m.predict(x0)
    gvar = m.gvar.numpy()
    eng = m._aux_engine
    assert eng is not None and eng.tdtype == torch.float32
    x0s, _ = m._standardise_x0(x0)
    xe = eng.x.to(torch.float64).cpu().numpy()
    th = eng.theta_dev.cpu().numpy()
    d, u, npad = eng.d, sb.unit("float32"), sb._pad128(eng.n)
    for k in range(m.q):
        ell, scale = th[k, :d], th[k, d]
        e = sb.kernel_parts(sb.rounded(x0s, "float32"), xe, ell, "matern32", "float32")[1].max(dim=1).values.numpy()
        bound = 2 * sb.C * (npad + d + e) * u * (2 * abs(scale) + np.abs(scale - gvar[k]))
        r = np.max(np.abs(np.diag(lc[k]) - gvar[k]) / bound)
        _record("model_f32", "float32", "diag_gvar", sb.Check(float(r), ("k%d" % k,)))
    s = m.sample(x0, size=50, seed=3, jitter=1e-3).numpy()
    assert s.shape == (50, m.p, 300) and np.all(np.isfinite(s))
