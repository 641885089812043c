"""Stage-wise componentwise bounds of the hot path on the GPU (tests/stage_bounds.py), every evaluation on three workspace
fills.

Each case evaluates one parameter point three times on the same engine: on a workspace (and predict scratch) filled with
zero bytes, with 0xFF bytes (NaN in both precisions) and with 0x5A bytes (huge finite values, which min / max would not
drop silently).  The C ABI promises nothing about the workspace's content on entry, so the output block, the fetched A,
L, L^-1, A^-1, b, z and the predictions must be bitwise identical over the three fills; a tile a schedule fails to write
shows up as NaN or as a difference.  The results of the 0xFF run then go through every stage check: build, Cholesky
residual, half_logdet, L^-1, A^-1, z, quad / gradient / gsig, predictions.  (The poison never becomes an address: the
only integer of the workspace is the info word, which the build launch -- or zero_stats_kernel when lcgp_potrf_logdet
runs on its own -- resets before anything reads it.)

Coverage of the input dimension.  build_kernel<T, DD, KERN> and grad_kernel<T, DD, KERN> are compiled per for_dim bucket
DD = 2, 4, 6, 10, 16, 32; d > 32 runs build_kernel<T, 32, KERN> in chunks of 32 dimensions and grad_kernel_wide<T, KERN>.
With T = double, float and KERN = Matern-3/2, SE, Matern-5/2 that is 36 narrow (DD, KERN, T) instantiations and 6 wide
(KERN, T) ones.
  - test_every_dimension_bucket reaches all 42, the three kernels and both storage types, at d = 1, 2 (DD = 2), 3, 4 (DD = 4),
    5, 6 (DD = 6), 7, 9, 10 (DD = 10), 11, 15, 16 (DD = 16), 17, 31, 32 (DD = 32, one ragged or full chunk), and in the
    wide kernels at 2 chunks (d = 33, 63 ragged; 64 full), 3 (65 ragged; 96 full) and 4 (97, 126 ragged), n = 130.
  - test_wide_partials_over_many_tiles: 171 lower tiles of partials per component, q = 3: Matern-3/2 at DD = 16 (d = 16),
    DD = 32 (17, 32) and wide at 2 and 4 chunks (33, 126); SE at DD = 32 (17) and wide at 4 chunks (126); Matern-5/2 at
    DD = 10 (d = 10), 16 (16), 32 (17) and wide at 4 chunks (126); both types.
  - test_dimension_extremes: the wide kernels at 2 and 4 chunks (d = 33, 126), the three kernels, both types, with C0 past its
    cut-off (collapsed lengthscales) and with S_j ~ 0 in every chunk (a third of the lengthscales at 1e3).
  - test_matern52_cutoff_in_the_narrow_buckets: grad_kernel skips an entry whose exponent is below exp_floor only where
    DD > (KERN == 2 ? 8 : 16), so the buckets DD = 10 and 16 take that branch for Matern-5/2 alone: C0 around its cut-off
    at d = 6 (DD = 6, no skip), 7, 10 (DD = 10) and 16 (DD = 16), and every lengthscale at 1e-6 at d = 6, 10, 16 (the
    polynomial overflows float32, the exponential is zero: A is diagonal, the gradient finite).
  - test_replicated_path_dimensions: sr != 1 at DD = 6 (d = 5), DD = 32 (17) and wide at 4 chunks (126), the three kernels,
    both types.
  - test_tile_panel_and_pair_boundaries (Matern-3/2 at DD = 2, 4, 6, 10 and wide at 2 chunks),
    test_se_kernel_and_replicated_path and test_matern52_kernel (DD = 4) at the tile and panel edges of n.
Predictions at the training inputs: test_predict_at_training_inputs calls lcgp_predict with x0 = x[lo : lo + m] and
same = 1 + lo (lo at the 64-block and 128-pad edges and the last row; m = 1, 64, 65 and the whole set; n = 257 and 1025,
full and rep paths) and the engine's predict_block(x, same=True) at PREDICT_CHUNK = 64 and 128, through
check_predict(same).

Run with -s to see the worst ratio per stage, dtype and case group."""
import ctypes as C
from collections import defaultdict

import numpy as np
import pytest
import torch

from lcgp_amd import _hip
from lcgp_amd.engine import HotPathEngine
from tests import stage_bounds as sb

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0x5A)
PLAIN = dict(fill_leaf=0, fill_step=0, pair_tiles=0, progressive_tiles=0, leaf_in_wide=0)
FORCE128 = dict(syrk_small_tiles=1, trtri_small_tiles=0, trtri_level_small=0, lauum_small_tiles=0)
FORCE64 = dict(syrk_small_tiles=100000, trtri_small_tiles=100000, trtri_level_small=100000, lauum_small_tiles=100000)

WORST = defaultdict(lambda: sb.Check(0.0, ()))       # (group, dtype, stage) -> worst Check over the group's cases


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst ratio |error| / bound per case group, dtype and stage (<= 1 passes)")
    for key in sorted(WORST):
        c = WORST[key]
        print("  %-13s %-8s %-15s %.3e  at %s" % (key + (c.ratio, c.where)))


def _sched(**fields):
    sc = _hip.default_sched()
    for k, v in fields.items():
        assert hasattr(sc, k), k
        setattr(sc, k, v)
    return sc


def _problem(seed, n, d, p, q, D=(1.0, 20.0), ell=(-1.5, 0.3), nug=(-4.0, -2.0), rep=False):
    """inputs in the unit box, random outputs, theta rows [ell | scale | nug | D | psi] (the engine's layout)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (n, d))
    Y = rng.standard_normal((p, n))
    sr = np.sqrt(rng.integers(1, 6, n).astype(np.float64)) if rep else None
    th = np.zeros((q, d + 3 + p))
    for k in range(q):
        th[k, :d] = np.sqrt(d) * np.exp(rng.uniform(*ell, d))
        th[k, d] = rng.uniform(0.5, 2.0)
        th[k, d + 1] = 10.0 ** rng.uniform(*nug)
        th[k, d + 2] = rng.uniform(*D)
        th[k, d + 3:] = rng.standard_normal(p) / np.sqrt(p)
    return x, Y, sr, th


def _fetch(eng, which, k, matrix):
    n = eng.n
    out = torch.empty((n, n) if matrix else (n,), dtype=eng.tdtype, device=eng.device)
    fn = eng.lib.lcgp_fetch_matrix if matrix else eng.lib.lcgp_fetch_vector
    _hip.check(fn(eng._stream(), eng.dtype, n, eng.d, eng.p, eng.q_local, eng._p(eng.workspace), int(which), int(k),
                  eng._p(out)), "lcgp_fetch")
    return out


def _filled(shape, dtype, fill, device):
    """a tensor whose every byte is `fill`"""
    t = torch.empty(shape, dtype=dtype, device=device)
    t.view(torch.uint8).fill_(fill)
    return t


def _predict(eng, x0, fill, same=0):
    """lcgp_predict (one call: n0 <= PREDICT_CHUNK) with its scratch AND its ghat / gvar rows filled with `fill`, so a
    slot the library does not write keeps the poison and differs between the fills.  same: as in the C ABI (0 = new
    inputs; else x0 is x[same - 1 : same - 1 + n0])"""
    n0 = x0.shape[0]
    nbytes = C.c_size_t(0)
    _hip.check(eng.lib.lcgp_predict_scratch_bytes(eng.dtype, eng.n, eng.q_local, n0, C.byref(nbytes)), "scratch")
    scratch = _filled((int(nbytes.value),), torch.uint8, fill, eng.device)
    out = _filled((2, eng.q_local, n0), torch.float64, fill, eng.device)
    x0d = torch.as_tensor(np.ascontiguousarray(x0, np.float64)).to(eng.device, eng.tdtype).contiguous()
    _hip.check(eng.lib.lcgp_predict(eng._stream(), eng.dtype, eng.kernel_id, eng.n, eng.d, eng.p, eng.q_local, eng._p(eng.x),
                                    eng._p(eng.sr), eng._p(eng.theta_dev), eng._p(eng.workspace), n0, eng._p(x0d), int(same),
                                    eng._p(scratch), eng._p(out[0]), eng._p(out[1]), n0), "lcgp_predict")
    return out


def _run_nll(eng, th, fill, comps, x0):
    """build (A), then the whole path on a freshly poisoned workspace and output block (out, L, L^-1, A^-1, b, z) and
    the predictions (x0 = None: none)"""
    r = {}
    eng.workspace.fill_(fill)
    eng.upload_theta(th)
    with torch.cuda.device(eng.device):
        _hip.check(eng.lib.lcgp_kernel_build(eng._stream(), eng.dtype, eng.kernel_id, eng.n, eng.d, eng.p, eng.q_local,
                                             eng._p(eng.x), eng._p(eng.sr), eng._p(eng.theta_dev), eng._p(eng.workspace)),
                   "lcgp_kernel_build")
        for k in comps:
            r["A", k] = _fetch(eng, 0, k, True)
        eng.workspace.fill_(fill)
        eng.out_dev.view(torch.uint8).fill_(fill)
        eng.enqueue()
        r["out"] = eng.out_dev.clone()
        for k in comps:
            r["L", k], r["W", k], r["V", k] = (_fetch(eng, w, k, True) for w in (0, 1, 2))
            r["b", k], r["z", k] = _fetch(eng, 0, k, False), _fetch(eng, 1, k, False)
        if x0 is not None:
            r["pred"] = _predict(eng, x0, fill)
    return r


def _run_stages(eng, th, fill, comps):
    """the stage-by-stage ABI path: lcgp_kernel_build, lcgp_potrf_logdet (a plan without the inverse), lcgp_trtri, lcgp_lauum"""
    r = {}
    eng.workspace.fill_(fill)
    eng.upload_theta(th)
    q = eng.q_local
    with torch.cuda.device(eng.device):
        st = eng._stream()
        args = (eng.dtype, eng.n, eng.d, eng.p, q)
        _hip.check(eng.lib.lcgp_kernel_build(st, eng.dtype, eng.kernel_id, eng.n, eng.d, eng.p, q, eng._p(eng.x),
                                             eng._p(eng.sr), eng._p(eng.theta_dev), eng._p(eng.workspace)), "kernel_build")
        for k in comps:
            r["A", k] = _fetch(eng, 0, k, True)
        hl = _filled((q,), torch.float64, fill, eng.device)
        info = _filled((q,), torch.int32, fill, eng.device)
        _hip.check(eng.lib.lcgp_potrf_logdet(st, *args, eng._p(eng.workspace), eng._p(hl), eng._p(info), eng._sched(), None),
                   "potrf_logdet")
        _hip.check(eng.lib.lcgp_trtri(st, *args, eng._p(eng.workspace), eng._sched()), "trtri")
        _hip.check(eng.lib.lcgp_lauum(st, *args, eng._p(eng.workspace), eng._sched()), "lauum")
        r["half_logdet"], r["info"] = hl.clone(), info.clone()
        for k in comps:
            r["L", k], r["W", k], r["V", k] = (_fetch(eng, w, k, True) for w in (0, 1, 2))
    return r


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _poisoned(run, *args):
    """the run on the three fills; asserts bitwise equality and returns the 0xFF run (one other run held at a time)"""
    base = run(*args[:2], 0xFF, *args[2:])
    for f in FILLS:
        if f == 0xFF:
            continue
        other = run(*args[:2], f, *args[2:])
        assert other.keys() == base.keys()
        for key in base:
            assert torch.equal(_bits(other[key]), _bits(base[key])), ("fill 0x%02X changes" % f, key)
        del other
    return base


def _record(group, dtype, stage, c, where_extra=None):
    key = (group, dtype, stage)
    if c.ratio >= WORST[key].ratio:
        WORST[key] = sb.Check(c.ratio, (where_extra,) + tuple(c.where) if where_extra is not None else c.where)
    assert c.ratio <= 1.0, (group, dtype, stage, c, where_extra)


def _check_all(group, eng, x, Y, sr, th, kernel, dtype, r, comps, x0):
    out = r["out"].cpu().numpy()
    pred = r["pred"]
    for k in comps:
        A, L, W, V, b, z = (r[s, k] for s in ("A", "L", "W", "V", "b", "z"))
        assert out[k, 2] == 0, ("info", k, out[k, 2])
        tag = "n%d d%d k%d" % (x.shape[0], x.shape[1], k)
        _record(group, dtype, "build", sb.check_build(A, b, x, Y, sr, th[k], kernel, dtype), tag)
        _record(group, dtype, "cholesky", sb.check_cholesky(A, L, dtype), tag)
        _record(group, dtype, "half_logdet", sb.check_half_logdet(L, out[k, 0], dtype), tag)
        _record(group, dtype, "inverse_factor", sb.check_inverse_factor(L, W, dtype), tag)
        _record(group, dtype, "inverse", sb.check_inverse(W, V, dtype), tag)
        _record(group, dtype, "z", sb.check_z(V, b, z, dtype), tag)
        _record(group, dtype, "outputs", sb.check_outputs(out[k], x, Y, sr, th[k], V, b, z, kernel, dtype), tag)
        _record(group, dtype, "predict", sb.check_predict(pred[0, k], pred[1, k], x0, x, sr, th[k], W, z, kernel, dtype), tag)


def _comps(n, q):
    return list(range(q)) if n <= 2000 else sorted({0, q - 1})


def _case(group, dtype, n, d, p, q, seed, scheds, kernel="matern32", rep=False, theta=None, **prob):
    """theta: a function th -> th applied to _problem's parameter rows (knobs _problem does not have)"""
    x, Y, sr, th = _problem(seed, n, d, p, q, rep=rep, **prob)
    if theta is not None:
        th = theta(th)
    x0 = np.random.default_rng(seed + 1).uniform(-0.1, 1.1, (37, d))
    eng = HotPathEngine(x, Y, sr=sr, q_local=q, dtype=dtype, kernel=kernel)
    comps = _comps(n, q)
    for fields in scheds:
        eng.sched = _sched(**fields)
        r = _poisoned(_run_nll, eng, th, comps, x0)
        _check_all(group, eng, x, Y, sr, th, kernel, dtype, r, comps, x0)
    return eng


# ----------------------------------------------------------------------------------------------------------------------
BOUNDARY_N = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 385, 511, 512, 513, 1023, 1025)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_tile_panel_and_pair_boundaries(dtype):
    """n at every 64 / 128-tile and panel edge (float64 panels are 256 columns wide, float32 512), with the default and the
    plainest schedule; q cycles over 1, 2, 3, 5 and d over 1, 3, 6, 10, 33"""
    for i, n in enumerate(BOUNDARY_N):
        q, d = (1, 2, 3, 5)[i % 4], (1, 3, 6, 10, 33)[i % 5]
        _case("boundary", dtype, n, d, 3, q, 100 + i, ({}, PLAIN))


# the schedule variants of tests/test_gpu_edge_cases.py and tools/sched_fuzz.py, deduplicated, grouped by the size they
# were written for
P30 = 1 << 30
VARIANTS_700 = (
    {}, PLAIN, dict(outer_blocks=1), dict(outer_blocks=2), dict(outer_blocks=3), dict(outer_blocks=8),
    dict(fill_leaf=16, fill_step=24), dict(leaf_in_wide=100000), dict(leaf_in_wide=100000, outer_blocks=2),
    dict(trtri_level_small=0), dict(trtri_level_small=100000, trtri_small_tiles=0), dict(lauum_small_tiles=0),
    dict(lauum_small_tiles=100000, trtri_small_tiles=100000),
    dict(pair_tiles=1, progressive_tiles=0), dict(pair_tiles=1, progressive_tiles=0, leaf_in_wide=0),
    dict(pair_tiles=1, progressive_tiles=0, leaf_in_wide=0, outer_blocks=2, fill_leaf=4, fill_step=4),
    dict(progressive_tiles=P30), dict(progressive_tiles=P30, outer_blocks=2), dict(progressive_tiles=P30, outer_blocks=8),
    dict(progressive_tiles=P30, fill_leaf=0, fill_step=0), dict(progressive_tiles=P30, fill_leaf=12, fill_step=20),
    dict(progressive_tiles=P30, progressive_far=0), dict(progressive_tiles=P30, leaf_in_wide=0),
    dict(progressive_tiles=P30, outer_blocks=3), dict(progressive_tiles=P30, progressive_lauum=0),
    dict(progressive_tiles=P30, progressive_lauum=0, outer_blocks=2), FORCE64, FORCE128)
VARIANTS_1500 = (
    {}, PLAIN, dict(syrk_small_tiles=16), dict(syrk_small_tiles=16, leaf_in_wide=0), dict(syrk_small_tiles=16, leaf_in_wide=100000),
    dict(syrk_small_tiles=16, fill_leaf=40, fill_step=56), dict(syrk_small_tiles=16, outer_blocks=2),
    dict(syrk_small_tiles=16, outer_blocks=8), dict(syrk_small_tiles=200, leaf_in_wide=300), dict(syrk_small_tiles=1, fill_leaf=8, fill_step=8),
    dict(pair_tiles=1, progressive_tiles=0, leaf_in_wide=0), dict(pair_tiles=1, progressive_tiles=0, leaf_in_wide=0, syrk_small_tiles=16),
    dict(pair_tiles=1, progressive_tiles=0, leaf_in_wide=0, fill_leaf=8, fill_step=8, outer_blocks=2),
    dict(pair_tiles=1, progressive_tiles=0, leaf_in_wide=0, fill_leaf=8, fill_step=8, syrk_small_tiles=16),
    dict(pair_tiles=50, progressive_tiles=0, fill_leaf=3, fill_step=5, outer_blocks=6),
    dict(progressive_tiles=P30, syrk_small_tiles=16), dict(progressive_tiles=P30, progressive_far=0, syrk_small_tiles=16),
    dict(progressive_tiles=P30, fill_leaf=40, fill_step=56), dict(progressive_tiles=P30, outer_blocks=8),
    dict(progressive_tiles=P30, progressive_lauum=0, syrk_small_tiles=16), FORCE64, FORCE128)
VARIANTS_2113 = (
    {}, PLAIN, dict(progressive_tiles=P30), dict(progressive_tiles=P30, fill_leaf=6, fill_step=6),
    dict(progressive_tiles=P30, progressive_far=0), dict(progressive_tiles=P30, progressive_lauum=0, fill_leaf=30, fill_step=18),
    dict(pair_tiles=1, progressive_tiles=0, leaf_in_wide=0, syrk_small_tiles=16), dict(FORCE128, outer_blocks=8), FORCE64)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n,q,variants", [(700, 4, VARIANTS_700), (1500, 4, VARIANTS_1500), (2113, 6, VARIANTS_2113)],
                         ids=["n700", "n1500", "n2113"])
def test_every_schedule_variant(dtype, n, q, variants):
    _case("schedules", dtype, n, 3, 5, q, 200 + n, variants)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", [257, 1500])
@pytest.mark.parametrize("tiles", ["64", "128"])
def test_stage_by_stage_abi(dtype, n, tiles):
    """lcgp_kernel_build, lcgp_potrf_logdet, lcgp_trtri, lcgp_lauum as separate calls, 64- or 128-tile kernels forced"""
    q, d = 3, 3
    x, Y, sr, th = _problem(300 + n, n, d, 4, q)
    eng = HotPathEngine(x, Y, q_local=q, dtype=dtype)
    eng.sched = _sched(**(FORCE64 if tiles == "64" else FORCE128))
    comps = _comps(n, q)
    r = _poisoned(_run_stages, eng, th, comps)
    assert torch.all(r["info"] == 0), r["info"]
    hl = r["half_logdet"].cpu().numpy()
    for k in comps:
        A, L, W, V = (r[s, k] for s in ("A", "L", "W", "V"))
        _record("abi_stages", dtype, "build", sb.check_build(A, None, x, Y, sr, th[k], "matern32", dtype), k)
        _record("abi_stages", dtype, "cholesky", sb.check_cholesky(A, L, dtype), k)
        _record("abi_stages", dtype, "half_logdet", sb.check_half_logdet(L, hl[k], dtype), k)
        _record("abi_stages", dtype, "inverse_factor", sb.check_inverse_factor(L, W, dtype), k)
        _record("abi_stages", dtype, "inverse", sb.check_inverse(W, V, dtype), k)


@pytest.mark.parametrize("dtype,kappa", [("float64", 1e10), ("float32", 1e5)])
def test_ill_conditioned(dtype, kappa):
    """kappa(A) ~ D scale n for smooth C: large D, long lengthscales, the smallest nugget; the componentwise Cholesky bound
    does not depend on kappa"""
    n = 700
    _case("conditioning", dtype, n, 2, 3, 2, 401, ({}, PLAIN), D=(kappa / n, kappa / n), ell=(1.0, 1.2), nug=(-7.0, -7.0))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_near_duplicate_and_collapsed_inputs(dtype):
    """rows of x 1e-7 apart (C almost singular off the nugget), and every lengthscale at 1e-6 (C0 past the cut-off:
    the polynomial may overflow while the exponential underflows; A is the identity plus the nugget term)"""
    n, d = 500, 3
    x, Y, sr, th = _problem(402, n, d, 3, 2)
    x[100:180] = x[300:380] + 1e-7
    eng = HotPathEngine(x, Y, q_local=2, dtype=dtype)
    x0 = np.random.default_rng(403).uniform(0.0, 1.0, (37, d))
    for ell in (None, 1e-6):
        t = th.copy()
        if ell is not None:
            t[:, :d] = ell
        for fields in ({}, PLAIN):
            eng.sched = _sched(**fields)
            r = _poisoned(_run_nll, eng, t, [0, 1], x0)
            _check_all("duplicates" if ell is None else "collapsed", eng, x, Y, sr, t, "matern32", dtype, r, [0, 1], x0)
    _case("collapsed", dtype, 300, 10, 4, 2, 404, ({},), ell=(np.log(1e-6 / np.sqrt(10)),) * 2)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", [200, 1025])
def test_se_kernel_and_replicated_path(dtype, n):
    _case("se", dtype, n, 3, 4, 2, 500 + n, ({}, PLAIN), kernel="se")
    _case("rep", dtype, n, 3, 4, 2, 600 + n, ({}, PLAIN), rep=True)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", [200, 1025])
def test_matern52_kernel(dtype, n):
    _case("m52", dtype, n, 3, 4, 2, 650 + n, ({}, PLAIN), kernel="matern52")


def _config_problem(c, dtype, n=None):
    """configs[c - 1] of the benchmark (synth.make_config(c): its own data, q and standardisation) at the second parameter
    point of synth.param_points, optionally cut to its first n points: the model's engine and its theta rows"""
    from lcgp_amd import LCGP, synth
    x, y, cfg = synth.make_config(c)
    if n is not None:
        x, y = x[:n], y[:, :n]
    m = LCGP(y=y, x=x, q=cfg['q'], dtype=dtype)
    m.float32_fallback = False
    m._set_flat(synth.param_points(c, m._get_flat())[1])
    eng = m._get_engine()
    sig_eff = np.exp(0.5 * np.repeat(m.lsigma2s.numpy(), np.asarray(m.diag_error_structure, int))) / m._std
    th = m._theta_rows(sig_eff)
    xs = eng.x.to(torch.float64).cpu().numpy()
    Ys = eng.Y.to(torch.float64).cpu().numpy()
    return m, eng, xs, Ys, th


@pytest.mark.parametrize("c,dtype,n", [(3, "float64", None), (4, "float32", 4096)], ids=["cfg2_fp64", "cfg3_prefix4096_fp32"])
def test_headline_configurations(c, dtype, n):
    """configs[2] (n = 4096, d = 6, p = 64, q = 8, float64) and the 4096-point prefix of configs[3] (d = 10, p = 32, q = 8,
    float32): the configurations' own data and standardisation, all eight components, default schedule, every stage"""
    m, eng, x, Y, th = _config_problem(c, dtype, n)
    q = eng.q_local
    x0 = x[:37] * 0.98 + 0.01
    r = _poisoned(_run_nll, eng, th, list(range(q)), x0)
    _check_all("headline", eng, x, Y, None, th, "matern32", dtype, r, list(range(q)), x0)


def test_cfg3_full_size_float32():
    """configs[3] at its full size (n = 16384, float32), components 0 and 7, on the three fills: A, the Cholesky residual,
    half_logdet, L^-1, A^-1 = W^T W and z, each entry against its bound (the float64 reference matrices live on the
    device: about 20 GB per check).  The output and predict checks stop at the 4096-point prefix above."""
    m, eng, x, Y, th = _config_problem(4, "float32")
    comps = [0, eng.q_local - 1]
    r = _poisoned(_run_nll, eng, th, comps, None)
    out = r["out"].cpu().numpy()
    g, dt = "cfg3_full", "float32"
    for k in comps:
        A, L, W, V, b, z = (r[s, k] for s in ("A", "L", "W", "V", "b", "z"))
        assert out[k, 2] == 0, ("info", k, out[k, 2])
        _record(g, dt, "build", sb.check_build(A, b, x, Y, None, th[k], "matern32", dt), k)
        _record(g, dt, "cholesky", sb.check_cholesky(A, L, dt), k)
        _record(g, dt, "half_logdet", sb.check_half_logdet(L, out[k, 0], dt), k)
        _record(g, dt, "inverse_factor", sb.check_inverse_factor(L, W, dt), k)
        _record(g, dt, "inverse", sb.check_inverse(W, V, dt), k)
        _record(g, dt, "z", sb.check_z(V, b, z, dt), k)
        del A, L, W, V, b, z
        torch.cuda.empty_cache()


# ----------------------------------------------------------------------------------------------------------------------
# input dimensions: every build_kernel / grad_kernel instantiation (for_dim: DD = 2, 4, 6, 10, 16, 32) and grad_kernel_wide
# with one to four 32-dimension chunks, both kernels, both storage types
# ----------------------------------------------------------------------------------------------------------------------
BUCKET_DIMS = (1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97, 126)
KERNELS = ("matern32", "se", "matern52")
GROUP = {"matern32": "m32", "se": "se", "matern52": "m52"}


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_every_dimension_bucket(dtype, kernel):
    """each for_dim bucket's edges and a padded interior point (DD = 2: 1, 2; 4: 3, 4; 6: 5, 6; 10: 7, 9, 10; 16: 11, 15,
    16; 32: 17, 31, 32) and the wide gradient at 1 .. 4 chunks, full and ragged (33, 63, 64, 65, 96, 97, 126); n = 130
    (three 64-blocks, the last ragged), q = 2, default and plainest schedule, every stage"""
    for i, d in enumerate(BUCKET_DIMS):
        _case("dim_" + GROUP[kernel], dtype, 130, d, 3, 2, 700 + i, ({}, PLAIN), kernel=kernel)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_wide_partials_over_many_tiles(dtype):
    """n = 1025 (npad = 1152: 171 lower tiles), q = 3: the per-tile gradient partials (stride DMAX + 2 narrow, d + 2 wide, a
    full 128-double slot at d = 126) of every component; a partial at the wrong stride or component offset lands in a
    neighbour's slot and fails that component's outputs check"""
    cases = ([("matern32", d) for d in (16, 17, 32, 33, 126)] + [("se", d) for d in (17, 126)] +
             [("matern52", d) for d in (10, 16, 17, 126)])
    for i, (kernel, d) in enumerate(cases):
        _case("tiles_" + GROUP[kernel], dtype, 1025, d, 3, 3, 800 + i, ({},), kernel=kernel)


def _cut_ell(d, dtype, kernel):
    """_problem's log-lengthscale band whose mean exponent is 1.1 times the C0 cut-off of the dtype (x uniform in the unit
    box: E|dx| = 1/3, E dx^2 = 1/6): 75 - 93 % of the entries pass the cut-off (at d = 126 all of those only once a later
    32-dimension chunk is summed, at d = 33 5 - 8 % only with dimension 32), and the rest sit close to it"""
    f = 1.1 * abs(sb.EXP_FLOOR[dtype])
    if kernel in ("matern32", "matern52"):          # the exponent is sum S in both
        ell = d / (3.0 * f)
    elif kernel == "se":
        ell = np.sqrt(d / (12.0 * f))
    else:
        raise ValueError(kernel)
    c = float(np.log(ell / np.sqrt(d)))
    return (c - 0.15, c + 0.15)


def _ard(th, d):
    """every third lengthscale at 1e3 (S ~ 1e-3: those dimensions barely count), spread over the chunks"""
    th = th.copy()
    th[:, 0:d:3] = 1e3
    return th


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_dimension_extremes(dtype):
    """d = 33 and 126, n = 257, every kernel: (a) collapsed lengthscales, most C0 entries past the exp cut-off, at d = 126
    only across chunk boundaries (_cut_ell); (b) ARD-style lengthscales, a third of the dimensions at 1e3 and the rest short: the
    wide kernel's prod / (1 + S_j) at S_j ~ 0 and exponent sums spread over every chunk.  A stays well conditioned (C0
    small off the diagonal, the nugget on it)"""
    for i, d in enumerate((33, 126)):
        for j, kernel in enumerate(KERNELS):
            seed = 900 + 10 * i + 2 * j
            _case("collapse_" + GROUP[kernel], dtype, 257, d, 3, 2, seed, ({},), kernel=kernel, ell=_cut_ell(d, dtype, kernel))
            _case("ard_" + GROUP[kernel], dtype, 257, d, 3, 2, seed + 1, ({},), kernel=kernel, ell=(-2.0, -0.5),
                  theta=lambda th, d=d: _ard(th, d))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_matern52_cutoff_in_the_narrow_buckets(dtype):
    """grad_kernel<T, DD, 2> leaves an entry out (`continue`) when its exponent is below exp_floor only for DD > 8, where
    Matern-3/2 and SE do so for DD > 16: DD = 10 and 16 have that branch for this kernel alone.  n = 257, q = 2.
    (a) C0 around its cut-off (_cut_ell) at d = 6 (DD = 6: no skip), 7 and 10 (DD = 10) and 16 (DD = 16);
    (b) every lengthscale at 1e-6 at d = 6, 10, 16 with D <= 2: S ~ 1e6 per dimension, f(S)^d overflows float32 (poly_cap and
    fmin must hold it) while the exponential is zero, so the off-diagonal of A is zero exactly and A the nugget diagonal;
    the output row is finite and within check_outputs (a NaN counts as inf there)."""
    n, q, p = 257, 2, 3
    for i, d in enumerate((6, 7, 10, 16)):
        _case("cutoff_m52", dtype, n, d, p, q, 960 + i, ({},), kernel="matern52", ell=_cut_ell(d, dtype, "matern52"))
    for i, d in enumerate((6, 10, 16)):
        x, Y, sr, th = _problem(970 + i, n, d, p, q, D=(1.0, 2.0))
        th[:, :d] = 1e-6
        x0 = np.random.default_rng(980 + i).uniform(-0.1, 1.1, (37, d))
        eng = HotPathEngine(x, Y, sr=sr, q_local=q, dtype=dtype, kernel="matern52")
        eng.sched = _sched()
        r = _poisoned(_run_nll, eng, th, [0, 1], x0)
        out = r["out"].cpu().numpy()
        assert np.all(np.isfinite(out)), (d, out)
        for k in range(q):
            A = r["A", k]
            assert torch.all(torch.isfinite(A)), (d, k)
            assert torch.count_nonzero(A - torch.diag(torch.diagonal(A))) == 0, (d, k)
        _check_all("collapsed_m52", eng, x, Y, sr, th, "matern52", dtype, r, [0, 1], x0)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_replicated_path_dimensions(dtype):
    """sr != 1 (replicates) at d = 5 (DD = 6), 17 (DD = 32) and 126 (four wide chunks), every kernel, n = 200"""
    for i, d in enumerate((5, 17, 126)):
        for j, kernel in enumerate(KERNELS):
            _case("rep_" + GROUP[kernel], dtype, 200, d, 3, 2, 950 + 2 * i + j, ({}, PLAIN), kernel=kernel, rep=True)


# ----------------------------------------------------------------------------------------------------------------------
# predictions at the training inputs: the nugget term of x0 row i on column i + same - 1
# ----------------------------------------------------------------------------------------------------------------------
PRED_LO = (0, 1, 63, 64, 127, 128)
PRED_M = (1, 64, 65)


def _train_slices(n):
    """(lo, m): lo at 0, 1, 63, 64, 127, 128 and the last row, m = 1, 64, 65 where they fit, and the whole set"""
    out = [(lo, m) for lo in PRED_LO + (n - 1,) for m in PRED_M if lo + m <= n]
    return sorted(set(out)) + [(0, n)]


def _fitted(seed, n, d, q, dtype, kernel, rep):
    x, Y, sr, th = _problem(seed, n, d, 3, q, rep=rep)
    eng = HotPathEngine(x, Y, sr=sr, q_local=q, dtype=dtype, kernel=kernel)
    out = eng.evaluate(th)
    assert np.all(out[:, 2] == 0), out[:, 2]
    Wz = [(_fetch(eng, 1, k, True), _fetch(eng, 1, k, False)) for k in range(q)]
    return eng, x, sr, th, Wz


def _run_predict(eng, x0, fill, same):
    return {"pred": _predict(eng, x0, fill, same)}


def _run_predict_block(eng, x0, fill, chunk):
    """engine.predict_block(x0, same=True) with PREDICT_CHUNK = chunk and the engine's scratch filled with `fill`"""
    import lcgp_amd.engine as eng_mod
    old = eng_mod.PREDICT_CHUNK
    try:
        eng_mod.PREDICT_CHUNK = chunk
        nbytes = eng._nbytes("lcgp_predict_scratch_bytes", eng.dtype, eng.n, eng.q_local, min(chunk, x0.shape[0]))
        eng._grow_scratch(nbytes).fill_(fill)
        return {"pred": eng.predict_block(x0, same=True).clone()}
    finally:
        eng_mod.PREDICT_CHUNK = old


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_predict_at_training_inputs(dtype, kernel):
    """lcgp_predict with x0 = x[lo : lo + m] and same = 1 + lo (the nugget term scale nt sr_j on column lo + i of row i)
    at the 64-block and 128-pad edges, one row to the whole set, n = 257 and 1025, full and rep paths; then the engine's
    chunked predict_block(x, same=True) with PREDICT_CHUNK = 64 and 128, whose chunks after the first pass same = 1 + lo.
    Every call on the three fills (bitwise), every component through check_predict(same)."""
    for i, (n, rep) in enumerate(((257, False), (257, True), (1025, False), (1025, True))):
        group = "same_" + GROUP[kernel]
        eng, x, sr, th, Wz = _fitted(1000 + i, n, 3, 2, dtype, kernel, rep)
        for lo, m in _train_slices(n):
            x0 = x[lo:lo + m]
            r = _poisoned(_run_predict, eng, x0, 1 + lo)["pred"]
            for k, (W, z) in enumerate(Wz):
                c = sb.check_predict(r[0, k], r[1, k], x0, x, sr, th[k], W, z, kernel, dtype, same=1 + lo)
                _record(group, dtype, "predict", c, "n%d rep%d lo%d m%d k%d" % (n, rep, lo, m, k))
        for chunk in (64, 128):
            r = _poisoned(_run_predict_block, eng, x, chunk)["pred"]
            for k, (W, z) in enumerate(Wz):
                c = sb.check_predict(r[0, k], r[1, k], x, x, sr, th[k], W, z, kernel, dtype, same=1)
                _record(group, dtype, "predict_block", c, "n%d rep%d chunk%d k%d" % (n, rep, chunk, k))
