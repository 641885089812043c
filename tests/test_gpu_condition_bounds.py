"""Stage-wise componentwise bounds of the conditioned view on the GPU (tests/stage_bounds.py), every run on three fills.

The two C entries are called directly with buffers of this test's own (tests/test_gpu_condition.py::_raw shows the calls; the
layouts are those of cond_carve, do_condition_prepare and do_condition_predict in lcgp_hip.hip):
  - lcgp_condition_prepare -> the info words; the state, whole (U_n: q slabs mpad x npad, the dense L_S^-1: q slabs mpad x
    mpad, v: q x mpad doubles); X_n and ghat(xn) / gvar(xn) from its scratch (q slabs mpad x npad, then at a 256-aligned offset
    2 q mpad doubles); L_S and L_S^-1 fetched from the cond workspace (n = m) and the padding rows of its matrix slot;
  - lcgp_condition_predict -> X_0, U_0 (q slabs n0pad x npad each) and, at a 256-aligned offset, Sigma_0n and T (q slabs n0pad x
    mpad each) from its scratch, whole; ghat / gvar;
  - lcgp_predict(same = 0) on the same rows, separately: the ghat / gvar the view's correction starts from.
Before each run the cond workspace, the state, both scratch buffers, the outputs and the info words are filled with 0x00, 0xFF
(NaN in both precisions) and 0x5A bytes in turn: everything read back must be bitwise identical over the fills, every info word
0, and every check of the 0xFF run must pass:
    cross_n (X_n), u_n (U_n), pred_n (ghat / gvar at xn), cond_s (L_S L_S^T against S_ref), cond_winv (L_S^-1), cond_v (v),
    cross_0 (X_0), u_0 (U_0), cond_cross (Sigma_0n), cond_t (T), cond_out (the corrected ghat / gvar against lcgp_predict's).
Exact (bitwise) next to them: the state's dense L_S^-1 equals the fetched W slot on the lower triangle, is zero above the diagonal
over the whole mpad x mpad and the identity from row m on; v is zero on m .. mpad - 1; Sigma_0n is zero on the rows from n0 and
the columns from m on; the padding rows of the cond workspace's matrix slot hold the identity after the factorisation; the words
the preparation does not write (ghat / gvar of xn beyond m, the output columns between n0 and out_stride) keep their fill.
(The zeros off the copied triangle are compared by value: the triangular inverse leaves -0 = -(1 x 0 x w) below the diagonal of
the identity rows of the padding, which the dense copy carries over and which adds nothing to T.)

Shapes (the smallest that reach every path): n = 333 (npad 384), q_local = 3 and once 1; m in {1, 70, 128, 129, 300} with n0 = 130
(a single pivot; a short tile; mpad without padding; 127 padding columns; mpad = 384) and n0 in {1, 64, 127, 128} with m = 70 (the
last sizes on 64-row tiles, the first on 128-row tiles; n0 = 130 pads to 256); d = 1 and 6 throughout, the three kernels, both
precisions, the full path and the replicated one (sr != 1, counts 1 .. 3 at the new inputs).

Run with -s to see the worst ratio per case group, dtype and stage."""
import ctypes as C
from collections import defaultdict

import numpy as np
import pytest
import torch

from lcgp_amd import _hip
from lcgp_amd.engine import HotPathEngine
from tests import stage_bounds as sb
from tests.test_gpu_stage_bounds import FILLS, _bits, _config_problem, _fetch, _filled, _predict, _problem

pytestmark = pytest.mark.gpu

KERNELS = ("matern32", "se", "matern52")
GROUP = {"matern32": "m32", "se": "se", "matern52": "m52"}
N = 333
SHAPES = [(m, 130) for m in (1, 70, 128, 129, 300)] + [(70, n0) for n0 in (1, 64, 127, 128)]          # (m, n0)

WORST = defaultdict(lambda: sb.Check(0.0, ()))       # (group, dtype, stage) -> worst Check over the group's cases


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst ratio |error| / bound per case group, dtype and stage of the conditioned view (<= 1 passes)")
    for key in sorted(WORST):
        c = WORST[key]
        print("  %-12s %-8s %-11s %.3e  at %s" % (key + (c.ratio, c.where)))


def _record(group, dtype, stage, c, where_extra=None):
    key = (group, dtype, stage)
    if c.ratio >= WORST[key].ratio:
        WORST[key] = sb.Check(c.ratio, (where_extra,) + tuple(c.where) if where_extra is not None else c.where)
    assert c.ratio <= 1.0, (group, dtype, stage, c, where_extra)


def _bytes(fn, *args):
    nbytes = C.c_size_t(0)
    _hip.check(fn(*args, C.byref(nbytes)), "bytes")
    return int(nbytes.value)


def _align256(nbytes):
    return -(-int(nbytes) // 256) * 256


def _dev(eng, a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a, np.float64)).to(eng.device, eng.tdtype if dtype is None else dtype).contiguous()


def _keeps(t, fill):
    return bool(torch.all(t.contiguous().view(torch.uint8) == fill))


def _fetch_cond(eng, cws, m, which):
    out = torch.empty((eng.q_local, m, m), dtype=eng.tdtype, device=eng.device)
    for k in range(eng.q_local):
        _hip.check(eng.lib.lcgp_fetch_matrix(eng._stream(), eng.dtype, m, eng.d, eng.p, eng.q_local, eng._p(cws), int(which), k,
                                             eng._p(out[k])), "lcgp_fetch_matrix")
    return out


def _run_cond(fill, eng, xn, t, r, x0, ldo):
    """lcgp_condition_prepare, lcgp_condition_predict and a separate lcgp_predict on freshly filled memory; everything the checks
    read, cloned"""
    q, d, n, m, n0 = eng.q_local, eng.d, eng.n, xn.shape[0], x0.shape[0]
    npad, mpad, n0pad = sb._pad128(n), sb._pad128(m), sb.predict_pad(n0)
    lib, dev, p = eng.lib, eng.device, eng._p
    esz = torch.empty((), dtype=eng.tdtype).element_size()
    res = {}
    with torch.cuda.device(dev):
        st = eng._stream()
        cws = _filled((_bytes(lib.lcgp_workspace_bytes, eng.dtype, m, d, eng.p, q),), torch.uint8, fill, dev)
        state = _filled((_bytes(lib.lcgp_condition_state_bytes, eng.dtype, n, d, q, m),), torch.uint8, fill, dev)
        nprep = _bytes(lib.lcgp_condition_scratch_bytes, eng.dtype, n, q, m, 0)
        prep = _filled((nprep,), torch.uint8, fill, dev)
        info = _filled((q,), torch.int32, fill, dev)
        xnd, x0d = _dev(eng, xn), _dev(eng, x0)
        td = _dev(eng, t, torch.float64)
        rd = None if r is None else _dev(eng, r, torch.float64)
        _hip.check(lib.lcgp_condition_prepare(st, eng.dtype, eng.kernel_id, n, d, eng.p, q, p(eng.x), p(eng.sr), p(eng.theta_dev),
                                              p(eng.workspace), m, p(xnd), p(td), p(rd), p(prep), nprep, p(cws), p(state), p(info)),
                   "lcgp_condition_prepare")
        res["info"] = info.clone()
        res["state"] = state.clone()
        slab = mpad * npad
        res["Xn"] = prep.view(eng.tdtype)[:q * slab].view(q, mpad, npad).clone()
        off = _align256(q * slab * esz)
        gn = prep[off:off + 2 * q * mpad * 8].view(torch.float64).view(2, q, mpad)
        assert _keeps(gn[:, :, m:], fill), "ghat / gvar of xn written beyond m"
        res["pred_n"] = gn[:, :, :m].clone()
        res["LS"], res["WS"] = _fetch_cond(eng, cws, m, 0), _fetch_cond(eng, cws, m, 1)
        slot = cws.view(eng.tdtype)[:q * mpad * mpad].view(q, mpad, mpad)          # the matrix slot: offset 0 of the workspace
        res["L_pad"] = torch.tril(slot)[:, m:, :].clone()
        del prep, gn
        npred = _bytes(lib.lcgp_condition_scratch_bytes, eng.dtype, n, q, m, n0)
        scratch = _filled((npred,), torch.uint8, fill, dev)
        out = _filled((2, q, ldo), torch.float64, fill, dev)
        _hip.check(lib.lcgp_condition_predict(st, eng.dtype, eng.kernel_id, n, d, eng.p, q, p(eng.x), p(eng.sr), p(eng.theta_dev),
                                              p(eng.workspace), p(state), m, p(xnd), n0, p(x0d), p(scratch), npred, p(out[0]),
                                              p(out[1]), ldo), "lcgp_condition_predict")
        assert _keeps(out[:, :, n0:], fill), "output columns between n0 and out_stride written"
        assert torch.equal(_bits(state), _bits(res["state"])), "lcgp_condition_predict wrote to the state"
        res["out"] = out[:, :, :n0].clone()
        s0, cs = n0pad * npad, n0pad * mpad
        sc = scratch.view(eng.tdtype)
        res["X0"] = sc[:q * s0].view(q, n0pad, npad).clone()
        res["U0"] = sc[q * s0:2 * q * s0].view(q, n0pad, npad).clone()
        off = _align256(2 * q * s0 * esz) // esz
        res["Sg"] = sc[off:off + q * cs].view(q, n0pad, mpad).clone()
        res["T"] = sc[off + q * cs:off + 2 * q * cs].view(q, n0pad, mpad).clone()
        del scratch, sc
        res["pred0"] = _predict(eng, x0, fill)
    return res


def _three(eng, xn, t, r, x0, ldo):
    base = _run_cond(0xFF, eng, xn, t, r, x0, ldo)
    for f in FILLS:
        if f == 0xFF:
            continue
        other = _run_cond(f, eng, xn, t, r, x0, ldo)
        assert other.keys() == base.keys()
        for key in base:
            assert torch.equal(_bits(other[key]), _bits(base[key])), ("fill 0x%02X changes" % f, key)
        del other
    return base


def _state_views(eng, state, m):
    """U_n (q, mpad, npad), the dense L_S^-1 (q, mpad, mpad), v (q, mpad doubles): cond_carve's layout"""
    q, npad, mpad = eng.q_local, sb._pad128(eng.n), sb._pad128(m)
    esz = torch.empty((), dtype=eng.tdtype).element_size()
    off_w = _align256(q * mpad * npad * esz)
    off_v = off_w + _align256(q * mpad * mpad * esz)
    un = state[:q * mpad * npad * esz].view(eng.tdtype).view(q, mpad, npad)
    wd = state[off_w:off_w + q * mpad * mpad * esz].view(eng.tdtype).view(q, mpad, mpad)
    v = state[off_v:off_v + q * mpad * 8].view(torch.float64).view(q, mpad)
    return un, wd, v


def _cond_case(group, eng, x, sr, th, kernel, dtype, xn, t, r, x0, comps=None, ldo=None, margin=False):
    """the three-fill run and every check for the components `comps` (default: all).  margin: also print and assert the
    definiteness margin of S (test_ill_conditioned_s)"""
    q, n, m, n0 = eng.q_local, eng.n, xn.shape[0], x0.shape[0]
    res = _three(eng, xn, t, r, x0, ldo or n0)
    assert torch.all(res["info"] == 0), (group, dtype, m, n0, res["info"])
    mpad = sb._pad128(m)
    ident = torch.eye(mpad, dtype=eng.tdtype, device=eng.device)[m:, :]
    assert torch.equal(res["L_pad"], ident.expand_as(res["L_pad"])), (group, dtype, m, "padding of the matrix slot")
    un, wd, v = _state_views(eng, res["state"], m)
    assert torch.all(v[:, m:] == 0), (group, dtype, m, "v on the padding")
    sg = res["Sg"]
    assert torch.all(sg[:, n0:, :] == 0) and torch.all(sg[:, :, m:] == 0), (group, dtype, m, n0, "padding of Sigma_0n")
    for k in (range(q) if comps is None else comps):
        tag = "d=%d m=%d n0=%d k%d" % (eng.d, m, n0, k)
        W, z = _fetch(eng, 1, k, True), _fetch(eng, 1, k, False)
        Xn, Un, LS, WS, Wd = res["Xn"][k, :m, :n], un[k, :m, :n], res["LS"][k], res["WS"][k], wd[k]
        X0, U0, Sg, Tm = res["X0"][k, :n0, :n], res["U0"][k, :n0, :n], sg[k, :n0, :m], res["T"][k, :n0, :m]
        gn, g0, g1 = res["pred_n"][:, k], res["pred0"][:, k], res["out"][:, k]

        def rec(stage, c):
            _record(group, dtype, stage, c, tag)
        rec("cross_n", sb.check_cov_cross(Xn, xn, x, sr, th[k], kernel, dtype))
        rec("u_n", sb.check_cov_u(Un, Xn, W, dtype))
        rec("pred_n", sb.check_predict(gn[0], gn[1], xn, x, sr, th[k], W, z, kernel, dtype))
        rec("cond_s", sb.check_cond_s(LS, Un, xn, r, th[k], kernel, dtype))
        rec("cond_winv", sb.check_inverse_factor(LS, WS, dtype))
        dense = sb.check_cond_dense_inverse(Wd, WS, m)
        if dense.ratio != 0:
            at = torch.nonzero(sb.cond_dense_mismatch(Wd, WS, m))[:8]
            print("dense L_S^-1 %s %s %s: first mismatches (row, column, value) %s"
                  % (group, dtype, tag, [(int(i), int(j), float(Wd[i, j])) for i, j in at]))
        assert dense.ratio == 0, (group, dtype, tag, "dense L_S^-1 of the state", dense)
        rec("cond_v", sb.check_cond_v(v[k], Wd, t[k], gn[0], m))
        rec("cross_0", sb.check_cov_cross(X0, x0, x, sr, th[k], kernel, dtype))
        rec("u_0", sb.check_cov_u(U0, X0, W, dtype))
        rec("cond_cross", sb.check_cond_cross(Sg, U0, Un, x0, xn, th[k], kernel, dtype))
        rec("cond_t", sb.check_cov_u(Tm, Sg, Wd[:m, :m], dtype))
        rec("cond_out", sb.check_cond_out(g1[0], g1[1], Tm, v[k], g0[0], g0[1], m))
        if margin:
            ref, bound, _ = sb.cond_s_ref_bound(LS, Un, xn, r, th[k], kernel, dtype)
            b = torch.tril(bound) + torch.tril(bound, -1).T
            lam, row = float(torch.linalg.eigvalsh(ref)[0]), float(b.sum(dim=1).max())
            print("condition bounds %s %s %s: smallest eigenvalue of S_ref %.3e, largest row sum of the cond_s bound %.3e, "
                  "margin %.1f (> 10), condition number %.2e" % (group, dtype, tag, lam, row, lam / row,
                                                                 float(torch.linalg.cond(ref))))
            assert lam > 10.0 * row, (group, dtype, tag, lam, row)
        del W
    return res


def _engine(seed, d, q, dtype, kernel="matern32", rep=False, n=N, **prob):
    x, Y, sr, th = _problem(seed, n, d, 3, q, rep=rep, **prob)
    eng = HotPathEngine(x, Y, sr=sr, q_local=q, dtype=dtype, kernel=kernel)
    out = eng.evaluate(th)
    assert np.all(out[:, 2] == 0), out[:, 2]
    return eng, x, sr, th


def _new(seed, m, n0, d, q, rep, lo=None, hi=None):
    """m new inputs in the box of the data and n0 prediction inputs around it, latent observations t (q, m), replicate counts
    1 .. 3 on the rep path (None on the full one)"""
    rng = np.random.default_rng(seed)
    lo = np.zeros(d) if lo is None else lo
    hi = np.ones(d) if hi is None else hi
    xn = lo + (hi - lo) * rng.uniform(0.0, 1.0, (m, d))
    x0 = lo + (hi - lo) * rng.uniform(-0.1, 1.1, (n0, d))
    t = rng.standard_normal((q, m))
    r = (1.0 + rng.permutation(m) % 3) if rep else None
    return xn, t, r, x0


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rep", [False, True], ids=["full", "rep"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_tile_edges_of_m_and_n0(dtype, kernel, rep):
    """every (m, n0) of SHAPES at d = 1 and d = 6, q_local = 3 with its own theta each"""
    for d in (1, 6):
        eng, x, sr, th = _engine(1100 + d, d, 3, dtype, kernel, rep)
        for i, (m, n0) in enumerate(SHAPES):
            xn, t, r, x0 = _new(1110 + 10 * d + i, m, n0, d, 3, rep)
            _cond_case(("rep_" if rep else "full_") + GROUP[kernel], eng, x, sr, th, kernel, dtype, xn, t, r, x0)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_one_component_and_out_stride(dtype):
    """q_local = 1; then q_local = 3 with out_stride = 200 > n0 = 130 into a poisoned output block: the columns between n0 and the
    stride keep their fill (_run_cond asserts it)"""
    eng, x, sr, th = _engine(1200, 6, 1, dtype, rep=True)
    xn, t, r, x0 = _new(1201, 70, 130, 6, 1, True)
    _cond_case("q1", eng, x, sr, th, "matern32", dtype, xn, t, r, x0)
    eng, x, sr, th = _engine(1202, 6, 3, dtype, "se")
    xn, t, r, x0 = _new(1203, 129, 130, 6, 3, False)
    _cond_case("stride", eng, x, sr, th, "se", dtype, xn, t, r, x0, ldo=200)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_wider_dimension_buckets(dtype):
    """Matern-5/2 at one dimension of each wider for_dim bucket (DD = 10: d = 9; 16: 15; 32: 31) and in the wide variant (d = 33:
    two 32-dimension chunks of cross_kernel, the second with one dimension)"""
    for i, d in enumerate((9, 15, 31, 33)):
        eng, x, sr, th = _engine(1300 + i, d, 3, dtype, "matern52", rep=bool(i % 2))
        xn, t, r, x0 = _new(1310 + i, 70, 130, d, 3, bool(i % 2))
        _cond_case("dims_m52", eng, x, sr, th, "matern52", dtype, xn, t, r, x0)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_lengthscales_at_the_c0_cutoff(dtype, kernel):
    """every lengthscale at 1e-6: C0 between distinct inputs is past its cut-off (zero), U_n and U_0 vanish, S is (scale + tau) I
    to rounding for ANY distinct xn, so it stays definite; rows 0 .. 2 of x0 equal rows of xn, where C0 = 1 and Sigma_0n holds
    scale (1 - nt) exactly"""
    d = 6
    x, Y, sr, th = _problem(1400, N, d, 3, 3, D=(1.0, 2.0))
    th[:, :d] = 1e-6
    eng = HotPathEngine(x, Y, sr=sr, q_local=3, dtype=dtype, kernel=kernel)
    assert np.all(eng.evaluate(th)[:, 2] == 0)
    xn, t, r, x0 = _new(1401, 70, 130, d, 3, False)
    x0[:3] = xn[[0, 64, 69]]
    res = _cond_case("cutoff_" + GROUP[kernel], eng, x, sr, th, kernel, dtype, xn, t, r, x0)
    assert torch.all(torch.isfinite(res["out"]))


@pytest.mark.parametrize("rep", [False, True], ids=["full", "rep"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_rows_of_x0_equal_to_rows_of_xn(dtype, kernel, rep):
    """x0 rows 0 .. 4 are xn rows 0, 1, 63, 64, 69 (m = 70, n0 = 130, d = 6): no nugget term enters Sigma_0n (check_cond_cross has
    none), and gvar there cancels from gvar_0 down to about tau, which cond_out's bound -- relative to gvar_0 + sum T^2 -- must
    still hold; the cancellation is printed"""
    d = 6
    eng, x, sr, th = _engine(1500, d, 3, dtype, kernel, rep)
    xn, t, r, x0 = _new(1501, 70, 130, d, 3, rep)
    rows = [0, 1, 63, 64, 69]
    x0[:5] = xn[rows]
    res = _cond_case("equal_" + GROUP[kernel], eng, x, sr, th, kernel, dtype, xn, t, r, x0)
    g0, g1 = res["pred0"][1, :, :5].cpu().numpy(), res["out"][1, :, :5].cpu().numpy()
    tau = np.stack([sb.cond_tau(th[k], r, 70, d)[rows] for k in range(3)])
    print("condition bounds equal rows %s %s %s: gvar before / after %.3e, after / tau in [%.3f, %.3f]"
          % (dtype, kernel, "rep" if rep else "full", np.max(g0 / g1), np.min(g1 / tau), np.max(g1 / tau)))
    assert np.all(g1 > 0) and np.all(g1 < g0)


# The ill-conditioned case.  S = Sigma_nn + diag(tau) is ill-conditioned where the posterior covariance Sigma_nn of the new inputs
# is large and smooth against tau = 1 / D: new inputs OUTSIDE the data (the unit box shifted by ILL_OFFSET, three lengthscales
# away), in pairs ILL_SPACING apart, the smallest nugget, large D.  (Inside the data a large D leaves Sigma_nn near zero and S near
# tau I, whatever the spacing.)  D per storage type was chosen on the CPU -- numpy float64, the emulated fit of the same problem --
# so that the smallest eigenvalue of the float64 S_ref exceeds ten times the largest row sum of the cond_s bound of that
# precision: S then stays definite under any error the bound admits, and info is 0.  There: float64, D = 1e7: margins 358 and
# 166, condition numbers 2.5e8 and 3.7e8; float32, whose bound has row sums of ~1e-2 scale at m = 70, takes the milder D = 2:
# margins 58 and 24, condition numbers 85 and 190 (D = 5 leaves 8.7), as test_gpu_stage_bounds.test_ill_conditioned does with kappa.
ILL_D = {"float64": 1e7, "float32": 2.0}
ILL_SPACING = 1e-4
ILL_OFFSET = 3.0


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_ill_conditioned_s(dtype):
    """the margin is measured on the library's own U_n, printed and asserted per component; info = 0 in both precisions; every
    stage holds its bound, none of which carries the condition number of S.  Every other row of x0 lies among the new inputs"""
    d, m = 2, 70
    Dv = ILL_D[dtype]
    eng, x, sr, th = _engine(1600, d, 2, dtype, D=(Dv, Dv), ell=(-0.5, 0.0), nug=(-7.0, -7.0))
    xn, t, r, x0 = _new(1601, m, 130, d, 2, False)
    xn += ILL_OFFSET
    xn[1::2] = xn[0::2] + ILL_SPACING
    x0[::2] += ILL_OFFSET
    _cond_case("ill_cond", eng, x, sr, th, "matern32", dtype, xn, t, r, x0, margin=True)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_headline_configuration(dtype):
    """configs[2] of the benchmark (n = 4096, d = 6, q = 8) with its own data, standardisation and parameters, m = 150, n0 = 130,
    components 0 and 7"""
    mdl, eng, x, Y, th = _config_problem(3, dtype)
    out = eng.evaluate(th)
    assert np.all(out[:, 2] == 0), out[:, 2]
    lo, hi = x.min(axis=0), x.max(axis=0)
    xn, t, r, x0 = _new(1700, 150, 130, x.shape[1], eng.q_local, False, lo, hi)
    _cond_case("headline", eng, x, None, th, "matern32", dtype, xn, t, r, x0, comps=[0, eng.q_local - 1])
    torch.cuda.empty_cache()
