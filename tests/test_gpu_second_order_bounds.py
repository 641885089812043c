"""Stage-wise componentwise bounds of the two second-order input queries on the GPU (tests/stage_bounds.py), every run on three
fills.

lcgp_predict_hess and lcgp_predict_gradcov are called directly on the workspace of an evaluated engine, their scratch and every
output buffer filled with 0x00, 0xFF (NaN in both precisions) and 0x5A bytes in turn.  Everything read back must be bitwise
identical over the fills, the tail out_stride - n0 of every output row must still hold the fill, and every check of the 0xFF run
must pass (ratio <= 1 against the derived bound, entry by entry):
  - hess: V and U from the first 2 q slabs of the scratch (n0pad x npad), DX from the next q slabs (rows_pad x npad, rows_pad =
    n0 d rounded up to 128, to 64 below 128), P from the last q -> pdx, p (check_cov_u on n0 d rows), phess; the four first-order
    outputs are bitwise those of lcgp_predict_grad;
  - gradcov: DX then P.  Three calls per fill: without weights (DX is read only here: a weighted call parks its partial sums over
    the DX slabs), with weights and gamma, with weights and gamma = NULL.  P and gamma of the weighted call are bitwise those of
    the unweighted one, M is bitwise the same with and without gamma, dghat is bitwise lcgp_predict_grad's -> pdx, p, gradcov
    (gamma entry by entry, dghat through the mean half of check_pgrad), gradcov_sum (M from a non-zero random start).
Exact statements, not bounds: the columns n .. npad and the rows n0 d .. rows_pad of every DX slab are bitwise zero, and DX is
exactly zero where a row of x0 is a training input (s = 0).

Coverage.  Dimensions d = 1 .. 126: one to 32 PH_B = 4 blocks and up to 528 block pairs (tri_decode), diagonal and off-diagonal,
blocks reaching past d (3, 5, 9, 17, 33, 65, 126), phess_kernel's WIDE variant from d = 17, pdx_kernel's DMAX = 32 restage from
d = 33.  Rows n0 = 1 .. 65: four inputs per Gram workgroup, PH_PTS = 16, PG_ROWS = 32, n0 d on both sides of 128 (64- and 128-
tiles of the product).  Columns n = 127 .. 131, 257: every n % VN (VN = 2 / 4), npad = 128, 256, 384.  The partial sums at their
tightest fit over the DX slabs (float32, npad = 128, d = 126, n0 = 1).  Dead waves in the last workgroup of the weighted sum.

Run with -s to see the worst ratio per case group, dtype and stage."""
from collections import defaultdict

import numpy as np
import pytest
import torch

from lcgp_amd import _hip
from tests import stage_bounds as sb
from tests.test_gpu_postfit_bounds import _bytes, _dev, _engine, _run_pgrad, _three, _x0
from tests.test_gpu_stage_bounds import FILLS, _bits, _fetch, _filled, _problem  # noqa: F401  (the shared helpers)

pytestmark = pytest.mark.gpu

WORST = defaultdict(lambda: sb.Check(0.0, ()))       # (group, dtype, stage) -> worst Check over the group's cases


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst ratio |error| / bound per case group, dtype and stage of the second-order queries (<= 1 passes)")
    for key in sorted(WORST):
        c = WORST[key]
        print("  %-14s %-8s %-12s %.3e  at %s" % (key + (c.ratio, c.where)))


def _record(group, dtype, stage, c, where_extra=None):
    key = (group, dtype, stage)
    if c.ratio >= WORST[key].ratio:
        WORST[key] = sb.Check(c.ratio, (where_extra,) + tuple(c.where) if where_extra is not None else c.where)
    assert c.ratio <= 1.0, (group, dtype, stage, c, where_extra)


def _group(name, kernel):
    return name + "_m52" if kernel == "matern52" else name


def _keeps_fill(t, n0, fill):
    """the rows n0 .. out_stride of an output (q x out_stride x ...) still hold the fill"""
    return bool(torch.all(t[:, n0:].contiguous().view(torch.uint8) == fill))


def _dx_slabs(sc, off, q, rows_pad, npad, rows, n):
    """q slabs rows_pad x npad from element `off` of the scratch: asserts the exact-zero padding (columns n .. npad, rows
    `rows` .. rows_pad, bitwise) and returns the rows x n part"""
    s = sc[off:off + q * rows_pad * npad].view(q, rows_pad, npad)
    assert not bool(_bits(s[:, :, n:].contiguous()).any()), "DX: columns n .. npad are not bitwise zero"
    assert not bool(_bits(s[:, rows:, :].contiguous()).any()), "DX: rows n0 d .. rows_pad are not bitwise zero"
    return s[:, :rows, :n].clone()


# ---- lcgp_predict_hess ---------------------------------------------------------------------------------------------------
def _run_hess(fill, eng, x0, ldo):
    q, n0, d, n = eng.q_local, x0.shape[0], eng.d, eng.n
    n0pad, npad, rows, rows_pad = sb.predict_pad(n0), sb._pad128(n), n0 * d, sb.predict_pad(n0 * d)
    tri = d * (d + 1) // 2
    lib, dev = eng.lib, eng.device
    with torch.cuda.device(dev):
        nbytes = _bytes(lib.lcgp_predict_hess_scratch_bytes, eng.dtype, n, d, q, n0)
        scratch = _filled((nbytes,), torch.uint8, fill, dev)
        sc = scratch.view(eng.tdtype)
        assert sc.numel() == 2 * q * (n0pad + rows_pad) * npad, (sc.numel(), q, n0pad, rows_pad, npad)
        g = _filled((2, q, ldo), torch.float64, fill, dev)
        dg = _filled((2, q, ldo, d), torch.float64, fill, dev)
        hs = _filled((2, q, ldo, tri), torch.float64, fill, dev)
        x0d = _dev(eng, x0)
        _hip.check(lib.lcgp_predict_hess(eng._stream(), eng.dtype, eng.kernel_id, n, d, eng.p, q, eng._p(eng.x), eng._p(eng.sr),
                                         eng._p(eng.theta_dev), eng._p(eng.workspace), n0, eng._p(x0d), eng._p(scratch),
                                         eng._p(g[0]), eng._p(g[1]), eng._p(dg[0]), eng._p(dg[1]), eng._p(hs[0]), eng._p(hs[1]),
                                         ldo), "lcgp_predict_hess")
        for t in (g[0], g[1], dg[0], dg[1], hs[0], hs[1]):
            assert _keeps_fill(t, n0, fill)
        slab, dslab = n0pad * npad, rows_pad * npad
        return dict(V=sc[:q * slab].view(q, n0pad, npad)[:, :n0, :n].clone(),
                    U=sc[q * slab:2 * q * slab].view(q, n0pad, npad)[:, :n0, :n].clone(),
                    DX=_dx_slabs(sc, 2 * q * slab, q, rows_pad, npad, rows, n),
                    P=sc[2 * q * slab + q * dslab:].view(q, rows_pad, npad)[:, :rows, :n].clone(),
                    g=g[:, :, :n0].clone(), dg=dg[:, :, :n0].clone(), hs=hs[:, :, :n0].clone())


def _zero_at_training_inputs(DX, d, ntrain):
    for i in range(ntrain):
        assert not bool(_bits(DX[:, i * d:(i + 1) * d, i].contiguous()).any()), ("DX at training input", i)


def _hess_case(group, eng, x, sr, th, kernel, dtype, x0, ntrain=0, ldo=None):
    n0, d = x0.shape
    ldo = ldo or n0
    r = _three(_run_hess, eng, x0, ldo)
    first = _run_pgrad(0xFF, eng, x0, ldo)
    assert torch.equal(_bits(r["g"]), _bits(first["g"])) and torch.equal(_bits(r["dg"]), _bits(first["dg"])), \
        "the first-order outputs of lcgp_predict_hess are not bitwise those of lcgp_predict_grad"
    assert torch.equal(_bits(r["V"]), _bits(first["V"]))
    del first
    _zero_at_training_inputs(r["DX"], d, ntrain)
    for k in range(eng.q_local):
        tag = "n=%d d=%d n0=%d k%d" % (eng.n, d, n0, k)
        W, z = _fetch(eng, 1, k, True), _fetch(eng, 1, k, False)
        _record(group, dtype, "hess_pdx", sb.check_pdx(r["DX"][k], x0, x, sr, th[k], kernel, dtype), tag)
        _record(group, dtype, "hess_p", sb.check_cov_u(r["P"][k], r["DX"][k], W, dtype), tag)
        _record(group, dtype, "phess", sb.check_phess(r["hs"][0, k], r["hs"][1, k], x0, x, sr, th[k], z, r["V"][k], r["P"][k],
                                                      kernel, dtype), tag)
        del W


# ---- lcgp_predict_gradcov ------------------------------------------------------------------------------------------------
def _run_gradcov(fill, eng, x0, ldo, w, M0):
    """w = None: one call (gamma).  Else three: (gamma, no w), (gamma, w, M), (NULL, w, M), M starting from M0 in both"""
    q, n0, d, n = eng.q_local, x0.shape[0], eng.d, eng.n
    npad, rows, rows_pad = sb._pad128(n), n0 * d, sb.predict_pad(n0 * d)
    tri = d * (d + 1) // 2
    lib, dev = eng.lib, eng.device
    r = {}
    with torch.cuda.device(dev):
        nbytes = _bytes(lib.lcgp_predict_gradcov_scratch_bytes, eng.dtype, n, d, q, n0)
        assert nbytes == 2 * q * rows_pad * npad * (4 if eng.tdtype == torch.float32 else 8), (nbytes, q, rows_pad, npad)
        x0d = _dev(eng, x0)
        wd = None if w is None else _dev(eng, w, torch.float64)
        dslab = rows_pad * npad

        def call(with_gamma, with_w):
            scratch = _filled((nbytes,), torch.uint8, fill, dev)
            dgh = _filled((q, ldo, d), torch.float64, fill, dev)
            gam = _filled((q, ldo, tri), torch.float64, fill, dev) if with_gamma else None
            M = _dev(eng, M0, torch.float64).clone() if with_w else None
            _hip.check(lib.lcgp_predict_gradcov(eng._stream(), eng.dtype, eng.kernel_id, n, d, eng.p, q, eng._p(eng.x),
                                                eng._p(eng.sr), eng._p(eng.theta_dev), eng._p(eng.workspace), n0, eng._p(x0d),
                                                eng._p(scratch), eng._p(dgh), eng._p(gam), eng._p(wd if with_w else None),
                                                eng._p(M), ldo), "lcgp_predict_gradcov")
            assert _keeps_fill(dgh, n0, fill) and (gam is None or _keeps_fill(gam, n0, fill))
            sc = scratch.view(eng.tdtype)
            Pm = sc[q * dslab:].view(q, rows_pad, npad)[:, :rows, :n].clone()
            DX = None if with_w else _dx_slabs(sc, 0, q, rows_pad, npad, rows, n)
            return dgh[:, :n0].clone(), None if gam is None else gam[:, :n0].clone(), Pm, DX, M

        r["dghat"], r["gamma"], r["P"], r["DX"], _ = call(True, False)
        if w is not None:
            dg2, gam2, P2, _, r["M"] = call(True, True)
            assert torch.equal(_bits(P2), _bits(r["P"])), "P is changed by the weighted call (partial sums over the DX slabs)"
            assert torch.equal(_bits(gam2), _bits(r["gamma"])) and torch.equal(_bits(dg2), _bits(r["dghat"]))
            dg3, _, P3, _, M3 = call(False, True)
            assert torch.equal(_bits(P3), _bits(r["P"])), "P is changed by the weighted call without gamma"
            assert torch.equal(_bits(M3), _bits(r["M"])), "M depends on whether gamma is written"
            assert torch.equal(_bits(dg3), _bits(r["dghat"]))
    return r


def _w(n0, seed):
    """weights with zeros and one negative entry"""
    w = np.random.default_rng(seed).uniform(0.1, 1.0, n0)
    w[::3] = 0.0
    w[min(1, n0 - 1)] = -0.4
    return w


def _gradcov_case(group, eng, x, sr, th, kernel, dtype, x0, ntrain=0, ldo=None, weighted=True, seed=0):
    n0, d = x0.shape
    ldo = ldo or n0
    w = _w(n0, 4000 + seed) if weighted else None
    M0 = np.random.default_rng(4100 + seed).standard_normal((eng.q_local, d * (d + 1) // 2))
    r = _three(_run_gradcov, eng, x0, ldo, w, M0)
    first = _run_pgrad(0xFF, eng, x0, ldo)
    assert torch.equal(_bits(r["dghat"]), _bits(first["dg"][0])), "dghat is not bitwise that of lcgp_predict_grad"
    del first
    _zero_at_training_inputs(r["DX"], d, ntrain)
    for k in range(eng.q_local):
        tag = "n=%d d=%d n0=%d k%d" % (eng.n, d, n0, k)
        W, z = _fetch(eng, 1, k, True), _fetch(eng, 1, k, False)
        _record(group, dtype, "gc_pdx", sb.check_pdx(r["DX"][k], x0, x, sr, th[k], kernel, dtype), tag)
        _record(group, dtype, "gc_p", sb.check_cov_u(r["P"][k], r["DX"][k], W, dtype), tag)
        _record(group, dtype, "gradcov", sb.check_gradcov(r["gamma"][k], r["dghat"][k], x0, x, sr, th[k], z, r["P"][k], kernel,
                                                          dtype), tag)
        if weighted:
            _record(group, dtype, "gradcov_sum", sb.check_gradcov_sum(r["M"][k], M0[k], r["gamma"][k], w), tag)
        del W


# ----------------------------------------------------------------------------------------------------------------------
SO_DIMS = (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 65, 126)


@pytest.mark.parametrize("rep", [False, True], ids=["full", "rep"])
@pytest.mark.parametrize("kernel", ["matern32", "se", "matern52"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("d", SO_DIMS)
def test_dimensions(d, dtype, kernel, rep):
    """d on both sides of every PH_B = 4 block edge it can reach, of WIDE (16 / 17) and of the DMAX restage (32 / 33), up to
    the 528 block pairs of d = 126; n = 301 (odd, 1 mod 4); n0 = 37, 9 from d = 65 on; three training inputs among x0"""
    n0 = 9 if d >= 65 else 37
    eng, x, sr, th = _engine(5000 + d, 301, d, 2, dtype, kernel=kernel, rep=rep)
    x0 = _x0(5200 + d, n0, d, x, 3)
    _hess_case(_group("dims", kernel), eng, x, sr, th, kernel, dtype, x0, 3)
    _gradcov_case(_group("dims", kernel), eng, x, sr, th, kernel, dtype, x0, 3, seed=d)


SO_ROWS = (1, 3, 4, 5, 15, 16, 17, 21, 22, 31, 32, 33, 65)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_rows(dtype):
    """d = 6, out_stride = n0 + 3: n0 around the four waves of a Gram workgroup, PH_PTS = 16, PG_ROWS = 32 and n0 d = 128 (21 /
    22: the product's 64- against 128-tiles); the first three rows are training inputs when n0 > 3"""
    d = 6
    eng, x, sr, th = _engine(5400, 300, d, 2, dtype)
    for n0 in SO_ROWS:
        nt = 3 if n0 > 3 else 0
        x0 = _x0(5401 + n0, n0, d, x, nt)
        _hess_case("rows", eng, x, sr, th, "matern32", dtype, x0, nt, ldo=n0 + 3)
        _gradcov_case("rows", eng, x, sr, th, "matern32", dtype, x0, nt, ldo=n0 + 3, seed=n0)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_columns(dtype):
    """d = 5, n0 = 20: every n % VN (VN = 2 in float64, 4 in float32) and npad = 128, 256, 384"""
    d = 5
    for n in (127, 128, 129, 130, 131, 257):
        eng, x, sr, th = _engine(5600 + n, n, d, 2, dtype)
        x0 = _x0(5700 + n, 20, d, x, 3)
        _hess_case("columns", eng, x, sr, th, "matern32", dtype, x0, 3)
        _gradcov_case("columns", eng, x, sr, th, "matern32", dtype, x0, 3, seed=n)


@pytest.mark.parametrize("d,n0", [(126, 1), (126, 2), (126, 5), (125, 1), (63, 1)])
def test_partial_sums_tightest_fit(d, n0):
    """float32, n = 100 (npad = 128), q = 2: the per-workgroup partial sums (q ceil(n0 / 4) d (d + 1) / 2 doubles) parked over
    the DX slabs (q rows_pad npad floats) -- 64008 of 65536 bytes per component at d = 126, n0 = 1.  P is bitwise that of the
    unweighted call (asserted in _run_gradcov), with gamma written and NULL; M of both components within its bound"""
    eng, x, sr, th = _engine(5800 + d, 100, d, 2, "float32")
    rows_pad = sb.predict_pad(n0 * d)
    assert 2 * -(-n0 // 4) * (d * (d + 1) // 2) * 8 <= 2 * rows_pad * 128 * 4
    _gradcov_case("partial_sums", eng, x, sr, th, "matern32", "float32", _x0(5900 + d + n0, n0, d), seed=d + n0)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_weights_with_dead_waves(dtype):
    """n0 = 6, 7: two and one dead waves in the last workgroup; w with zeros and one negative entry, M from a random start"""
    eng, x, sr, th = _engine(6000, 200, 6, 2, dtype, rep=True)
    for n0 in (6, 7):
        _gradcov_case("weights", eng, x, sr, th, "matern32", dtype, _x0(6001 + n0, n0, 6, x, 2), 2, seed=n0)
