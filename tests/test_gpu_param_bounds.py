"""Stage-wise componentwise bounds of the two parameter-space queries on the GPU (tests/stage_bounds.py), every run on three
fills.

lcgp_nll_hess and lcgp_predict_paramgrad are called directly on the workspace of an evaluated float64 engine, their scratch and
every output buffer filled with 0x00, 0xFF (NaN) and 0x5A bytes in turn.  Both leave every intermediate in their scratch, carved
here by sb.hess_layout / sb.pgrad_layout -- restatements of hess_carve / pgrad_carve whose byte totals must equal the library's
*_scratch_bytes, so a layout change fails loudly instead of shifting every slice.  Everything read back must be bitwise identical
over the fills, the rows of the outputs outside the group's components and the tail out_stride - n0 of every output row must
still hold the fill, and every check of the 0xFF run must pass (ratio <= 1 against the derived bound, entry by entry):
  - nll_hess: hess_prep, hess_mirror, hess_da (E holds d_{d-1}A), hess_y, hess_g, hess_trace, hess_contract, hess_vectors, hess_out;
  - predict_paramgrad: hess_prep, hess_da, pp_y, pp_t, pp_rowdot, pp_sums, pp_vy, pp_out; with same = 0, V, ghat and gvar are bitwise
    those of lcgp_predict_grad (whose stages tests/test_gpu_postfit_bounds.py checks).

Coverage.  nll_hess: d = 1 .. 17 -- one, two (4 / 5: a block reaching past d), three (9) and five (17) HS_B = 4 blocks, up to 15
block pairs, diagonal and off-diagonal; m = d + 2 on both sides of HS_JC = 8 (d = 6 / 7), three chunks of j at d = 17; n = 63 .. 257
-- a second band all padding (63), ragged bands, npad = 128, 256, 384; p = 1 .. 129 -- ppad = 256, two row tiles of Q; the three
kernels, full and rep (non-constant s: s_b against s_a); the groupings (k0, q_group) = (0, 3), (1, 2), (2, 1), bitwise.
predict_paramgrad: d on both sides of PP_DB = 16 and three blocks (33); n0 on both sides of predict_pad and of the 128-row slab
(n0p != n0r below 65); p = 129; same = 0 with training inputs among x0 (phi = 0), same = 1 on the whole training set, same = lo + 1
on a middle slice; out_stride > n0; the groupings.

Run with -s to see the worst ratio per case group and stage."""
from collections import defaultdict

import numpy as np
import pytest
import torch

from lcgp_amd import _hip
from lcgp_amd.engine import HotPathEngine
from tests import stage_bounds as sb
from tests.test_gpu_postfit_bounds import _bytes, _dev, _run_pgrad, _three, _x0
from tests.test_gpu_stage_bounds import _bits, _fetch, _filled, _problem

pytestmark = pytest.mark.gpu

WORST = defaultdict(lambda: sb.Check(0.0, ()))       # (group, stage) -> worst Check over the group's cases
KERNELS = ("matern32", "se", "matern52")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst ratio |error| / bound per case group and stage of the parameter-space queries (<= 1 passes)")
    for key in sorted(WORST):
        c = WORST[key]
        print("  %-16s %-14s %.3e  at %s" % (key + (c.ratio, c.where)))


def _record(group, stage, c, tag):
    key = (group, stage)
    if c.ratio >= WORST[key].ratio:
        WORST[key] = sb.Check(c.ratio, (tag,) + tuple(c.where))
    assert c.ratio <= 1.0, (group, stage, c, tag)


def _group(name, kernel):
    return name if kernel == "matern32" else name + "_" + {"se": "se", "matern52": "m52"}[kernel]


def _engine(seed, n, d, q=3, p=3, kernel="matern32", rep=False):
    """the float64 engine of tests/test_gpu_postfit_bounds.py with p outputs, evaluated; Y is returned for the checks"""
    x, Y, sr, th = _problem(seed, n, d, p, q, rep=rep)
    eng = HotPathEngine(x, Y, sr=sr, q_local=q, dtype="float64", kernel=kernel)
    out = eng.evaluate(th)
    assert np.all(out[:, 2] == 0), out[:, 2]
    return eng, x, Y, sr, th


def _part(sc, off, shape):
    return sc[off:off + int(np.prod(shape))].view(*shape).clone()


def _outside_keeps_fill(t, k0, qg, fill, dim=0):
    """the slices of `t` along `dim` of the components outside [k0, k0 + qg) still hold the fill"""
    keep = [k for k in range(t.shape[dim]) if not k0 <= k < k0 + qg]
    return not keep or bool(torch.all(t.index_select(dim, torch.as_tensor(keep, device=t.device)).contiguous().view(torch.uint8) == fill))


# ---- lcgp_nll_hess -------------------------------------------------------------------------------------------------------
def _run_hess(fill, eng, k0, qg):
    q, n, d, p = eng.q_local, eng.n, eng.d, eng.p
    lib, dev = eng.lib, eng.device
    L = sb.hess_layout(n, d, p, qg)
    m, npad, ppad, nb = L["m"], L["npad"], L["ppad"], L["nb"]
    with torch.cuda.device(dev):
        nbytes = _bytes(lib.lcgp_nll_hess_scratch_bytes, eng.dtype, n, d, p, qg)
        assert nbytes == L["total"], ("hess_layout against lcgp_nll_hess_scratch_bytes", nbytes, L["total"])
        scratch = _filled((nbytes,), torch.uint8, fill, dev)
        out = _filled((q, lib.lcgp_nll_hess_width(d, p)), torch.float64, fill, dev)
        _hip.check(lib.lcgp_nll_hess(*eng._head(Y=True), k0, qg, eng._p(scratch), eng._p(out)), "lcgp_nll_hess")
        assert _outside_keeps_fill(out, k0, qg, fill), "rows of out outside the group are written"
        sc = scratch.view(torch.float64)
        return dict(AI=_part(sc, L["ai"], (qg, npad, npad)), E=_part(sc, L["e"], (qg, npad, npad)),
                    G=_part(sc, L["g"], (qg, m, npad, npad)), xs=_part(sc, L["xs"], (qg, d, npad)),
                    yv=_part(sc, L["yv"], (qg, m, npad)), uv=_part(sc, L["uv"], (qg, m, npad)), YP=_part(sc, L["yp"], (ppad, npad)),
                    Q=_part(sc, L["q"], (qg, ppad, npad)), tp=_part(sc, L["tp"], (qg, L["npair"], nb)),
                    cp=_part(sc, L["cp"], (qg, L["npb"], nb, sb.HS_SLOTS)), dot=_part(sc, L["dot"], (qg, m, m)),
                    out=out[k0:k0 + qg].clone())


def _hess_case(group, eng, x, Y, sr, th, kernel, k0=0, qg=None):
    n, d, p = eng.n, eng.d, eng.p
    qg = eng.q_local - k0 if qg is None else qg
    r = _three(_run_hess, eng, k0, qg)
    for kk in range(qg):
        k = k0 + kk
        tag = "n=%d d=%d p=%d k%d" % (n, d, p, k)
        V, b, z = _fetch(eng, 2, k, True), _fetch(eng, 0, k, False), _fetch(eng, 1, k, False)
        R = sb.hess_parts(r["xs"][kk], sr, th[k], kernel, n)
        AI, G, E, yv = r["AI"][kk], r["G"][kk], r["E"][kk], r["yv"][kk]
        _record(group, "hess_prep", sb.check_hess_prep(r["xs"][kk], yv, x, sr, th[k], b, z), tag)
        _record(group, "hess_mirror", sb.check_hess_mirror(AI, G[d], G[d + 1], V, sr, th[k], n, d), tag)
        _record(group, "hess_da", sb.check_hess_da(E, R, d - 1), tag)
        _record(group, "hess_y", sb.check_hess_y(yv, R, z), tag)
        _record(group, "hess_g", sb.check_hess_g(G, AI, E, R), tag)
        _record(group, "hess_trace", sb.check_hess_trace(r["tp"][kk], G, n), tag)
        _record(group, "hess_contract", sb.check_hess_contract(r["cp"][kk], AI, R, z, th[k]), tag)
        _record(group, "hess_vectors", sb.check_hess_vectors(r["uv"][kk], r["dot"][kk], r["YP"], r["Q"][kk], AI, yv, Y, n), tag)
        _record(group, "hess_out", sb.check_hess_out(r["out"][kk], r["YP"], r["uv"][kk], r["Q"][kk], b, z, r["tp"][kk], r["cp"][kk],
                                                     r["dot"][kk], th[k], n, d, p), tag)
        del V, R
    return r


HESS_DIMS = (1, 3, 4, 5, 6, 7, 9, 17)
HESS_N = (63, 64, 65, 127, 128, 129, 200, 257)


@pytest.mark.parametrize("d", HESS_DIMS)
def test_hess_dimensions(d):
    """n = 129: one block of four dimensions against two (4 / 5, the second reaching past d), m = 8 against 9 (6 / 7: one HS_JC
    chunk of j against two), three blocks and six pairs (9), five blocks, fifteen pairs and three chunks (17)"""
    eng, x, Y, sr, th = _engine(7000 + d, 129, d)
    _hess_case("hess_dims", eng, x, Y, sr, th, "matern32")


@pytest.mark.parametrize("n", HESS_N)
def test_hess_training_set_sizes(n):
    """d = 5: npad = 128 with the second band all padding (63), exact and ragged bands, npad = 384 with six bands and three
    128-tiles a side (257)"""
    eng, x, Y, sr, th = _engine(7100 + n, n, 5)
    _hess_case("hess_sizes", eng, x, Y, sr, th, "matern32")


@pytest.mark.parametrize("p", [1, 4, 128, 129])
def test_hess_outputs(p):
    """n = 129, d = 5: ppad = 128 and 256 (p = 129: two row tiles of Q = Y A^-1)"""
    eng, x, Y, sr, th = _engine(7200 + p, 129, 5, p=p)
    _hess_case("hess_outputs", eng, x, Y, sr, th, "matern32")


@pytest.mark.parametrize("n,d", [(129, 5), (200, 9)])
@pytest.mark.parametrize("rep", [False, True], ids=["full", "rep"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_hess_kernels_and_replicated_path(kernel, rep, n, d):
    eng, x, Y, sr, th = _engine(7300 + n, n, d, kernel=kernel, rep=rep)
    _hess_case(_group("hess_rep" if rep else "hess_full", kernel), eng, x, Y, sr, th, kernel)


def test_hess_groupings():
    """(k0, q_group) = (0, 3), (1, 2), (2, 1) on the replicated path: the rows outside the group keep the fill (asserted in
    _run_hess), the group's rows are bitwise those of the (0, 3) call, and every stage holds in every grouping"""
    eng, x, Y, sr, th = _engine(7400, 129, 5, rep=True)
    base = _hess_case("hess_groups", eng, x, Y, sr, th, "matern32", 0, 3)["out"]
    for k0, qg in ((1, 2), (2, 1)):
        r = _hess_case("hess_groups", eng, x, Y, sr, th, "matern32", k0, qg)
        assert torch.equal(_bits(r["out"]), _bits(base[k0:k0 + qg])), ("grouping changes the result", k0, qg)


# ---- lcgp_predict_paramgrad ------------------------------------------------------------------------------------------------
def _run_pp(fill, eng, x0, same, ldo, k0, qg):
    q, n, d, p, n0 = eng.q_local, eng.n, eng.d, eng.p, x0.shape[0]
    lib, dev = eng.lib, eng.device
    L = sb.pgrad_layout(n, d, p, qg, n0)
    m, npad, ppad, n0r, nsum = L["m"], L["npad"], L["ppad"], L["n0r"], L["nsum"]
    with torch.cuda.device(dev):
        nbytes = _bytes(lib.lcgp_predict_paramgrad_scratch_bytes, eng.dtype, n, d, p, qg, n0)
        assert nbytes == L["total"], ("pgrad_layout against lcgp_predict_paramgrad_scratch_bytes", nbytes, L["total"])
        scratch = _filled((nbytes,), torch.uint8, fill, dev)
        g = _filled((2, q, ldo), torch.float64, fill, dev)
        dg = _filled((2, q, ldo, m), torch.float64, fill, dev)
        dn = _filled((q, ldo, p), torch.float64, fill, dev)
        x0d = _dev(eng, x0)
        _hip.check(lib.lcgp_predict_paramgrad(*eng._head(Y=True), k0, qg, n0, eng._p(x0d), int(same), eng._p(scratch), eng._p(g[0]),
                                              eng._p(g[1]), eng._p(dg[0]), eng._p(dg[1]), eng._p(dn), ldo), "lcgp_predict_paramgrad")
        for t, dim in ((g, 1), (dg, 1), (dn, 0)):
            assert _outside_keeps_fill(t, k0, qg, fill, dim), "outputs of components outside the group are written"
        for t in (g[:, :, n0:], dg[:, :, n0:], dn[:, n0:]):
            assert bool(torch.all(t.contiguous().view(torch.uint8) == fill)), "the tail n0 .. out_stride of an output row is written"
        sc = scratch.view(torch.float64)
        return dict(V=_part(sc, L["x"], (qg, n0r, npad))[:, :n0, :n].clone(), T=_part(sc, L["u"], (qg, n0r, npad))[:, :n0, :n].clone(),
                    E=_part(sc, L["e"], (qg, npad, npad)), xs=_part(sc, L["xs"], (qg, d, npad)), yv=_part(sc, L["yv"], (qg, m, npad)),
                    YT=_part(sc, L["yt"], (npad, ppad)), VY=_part(sc, L["vy"], (qg, n0r, ppad))[:, :n0].clone(),
                    rd=_part(sc, L["rd"], (qg, d, n0r))[:, :, :n0].clone(), sums=_part(sc, L["sum"], (qg, n0r, nsum))[:, :n0].clone(),
                    g=g[:, k0:k0 + qg, :n0].clone(), dg=dg[:, k0:k0 + qg, :n0].clone(), dn=dn[k0:k0 + qg, :n0].clone())


def _pp_case(group, eng, x, Y, sr, th, kernel, x0, same=0, ldo=None, k0=0, qg=None):
    n, d, p, n0 = eng.n, eng.d, eng.p, x0.shape[0]
    qg = eng.q_local - k0 if qg is None else qg
    r = _three(_run_pp, eng, x0, same, ldo or n0, k0, qg)
    if same == 0:
        first = _run_pgrad(0xFF, eng, x0, n0)
        assert torch.equal(_bits(r["V"]), _bits(first["V"][k0:k0 + qg])), "V is not bitwise that of lcgp_predict_grad"
        assert torch.equal(_bits(r["g"]), _bits(first["g"][:, k0:k0 + qg])), "ghat / gvar are not bitwise those of lcgp_predict_grad"
        del first
    for kk in range(qg):
        k = k0 + kk
        tag = "n=%d d=%d p=%d n0=%d same=%d k%d" % (n, d, p, n0, same, k)
        b, z = _fetch(eng, 0, k, False), _fetch(eng, 1, k, False)
        R = sb.hess_parts(r["xs"][kk], sr, th[k], kernel, n)
        V, T, E, yv = r["V"][kk], r["T"][kk], r["E"][kk], r["yv"][kk]
        _record(group, "hess_prep", sb.check_hess_prep(r["xs"][kk], yv, x, sr, th[k], b, z), tag)
        _record(group, "hess_da", sb.check_hess_da(E, R, d - 1), tag)
        _record(group, "pp_y", sb.check_pp_y(yv, R, z), tag)
        _record(group, "pp_t", sb.check_pp_t(T, V, E, n0, n), tag)
        _record(group, "pp_rowdot", sb.check_pp_rowdot(r["rd"][kk], T, V, R, n0), tag)
        _record(group, "pp_sums", sb.check_pp_sums(r["sums"][kk], x0, r["xs"][kk], z, V, yv, sr, th[k], kernel, same, n0, n), tag)
        _record(group, "pp_vy", sb.check_pp_vy(r["YT"], r["VY"][kk], V, Y, n0, n), tag)
        _record(group, "pp_out", sb.check_pp_out(r["dg"][0, kk], r["dg"][1, kk], r["dn"][kk], r["sums"][kk], r["rd"][kk], r["VY"][kk],
                                                 th[k], d, p, n0), tag)
        del R
    return r


@pytest.mark.parametrize("d", [1, 15, 16, 17, 33])
def test_pp_dimensions(d):
    """n = 129, n0 = 20, three training inputs among x0: one PP_DB = 16 block, full (16), two (17) and three (33)"""
    eng, x, Y, sr, th = _engine(7500 + d, 129, d)
    _pp_case("pp_dims", eng, x, Y, sr, th, "matern32", _x0(7600 + d, 20, d, x, 3))


@pytest.mark.parametrize("n", [127, 129, 257])
def test_pp_training_set_sizes(n):
    eng, x, Y, sr, th = _engine(7700 + n, n, 5)
    _pp_case("pp_sizes", eng, x, Y, sr, th, "matern32", _x0(7800 + n, 65, 5, x, 3))


def test_pp_rows():
    """n = 200, d = 5, out_stride = n0 + 3: n0 on both sides of predict_pad (64 below 128 rows) and of the 128-row slab"""
    eng, x, Y, sr, th = _engine(7900, 200, 5, q=2)
    for n0 in (1, 63, 64, 65, 127, 128, 129):
        nt = 3 if n0 > 3 else 0
        _pp_case("pp_rows", eng, x, Y, sr, th, "matern32", _x0(7901 + n0, n0, 5, x, nt), ldo=n0 + 3)


@pytest.mark.parametrize("p", [1, 129])
def test_pp_outputs(p):
    eng, x, Y, sr, th = _engine(8000 + p, 129, 5, p=p)
    _pp_case("pp_outputs", eng, x, Y, sr, th, "matern32", _x0(8100 + p, 65, 5, x, 3))


def test_pp_at_training_inputs():
    """same = 1 with x0 the training set (n0 = n = 129) and same = lo + 1 on the middle slice lo = 40 .. 90, as a chunked caller
    passes it, with out_stride > n0; the replicated path, so that s at c* is visible"""
    eng, x, Y, sr, th = _engine(8200, 129, 5, rep=True)
    _pp_case("pp_same", eng, x, Y, sr, th, "matern32", x.copy(), same=1)
    _pp_case("pp_same", eng, x, Y, sr, th, "matern32", x[40:90].copy(), same=41, ldo=53)


@pytest.mark.parametrize("rep", [False, True], ids=["full", "rep"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_pp_kernels_and_replicated_path(kernel, rep):
    eng, x, Y, sr, th = _engine(8300, 129, 17, kernel=kernel, rep=rep)
    _pp_case(_group("pp_rep" if rep else "pp_full", kernel), eng, x, Y, sr, th, kernel, _x0(8301, 65, 17, x, 3))


def test_pp_groupings():
    """(k0, q_group) = (0, 3), (1, 2), (2, 1): the outputs of the components outside the group keep the fill (asserted in
    _run_pp) and the group's outputs are bitwise those of the (0, 3) call"""
    eng, x, Y, sr, th = _engine(8400, 129, 5, rep=True)
    x0 = _x0(8401, 65, 5, x, 3)
    base = _pp_case("pp_groups", eng, x, Y, sr, th, "matern32", x0)
    for k0, qg in ((1, 2), (2, 1)):
        r = _pp_case("pp_groups", eng, x, Y, sr, th, "matern32", x0, k0=k0, qg=qg)
        for key, dim in (("g", 1), ("dg", 1), ("dn", 0)):
            want = base[key].narrow(dim, k0, qg)
            assert torch.equal(_bits(r[key]), _bits(want)), ("grouping changes the result", key, k0, qg)
