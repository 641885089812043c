"""Stage-wise componentwise bounds of the box-averaged predictions on the GPU (tests/stage_bounds.py), every run on three fills.

lcgp_predict_marginal and lcgp_condition_predict_marginal are called directly on an evaluated engine's workspace with buffers of
this test's own.  The scratch is read at the offsets do_predict_marginal carves (lcgp_hip.hip), and its size is asserted against
that arithmetic:
  model   X, U (q slabs n0pad x npad each), then the table (q d npad doubles) and I2 (q d doubles);
  view    X, U, at a 256-aligned offset Sigma_0n and T (q slabs n0pad x mpad each), at the next 256-aligned offset the table,
          I2 and the table over xn (q d mpad doubles).
Before each run the scratch, the outputs (ghat, gvar, gcov) and the widened reference row are filled with 0x00, 0xFF (NaN in both
precisions) and 0x5A bytes in turn: everything read back must be bitwise identical over the fills, the output columns between n0
and out_stride must keep the fill, and every check of the 0xFF run must be at or below 1:
    table (the 1-D averages and I2 against mpmath; padding columns bitwise 1), cross (the masked rows; rows with an empty mask
    bitwise lcgp_predict's), u (U = X W^T), out (ghat, gvar with the averaged prior); on a view table_n (the table over xn),
    cond_cross (Sigma_0n), cond_t (T), cond_out (against the ghat / gvar of the model's own call on the same rows, whose X, U,
    table and I2 the view's first launches must equal bitwise); gcov (the widened row bitwise [U_r | T_r], then the covariances).
Entries of x0 and of the reference row under their masks are NaN on the device throughout.

Shapes (the smallest that reach every path): n in {127, 128, 129, 257} (npad 128, 256, 384: the second 256-thread block of the
table kernel, part full), d in {1, 3, 32, 33, 34, 126}, n0 in {1, 63, 64, 65, 129}, m in {1, 64, 65, 130}, q_local = 2, the three
kernels, both precisions, the full path and the replicated one.  Lengthscales run from 0.02 to 30 within a theta row.

Run with -s to see the worst ratio per case group, dtype and stage, and the worst error of I1 relative to its exact value per box
class (profiles/stage_bounds_marginal.txt holds that report from an MI355X)."""
import ctypes as C
from collections import defaultdict

import numpy as np
import pytest
import torch

from lcgp_amd import _hip
from lcgp_amd.engine import HotPathEngine
from tests import stage_bounds as sb
from tests.test_gpu_condition_bounds import _align256, _bytes, _dev, _keeps, _state_views
from tests.test_gpu_stage_bounds import FILLS, _bits, _fetch, _filled, _problem
from tests.test_stage_bounds_cpu import _mg_rows

pytestmark = pytest.mark.gpu

KERNELS = ("matern32", "se", "matern52")
GROUP = {"matern32": "m32", "se": "se", "matern52": "m52"}
Q = 2

WORST = defaultdict(lambda: sb.Check(0.0, ()))       # (group, dtype, stage) -> worst Check over the group's cases
REL_I1 = defaultdict(float)                           # (box class, kernel) -> worst |I1 - exact| / exact in units of u


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst ratio |error| / bound per case group, dtype and stage of the box-averaged predictions (<= 1 passes)")
    for key in sorted(WORST):
        c = WORST[key]
        print("  %-12s %-8s %-11s %.3e  at %s" % (key + (c.ratio, c.where)))
    print("worst error of the table's I1 relative to the exact value, in units of u = 2^-53, per box class and kernel "
          "(entries above 1e-290)")
    for key in sorted(REL_I1):
        print("  %-10s %-9s %.3e" % (key + (REL_I1[key],)))


def _record(group, dtype, stage, c, where_extra=None):
    key = (group, dtype, stage)
    if c.ratio >= WORST[key].ratio:
        WORST[key] = sb.Check(c.ratio, (where_extra,) + tuple(c.where) if where_extra is not None else c.where)
    assert c.ratio <= 1.0, (group, dtype, stage, c, where_extra)


def _nan_under(a, mask):
    return np.where(np.asarray(mask) != 0, np.nan, np.nan_to_num(np.asarray(a, np.float64)))


def _call(fill, eng, view, x0, mask, box, ldo, entry="cond", ref=None):
    """one pass on freshly filled memory; everything the checks read, cloned.  view: the dict of HotPathEngine.condition_begin or
    None.  entry: "plain" = lcgp_predict_marginal (model only).  ref: None, or a dict with row (the pass row whose widened row is
    written out; None: none), inp (a widened row from another call, or "own": the one this call writes), x, mask (the reference
    row's values and mask): gcov is computed when inp is given"""
    q, d, n, n0 = eng.q_local, eng.d, eng.n, x0.shape[0]
    m = 0 if view is None else view["m"]
    npad, mpad, n0pad = sb._pad128(n), (sb._pad128(m) if m else 0), sb.predict_pad(n0)
    lib, dev, p = eng.lib, eng.device, eng._p
    esz = torch.empty((), dtype=eng.tdtype).element_size()
    slab, cslab = n0pad * npad, n0pad * mpad
    res = {}
    with torch.cuda.device(dev):
        st = eng._stream()
        if entry == "plain":
            nbytes = _bytes(lib.lcgp_predict_marginal_scratch_bytes, eng.dtype, n, d, q, n0)
        else:
            nbytes = _bytes(lib.lcgp_condition_predict_marginal_scratch_bytes, eng.dtype, n, d, q, m, n0)
        off_sg = _align256(2 * q * slab * esz)
        off_tab = 2 * q * slab * esz if m == 0 else off_sg + _align256(2 * q * cslab * esz)
        assert nbytes == off_tab + q * d * (npad + 1 + mpad) * 8, (nbytes, off_tab, q, d, npad, mpad)
        scratch = _filled((nbytes,), torch.uint8, fill, dev)
        out = _filled((3, q, ldo), torch.float64, fill, dev)
        x0d = _dev(eng, _nan_under(x0, mask))
        md = torch.as_tensor(np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)).to(dev)
        bd = torch.as_tensor(np.ascontiguousarray(box, np.float64)).to(dev)
        head = (st, eng.dtype, eng.kernel_id, n, d, eng.p, q, p(eng.x), p(eng.sr), p(eng.theta_dev), p(eng.workspace))
        if entry == "plain":
            assert view is None and ref is None
            _hip.check(lib.lcgp_predict_marginal(*head, n0, p(x0d), p(md), p(bd), p(scratch), p(out[0]), p(out[1]), ldo),
                       "lcgp_predict_marginal")
        else:
            vw = (None, 0, None) if view is None else (p(view["state"]), m, p(view["xn"]))
            refs = (0, None, None, None, None, None)
            if ref is not None:
                row = _filled((q, npad + mpad), eng.tdtype, fill, dev)
                if ref.get("inp") is not None and not isinstance(ref["inp"], str):
                    row.copy_(ref["inp"])
                xrd = _dev(eng, _nan_under(ref["x"], ref["mask"]).reshape(1, d))
                mrd = torch.as_tensor(np.ascontiguousarray(np.asarray(ref["mask"]).reshape(1, d) != 0, np.uint8)).to(dev)
                gives = ref.get("inp") is not None
                refs = (ref["row"] or 0, p(row) if ref.get("row") is not None else None, p(row) if gives else None,
                        p(xrd) if gives else None, p(mrd) if gives else None, p(out[2]) if gives else None)
            _hip.check(lib.lcgp_condition_predict_marginal(*head, *vw, n0, p(x0d), p(md), p(bd), p(scratch), nbytes, p(out[0]),
                                                           p(out[1]), ldo, *refs), "lcgp_condition_predict_marginal")
            if ref is not None:
                res["ref"] = row.clone()
        gc = ref is not None and ref.get("inp") is not None
        assert _keeps(out[:2 + gc, :, n0:], fill), "output columns between n0 and out_stride written"
        assert gc or _keeps(out[2], fill), "gcov written without a reference row"
        res["out"] = out[:2 + gc, :, :n0].clone()
        sc = scratch.view(eng.tdtype)
        res["X"] = sc[:q * slab].view(q, n0pad, npad).clone()
        res["U"] = sc[q * slab:2 * q * slab].view(q, n0pad, npad).clone()
        tb = scratch[off_tab:].view(torch.float64)
        res["tab"] = tb[:q * d * npad].view(q, d, npad).clone()
        res["i2"] = tb[q * d * npad:q * d * (npad + 1)].view(q, d).clone()
        if m:
            o = off_sg // esz
            res["Sg"] = sc[o:o + q * cslab].view(q, n0pad, mpad).clone()
            res["T"] = sc[o + q * cslab:o + 2 * q * cslab].view(q, n0pad, mpad).clone()
            res["tabn"] = tb[q * d * (npad + 1):].view(q, d, mpad).clone()
    return res


def _three(*args, **kw):
    base = _call(0xFF, *args, **kw)
    for f in FILLS:
        if f == 0xFF:
            continue
        other = _call(f, *args, **kw)
        assert other.keys() == base.keys()
        for key in base:
            assert torch.equal(_bits(other[key]), _bits(base[key])), ("fill 0x%02X changes" % f, key)
        del other
    return base


def _plain_X(eng, x0z):
    """X (q, n0pad, npad) of lcgp_predict(same = 0) on the rows x0z: the plain cross_kernel"""
    q, n, n0 = eng.q_local, eng.n, x0z.shape[0]
    nbytes = _bytes(eng.lib.lcgp_predict_scratch_bytes, eng.dtype, n, q, n0)
    scratch = _filled((nbytes,), torch.uint8, 0xFF, eng.device)
    out = _filled((2, q, n0), torch.float64, 0xFF, eng.device)
    x0d = _dev(eng, x0z)
    _hip.check(eng.lib.lcgp_predict(eng._stream(), eng.dtype, eng.kernel_id, n, eng.d, eng.p, q, eng._p(eng.x), eng._p(eng.sr),
                                    eng._p(eng.theta_dev), eng._p(eng.workspace), n0, eng._p(x0d), 0, eng._p(scratch),
                                    eng._p(out[0]), eng._p(out[1]), n0), "lcgp_predict")
    return scratch.view(eng.tdtype)[:q * sb.predict_pad(n0) * sb._pad128(n)].view(q, sb.predict_pad(n0), sb._pad128(n)).clone()


def _rel_i1(cls, kernel, tab, x, th, box, dtype, n):
    """the worst relative error of the table's I1 for the report (not asserted: the narrow-box loss is a property of the formula)"""
    xr = sb.rounded(x, dtype)
    for k in range(tab.shape[0]):
        for l in range(xr.shape[1]):
            ex = np.array([float(v) for v in sb.marg_exact(kernel, xr[:, l], box[0][l], box[1][l], th[k][l])])
            ok = ex > 1e-290
            if ok.any():
                rel = np.max(np.abs(tab[k, l, :n][ok] - ex[ok]) / ex[ok]) / sb.unit("float64")
                REL_I1[cls, kernel] = max(REL_I1[cls, kernel], float(rel))


def _case(group, eng, x, sr, th, kernel, dtype, x0, mask, box, view=None, vin=None, ldo=None, entry="cond", ref=None, cls=None):
    """the three-fill run and every check.  vin = (xn, t, r) of the view.  ref: _call's, with inp = "own" for the same pass"""
    q, n, d, n0 = eng.q_local, eng.n, eng.d, x0.shape[0]
    m = 0 if view is None else view["m"]
    npad, mpad = sb._pad128(n), (sb._pad128(m) if m else 0)
    res = _three(eng, view, x0, mask, box, ldo or n0, entry=entry, ref=ref)
    tag0 = "n=%d d=%d n0=%d m=%d" % (n, d, n0, m)

    def rec(stage, c, tag=tag0):
        _record(group, dtype, stage, c, tag)
    tab, i2 = res["tab"].cpu().numpy(), res["i2"].cpu().numpy()
    rec("table", sb.check_marg_table(tab, i2, x, th, box, kernel, dtype, n, npad))
    if cls is not None:
        _rel_i1(cls, kernel, tab, x, th, box, dtype, n)
    assert torch.all(res["X"][:, n0:, :] == 0) and torch.all(res["X"][:, :, n:] == 0), (group, dtype, tag0, "padding of X")
    empty = ~(np.asarray(mask) != 0).any(axis=1)
    plain = _plain_X(eng, np.nan_to_num(_nan_under(x0, mask))) if empty.any() else None
    base = None
    if m:
        xn, t, r = vin
        base = _call(0xFF, eng, None, x0, mask, box, n0, entry="plain")
        for key in ("X", "U", "tab", "i2"):
            assert torch.equal(_bits(base[key]), _bits(res[key])), (group, dtype, tag0, "the view's first launches differ", key)
        rec("table_n", sb.check_marg_table(res["tabn"].cpu().numpy(), i2, xn, th, box, kernel, dtype, m, mpad))
        un, wd, v = _state_views(eng, view["state"], m)
        sg = res["Sg"]
        assert torch.all(sg[:, n0:, :] == 0) and torch.all(sg[:, :, m:] == 0), (group, dtype, tag0, "padding of Sigma_0n")
    for k in range(q):
        tag = tag0 + " k%d" % k
        W, z = _fetch(eng, 1, k, True), _fetch(eng, 1, k, False)
        X, U = res["X"][k, :n0, :n], res["U"][k, :n0, :n]
        g = res["out"][:, k]
        rec("cross", sb.check_marg_cross(X, res["tab"][k], x0, mask, x, sr, th[k], kernel, dtype,
                                         plain=None if plain is None else plain[k, :n0, :n]), tag)
        rec("u", sb.check_cov_u(U, X, W, dtype), tag)
        if m == 0:
            rec("out", sb.check_marg_out(g[0], g[1], X, U, z, i2[k], mask, th[k], dtype), tag)
            Tm = None
        else:
            g0 = base["out"][:, k]
            rec("out", sb.check_marg_out(g0[0], g0[1], X, U, z, i2[k], mask, th[k], dtype), tag)
            Sg, Tm = sg[k, :n0, :m], res["T"][k, :n0, :m]
            rec("cond_cross", sb.check_marg_cond_cross(Sg, U, un[k, :m, :n], res["tabn"][k], x0, mask, xn, th[k], kernel, dtype), tag)
            rec("cond_t", sb.check_cov_u(Tm, Sg, wd[k][:m, :m], dtype), tag)
            rec("cond_out", sb.check_cond_out(g[0], g[1], Tm, v[k], g0[0], g0[1], m), tag)
        if ref is not None and ref.get("inp") is not None:
            rows = None
            if ref.get("row") is not None:
                rows = (res["U"][k, ref["row"]], res["T"][k, ref["row"]] if m else None)
            rec("gcov", sb.check_marg_refcov(g[2], res["U"][k, :n0], None if Tm is None else res["T"][k, :n0], res["ref"][k], x0, mask,
                                             ref["x"], ref["mask"], box, i2[k], th[k], kernel, dtype, n, m, ref_rows=rows), tag)
        del W
    return res


def _theta_rows(th, d, kernel):
    """lengthscales from 0.02 to 30 within each theta row (in place).  d <= 6: a geometric ladder, reversed for the second component;
    wider d: the extremes on dimensions 0 and 1 (swapped for the second component, which shares the other lengthscales with the
    first: the mpmath values are cached per lengthscale), 0.1 in place of 0.02 for SE, whose C0 is otherwise past its cut-off for
    nearly every pair and leaves the masked rows nothing to show"""
    if d == 1:
        th[:, 0] = (0.3, 2.0)[:th.shape[0]]
    elif d <= 6:
        lad = np.geomspace(0.02, 30.0, d)
        for k in range(th.shape[0]):
            th[k, :d] = lad if k % 2 == 0 else lad[::-1]
    else:
        small = 0.1 if kernel == "se" else 0.02
        th[1:, :d] = th[0, :d]
        th[0, 0], th[0, 1] = small, 30.0
        th[1:, 0], th[1:, 1] = 30.0, small
    return th


def _engine(seed, n, d, dtype, kernel, rep, ell=None):
    x, Y, sr, th = _problem(seed, n, d, 3, Q, rep=rep)
    if d > 6:
        x = np.asarray(x, np.float32).astype(np.float64)      # (both precisions then share the mpmath values of the table)
    th = _theta_rows(th, d, kernel)
    if ell is not None:
        th[:, :d] = ell
    eng = HotPathEngine(x, Y, sr=sr, q_local=Q, dtype=dtype, kernel=kernel)
    out = eng.evaluate(th)
    assert np.all(out[:, 2] == 0), out[:, 2]
    return eng, x, sr, th


def _box(d, lo, hi):
    return np.stack([np.full(d, float(lo)), np.full(d, float(hi))])


def _view(eng, seed, m, d, rep, x0=None, mask=None, equal=()):
    """m new inputs inside and outside the unit box (so also of any sub-box), observations and counts; rows `equal` = ((i, j), ..) of
    x0 are set to rows of xn where they keep the dimension (in place)"""
    rng = np.random.default_rng(seed)
    xn = rng.uniform(-0.2, 1.2, (m, d))
    if d > 6:
        xn = np.asarray(xn, np.float32).astype(np.float64)
    t = rng.standard_normal((Q, m))
    r = (1.0 + rng.permutation(m) % 3) if rep else None
    for i, j in equal:
        x0[i] = np.where(mask[i], np.nan, xn[j % m])
    return eng.condition_begin(xn, t, r), (xn, t, r)


SHAPES = [(127, 1, 1), (128, 3, 63), (129, 32, 64), (257, 33, 65), (129, 34, 129), (127, 126, 64)]      # (n, d, n0)


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_edges_of_n_d_and_n0(dtype, kernel):
    """every (n, d, n0) of SHAPES through lcgp_predict_marginal, the default box and a sub-box in turn, the full and the replicated
    path in turn (each kernel sees both); n0 = 1 is a masked row"""
    for i, (n, d, n0) in enumerate(SHAPES):
        rep = bool((i + KERNELS.index(kernel)) % 2)
        eng, x, sr, th = _engine(2100 + i, n, d, dtype, kernel, rep)
        x0, mask = _mg_rows(d, n0, 2110 + i, shift=4 if n0 == 1 else 0)
        box = _box(d, 0.0, 1.0) if i % 2 else _box(d, 0.3, 0.75)
        _case(("rep_" if rep else "full_") + GROUP[kernel], eng, x, sr, th, kernel, dtype, x0, mask, box, entry="plain")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_boxes(dtype, kernel):
    """n = 129, d = 3, lengthscales 0.02, 0.77, 30 (and reversed): the default box; a sub-box with inputs outside on both sides; a
    narrow box (w = 1e-3: the error relative to I1 grows like ell / w, which the bound admits and the report records); a box more
    than one of the longest lengthscales away from every input (every entry takes the tail branch; the short lengthscales
    underflow); a box whose ends are coordinates of training inputs (x on lo and on hi exactly)"""
    n, d, n0 = 129, 3, 65
    eng, x, sr, th = _engine(2200, n, d, dtype, kernel, True)
    x0, mask = _mg_rows(d, n0, 2201)
    xs = np.sort(sb.rounded(x, dtype), axis=0)         # (the stored inputs: x sits on lo and on hi in both precisions)
    boxes = dict(default=_box(d, 0.0, 1.0), sub=_box(d, 0.3, 0.75), narrow=_box(d, 0.4, 0.401), far=_box(d, 40.0, 41.0),
                 edges=np.stack([xs[20], xs[100]]))
    for cls, box in boxes.items():
        assert cls != "far" or np.all((box[0] - x.max(axis=0)) / th[:, :d].max() > 1.0)
        assert cls != "sub" or (np.any(x < box[0]) and np.any(x > box[1]))
        _case("box_" + cls, eng, x, sr, th, kernel, dtype, x0, mask, box, cls=cls)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_lengthscales_at_the_c0_cutoff(dtype, kernel):
    """every lengthscale at 1e-6: b is 1e5 and more for every input outside the sub-box (the tails are zero), inside it both F
    saturate; the kept dimensions of the masked rows are past the C0 cut-off.  Every output stays finite"""
    n, d, n0 = 129, 3, 64
    eng, x, sr, th = _engine(2300, n, d, dtype, kernel, False, ell=1e-6)
    x0, mask = _mg_rows(d, n0, 2301)
    res = _case("cutoff", eng, x, sr, th, kernel, dtype, x0, mask, _box(d, 0.3, 0.75), ldo=200)
    assert torch.all(torch.isfinite(res["out"]))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_view(dtype, kernel):
    """m in {1, 64, 65, 130} at d = 3 and m = 65 at d = 34 (the table over xn restaged per 32-dimension chunk), n = 129, n0 = 65, a
    sub-box with xn inside and outside it, rows 0, 6, 9 of x0 equal to rows of xn where they keep the dimension; the replicated
    path (counts 1 .. 3) in turn"""
    for i, (m, d) in enumerate([(1, 3), (64, 3), (65, 3), (130, 3), (65, 34)]):
        rep = bool((i + KERNELS.index(kernel)) % 2)
        eng, x, sr, th = _engine(2400 + i, 129, d, dtype, kernel, rep)
        x0, mask = _mg_rows(d, 65, 2410 + i)
        view, vin = _view(eng, 2420 + i, m, d, rep, x0, mask, equal=((0, 0), (6, 63), (9, 64)))
        _case("view_" + GROUP[kernel], eng, x, sr, th, kernel, dtype, x0, mask, _box(d, 0.3, 0.75), view=view, vin=vin, ldo=70)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_gcov(dtype, kernel):
    """the covariance with a reference row, on the model (m = 0) and on a view (m = 65): reference rows with an empty, a full and a
    mixed mask (rows 0, 3, 4 of the pass), once written out and read in the same pass -- row r then equals the reference row --
    and once taken from another call, whose rows are others but for row 2, a copy of the reference row"""
    n, d, n0 = 129, 3, 65
    eng, x, sr, th = _engine(2500, n, d, dtype, kernel, True)
    box = _box(d, 0.3, 0.75)
    x0, mask = _mg_rows(d, n0, 2501)
    xb, mb = _mg_rows(d, 33, 2502, shift=2)
    for m in (0, 65):
        view, vin = (None, None) if m == 0 else _view(eng, 2503, m, d, True)
        for r in (0, 3, 4):
            ref = dict(row=r, inp="own", x=x0[r], mask=mask[r])
            res = _case("gcov_" + GROUP[kernel], eng, x, sr, th, kernel, dtype, x0, mask, box, view=view, vin=vin, ref=ref)
            xb[2], mb[2] = x0[r], mask[r]
            other = dict(row=None, inp=res["ref"], x=x0[r], mask=mask[r])
            _case("gcov_" + GROUP[kernel], eng, x, sr, th, kernel, dtype, xb, mb, box, view=view, vin=vin, ref=other)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_both_entries_agree_bitwise(dtype):
    """lcgp_condition_predict_marginal without a state (m = 0) against lcgp_predict_marginal on the same rows: the same launches"""
    n, d, n0 = 128, 3, 63
    eng, x, sr, th = _engine(2600, n, d, dtype, "matern52", False)
    x0, mask = _mg_rows(d, n0, 2601)
    box = _box(d, 0.0, 1.0)
    a = _call(0xFF, eng, None, x0, mask, box, n0, entry="plain")
    b = _call(0xFF, eng, None, x0, mask, box, n0, entry="cond")
    assert a.keys() == b.keys()
    for key in a:
        assert torch.equal(_bits(a[key]), _bits(b[key])), key
