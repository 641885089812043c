"""The Sobol stage bounds of tests/stage_bounds.py have teeth (no GPU).

sobol_J, sobol_moments and sobol_segment of lcgp_hip.hip are restated here in numpy operation by operation (the 30-term Horner
chain with the backward recurrence, expm1 and the forward recurrence from gamma L = 4 on, the three anchored segments, the SE
branches), and the pair, subset and reduce launches are emulated around them: the table from tests/marginal_ref.py, the tile sums
part[pair, r, c, s] in a scratch that holds only the last batch, out in batches of 64 pairs and chunks of 32 masks.  The emulation
passes sobol_means, sobol_element (against mpmath), sobol_tile, sobol_rows and sobol_reduce with ratios at or below 1, and each
defect fails the check of its own stage (the defects of sobol_J over the case table itself, which is what the GPU test sends):
  element  the series used at gamma L >= 4; the forward recurrence at gamma L = 0.1; ten series terms; the SE near-branch
           formula in the far tail; the middle segment anchored at the wrong centre; a subset product with one mask bit shifted;
           the second chunk's masks taken from the first
  tile     `twice` on a diagonal tile; the ragged last column included with stale data; a tile of pair r in the slot of pair
           r + 1 in the second batch; one element of a far tile off by 1e-9 of its own value (which today's bar, 1e-12 of the whole
           sum's size, passes)
  rows     the out row offset of the second batch off by one row
  reduce   an upper tile of a pair k = k' read by the reduction
Also here: every branch class of sb.sobol_classes holds at least 8 elements of the case table per kernel; the measurement of
tests/sobol_ref.pair_integral against mpmath that sets sb.SOBOL_KJ; sb.sobol_exact_J against quadrature; the layout restatements
against the library's *_scratch_bytes entries.
The matrix-weighted pass and the view: the emulation with a matrix Q passes sobol_tile / sobol_rows with the S0 column;
sobol_stage_q without the mirror in a diagonal tile and the view's D A^-1 added beyond nt fail sobol_tile; P with L_S^-1 transposed
fails sobol_p; a K-stage left out of E = P P^T fails sobol_e."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

from tests import marginal_ref as mref
from tests import sobol_ref
from tests import stage_bounds as sb

KERNELS = ("matern32", "se", "matern52")
BOXES = ((0.0, 1.0), (0.3, 0.75))
TS = sb.TS


# ----------------------------------------------------------------------------------------------------------------------
# the device functions, restated
# ----------------------------------------------------------------------------------------------------------------------
def emul_moments(g, L, NT, defect=None):
    x = g * L
    eL = np.exp(-x)
    Ln = [np.ones_like(L)]
    for n in range(1, NT + 2):
        Ln.append(Ln[-1] * L)
    terms = 10 if defect == "ten_terms" else 30
    s = np.ones_like(x)
    for j in range(terms, 0, -1):
        s = (s * x) * (1.0 / (NT + 1 + j)) + 1.0
    ms = [None] * (NT + 1)
    ms[NT] = eL * Ln[NT + 1] * s * (1.0 / (NT + 1))
    for n in range(NT, 0, -1):
        ms[n - 1] = (g * ms[n] + Ln[n] * eL) * (1.0 / n)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rg = 1.0 / g
        mf = [-np.expm1(-x) * rg]
        for n in range(1, NT + 1):
            mf.append((n * mf[n - 1] - Ln[n] * eL) * rg)
    small = x < 4.0
    if defect == "series_everywhere":
        small = np.ones_like(small)
    if defect == "forward_small":
        small = x < 0.05
    return [np.where(small, a, b) for a, b in zip(ms, mf)]


def emul_segment(kernel, L, s0a, s0b, al, be, defect=None):
    NT = 2 if kernel == "matern32" else 4
    m = emul_moments(al + be, L, NT, defect)
    if kernel == "matern32":
        a0, b0 = 1.0 + s0a, 1.0 + s0b
        tot = a0 * b0 * m[0] + (a0 * be + al * b0) * m[1] + al * be * m[2]
    else:
        a0, a1, a2 = 1.0 + (s0a * (1.0 / 3.0) * s0a + s0a), al * (s0a * (2.0 / 3.0) + 1.0), al * al * (1.0 / 3.0)
        b0, b1, b2 = 1.0 + (s0b * (1.0 / 3.0) * s0b + s0b), be * (s0b * (2.0 / 3.0) + 1.0), be * be * (1.0 / 3.0)
        tot = a0 * b0 * m[0] + (a0 * b1 + a1 * b0) * m[1] + ((a0 * b2 + a2 * b0) + a1 * b1) * m[2] + (a1 * b2 + a2 * b1) * m[3] + \
            a2 * b2 * m[4]
    return np.exp(-(s0a + s0b)) * tot


def emul_J(kernel, u, a, v, b, lo, hi, defect=None):
    """sobol_dim + sobol_J of lcgp_hip.hip in numpy (arrays broadcast)"""
    u, a, v, b, lo, hi = np.broadcast_arrays(*(np.asarray(t, np.float64) for t in (u, a, v, b, lo, hi)))
    if kernel == "se":
        p = sb._sobol_se_parts(u, a, v, b, lo, hi)
        F = lambda t: mref.F("se", t)                      # noqa: E731
        Fc = lambda t: mref.Fc("se", t)                    # noqa: E731
        far = p["bn"] > 1.0
        if defect == "se_near_in_far":
            far = np.zeros_like(far)
        r = np.where(p["inside"], F(p["b1"]) + F(p["b2"]), np.where(far, Fc(p["bn"]) - Fc(p["bf"]), F(p["bf"]) - F(p["bn"])))
        return p["pref"] * p["c1"] * r * p["rw"]
    p = sb._sobol_matern_parts(u, a, v, b, lo, hi)
    uu, vv, ra, rb, cu, cv = p["u"], p["v"], p["ra"], p["rb"], p["cu"], p["cv"]
    seg = lambda *args: emul_segment(kernel, *args, defect)           # noqa: E731
    tot = seg(cu - lo, np.abs(uu - cu) * ra, np.abs(vv - cu) * rb, ra, rb)
    left = rb <= ra
    if defect == "wrong_anchor":                           # the distances of the other end under the same slopes
        sa, sb_ = np.where(left, np.abs(cv - uu) * ra, np.abs(cu - uu) * ra), np.where(left, np.abs(vv - cv) * rb, np.abs(vv - cu) * rb)
    else:
        sa, sb_ = np.where(left, np.abs(cu - uu) * ra, np.abs(cv - uu) * ra), np.where(left, np.abs(vv - cu) * rb, np.abs(vv - cv) * rb)
    tot = tot + seg(cv - cu, sa, sb_, np.where(left, ra, -ra), np.where(left, -rb, rb))
    tot = tot + seg(hi - cv, np.abs(cv - uu) * ra, np.abs(cv - vv) * rb, ra, rb)
    return tot * (1.0 / (hi - lo))


def emul_element_rows(kernel, U, A, V, B, box, masks, defect=None):
    """(M_u - M_0) of one element per row: what the one-hot launches return"""
    U, A, V, B, box = (np.asarray(t, np.float64) for t in (U, A, V, B, box))
    m, d = U.shape
    J = np.stack([emul_J(kernel, U[:, l], A[:, l], V[:, l], B[:, l], box[0, l], box[1, l], defect) for l in range(d)], axis=1)
    Aa = np.stack([mref.I1(kernel, U[:, l], box[0, l], box[1, l], A[:, l]) * mref.I1(kernel, V[:, l], box[0, l], box[1, l], B[:, l])
                   for l in range(d)], axis=1)
    M0 = np.prod(Aa, axis=1)
    out = np.empty((m, len(masks)))
    for s, mask in enumerate(masks):
        if defect == "mask_shift" and mask:
            mask = (mask << 1) & ((1 << d) - 1) | (mask >> (d - 1))
        if defect == "chunk_masks" and s >= sb.SOBOL_CHUNK:
            mask = masks[s - sb.SOBOL_CHUNK]
        bits = np.array([(mask >> l) & 1 for l in range(d)], bool)
        out[:, s] = np.prod(np.where(bits, J, Aa), axis=1) - M0
    return out


def emul_pairs(kernel, x, w, ell, box, pairs, masks, defect=None, fill=np.nan, Q=None):
    """the table, the means, the scratch's part after the LAST batch (earlier batches overwritten, unwritten slots keep `fill`)
    and out (npairs, len(masks)) of the pair pass (masks = sb.sobol_std_masks(d)) or one chunk of the subset pass"""
    x, w, ell, box = (np.asarray(t, np.float64) for t in (x, w, ell, box))
    n, d = x.shape
    q = w.shape[0]
    nt = (n + TS - 1) // TS
    tab = np.stack([np.stack([mref.I1(kernel, x[:, l], box[0, l], box[1, l], ell[k, l]) for l in range(d)]) for k in range(q)])
    means = np.sum(w * np.prod(tab, axis=1), axis=1)
    npairs, cols = len(pairs), len(masks) + (1 if Q is not None else 0)     # (Q: per component a full matrix; one more sum, S0)
    part = np.full((min(npairs, sb.SOBOL_BATCH), nt, nt, cols), fill)
    out = np.full((npairs + 1, cols), fill)
    for p0 in range(0, npairs, sb.SOBOL_BATCH):
        nb = min(sb.SOBOL_BATCH, npairs - p0)
        for z in range(nb):
            k, kp = pairs[p0 + z]
            J = np.stack([emul_J(kernel, x[:, None, l], ell[k, l], x[None, :, l], ell[kp, l], box[0, l], box[1, l]) for l in range(d)], -1)
            Aa = tab[k].T[:, None, :] * tab[kp].T[None, :, :]
            M0 = np.prod(Aa, axis=-1)
            wgt = w[k][:, None] * w[kp][None, :]
            if Q is not None:
                Qk = np.array(Q[k], np.float64)
                if defect == "no_mirror":                  # sobol_stage_q without the mirrored write: zeros above the diagonal
                    for r in range(nt):
                        blk = Qk[r * TS:(r + 1) * TS, r * TS:(r + 1) * TS]
                        blk[np.triu_indices(blk.shape[0], 1)] = 0.0
                wgt = wgt * Qk
            el = np.stack([wgt * (np.prod(np.where([(m >> l) & 1 for l in range(d)], J, Aa), axis=-1) - M0) for m in masks], -1)
            if Q is not None:
                el = np.concatenate([el, (wgt * M0)[..., None]], axis=-1)
            if defect == "far_element" and p0 == 0 and z == 0:
                el[n - 1, 0] *= 1.0 + 1e-9
            slot = z + 1 if (defect == "slot_shift" and p0 > 0 and z + 1 < part.shape[0]) else z
            for r in range(nt):
                for c in range(nt):
                    if k == kp and c > r:
                        continue
                    t = el[r * TS:(r + 1) * TS, c * TS:(c + 1) * TS].sum(axis=(0, 1))
                    if defect == "ragged_stale" and (c + 1) * TS > n:
                        t = t + 1e-3 * np.abs(t) + 1e-300
                    twice = 2.0 if (k == kp and (c < r or defect == "twice_diag")) else 1.0
                    part[slot, r, c] = twice * t
            keep = np.tril(np.ones((nt, nt), bool)) if (k == kp and defect != "reduce_upper") else np.ones((nt, nt), bool)
            row = p0 + z + (1 if (defect == "out_offset" and p0 > 0) else 0)
            out[row] = part[z][keep].sum(axis=0)
    return dict(tab=tab, means=means, part=part, out=out[:npairs])


# ----------------------------------------------------------------------------------------------------------------------
# the case table and the constants
# ----------------------------------------------------------------------------------------------------------------------
_TABLE = {}


def case_table(kernel):
    """the case table of both boxes with the reference's and the emulation's J measured against mpmath: computed once"""
    if kernel not in _TABLE:
        per = []
        for lo, hi in BOXES:
            rows = sb.sobol_cases(kernel, lo, hi)
            ref = sobol_ref.pair_integral(kernel, lo, hi, rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3])
            rel, ex = sb.sobol_j_measure(kernel, ref, rows, lo, hi)
            per.append(dict(lo=lo, hi=hi, rows=rows, ref=ref, rel=rel, exact=ex,
                            classes=sb.sobol_classes(kernel, rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], lo, hi)))
        _TABLE[kernel] = per
    return _TABLE[kernel]


def element_inputs(rows, lo, hi, d, first=0, count=None):
    """(U, A, V, B, box) of the element stage at input dimension d from the 1-D table: input l < 3 walks the table shifted by
    7 l rows, the others hold two benign centres and scales (one J each, cached in the mpmath reference)"""
    m = len(rows)
    idx = np.arange(first, first + (count or m)) % m
    U, A, V, B = (np.empty((len(idx), d)) for _ in range(4))
    for l in range(d):
        if l < 3:
            sel = rows[(idx + 7 * l) % m]
            U[:, l], A[:, l], V[:, l], B[:, l] = sel.T
        else:
            w = hi - lo
            U[:, l], V[:, l] = lo + (0.4 if l % 2 else 0.55) * w, lo + (0.7 if l % 2 else 0.35) * w
            A[:, l], B[:, l] = (0.8 if l % 2 else 1.7) * w, (1.3 if l % 2 else 0.9) * w
    return U, A, V, B, np.stack([np.full(d, lo), np.full(d, hi)])


def subset_masks(d, count, seed=5):
    """the empty mask, the full one, singletons, complements and random masks: `count` of them"""
    full = (1 << d) - 1
    ms = [0, full] + [1 << l for l in range(d)] + [full ^ (1 << l) for l in range(d)]
    rng = np.random.default_rng(seed)
    while len(ms) < count:
        ms.append(int(rng.integers(1, full + 1)))
    return ms[:count]


@pytest.mark.parametrize("kernel", KERNELS)
def test_every_branch_class_holds_eight_elements(kernel):
    tot = {}
    for t in case_table(kernel):
        for name, sel in t["classes"].items():
            tot[name] = tot.get(name, 0) + int(np.sum(sel))
    print(kernel, tot)
    assert all(v >= 8 for v in tot.values()), tot
    assert sum(len(t["rows"]) for t in case_table(kernel)) <= 500


def measured_kj(kernel):
    out = {}
    for t in case_table(kernel):
        r = t["rows"]
        p = sb._sobol_matern_parts(r[:, 0], r[:, 1], r[:, 2], r[:, 3], t["lo"], t["hi"])
        for s, kind in ((0, "outer"), (1, "middle"), (2, "outer")):
            for br in ("series", "forward"):
                sel = (p["L"][s] > 0.0) & ((p["x"][s] < sb.SOBOL_SERIES_BELOW) == (br == "series")) & ~np.isnan(t["rel"])
                assert sel.sum() >= 8
                out[kind, br] = max(out.get((kind, br), 0.0), float(np.max(t["rel"][sel])))
                out[kind, br, 0] = max(out.get((kind, br, 0), 0.0), float(np.max(t["rel"][sel] / (1.0 + p["smin"][sel]))))
    return out


@pytest.mark.parametrize("kernel", ("matern32", "matern52"))
def test_matern_constants_are_the_measured_reference_error(kernel):
    """SOBOL_KJ is the worst error of the REFERENCE against mpmath per class in units of u relative to J, rounded up: not below
    the measurement, and not above it by more than rounding up (nothing fitted to a device)"""
    for key, val in sorted(measured_kj(kernel).items(), key=str):
        k = sb.SOBOL_KJ[(kernel,) + key] if len(key) == 2 else sb.SOBOL_KJ0[(kernel,) + key[:2]]
        print("reference against mpmath  %-9s %-7s %-8s measured %8.3f %-10s constant %g" %
              ((kernel,) + key[:2] + (val, "u" if len(key) == 2 else "u (1 + s0)", k)))
        assert val <= k <= np.ceil(val) + 1.0, (kernel, key, val, k)


def test_se_reference_meets_the_derived_bound():
    for t in case_table("se"):
        r = t["rows"]
        bd = sb._sobol_se_bound(r[:, 0], r[:, 1], r[:, 2], r[:, 3], t["lo"], t["hi"])
        ok = ~np.isnan(t["rel"])
        ratio = t["rel"][ok] * t["exact"][ok] / (sb.C * bd[ok])
        print("se reference against mpmath: worst |error| / (C bound) %.3f, worst error %.1f u relative to J" %
              (ratio.max(), t["rel"][ok].max()))
        assert ratio.max() <= 1.0
        assert np.median(ratio) > 1e-3                     # the bound follows the error: it is not orders above everywhere


@pytest.mark.parametrize("kernel", KERNELS)
def test_exact_J_against_quadrature(kernel):
    def kap(s):
        return mp.exp(-s * s / 2) if kernel == "se" else ((1 + s) if kernel == "matern32" else (1 + s + s * s / 3)) * mp.exp(-s)
    for (u, a, v, b, lo, hi) in [(0.2, 0.3, 0.7, 1.0, 0.0, 1.0), (0.9, 0.05, -0.2, 2.0, 0.3, 0.75), (0.5, 1.0, 0.5, 1.0, 0.0, 1.0),
                                 (1.4, 0.2, 1.1, 0.21, 0.0, 1.0), (0.31, 3.0, 0.74, 3.0 * (1 + 1e-12), 0.3, 0.75)]:
        with mp.workdps(30):
            pts = sorted({lo, hi, min(max(u, lo), hi), min(max(v, lo), hi)})
            want = mp.quad(lambda t: kap(abs(t - u) / a) * kap(abs(t - v) / b), pts) / (mp.mpf(hi) - mp.mpf(lo))
            assert abs(sb.sobol_exact_J(kernel, u, a, v, b, lo, hi) - want) <= mp.mpf(10) ** -25 * want


# ----------------------------------------------------------------------------------------------------------------------
# the element stage
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("d", [1, 3, 9])
def test_element_emulation_passes(kernel, d):
    worst = 0.0
    for t in case_table(kernel):
        U, A, V, B, box = element_inputs(t["rows"], t["lo"], t["hi"], d, count=None if d == 1 else 96)
        masks = sb.sobol_std_masks(d)
        rows = emul_element_rows(kernel, U, A, V, B, box, masks)
        assert np.all(np.isfinite(rows))
        c = sb.check_sobol_element(rows, kernel, U, A, V, B, box, masks)
        worst = max(worst, c.ratio)
        assert c.ratio <= 1.0, (kernel, d, c)
    print("element emulation", kernel, d, "worst ratio", worst)


ELEMENT_DEFECTS = {"matern32": ("series_everywhere", "forward_small", "ten_terms", "wrong_anchor"),
                   "matern52": ("series_everywhere", "forward_small", "ten_terms", "wrong_anchor"), "se": ("se_near_in_far",)}


# forward_small fails Matern-3/2 by a thin margin (2.3 with C = 4 inside the bound) and only on the rows of sb.sobol_cases with
# gamma L from 0.05 to 0.3 at moderate scales: NT = 2 amplifies by (2 / x)(3 / x) only, and elsewhere s0 or M_0 hides it.  Shrinking
# or removing those rows loses this defect -- and with it the GPU test's sight of a forward recurrence taken too early.
@pytest.mark.parametrize("kernel", KERNELS)
def test_element_defects_fail(kernel):
    for defect in ELEMENT_DEFECTS[kernel]:
        bad = 0.0
        for t in case_table(kernel):
            r, (lo, hi) = t["rows"], (t["lo"], t["hi"])
            U, A, V, B, box = element_inputs(r, lo, hi, 1)
            c = sb.check_sobol_element(emul_element_rows(kernel, U, A, V, B, box, [1], defect), kernel, U, A, V, B, box, [1])
            bad = max(bad, c.ratio)
        print("element defect", kernel, defect, bad)
        assert bad > 1.0, (kernel, defect, bad)


@pytest.mark.parametrize("defect", ["mask_shift", "chunk_masks"])
def test_subset_defects_fail_the_element_stage(defect):
    t = case_table("matern52")[1]
    U, A, V, B, box = element_inputs(t["rows"], t["lo"], t["hi"], 3, count=40)
    masks = subset_masks(3, 33) if defect == "chunk_masks" else subset_masks(3, 8)
    if defect == "chunk_masks":
        masks[32] = 5                                      # (the first chunk's mask 0 is the empty one)
    good = sb.check_sobol_element(emul_element_rows("matern52", U, A, V, B, box, masks), "matern52", U, A, V, B, box, masks)
    bad = sb.check_sobol_element(emul_element_rows("matern52", U, A, V, B, box, masks, defect), "matern52", U, A, V, B, box, masks)
    assert good.ratio <= 1.0 < bad.ratio, (good, bad)
    if defect == "chunk_masks":
        assert bad.where[1] == 32


def test_a_nonzero_empty_mask_fails():
    t = case_table("se")[0]
    U, A, V, B, box = element_inputs(t["rows"], t["lo"], t["hi"], 2, count=4)
    rows = emul_element_rows("se", U, A, V, B, box, [0, 3])
    assert np.all(rows[:, 0] == 0.0) and sb.check_sobol_element(rows, "se", U, A, V, B, box, [0, 3]).ratio <= 1.0
    rows[2, 0] = 1e-300
    assert sb.check_sobol_element(rows, "se", U, A, V, B, box, [0, 3]).ratio == np.inf


# ----------------------------------------------------------------------------------------------------------------------
# tiles, rows, the reduction, the batches
# ----------------------------------------------------------------------------------------------------------------------
def clustered(n, d, q, seed, lo=0.0, hi=1.0):
    """x in clusters sorted by index (tiles many orders of magnitude apart for short length scales, some centres outside the
    sub-box), weights of mixed sign, length scales from 0.02 to 3"""
    rng = np.random.default_rng(seed)
    cen = np.sort(rng.uniform(-0.05, 1.05, (max(1, -(-n // 24)), d)), axis=0)
    x = cen[np.arange(n) // 24] + 0.01 * rng.standard_normal((n, d))
    w = rng.standard_normal((q, n)) * np.exp(rng.uniform(-3, 3, (q, n)))
    ell = np.exp(rng.uniform(np.log(0.02), np.log(3.0), (q, d)))
    return x, w, ell, np.stack([np.full(d, lo), np.full(d, hi)])


def stage_checks(kernel, x, w, ell, box, pairs, masks, res, last_only=False):
    """the checks of the emulated (or fetched) pass: means, every tile of the last batch, every row against the summed tile
    reference, the last batch's rows against the library's own part"""
    npairs = len(pairs)
    p_last = (npairs - 1) // sb.SOBOL_BATCH * sb.SOBOL_BATCH
    out = dict(means=sb.check_sobol_means(res["means"], res["tab"], w), tile=sb.Check(0.0, ()), rows=sb.Check(0.0, ()),
               reduce=sb.Check(0.0, ()))
    refs = {}
    for r, (k, kp) in enumerate(pairs):
        if (k, kp) not in refs:
            refs[k, kp] = sb.sobol_tile_reference(kernel, x, w, ell, box, res["tab"], k, kp, masks)
        ref, bnd = refs[k, kp]
        if r >= p_last:
            c = sb.check_sobol_tile(res["part"][r - p_last], ref, bnd)
            out["tile"] = sb.combine(out["tile"], sb.Check(c.ratio, (r,) + c.where))
            c = sb.check_sobol_reduce(res["out"][r], res["part"][r - p_last], k == kp)
            out["reduce"] = sb.combine(out["reduce"], sb.Check(c.ratio, (r,) + c.where))
        c = sb.check_sobol_rows(res["out"][r], ref, bnd)
        out["rows"] = sb.combine(out["rows"], sb.Check(c.ratio, (r,) + c.where))
    return out


def batch_problem(kernel, npairs=70, n=70, d=2, q=4, seed=3):
    x, w, ell, box = clustered(n, d, q, seed, *BOXES[seed % 2])
    base = [(k, kp) for k in range(q) for kp in range(k, q)]
    pairs = [base[(3 * i) % len(base)] for i in range(npairs)]
    for i in range(1, npairs, sb.SOBOL_BATCH):             # slot 1 of EVERY batch holds a pair k = k': no batch writes its upper
        pairs[i] = (1, 1)                                  # tiles (a slot keeps what an earlier batch's pair k != k' left there)
    return x, w, ell, box, pairs, sb.sobol_std_masks(d)


@pytest.mark.parametrize("kernel", KERNELS)
def test_pair_emulation_passes_every_stage(kernel):
    for seed, n in ((3, 70), (4, 129)):
        x, w, ell, box, pairs, masks = batch_problem(kernel, npairs=66, n=n, seed=seed)
        res = emul_pairs(kernel, x, w, ell, box, pairs, masks)
        got = stage_checks(kernel, x, w, ell, box, pairs, masks, res)
        print("pair emulation", kernel, n, {k: "%.2e" % v.ratio for k, v in got.items()})
        assert all(c.ratio <= 1.0 for c in got.values()), got
        nt = res["part"].shape[1]
        upper = [res["part"][z, r, c] for z, (k, kp) in enumerate(pairs[64:]) if z == 1 for r in range(nt) for c in range(r + 1, nt)]
        assert upper and all(np.all(np.isnan(t)) for t in upper)      # never written: the fill stays


@pytest.mark.parametrize("defect,stage", [("twice_diag", "tile"), ("ragged_stale", "tile"), ("slot_shift", "tile"),
                                          ("out_offset", "rows"), ("reduce_upper", "reduce")])
def test_launch_defects_fail_their_stage(defect, stage):
    kernel = "matern32"
    x, w, ell, box, pairs, masks = batch_problem(kernel, npairs=70)
    res = emul_pairs(kernel, x, w, ell, box, pairs, masks, defect)
    got = stage_checks(kernel, x, w, ell, box, pairs, masks, res)
    print(defect, {k: "%.2e" % v.ratio for k, v in got.items()})
    assert got[stage].ratio > 1.0, (defect, got)
    assert got["means"].ratio <= 1.0
    if stage == "tile" and defect != "slot_shift":         # (there the emulated reduction adds a slot nothing wrote)
        assert got["reduce"].ratio <= 1.0                  # the reduction adds what it is given: its stage stays clean
    if stage == "reduce":
        assert got["tile"].ratio <= 1.0


def test_a_far_element_off_by_1e_9_fails_its_tile_and_passes_the_whole_sum_bar():
    kernel = "se"
    x, w, ell, box, pairs, masks = batch_problem(kernel, npairs=3, n=129, seed=4)
    good = emul_pairs(kernel, x, w, ell, box, pairs, masks)
    bad = emul_pairs(kernel, x, w, ell, box, pairs, masks, "far_element")
    k, kp = pairs[0]
    assert bad["part"][0, 2, 0, 0] != good["part"][0, 2, 0, 0]
    _, _, size = sobol_ref.pair_sums(kernel, x, w[k], ell[k], w[kp], ell[kp], box)
    want = sobol_ref.pair_sums(kernel, x, w[k], ell[k], w[kp], ell[kp], box)[0]
    assert np.all(np.abs(bad["out"][0] - want) <= 1e-12 * size)        # the bar of tests/test_gpu_sobol.py
    got = stage_checks(kernel, x, w, ell, box, pairs, masks, bad)
    assert got["tile"].ratio > 1.0 and got["tile"].where[:3] == (0, 2, 0), got
    assert stage_checks(kernel, x, w, ell, box, pairs, masks, good)["tile"].ratio <= 1.0


def test_means_check():
    x, w, ell, box = clustered(513, 3, 2, 9)
    res = emul_pairs("matern52", x[:70], w[:, :70], ell, box, [(0, 1)], [1])
    assert sb.check_sobol_means(res["means"], res["tab"], w[:, :70]).ratio <= 1.0
    bad = res["means"].copy()
    bad[1] -= w[1, 69] * np.prod(res["tab"][1, :, 69])                 # the last term of a part-full trip left out
    assert sb.check_sobol_means(bad, res["tab"], w[:, :70]).ratio > 1.0


# ----------------------------------------------------------------------------------------------------------------------
# the layouts against the library
# ----------------------------------------------------------------------------------------------------------------------
def test_layouts_against_the_scratch_bytes_entries():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    nb = C.c_size_t(0)
    for n, d, q, npairs in [(1, 1, 1, 1), (64, 16, 64, 65), (65, 17, 3, 6), (70, 2, 12, 130), (1025, 1, 2, 2), (150, 3, 3, 6)]:
        assert lib.lcgp_sobol_scratch_bytes(n, d, q, npairs, C.byref(nb)) == 0
        assert nb.value == sb.sobol_layout(n, d, q, npairs)["total"], (n, d, q, npairs)
        assert lib.lcgp_sobol_matrix_scratch_bytes(n, d, q, min(npairs, q), C.byref(nb)) == 0
        assert nb.value == sb.sobol_layout(n, d, q, min(npairs, q), extra=1)["total"], (n, d, q, npairs)
        if d <= 16:
            assert lib.lcgp_sobol_subset_scratch_bytes(n, d, q, npairs, 33, C.byref(nb)) == 0
            assert nb.value == sb.sobol_subset_layout(n, d, q, npairs)["total"], (n, d, q, npairs)
            assert lib.lcgp_sobol_subset_chunk(d) == sb.SOBOL_CHUNK
        else:
            assert lib.lcgp_sobol_subset_scratch_bytes(n, d, q, npairs, 33, C.byref(nb)) < 0
            assert b"[1, 16]" in lib.lcgp_last_error()


# ----------------------------------------------------------------------------------------------------------------------
# the matrix-weighted pass and the view
# ----------------------------------------------------------------------------------------------------------------------
def _spd(n, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, n)) / np.sqrt(n)
    return B @ B.T + 0.1 * np.eye(n)


def _mat_checks(kernel, x, v, ell, box, masks, res, Q, k=0):
    ref, bnd = sb.sobol_tile_reference(kernel, x, v, ell, box, res["tab"], k, k, masks, Q=Q)
    return dict(tile=sb.check_sobol_tile(res["part"][0], ref, bnd), rows=sb.check_sobol_rows(res["out"][0], ref, bnd),
                reduce=sb.check_sobol_reduce(res["out"][0], res["part"][0], True))


@pytest.mark.parametrize("kernel", KERNELS)
def test_matrix_weighted_emulation_and_the_missing_mirror(kernel):
    n, d = 129, 2
    x, v, ell, box = clustered(n, d, 1, 11, *BOXES[1])
    Q = _spd(n, 12)
    masks = sb.sobol_std_masks(d)
    good = emul_pairs(kernel, x, v, ell, box, [(0, 0)], masks, Q=[Q])
    got = _mat_checks(kernel, x, v, ell, box, masks, good, Q)
    assert all(c.ratio <= 1.0 for c in got.values()), got
    # weights on two rows of one diagonal tile: the tile sum holds Q[3, 40] through the mirrored write alone
    v2 = np.zeros_like(v)
    v2[0, [3, 40]] = (1.5, -0.7)
    assert _mat_checks(kernel, x, v2, ell, box, masks, emul_pairs(kernel, x, v2, ell, box, [(0, 0)], masks, Q=[Q]), Q)["tile"].ratio <= 1.0
    bad = _mat_checks(kernel, x, v2, ell, box, masks, emul_pairs(kernel, x, v2, ell, box, [(0, 0)], masks, "no_mirror", Q=[Q]), Q)
    assert bad["tile"].ratio > 1.0 and bad["tile"].where[:2] == (0, 0) and bad["reduce"].ratio <= 1.0, bad


def _view_parts(n, m, seed):
    """G (mpad, npad), the dense L_S^-1 (mpad, mpad; lower), D, A^-1 (n, n) of an emulated view, and P, E as the library forms
    them"""
    rng = np.random.default_rng(seed)
    npad, mpad, Npad = sb._pad128(n), sb._pad128(m), -(-(n + m) // TS) * TS
    G = np.zeros((mpad, npad))
    G[:m, :n] = rng.standard_normal((m, n)) / np.sqrt(n)
    Wd = np.zeros((mpad, mpad))
    Wd[:m, :m] = np.tril(rng.standard_normal((m, m))) + 2.0 * np.eye(m)
    D = 3.7
    P = np.zeros((Npad, mpad))
    P[:n, :m] = D * G[:m, :n].T
    P[n:n + m, :m] = Wd[:m, :m].T
    E = np.zeros((Npad, Npad))
    E[:] = P @ P.T
    for r in range(Npad // TS):
        E[r * TS:(r + 1) * TS, (r + 1) * TS:] = 0.0        # the lower tiles only
    return G, Wd, D, _spd(n, seed + 1), P, E


def test_view_stages_and_their_defects():
    kernel, n, m, d = "matern32", 100, 40, 2
    G, Wd, D, Ainv, P, E = _view_parts(n, m, 21)
    assert sb.check_sobol_p(P, G, Wd, D, n, m).ratio <= 1.0
    rng = np.random.default_rng(24)
    Un = np.zeros((Wd.shape[0], sb._pad128(n)))
    Un[:m, :n] = rng.standard_normal((m, n))
    T = -(Wd @ Un)
    assert sb.check_sobol_t(T, Wd, Un, m).ratio <= 1.0
    Tb = T + Wd[:, 32:m] @ Un[32:m]                        # a K-stage left out
    assert sb.check_sobol_t(Tb, Wd, Un, m).ratio > 1.0
    assert sb.check_sobol_t(-T, Wd, Un, m).ratio > 1.0     # the sign of "0 - L_S^-1 U_n"
    assert sb.check_sobol_e(E, P, m).ratio <= 1.0
    Pt = P.copy()
    Pt[n:n + m, :m] = Wd[:m, :m]                           # L_S^-1 transposed
    assert sb.check_sobol_p(Pt, G, Wd, D, n, m).ratio > 1.0
    Pz = P.copy()
    Pz[n + m:, 0] = 1e-300                                 # a padding row that is not zero
    assert sb.check_sobol_p(Pz, G, Wd, D, n, m).ratio > 1.0
    Eb = E.copy()
    Eb[TS:2 * TS, :TS] -= P[TS:2 * TS, 32:m] @ P[:TS, 32:m].T      # a K-stage left out of a strictly lower tile
    assert sb.check_sobol_e(Eb, P, m).ratio > 1.0
    N = n + m
    x, v, ell, box = clustered(N, d, 1, 22, *BOXES[0])
    masks = sb.sobol_std_masks(d)
    Qp = sb.sobol_view_q(E, Ainv, D, n, N)
    good = emul_pairs(kernel, x, v, ell, box, [(0, 0)], masks, Q=[Qp])
    got = _mat_checks(kernel, x, v, ell, box, masks, good, Qp)
    assert all(c.ratio <= 1.0 for c in got.values()), got
    Abig = _spd(N, 23)
    Abig[:n, :n] = Ainv
    Qbad = sb.sobol_view_q(E, Abig, D, N, N)               # D A^-1 added beyond nt (nt = 100 cuts the diagonal tile 1)
    bad = _mat_checks(kernel, x, v, ell, box, masks, emul_pairs(kernel, x, v, ell, box, [(0, 0)], masks, Q=[Qbad]), Qp)
    assert bad["tile"].ratio > 1.0 and bad["tile"].where[0] >= 1, bad


def test_view_layout_against_the_scratch_bytes_entries():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    nb = C.c_size_t(0)
    for n, d, q, m in [(100, 2, 2, 40), (150, 3, 2, 70), (128, 2, 2, 64), (100, 2, 3, 1), (70, 16, 2, 150)]:
        assert lib.lcgp_condition_sobol_scratch_bytes(n, d, q, m, 1, C.byref(nb)) == 0
        assert nb.value == sb.cond_sobol_layout(n, d, q, m)["total"], (n, d, q, m)
        assert lib.lcgp_condition_sobol_subset_scratch_bytes(n, d, q, m, 1, 33, C.byref(nb)) == 0
        assert nb.value == sb.cond_sobol_layout(n, d, q, m, subset=True)["total"], (n, d, q, m)
    assert lib.lcgp_condition_sobol_subset_scratch_bytes(100, 17, 2, 40, 1, 3, C.byref(nb)) < 0
