"""Stage-wise bounds of the Sobol pair and subset passes on the GPU (tests/stage_bounds.py, the Sobol section), every run on three
fills.

lcgp_sobol_pairs and lcgp_sobol_subset_pairs are called directly through _hip with buffers of this test's own: they need no fitted
model, so x, w, ell, the box and the pair list are built to reach what fitted parameters rarely do.  The scratch is read at the
offsets of do_sobol_pairs / do_sobol_subset_pairs (sb.sobol_layout, sb.sobol_subset_layout), its size asserted against the
library's *_scratch_bytes.  Scratch and out are filled with 0x00, 0xFF (NaN) and 0x5A bytes in turn: everything read back is
bitwise identical over the fills, the row of `out` behind the last pair and the upper tiles of `part` of a pair k = k' keep the
fill, and every check of the 0xFF run is at or below 1:
    table    tab[k, l, i] against mpmath (sb.marg_table_ratios), lengthscales 0.02 .. 30, centres inside, on and outside the box
    means    means[k] against the sum from the library's own table; n in {1, 255, 256, 257, 513}
    element  one-hot weights: each row is (M_u - M_0) of ONE element, against mpmath, over the case table sb.sobol_cases (every
             branch class of sobol_J at least 8 times per kernel) through sobol_pair_kernel (d = 1, 3, 8: DD = 8; 9, 16: DD = 16),
             sobol_pair_wide_kernel (d = 17) and sobol_subset_kernel (d = 3, 8, 9, 16; 33 masks at d = 8, one at d = 3; d = 17
             refused)
    tile     every part[pair, r, c, s] against the float64 reference from the library's table; clustered x, weights of mixed
             sign, n in {1, 63, 64, 65, 129}, pairs k = k' and k != k', the three kernels and the subset kernel's last chunk
    rows     every row of out against the summed tile references: 64, 65 and 130 pairs (q_all = 12, n = 70, d = 2), 65 pairs x 33
             masks; a repeated pair is bitwise equal across batches; the slots of part behind the last batch's pairs hold
             bitwise what the batch before wrote
    reduce   out against the sum of the library's own part; n = 1025 (17 x 17 tiles: two trips of the reductions' loops)
A slot's upper tiles keep the fill only where no earlier batch held a pair k != k' in that slot (the scratch is reused), so the
batch cases put their pairs k = k' in the same slots of every batch.

The matrix-weighted entry lcgp_sobol_matrix_pairs (SOBOL_MAT) and the view's lcgp_condition_sobol_matrix_pairs (SOBOL_VIEW) run on
an evaluated engine: tile (with the S0 column), rows and reduce against Q = the fetched A^-1, resp. Q' = E + D A^-1 [i, i' < n] from
the LIBRARY'S E read at cond_sobol_carve's offsets (sb.cond_sobol_layout); weights on two rows i, j only, so that a tile sum
holds one off-diagonal entry Q[i, j] beside Q[i, i] and Q[j, j] (above the diagonal of a diagonal tile it arrives through the
mirrored write of sobol_stage_q alone; the ragged last row; a strictly lower tile), on both boxes; 65 ks; on the view T = -L_S^-1 U_n
and G = T W against their own inputs from the state and the fetched L^-1 (sobol_t, check_pgrad_v), P entry by entry (sobol_p) and
the lower tiles of E = P P^T (sobol_e), with nt inside a diagonal tile (n = 100, m = 40), inside a lower tile's rows (150, 70), on
a tile edge (128, 64), m = 1 and m > n (70, 150).  The subset forms lcgp_sobol_matrix_subset_pairs (n = 129, 150) and
lcgp_condition_sobol_matrix_subset_pairs (100 + 40) run 34 masks through sobol_subset_kernel's MAT and VIEW instances: the last
chunk's tile sums, every row, the reduction; the view's preparation bitwise that of the pair form.

Run with -s for the worst ratio per stage, kernel and path and the worst element error in units of u (M_u + M_0) per branch class
(profiles/stage_bounds_sobol.txt holds that report from an MI355X)."""
import ctypes as C
from collections import defaultdict

import numpy as np
import pytest
import torch

from lcgp_amd import _hip
from tests import stage_bounds as sb
from tests.test_gpu_condition_bounds import _state_views
from tests.test_gpu_marginal_bounds import _engine, _view
from tests.test_gpu_stage_bounds import FILLS, _bits, _fetch, _filled
from tests.test_sobol_bounds_cpu import BOXES, batch_problem, case_table, clustered, element_inputs, subset_masks

pytestmark = pytest.mark.gpu

KERNELS = ("matern32", "se", "matern52")
KID = {"matern32": 0, "se": 1, "matern52": 2}
DEV = "cuda:0"
WORST = defaultdict(lambda: sb.Check(0.0, ()))       # (stage, kernel, path) -> worst Check
CLASS_ERR = defaultdict(float)                        # (kernel, class) -> worst element error in u (M_u + M_0), d = 1


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst ratio |error| / bound per stage, kernel and path of the Sobol passes (<= 1 passes)")
    for key in sorted(WORST):
        print("  %-8s %-9s %-14s %.3e  at %s" % (key + (WORST[key].ratio, WORST[key].where)))
    print("worst error of one element's M_u - M_0 in units of u (M_u + M_0) per kernel and branch class (d = 1, pair kernel)")
    for key in sorted(CLASS_ERR):
        print("  %-9s %-24s %.3e" % (key + (CLASS_ERR[key],)))


def _record(stage, kernel, path, c, extra=None):
    key = (stage, kernel, path)
    if c.ratio >= WORST[key].ratio:
        WORST[key] = sb.Check(c.ratio, ((extra,) + tuple(c.where)) if extra is not None else c.where)
    assert c.ratio <= 1.0, (stage, kernel, path, c, extra)


def _lib():
    return _hip.load()


def _launch(fill, kernel, x, w, ell, box, pairs, masks=None):
    """one pass on freshly filled scratch and out.  masks: None for lcgp_sobol_pairs, else the bit masks of
    lcgp_sobol_subset_pairs.  In the slots of part whose pair is k = k' in EVERY batch the upper tiles must keep the fill.
    Returns tab, means, part (those upper tiles zeroed after the fill check, so that runs compare bitwise), out (npairs, cols)."""
    lib = _lib()
    x, w, ell, box = (np.ascontiguousarray(t, np.float64) for t in (x, w, ell, box))
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    n, d = x.shape
    q, npairs = w.shape[0], len(pairs)
    nbytes = C.c_size_t(0)
    if masks is None:
        lay, ocols = sb.sobol_layout(n, d, q, npairs), 2 * d + 2
        _hip.check(lib.lcgp_sobol_scratch_bytes(n, d, q, npairs, C.byref(nbytes)), "bytes")
    else:
        lay, ocols = sb.sobol_subset_layout(n, d, q, npairs), len(masks)
        _hip.check(lib.lcgp_sobol_subset_scratch_bytes(n, d, q, npairs, len(masks), C.byref(nbytes)), "bytes")
    assert nbytes.value == lay["total"], (nbytes.value, lay)
    nt, nb, cols = lay["ntile"], lay["nb"], lay["cols"]
    p = lambda t: C.c_void_p(t.data_ptr())                 # noqa: E731
    with torch.cuda.device(DEV):
        dev = [torch.as_tensor(a).to(DEV) for a in (x, w, ell, box)]
        scratch = _filled((lay["total"] // 8,), torch.float64, fill, DEV)
        out = _filled((npairs + 1, ocols), torch.float64, fill, DEV)
        st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        pp = pairs.ctypes.data_as(C.POINTER(C.c_int))
        if masks is None:
            _hip.check(lib.lcgp_sobol_pairs(st, KID[kernel], n, d, q, *[p(t) for t in dev], pp, npairs, p(scratch), p(out)),
                       "lcgp_sobol_pairs")
        else:
            mk = (C.c_uint64 * len(masks))(*masks)
            _hip.check(lib.lcgp_sobol_subset_pairs(st, KID[kernel], n, d, q, *[p(t) for t in dev], pp, npairs, mk, len(masks),
                                                   p(scratch), p(out)), "lcgp_sobol_subset_pairs")
        torch.cuda.synchronize()
        keeps = lambda t: bool(torch.all(_bits(t) == fill))            # noqa: E731
        assert keeps(out[npairs]), "out written behind its last row"
        part = scratch[lay["part"]:].view(nb, nt, nt, cols).clone()
        for z in range(nb):                                # every pair that any batch put into slot z
            writers = pairs[z::sb.SOBOL_BATCH]
            if np.all(writers[:, 0] == writers[:, 1]):
                for r in range(nt - 1):
                    assert keeps(part[z, r, r + 1:]), ("an upper tile of a pair k = k' written", z, r)
                    part[z, r, r + 1:] = 0.0
        res = dict(tab=scratch[:q * d * n].view(q, d, n).clone().cpu(), means=scratch[lay["means"]:lay["means"] + q].clone().cpu(),
                   part=part.cpu(), out=out[:npairs].clone().cpu())
    return res


def _three(*args, **kw):
    base = _launch(0xFF, *args, **kw)
    for f in FILLS:
        if f == 0xFF:
            continue
        other = _launch(f, *args, **kw)
        for key in base:
            assert torch.equal(_bits(other[key]), _bits(base[key])), ("fill 0x%02X changes" % f, key)
    return base


def _split_out(res, d, pairs):
    """the pair pass's out: (rows (npairs, 2 d + 1), the last column); the last column is bitwise means[k] for k = k', else 0.0"""
    out = res["out"].numpy()
    for r, (k, kp) in enumerate(pairs):
        want = res["means"][k].item() if k == kp else 0.0
        assert out[r, 2 * d + 1] == want and not (k != kp and np.signbit(out[r, 2 * d + 1])), (r, k, kp)
    return out[:, :2 * d + 1]


# ----------------------------------------------------------------------------------------------------------------------
# stage 1: the table and the means
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_table_and_means(kernel, n):
    rng = np.random.default_rng(n)
    d, q = 2, 2
    for lo, hi in BOXES:
        x = rng.uniform(-0.2, 1.2, (n, d))
        x[:: 7, 0], x[3:: 11, 1] = lo, hi                  # centres on the ends
        w = rng.standard_normal((q, n)) * np.exp(rng.uniform(-2, 2, (q, n)))
        ell = np.array([[0.02, 30.0], [1.0, 0.3]]) * (hi - lo)
        box = np.stack([np.full(d, lo), np.full(d, hi)])
        res = _three(kernel, x, w, ell, box, [(0, 1), (1, 1)])
        _record("means", kernel, "n=%d" % n, sb.check_sobol_means(res["means"], res["tab"], w))
        _split_out(res, d, [(0, 1), (1, 1)])
        tab = res["tab"].numpy()
        for k in range(q):
            for l in range(d):
                r = sb.marg_table_ratios(kernel, tab[k, l], x[:, l], lo, hi, ell[k, l])
                _record("table", kernel, "n=%d" % n, sb.Check(float(r.max()), (k, l, int(r.argmax()) // sb.TS)))


# ----------------------------------------------------------------------------------------------------------------------
# stage 2: every element on its own
# ----------------------------------------------------------------------------------------------------------------------
def _one_hot_problem(U, A, V, B, first, count):
    """cases first .. first + count - 1 (at most 32) as a launch: component 2 e holds centre U[e] (point 2 e) and scales A[e],
    component 2 e + 1 holds V[e] (point 2 e + 1) and B[e]; the pairs (2 e, 2 e + 1), then (2 e, 2 e) for the first four cases
    (an element on the diagonal: u = v, a = b).  Returns x, w, ell, pairs and the rows (U, A, V, B) in the order of the pairs"""
    sel = np.arange(first, min(first + count, len(U)))
    m, d = len(sel), U.shape[1]
    x, ell, w = np.empty((2 * m, d)), np.empty((2 * m, d)), np.eye(2 * m)
    x[0::2], x[1::2], ell[0::2], ell[1::2] = U[sel], V[sel], A[sel], B[sel]
    pairs = [(2 * e, 2 * e + 1) for e in range(m)] + [(2 * e, 2 * e) for e in range(min(m, 4))]
    dg = sel[:min(m, 4)]
    rows = tuple(np.concatenate([a[sel], b[dg]]) for a, b in ((U, U), (A, A), (V, U), (B, A)))
    return x, w, ell, pairs, rows


def _element_run(kernel, d, path, masks, count, collect=False):
    for t in case_table(kernel):
        lo, hi = t["lo"], t["hi"]
        U, A, V, B, box = element_inputs(t["rows"], lo, hi, d, count=count)
        for first in range(0, len(U), 30):
            x, w, ell, pairs, (Ur, Ar, Vr, Br) = _one_hot_problem(U, A, V, B, first, 30)
            assert len(x) <= 64 and len(pairs) <= 64
            res = _three(kernel, x, w, ell, box, pairs, masks=masks if path == "subset" else None)
            rows = res["out"].numpy() if path.startswith("subset") else _split_out(res, d, pairs)
            assert np.all(np.isfinite(rows)), "a non-finite J in the tile"
            detail = [] if collect else None
            c = sb.check_sobol_element(rows, kernel, Ur, Ar, Vr, Br, box, masks, detail)
            _record("element", kernel, "%s d=%d" % (path, d), c, (lo, first))
            if collect:
                cl = sb.sobol_classes(kernel, Ur[:, 0], Ar[:, 0], Vr[:, 0], Br[:, 0], lo, hi)
                for e, _, v in detail:
                    for name, selc in cl.items():
                        if selc[e]:
                            CLASS_ERR[kernel, name] = max(CLASS_ERR[kernel, name], v)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("d", [1, 3, 8, 9, 16, 17])
def test_elements_through_the_pair_kernels(kernel, d):
    """d <= 8: sobol_pair_kernel<DD = 8>, d <= 16: <DD = 16>, d = 17: sobol_pair_wide_kernel; all 2 d + 1 columns.  The whole
    case table at d = 1, 90 elements per box from d = 3 on (three adversarial inputs, the others benign)"""
    _element_run(kernel, d, "pair" if d <= 16 else "wide", sb.sobol_std_masks(d), None if d == 1 else 90, collect=d == 1)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("d,nsub", [(3, 1), (3, 8), (8, 33), (9, 20), (16, 34)])
def test_elements_through_the_subset_kernel(kernel, d, nsub):
    """the empty mask (exactly 0.0), the full one, singletons, complements, random masks; 33 and 34 masks: a second chunk forms
    the integrals again; nsub = 1: a single mask alone"""
    masks = [5] if nsub == 1 else subset_masks(d, nsub)
    _element_run(kernel, d, "subset", masks, 60)


def test_the_subset_entries_refuse_d_17():
    lib = _lib()
    nb = C.c_size_t(0)
    assert lib.lcgp_sobol_subset_scratch_bytes(64, 17, 2, 1, 1, C.byref(nb)) < 0 and b"[1, 16]" in lib.lcgp_last_error()
    # lcgp_sobol_subset_pairs runs sobol_subset_check (d first) before it looks at any pointer or enqueues anything, so the
    # placeholders below are never dereferenced (tests/test_sobol_host.py::test_c_abi_of_the_sobol_entry relies on the same order)
    dummy, pr, mk = C.c_void_p(16), (C.c_int * 2)(0, 1), (C.c_uint64 * 1)(1)
    assert lib.lcgp_sobol_subset_pairs(None, 0, 64, 17, 2, dummy, dummy, dummy, dummy, pr, 1, mk, 1, dummy, dummy) < 0
    assert b"[1, 16]" in lib.lcgp_last_error()


# ----------------------------------------------------------------------------------------------------------------------
# stages 3 and 4: tiles, rows, the reduction, the batches
# ----------------------------------------------------------------------------------------------------------------------
def _stages(kernel, path, x, w, ell, box, pairs, masks, res, d, tiles=None, rows=True):
    """tile / reduce of the last batch's pairs and rows of every pair; tiles: (rows, cols) of tile indices to sample"""
    out = res["out"].numpy() if path.startswith("subset") else _split_out(res, d, pairs)
    part = res["part"].numpy()
    if path.startswith("subset"):                          # the scratch holds the LAST chunk's tile sums
        c0 = (len(masks) - 1) // sb.SOBOL_CHUNK * sb.SOBOL_CHUNK
        pmasks, pout = masks[c0:], out[:, c0:]
        assert np.all(part[..., len(pmasks):] == 0.0)      # (the idle accumulators of a part-full chunk: exactly 0)
        part = part[..., :len(pmasks)]
    else:
        pmasks, pout = masks, out
    last0 = (len(pairs) - 1) // sb.SOBOL_BATCH * sb.SOBOL_BATCH
    refs = {}
    for r, (k, kp) in enumerate(pairs):
        if (k, kp) not in refs:
            kw = {} if tiles is None else dict(rows=tiles[0], cols=tiles[1])
            refs[k, kp] = sb.sobol_tile_reference(kernel, x, w, ell, box, res["tab"], k, kp, masks, **kw)
        ref, bnd = refs[k, kp]
        if r >= last0:
            sel = slice(len(masks) - len(pmasks), None)
            c = sb.check_sobol_tile(part[r - last0], ref[..., sel], bnd[..., sel])
            _record("tile", kernel, path, c, r)
            _record("reduce", kernel, path, sb.check_sobol_reduce(pout[r], part[r - last0], k == kp), r)
        if rows:
            _record("rows", kernel, path, sb.check_sobol_rows(out[r], ref, bnd), r)
    return out


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_tiles_of_the_pair_kernel(kernel, n):
    for seed, (lo, hi) in enumerate(BOXES):
        x, w, ell, box = clustered(n, 2, 3, 20 + seed, lo, hi)
        pairs = [(0, 0), (0, 1), (2, 2), (1, 2)]
        res = _three(kernel, x, w, ell, box, pairs)
        _record("means", kernel, "n=%d" % n, sb.check_sobol_means(res["means"], res["tab"], w))
        _stages(kernel, "pair", x, w, ell, box, pairs, sb.sobol_std_masks(2), res, 2)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("d,n", [(9, 65), (17, 70)])
def test_tiles_of_the_wider_kernels(kernel, d, n):
    x, w, ell, box = clustered(n, d, 2, 30 + d, *BOXES[1])
    ell = ell * 4.0                                        # (products of d factors: keep the far tiles above the floor)
    pairs = [(0, 0), (0, 1)]
    res = _three(kernel, x, w, ell, box, pairs)
    _stages(kernel, "pair16" if d <= 16 else "wide", x, w, ell, box, pairs, sb.sobol_std_masks(d), res, d)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("d,n,nsub", [(2, 129, 4), (3, 65, 33), (9, 70, 6)])
def test_tiles_of_the_subset_kernel(kernel, d, n, nsub):
    x, w, ell, box = clustered(n, d, 3, 40 + d, *BOXES[d % 2])
    pairs = [(1, 1), (0, 2), (2, 0)]
    masks = subset_masks(d, nsub)
    res = _three(kernel, x, w, ell, box, pairs, masks=masks)
    _stages(kernel, "subset", x, w, ell, box, pairs, masks, res, d)


def _batch_case(kernel, npairs):
    """q_all = 12, n = 70, d = 2; pairs repeated to fill; slots 1 and 40 hold a pair k = k' in every batch"""
    x, w, ell, box, _, masks = batch_problem(kernel, npairs=1, q=12, seed=7)
    base = [(k, kp) for k in range(12) for kp in range(k, 12)]
    pairs = [base[(5 * i) % len(base)] for i in range(npairs)]
    for s0 in range(0, npairs, sb.SOBOL_BATCH):
        for z, k in ((1, 3), (40, 7)):
            if s0 + z < npairs:
                pairs[s0 + z] = (k, k)
    pairs[-1] = pairs[0]                                   # a repeated pair in the first and the last batch
    return x, w, ell, box, pairs, masks


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("npairs", [64, 65, 130])
def test_batches_of_pairs(kernel, npairs):
    x, w, ell, box, pairs, masks = _batch_case(kernel, npairs)
    res = _three(kernel, x, w, ell, box, pairs)
    out = _stages(kernel, "pair batches", x, w, ell, box, pairs, masks, res, 2)
    seen = {}
    for r, pr in enumerate(pairs):
        if pr in seen:
            assert np.array_equal(out[r].view(np.int64), out[seen[pr]].view(np.int64)), ("a repeated pair differs", r, seen[pr])
        seen.setdefault(pr, r)
    if npairs == 65:                                       # slots 1 .. 63 hold bitwise what the first batch wrote
        first = _launch(0xFF, kernel, x, w, ell, box, pairs[:64])
        a, b = res["part"][1:], first["part"][1:]
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("kernel", KERNELS)
def test_batches_of_pairs_and_chunks_of_masks(kernel):
    """65 pairs x 33 masks: two batches of two chunks each, rows nsub apart"""
    x, w, ell, box, pairs, _ = _batch_case(kernel, 65)
    masks = subset_masks(2, 33)
    res = _three(kernel, x, w, ell, box, pairs, masks=masks)
    out = _stages(kernel, "subset batches", x, w, ell, box, pairs, masks, res, 2)
    seen = {}
    for r, pr in enumerate(pairs):
        if pr in seen:
            assert np.array_equal(out[r].view(np.int64), out[seen[pr]].view(np.int64)), ("a repeated pair differs", r, seen[pr])
        seen.setdefault(pr, r)
    assert pairs[64] in pairs[:64]
    first = _launch(0xFF, kernel, x, w, ell, box, pairs[:64], masks=masks)      # slots 1 .. 63: the first batch's last chunk
    assert torch.equal(_bits(res["part"][1:]), _bits(first["part"][1:]))
    assert np.all(out[:, [s for s, m in enumerate(masks) if m == 0]] == 0.0)
    same = [s for s, m in enumerate(masks) if m == masks[32]]
    assert len(same) > 1 and all(np.array_equal(out[:, s], out[:, 32]) for s in same)     # a mask's sum does not depend on its place


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("path", ["pair", "subset"])
def test_more_than_256_tiles(kernel, path):
    """n = 1025, d = 1: 17 x 17 tiles, the strided loops of the two reductions run twice.  A dozen tiles sampled for the tile
    stage (corners, diagonal, the ragged last row and column); the reduction over all of them"""
    x, w, ell, box = clustered(1025, 1, 2, 50, *BOXES[0])
    pairs = [(0, 1), (1, 1)]
    masks = sb.sobol_std_masks(1) if path == "pair" else [1, 0, 1]
    res = _three(kernel, x, w, ell, box, pairs, masks=None if path == "pair" else masks)
    _record("means", kernel, "n=1025", sb.check_sobol_means(res["means"], res["tab"], w))
    _stages(kernel, path + " n=1025", x, w, ell, box, pairs, masks, res, 1, tiles=([0, 8, 15, 16], [0, 8, 16]), rows=False)


# ----------------------------------------------------------------------------------------------------------------------
# the matrix-weighted entry and the conditioned view
# ----------------------------------------------------------------------------------------------------------------------
def _launch_matrix(fill, eng, view, x, v, ell, box, ks, masks=None):
    """lcgp_sobol_matrix_pairs (view None) or lcgp_condition_sobol_matrix_pairs on freshly filled scratch and out; with masks their
    subset forms (part: the last chunk's tile sums, out: nks x nsub).  The view's T, G, P, E and the word neg are those of the LAST
    component of ks"""
    lib, kernel_dev = eng.lib, eng.device
    x, v, ell, box = (np.ascontiguousarray(t, np.float64) for t in (x, v, ell, box))
    ks = np.ascontiguousarray(ks, np.int32)
    N, d = x.shape
    q, nks, n = eng.q_local, len(ks), eng.n
    nbytes = C.c_size_t(0)
    nsub = 0 if masks is None else len(masks)
    ocols = nsub if nsub else 2 * d + 2
    if view is None and not nsub:
        lay = sb.sobol_layout(N, d, q, nks, extra=1)
        _hip.check(lib.lcgp_sobol_matrix_scratch_bytes(N, d, q, nks, C.byref(nbytes)), "bytes")
    elif view is None:
        lay = sb.sobol_subset_layout(N, d, q, nks)
        _hip.check(lib.lcgp_sobol_subset_scratch_bytes(N, d, q, nks, nsub, C.byref(nbytes)), "bytes")
    else:
        m = view["m"]
        assert N == n + m
        lay = sb.cond_sobol_layout(n, d, q, m, subset=bool(nsub))
        lay["nb"], lay["cols"] = 1, sb.SOBOL_CHUNK if nsub else 2 * d + 2
        if nsub:
            _hip.check(lib.lcgp_condition_sobol_subset_scratch_bytes(n, d, q, m, nks, nsub, C.byref(nbytes)), "bytes")
        else:
            _hip.check(lib.lcgp_condition_sobol_scratch_bytes(n, d, q, m, nks, C.byref(nbytes)), "bytes")
    assert nbytes.value == lay["total"], (nbytes.value, lay)
    nt, nb, cols = lay["ntile"], lay["nb"], lay["cols"]
    p = eng._p
    with torch.cuda.device(kernel_dev):
        xd, vd, ed, bd = [torch.as_tensor(a).to(kernel_dev) for a in (x, v, ell, box)]
        scratch = _filled((lay["total"] // 8,), torch.float64, fill, kernel_dev)
        out = _filled((nks + 1, ocols), torch.float64, fill, kernel_dev)
        kp = ks.ctypes.data_as(C.POINTER(C.c_int))
        mk = (C.c_uint64 * max(nsub, 1))(*(masks or [0]))
        if view is None and nsub:
            _hip.check(lib.lcgp_sobol_matrix_subset_pairs(eng._stream(), eng.dtype, eng.kernel_id, N, d, eng.p, q, p(xd), p(vd), p(ed),
                                                          p(bd), p(eng.workspace), kp, nks, mk, nsub, p(scratch), p(out)),
                       "lcgp_sobol_matrix_subset_pairs")
        elif nsub:
            _hip.check(lib.lcgp_condition_sobol_matrix_subset_pairs(
                eng._stream(), eng.dtype, eng.kernel_id, n, d, eng.p, q, p(eng.theta_dev), p(eng.workspace), p(view["state"]), m,
                p(xd), p(vd), p(ed), p(bd), kp, nks, mk, nsub, p(scratch), lay["total"], p(out)),
                "lcgp_condition_sobol_matrix_subset_pairs")
        elif view is None:
            _hip.check(lib.lcgp_sobol_matrix_pairs(eng._stream(), eng.dtype, eng.kernel_id, N, d, eng.p, q, p(xd), p(vd), p(ed), p(bd),
                                                   p(eng.workspace), kp, nks, p(scratch), p(out)), "lcgp_sobol_matrix_pairs")
        else:
            _hip.check(lib.lcgp_condition_sobol_matrix_pairs(
                eng._stream(), eng.dtype, eng.kernel_id, n, d, eng.p, q, p(eng.theta_dev), p(eng.workspace), p(view["state"]), m,
                p(xd), p(vd), p(ed), p(bd), kp, nks, p(scratch), lay["total"], p(out)), "lcgp_condition_sobol_matrix_pairs")
        torch.cuda.synchronize()
        keeps = lambda t: bool(torch.all(_bits(t) == fill))            # noqa: E731
        assert keeps(out[nks]), "out written behind its last row"
        part = scratch[lay["part"]:lay["part"] + nb * nt * nt * cols].view(nb, nt, nt, cols).clone()
        for z in range(nb):                                # every pair is k = k': no upper tile is ever written
            for r in range(nt - 1):
                assert keeps(part[z, r, r + 1:]), ("an upper tile written", z, r)
                part[z, r, r + 1:] = 0.0
        res = dict(tab=scratch[lay["tab"]:lay["tab"] + q * d * N].view(q, d, N).clone().cpu(),
                   means=scratch[lay["means"]:lay["means"] + q].clone().cpu(), part=part.cpu(), out=out[:nks].clone().cpu())
        if view is not None:
            Np, npad, mpad = lay["Npad"], lay["npad"], lay["mpad"]
            assert scratch[lay["neg"]].item() == -1.0
            res["T"] = scratch[lay["t"]:lay["t"] + mpad * npad].view(mpad, npad).clone().cpu()
            res["G"] = scratch[lay["g"]:lay["g"] + mpad * npad].view(mpad, npad).clone().cpu()
            res["P"] = scratch[lay["p"]:lay["p"] + Np * mpad].view(Np, mpad).clone().cpu()
            res["E"] = scratch[lay["e"]:lay["e"] + Np * Np].view(Np, Np).clone().cpu()
    return res


def _three_matrix(*args):
    base = _launch_matrix(0xFF, *args)
    for f in FILLS:
        if f != 0xFF:
            other = _launch_matrix(f, *args)
            for key in base:
                assert torch.equal(_bits(other[key]), _bits(base[key])), ("fill 0x%02X changes" % f, key)
    return base


def _matrix_stages(kernel, path, x, v, ell, box, res, Qs, ks, d, masks=None):
    """tile / reduce of the last batch's components, rows of all; Qs[k]: the full matrix of component k.  masks: the subset form
    (no S0 column; part holds the last chunk's tile sums, its idle columns exactly 0)"""
    subset = masks is not None
    masks = masks if subset else sb.sobol_std_masks(d)
    out, part = res["out"].numpy(), res["part"].numpy()
    c0 = (len(masks) - 1) // sb.SOBOL_CHUNK * sb.SOBOL_CHUNK if subset else 0
    if subset:
        assert np.all(part[..., len(masks) - c0:] == 0.0)
        part = part[..., :len(masks) - c0]
    last0 = (len(ks) - 1) // sb.SOBOL_BATCH * sb.SOBOL_BATCH
    refs = {}
    for r, k in enumerate(ks):
        if k not in refs:
            ref, bnd = sb.sobol_tile_reference(kernel, x, v, ell, box, res["tab"], k, k, masks, Q=Qs[k])
            refs[k] = (ref[..., :len(masks)], bnd[..., :len(masks)]) if subset else (ref, bnd)
        ref, bnd = refs[k]
        if r >= last0 and r - last0 < part.shape[0]:
            c = sb.check_sobol_tile(part[r - last0], ref[..., c0:], bnd[..., c0:])
            _record("tile", kernel, path, c, r)
            _record("reduce", kernel, path, sb.check_sobol_reduce(out[r, c0:], part[r - last0], True), r)
        _record("rows", kernel, path, sb.check_sobol_rows(out[r], ref, bnd), r)
    if subset:
        assert np.all(out[:, [s for s, mk in enumerate(masks) if mk == 0]] == 0.0)
    return out


def _sparse_rows(n):
    """pairs of rows that carry all the weight: above the diagonal of a diagonal tile, the last (ragged) row against a row of
    tile 0 (a strictly lower tile), two rows of the ragged diagonal tile"""
    return [(3, 40), (n - 1, 5), (n - 2, n - 1) if n % 64 > 1 else (n - 1, 70)]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [129, 150])
def test_matrix_weighted_tiles(kernel, n):
    d = 2
    eng, x, sr, th = _engine(3000 + n, n, d, "float64", kernel, rep=(n == 150))
    Qs = [_fetch(eng, 2, k, True).cpu().numpy() for k in range(eng.q_local)]
    assert all(np.array_equal(Q, Q.T) for Q in Qs)
    ell = th[:, :d]
    rng = np.random.default_rng(n)
    dense = rng.standard_normal((eng.q_local, n)) * np.exp(rng.uniform(-2, 2, (eng.q_local, n)))
    for lo, hi in BOXES:
        box = np.stack([np.full(d, lo), np.full(d, hi)])
        res = _three_matrix(eng, None, x, dense, ell, box, [1, 0])
        _record("means", kernel, "matrix", sb.check_sobol_means(res["means"], res["tab"], dense))
        _matrix_stages(kernel, "matrix", x, dense, ell, box, res, Qs, [1, 0], d)
        for i, j in _sparse_rows(n):
            v = np.zeros((eng.q_local, n))
            v[:, i], v[:, j] = (1.5, -0.7), (-0.4, 2.0)
            res = _three_matrix(eng, None, x, v, ell, box, [0, 1])
            _matrix_stages(kernel, "matrix 1 entry", x, v, ell, box, res, Qs, [0, 1], d)
    # lcgp_sobol_matrix_subset_pairs (sobol_subset_kernel<MAT>): 34 masks, the last chunk holds two; the weights on rows 3 and 40
    # (the mirrored write) and the dense ones
    masks = subset_masks(d, 34)
    v = np.zeros((eng.q_local, n))
    v[:, 3], v[:, 40] = (1.5, -0.7), (-0.4, 2.0)
    for vv, path in ((v, "matrix subset 1"), (dense, "matrix subset")):
        res = _three_matrix(eng, None, x, vv, ell, box, [1, 0], masks)
        _matrix_stages(kernel, path, x, vv, ell, box, res, Qs, [1, 0], d, masks)


@pytest.mark.parametrize("kernel", KERNELS)
def test_matrix_weighted_65_components(kernel):
    """ks may repeat: 65 of them are two batches; a repeated component is bitwise equal across batches"""
    n, d = 70, 2
    eng, x, sr, th = _engine(3100, n, d, "float64", kernel, rep=False)
    Qs = [_fetch(eng, 2, k, True).cpu().numpy() for k in range(eng.q_local)]
    rng = np.random.default_rng(5)
    v = rng.standard_normal((eng.q_local, n))
    ks = [(i * 7) % 3 % 2 for i in range(65)]
    box = np.stack([np.full(d, 0.3), np.full(d, 0.75)])
    res = _three_matrix(eng, None, x, v, th[:, :d], box, ks)
    out = _matrix_stages(kernel, "matrix 65 ks", x, v, th[:, :d], box, res, Qs, ks, d)
    for r, k in enumerate(ks):
        assert np.array_equal(out[r].view(np.int64), out[ks.index(k)].view(np.int64)), (r, k)


VIEW_CASES = [(k, 100, 40) for k in KERNELS] + [(k, 150, 70) for k in KERNELS] + \
    [("se", 128, 64), ("matern32", 100, 1), ("matern52", 70, 150)]


@pytest.mark.parametrize("kernel,n,m", VIEW_CASES)
def test_view_stages(kernel, n, m):
    """the first two cases on the three kernels, full (n = 100) and rep (n = 150); the others on one kernel each"""
    d = 2
    eng, x, sr, th = _engine(3200 + n + m, n, d, "float64", kernel, rep=(n == 150))
    view, (xn, _, _) = _view(eng, 3300 + m, m, d, rep=(n == 150))
    N = n + m
    xa = np.concatenate([x, xn])
    un, wd, _ = _state_views(eng, view["state"], m)
    rng = np.random.default_rng(n + m)
    v = rng.standard_normal((eng.q_local, N)) * np.exp(rng.uniform(-2, 2, (eng.q_local, N)))
    box = np.stack([np.full(d, 0.3), np.full(d, 0.75)]) if m % 2 else np.stack([np.zeros(d), np.ones(d)])
    path = "view %d+%d" % (n, m)
    for k in range(eng.q_local):
        res = _three_matrix(eng, view, xa, v, th[:, :d], box, [k])
        D = th[k, d + 2]
        P, E = res["P"].numpy(), res["E"].numpy()
        eerr = np.tril(np.abs(E - P @ P.T))
        print("view", kernel, n, m, k, "max |P| training rows %.3e new rows %.3e, max |E| %.3e, entries of E that differ from numpy's "
              "P P^T: %d, largest difference %.3e" % (np.abs(P[:n]).max(), np.abs(P[n:]).max(), np.abs(E).max(),
                                                      int((eerr > 0).sum()), eerr.max()))
        assert np.abs(P[:n]).max() > 0.0 and np.abs(P[n:N]).max() > 0.0 and np.abs(E[N - 1, :N]).max() > 0.0     # nothing vacuous
        _record("p", kernel, path, sb.check_sobol_p(res["P"], res["G"], wd[k].cpu(), D, n, m), k)
        _record("e", kernel, path, sb.check_sobol_e(res["E"], res["P"], m), k)
        Qp = sb.sobol_view_q(res["E"], _fetch(eng, 2, k, True).cpu(), D, n, N)
        _record("means", kernel, path, sb.check_sobol_means(res["means"], res["tab"], v))
        assert np.abs(res["T"].numpy()[:m, :n]).max() > 0.0 and np.abs(res["G"].numpy()[:m, :n]).max() > 0.0
        _record("t", kernel, path, sb.check_sobol_t(res["T"], wd[k].cpu(), un[k].cpu(), m), k)
        _record("g", kernel, path, sb.check_pgrad_v(res["G"], res["T"][:, :n], _fetch(eng, 1, k, True).cpu(), "float64"), k)
        _matrix_stages(kernel, path, xa, v, th[:, :d], box, res, {k: Qp}, [k], d)
        if (n, m) == (100, 40):                            # the subset form: the same preparation, sobol_subset_kernel<VIEW>
            masks = subset_masks(d, 34)
            sub = _three_matrix(eng, view, xa, v, th[:, :d], box, [k], masks)
            for key in ("T", "G", "P", "E", "tab", "means"):
                assert torch.equal(_bits(sub[key]), _bits(res[key])), key
            _matrix_stages(kernel, "view subset", xa, v, th[:, :d], box, sub, {k: Qp}, [k], d, masks)
