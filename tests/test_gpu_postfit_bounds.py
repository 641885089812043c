"""Stage-wise componentwise bounds of the post-fit queries on the GPU (tests/stage_bounds.py), every run on three fills.

The C entries are called directly on the workspace of an evaluated engine:
  - lcgp_predict_grad: V = U W and U read back from its scratch (lcgp_predict's layout: q slabs of X, n0pad x npad, with V
    written over them, then q slabs of U), ghat / gvar, dghat / dgvar -> pgrad_v, predict, pgrad;
  - lcgp_loo -> loo;
  - lcgp_cv_gather -> the raw matrix slots and the fetched fold matrices M -> lcgp_potrf_logdet on the fold workspace (info and
    half-logdet words) -> L -> lcgp_potri -> L^-1 and M^-1 -> lcgp_cv_apply -> cv_gather (bitwise), cv_factor, cv_inv_factor,
    cv_inverse, cv_apply;
  - lcgp_variance_reduction_prepare, then lcgp_variance_reduction with separate candidates and with candidates taken from the
    reference set (cand_row0 >= 0) -> vr.
Before each run the scratch, the fold workspace, the outputs and the info / half-logdet words are filled with 0x00, 0xFF (NaN
in both precisions) and 0x5A bytes in turn: everything read back must be bitwise identical over the fills, every fold info
word 0, and every check of the 0xFF run must pass.

Coverage.  VR_XBLK = 2048 (the passes of vr_form): n_ref and n_cand of 2049 and 4200, and cand_row0 = 2048 on a 4200-point
reference set; VR_DC = 16 (the dimension chunks of the OP_VR epilogue): d = 15, 16, 17, 32, 33, 126 with n_ref = 2100.
pgrad_kernel: d = 1 .. 126 reaches every for_dim bucket (2, 4, 6, 10, 16) and the wide variant with one to four 32-dimension
chunks; n0 = 31, 32, 33, 64, 65, 129 the PG_ROWS = 32 row blocks.

Run with -s to see the worst ratio per case group, dtype and stage."""
import ctypes as C
from collections import defaultdict

import numpy as np
import pytest
import torch

from lcgp_amd import _hip
from lcgp_amd.engine import HotPathEngine
from tests import stage_bounds as sb
from tests.test_gpu_stage_bounds import FILLS, _bits, _config_problem, _fetch, _filled, _problem

pytestmark = pytest.mark.gpu

WORST = defaultdict(lambda: sb.Check(0.0, ()))       # (group, dtype, stage) -> worst Check over the group's cases


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst ratio |error| / bound per case group, dtype and stage of the post-fit queries (<= 1 passes)")
    for key in sorted(WORST):
        c = WORST[key]
        print("  %-14s %-8s %-13s %.3e  at %s" % (key + (c.ratio, c.where)))


def _record(group, dtype, stage, c, where_extra=None):
    key = (group, dtype, stage)
    if c.ratio >= WORST[key].ratio:
        WORST[key] = sb.Check(c.ratio, (where_extra,) + tuple(c.where) if where_extra is not None else c.where)
    assert c.ratio <= 1.0, (group, dtype, stage, c, where_extra)


def _bytes(fn, *args):
    nbytes = C.c_size_t(0)
    _hip.check(fn(*args, C.byref(nbytes)), "bytes")
    return int(nbytes.value)


def _three(run, *args):
    """run(fill, *args) on the three fills; asserts bitwise equality and returns the 0xFF run (one other run held at a time)"""
    base = run(0xFF, *args)
    for f in FILLS:
        if f == 0xFF:
            continue
        other = run(f, *args)
        assert other.keys() == base.keys()
        for key in base:
            assert torch.equal(_bits(other[key]), _bits(base[key])), ("fill 0x%02X changes" % f, key)
        del other
    return base


def _dev(eng, a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a)).to(eng.device, eng.tdtype if dtype is None else dtype).contiguous()


def _engine(seed, n, d, q, dtype, kernel="matern32", rep=False, **prob):
    x, Y, sr, th = _problem(seed, n, d, 3, q, rep=rep, **prob)
    eng = HotPathEngine(x, Y, sr=sr, q_local=q, dtype=dtype, kernel=kernel)
    out = eng.evaluate(th)
    assert np.all(out[:, 2] == 0), out[:, 2]
    return eng, x, sr, th


def _x0(seed, n0, d, x=None, ntrain=0):
    """n0 new inputs around the unit box; the first ntrain of them training inputs (dx = 0 in the gradient)"""
    x0 = np.random.default_rng(seed).uniform(-0.1, 1.1, (n0, d))
    if ntrain:
        x0[:ntrain] = x[:ntrain]
    return x0


# ---- predict_grad ------------------------------------------------------------------------------------------------------
def _run_pgrad(fill, eng, x0, ldo):
    q, n0, d, n = eng.q_local, x0.shape[0], eng.d, eng.n
    n0pad, npad = sb.predict_pad(n0), sb._pad128(n)
    lib, dev = eng.lib, eng.device
    with torch.cuda.device(dev):
        scratch = _filled((_bytes(lib.lcgp_predict_grad_scratch_bytes, eng.dtype, n, q, n0),), torch.uint8, fill, dev)
        g = _filled((2, q, ldo), torch.float64, fill, dev)
        dg = _filled((2, q, ldo, d), torch.float64, fill, dev)
        x0d = _dev(eng, x0)
        _hip.check(lib.lcgp_predict_grad(eng._stream(), eng.dtype, eng.kernel_id, n, d, eng.p, q, eng._p(eng.x), eng._p(eng.sr),
                                         eng._p(eng.theta_dev), eng._p(eng.workspace), n0, eng._p(x0d), eng._p(scratch),
                                         eng._p(g[0]), eng._p(g[1]), eng._p(dg[0]), eng._p(dg[1]), ldo), "lcgp_predict_grad")
        # out_stride > n0: the rest of each output row keeps the fill
        assert torch.all(g[:, :, n0:].contiguous().view(torch.uint8) == fill)
        assert torch.all(dg[:, :, n0:].contiguous().view(torch.uint8) == fill)
        slab = n0pad * npad
        sc = scratch.view(eng.tdtype)
        return dict(V=sc[:q * slab].view(q, n0pad, npad)[:, :n0, :n].clone(),
                    U=sc[q * slab:2 * q * slab].view(q, n0pad, npad)[:, :n0, :n].clone(),
                    g=g[:, :, :n0].clone(), dg=dg[:, :, :n0].clone())


def _pgrad_case(group, eng, x, sr, th, kernel, dtype, x0, comps=None, ldo=None):
    n0 = x0.shape[0]
    r = _three(_run_pgrad, eng, x0, ldo or n0)
    for k in (range(eng.q_local) if comps is None else comps):
        tag = "n=%d d=%d n0=%d k%d" % (eng.n, eng.d, n0, k)
        W, z = _fetch(eng, 1, k, True), _fetch(eng, 1, k, False)
        V = r["V"][k]
        _record(group, dtype, "pgrad_v", sb.check_pgrad_v(V, r["U"][k], W, dtype), tag)
        _record(group, dtype, "predict", sb.check_predict(r["g"][0, k], r["g"][1, k], x0, x, sr, th[k], W, z, kernel, dtype), tag)
        _record(group, dtype, "pgrad", sb.check_pgrad(r["dg"][0, k], r["dg"][1, k], x0, x, sr, th[k], z, V, kernel, dtype), tag)
        del W, V


# ---- leave-one-out and k-fold ----------------------------------------------------------------------------------------------
def _run_loo(fill, eng):
    with torch.cuda.device(eng.device):
        out = _filled((2, eng.q_local, eng.n), torch.float64, fill, eng.device)
        _hip.check(eng.lib.lcgp_loo(eng._stream(), eng.dtype, eng.n, eng.d, eng.p, eng.q_local, eng._p(eng.sr),
                                    eng._p(eng.theta_dev), eng._p(eng.workspace), eng._p(out[0]), eng._p(out[1]), eng.n), "lcgp_loo")
        return dict(loo=out)


def _loo_case(group, eng, sr, th, dtype, comps=None):
    r = _three(_run_loo, eng)
    for k in (range(eng.q_local) if comps is None else comps):
        V, b, z = _fetch(eng, 2, k, True), _fetch(eng, 0, k, False), _fetch(eng, 1, k, False)
        _record(group, dtype, "loo", sb.check_loo(r["loo"][0, k], r["loo"][1, k], V, b, z, sr, th[k], dtype, eng.d),
                "n=%d k%d" % (eng.n, k))
        del V
    return r["loo"]


def _upper_tiles(mpad, device):
    blk = torch.arange(mpad, device=device) // sb.TS
    return blk[:, None] < blk[None, :]


def _run_cv(fill, eng, folds, slots):
    """gather -> factor -> inverse -> apply on a filled fold workspace.  slots: the slots whose fold matrix, factor and
    inverses are fetched; M^-1 of every slot is read from the lower storage of the workspace's V slot (the layout of
    lcgp_workspace_bytes(dtype, mmax, d, p, q_local F): matrix, L^-1 and A^-1 slots of q_local F mpad^2 elements each, from
    offset 0) and checked against the fetched one on `slots`."""
    q, n, d, p = eng.q_local, eng.n, eng.d, eng.p
    F = len(folds)
    ptr = np.r_[0, np.cumsum([len(f) for f in folds])]
    host = np.ascontiguousarray(np.concatenate([ptr, np.concatenate(folds)]).astype(np.int32))
    hp = C.c_void_p(host.ctypes.data)
    mmax = max(len(f) for f in folds)
    mpad, qF = sb._pad128(mmax), q * F
    lib, dev = eng.lib, eng.device
    r = {}
    with torch.cuda.device(dev):
        st = eng._stream()
        cws = _filled((_bytes(lib.lcgp_cv_workspace_bytes, eng.dtype, n, d, p, q, F, hp),), torch.uint8, fill, dev)
        fd = torch.as_tensor(host).to(dev)
        _hip.check(lib.lcgp_cv_gather(st, eng.dtype, n, d, p, q, eng._p(eng.workspace), F, hp, eng._p(fd), eng._p(cws)),
                   "lcgp_cv_gather")
        el = cws.view(eng.tdtype)
        mat = mpad * mpad
        up = _upper_tiles(mpad, dev)

        def fetch(which, s):
            out = torch.empty((mmax, mmax), dtype=eng.tdtype, device=dev)
            _hip.check(lib.lcgp_fetch_matrix(st, eng.dtype, mmax, d, p, qF, eng._p(cws), which, s, eng._p(out)), "fetch")
            return out

        for s in slots:
            sl = el[s * mat:(s + 1) * mat].view(mpad, mpad).clone()
            r["slot", s] = sl.masked_fill(up, 0)                 # the strict upper tiles are never written
            r["M", s] = fetch(0, s)
        hl = _filled((qF,), torch.float64, fill, dev)
        info = _filled((qF,), torch.int32, fill, dev)
        _hip.check(lib.lcgp_potrf_logdet(st, eng.dtype, mmax, d, p, qF, eng._p(cws), eng._p(hl), eng._p(info), None, None),
                   "lcgp_potrf_logdet")
        r["info"], r["half_logdet"] = info.clone(), hl.clone()
        for s in slots:
            r["L", s] = fetch(0, s)
        _hip.check(lib.lcgp_potri(st, eng.dtype, mmax, d, p, qF, eng._p(cws), None), "lcgp_potri")
        for s in slots:
            r["W", s], r["Mi", s] = fetch(1, s), fetch(2, s)
        vs = el[2 * qF * mat:3 * qF * mat].view(qF, mpad, mpad)[:, :mmax, :mmax]
        lo = torch.tril(vs)
        r["Mi_all"] = lo + torch.tril(lo, -1).transpose(1, 2)
        del vs, lo
        out = _filled((2, q, n), torch.float64, fill, dev)
        _hip.check(lib.lcgp_cv_apply(st, eng.dtype, n, d, p, q, eng._p(eng.sr), eng._p(eng.theta_dev), eng._p(eng.workspace), F,
                                     hp, eng._p(fd), eng._p(cws), eng._p(out[0]), eng._p(out[1]), n), "lcgp_cv_apply")
        r["cv"] = out
        del cws, el
    return r


def _partition(n, mmax, seed):
    """a random partition of 0 .. n-1 into sorted folds of at most mmax inputs, the first of exactly min(mmax, n)"""
    perm = np.random.default_rng(seed).permutation(n)
    return [np.sort(perm[i:i + mmax]) for i in range(0, n, mmax)]


def _cv_case(group, eng, sr, th, dtype, folds, check_folds=None, comps=None):
    """every fold's apply (every position), the gather / factor / inverse of the folds `check_folds` (default: all)"""
    q, F = eng.q_local, len(folds)
    mmax = max(len(f) for f in folds)
    comps = list(range(q)) if comps is None else comps
    check_folds = range(F) if check_folds is None else check_folds
    slots = [f * q + k for f in check_folds for k in comps]
    r = _three(_run_cv, eng, folds, slots)
    assert torch.all(r["info"] == 0), (group, dtype, r["info"])
    for k in comps:
        V, b, z = _fetch(eng, 2, k, True), _fetch(eng, 0, k, False), _fetch(eng, 1, k, False)
        for f in check_folds:
            s, tag = f * q + k, "mmax=%d f%d k%d" % (mmax, f, k)
            assert torch.equal(_bits(r["Mi_all"][s]), _bits(r["Mi", s])), ("V slot layout", s)
            _record(group, dtype, "cv_gather", sb.check_cv_gather(r["slot", s], V, folds[f], mmax), tag)
            _record(group, dtype, "cv_factor", sb.check_cholesky_inverse_solve(r["M", s], r["L", s], dtype), tag)
            _record(group, dtype, "cv_inv_factor", sb.check_inverse_factor(r["L", s], r["W", s], dtype), tag)
            _record(group, dtype, "cv_inverse", sb.check_inverse(r["W", s], r["Mi", s], dtype), tag)
        for f in range(F):
            m = len(folds[f])
            _record(group, dtype, "cv_apply", sb.check_cv_apply(r["cv"][0, k], r["cv"][1, k], r["Mi_all"][f * q + k][:m, :m], b, z,
                                                                sr, th[k], folds[f], dtype, eng.d), "mmax=%d f%d k%d" % (mmax, f, k))
        del V
    return r["cv"]


# ---- variance reduction ----------------------------------------------------------------------------------------------------
def _run_vr(fill, eng, xr, w, calls):
    """prepare on x_ref, then every call: ("sep", x_cand, match, r) or ("shared", cand_row0, n_cand, r)"""
    q, n, d, p = eng.q_local, eng.n, eng.d, eng.p
    n_ref = xr.shape[0]
    ncmax = max(c[1].shape[0] if c[0] == "sep" else c[2] for c in calls)
    lib, dev = eng.lib, eng.device
    r = {}
    with torch.cuda.device(dev):
        st = eng._stream()
        scratch = _filled((_bytes(lib.lcgp_variance_reduction_scratch_bytes, eng.dtype, n, q, n_ref, ncmax),), torch.uint8, fill, dev)
        xrd, wd = _dev(eng, xr), _dev(eng, w, torch.float64)
        args = (eng.dtype, eng.kernel_id, n, d, p, q, eng._p(eng.x), eng._p(eng.sr), eng._p(eng.theta_dev), eng._p(eng.workspace))
        _hip.check(lib.lcgp_variance_reduction_prepare(st, *args, n_ref, eng._p(xrd), eng._p(scratch)), "vr_prepare")
        for i, c in enumerate(calls):
            if c[0] == "sep":
                _, xc, match, rr = c
                nc = xc.shape[0]
                xcd = _dev(eng, xc)
                mh = None if match is None else np.ascontiguousarray(match, np.int32)
                md = None if match is None else torch.as_tensor(mh).to(dev)
                out = _filled((q, nc), torch.float64, fill, dev)
                _hip.check(lib.lcgp_variance_reduction(st, *args, n_ref, eng._p(xrd), eng._p(wd), nc, eng._p(xcd),
                                                       C.c_void_p(0) if mh is None else C.c_void_p(mh.ctypes.data),
                                                       C.c_void_p(0) if md is None else eng._p(md), -1, int(rr), eng._p(scratch),
                                                       eng._p(out), nc), "lcgp_variance_reduction")
            else:
                _, row0, nc, rr = c
                out = _filled((q, nc), torch.float64, fill, dev)
                _hip.check(lib.lcgp_variance_reduction(st, *args, n_ref, eng._p(xrd), eng._p(wd), nc, C.c_void_p(0), C.c_void_p(0),
                                                       C.c_void_p(0), int(row0), int(rr), eng._p(scratch), eng._p(out), nc),
                           "lcgp_variance_reduction")
            r["out", i] = out
        del scratch
    return r


def _weights(n_ref, seed):
    w = np.random.default_rng(seed).uniform(0.0, 1.0, n_ref)
    w[::5] = 0.0
    if not w.any():
        w[:] = 1.0
    return w / w.sum()


def _vr_case(group, eng, x, sr, th, kernel, dtype, xr, w, calls, comps=None):
    r = _three(_run_vr, eng, xr, w, calls)
    for k in (range(eng.q_local) if comps is None else comps):
        W = _fetch(eng, 1, k, True)
        for i, c in enumerate(calls):
            if c[0] == "sep":
                _, xc, match, rr = c
                tag = "n_ref=%d n_cand=%d r=%d k%d" % (xr.shape[0], xc.shape[0], rr, k)
            else:
                _, row0, nc, rr = c
                xc, match = xr[row0:row0 + nc], None
                tag = "n_ref=%d row0=%d n_cand=%d k%d" % (xr.shape[0], row0, nc, k)
            _record(group, dtype, "vr", sb.check_vr(r["out", i][k], xr, w, xc, match, rr, x, sr, th[k], W, kernel, dtype), tag)
        del W


def _matched(x, nc, seed, d, nmatch=3):
    """nc candidates, the first nmatch of them replicates of training inputs (match = their index)"""
    rng = np.random.default_rng(seed)
    xc = rng.uniform(-0.1, 1.1, (nc, d))
    match = -np.ones(nc, np.int64)
    m = min(nmatch, nc, x.shape[0])
    idx = rng.choice(x.shape[0], m, replace=False)
    xc[:m], match[:m] = x[idx], idx
    return xc, match


# ----------------------------------------------------------------------------------------------------------------------
TRAIN_N = (1, 2, 63, 64, 65, 127, 128, 129, 257, 1025)


def _group(name, kernel):
    """the Matern-5/2 cases report under a group of their own (Matern-3/2 and SE share the plain one, as before)"""
    return name + "_m52" if kernel == "matern52" else name


def _all_paths(group, eng, x, sr, th, kernel, dtype, seed):
    n, d = eng.n, eng.d
    _pgrad_case(group, eng, x, sr, th, kernel, dtype, _x0(seed, 33, d, x, min(n, 5)))
    _loo_case(group, eng, sr, th, dtype)
    _cv_case(group, eng, sr, th, dtype, _partition(n, max(1, -(-n // 3)), seed))
    xr = _x0(seed + 1, 65, d)
    xc, match = _matched(x, 63, seed + 2, d)
    _vr_case(group, eng, x, sr, th, kernel, dtype, xr, _weights(65, seed), [("sep", xc, match, 3), ("shared", 1, 64, 1)])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_training_set_sizes(dtype):
    """n on every tile / panel edge, q = 2, full path; the rep path (sr != 1) at n = 129 and 1025"""
    for i, n in enumerate(TRAIN_N):
        eng, x, sr, th = _engine(1000 + i, n, 3, 2, dtype)
        _all_paths("train_n", eng, x, sr, th, "matern32", dtype, 1100 + i)
    for n in (129, 1025):
        eng, x, sr, th = _engine(1200 + n, n, 3, 2, dtype, rep=True)
        _all_paths("train_n_rep", eng, x, sr, th, "matern32", dtype, 1300 + n)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_predict_grad_rows(dtype):
    """n0 around the PG_ROWS = 32 row blocks and the 64 / 128 scratch padding, training inputs among x0; one call with
    out_stride > n0"""
    eng, x, sr, th = _engine(1400, 200, 3, 2, dtype)
    for n0 in (1, 31, 32, 33, 64, 65, 129):
        _pgrad_case("pgrad_rows", eng, x, sr, th, "matern32", dtype, _x0(1401 + n0, n0, 3, x, min(n0, 4)))
    _pgrad_case("pgrad_rows", eng, x, sr, th, "matern32", dtype, _x0(1500, 65, 3, x, 4), ldo=100)


PG_DIMS = (1, 2, 3, 4, 5, 6, 7, 10, 11, 16, 17, 32, 33, 64, 65, 126)


@pytest.mark.parametrize("kernel", ["matern32", "se", "matern52"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_predict_grad_dimensions(dtype, kernel):
    """every for_dim bucket (2, 4, 6, 10, 16) on both sides of its edge and the wide variant with 1 .. 4 chunks of 32"""
    for d in PG_DIMS:
        eng, x, sr, th = _engine(1600 + d, 70, d, 2, dtype, kernel=kernel)
        _pgrad_case(_group("pgrad_dims", kernel), eng, x, sr, th, kernel, dtype, _x0(1700 + d, 40, d, x, 3))


CV_MMAX = (1, 63, 64, 65, 127, 128, 129)


@pytest.mark.parametrize("rep", [False, True], ids=["full", "rep"])
@pytest.mark.parametrize("kernel", ["matern32", "se", "matern52"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_loo_and_folds(dtype, kernel, rep):
    """folds of at most mmax inputs for mmax on every tile edge of the fold workspace, and one fold holding the whole set;
    gather / factor / inverse checked on the first, a middle and the last fold, the apply on every fold"""
    n = 300
    eng, x, sr, th = _engine(1800 + rep, n, 3, 2, dtype, kernel=kernel, rep=rep)
    _loo_case(_group("loo_cv", kernel), eng, sr, th, dtype)
    for mm in CV_MMAX + (n,):
        folds = _partition(n, mm, 1900 + mm)
        F = len(folds)
        _cv_case(_group("loo_cv", kernel), eng, sr, th, dtype, folds, sorted({0, F // 2, F - 1}))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_singleton_folds(dtype):
    """n = 1025, q = 3, F = n singleton folds: 3075 slots of the fold workspace (mmax = 1, mpad = 128); the slots of the first,
    a middle and the last fold checked stage by stage, the apply at every position, and the LOO of every position -- which
    is checked against its own closed form"""
    n = 1025
    eng, x, sr, th = _engine(2000, n, 3, 3, dtype)
    _loo_case("singleton", eng, sr, th, dtype)
    folds = [np.array([i]) for i in range(n)]
    _cv_case("singleton", eng, sr, th, dtype, folds, [0, n // 2, n - 1])
    torch.cuda.empty_cache()


VR_PAIRS = ((1, 4200), (63, 2049), (64, 2048), (65, 2047), (2047, 65), (2048, 64), (2049, 63), (4200, 1))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_vr_set_sizes(dtype):
    """n_ref and n_cand at 1, 63, 64, 65, 2047, 2048, 2049, 4200 (the VR_XBLK = 2048 passes of vr_form on either side),
    matched candidates; on the 4200-point reference set also shared candidates from cand_row0 = 2048 on, across the pass
    edge and at the last row, and 4200 separate candidates"""
    eng, x, sr, th = _engine(2100, 300, 3, 2, dtype)
    for i, (nr, nc) in enumerate(VR_PAIRS):
        xr = _x0(2200 + i, nr, 3)
        xc, match = _matched(x, nc, 2300 + i, 3)
        calls = [("sep", xc, match, 3)]
        if nr == 4200:
            calls += [("shared", 2048, 2152, 1), ("shared", 2000, 100, 3), ("shared", 4199, 1, 1)]
        _vr_case("vr_sizes", eng, x, sr, th, "matern32", dtype, xr, _weights(nr, 2400 + i), calls)
    xr = _x0(2500, 4200, 3)
    _vr_case("vr_sizes", eng, x, sr, th, "matern32", dtype, xr, _weights(4200, 2501),
             [("sep", _x0(2502, 4200, 3), None, 1), ("shared", 0, 4200, 3)])


VR_DIMS = (1, 15, 16, 17, 32, 33, 126)


@pytest.mark.parametrize("kernel", ["matern32", "se", "matern52"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_vr_dimensions(dtype, kernel):
    """d on both sides of the VR_DC = 16 dimension chunks of the epilogue; n_ref = 2100 (a second vr_form pass), separate
    matched candidates and shared ones from cand_row0 = 2048"""
    for d in VR_DIMS:
        eng, x, sr, th = _engine(2600 + d, 100, d, 2, dtype, kernel=kernel)
        xr = _x0(2700 + d, 2100, d)
        xc, match = _matched(x, 70, 2800 + d, d)
        _vr_case(_group("vr_dims", kernel), eng, x, sr, th, kernel, dtype, xr, _weights(2100, d),
                 [("sep", xc, match, 3), ("shared", 2048, 52, 1)])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_vr_replicated_path(dtype):
    """sr != 1: candidates that replicate training inputs (the nugget term scale nt sr_i at column i), r = 1 and 3"""
    eng, x, sr, th = _engine(2900, 400, 3, 3, dtype, rep=True)
    xr = _x0(2901, 2100, 3)
    xc, match = _matched(x, 200, 2902, 3, nmatch=40)
    w = _weights(2100, 2903)
    _vr_case("vr_rep", eng, x, sr, th, "matern32", dtype, xr, w,
             [("sep", xc, match, 1), ("sep", xc, match, 3), ("shared", 2048, 52, 3)])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_headline_configuration(dtype):
    """configs[2] (n = 4096, d = 6, q = 8) with its own data, standardisation and parameters, components 0 and 7:
    predict_grad at 2000 new inputs, LOO, predict_cv(10)'s folds, VR of 2000 candidates against 4096 reference points"""
    m, eng, x, Y, th = _config_problem(3, dtype)
    out = eng.evaluate(th)
    assert np.all(out[:, 2] == 0), out[:, 2]
    comps = [0, eng.q_local - 1]
    lo, hi = x.min(axis=0), x.max(axis=0)
    rng = np.random.default_rng(3000)
    x0 = lo + (hi - lo) * rng.uniform(0.0, 1.0, (2000, x.shape[1]))
    x0[:10] = x[:10]
    _pgrad_case("headline", eng, x, None, th, "matern32", dtype, x0, comps)
    _loo_case("headline", eng, None, th, dtype, comps)
    _, ptr, idx = m._cv_labels(10, 0)
    folds = [np.asarray(idx[ptr[f]:ptr[f + 1]]) for f in range(len(ptr) - 1)]
    _cv_case("headline", eng, None, th, dtype, folds, [0, 5, 9], comps)
    torch.cuda.empty_cache()
    xr = lo + (hi - lo) * rng.uniform(0.0, 1.0, (4096, x.shape[1]))
    _vr_case("headline", eng, x, None, th, "matern32", dtype, xr, _weights(4096, 3001), [("sep", x0, None, 1)], comps)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype,kappa", [("float64", 1e10), ("float32", 1e5)])
def test_ill_conditioned(dtype, kappa):
    """kappa(A) ~ 1e10 (float64) / 1e5 (float32): test_gpu_stage_bounds.test_ill_conditioned's parameters; every bound starts
    from the library's own stored stage, so none carries kappa"""
    n = 700
    eng, x, sr, th = _engine(401, n, 2, 2, dtype, D=(kappa / n, kappa / n), ell=(1.0, 1.2), nug=(-7.0, -7.0))
    _pgrad_case("conditioning", eng, x, sr, th, "matern32", dtype, _x0(3100, 65, 2, x, 5))
    _loo_case("conditioning", eng, sr, th, dtype)
    _cv_case("conditioning", eng, sr, th, dtype, _partition(n, 140, 3101), [0, 2, 4])
    xc, match = _matched(x, 65, 3102, 2)
    _vr_case("conditioning", eng, x, sr, th, "matern32", dtype, _x0(3103, 300, 2), _weights(300, 3104), [("sep", xc, match, 3)])
