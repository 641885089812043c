"""Writes abi_refusals.json: what the C ABI entries that have a twin on a conditioned view answer to a broken argument.

Run it against the library of the commit whose behaviour is to be pinned (the parent of a change to the argument checks):

    LCGP_HIP_LIB=/path/to/that/liblcgp_hip.so python tests/golden/gen_abi_refusals.py

Every case starts from a call whose scalars are valid and whose pointers are the dummy address 16 (never dereferenced: each
case is refused on the host before anything is enqueued), or a small real array where the checks read one on the host, and
breaks what ONE `return bad(...)` statement of lcgp_hip.hip tests; a NULL test of several pointers gets one case per
pointer.  Where a model entry and its view twin make the same tests in a different order (the selection entries and their
scratch pointer), one more case with two things broken pins each entry's own order.  The cases are derived from the source
by hand, site by site: no fuzzing, since a call the library does not refuse would go on to enqueue.  The generator asserts
that every case returns -1 with the expected fragment in lcgp_last_error() and records the whole text.
tests/test_abi_refusals.py replays the table (no device needed).

Encoding of an argument in the JSON: an int; null = NULL; "P" = the dummy pointer; {"i32": [...]} / {"u64": [...]} = a
real host array; {"f": "<repr>"} = a double; "&size" / "&ptr" = the address of a size_t / pointer the entry may write.
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

P, BIG, INT_MAX = "P", 1 << 40, 2 ** 31 - 1
NULL, BYTES, BOTH = "NULL pointer", "bytes is NULL", "both be NULL or both be given"
SMALL = "scratch is smaller than"


def encode(argtype, v):
    """the ctypes object of one encoded argument (its owner is returned too, to keep arrays alive)"""
    import numpy as np
    if isinstance(v, dict) and "f" in v:
        return float(v["f"]), None
    if isinstance(v, dict):
        (kind, vals), = v.items()
        a = np.ascontiguousarray(vals, {"i32": np.int32, "u64": np.uint64}[kind])
        return (C.c_void_p(a.ctypes.data) if argtype is C.c_void_p else a.ctypes.data_as(argtype)), a
    if v == "&size":
        o = C.c_size_t(0)
        return C.byref(o), o
    if v == "&ptr":
        o = C.c_void_p(0)
        return C.byref(o), o
    if v == P:
        return (C.c_void_p(16) if argtype is C.c_void_p else C.cast(C.c_void_p(16), argtype)), None
    return v, None


def call(lib, signatures, entry, args):
    """(return code, lcgp_last_error() text) of entry on the encoded args"""
    argtypes = signatures[entry][1]
    assert len(argtypes) == len(args), (entry, len(argtypes), len(args))
    enc = [encode(t, v) for t, v in zip(argtypes, args)]
    rc = getattr(lib, entry)(*[e[0] for e in enc])
    return rc, lib.lcgp_last_error().decode()


# ---- the argument lists (in the order of include/lcgp_hip.h) with their valid defaults ----
HEAD = [("stream", None), ("dtype", 0), ("kern", 0), ("n", 50), ("d", 2), ("p", 3), ("q", 2), ("x", P), ("sr", None),
        ("theta", P), ("ws", P)]
VIEW = [("state", P), ("m", 4), ("xn", P)]
SC = [("scratch", P)]
SCV = [("scratch", P), ("nsc", BIG)]


def without(spec, *names):
    return [a for a in spec if a[0] not in names]


# check_common with a kernel id, then without (the *_bytes queries and the entries that take no kernel)
COMMON = [(dict(dtype=2), "dtype must be"), (dict(kern=3), "kernel_id must be"), (dict(n=0), "n < 1"), (dict(d=0), "d must be"),
          (dict(d=127), "d must be"), (dict(p=0), "p < 1"), (dict(q=0), "q_local must be"), (dict(q=65536), "q_local must be")]
COMMON_ND = [c for c in COMMON if not set(c[0]) & {"kern", "p"}]
COMMON_N = [c for c in COMMON_ND if "d" not in c[0]]
# the plain dtype / sizes tests of the scratch queries that do not go through check_common
PLAIN = [(dict(dtype=2), "dtype must be"), (dict(n=0), "must be >= 1"), (dict(q=0), "must be >= 1")]
DIM = [(dict(d=0), "d must be"), (dict(d=127), "d must be")]
ROWS = [(dict(n0=2097153), "n0 * d must be")]
VR = [(dict(nr=0), "n_ref must be"), (dict(nc=0), "n_cand must be")]
SEL = VR + [(dict(size=0), "size must be"), (dict(size=7), "size must be")]
M1 = [(dict(m=0), "m < 1")]
MATCH = [(dict(mh={"i32": [-1, 3, 49, -1]}, md=None), BOTH), (dict(mh=None, md=P), BOTH),
         (dict(mh={"i32": [-1, 3, 50, -1, 0, 0]}, md=P), "match must be -1 or"), (dict(mh={"i32": [-2, 0, 0, 0, 0, 0]}, md=P), "match must be -1 or")]
ROW0 = [(dict(row0=-2), "cand_row0 must be -1"), (dict(row0=8, xc=None), "cand_row0 + n_cand"), (dict(xc=None), NULL)]
STEP = [(dict(step=-1), "step must be"), (dict(step=3), "step must be")]
STRIDE = [(dict(stride=3), "out_stride must be")]
JITTER = [(dict(jitter={"f": "-1.0"}), "jitter must be"), (dict(jitter={"f": "nan"}), "jitter must be"),
          (dict(jitter={"f": "inf"}), "jitter must be")]
KS = [(dict(nks=0), "nks < 1"), (dict(ks={"i32": [0, 2]}), "ks must hold"), (dict(ks={"i32": [-1, 0]}), "ks must hold")]
MASKS = [(dict(d=17), "subset pass takes d"), (dict(nsub=0), "nsub < 1"), (dict(masks={"u64": [1, 4]}), "a mask has a bit")]


def nulls(*names, msg=NULL):
    return [({k: None}, msg) for k in names]


def scratch_cases(lib, signatures, sizer, args, what=SMALL):
    """the two cases of a scratch_bytes test: one byte short of what `sizer` returns for args, and 0"""
    o = C.c_size_t(0)
    assert getattr(lib, sizer)(*args, C.byref(o)) == 0, (sizer, args, lib.lcgp_last_error())
    return [(dict(nsc=o.value - 1), what), (dict(nsc=0), what)]


def entries(lib, sig):
    """[(entry, [(name, default)], [(overrides, fragment)])]"""
    def need(sizer, *args, what=SMALL):
        return scratch_cases(lib, sig, sizer, args, what)
    E = []
    vr_tail = [("nr", 10), ("xr", P), ("w", P), ("nc", 4), ("xc", P)]
    # ---- variance reduction ----
    E.append(("lcgp_variance_reduction_scratch_bytes", [("dtype", 0), ("n", 50), ("q", 2), ("nr", 10), ("nc", 4), ("bytes", "&size")],
              COMMON_N + VR + nulls("bytes", msg=BYTES)))
    E.append(("lcgp_condition_vr_scratch_bytes", [("dtype", 0), ("n", 50), ("q", 2), ("m", 4), ("nr", 10), ("nc", 4), ("bytes", "&size")],
              COMMON_N + M1 + VR + nulls("bytes", msg=BYTES)))
    E.append(("lcgp_variance_reduction_prepare", HEAD + [("nr", 10), ("xr", P)] + SC,
              COMMON + VR[:1] + nulls("x", "theta", "ws", "xr", "scratch")))
    E.append(("lcgp_condition_vr_prepare", HEAD + VIEW + [("nr", 10), ("xr", P)] + SCV,
              COMMON + M1 + VR[:1] + nulls("x", "theta", "ws", "state", "xn", "xr", "scratch")
              + need("lcgp_condition_vr_scratch_bytes", 0, 50, 2, 4, 10, 1)))
    vr_args = vr_tail + [("mh", None), ("md", None), ("row0", -1), ("r", 1)]
    vr_cases = (COMMON + VR + [(dict(r=0), "r must be")] + ROW0 + [(dict(row0=0), "x_cand and match must be NULL"),
                (dict(row0=0, xc=None, mh={"i32": [-1, 3, 49, -1]}, md=P), "x_cand and match must be NULL")] + MATCH)
    E.append(("lcgp_variance_reduction", HEAD + vr_args + SC + [("out", P), ("stride", 0)],
              vr_cases + nulls("x", "theta", "ws", "xr", "w", "scratch", "out") + STRIDE))
    E.append(("lcgp_condition_vr", HEAD + VIEW + vr_args + SCV + [("out", P), ("stride", 0)],
              vr_cases + M1 + nulls("x", "theta", "ws", "state", "xn", "xr", "w", "scratch", "out") + STRIDE
              + need("lcgp_condition_vr_scratch_bytes", 0, 50, 2, 4, 10, 4)))
    many = [(dict(nc=65408), "n_cand must be <= 65407")]
    E.append(("lcgp_variance_reduction_grad_scratch_bytes",
              [("dtype", 0), ("n", 50), ("d", 2), ("q", 2), ("nr", 10), ("nc", 4), ("bytes", "&size")],
              COMMON_ND + VR + many + nulls("bytes", msg=BYTES)))
    E.append(("lcgp_condition_vr_grad_scratch_bytes",
              [("dtype", 0), ("n", 50), ("d", 2), ("q", 2), ("m", 4), ("nr", 10), ("nc", 4), ("bytes", "&size")],
              COMMON_ND + M1 + VR + many + nulls("bytes", msg=BYTES)))
    vrg_args = vr_tail + [("row0", -1), ("r", 1)]
    vrg_cases = COMMON + VR + many + [(dict(r=0), "r must be")] + ROW0 + [(dict(row0=0), "x_cand must be NULL")]
    E.append(("lcgp_variance_reduction_grad", HEAD + vrg_args + SC + [("out", P), ("stride", 0), ("dout", P)],
              vrg_cases + nulls("x", "theta", "ws", "xr", "w", "scratch", "out", "dout") + STRIDE))
    E.append(("lcgp_condition_vr_grad", HEAD + VIEW + vrg_args + SCV + [("out", P), ("stride", 0), ("dout", P)],
              vrg_cases + M1 + nulls("x", "theta", "ws", "state", "xn", "xr", "w", "scratch", "out", "dout") + STRIDE
              + need("lcgp_condition_vr_grad_scratch_bytes", 0, 50, 2, 2, 4, 10, 4)))
    # ---- greedy selection ----
    dims = [("dtype", 0), ("n", 50), ("d", 2), ("q", 2)]
    sel = [("nr", 10), ("nc", 6), ("size", 3)]
    need_sel = need("lcgp_condition_select_scratch_bytes", 0, 50, 2, 2, 4, 10, 6, 3)
    for view in (False, True):
        pre = "lcgp_condition_select_" if view else "lcgp_select_"
        mv, m1, sc, sz = ([("m", 4)], M1, SCV, need_sel) if view else ([], [], SC, [])

        def first(**kw):
            """two things broken: a view entry tests its scratch pointer before its own arguments, a model entry behind them"""
            (name, _), = kw.items()
            return [(dict(kw, scratch=None), NULL if view else name + " must be")]
        E.append((pre + "scratch_bytes", dims + mv + sel + [("bytes", "&size")], COMMON_ND + m1 + SEL + nulls("bytes", msg=BYTES)))
        E.append((pre + "begin", HEAD + (VIEW if view else []) + [("nr", 10), ("xr", P), ("w", P), ("nc", 6), ("xc", P), ("mh", None),
                                                                  ("md", None), ("r", 1), ("size", 3), ("rows", 2048)] + sc,
                  COMMON + m1 + SEL + [(dict(r=0), "r must be"), (dict(rows=0), "pass_rows must be"), (dict(rows=2049), "pass_rows must be")]
                  + MATCH + nulls("x", "theta", "ws", "xr", "w", "xc", "scratch") + (nulls("state", "xn") if view else []) + sz + first(r=0)))
        E.append((pre + "score", [("stream", None)] + dims + mv + sel + [("step", 0), ("omega", P)] + sc + [("out", None)],
                  COMMON_ND + m1 + SEL + STEP + nulls("omega", "scratch") + sz + first(step=-1)))
        E.append((pre + "picks", dims + mv + sel + sc + [("picks", "&ptr")], COMMON_ND + m1 + SEL + nulls("scratch", "picks") + sz))
        E.append((pre + "condition", without(HEAD, "x", "sr", "ws") + mv + sel + [("r", 1), ("step", 0), ("pick", P)] + sc,
                  COMMON + m1 + SEL + [(dict(r=0), "r must be")] + STEP + nulls("theta", "pick", "scratch") + sz + first(r=0)))
        E.append((pre + "state", [("stream", None)] + dims + mv + sel + [("which", 0)] + sc + [("out", P)],
                  COMMON_ND + m1 + SEL + [(dict(which=2), "which must be"), (dict(which=-1), "which must be")]
                  + nulls("scratch", "out") + sz + first(which=2)))
    # ---- per-point queries ----
    E.append(("lcgp_predict_scratch_bytes", [("dtype", 0), ("n", 50), ("q", 2), ("n0", 5), ("bytes", "&size")],
              PLAIN + [(dict(n0=0), "must be >= 1")] + nulls("bytes", msg=BYTES)))
    E.append(("lcgp_predict_grad_scratch_bytes", [("dtype", 0), ("n", 50), ("q", 2), ("n0", 5), ("bytes", "&size")],
              PLAIN + [(dict(n0=0), "must be >= 1")] + nulls("bytes", msg=BYTES)))
    E.append(("lcgp_condition_scratch_bytes", [("dtype", 0), ("n", 50), ("q", 2), ("m", 4), ("n0", 5), ("bytes", "&size")],
              PLAIN + M1 + [(dict(n0=-1), "n0 < 0")] + nulls("bytes", msg=BYTES)))
    E.append(("lcgp_condition_predict_grad_scratch_bytes", [("dtype", 0), ("n", 50), ("q", 2), ("m", 4), ("n0", 5), ("bytes", "&size")],
              PLAIN + M1 + [(dict(n0=0), "n0 < 1")] + nulls("bytes", msg=BYTES)))
    n0x0 = [("n0", 5), ("x0", P)]
    N0 = [(dict(n0=0), "n0 < 1")]
    mean = [("ghat", P), ("gvar", P)]
    jac = mean + [("dghat", P), ("dgvar", P)]
    hes = jac + [("d2ghat", P), ("d2gvar", P)]
    gs = [("gs", P)]
    E.append(("lcgp_predict", HEAD + n0x0 + [("same", 0)] + SC + mean + [("stride", 0)],
              COMMON + N0 + nulls("x", "theta", "ws", "x0", "scratch", "ghat", "gvar") + STRIDE))
    E.append(("lcgp_condition_predict", HEAD + VIEW + n0x0 + SCV + mean + [("stride", 0)],
              COMMON + M1 + N0 + nulls("x", "theta", "ws", "state", "xn", "x0", "scratch", "ghat", "gvar") + STRIDE
              + need("lcgp_condition_scratch_bytes", 0, 50, 2, 4, 5)))
    E.append(("lcgp_predict_grad", HEAD + n0x0 + SC + jac + [("stride", 0)],
              COMMON + N0 + nulls("x", "theta", "ws", "x0", "scratch", "ghat", "gvar", "dghat", "dgvar") + STRIDE))
    E.append(("lcgp_condition_predict_grad", HEAD + VIEW + gs + n0x0 + SCV + jac + [("stride", 0)],
              COMMON + M1 + N0 + nulls("x", "theta", "ws", "state", "xn", "gs", "x0", "scratch", "ghat", "gvar", "dghat", "dgvar")
              + STRIDE + need("lcgp_condition_predict_grad_scratch_bytes", 0, 50, 2, 4, 5)))
    for name in ("hess", "gradcov"):
        outs = hes if name == "hess" else [("dghat", P), ("gamma", P), ("w", None), ("M", None)]
        ptrs = [a[0] for a in hes] if name == "hess" else ["dghat"]
        extra = [] if name == "hess" else [(dict(gamma=None), "gamma may only be NULL"), (dict(w=P), "w and M go together"),
                                           (dict(M=P), "w and M go together")]
        E.append(("lcgp_predict_%s_scratch_bytes" % name, [("dtype", 0), ("n", 50), ("d", 2), ("q", 2), ("n0", 5), ("bytes", "&size")],
                  PLAIN + [(dict(n0=0), "must be >= 1")] + DIM + ROWS + nulls("bytes", msg=BYTES)))
        E.append(("lcgp_condition_predict_%s_scratch_bytes" % name,
                  [("dtype", 0), ("n", 50), ("d", 2), ("q", 2), ("m", 4), ("n0", 5), ("bytes", "&size")],
                  PLAIN + DIM + M1 + N0 + ROWS + nulls("bytes", msg=BYTES)))
        E.append(("lcgp_predict_" + name, HEAD + n0x0 + SC + outs + [("stride", 0)],
                  COMMON + N0 + ROWS + nulls("x", "theta", "ws", "x0", "scratch", *ptrs) + extra + STRIDE))
        E.append(("lcgp_condition_predict_" + name, HEAD + VIEW + gs + n0x0 + SCV + outs + [("stride", 0)],
                  COMMON + M1 + N0 + ROWS + nulls("x", "theta", "ws", "state", "xn", "gs", "x0", "scratch", *ptrs) + extra + STRIDE
                  + need("lcgp_condition_predict_%s_scratch_bytes" % name, 0, 50, 2, 2, 4, 5)))
    # ---- joint covariance ----
    E.append(("lcgp_predict_cov_scratch_bytes", [("dtype", 0), ("n", 50), ("q", 2), ("n0", 5), ("bytes", "&size")],
              PLAIN + [(dict(n0=0), "must be >= 1")] + nulls("bytes", msg=BYTES)))
    E.append(("lcgp_condition_predict_cov_scratch_bytes", [("dtype", 0), ("n", 50), ("q", 2), ("m", 4), ("n0", 5), ("bytes", "&size")],
              COMMON_N + M1 + N0 + nulls("bytes", msg=BYTES)))
    E.append(("lcgp_predict_cov", HEAD + n0x0 + [("same", 0)] + SC + [("cws", P), ("jitter", {"f": "0.0"})],
              COMMON + N0 + [(dict(same=-1), "same must be"), (dict(same=47), "same must be")] + JITTER
              + nulls("x", "theta", "ws", "x0", "scratch", "cws")))
    E.append(("lcgp_condition_predict_cov", HEAD + VIEW + n0x0 + SCV + [("cws", P), ("jitter", {"f": "0.0"})],
              COMMON + M1 + N0 + JITTER + nulls("x", "theta", "ws", "state", "xn", "x0", "scratch", "cws")
              + need("lcgp_condition_predict_cov_scratch_bytes", 0, 50, 2, 4, 5)))
    # ---- box-averaged predictions ----
    E.append(("lcgp_predict_marginal_scratch_bytes", [("dtype", 0), ("n", 50), ("d", 2), ("q", 2), ("n0", 5), ("bytes", "&size")],
              DIM + PLAIN + [(dict(n0=0), "must be >= 1")] + nulls("bytes", msg=BYTES)))
    E.append(("lcgp_condition_predict_marginal_scratch_bytes",
              [("dtype", 0), ("n", 50), ("d", 2), ("q", 2), ("m", 4), ("n0", 5), ("bytes", "&size")],
              [(dict(m=-1), "m < 0")] + DIM + PLAIN + [(dict(n0=0), "must be >= 1")] + nulls("bytes", msg=BYTES)
              + [(dict(m=0, **kw), msg) for kw, msg in DIM + PLAIN + [(dict(n0=0), "must be >= 1")] + nulls("bytes", msg=BYTES)]))
    marg = n0x0 + [("mask", P), ("box", P)]
    E.append(("lcgp_predict_marginal", HEAD + marg + SC + mean + [("stride", 0)],
              COMMON + N0 + nulls("x", "theta", "ws", "x0", "mask", "box", "scratch", "ghat", "gvar") + STRIDE))
    refs = [("ref_row", 0), ("ref_out", None), ("ref_in", None), ("ref_x", None), ("ref_mask", None), ("gcov", None)]
    bare = dict(state=None, m=0, xn=None)
    E.append(("lcgp_condition_predict_marginal", HEAD + VIEW + marg + SCV + mean + [("stride", 0)] + refs,
              COMMON + [(dict(m=0), "m must be >= 1 with a state"), (dict(state=None), "m must be >= 1 with a state")] + N0
              + nulls("x", "theta", "ws", "x0", "mask", "box", "scratch", "ghat", "gvar", "xn")
              + [(dict(ref_out=P, ref_row=-1), "ref_row must be"), (dict(ref_out=P, ref_row=5), "ref_row must be"),
                 (dict(ref_in=P, ref_mask=P, gcov=P), "ref_in needs"), (dict(ref_in=P, ref_x=P, gcov=P), "ref_in needs"),
                 (dict(ref_in=P, ref_x=P, ref_mask=P), "ref_in needs")] + STRIDE
              + need("lcgp_condition_predict_marginal_scratch_bytes", 0, 50, 2, 2, 4, 5)
              + [(dict(bare, **kw), msg) for kw, msg in COMMON + N0 + nulls("x", "scratch") + STRIDE
                 + need("lcgp_condition_predict_marginal_scratch_bytes", 0, 50, 2, 2, 0, 5)]))
    # ---- matrix-weighted Sobol sums ----
    sob = [("x", P), ("v", P), ("ell", P), ("box", P), ("ws", P), ("ks", {"i32": [0, 1]}), ("nks", 2)]
    msk = [("masks", {"u64": [1, 2]}), ("nsub", 2)]
    out = [("scratch", P), ("out", P)]
    f64 = [(dict(dtype=1), "float64 workspace"), (dict(dtype=2), "float64 workspace")]
    wide = [(dict(n=4194241), "n must be at most")]
    E.append(("lcgp_sobol_matrix_pairs", HEAD[:7] + sob + out,
              f64 + COMMON[1:] + wide + KS + nulls("x", "v", "ell", "box", "ws", "ks", "scratch", "out")))
    E.append(("lcgp_sobol_matrix_subset_pairs", HEAD[:7] + sob + msk + out,
              f64 + COMMON[1:] + MASKS + wide + KS + nulls("x", "v", "ell", "box", "ws", "ks", "masks", "scratch", "out")))
    csob = [("theta", P), ("ws", P), ("state", P), ("m", 4), ("xa", P), ("v", P), ("ell", P), ("box", P), ("ks", {"i32": [0, 1]}), ("nks", 2)]
    cout = [("scratch", P), ("nsc", BIG), ("out", P)]
    cwide = [(dict(n=INT_MAX), "n + m overflows"), (dict(n=4194240), "n must be at most")]
    cptr = ("theta", "ws", "state", "xa", "v", "ell", "box", "ks", "scratch", "out")
    E.append(("lcgp_condition_sobol_matrix_pairs", HEAD[:7] + csob + cout,
              f64 + COMMON[1:] + M1 + cwide + KS + nulls(*cptr)
              + need("lcgp_condition_sobol_scratch_bytes", 50, 2, 2, 4, 2, what="scratch too small")))
    E.append(("lcgp_condition_sobol_matrix_subset_pairs", HEAD[:7] + csob + msk + cout,
              f64 + COMMON[1:] + MASKS + M1 + cwide + KS + nulls(*cptr, "masks")
              + need("lcgp_condition_sobol_subset_scratch_bytes", 50, 2, 2, 4, 2, 2, what="scratch too small")))
    # (the two scratch queries of the view's Sobol passes: no twin of the same shape, but the view entries test against them)
    csz = [("n", 50), ("d", 2), ("q", 2), ("m", 4), ("nks", 2)]
    cszc = ([(dict(n=0), "n < 1")] + M1 + cwide + DIM + [(dict(q=0), "q_all must be"), (dict(q=65536), "q_all must be"), KS[0]]
            + nulls("bytes", msg=BYTES))
    E.append(("lcgp_condition_sobol_scratch_bytes", csz + [("bytes", "&size")], cszc))
    E.append(("lcgp_condition_sobol_subset_scratch_bytes", csz + [("nsub", 2), ("bytes", "&size")],
              [c for c in cszc if c[0] != dict(d=127)] + MASKS[:2]))
    return E


# bad() sites of these entries that no argument tuple reaches (an earlier test of the same entry already refuses it)
UNREACHED = [
    "sobol_check from lcgp_sobol_matrix_pairs / lcgp_sobol_matrix_subset_pairs and, through cond_sobol_check, their twins on a "
    "view: 'n < 1' (the view: for n + m), 'd must be in [1, 126]', 'q_all must be in [1, 65535]', 'npairs < 1' (check_common "
    "refuses the first three before, npairs is the constant 1)",
    "sobol_subset_check from lcgp_sobol_matrix_subset_pairs: the same sobol_check sites (its own d > 16 and nsub < 1 tests are "
    "in the table)",
    "check_common 'dtype must be' from the four Sobol matrix entries: their own float64 test refuses every other dtype first",
    "lcgp_condition_predict_hess / _gradcov repeated their scratch query's 'dtype must be', 'n, q_local must be' and 'd must be' "
    "tests behind check_common, which refuses all three before",
    "lcgp_condition_predict_marginal: the return code of its own call of lcgp_condition_predict_marginal_scratch_bytes (every test of "
    "that query was made before)",
    "lcgp_condition_predict_marginal 'NULL pointer' for xn needs a state (the case is in the table); without a state xn is not read",
]


def main():
    from lcgp_amd import _hip
    lib = _hip.load()
    rows = []
    for entry, spec, cases in entries(lib, _hip.SIGNATURES):
        names = [a[0] for a in spec]
        for kw, frag in cases:
            assert set(kw) <= set(names), (entry, kw)
            args = [kw.get(k, v) for k, v in spec]
            rc, text = call(lib, _hip.SIGNATURES, entry, args)
            assert rc == -1 and frag in text, (entry, kw, rc, text, frag)
            rows.append([entry, args, rc, text])
    doc = {"comment": "generated by tests/golden/gen_abi_refusals.py; rows = [entry, arguments, return code, lcgp_last_error()]",
           "library_version": lib.lcgp_version(), "library_source_hash": _hip.loaded_hash(), "unreached": UNREACHED, "rows": rows}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "abi_refusals.json")
    with open(path, "w") as f:
        f.write("{\n")
        for k in ("comment", "library_version", "library_source_hash", "unreached"):
            f.write(" %s: %s,\n" % (json.dumps(k), json.dumps(doc[k])))
        f.write(' "rows": [\n' + ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows) + "\n ]\n}\n")
    print("%d cases of %d entries -> %s" % (len(rows), len({r[0] for r in rows}), path))


if __name__ == "__main__":
    main()
