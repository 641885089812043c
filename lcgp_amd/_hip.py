"""ctypes binding of liblcgp_hip.so (the C ABI declared in include/lcgp_hip.h).

The library is built in-tree by `make` / `__graft_entry__.build()`.  There is NO CPU fallback: if the
shared object is missing or no GPU is visible, every hot-path call raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
# (LCGP_HIP_LIB: tools only -- the variant builds of tools/ab_builds.sh / trace_variants.sh; tests and the package use the in-tree library)
LIB_PATH = os.environ.get("LCGP_HIP_LIB") or os.path.join(_HERE, "liblcgp_hip.so")
SRC_PATH = os.path.join(_HERE, "csrc", "lcgp_hip.hip")
HDR_PATH = os.path.join(_ROOT, "include", "lcgp_hip.h")
SCHED_PATH = os.path.join(_HERE, "csrc", "fill_sched.h")
SUBSET_PATH = os.path.join(_HERE, "csrc", "sobol_subset.h")

F64, F32 = 0, 1
# include/lcgp_hip.h: LCGP_KERNEL_MATERN32 (the reference's) / LCGP_KERNEL_SE / LCGP_KERNEL_MATERN52 (extensions, parity unpinned)
KERNELS = {"matern32": 0, "se": 1, "matern52": 2}


class Sched(C.Structure):
    """lcgp_sched of include/lcgp_hip.h: launch shapes of the factorisation / inverse, passed per call."""
    _fields_ = [("outer_blocks", C.c_int), ("syrk_small_tiles", C.c_int), ("trtri_small_tiles", C.c_int),
                ("lauum_small_tiles", C.c_int), ("trtri_level_small", C.c_int), ("fill_leaf", C.c_int),
                ("fill_step", C.c_int), ("leaf_in_wide", C.c_int), ("progressive_tiles", C.c_int), ("progressive_far", C.c_int), ("progressive_lauum", C.c_int), ("pair_tiles", C.c_int)]


# every symbol include/lcgp_hip.h declares: name -> (restype, argtypes)
_vp, _i, _d = C.c_void_p, C.c_int, C.c_double
_sp = C.POINTER(Sched)
SIGNATURES = {
    "lcgp_version": (_i, []),
    "lcgp_source_hash": (C.c_char_p, []),
    "lcgp_last_error": (C.c_char_p, []),
    "lcgp_theta_width": (_i, [_i, _i]),
    "lcgp_out_width": (_i, [_i, _i]),
    "lcgp_partial_width": (_i, [_i, _i, _i]),
    "lcgp_sched_default": (_i, [_sp]),
    "lcgp_workspace_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_predict_scratch_bytes": (_i, [_i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_matern32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, C.POINTER(_d), _d, _d, _i, _vp]),
    "lcgp_covmat": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, C.POINTER(_d), _d, _d, _i, _vp]),
    "lcgp_kernel_build": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "lcgp_potrf_logdet": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sp, _vp]),
    "lcgp_potri": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _sp]),
    "lcgp_trtri": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _sp]),
    "lcgp_lauum": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _sp]),
    "lcgp_lauum_clock": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "lcgp_fetch_matrix": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "lcgp_fetch_vector": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "lcgp_nll_grad": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sp, _vp]),
    "lcgp_nll_hess_width": (_i, [_i, _i]),
    "lcgp_nll_hess_scratch_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_nll_hess": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "lcgp_predict_paramgrad_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_predict_paramgrad": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _i]),
    "lcgp_plan_bytes": (_i, [_i, _i, _i, _i, _sp, C.POINTER(C.c_size_t)]),
    "lcgp_plan_build": (_i, [_i, _i, _i, _i, _sp, _vp, C.c_size_t]),
    "lcgp_plan_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "lcgp_pack_partial": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "lcgp_predict": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i]),
    "lcgp_predict_marginal_scratch_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_predict_marginal": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i]),
    "lcgp_predict_grad_scratch_bytes": (_i, [_i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_predict_grad": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i]),
    "lcgp_predict_hess_scratch_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_predict_hess": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i]),
    "lcgp_predict_gradcov_scratch_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_predict_gradcov": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i]),
    "lcgp_predict_cov_scratch_bytes": (_i, [_i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_predict_cov": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _d]),
    "lcgp_sample_scratch_bytes": (_i, [_i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_sample_latent": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "lcgp_condition_scratch_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_condition_state_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_condition_prepare": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp]),
    "lcgp_condition_predict": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, C.c_size_t, _vp, _vp,
                                    _i]),
    "lcgp_condition_predict_marginal_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_condition_predict_marginal": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp,
                                             C.c_size_t, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "lcgp_condition_grad_state_bytes": (_i, [_i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_condition_grad_prepare": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp]),
    "lcgp_condition_grad_fetch": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "lcgp_condition_predict_grad_scratch_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_condition_predict_grad": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, C.c_size_t,
                                         _vp, _vp, _vp, _vp, _i]),
    "lcgp_condition_predict_hess_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_condition_predict_hess": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, C.c_size_t,
                                         _vp, _vp, _vp, _vp, _vp, _vp, _i]),
    "lcgp_condition_predict_gradcov_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_condition_predict_gradcov": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp,
                                            C.c_size_t, _vp, _vp, _vp, _vp, _i]),
    "lcgp_loo": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i]),
    "lcgp_cv_workspace_bytes": (_i, [_i, _i, _i, _i, _i, _i, _vp, C.POINTER(C.c_size_t)]),
    "lcgp_cv_gather": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "lcgp_cv_apply": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i]),
    "lcgp_variance_reduction_scratch_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_variance_reduction_prepare": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "lcgp_variance_reduction": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _i,
                                     _vp, _vp, _i]),
    "lcgp_variance_reduction_grad_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_variance_reduction_grad": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _i,
                                          _vp]),
    "lcgp_select_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_select_begin": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "lcgp_select_score": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "lcgp_select_picks": (_i, [_i, _i, _i, _i, _i, _i, _i, _vp, C.POINTER(_vp)]),
    "lcgp_select_condition": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "lcgp_select_state": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "lcgp_condition_vr_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_condition_vr_prepare": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, C.c_size_t]),
    "lcgp_condition_vr": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _i,
                               _vp, C.c_size_t, _vp, _i]),
    "lcgp_condition_vr_grad_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_condition_vr_grad": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _i,
                                    _vp, C.c_size_t, _vp, _i, _vp]),
    "lcgp_condition_select_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_condition_select_begin": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp,
                                         _i, _i, _i, _vp, C.c_size_t]),
    "lcgp_condition_select_score": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, C.c_size_t, _vp]),
    "lcgp_condition_select_picks": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _vp, C.c_size_t, C.POINTER(_vp)]),
    "lcgp_condition_select_condition": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, C.c_size_t]),
    "lcgp_condition_select_state": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, C.c_size_t, _vp]),
    "lcgp_condition_predict_cov_scratch_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_condition_predict_cov": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, C.c_size_t,
                                        _vp, _d]),
    "lcgp_calib_rows": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _d, _d, _vp, _vp, _vp, _vp]),
    "lcgp_calib_hess_rows": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _d, _d, _vp, _vp, _vp, _vp, _vp,
                                  _vp]),
    "lcgp_sobol_scratch_bytes": (_i, [_i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_sobol_pairs": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, C.POINTER(_i), _i, _vp, _vp]),
    "lcgp_sobol_matrix_scratch_bytes": (_i, [_i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_sobol_matrix_pairs": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i), _i, _vp, _vp]),
    "lcgp_condition_sobol_scratch_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_condition_sobol_matrix_pairs": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, C.POINTER(_i), _i,
                                               _vp, C.c_size_t, _vp]),
    "lcgp_sobol_subset_chunk": (_i, [_i]),
    "lcgp_sobol_subset_scratch_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_sobol_subset_pairs": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, C.POINTER(_i), _i, C.POINTER(C.c_uint64), _i, _vp, _vp]),
    "lcgp_sobol_matrix_subset_pairs": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i), _i,
                                            C.POINTER(C.c_uint64), _i, _vp, _vp]),
    "lcgp_condition_sobol_subset_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_condition_sobol_matrix_subset_pairs": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp,
                                                      C.POINTER(_i), _i, C.POINTER(C.c_uint64), _i, _vp, C.c_size_t, _vp]),
    "lcgp_box_alc_scratch_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "lcgp_box_alc": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _i]),
}

_lib = None


def source_hash() -> str:
    """sha256 over the sources the library is built from (first 16 hex digits); compiled into the binary as
    LCGP_SRC_HASH and returned by lcgp_source_hash(), so source and binary can be compared on any box."""
    import hashlib
    h = hashlib.sha256()
    for path in (SRC_PATH, HDR_PATH, SCHED_PATH, SUBSET_PATH):
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def binary_hash():
    """LCGP_SRC_HASH of the shared object on disk (read from the file, the library is not loaded), or None."""
    import re
    if not os.path.exists(LIB_PATH):
        return None
    with open(LIB_PATH, "rb") as f:
        m = re.search(rb"LCGP_SRC_HASH=([0-9a-f]{16})", f.read())
    return m.group(1).decode() if m else None


def needs_build() -> bool:
    return binary_hash() != source_hash()


def build_library(force: bool = False, verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 -> lcgp_amd/liblcgp_hip.so (cross-compiles without a GPU).  Rebuilds whenever the
    hash embedded in the binary differs from the hash of the sources (not an mtime test)."""
    if not force and not needs_build():
        return LIB_PATH
    cmd = ["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-shared",
           '-DLCGP_SRC_HASH="LCGP_SRC_HASH=%s"' % source_hash(), "-o", LIB_PATH, SRC_PATH]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(" ".join(cmd))
        print(res.stdout, res.stderr)
    if res.returncode != 0:
        raise RuntimeError("building liblcgp_hip.so failed:\n" + res.stderr)
    return LIB_PATH


def load():
    """Returns the loaded library with argtypes set; raises if it is not there (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "lcgp_amd: %s is missing -- build it with `make` or `python -c 'import __graft_entry__ as g; g.build()'`. "
            "The LCGP hot path has no CPU fallback." % LIB_PATH)
    # torch must own the HIP runtime of the process (same SONAME, loaded first)
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header and library out of sync
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def loaded_hash() -> str:
    """The source hash the LOADED library reports."""
    return load().lcgp_source_hash().decode().split("=")[-1]


def default_sched() -> Sched:
    s = Sched()
    check(load().lcgp_sched_default(C.byref(s)), "lcgp_sched_default")
    return s


def check(rc: int, what: str):
    if rc != 0:
        msg = load().lcgp_last_error().decode("utf-8", "replace")
        raise RuntimeError("%s failed (rc=%d): %s" % (what, rc, msg))


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("lcgp_amd: the LCGP hot path runs on an AMD GPU (gfx950) only; no GPU is visible "
                           "and there is deliberately no CPU fallback.")
