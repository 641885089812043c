"""Device-side state of one rank's share of the hot path: resident inputs, workspace, theta/out blocks.

PyTorch is plumbing here (device memory, the current HIP stream, pinned staging); all arithmetic of the path
runs in liblcgp_hip.so through the C ABI (include/lcgp_hip.h).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _hip

_DT = {"float64": _hip.F64, "f64": _hip.F64, "float32": _hip.F32, "f32": _hip.F32}

# rows of x0 handled per lcgp_predict call: bounds the scratch (2 * q_local * chunk * npad elements) however many
# new inputs a caller passes (the reference has no limit on n0 either)
PREDICT_CHUNK = 2048
# draws per lcgp_sample_latent call (bounds its scratch, 2 * q_local * chunk * n0pad elements)
SAMPLE_CHUNK = 4096


def point_passes(n0, chunk, keep_tiles):
    """The passes of a chunked per-point query over n0 rows, chunk rows at a time, as a list of (lo, rows, fresh): the pass
    hands rows lo .. lo + rows to the library, and fresh is the first of them that no earlier pass produced.  keep_tiles: a
    pass never runs below 128 rows while n0 has them -- the library forms its rows on 128-row tiles from 128 rows on and on
    64-row tiles below, in different summation orders -- so a short last pass is moved back over its predecessor (the same
    values again; fresh > lo then, else fresh == lo).  That makes results bitwise independent of the chunk."""
    passes = []
    for fresh in range(0, n0, chunk):
        lo, rows = fresh, min(chunk, n0 - fresh)
        if keep_tiles and rows < 128 <= n0:
            lo, rows = n0 - 128, 128
        passes.append((lo, rows, fresh))
    return passes


# the chunked per-point queries: the public name in the error text, (entry, scratch query) of the fitted model and of a
# conditioned view, whether a pass keeps 128-row tiles (point_passes; these also pass d to the scratch query and check the
# fitted model's scratch against the free memory), and for the memory refusal what a pass forms and its rows of width n per
# new input
_POINT_QUERIES = {
    'predict': ("predict", ("lcgp_predict", "lcgp_predict_scratch_bytes"),
                ("lcgp_condition_predict", "lcgp_condition_scratch_bytes"), False, "prediction", lambda d: 1),
    # (lcgp_predict_grad_scratch_bytes is lcgp_predict_scratch_bytes)
    'grad': ("predict_grad", ("lcgp_predict_grad", "lcgp_predict_scratch_bytes"),
             ("lcgp_condition_predict_grad", "lcgp_condition_predict_grad_scratch_bytes"), False, "gradient", lambda d: 1),
    'hess': ("predict_hess", ("lcgp_predict_hess", "lcgp_predict_hess_scratch_bytes"),
             ("lcgp_condition_predict_hess", "lcgp_condition_predict_hess_scratch_bytes"), True, "Hessians", lambda d: d + 1),
    'gradcov': ("predict_grad_cov", ("lcgp_predict_gradcov", "lcgp_predict_gradcov_scratch_bytes"),
                ("lcgp_condition_predict_gradcov", "lcgp_condition_predict_gradcov_scratch_bytes"), True,
                "gradient covariances", lambda d: d),
}


# the design queries: the (scratch query, entries ...) of the fitted model and of a conditioned view (the selection: the
# prefix of its family).  A view's entries take the view behind the workspace, m behind q_local in the dims of the scratch
# query and the scratch size behind the scratch (_design_open).
_DESIGN_QUERIES = {
    'vr': (("lcgp_variance_reduction_scratch_bytes", "lcgp_variance_reduction_prepare", "lcgp_variance_reduction"),
           ("lcgp_condition_vr_scratch_bytes", "lcgp_condition_vr_prepare", "lcgp_condition_vr")),
    'vr_grad': (("lcgp_variance_reduction_grad_scratch_bytes", "lcgp_variance_reduction_prepare", "lcgp_variance_reduction_grad"),
                ("lcgp_condition_vr_grad_scratch_bytes", "lcgp_condition_vr_prepare", "lcgp_condition_vr_grad")),
    'select': (("lcgp_select_scratch_bytes", "lcgp_select_"), ("lcgp_condition_select_scratch_bytes", "lcgp_condition_select_")),
}

# the Sobol passes (_sobol_pass): (entry, scratch query) of the 2 d + 1 standard subsets and of a caller's masks, then what the
# memory refusal names ("pair" / "subset" goes in)
_SOBOL_PASSES = {
    'pairs': (("lcgp_sobol_pairs", "lcgp_sobol_scratch_bytes"), ("lcgp_sobol_subset_pairs", "lcgp_sobol_subset_scratch_bytes"),
              "the Sobol %s sums"),
    'matrix': (("lcgp_sobol_matrix_pairs", "lcgp_sobol_matrix_scratch_bytes"),
               ("lcgp_sobol_matrix_subset_pairs", "lcgp_sobol_subset_scratch_bytes"), "the matrix-weighted Sobol %s sums"),
    'view': (("lcgp_condition_sobol_matrix_pairs", "lcgp_condition_sobol_scratch_bytes"),
             ("lcgp_condition_sobol_matrix_subset_pairs", "lcgp_condition_sobol_subset_scratch_bytes"),
             "the matrix-weighted Sobol %s sums of a conditioned view"),
}


def _checked_box(box, what):
    """box (2, d) = [lo; hi] after the check that it has a volume; `what` names the caller in the refusal"""
    if not np.all(box[1] > box[0]):
        raise ValueError("%s: the box needs hi > lo in every dimension" % what)
    return box


def _match_or_none(match):
    """match as contiguous int32, or None when there is none or no candidate replicates a training input"""
    match = None if match is None else np.ascontiguousarray(match, np.int32)
    return match if match is not None and np.any(match >= 0) else None


def _split_sums(res):
    """(sums, s0): all but the last column of a pass over the standard subsets, and the last"""
    return res[:, :-1].copy(), res[:, -1].copy()


class HotPathEngine:
    """Holds x (n,d), Y (p,n), optional sr (n) and the workspace for the local components on one GPU.

    `comp_ids` are the GLOBAL indices of the local components (k -> rank k mod G) and `q_total` the number of
    components over all ranks; they place this rank's gradient slots in the vector the ranks all-reduce
    (`evaluate_partial`).  Defaults: a single rank holding components 0 .. q_local-1."""

    def __init__(self, x, Y, sr=None, q_local=1, dtype="float64", device=None, comp_ids=None, q_total=None, kernel="matern32"):
        import torch
        _hip.require_gpu()
        self.lib = _hip.load()
        self.kernel_id = _hip.KERNELS[kernel]      # covariance kernel of the latent components (the reference: Matern-3/2 only)
        self.torch = torch
        self.dtype_name = "float64" if _DT[dtype] == _hip.F64 else "float32"
        self.dtype = _DT[dtype]
        self.tdtype = torch.float64 if self.dtype == _hip.F64 else torch.float32
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        x = np.ascontiguousarray(x, dtype=np.float64)
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        self.n, self.d = x.shape
        self.p = Y.shape[0]
        assert Y.shape[1] == self.n
        self.q_local = int(q_local)
        comp_ids = list(range(self.q_local)) if comp_ids is None else [int(k) for k in comp_ids]
        assert len(comp_ids) == self.q_local
        self.q_total = int(q_total) if q_total is not None else (max(comp_ids) + 1 if comp_ids else 1)
        assert all(0 <= k < self.q_total for k in comp_ids)
        self._sched_obj = None       # an _hip.Sched to override the launch schedule (tests / tools); None = defaults
        self.use_plan = True         # the launch plan is built once per schedule (lcgp_plan_build) and passed with every call
        # slot -> ((n, q), host block): the evaluation's plans (slots True / False = with_inverse, at self.sched), the latest
        # plan of the joint covariance ('cov') and of the CV folds ('cv') (default schedule)
        self._plans = {}
        with torch.cuda.device(self.device):
            self.x = torch.as_tensor(x).to(self.device, self.tdtype).contiguous()
            self.Y = torch.as_tensor(Y).to(self.device, self.tdtype).contiguous()
            self.sr = None if sr is None else torch.as_tensor(np.ascontiguousarray(sr, np.float64)).to(
                self.device, self.tdtype).contiguous()
            self.workspace_bytes = self._nbytes("lcgp_workspace_bytes", self.dtype, self.n, self.d, self.p, self.q_local)
            # zero-filled, i.e. touched once here: the first evaluation of a fresh engine otherwise pays 30-70 ms of first-touch
            # page mapping for its 3 x q_local matrices inside the optimiser's first step (and the clock words start at zero)
            self.workspace = torch.zeros(self.workspace_bytes, dtype=torch.uint8, device=self.device)
            self.tw = self.lib.lcgp_theta_width(self.d, self.p)
            self.ow = self.lib.lcgp_out_width(self.d, self.p)
            self.pw = self.lib.lcgp_partial_width(self.d, self.p, self.q_total)
            # one upload per evaluation: the theta rows and, behind them, the guard word of the lock-step check
            self._theta_flat = torch.zeros(self.q_local * self.tw + 1, dtype=torch.float64, device=self.device)
            self.theta_dev = self._theta_flat[:self.q_local * self.tw].view(self.q_local, self.tw)
            self.guard_dev = self._theta_flat[self.q_local * self.tw:]
            # two pinned staging rows used alternately: the H2D copy of one evaluation may still be in flight when the
            # host packs the next one (evaluate() itself synchronises, enqueue-style callers do not)
            self._theta_pin = [torch.zeros(self.q_local * self.tw + 1, dtype=torch.float64).pin_memory() for _ in range(2)]
            self._theta_pin_np = [t.numpy() for t in self._theta_pin]      # the same memory, for host-side writes
            self._pin_event = [None, None]
            self._pin_next = 0
            self._nll_ptrs = None
            self._pack_ptrs = None
            self.out_dev = torch.zeros((self.q_local, self.ow), dtype=torch.float64, device=self.device)
            self.comp_dev = torch.as_tensor(np.asarray(comp_ids, np.int32)).to(self.device)
            self.partial_dev = torch.zeros(self.pw, dtype=torch.float64, device=self.device)
            self._scratch = None
            self._cov_ws = None          # (n0, workspace) of the joint covariance (form_cov)
            self._cv_ws = None           # ((mmax, F), workspace) of the fold matrices (cv_block)
            self._cond_ws = None         # (m, workspace) of the conditioning matrices S_k (condition_begin)
            self._sel = None             # state of a running greedy selection (select_begin)
        self._theta_last = None

    # ------------------------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _p(self, t):
        return C.c_void_p(0 if t is None else t.data_ptr())

    def _head(self, Y=False):
        """what the entries that read the fitted model begin with: (stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta,
        workspace); Y: with Y behind x (the entries that differentiate in the parameters)"""
        held = (self.x, self.Y, self.sr, self.theta_dev, self.workspace) if Y else (self.x, self.sr, self.theta_dev, self.workspace)
        return (self._stream(), self.dtype, self.kernel_id, self.n, self.d, self.p, self.q_local) + tuple(self._p(t) for t in held)

    def _upload_x0(self, x0s):
        """(n0, x0s on the device in the engine's dtype) for n0 >= 1 standardised new inputs x0s (n0, d)"""
        x0s = np.ascontiguousarray(x0s, np.float64)
        assert x0s.ndim == 2 and x0s.shape[1] == self.d and x0s.shape[0] >= 1
        return x0s.shape[0], self.torch.as_tensor(x0s).to(self.device, self.tdtype).contiguous()

    @property
    def sched(self):
        return self._sched_obj

    @sched.setter
    def sched(self, s):
        self._sched_obj = s
        self._plans.pop(True, None)  # a plan carries the schedule it was built for (the 'cov' / 'cv' plans: the default one)
        self._plans.pop(False, None)

    def _sched(self):
        return None if self._sched_obj is None else C.byref(self._sched_obj)

    def _nbytes(self, entry, *args):
        """the size one of the library's *_bytes queries (named `entry`) returns for args"""
        nbytes = C.c_size_t(0)
        _hip.check(getattr(self.lib, entry)(*args, C.byref(nbytes)), entry)
        return int(nbytes.value)

    def _build_plan(self, n, q, with_inverse, sched):
        """the launch plan of the factorisation of q matrices of order n as a numpy byte block (lcgp_plan_build): host-only,
        a function of (dtype, n, q, with_inverse, schedule) and nothing else"""
        nbytes = self._nbytes("lcgp_plan_bytes", self.dtype, n, q, int(with_inverse), sched)
        host = np.zeros(nbytes, dtype=np.uint8)
        _hip.check(self.lib.lcgp_plan_build(self.dtype, n, q, int(with_inverse), sched, C.c_void_p(host.ctypes.data), nbytes),
                   "lcgp_plan_build")
        return host

    def _cached_plan(self, slot, n, q, with_inverse=False, sched=None):
        """the plan held in `slot`, rebuilt when (n, q) differ from those it was built for: one plan per slot"""
        held = self._plans.get(slot)
        if held is None or held[0] != (n, q):
            held = self._plans[slot] = ((n, q), self._build_plan(n, q, with_inverse, sched))
        return held[1]

    def plan(self, with_inverse=True):
        """host pointer of the launch plan of the factorisation for the current schedule: planned ONCE (lcgp_plan_build), the
        position-independent block kept in host memory and passed with every evaluation.  NULL with `use_plan = False`:
        the library then plans per call."""
        if not self.use_plan:
            return C.c_void_p(0)
        key = bool(with_inverse)
        return C.c_void_p(self._cached_plan(key, self.n, self.q_local, key, self._sched()).ctypes.data)

    def plan_info(self, with_inverse=True):
        """launches / what the plan leaves behind the factorisation (lcgp_plan_info)"""
        key = bool(with_inverse)
        # (use_plan = False: a temporary plan, what the library would plan per call)
        host = self._cached_plan(key, self.n, self.q_local, key, self._sched()) if self.use_plan else \
            self._build_plan(self.n, self.q_local, key, self._sched())
        v = [C.c_int(0) for _ in range(2)]
        _hip.check(self.lib.lcgp_plan_info(C.c_void_p(host.ctypes.data), *[C.byref(x) for x in v]), "lcgp_plan_info")
        return dict(zip(("launches", "inverse_done"), (x.value for x in v)))

    def upload_theta(self, theta_rows, guard=0.0, stream=None):
        torch = self.torch
        theta_rows = np.asarray(theta_rows, dtype=np.float64).reshape(self.q_local, self.tw)
        i = self._pin_next
        self._pin_next ^= 1
        ev = self._pin_event[i]
        if ev is not None:
            ev.synchronize()                      # the copy that last read this staging buffer has completed
        else:
            ev = self._pin_event[i] = torch.cuda.Event()
        # (the pinned staging rows are written through their numpy views: no torch op per evaluation on the host side)
        pin = self._theta_pin_np[i]
        pin[:-1] = theta_rows.reshape(-1)
        pin[-1] = float(guard)
        if stream is None:
            with torch.cuda.device(self.device):
                self._theta_flat.copy_(self._theta_pin[i], non_blocking=True)
                ev.record(torch.cuda.current_stream(self.device))
        else:                                     # (the caller is inside the device context and holds the current stream)
            self._theta_flat.copy_(self._theta_pin[i], non_blocking=True)
            ev.record(stream)
        self._theta_last = theta_rows.copy()

    def _nll_args(self):
        """the constant pointer arguments of lcgp_nll_grad as ctypes objects, made once (the tensors live as long as the engine)"""
        if self._nll_ptrs is None:
            self._nll_ptrs = tuple(self._p(t) for t in (self.x, self.Y, self.sr, self.theta_dev, self.workspace, self.out_dev))
        return self._nll_ptrs

    def enqueue(self, stream=None):
        """One pass of the hot path over the resident theta block (asynchronous)."""
        if stream is not None:                    # (inside the device context already)
            _hip.check(self.lib.lcgp_nll_grad(C.c_void_p(stream.cuda_stream), self.dtype, self.kernel_id, self.n, self.d, self.p, self.q_local,
                                              *self._nll_args(), self._sched(), self.plan(True)), "lcgp_nll_grad")
            return
        with self.torch.cuda.device(self.device):
            _hip.check(self.lib.lcgp_nll_grad(self._stream(), self.dtype, self.kernel_id, self.n, self.d, self.p, self.q_local,
                                              *self._nll_args(), self._sched(), self.plan(True)),
                       "lcgp_nll_grad")

    def evaluate(self, theta_rows):
        """theta rows (q_local, d+3+p) -> output rows (q_local, d+5+p) on the host (synchronises)."""
        self.upload_theta(theta_rows)
        self.enqueue()
        return self.out_dev.cpu().numpy()

    def evaluate_partial(self, theta_rows, guard=0.0):
        """theta rows -> this rank's share of the reduced vector, LEFT ON THE DEVICE (lcgp_pack_partial): the caller
        all-reduces it in place over the ranks (RCCL) and copies it to the host once.  `guard` travels in its last slot."""
        if self._pack_ptrs is None:
            self._pack_ptrs = tuple(self._p(t) for t in (self.comp_dev, self.theta_dev, self.out_dev, self.guard_dev, self.partial_dev))
        torch = self.torch
        with torch.cuda.device(self.device):      # one device context and one stream lookup per evaluation
            st = torch.cuda.current_stream(self.device)
            self.upload_theta(theta_rows, guard, st)
            self.enqueue(st)
            _hip.check(self.lib.lcgp_pack_partial(C.c_void_p(st.cuda_stream), self.d, self.p, self.q_local, self.q_total,
                                                  *self._pack_ptrs), "lcgp_pack_partial")
        return self.partial_dev

    def is_current(self, theta_rows):
        return self._theta_last is not None and np.array_equal(
            self._theta_last, np.asarray(theta_rows, np.float64).reshape(self.q_local, self.tw))

    # ------------------------------------------------------------------------------------------------
    def _point_check(self, query, state):
        """_view_args(state) after the check that an evaluation stands behind the query (a view: that it is still the view's)"""
        if state is None and self._theta_last is None:
            raise RuntimeError("%s() needs a preceding evaluate() at the current parameters" % _POINT_QUERIES[query][0])
        return self._view_args(state)

    def _point_query(self, query, x0s, state, same=False):
        """What the chunked per-point queries (_POINT_QUERIES) share, for the fitted model (state = None) or the view `state`
        (condition_begin), inside the device context: the checks, the view's grad state where the entry takes one, x0s on the
        device and the engine's scratch grown for one pass.  Returns (n0, passes, run): passes = point_passes(...), and
        run(lo, rows, *outs) calls the entry on rows lo .. lo + rows of x0s with the output pointers outs.  The entries on a
        view take the view behind the workspace and the scratch size behind the scratch; same goes to lcgp_predict only."""
        _, base, on_view, keep_tiles, what, per_input = _POINT_QUERIES[query]
        m, view, _ = self._point_check(query, state)
        assert state is None or not same
        entry, sizer = base if state is None else on_view
        d, q = self.d, self.q_local
        if state is not None and query != 'predict':
            view += (self._p(self._condition_grad_state(state)),)
        n0, x0d = self._upload_x0(x0s)
        chunk = min(n0, max(128, PREDICT_CHUNK // d) if keep_tiles else PREDICT_CHUNK)
        dims = (self.dtype, self.n) + ((d,) if keep_tiles else ()) + (q,) + (() if state is None else (m,)) + (chunk,)
        refusal = None                                  # (the fitted model's predict and predict_grad: PREDICT_CHUNK bounds it)
        if keep_tiles or state is not None:
            refusal = ("the %s%s of %d new inputs per pass" % ("" if state is None else "conditioned ", what, chunk),
                       "%d components of %d x %s, twice" % (q, chunk * per_input(d), "n" if state is None else "(n + m)"),
                       "lower lcgp_amd.engine.PREDICT_CHUNK")
        scratch = self._grow_scratch(self._nbytes(sizer, *dims), refusal)
        scs = (self._p(scratch),) if state is None else (self._p(scratch), scratch.numel())
        head, fn = self._head() + view, getattr(self.lib, entry)

        def run(lo, rows, *outs):
            x0p = C.c_void_p(x0d.data_ptr() + lo * d * x0d.element_size())
            # the nugget term only exists when x0 IS the training set (covmat.py:46-51): then n0 == n and the diagonal of
            # the full cross matrix falls on rows lo .. lo + rows of this pass
            sm = ((1 + lo) if same else 0,) if entry == "lcgp_predict" else ()
            _hip.check(fn(*head, rows, x0p, *sm, *scs, *outs, n0), entry)
        return n0, point_passes(n0, chunk, keep_tiles), run

    def _predict_chunks(self, query, x0s, state, same=False):
        """predict_block, predict_grad_block or predict_hess_block (query = 'predict', 'grad', 'hess'): the list of the (2,
        q_local, n0[, width]) result blocks: the values, the Jacobians of width d, the Hessians of width d (d + 1) / 2.  Every
        pass writes its rows of the result blocks in place (row stride = n0): no per-pass temporaries, no device-to-device
        copies"""
        torch, d = self.torch, self.d
        tails = {'predict': [()], 'grad': [(), (d,)], 'hess': [(), (d,), (d * (d + 1) // 2,)]}[query]
        with torch.cuda.device(self.device):
            n0, passes, run = self._point_query(query, x0s, state, same)
            blocks = [torch.empty((2, self.q_local, n0) + tail, dtype=torch.float64, device=self.device) for tail in tails]
            for lo, rows, _ in passes:
                run(lo, rows, *[C.c_void_p(t[h].data_ptr() + 8 * lo * t.stride(2)) for t in blocks for h in (0, 1)])
            return blocks

    def predict_block(self, x0s, same=False, state=None):
        """(2, q_local, n0) float64 DEVICE tensor [ghat; gvar] for standardised x0s, from the factorisation of the last
        evaluate() (lcgp_predict).  x0 is processed in chunks of PREDICT_CHUNK rows with one engine-owned scratch buffer:
        passes that write their columns of the one result block in place.
          state: a view's state (condition_begin): the prediction of the conditioned model (lcgp_condition_predict:
                 lcgp_predict's launches with same = 0, then the rank-m correction; same must be False).  The base
                 factorisation must still be the one the state was built from."""
        return self._predict_chunks('predict', x0s, state, same)[0]

    def predict_grad_block(self, x0s, state=None):
        """(block, jac) float64 DEVICE tensors for standardised x0s, from the factorisation of the last evaluate():
        block (2, q_local, n0) = [ghat; gvar], bitwise predict_block(x0s, same=False); jac (2, q_local, n0, d) = [dghat; dgvar],
        the derivatives with respect to x0s (lcgp_predict_grad: no nugget term, the gradient of the continuous surface).
        Chunked like predict_block (PREDICT_CHUNK rows per call) and sharing its scratch.
          state: a view's state (condition_begin): block bitwise predict_block(x0s, state=state) and its derivatives
                 (lcgp_condition_predict_grad: the continuous surface also at the view's own new inputs); the scratch is that
                 of predict_block on the view.  The base factorisation must still be the one the state was built from."""
        return tuple(self._predict_chunks('grad', x0s, state))

    def predict_paramgrad_block(self, x0s, same=False, q_group=None):
        """(block, dk, dn) float64 DEVICE tensors for standardised x0s, from the factorisation of the last evaluate() -- which
        is only read (lcgp_predict_paramgrad): block (2, q_local, n0) = [ghat; gvar], bitwise predict_block(x0s, same) while both
        take one pass; dk (2, q_local, n0, d + 2) = [dghat; dgvar], the derivatives in the component's CONSTRAINED kernel
        parameters [ell_0 .. ell_{d-1}, scale, nug]; dn (q_local, n0, p) = d ghat / d built noise parameters (gvar has none).
        float64 engines only.  x0s goes in chunks of PREDICT_CHUNK rows, the local components in groups as large as the free
        device memory allows (q_group: at most that many, for tests; results are bitwise independent of the grouping): the
        scratch holds 2 chunk_pad npad + npad^2 doubles per component processed at once.  Raises ValueError when even one
        component does not fit."""
        torch = self.torch
        if self._theta_last is None:
            raise RuntimeError("predict_param_grad() needs a preceding evaluate() at the current parameters")
        if self.dtype != _hip.F64:
            raise RuntimeError("the parameter derivatives of the prediction are float64 only: evaluate on a float64 engine")
        x0s = np.ascontiguousarray(x0s, np.float64)
        n0, d, m = x0s.shape[0], self.d, self.d + 2
        assert x0s.ndim == 2 and x0s.shape[1] == d and n0 >= 1
        chunk = min(n0, PREDICT_CHUNK)
        with torch.cuda.device(self.device):
            group, nbytes = self._fit_group("lcgp_predict_paramgrad_scratch_bytes", self.dtype, self.n, d, self.p, None, chunk,
                                            q_group=q_group)
            scp = self._p(self._grow_scratch(nbytes, ("the parameter derivatives of %d new inputs per pass" % chunk,
                                                      "one n x n matrix and two of %d x n per component" % chunk,
                                                      "use fewer training inputs per GPU or lower lcgp_amd.engine.PREDICT_CHUNK")))
            x0d = torch.as_tensor(x0s).to(self.device).contiguous()
            out = torch.empty((2, self.q_local, n0), dtype=torch.float64, device=self.device)
            dk = torch.empty((2, self.q_local, n0, m), dtype=torch.float64, device=self.device)
            dn = torch.empty((self.q_local, n0, self.p), dtype=torch.float64, device=self.device)
            head = self._head(Y=True)
            for lo, rows, _ in point_passes(n0, chunk, False):
                for k0 in range(0, self.q_local, group):
                    _hip.check(self.lib.lcgp_predict_paramgrad(
                        *head, k0, min(group, self.q_local - k0), rows,
                        C.c_void_p(x0d.data_ptr() + 8 * lo * d), (1 + lo) if same else 0, scp,
                        C.c_void_p(out[0].data_ptr() + 8 * lo), C.c_void_p(out[1].data_ptr() + 8 * lo),
                        C.c_void_p(dk[0].data_ptr() + 8 * lo * m), C.c_void_p(dk[1].data_ptr() + 8 * lo * m),
                        C.c_void_p(dn.data_ptr() + 8 * lo * self.p), n0), "lcgp_predict_paramgrad")
            return out, dk, dn

    def predict_hess_block(self, x0s, state=None):
        """(block, jac, hess) float64 DEVICE tensors for standardised x0s, from the factorisation of the last evaluate():
        block (2, q_local, n0) and jac (2, q_local, n0, d) bitwise those of predict_grad_block(x0s); hess (2, q_local, n0,
        d (d + 1) / 2) = [d2ghat; d2gvar], the packed lower triangles (entry (l, m <= l) at l (l + 1) / 2 + m) of the Hessians
        with respect to x0s (lcgp_predict_hess).  Chunked so that one call forms at most PREDICT_CHUNK rows of P (chunk * d <=
        PREDICT_CHUNK) but never fewer than 128 new inputs while n0 has them: the library forms V on 128-row tiles from 128 new
        inputs on and on 64-row tiles below, in different summation orders, so a last pass of fewer than 128 inputs is moved
        back to overlap its predecessor (the same values again; point_passes).  All results are therefore bitwise independent
        of PREDICT_CHUNK.  The scratch holds 2 q_local (chunk_pad + (chunk d)_pad) npad elements, chunk = max(128,
        PREDICT_CHUNK // d); raises ValueError when it does not fit in the free device memory.
          state: a view's state (condition_begin): block and jac bitwise those of predict_grad_block(x0s, state=state), hess
                 [d2ghat'; d2gvar'] of the conditioned model (lcgp_condition_predict_hess), chunked the same way.  The scratch
                 holds that of predict_grad_block on the view and q_local (chunk d)_pad (2 npad + 3 mpad) elements.  The base
                 factorisation must still be the one the state was built from."""
        return tuple(self._predict_chunks('hess', x0s, state))

    def grad_cov_block(self, x0s, w=None, per_point=True, state=None):
        """(dghat, gamma, M) float64 DEVICE tensors for standardised x0s, from the factorisation of the last evaluate()
        (lcgp_predict_gradcov): dghat (q_local, n0, d) bitwise that of predict_grad_block(x0s); gamma (q_local, n0, d (d + 1)
        / 2), the packed lower triangles (entry (l, m <= l) at l (l + 1) / 2 + m) of the posterior covariance of the latent
        gradient at each new input, or None with per_point=False (w is then required and the per-point tensor is never
        formed); M (q_local, d (d + 1) / 2) = sum_i w_i gamma[:, i] for n0 weights w, reduced on the device in a fixed order,
        or None without w.  Chunked as predict_hess_block is (at most PREDICT_CHUNK rows of P per pass, never fewer than 128
        new inputs while n0 has them, a short last pass moved back so that P is formed on 128-row tiles in every pass of a
        call with several): dghat and gamma are bitwise independent of PREDICT_CHUNK.  The rows a moved-back pass repeats
        weigh zero in it.  The scratch holds 2 q_local (chunk d)_pad npad elements; raises ValueError when it does not fit in
        the free device memory.
          state: a view's state (condition_begin): dghat bitwise that of predict_grad_block(x0s, state=state), gamma the
                 covariance of the latent gradient given the view's runs too (lcgp_condition_predict_gradcov), chunked and
                 weighted the same way.  The scratch holds q_local (chunk d)_pad (2 npad + 3 mpad) elements.  The base
                 factorisation must still be the one the state was built from."""
        torch, d = self.torch, self.d
        if w is None and not per_point:
            self._point_check('gradcov', state)         # (an engine never evaluated or a stale view is reported first)
            raise ValueError("%sgrad_cov_block: per_point=False needs weights" % ("" if state is None else "condition_"))
        tri = d * (d + 1) // 2
        with torch.cuda.device(self.device):
            n0, passes, run = self._point_query('gradcov', x0s, state)
            dghat = torch.empty((self.q_local, n0, d), dtype=torch.float64, device=self.device)
            gamma = torch.empty((self.q_local, n0, tri), dtype=torch.float64, device=self.device) if per_point else None
            M = wd = None
            if w is not None:
                w = np.ascontiguousarray(w, np.float64).reshape(-1)
                assert w.shape == (n0,)
                wd = torch.as_tensor(w).to(self.device)
                M = torch.zeros((self.q_local, tri), dtype=torch.float64, device=self.device)
            for lo, rows, fresh in passes:
                wl = None if wd is None else wd[lo:lo + rows]
                if wd is not None and fresh > lo:       # the rows lo .. fresh were summed by the pass before
                    wl = wl.clone()
                    wl[:fresh - lo] = 0.0
                run(lo, rows, C.c_void_p(dghat.data_ptr() + 8 * lo * d),
                    None if gamma is None else C.c_void_p(gamma.data_ptr() + 8 * lo * tri), self._p(wl),
                    None if M is None else self._p(M))
            return dghat, gamma, M

    def predict_marginal_block(self, x0s, mask, box, state=None, ref=None):
        """(2, q_local, n0) float64 DEVICE tensor [ghat; gvar] of the latent components AVERAGED over the dimensions mask marks
        (mask (n0, d), non-zero = integrated out), uniformly over box (2, d) = [lo; hi] in standardised inputs, from the
        factorisation of the last evaluate() (lcgp_predict_marginal).  Entries of x0s under the mask are never read on the
        device (they are uploaded as zeros: NaN is allowed there).  A row with an empty mask is bitwise predict_block(x0s,
        same=False)'s while both take one pass.  Chunked like predict_block with the engine's scratch, a pass never below 128
        rows while n0 has them and a short last pass moved back over its predecessor (the same values again), so that every
        pass forms U on the same tile size: results are bitwise independent of PREDICT_CHUNK.
          state: a view's state (condition_begin): the averages of the conditioned model (lcgp_condition_predict_marginal); a
                 row with an empty mask is then bitwise condition_predict_block's while both take one pass.  The base
                 factorisation must still be the one the state was built from.
          ref:   (x_ref_s (d,), mask_ref (d,)), one more row: the result is (3, q_local, n0) with gcov third, the posterior
                 covariance of every row's average with that row's (continuous surface, no nugget term).  A one-row pass
                 writes the reference row's widened row [U_r | T_r] out first; the chunked passes then read it.  The first two
                 rows are bitwise those without ref."""
        torch = self.torch
        if self._theta_last is None:
            raise RuntimeError("predict_marginal() needs a preceding evaluate() at the current parameters")
        n0, d = np.shape(x0s)[0], self.d
        mask = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        box = np.ascontiguousarray(box, np.float64)
        assert np.shape(x0s) == (n0, d) and mask.shape == (n0, d) and box.shape == (2, d) and n0 >= 1
        _checked_box(box, "predict_marginal_block")
        chunk = min(n0, max(128, PREDICT_CHUNK))
        m, view, kp = self._view_args(state)
        with torch.cuda.device(self.device):
            _, x0d = self._upload_x0(np.where(mask != 0, 0.0, np.asarray(x0s, np.float64)))
            md = torch.as_tensor(mask).to(self.device)
            bd = torch.as_tensor(box).to(self.device)
            out = torch.empty((2 if ref is None else 3, self.q_local, n0), dtype=torch.float64, device=self.device)
            base = self._head()
            plain = state is None and ref is None
            if plain:
                scratch = self._grow_scratch(self._nbytes("lcgp_predict_marginal_scratch_bytes", self.dtype, self.n, d,
                                                          self.q_local, chunk))
            else:
                scratch = self._grow_scratch(
                    self._nbytes("lcgp_condition_predict_marginal_scratch_bytes", self.dtype, self.n, d, self.q_local, m, chunk),
                    ("the box-averaged prediction of %d rows per pass" % chunk,
                     "%d components of %d x K', K' = npad + mpad = %d, twice" % (self.q_local, chunk, kp),
                     "lower lcgp_amd.engine.PREDICT_CHUNK"))
            scp = self._p(scratch)
            head = base + (view if view else (None, 0, None))
            refs = (0, None, None, None, None)          # ref_row, ref_out, ref_in, ref_x, ref_mask
            if ref is not None:
                mr = np.ascontiguousarray(np.asarray(ref[1]) != 0, np.uint8).reshape(1, d)
                xr = np.ascontiguousarray(np.where(mr != 0, 0.0, np.asarray(ref[0], np.float64).reshape(1, d)))
                xrd = torch.as_tensor(xr).to(self.device, self.tdtype).contiguous()
                mrd = torch.as_tensor(mr).to(self.device)
                row = torch.empty((self.q_local, kp), dtype=self.tdtype, device=self.device)
                one = torch.empty((2, self.q_local, 1), dtype=torch.float64, device=self.device)
                _hip.check(self.lib.lcgp_condition_predict_marginal(
                    *head, 1, self._p(xrd), self._p(mrd), self._p(bd), scp, scratch.numel(), self._p(one[0]), self._p(one[1]), 1,
                    0, self._p(row), None, None, None, None), "lcgp_condition_predict_marginal")
                refs = (0, None, self._p(row), self._p(xrd), self._p(mrd))
            for lo, rows, _ in point_passes(n0, chunk, True):
                x0p, mp = C.c_void_p(x0d.data_ptr() + lo * d * x0d.element_size()), C.c_void_p(md.data_ptr() + lo * d)
                ghp, gvp = C.c_void_p(out[0].data_ptr() + 8 * lo), C.c_void_p(out[1].data_ptr() + 8 * lo)
                if plain:
                    _hip.check(self.lib.lcgp_predict_marginal(*base, rows, x0p, mp, self._p(bd), scp, ghp, gvp, n0),
                               "lcgp_predict_marginal")
                else:
                    gcp = None if ref is None else C.c_void_p(out[2].data_ptr() + 8 * lo)
                    _hip.check(self.lib.lcgp_condition_predict_marginal(
                        *head, rows, x0p, mp, self._p(bd), scp, scratch.numel(), ghp, gvp, n0, *refs, gcp),
                        "lcgp_condition_predict_marginal")
            return out

    def sobol_pairs(self, x, w, ell, box, pairs):
        """The pair sums behind the closed-form Sobol indices (lcgp_sobol_pairs), always float64: x (n, d) standardised inputs,
        w (q_all, n) the weight vectors of ALL components (scale (1 - nt) sr o z), ell (q_all, d) their length scales, box
        (2, d) = [lo; hi] standardised, pairs (npairs, 2) component indices.  Returns host arrays (D (npairs, 2 d + 1), means
        (npairs,)): row r = D_u of the pair for u = {l} (l = 0 .. d - 1), all but l, all inputs; means[r] = the box mean of
        component k where the pair is (k, k), 0 elsewhere.  Nothing of the factorisation is read; the tile sums go through the
        engine's scratch and are added in a fixed order (two calls agree bit for bit)."""
        return _split_sums(self._sobol_pass("sobol_pairs", 'pairs', x, w, ell, box, pairs)[0])

    def sobol_matrix_sums(self, x, v, ell, box, ks):
        """The pair sums of sobol_pairs for the pairs (k, k) of the LOCAL components ks, weighted by the matrix
        Q[i, i'] = v[k, i] v[k, i'] A_k^-1[i, i'] instead of a product of two vectors (lcgp_sobol_matrix_pairs):
        x (n, d) standardised inputs, v (q_local, n) the row vectors c sr sqrt(D) and ell (q_local, d) the length scales of the
        local components, box (2, d) standardised, ks local component indices.  Returns host arrays (sums (len(ks), 2 d + 1),
        s0 (len(ks),)): sum Q (M_u - M_0) for u = {l}, all but l, all inputs, and S0 = sum Q M_0.  A^-1 is read in place from the
        float64 workspace of the last evaluate(); the tile sums go through the engine's scratch in a fixed order."""
        return _split_sums(self._sobol_pass("sobol_matrix_sums", 'matrix', x, v, ell, box, ks)[0])

    def condition_sobol_matrix_sums(self, state, v, ell, box, ks):
        """sobol_matrix_sums on the view `state` (lcgp_condition_sobol_matrix_pairs): over the N = n + m centres
        [x; xn], weighted by Q'[i, i'] = v[k, i] v[k, i'] (E[i, i'] + D_k A_k^-1[i, i'] where both are training inputs), E the
        rank-m term of the view.  v (q_local, N) holds c sr on the training rows and c on the new ones (D lives inside the
        matrices), ell (q_local, d), box (2, d) standardised, ks local component indices.  Returns host arrays (sums (len(ks),
        2 d + 1), s0 (len(ks),)).  The float64 workspace, the view's state and its grad state are only read; E of one component
        at a time lives in the engine's scratch."""
        return _split_sums(self._sobol_pass("condition_sobol_matrix_sums", 'view', None, v, ell, box, ks, state=state)[0])

    def _sobol_pass(self, caller, kind, x, wv, ell, box, idx, masks=None, state=None):
        """One Sobol pass (_SOBOL_PASSES[kind]) for the public method `caller`: the conversions and checks, the inputs on the
        device, the engine's scratch grown for it, the call and the fetch.  'pairs': the weights wv (q_all, n) of all components
        and idx = pairs (npairs, 2); 'matrix' / 'view': the row vectors wv of the local components, idx = ks, and the float64
        factorisation of the last evaluate(); 'view' takes its centres [x; xn] from the view `state`, not x.  masks: the pass over
        a caller's subsets (an output column per mask) instead of the 2 d + 1 standard ones and the mean term.  Returns the
        host array of the sums and the scratch."""
        torch = self.torch
        entry, sizer = _SOBOL_PASSES[kind][0 if masks is None else 1]
        if kind != 'pairs':
            assert self.dtype == _hip.F64, "%s reads the A^-1 %sof a float64 engine" % (caller, "and the view state " if state else "")
            if self._theta_last is None:
                raise RuntimeError("%s() needs a preceding evaluate() at the current parameters" % caller)
        if state is None:
            x = np.ascontiguousarray(x, np.float64)
            (n, d), m = x.shape, 0
        else:
            n, d, m = self.n, self.d, state['m']
        wv = np.ascontiguousarray(wv, np.float64)
        ell = np.ascontiguousarray(ell, np.float64)
        box = np.ascontiguousarray(box, np.float64)
        idx = np.ascontiguousarray(idx, np.int32)
        if kind == 'pairs':
            q, nidx = wv.shape[0], idx.shape[0]
            assert idx.shape == (nidx, 2)
        else:
            idx = idx.reshape(-1)
            q, nidx = self.q_local, idx.shape[0]
            assert n == self.n and d == self.d
        assert wv.shape == (q, n + m) and ell.shape == (q, d) and box.shape == (2, d)
        tail = ()
        if masks is not None:
            masks = self._subset_masks(masks, d, caller)
            tail = (masks.ctypes.data_as(C.POINTER(C.c_uint64)), masks.shape[0])
        _checked_box(box, caller)
        tiles = -(-(n + m) // 64)
        what = _SOBOL_PASSES[kind][2] % ("pair" if masks is None else "subset")
        if state is None:
            refusal = (what, "%d tile sums of %d %s at a time" % (tiles ** 2, min(nidx, 64), "pairs" if kind == 'pairs' else "components"),
                       "use fewer training inputs")
        else:
            refusal = (what, "one component's %d x %d matrix E and %d tile sums" % (64 * tiles, 64 * tiles, tiles ** 2),
                       "condition on fewer new inputs at a time")
        with torch.cuda.device(self.device):
            if state is None:
                model = () if kind == 'pairs' else (self.dtype,)
                head = (self._stream(),) + model + (self.kernel_id, n, d) + (() if kind == 'pairs' else (self.p,)) + (q,)
                dev = [torch.as_tensor(a).to(self.device) for a in (x, wv, ell, box)]
                head += tuple(self._p(t) for t in dev) + (() if kind == 'pairs' else (self._p(self.workspace),))
                dims = (n, d, q, nidx)
            else:
                self._condition_grad_state(state)
                xa = torch.cat([self.x, state['xn']]).contiguous()           # (float64: the engine's dtype)
                dev = [torch.as_tensor(a).to(self.device) for a in (wv, ell, box)]
                head = (self._stream(), self.dtype, self.kernel_id, n, d, self.p, q, self._p(self.theta_dev), self._p(self.workspace),
                        self._p(state['state']), m, self._p(xa)) + tuple(self._p(t) for t in dev)
                dims = (n, d, q, m, nidx)
            scratch = self._grow_scratch(self._nbytes(sizer, *dims, *tail[1:]), refusal)
            out = torch.empty((nidx, 2 * d + 2 if masks is None else tail[1]), dtype=torch.float64, device=self.device)
            scs = (self._p(scratch),) if state is None else (self._p(scratch), scratch.numel())
            _hip.check(getattr(self.lib, entry)(*head, idx.ctypes.data_as(C.POINTER(C.c_int)), nidx, *tail, *scs, self._p(out)), entry)
            return out.cpu().numpy(), scratch

    # ---- the same three passes for a caller's list of input subsets ----
    def _subset_masks(self, masks, d, what):
        """the checked uint64 masks (bit l set: input l is in the subset) of a subset pass over d inputs"""
        masks = np.ascontiguousarray(masks, np.uint64).reshape(-1)
        if d > 16:
            raise ValueError("%s: the subset pass takes at most 16 inputs (d = %d)" % (what, d))
        if masks.shape[0] < 1 or np.any(masks >> np.uint64(d)):
            raise ValueError("%s: needs at least one mask, and no mask may have a bit at or above d = %d" % (what, d))
        return masks

    def sobol_subset_pairs(self, x, w, ell, box, pairs, masks):
        """sobol_pairs for a list of subsets of the inputs (lcgp_sobol_subset_pairs): masks (nsub,) bit masks, bit
        l set when input l is in the subset u; the other arguments as there.  Returns host arrays (D (npairs, nsub), means
        (npairs,)): D[r, s] = D_u of the pair for u = masks[s] (the empty mask: exactly 0); means as sobol_pairs returns them.
        lcgp_sobol_subset_chunk(d) masks per launch; d <= 16."""
        res, scratch = self._sobol_pass("sobol_subset_pairs", 'pairs', x, w, ell, box, pairs, masks)
        pairs = np.asarray(pairs, np.int32)
        (n, d), q_all = np.shape(x), np.shape(w)[0]
        with self.torch.cuda.device(self.device):
            # (the box means of the components follow the table in the scratch: include/lcgp_hip.h)
            comp = scratch[8 * q_all * d * n:8 * (q_all * d * n + q_all)].view(self.torch.float64).cpu().numpy()
        means = np.where(pairs[:, 0] == pairs[:, 1], comp[pairs[:, 0]], 0.0)
        return res, means

    def sobol_matrix_subset_sums(self, x, v, ell, box, ks, masks):
        """sobol_matrix_sums for a list of subsets of the inputs (lcgp_sobol_matrix_subset_pairs): masks (nsub,)
        as in sobol_subset_pairs, the other arguments as there.  Returns the host array sums (len(ks), nsub) = sum Q (M_u - M_0)
        for u = masks[s]; no S0 (the corrections of the subsets do not need it)."""
        return self._sobol_pass("sobol_matrix_subset_sums", 'matrix', x, v, ell, box, ks, masks)[0]

    def condition_sobol_matrix_subset_sums(self, state, v, ell, box, ks, masks):
        """condition_sobol_matrix_sums for a list of subsets of the inputs (lcgp_condition_sobol_matrix_subset_pairs; DESIGN.md
        4.25): masks (nsub,) as in sobol_subset_pairs, the other arguments as there.  Returns the host array sums (len(ks), nsub)
        = sum Q' (M_u - M_0) over the N = n + m centres.  E is prepared once per component, whatever the number of masks."""
        return self._sobol_pass("condition_sobol_matrix_subset_sums", 'view', None, v, ell, box, ks, masks, state)[0]

    def condition_mean_vectors(self, state):
        """(z' (q_local, n), w (q_local, m)) of the view `state` on the host: its mean surface is X_0 z' + c^x(x0, xn) w (the grad
        state of lcgp_condition_grad_prepare, built on first use)"""
        torch = self.torch
        m = state['m']
        with torch.cuda.device(self.device):
            gs = self._condition_grad_state(state)
            w = torch.empty((self.q_local, m), dtype=torch.float64, device=self.device)
            z = torch.empty((self.q_local, self.n), dtype=torch.float64, device=self.device)
            _hip.check(self.lib.lcgp_condition_grad_fetch(self._stream(), self.n, self.q_local, m, self._p(gs), self._p(w),
                                                          self._p(z)), "lcgp_condition_grad_fetch")
            return z.cpu().numpy(), w.cpu().numpy()

    def predict_device(self, x0s, same=False):
        """ghat, gvar (q_local, n0): the two halves of predict_block()"""
        out = self.predict_block(x0s, same)
        return out[0], out[1]

    def predict(self, x0s, same=False):
        ghat, gvar = self.predict_device(x0s, same)
        return ghat.cpu().numpy(), gvar.cpu().numpy()

    # ------------------------------------------------------------------------------------------------
    def _require_memory(self, nbytes, what, detail, advice):
        """ValueError before an allocation of nbytes that does not fit in the free device memory"""
        free, _ = self.torch.cuda.mem_get_info(self.device)
        free += self.torch.cuda.memory_reserved(self.device) - self.torch.cuda.memory_allocated(self.device)
        if nbytes > free:
            raise ValueError("%s needs %.2f GB of device memory (%s), %.2f GB are free: %s"
                             % (what, nbytes / 1e9, detail, free / 1e9, advice))

    def _fit_group(self, sizer, *dims, q_group=None):
        """(group, nbytes): how many local components a grouped query processes at once and the scratch `sizer` wants for them
        (dims: its arguments, None where the group goes).  All of them, or at most q_group, halved until the scratch fits in the
        free device memory -- the engine's own scratch counts as free -- or one component is left.  Inside the device context."""
        torch = self.torch
        free, _ = torch.cuda.mem_get_info(self.device)
        free += torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
        free += 0 if self._scratch is None else self._scratch.numel()
        group = self.q_local if q_group is None else max(1, min(int(q_group), self.q_local))
        while True:
            nbytes = self._nbytes(sizer, *[group if a is None else a for a in dims])
            if group == 1 or nbytes <= free:
                return group, nbytes
            group = (group + 1) // 2

    def _cov_refusal(self, what):
        """the free-memory check's text for the joint covariance's buffers"""
        return what, "%d components of n0 x n0, 3 matrices each" % self.q_local, "pass fewer new inputs"

    def _grow_scratch(self, nbytes, refusal=None):
        """the engine's one scratch buffer, grown to at least nbytes; with refusal (what, detail, advice) checked against the
        free device memory before it grows"""
        if self._scratch is None or self._scratch.numel() < nbytes:
            self._scratch = None
            if refusal is not None:
                self._require_memory(nbytes, *refusal)
            self._scratch = self.torch.empty(int(nbytes), dtype=self.torch.uint8, device=self.device)
        return self._scratch

    def _workspace2(self, slot, key, nbytes, refusal):
        """the second workspace cached in attribute `slot` ('_cov_ws', '_cv_ws' or '_cond_ws': a model can hold all) as (key, workspace);
        a new key releases the old one, then nbytes() is checked against the free device memory (refusal: what, detail,
        advice) and allocated"""
        held = getattr(self, slot)
        if held is not None and held[0] == key:
            return held[1]
        setattr(self, slot, None)
        nb = nbytes()
        self._require_memory(nb, *refusal)
        ws = self.torch.empty(nb, dtype=self.torch.uint8, device=self.device)
        setattr(self, slot, (key, ws))
        return ws

    def form_cov(self, x0s, same=False, jitter=0.0):
        """Sigma_k + jitter scale_k I of the local components into the cov workspace for n0 = len(x0s) (lcgp_predict_cov);
        returns the workspace (asynchronous)."""
        return self._form_cov(None, x0s, same, jitter)

    def _form_cov(self, state, x0s, same, jitter):
        """form_cov of the fitted model (state = None) or of the view `state` (condition_begin; lcgp_condition_predict_cov:
        the same launches on rows widened to K' = npad + mpad, same = 0)"""
        torch = self.torch
        if self._theta_last is None:
            raise RuntimeError("predict_cov() needs a preceding evaluate() at the current parameters")
        m, view, kp = self._view_args(state)
        x0s = np.ascontiguousarray(x0s, np.float64)
        n0 = x0s.shape[0]
        assert x0s.ndim == 2 and x0s.shape[1] == self.d and n0 >= 1
        if state is None:
            refusal = self._cov_refusal
        else:
            def refusal(what):
                return (what + " on a conditioned view",
                        "%d components of n0 x n0, 3 matrices each, and of n0 x K', K' = npad + mpad = %d" % (self.q_local, kp),
                        "pass fewer new inputs")
        with torch.cuda.device(self.device):
            # the second workspace, carved for n = n0, whose matrix slot receives Sigma_k + tau_k I and then its factor
            # (lcgp_potrf_logdet): 3 q_local n0pad^2 elements (n0pad = n0 rounded up to 128), 3.2 GB at n0 = 4096, q_local = 8
            # in float64
            cws = self._workspace2('_cov_ws', n0, lambda: self._nbytes("lcgp_workspace_bytes", self.dtype, n0, self.d, self.p, self.q_local),
                                   refusal("the joint covariance of %d new inputs" % n0))
            if state is None:
                nbytes = self._nbytes("lcgp_predict_cov_scratch_bytes", self.dtype, self.n, self.q_local, n0)
            else:
                nbytes = self._nbytes("lcgp_condition_predict_cov_scratch_bytes", self.dtype, self.n, self.q_local, m, n0)
            scratch = self._grow_scratch(nbytes, refusal("the scratch of the joint covariance"))
            x0d = torch.as_tensor(x0s).to(self.device, self.tdtype).contiguous()
            head = self._head()
            if state is None:
                _hip.check(self.lib.lcgp_predict_cov(*head, n0, self._p(x0d), 1 if same else 0, self._p(scratch), self._p(cws),
                                                     float(jitter)), "lcgp_predict_cov")
            else:
                _hip.check(self.lib.lcgp_condition_predict_cov(*head, *view, n0, self._p(x0d), self._p(scratch), scratch.numel(),
                                                               self._p(cws), float(jitter)), "lcgp_condition_predict_cov")
            return cws

    def fetch_cov(self, n0, which=0):
        """(q_local, n0, n0) DEVICE tensor of the engine's dtype: matrix slot of the cov workspace, lower triangle mirrored"""
        torch = self.torch
        cws = self._cov_ws[1]
        with torch.cuda.device(self.device):
            out = torch.empty((self.q_local, n0, n0), dtype=self.tdtype, device=self.device)
            for k in range(self.q_local):
                _hip.check(self.lib.lcgp_fetch_matrix(self._stream(), self.dtype, n0, self.d, self.p, self.q_local, self._p(cws),
                                                      int(which), k, self._p(out[k])), "lcgp_fetch_matrix")
            return out

    def predict_cov(self, x0s, same=False):
        """(q_local, n0, n0) float64 DEVICE tensor Sigma_k = C00_k - D_k U_k U_k^T of the local components (before any jitter
        or factorisation), from the factorisation of the last evaluate().  Memory: the cov workspace, 3 q_local n0pad^2
        elements, and a scratch of 2 q_local n0pad npad elements."""
        return self._predict_cov(None, x0s, same)

    def condition_predict_cov(self, state, x0s):
        """predict_cov of the view `state` (condition_begin): Sigma'_k = C00_k - D_k U^ U^^T on rows widened to K' = npad + mpad
        (lcgp_condition_predict_cov), same = 0.  Memory: the cov workspace and a scratch of q_local n0pad K' elements plus the
        row former's work areas.  The base factorisation must still be the one the state was built from."""
        return self._predict_cov(state, x0s, False)

    def _predict_cov(self, state, x0s, same):
        self._form_cov(state, x0s, same, 0.0)
        return self.fetch_cov(len(x0s)).to(self.torch.float64)

    def factor_cov(self, n0):
        """factorises Sigma_k + tau_k I in the cov workspace in place (lcgp_potrf_logdet, plan with_inverse = 0); returns the
        per-component info words on the host (0 = positive definite, else 1 + index of the first failing pivot)"""
        torch = self.torch
        plan = self._cached_plan('cov', n0, self.q_local)
        with torch.cuda.device(self.device):
            info = torch.zeros(self.q_local, dtype=torch.int32, device=self.device)
            _hip.check(self.lib.lcgp_potrf_logdet(self._stream(), self.dtype, n0, self.d, self.p, self.q_local,
                                                  self._p(self._cov_ws[1]), None, self._p(info), None,
                                                  C.c_void_p(plan.ctypes.data)), "lcgp_potrf_logdet")
            return info.cpu().numpy()

    def sample_latent(self, x0s, S, seeds, jitter=1e-10, same=False):
        """(q_local, S, n0) float64 DEVICE tensor of draws g_k = ghat_k + L_k eps_k, L_k L_k^T = Sigma_k + jitter scale_k I.
        eps_k (S x n0 standard normals) comes from numpy's default_rng(seeds[i]) for local component i, so a caller that
        seeds by GLOBAL component gets draws independent of the sharding.  Raises numpy.linalg.LinAlgError naming the local
        components whose Sigma_k + tau_k I is not numerically positive definite (the `info` words); never returns NaNs."""
        return self._sample_latent(None, x0s, S, seeds, jitter, same)

    def condition_sample_latent(self, state, x0s, S, seeds, jitter=1e-10):
        """sample_latent of the view `state` (condition_begin): draws ghat'_k + L_k eps_k, L_k L_k^T = Sigma'_k + jitter scale_k I,
        with ghat' condition_predict_block's and Sigma' condition_predict_cov's; the factorisation, the seeding and the draws
        are sample_latent's.  The base factorisation must still be the one the state was built from."""
        return self._sample_latent(state, x0s, S, seeds, jitter, False)

    def _sample_latent(self, state, x0s, S, seeds, jitter, same):
        torch = self.torch
        x0s = np.ascontiguousarray(x0s, np.float64)
        n0, S = x0s.shape[0], int(S)
        assert len(seeds) == self.q_local and S >= 1
        ghat = (self.predict_block(x0s, same) if state is None else self.condition_predict_block(state, x0s))[0]
        self._form_cov(state, x0s, same, jitter)
        info = self.factor_cov(n0)
        if np.any(info != 0):
            bad = [(i, int(v)) for i, v in enumerate(info) if v != 0]
            err = np.linalg.LinAlgError("Sigma_k + jitter * scale_k I is not numerically positive definite for local components "
                                        "(index, info) %s at jitter=%g" % (bad, jitter))
            err.info = info
            raise err
        eps_all = np.stack([np.random.default_rng(s).standard_normal((S, n0)) for s in seeds])
        with torch.cuda.device(self.device):
            out = torch.empty((self.q_local, S, n0), dtype=torch.float64, device=self.device)
            for lo in range(0, S, SAMPLE_CHUNK):
                m = min(SAMPLE_CHUNK, S - lo)
                scratch = self._grow_scratch(self._nbytes("lcgp_sample_scratch_bytes", self.dtype, n0, self.q_local, m),
                                             self._cov_refusal("the scratch of the joint covariance"))
                eps = torch.as_tensor(np.ascontiguousarray(eps_all[:, lo:lo + m])).to(self.device, self.tdtype).contiguous()
                dst = out if m == S else torch.empty((self.q_local, m, n0), dtype=torch.float64, device=self.device)
                _hip.check(self.lib.lcgp_sample_latent(self._stream(), self.dtype, n0, self.d, self.p, self.q_local, m,
                                                       self._p(self._cov_ws[1]), self._p(eps), self._p(ghat), n0,
                                                       self._p(scratch), self._p(dst)), "lcgp_sample_latent")
                if dst is not out:
                    out[:, lo:lo + m].copy_(dst)
            return out

    # ------------------------------------------------------------------------------------------------
    # conditioning on new runs without refactorising (lcgp_hip.h: lcgp_condition_prepare / lcgp_condition_predict)
    def condition_begin(self, xn_s, t, r=None):
        """The state of a view conditioned on m new unique inputs xn_s (m, d; standardised, none of them a training input) with
        latent observations t (q_local, m) and replicate counts r (m; None = ones), from the factorisation of the last
        evaluate(), which is only read (lcgp_condition_prepare): a dict holding the device state (U_n, L_S^-1 and v per local
        component), the inputs on the device and the theta rows it belongs to.  The conditioning matrices are factorised in a
        second workspace carved for n = m (3 q_local mpad^2 elements, mpad = m rounded up to 128); the state holds q_local mpad
        (npad + mpad) elements.  Raises ValueError when they do not fit in the free device memory, and
        numpy.linalg.LinAlgError carrying the per-local-component info words when an S_k is not numerically positive definite."""
        torch = self.torch
        if self._theta_last is None:
            raise RuntimeError("condition() needs a preceding evaluate() at the current parameters")
        xn_s = np.ascontiguousarray(xn_s, np.float64)
        m, d = xn_s.shape[0], self.d
        t = np.ascontiguousarray(t, np.float64)
        assert xn_s.ndim == 2 and xn_s.shape[1] == d and m >= 1 and t.shape == (self.q_local, m)
        assert r is None or np.shape(r) == (m,)
        refusal = ("conditioning on %d new inputs" % m, "%d components of %d x (n + 4 m)" % (self.q_local, m),
                   "condition on fewer new inputs at a time")
        with torch.cuda.device(self.device):
            cws = self._workspace2('_cond_ws', m, lambda: self._nbytes("lcgp_workspace_bytes", self.dtype, m, d, self.p, self.q_local),
                                   refusal)
            scratch = self._grow_scratch(self._nbytes("lcgp_condition_scratch_bytes", self.dtype, self.n, self.q_local, m, 0), refusal)
            nstate = self._nbytes("lcgp_condition_state_bytes", self.dtype, self.n, d, self.q_local, m)
            self._require_memory(nstate, *refusal)
            state = torch.empty(nstate, dtype=torch.uint8, device=self.device)
            xnd = torch.as_tensor(xn_s).to(self.device, self.tdtype).contiguous()
            td = torch.as_tensor(t).to(self.device)
            rd = None if r is None else torch.as_tensor(np.ascontiguousarray(r, np.float64)).to(self.device)
            info = torch.zeros(self.q_local, dtype=torch.int32, device=self.device)
            _hip.check(self.lib.lcgp_condition_prepare(
                *self._head(), m, self._p(xnd), self._p(td), self._p(rd), self._p(scratch), scratch.numel(), self._p(cws),
                self._p(state), self._p(info)), "lcgp_condition_prepare")
            info = info.cpu().numpy()
        if np.any(info != 0):
            err = np.linalg.LinAlgError("condition(): S_k is not numerically positive definite for local components (index, info) %s"
                                        % [(i, int(v)) for i, v in enumerate(info) if v != 0])
            err.info = info
            raise err
        return {'m': m, 'xn': xnd, 'state': state, 'theta': self._theta_last.copy()}

    def _condition_grad_state(self, state):
        """the grad state of the view `state` (w = L_S^-T v and z' per local component: lcgp_condition_grad_prepare), built on
        first use and kept with the view's state"""
        torch = self.torch
        gs = state.get('grad')
        if gs is None:
            m = state['m']
            gs = torch.empty(self._nbytes("lcgp_condition_grad_state_bytes", self.dtype, self.n, self.q_local, m),
                             dtype=torch.uint8, device=self.device)
            _hip.check(self.lib.lcgp_condition_grad_prepare(
                self._stream(), self.dtype, self.n, self.d, self.p, self.q_local, self._p(self.theta_dev), self._p(self.workspace),
                self._p(state['state']), m, self._p(gs)), "lcgp_condition_grad_prepare")
            state['grad'] = gs
        return gs

    # (the per-point queries of the view `state`: the fitted model's methods with state)
    def condition_predict_block(self, state, x0s):
        return self.predict_block(x0s, state=state)

    def condition_predict_grad_block(self, state, x0s):
        return self.predict_grad_block(x0s, state=state)

    def condition_predict_hess_block(self, state, x0s):
        return self.predict_hess_block(x0s, state=state)

    def condition_grad_cov_block(self, state, x0s, w=None, per_point=True):
        return self.grad_cov_block(x0s, w, per_point, state=state)

    # ------------------------------------------------------------------------------------------------
    # closed-form cross-validation at fixed parameters (lcgp_hip.h: lcgp_loo, lcgp_cv_gather / lcgp_cv_apply)
    def loo_block(self):
        """(2, q_local, n) float64 DEVICE tensor [ghat; gvar] of leave-one-out at every training input, from the factorisation
        of the last evaluate() (lcgp_loo: reads A^-1's diagonal, b and z; one launch)."""
        torch = self.torch
        if self._theta_last is None:
            raise RuntimeError("predict_loo() needs a preceding evaluate() at the current parameters")
        with torch.cuda.device(self.device):
            out = torch.empty((2, self.q_local, self.n), dtype=torch.float64, device=self.device)
            _hip.check(self.lib.lcgp_loo(self._stream(), self.dtype, self.n, self.d, self.p, self.q_local, self._p(self.sr),
                                         self._p(self.theta_dev), self._p(self.workspace), self._p(out[0]), self._p(out[1]),
                                         self.n), "lcgp_loo")
            self._raise_if_not_finite(out)
            return out

    def _raise_if_not_finite(self, out, info=None):
        """LinAlgError carrying per-local-component info words when a fold factorisation failed (info) or a result is not
        finite (never hand NaNs on)"""
        bad = ~self.torch.isfinite(out).reshape(2, self.q_local, -1).all(dim=2).all(dim=0)
        codes = bad.cpu().numpy().astype(np.int64)
        if info is not None:
            codes = np.where(info != 0, info, codes)
        if np.any(codes != 0):
            err = np.linalg.LinAlgError("cross-validation: a fold matrix of local components (index, info) %s is not numerically "
                                        "positive definite" % [(i, int(v)) for i, v in enumerate(codes) if v != 0])
            err.info = codes
            raise err

    def cv_block(self, fold_ptr, fold_idx, return_cov=False):
        """(2, q_local, n) float64 DEVICE tensor [ghat; gvar]: the prediction at the inputs of each fold of the model conditioned
        on the other folds (lcgp_cv_gather -> lcgp_potrf_logdet -> lcgp_potri -> lcgp_cv_apply).  fold_ptr (F + 1) / fold_idx
        (n): CSR over the training inputs, each fold sorted ascending.  return_cov: also a list of F float64 DEVICE tensors
        (q_local, m_f, m_f), the latent covariance of each fold.  Raises numpy.linalg.LinAlgError carrying per-local-component
        info words when a fold matrix is not numerically positive definite."""
        torch = self.torch
        if self._theta_last is None:
            raise RuntimeError("predict_cv() needs a preceding evaluate() at the current parameters")
        fold_ptr = np.asarray(fold_ptr, np.int64)
        F = len(fold_ptr) - 1
        folds_host = np.ascontiguousarray(np.concatenate([fold_ptr, np.asarray(fold_idx, np.int64)]).astype(np.int32))
        sizes = np.diff(fold_ptr)
        mmax = int(sizes.max()) if F >= 1 else 0
        qf = self.q_local * F
        with torch.cuda.device(self.device):
            # the fold workspace (carved for n = mmax and q_local F components): 3 q_local F mpad^2 elements (mpad = mmax rounded
            # up to 128)
            cws = self._workspace2('_cv_ws', (mmax, F), lambda: self._nbytes("lcgp_cv_workspace_bytes", self.dtype, self.n, self.d, self.p,
                                                                         self.q_local, F, C.c_void_p(folds_host.ctypes.data)),
                                   ("cross-validation over %d folds of up to %d inputs" % (F, mmax),
                                    "%d components x %d folds, 3 matrices each" % (self.q_local, F), "use fewer or smaller folds"))
            folds = torch.as_tensor(folds_host).to(self.device)
            hp = C.c_void_p(folds_host.ctypes.data)
            st = self._stream()
            _hip.check(self.lib.lcgp_cv_gather(st, self.dtype, self.n, self.d, self.p, self.q_local, self._p(self.workspace), F, hp,
                                               self._p(folds), self._p(cws)), "lcgp_cv_gather")
            info = torch.zeros(qf, dtype=torch.int32, device=self.device)
            _hip.check(self.lib.lcgp_potrf_logdet(st, self.dtype, mmax, self.d, self.p, qf, self._p(cws), None, self._p(info), None,
                                                  C.c_void_p(self._cached_plan('cv', mmax, qf).ctypes.data)), "lcgp_potrf_logdet")
            _hip.check(self.lib.lcgp_potri(st, self.dtype, mmax, self.d, self.p, qf, self._p(cws), None), "lcgp_potri")
            out = torch.empty((2, self.q_local, self.n), dtype=torch.float64, device=self.device)
            _hip.check(self.lib.lcgp_cv_apply(st, self.dtype, self.n, self.d, self.p, self.q_local, self._p(self.sr),
                                              self._p(self.theta_dev), self._p(self.workspace), F, hp, self._p(folds), self._p(cws),
                                              self._p(out[0]), self._p(out[1]), self.n), "lcgp_cv_apply")
            # a failed pivot of any fold of component k is reported on k (slot f * q_local + k)
            inf = info.cpu().numpy().reshape(F, self.q_local)
            self._raise_if_not_finite(out, np.where(inf != 0, inf, 0).max(axis=0))
            if not return_cov:
                return out
            covs = []
            mi = torch.empty((mmax, mmax), dtype=self.tdtype, device=self.device)
            D = self.theta_dev[:, self.d + 2]
            s = torch.ones(self.n, dtype=torch.float64, device=self.device) if self.sr is None else self.sr.to(torch.float64)
            for f in range(F):
                m = int(sizes[f])
                idx = folds[F + 1 + int(fold_ptr[f]):F + 1 + int(fold_ptr[f + 1])].long()
                sb = s[idx]
                cov = torch.empty((self.q_local, m, m), dtype=torch.float64, device=self.device)
                for k in range(self.q_local):
                    _hip.check(self.lib.lcgp_fetch_matrix(st, self.dtype, mmax, self.d, self.p, qf, self._p(cws), 2,
                                                          f * self.q_local + k, self._p(mi)), "lcgp_fetch_matrix")
                    cov[k] = mi[:m, :m]
                cov.diagonal(dim1=1, dim2=2).sub_(1.0)
                cov /= D[:, None, None] * (sb[:, None] * sb[None, :])[None]
                covs.append(cov)
            return out, covs

    # ------------------------------------------------------------------------------------------------
    # integrated variance reduction at fixed parameters (lcgp_hip.h: lcgp_variance_reduction_prepare / lcgp_variance_reduction)
    def _view_args(self, state):
        """what the entries on a conditioned view take beyond those of the fitted model: (m, (state, m, xn) pointers, K' = npad +
        mpad), after the staleness check of condition_predict_block; state = None (the fitted model): (0, (), npad)"""
        npad = -(-self.n // 128) * 128
        if state is None:
            return 0, (), npad
        if not self.is_current(state['theta']):
            raise RuntimeError("the conditioned view does not belong to the factorisation in the workspace")
        m = state['m']
        return m, (self._p(state['state']), m, self._p(state['xn'])), npad + -(-m // 128) * 128

    def _design_inputs(self, caller, x_cand_s, x_ref_s, w, match=None):
        """The host half of a design query: the check that an evaluation stands behind `caller`, then (x_cand_s, x_ref_s, match,
        shared): the checked float64 candidates (n_cand, d) and reference set (n_ref, d) with its n_ref weights w, match as
        _match_or_none leaves it; shared: x_ref_s was None, the reference set IS the candidate set"""
        if self._theta_last is None:
            raise RuntimeError("%s() needs a preceding evaluate() at the current parameters" % caller)
        x_cand_s = np.ascontiguousarray(x_cand_s, np.float64)
        assert x_cand_s.ndim == 2 and x_cand_s.shape[1] == self.d and x_cand_s.shape[0] >= 1
        match = _match_or_none(match)
        shared = x_ref_s is None
        x_ref_s = x_cand_s if shared else np.ascontiguousarray(x_ref_s, np.float64)
        assert x_ref_s.ndim == 2 and x_ref_s.shape[1] == self.d and x_ref_s.shape[0] >= 1 and len(w) == x_ref_s.shape[0]
        return x_cand_s, x_ref_s, match, shared

    def _design_open(self, query, view_args, lead, trail, refusal, x_ref_s, x_cand_s, w, match):
        """The device half of a design query (_DESIGN_QUERIES) on the fitted model or on a view (view_args = _view_args(state)),
        inside the device context: the engine's scratch grown to what the family's scratch query returns for lead + (m on a view)
        + trail (refusal: what, detail, advice of the free-memory check), then the inputs on the device.  Returns (the family's
        other entry names, the dims, (scratch[, scratch_bytes]) as the entries take them, the head with the view, (xr, xc, wd,
        md)); x_cand_s / match = None: no xc / md."""
        torch = self.torch
        m, view, _ = view_args
        sizer, *names = _DESIGN_QUERIES[query][1 if view else 0]
        dims = lead + ((m,) if view else ()) + trail
        scratch = self._grow_scratch(self._nbytes(sizer, *dims), refusal)
        xr = torch.as_tensor(x_ref_s).to(self.device, self.tdtype).contiguous()
        xc = None if x_cand_s is None else torch.as_tensor(x_cand_s).to(self.device, self.tdtype).contiguous()
        wd = torch.as_tensor(np.ascontiguousarray(w, np.float64)).to(self.device)
        md = None if match is None else torch.as_tensor(match).to(self.device)
        scs = (self._p(scratch), scratch.numel()) if view else (self._p(scratch),)
        return names, dims, scs, self._head() + view, (xr, xc, wd, md)

    def variance_reduction_block(self, x_cand_s, x_ref_s, w, match, r):
        return self._vr_block(None, x_cand_s, x_ref_s, w, match, r)

    def condition_variance_reduction_block(self, state, x_cand_s, x_ref_s, w, match, r):
        """variance_reduction_block of the view `state` (condition_begin): R'_k(c) of the model conditioned on the view's runs
        (lcgp_condition_vr_prepare / lcgp_condition_vr: the same launches on rows widened to K' = npad + mpad).  The base
        factorisation must still be the one the state was built from."""
        return self._vr_block(state, x_cand_s, x_ref_s, w, match, r)

    def _vr_block(self, state, x_cand_s, x_ref_s, w, match, r):
        """(q_local, n_cand) float64 DEVICE tensor R_k(c) = sum_t w_t Sigma_k(t, c)^2 / (max(Sigma_k^h(c, c), 0) + 1 / (D_k r)), from
        the factorisation of the last evaluate().  x_cand_s (n_cand, d) / x_ref_s (n_ref, d): standardised; x_ref_s = None: the
        reference set IS the candidate set.  w: n_ref weights (used as given).  match: None or n_cand ints, -1 or the training
        input a candidate replicates (its cross row carries the nugget term there).  U of the reference set is formed once per
        call; candidates go in chunks of PREDICT_CHUNK; with x_ref_s = None and no match one U serves both.  Raises ValueError
        when the scratch does not fit in the free device memory."""
        torch, d = self.torch, self.d
        x_cand_s, x_ref_s, match, shared = self._design_inputs("variance_reduction", x_cand_s, x_ref_s, w, match)
        shared = shared and match is None
        n_cand, n_ref = x_cand_s.shape[0], x_ref_s.shape[0]
        chunk = min(n_cand, PREDICT_CHUNK)
        va = self._view_args(state)
        with torch.cuda.device(self.device):
            detail = ("%d components of (n_ref + %d candidates) x n" % (self.q_local, chunk) if state is None else
                      "%d components of (n_ref + %d candidates) x K', K' = npad + mpad = %d" % (self.q_local, chunk, va[2]))
            (prepare, entry), _, scs, head, (xr, xc, wd, md) = self._design_open(
                'vr', va, (self.dtype, self.n, self.q_local), (n_ref, chunk),
                ("the variance reduction over %d reference points" % n_ref, detail, "pass fewer reference points"),
                x_ref_s, None if shared else x_cand_s, w, match)
            out = torch.empty((self.q_local, n_cand), dtype=torch.float64, device=self.device)
            _hip.check(getattr(self.lib, prepare)(*head, n_ref, self._p(xr), *scs), prepare)
            for lo in range(0, n_cand, chunk):
                rows = min(chunk, n_cand - lo)
                xcp = C.c_void_p(0) if shared else C.c_void_p(xc.data_ptr() + lo * d * xc.element_size())
                mh = C.c_void_p(0) if match is None else C.c_void_p(match.ctypes.data + 4 * lo)
                mdp = C.c_void_p(0) if match is None else C.c_void_p(md.data_ptr() + 4 * lo)
                _hip.check(getattr(self.lib, entry)(*head, n_ref, self._p(xr), self._p(wd), rows, xcp, mh, mdp,
                                                    lo if shared else -1, int(r), *scs, C.c_void_p(out.data_ptr() + 8 * lo),
                                                    n_cand), entry)
            return out

    def box_alc_block(self, x_cand_s, box_s, match, r, q_group=None):
        """(q_local, n_cand) float64 DEVICE tensor R_k(c), the drop of the box-integrated posterior variance IV_k if the simulator
        ran r more times at candidate c (lcgp_box_alc), from the factorisation of the last evaluate() -- which is
        only read.  x_cand_s (n_cand, d) standardised candidates, box_s (2, d) = [lo; hi] standardised, match as in
        variance_reduction_block.  float64 engines only.  The candidates go in chunks of PREDICT_CHUNK rows (never fewer than 128
        while there are that many: point_passes), the local components in groups halved until the scratch fits in the free device
        memory (q_group: at most that many, for tests): one npad^2 matrix and two chunk_pad x npad slabs per component processed
        at once; the matrix of a group is formed once and serves all chunks.  Results are bitwise independent of the chunking, of
        the grouping and of the scratch content.  Raises ValueError when even one component does not fit."""
        torch = self.torch
        if self._theta_last is None:
            raise RuntimeError("integrated_variance_reduction() needs a preceding evaluate() at the current parameters")
        if self.dtype != _hip.F64:
            raise RuntimeError("the exact box ALC is float64 only: evaluate on a float64 engine")
        x_cand_s = np.ascontiguousarray(x_cand_s, np.float64)
        box_s = np.ascontiguousarray(box_s, np.float64)
        n0, d = x_cand_s.shape[0], self.d
        assert x_cand_s.ndim == 2 and x_cand_s.shape[1] == d and n0 >= 1 and box_s.shape == (2, d)
        _checked_box(box_s, "box_alc_block")
        match = _match_or_none(match)
        chunk = min(n0, max(PREDICT_CHUNK, 128) if n0 >= 128 else PREDICT_CHUNK)
        with torch.cuda.device(self.device):
            group, nbytes = self._fit_group("lcgp_box_alc_scratch_bytes", self.dtype, self.n, d, None, chunk, q_group=q_group)
            scp = self._p(self._grow_scratch(nbytes, ("the exact box ALC of %d candidates per pass" % chunk,
                                                      "one n x n matrix and two of %d x n per component" % chunk,
                                                      "use fewer training inputs per GPU or lower lcgp_amd.engine.PREDICT_CHUNK")))
            xcd = torch.as_tensor(x_cand_s).to(self.device).contiguous()
            boxd = torch.as_tensor(box_s).to(self.device).contiguous()
            md = None if match is None else torch.as_tensor(match).to(self.device)
            out = torch.empty((self.q_local, n0), dtype=torch.float64, device=self.device)
            head = self._head()
            for k0 in range(0, self.q_local, group):
                for i, (lo, rows, _) in enumerate(point_passes(n0, chunk, True)):
                    _hip.check(self.lib.lcgp_box_alc(
                        *head, k0, min(group, self.q_local - k0), self._p(boxd), rows, C.c_void_p(xcd.data_ptr() + 8 * lo * d),
                        C.c_void_p(0) if md is None else C.c_void_p(md.data_ptr() + 4 * lo), int(r), 1 if i == 0 else 0, scp,
                        C.c_void_p(out.data_ptr() + 8 * lo), n0), "lcgp_box_alc")
            return out

    def variance_reduction_grad_block(self, x_cand_s, x_ref_s, w, r):
        return self._vr_grad_block(None, x_cand_s, x_ref_s, w, r)

    def condition_variance_reduction_grad_block(self, state, x_cand_s, x_ref_s, w, r):
        """variance_reduction_grad_block of the view `state` (condition_begin): R'_k(c) of the model conditioned on the view's runs
        and its gradient (lcgp_condition_vr_prepare once, lcgp_condition_vr_grad per chunk: the same launches on rows widened to
        K' = npad + mpad, and the contraction over the n + m columns).  The base factorisation must still be the one the state
        was built from."""
        return self._vr_grad_block(state, x_cand_s, x_ref_s, w, r)

    def _vr_grad_block(self, state, x_cand_s, x_ref_s, w, r):
        """R (q_local, n_cand) and dR (q_local, n_cand, d) float64 DEVICE tensors: variance_reduction_block's R_k(c) with every
        candidate a new input (no match) and its gradient with respect to the candidate's standardised location, x_ref_s and
        w held constant (also with x_ref_s = None, where the reference set is a copy of the candidates)
        (lcgp_variance_reduction_prepare once, lcgp_variance_reduction_grad per chunk of PREDICT_CHUNK candidates; on a view
        their lcgp_condition_vr_* siblings).  Raises ValueError when the scratch does not fit in the free device memory."""
        torch, d = self.torch, self.d
        x_cand_s, x_ref_s, _, shared = self._design_inputs("variance_reduction_grad", x_cand_s, x_ref_s, w)
        n_cand, n_ref = x_cand_s.shape[0], x_ref_s.shape[0]
        chunk = min(n_cand, PREDICT_CHUNK)
        va = self._view_args(state)
        with torch.cuda.device(self.device):
            detail = ("%d components of n_ref x n and %d candidates x (n_ref + 3 n)" % (self.q_local, chunk) if state is None else
                      "%d components of n_ref x K' and %d candidates x (n_ref + 2 K' + 2 n), K' = npad + mpad = %d"
                      % (self.q_local, chunk, va[2]))
            (prepare, entry), _, scs, head, (xr, xc, wd, _) = self._design_open(
                'vr_grad', va, (self.dtype, self.n, d, self.q_local), (n_ref, chunk),
                ("the variance reduction gradient over %d reference points" % n_ref, detail, "pass fewer reference points"),
                x_ref_s, None if shared else x_cand_s, w, None)
            out = torch.empty((self.q_local, n_cand), dtype=torch.float64, device=self.device)
            dout = torch.empty((self.q_local, n_cand, d), dtype=torch.float64, device=self.device)
            _hip.check(getattr(self.lib, prepare)(*head, n_ref, self._p(xr), *scs), prepare)
            for lo in range(0, n_cand, chunk):
                rows = min(chunk, n_cand - lo)
                xcp = C.c_void_p(0) if shared else C.c_void_p(xc.data_ptr() + lo * d * xc.element_size())
                _hip.check(getattr(self.lib, entry)(*head, n_ref, self._p(xr), self._p(wd), rows, xcp, lo if shared else -1, int(r),
                                                    *scs, C.c_void_p(out.data_ptr() + 8 * lo), n_cand,
                                                    C.c_void_p(dout.data_ptr() + 8 * lo * d)), entry)
            return out, dout

    # ------------------------------------------------------------------------------------------------
    # greedy batch design by sequential ALC (lcgp_hip.h: lcgp_select_begin / lcgp_select_score / lcgp_select_condition)
    def select_begin(self, x_cand_s, x_ref_s, w, match, r, size):
        return self._select_begin(None, x_cand_s, x_ref_s, w, match, r, size)

    def condition_select_begin(self, state, x_cand_s, x_ref_s, w, match, r, size):
        """select_begin on the view `state` (condition_begin): the selection starts from the model conditioned on the view's
        runs (lcgp_condition_select_begin).  condition_select_rows / condition_select_condition carry it on."""
        return self._select_begin(state, x_cand_s, x_ref_s, w, match, r, size)

    def _select_begin(self, state, x_cand_s, x_ref_s, w, match, r, size):
        """Starts a greedy selection of `size` of the candidates: U and gvar of the reference set and of ALL candidates into the
        engine's scratch (candidates in passes of PREDICT_CHUNK rows) and the step-0 state R = variance_reduction_block(...) bitwise.
        Arguments as variance_reduction_block.  Raises ValueError when the scratch does not fit in the free device memory.  The
        state lives in the engine's scratch: no other query may run between select_begin and the last select_condition."""
        x_cand_s, x_ref_s, match, _ = self._design_inputs("select_batch", x_cand_s, x_ref_s, w, match)
        n_cand, n_ref = x_cand_s.shape[0], x_ref_s.shape[0]
        assert 1 <= size <= n_cand
        self._sel = None
        va = m, view, kp = self._view_args(state)
        with self.torch.cuda.device(self.device):
            detail = ("%d components of (%d reference points + %d candidates) x %s, all resident"
                      % (self.q_local, n_ref, n_cand, "K', K' = npad + mpad = %d" % kp if view else "n"))
            # (dims: what every entry of the family takes; on a view m goes behind q_local)
            (pre,), dims, scs, head, (xr, xc, wd, md) = self._design_open(
                'select', va, (self.dtype, self.n, self.d, self.q_local), (n_ref, n_cand, int(size)),
                ("the batch selection over %d candidates" % n_cand, detail, "pass fewer candidates"), x_ref_s, x_cand_s, w, match)
            _hip.check(getattr(self.lib, pre + "begin")(
                *head, n_ref, self._p(xr), self._p(wd), n_cand, self._p(xc),
                C.c_void_p(0) if match is None else C.c_void_p(match.ctypes.data),
                C.c_void_p(0) if md is None else self._p(md), int(r), int(size),
                min(PREDICT_CHUNK, 2048), *scs), pre + "begin")
            picks = C.c_void_p(0)
            _hip.check(getattr(self.lib, pre + "picks")(*dims, *scs, C.byref(picks)), pre + "picks")
            self._sel = dict(dims=dims, scratch=self._scratch, scs=scs, pre=pre, m=m, n_ref=n_ref, n_cand=n_cand, size=int(size),
                             r=int(r), step=0, picks=picks.value, keep=(xr, xc, wd, md, state))

    def select_rows(self):
        """(q_local, n_cand) float64 DEVICE tensor: R_k(c) of the model conditioned on the picks made so far"""
        sel, torch = self._sel, self.torch
        with torch.cuda.device(self.device):
            out = torch.empty((self.q_local, sel['n_cand']), dtype=torch.float64, device=self.device)
            _hip.check(getattr(self.lib, sel['pre'] + "state")(self._stream(), *sel['dims'], 0, *sel['scs'], self._p(out)),
                       sel['pre'] + "state")
            return out

    def _select_condition(self, sel, pick_ptr):
        view = (sel['m'],) if sel['m'] else ()
        _hip.check(getattr(self.lib, sel['pre'] + "condition")(
            self._stream(), self.dtype, self.kernel_id, self.n, self.d, self.p, self.q_local, self._p(self.theta_dev), *view,
            sel['n_ref'], sel['n_cand'], sel['size'], sel['r'], sel['step'], C.c_void_p(pick_ptr), *sel['scs']),
            sel['pre'] + "condition")
        sel['step'] += 1

    def select_condition(self, j):
        """conditions the state on r runs at candidate j (a host int: the pick all ranks agreed on)"""
        sel, torch = self._sel, self.torch
        with torch.cuda.device(self.device):
            jd = torch.full((1,), int(j), dtype=torch.int32, device=self.device)
            self._select_condition(sel, jd.data_ptr())

    # (the view's selection lives in the same scratch and the same state record: these carry on whichever began)
    def condition_select_rows(self):
        """select_rows of a selection begun by condition_select_begin"""
        return self.select_rows()

    def condition_select_condition(self, j):
        """select_condition of a selection begun by condition_select_begin"""
        return self.select_condition(j)

    def select_batch_block(self, x_cand_s, x_ref_s, w, match, r, size, omega):
        return self._select_batch_block(None, x_cand_s, x_ref_s, w, match, r, size, omega)

    def condition_select_batch_block(self, state, x_cand_s, x_ref_s, w, match, r, size, omega):
        """select_batch_block on the view `state` (condition_begin)"""
        return self._select_batch_block(state, x_cand_s, x_ref_s, w, match, r, size, omega)

    def _select_batch_block(self, state, x_cand_s, x_ref_s, w, match, r, size, omega):
        """The whole greedy loop on the device for the engine's components (one rank holds them all): returns DEVICE tensors
        idx (size,) int32 and scores (size, n_cand) float64, row t = sum_k omega_k R_k^t, -inf at candidates picked before step t.
        All steps are enqueued without a host synchronisation (the kernels read each pick from device memory)."""
        torch = self.torch
        self._select_begin(state, x_cand_s, x_ref_s, w, match, r, size)
        sel = self._sel
        with torch.cuda.device(self.device):
            om = torch.as_tensor(np.ascontiguousarray(omega, np.float64)).to(self.device)
            scores = torch.empty((sel['size'], sel['n_cand']), dtype=torch.float64, device=self.device)
            st, score = self._stream(), getattr(self.lib, sel['pre'] + "score")
            for t in range(sel['size']):
                _hip.check(score(st, *sel['dims'], t, self._p(om), *sel['scs'],
                                 C.c_void_p(scores.data_ptr() + 8 * t * sel['n_cand'])), sel['pre'] + "score")
                if t + 1 < sel['size']:
                    self._select_condition(sel, sel['picks'] + 4 * t)
            idx = torch.empty(sel['size'], dtype=torch.int32, device=self.device)
            idx.copy_(self._select_picks_view(sel))
            self._sel = None
            return idx, scores

    def _select_picks_view(self, sel):
        """the picks word array of the scratch as an int32 view"""
        off = sel['picks'] - sel['scratch'].data_ptr()
        return sel['scratch'][off:off + 4 * sel['size']].view(self.torch.int32)

    # ------------------------------------------------------------------------------------------------
    # exact Hessian of the objective in the parameters (lcgp_hip.h: lcgp_nll_hess)
    def nll_hess_block(self):
        """(q_local, (d + 2)^2 + (d + 2) p + p^2) float64 DEVICE tensor: per local component the kernel block, the kernel x built
        noise block and the component's share of the built noise block of the Hessian of the objective in the CONSTRAINED
        parameters (lcgp_nll_hess), from the factorisation of the last evaluate() -- which it only reads.  float64 engines only.
        The scratch holds (d + 4) npad^2 doubles per component processed at once: the local components go in groups as large
        as the free device memory allows (results are bitwise independent of the grouping); raises ValueError when even one
        component does not fit."""
        torch = self.torch
        if self._theta_last is None:
            raise RuntimeError("loss_hessian() needs a preceding evaluate() at the current parameters")
        if self.dtype != _hip.F64:
            raise RuntimeError("the Hessian of the objective is float64 only: evaluate on a float64 engine")
        with torch.cuda.device(self.device):
            width = self.lib.lcgp_nll_hess_width(self.d, self.p)
            group, nbytes = self._fit_group("lcgp_nll_hess_scratch_bytes", self.dtype, self.n, self.d, self.p, None)
            scp = self._p(self._grow_scratch(nbytes, ("the Hessian of the objective", "%d matrices of n x n per component"
                                                      % (self.d + 4), "use fewer training inputs per GPU")))
            out = torch.empty((self.q_local, width), dtype=torch.float64, device=self.device)
            head = self._head(Y=True)
            for k0 in range(0, self.q_local, group):
                _hip.check(self.lib.lcgp_nll_hess(*head, k0, min(group, self.q_local - k0), scp, self._p(out)), "lcgp_nll_hess")
            return out

    def fetch_vector(self, which, k):
        torch = self.torch
        with torch.cuda.device(self.device):
            out = torch.empty(self.n, dtype=self.tdtype, device=self.device)
            _hip.check(self.lib.lcgp_fetch_vector(self._stream(), self.dtype, self.n, self.d, self.p, self.q_local,
                                                  self._p(self.workspace), int(which), int(k), self._p(out)),
                       "lcgp_fetch_vector")
            return out.cpu().numpy().astype(np.float64)

    def fetch_matrix(self, which, k):
        torch = self.torch
        with torch.cuda.device(self.device):
            out = torch.empty((self.n, self.n), dtype=self.tdtype, device=self.device)
            _hip.check(self.lib.lcgp_fetch_matrix(self._stream(), self.dtype, self.n, self.d, self.p, self.q_local,
                                                  self._p(self.workspace), int(which), int(k), self._p(out)),
                       "lcgp_fetch_matrix")
            return out.cpu().numpy().astype(np.float64)


def matern32_device(x1, x2, ell, scale, nug, same, dtype="float64", kernel="matern32"):
    """covmat.py:31-55 on the GPU: returns the (n1, n2) matrix as a numpy float64 array (kernel = "se" / "matern52":
    the squared-exponential and Matern-5/2 product kernels with the same scale / nugget structure, extensions the reference does
    not have)."""
    import torch
    _hip.require_gpu()
    lib = _hip.load()
    dt = _DT[dtype]
    tdt = torch.float64 if dt == _hip.F64 else torch.float32
    dev = torch.device("cuda", torch.cuda.current_device())
    a = torch.as_tensor(np.ascontiguousarray(x1, np.float64)).to(dev, tdt).contiguous()
    b = torch.as_tensor(np.ascontiguousarray(x2, np.float64)).to(dev, tdt).contiguous()
    n1, d = a.shape
    n2 = b.shape[0]
    out = torch.empty((n1, n2), dtype=tdt, device=dev)
    ell = np.ascontiguousarray(ell, np.float64)
    _hip.check(lib.lcgp_covmat(C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), dt, _hip.KERNELS[kernel], n1, n2, d,
                                 C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()),
                                 ell.ctypes.data_as(C.POINTER(C.c_double)), float(scale), float(nug), int(bool(same)),
                                 C.c_void_p(out.data_ptr())), "lcgp_covmat")
    return out.cpu().numpy().astype(np.float64)


def calib_rows_device(blk, jac, M, b, c0, lognorm, inv_range=None, want_sens=False):
    """lcgp_calib_rows on the device that holds `blk`: blk (2, q, n0) float64 DEVICE tensor [ghat; gvar] of ALL q components (a
    block of predict_block / predict_grad_block, read in place), jac (2, q, n0, d) = [dghat; dgvar] or None (no gradient),
    M (q, q), b (q,) and inv_range (d,) float64 tensors on the same device.  Returns device tensors (ll (n0,), dll (n0, d) or
    None, sens (2, q, n0) or None).  One launch; there is no torch formulation behind it."""
    import torch
    _hip.require_gpu()
    lib = _hip.load()
    dev = blk.device
    assert blk.dtype == torch.float64 and blk.is_contiguous() and blk.dim() == 3 and blk.shape[0] == 2
    _, q, n0 = blk.shape
    d = 1 if jac is None else int(jac.shape[3])
    assert jac is None or (jac.dtype == torch.float64 and jac.is_contiguous() and tuple(jac.shape) == (2, q, n0, d))
    assert M.is_contiguous() and tuple(M.shape) == (q, q) and tuple(b.shape) == (q,)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())   # noqa: E731
    with torch.cuda.device(dev):
        ll = torch.empty(n0, dtype=torch.float64, device=dev)
        dll = None if jac is None else torch.empty((n0, d), dtype=torch.float64, device=dev)
        sens = torch.empty((2, q, n0), dtype=torch.float64, device=dev) if want_sens else None
        _hip.check(lib.lcgp_calib_rows(C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), q, d, n0, p(blk[0]), p(blk[1]),
                                       p(None if jac is None else jac[0]), p(None if jac is None else jac[1]), n0, p(M), p(b),
                                       float(c0), float(lognorm), p(inv_range), p(ll), p(dll), p(sens)), "lcgp_calib_rows")
    return ll, dll, sens


def calib_hess_rows_device(blk, jac, hess, M, b, c0, lognorm, inv_range=None, want_sens=False, want_B=False):
    """lcgp_calib_hess_rows on the device that holds `blk`: blk (2, q, n0), jac (2, q, n0, d) and hess (2, q, n0, d (d + 1) / 2)
    = [d2ghat; d2gvar] (packed lower triangles) float64 DEVICE tensors of ALL q components (the blocks of predict_hess_block,
    read in place), M (q, q), b (q,) and inv_range (d,) float64 tensors on the same device.  Returns device tensors (ll (n0,),
    dll (n0, d), d2ll (n0, d (d + 1) / 2) packed, sens (2, q, n0) or None, B (n0, q, q) or None).  ll, dll and sens are bitwise
    calib_rows_device's.  Two launches; there is no torch formulation behind it."""
    import torch
    _hip.require_gpu()
    lib = _hip.load()
    dev = blk.device
    assert blk.dtype == torch.float64 and blk.is_contiguous() and blk.dim() == 3 and blk.shape[0] == 2
    _, q, n0 = blk.shape
    d = int(jac.shape[3])
    tri = d * (d + 1) // 2
    assert jac.dtype == torch.float64 and jac.is_contiguous() and tuple(jac.shape) == (2, q, n0, d)
    assert hess.dtype == torch.float64 and hess.is_contiguous() and tuple(hess.shape) == (2, q, n0, tri)
    assert M.is_contiguous() and tuple(M.shape) == (q, q) and tuple(b.shape) == (q,)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())   # noqa: E731
    with torch.cuda.device(dev):
        ll = torch.empty(n0, dtype=torch.float64, device=dev)
        dll = torch.empty((n0, d), dtype=torch.float64, device=dev)
        d2ll = torch.empty((n0, tri), dtype=torch.float64, device=dev)
        sens = torch.empty((2, q, n0), dtype=torch.float64, device=dev) if want_sens else None
        B = torch.empty((n0, q, q), dtype=torch.float64, device=dev) if want_B else None
        _hip.check(lib.lcgp_calib_hess_rows(C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), q, d, n0, p(blk[0]), p(blk[1]),
                                            p(jac[0]), p(jac[1]), p(hess[0]), p(hess[1]), n0, p(M), p(b), float(c0),
                                            float(lognorm), p(inv_range), p(ll), p(dll), p(d2ll), p(sens), p(B)),
                   "lcgp_calib_hess_rows")
    return ll, dll, d2ll, sens, B
