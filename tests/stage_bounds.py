"""Stage-wise componentwise error bounds of the hot path (build, Cholesky, L^-1, A^-1, z, outputs, predict), of the
joint path (cross covariance X, U = X W^T, Sigma + tau I, its factor, the draws) and of the post-fit queries (V = U W and
the input gradients of lcgp_predict_grad, leave-one-out, the k-fold gather / factor / inverse / apply, the integrated
variance reduction) and of the conditioned view (lcgp_condition_prepare / lcgp_condition_predict: S and its factor, the dense
L_S^-1, v, Sigma_0n, T and the corrected outputs) and of the two second-order input queries (lcgp_predict_hess: DX, P = DX W^T,
the packed Hessians; lcgp_predict_gradcov: dghat, Gamma and its weighted sum M) and of the box-averaged predictions
(lcgp_predict_marginal / lcgp_condition_predict_marginal: the table of 1-D averages against mpmath, the masked rows, the outputs
with the averaged prior, the view's stages and gcov) and of the two parameter-space queries (lcgp_nll_hess: xs and the two
closed-form vectors, the mirrored A^-1 with G_scale and G_nug, d_iA, y_i, G_i, the trace partials, the contraction slots, u_i / dot
/ YP / Q, the three output blocks; lcgp_predict_paramgrad: y_j, T, the row dots, the 3 d + 8 row sums, YT and V YT, the three
outputs -- with hess_layout / pgrad_layout restating the scratch layouts) and of the Sobol pair and subset passes (lcgp_sobol_pairs,
lcgp_sobol_subset_pairs: the table and the box means, every element on its own against mpmath through one-hot weights, every tile
sum, the rows of every batch and the reduction; lcgp_sobol_matrix_pairs with A^-1 as the weight matrix and the S0 column;
lcgp_condition_sobol_matrix_pairs: P, the lower tiles of E = P P^T, then the tiles with Q' = E + D A^-1 -- sobol_layout /
sobol_subset_layout / cond_sobol_layout restating the scratch; float64 only, in numpy on the host: its references are mpmath and
tests/sobol_ref.py).

Every check compares one stage of the library with a plain float64 reference computed from THE LIBRARY'S OWN INPUT TO THAT
STAGE (the fetched A for the Cholesky, the fetched L for L^-1, ...), so no bound carries a condition number.  Entries are
compared one by one (lower triangle for matrices): a wrong 64x64 tile of small far-off-diagonal entries is as visible as a
wrong diagonal one, which a normwise max|error| / max|ref| is not.

Every check returns a `Check`: the worst ratio |error| / bound over the entries (<= 1 passes; NaN counts as inf) and where
it sits -- (row block, column block) of 64 for matrices, (block,) for vectors, the output slot name for scalars.

Constants.  u is the unit roundoff of the stage's storage type (2^-53 float64, 2^-24 float32).  The standard model
fl(a op b) = (a op b)(1 + e), |e| <= u, gives for an inner product of k terms, in ANY summation order (blocked, MFMA,
tree), |fl(x^T y) - x^T y| <= gamma_k |x|^T |y|, gamma_k = k u / (1 - k u) <= 1.01 k u.  The library's error is bounded by
that with one more rounding for the final subtraction / store (k + 1), and the float64 reference computed here from the
fetched quantities commits at most the same again (for float64 stages) or a 2^-29 fraction of it (float32 stages).
Everything below therefore uses C = 4 on top of "k + small": 2 for the library plus the reference, 2 of margin for the
1.01 and the small additive terms.  Every bound also gets an absolute floor FLOOR_K x k x (smallest normal number of the
dtype) for the entries that underflow (C0 cut-off, far tails of L^-1 and A^-1).

The reference never calls the library.  It runs in torch float64 on the device of its inputs: numpy arrays are checked
on the CPU, device tensors on the device (rocBLAS there, not this library's kernels).
"""
from __future__ import annotations

import math
from collections import namedtuple

import mpmath as mp
import numpy as np
import scipy.special
import torch

TS = 64                  # tile size of the library (64 x 64 tiles): locations are reported in these blocks
C = 4.0                  # see the module docstring
FLOOR_K = 4.0
EXP_FLOOR = {"float64": -708.0, "float32": -87.0}     # lcgp_hip.hip exp_floor<T>(): below, C0 is zero for the path

Check = namedtuple("Check", "ratio where")


def dname(dtype) -> str:
    s = str(dtype)
    return "float32" if ("32" in s) else "float64"


def unit(dtype) -> float:
    return 2.0 ** -24 if dname(dtype) == "float32" else 2.0 ** -53


def tiny(dtype) -> float:
    return float(np.finfo(np.float32 if dname(dtype) == "float32" else np.float64).tiny)


def floor(dtype, k) -> float:
    """absolute floor for an entry with inner dimension k"""
    return FLOOR_K * max(int(k), 1) * tiny(dtype)


def rounded(a, dtype):
    """a rounded to the storage type (what the library holds after its upload), as float64 numpy"""
    return np.asarray(np.asarray(a, np.float64).astype(np.float32 if dname(dtype) == "float32" else np.float64), np.float64)


def _t(a, device=None):
    if isinstance(a, torch.Tensor):
        return a.to(device if device is not None else a.device, torch.float64)
    return torch.as_tensor(np.asarray(a, np.float64), device=device)


def _dev(*xs):
    for a in xs:
        if isinstance(a, torch.Tensor):
            return a.device
    return torch.device("cpu")


def worst(err, bound, lower=True) -> Check:
    """max over the entries of err / bound (lower triangle of a matrix when `lower`), with its 64-block location"""
    r = err / bound
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    if r.dim() == 2 and lower:
        r = torch.tril(r)
    if r.numel() == 0:
        return Check(0.0, ())
    idx = int(torch.argmax(r))
    if r.dim() == 2:
        i, j = divmod(idx, r.shape[1])
        return Check(float(r.view(-1)[idx]), (i // TS, j // TS))
    return Check(float(r.view(-1)[idx]), (idx // TS,))


def combine(*checks) -> Check:
    return max(checks, key=lambda c: c.ratio)


# ----------------------------------------------------------------------------------------------------------------------
# covariance pieces in float64
# ----------------------------------------------------------------------------------------------------------------------
KERNEL_NAMES = ("matern32", "se", "matern52")


def _known(kernel):
    if kernel not in KERNEL_NAMES:
        raise ValueError("unknown covariance kernel %r (one of %s)" % (kernel, ", ".join(KERNEL_NAMES)))


def kernel_parts(x1, x2, ell, kernel, dtype, device=None):
    """C0 (n1 x n2) of the latent kernel in float64 from the ROUNDED inputs, the error magnification E of its evaluation in
    the storage type, the mask of the entries past the library's C0 cut-off, and the lengthscale derivative factors
    F_l = ell_l dC0/d ell_l (a list of d matrices, computed lazily by `dC0`).

    E (units of u): the library stores x / ell rounded (|dS_l| <= u (|x1_l| + |x2_l|) / ell_l + u S_l), accumulates the
    exponent in the storage type (d - 1 roundings of a sum bounded by its absolute value) and evaluates exp with an
    error of at most one rounding of its argument's product with log2(e) plus one ulp (the float32 __expf: the sum-S term
    accounts for it) and the Matern polynomial with d fused multiply-adds.
      Matern32: d ln C0 / d S_l = -S_l / (1 + S_l), |.| <= 1:
          E = sum_l (|x1_l| + |x2_l|) / ell_l + (d + 1) sum_l S_l + d + 3
      SE: d ln C0 / d S_l = -S_l:
          E = sum_l S_l ((|x1_l| + |x2_l|) / ell_l + S_l) + (d + 1) 1/2 sum_l S_l^2 + 3
      Matern52: C0 = prod_l f(S_l) exp(-sum_l S_l), f(S) = 1 + S + S^2 / 3; d ln C0 / d S_l = -S_l (1 + S_l) / (3 f(S_l)),
      |.| = w(S_l) < 1, so the input and the exponent terms are those of Matern32 and the cut-off is the same (the exponent
      is sum S).  The polynomial: per dimension build_kernel does m52_fm1 = fma(sd * (1/3), sd, sd), then poly = fma(poly,
      fm1, poly).  Recounted from the code that is FOUR sources of error per dimension, not three: the constant 1/3 rounded
      to the storage type (u / 2 in both types), the product sd * (1/3), the inner fma, the outer fma.  The first two act on
      a = S^2 / 3 alone, the third on f - 1 = a + S, the fourth on the running product: relative to f they weigh
      1 + (2.5 a + S) / f(S) -- below 3 for S <= 7.5, and below 3.5 always.  The half beyond 3 is covered by the input term:
      it is counted with weight 1 where its true weight is w(S_l), and (1 - w(S)) 2 S = 2 S (3 + 2 S) / (3 f(S)) >= 3.3
      from S = 7.5 on (m_l >= S_l).  So three per dimension stand, where Matern32 has one:
          E = sum_l (|x1_l| + |x2_l|) / ell_l + (d + 1) sum_l S_l + 3 d + 3
      (cross_kernel, pgrad_kernel and the others evaluate the same two fmas per dimension in double.)
    Any other kernel name is a ValueError: no branch stands for "some Matern".
    """
    _known(kernel)
    dev = device if device is not None else _dev(x1, x2)
    a = _t(x1, dev)
    b = _t(x2, dev)
    ell = np.asarray(ell, np.float64)
    d = a.shape[1]
    ssum = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float64, device=dev)
    poly = torch.ones_like(ssum)
    mag = torch.zeros_like(ssum)
    for l in range(d):
        xa = a[:, l] / ell[l]
        xb = b[:, l] / ell[l]
        s = (xa[:, None] - xb[None, :]).abs()
        m = xa.abs()[:, None] + xb.abs()[None, :]
        if kernel == "se":
            ssum += 0.5 * s * s
            mag += s * (m + s)
        elif kernel == "matern32":
            ssum += s
            poly *= 1.0 + s
            mag += m
        elif kernel == "matern52":
            ssum += s
            poly *= 1.0 + s + s * s / 3.0
            mag += m
    if kernel == "se":
        c0 = torch.exp(-ssum)
        e = mag + (d + 1) * ssum + 3.0
    elif kernel == "matern32":
        c0 = poly * torch.exp(-ssum)
        e = mag + (d + 1) * ssum + d + 3.0
    elif kernel == "matern52":
        c0 = poly * torch.exp(-ssum)
        e = mag + (d + 1) * ssum + 3.0 * d + 3.0
    cut = ssum > -EXP_FLOOR[dname(dtype)]
    return c0, e, cut


def dC0(x1, x2, ell, kernel, device=None):
    """ell_l d C0 / d ell_l for every l (Matern32: C0 S_l^2 / (1 + S_l); SE: C0 S_l^2; Matern52: C0 S_l^2 (1 + S_l) /
    (3 f(S_l)), f(S) = 1 + S + S^2 / 3), float64.  This is the reference's own form: a product, a sum and a quotient on top
    of C0 in every kernel.  The library never divides in its narrow kernels: for Matern52 it forms m52_wl(S_l) = (S_l S_l)
    fma(S_l, 1/3, 1/3) (three roundings) times the product of the other dimensions' f (check_outputs counts them)."""
    _known(kernel)
    dev = device if device is not None else _dev(x1, x2)
    a, b = _t(x1, dev), _t(x2, dev)
    ell = np.asarray(ell, np.float64)
    c0 = kernel_parts(a, b, ell, kernel, "float64", dev)[0]
    out = []
    for l in range(a.shape[1]):
        s = (a[:, l][:, None] / ell[l] - b[:, l][None, :] / ell[l]).abs()
        if kernel == "se":
            out.append(c0 * s * s)
        elif kernel == "matern32":
            out.append(c0 * s * s / (1.0 + s))
        elif kernel == "matern52":
            out.append(c0 * s * s * (1.0 + s) / (3.0 + 3.0 * s + s * s))
    return out


def split_theta(th, d):
    th = np.asarray(th, np.float64)
    ell, scale, nug, D = th[:d], float(th[d]), float(th[d + 1]), float(th[d + 2])
    return ell, scale, nug, D, th[d + 3:]


# ----------------------------------------------------------------------------------------------------------------------
# stage checks
# ----------------------------------------------------------------------------------------------------------------------
def reference_A(x, sr, th, kernel, dtype, device=None):
    """A = I + D (C o sr sr^T) in float64 from the dtype-rounded x, sr (theta is float64 in both precisions)"""
    d = np.asarray(x).shape[1]
    ell, scale, nug, D, _ = split_theta(th, d)
    c0, e, cut = kernel_parts(rounded(x, dtype), rounded(x, dtype), ell, kernel, dtype, device)
    dev = c0.device
    n = c0.shape[0]
    s = _t(rounded(np.ones(n) if sr is None else sr, dtype), dev)
    ss = s[:, None] * s[None, :]
    nt = nug / (1.0 + nug)
    eye = torch.eye(n, dtype=torch.float64, device=dev)
    a = eye + D * scale * ss * ((1.0 - nt) * c0 + nt * eye)
    return a, e, cut, ss


def check_build(A, b, x, Y, sr, th, kernel, dtype) -> Check:
    """A (the fetched matrix after lcgp_kernel_build) and b (fetch_vector 0) against their float64 definitions.

    off the diagonal A_ij = ss_ij c_off C0_ij with c_off = D scale (1 - nt) rounded: relative error (E + 4) u (E of
    kernel_parts; c_off, ss_ij and two products: four roundings).  The diagonal adds 1 + (c_diag - 1) ss_ii with
    c_diag = 1 + D scale nt rounded: absolute error u ((1 + D scale nt) ss_ii + |A_ii|) -- the issue's bound
    c (d + 3 + sum S) u |A_ij - delta_ij| misses exactly this term (it is not relative to A_ii - 1).  Past the C0 cut-off
    (exponent below exp_floor) the library may return any value in [0, C0]: the bound there is |A_ij - delta_ij| itself.
    b_i = sum_a Y_ai psi_a is accumulated in float64 and rounded once to storage: C p u64 (|Y|^T |psi|)_i + 2 u |b_i|
    (the rounding to storage, with the margin factor 2 the other bounds carry in C).  b = None checks A alone (the
    stand-alone lcgp_kernel_build, which has no Y, does not form b).
    """
    dev = _dev(A, b)
    d = np.asarray(x).shape[1]
    u = unit(dtype)
    ell, scale, nug, D, psi = split_theta(th, d)
    aref, e, cut, ss = reference_A(x, sr, th, kernel, dtype, dev)
    n = aref.shape[0]
    eye = torch.eye(n, dtype=torch.float64, device=dev)
    off = (aref - eye).abs()
    nt = nug / (1.0 + nug)
    bound = C * (e + 4.0) * u * off + floor(dtype, d)
    bound = bound + torch.where(cut, off, torch.zeros_like(off))
    bound = bound + torch.diag(C * u * ((1.0 + abs(D * scale * nt)) * torch.diagonal(ss) + torch.diagonal(aref).abs()))
    ca = worst((_t(A, dev) - aref).abs(), bound)
    if b is None:
        return ca
    yr = _t(rounded(Y, dtype), dev)
    ps = _t(psi, dev)
    bref = yr.T @ ps
    bb = C * yr.shape[0] * unit("float64") * (yr.abs().T @ ps.abs()) + 2.0 * u * bref.abs() + floor(dtype, 1)
    cb = worst((_t(b, dev) - bref).abs(), bb)
    return combine(ca, cb)


def check_cholesky(A, L, dtype) -> Check:
    """|A - L L^T|_ij <= C (min(i, j) + 2) u (|L| |L^T|)_ij: the componentwise backward error of any Cholesky variant
    (blocked, right- or left-looking, MFMA) -- k = min(i, j) + 1 products plus the subtraction; independent of kappa(A)."""
    dev = _dev(A, L)
    a = _t(A, dev)
    l = torch.tril(_t(L, dev))
    n = a.shape[0]
    r = (a - l @ l.T).abs()
    idx = torch.arange(n, device=dev, dtype=torch.float64)
    k = torch.minimum(idx[:, None], idx[None, :]) + 2.0
    la = l.abs()
    return worst(r, C * k * unit(dtype) * (la @ la.T) + floor(dtype, n))


def check_cholesky_inverse_solve(A, L, dtype) -> Check:
    """check_cholesky's residual bound plus the error of the library's panel solve, which is NOT a substitution: the
    64-column panel tile is L_rc = A'_rc W_cc^T, a product with the explicit inverse W_cc of the diagonal block (chain_step,
    DESIGN.md).  With the residual |W_cc L_cc - I| <= c TS u |W_cc| |L_cc| of the inverse, the tile's residual is
        A'_rc - L_rc L_cc^T = A'_rc (I - W_cc L_cc)^T - E L_cc^T,   |E| <= TS u |A'_rc| |W_cc|^T,
    and with |A'_rc| <= |L_rc| |L_cc|^T (to first order) both terms are within
        C TS u |L_rc| (|L_cc|^T |W_cc|^T |L_cc|^T)        (entries of the strictly lower tiles (r, c), r > c)
    on top of check_cholesky's bound, which still covers the trailing updates and the diagonal blocks.  The new term is of
    the size of check_cholesky's when L_cc is well conditioned and grows with the componentwise condition of L_cc
    otherwise: a substitution would not have it (check_cholesky then holds independently of kappa), this product does --
    an ill-conditioned Sigma (a smooth prior over many new inputs, little data) exceeds check_cholesky's bound, this one
    not.  W_cc is the float64 inverse of the fetched diagonal block."""
    dev = _dev(A, L)
    a = _t(A, dev)
    l = torch.tril(_t(L, dev))
    r = (a - l @ l.T).abs()
    return worst(r, inverse_solve_bound(l, dtype))


def inverse_solve_bound(l, dtype):
    """the bound of check_cholesky_inverse_solve on |A - L L^T| (n x n float64 tensor) from the factor alone: l is the lower
    triangle of the fetched factor, float64.  check_cond_s adds it to the bound of the matrix the factor is held to."""
    dev = l.device
    n = l.shape[0]
    u = unit(dtype)
    idx = torch.arange(n, device=dev, dtype=torch.float64)
    k = torch.minimum(idx[:, None], idx[None, :]) + 2.0
    la = l.abs()
    bound = C * k * u * (la @ la.T) + floor(dtype, n)
    extra = torch.zeros_like(bound)
    for c in range(0, n, TS):
        e = min(c + TS, n)
        if e >= n:
            break
        lcc = l[c:e, c:e]
        wcc = torch.linalg.solve_triangular(lcc, torch.eye(e - c, dtype=torch.float64, device=dev), upper=False)
        m = lcc.abs().T @ wcc.abs().T @ lcc.abs().T
        extra[e:, c:e] = C * TS * u * (la[e:, c:e] @ m)
    return bound + extra


def check_half_logdet(L, half_logdet, dtype) -> Check:
    """half_logdet (the library sums 1/2 log(pivot) in float64) against fsum(log L_ii) of the fetched factor:
    C u (n sum |log L_ii| + n).  The second term is the rounding of each stored L_ii = sqrt(pivot): an absolute error of
    u in log L_ii however close L_ii is to 1 (the issue's c n u sum |log L_ii| alone misses it for A near I)."""
    dg = torch.diagonal(_t(L)).cpu().numpy()
    n = dg.size
    lg = np.log(dg)
    ref = math.fsum(lg)
    bound = C * unit(dtype) * (n * float(np.sum(np.abs(lg))) + n) + floor(dtype, n)
    r = abs(float(half_logdet) - ref) / bound
    return Check(r if np.isfinite(r) else math.inf, ("half_logdet",))


def check_inverse_factor(L, W, dtype) -> Check:
    """W = L^-1 against solve_triangular(L, I) in float64: 2 C n u (|W| |L| |W|)_ij.  Any method whose residual satisfies
    |W L - I| <= c n u |W| |L| (or |L W - I| <= c n u |L| |W|) has W - L^-1 = (W L - I) L^-1, so this forward bound holds
    for every blocked / level-parallel variant; the factor 2 covers W vs L^-1 on the right and the reference's own solve."""
    dev = _dev(L, W)
    l = torch.tril(_t(L, dev))
    n = l.shape[0]
    eye = torch.eye(n, dtype=torch.float64, device=dev)
    wref = torch.linalg.solve_triangular(l, eye, upper=False)
    wa = wref.abs()
    bound = 2.0 * C * n * unit(dtype) * (wa @ (l.abs() @ wa)) + floor(dtype, n)
    return worst((torch.tril(_t(W, dev)) - wref).abs(), bound)


def check_inverse(W, V, dtype) -> Check:
    """A^-1 = W^T W (lower triangle) against the float64 product of the fetched W: entry (i, j), i >= j, is an inner
    product over k = i .. n-1, i.e. n - max(i, j) terms: C (n - max(i, j) + 2) u (|W|^T |W|)_ij"""
    dev = _dev(W, V)
    w = torch.tril(_t(W, dev))
    n = w.shape[0]
    vref = w.T @ w
    idx = torch.arange(n, device=dev, dtype=torch.float64)
    k = n - torch.maximum(idx[:, None], idx[None, :]) + 2.0
    wa = w.abs()
    return worst((_t(V, dev) - vref).abs(), C * k * unit(dtype) * (wa.T @ wa) + floor(dtype, n))


def check_z(V, b, z, dtype) -> Check:
    """z = A^-1 b against V b (V symmetric, as fetched): C n u (|V| |b|) + 2 u |z| (the last term: rounding to storage)"""
    dev = _dev(V, b, z)
    v, bb = _t(V, dev), _t(b, dev)
    zref = v @ bb
    n = zref.shape[0]
    bound = C * n * unit(dtype) * (v.abs() @ bb.abs()) + 2.0 * unit(dtype) * zref.abs() + floor(dtype, n)
    return worst((_t(z, dev) - zref).abs(), bound)


def reference_outputs(x, Y, sr, th, V, b, z, kernel, dtype):
    """(ref, bound) float64 tensors over the output row [quad, g_ell_0 .. g_ell_{d-1}, g_scale, g_nug, gsig_0 .. gsig_{p-1}]
    from the library's V, b, z and the float64 kernel of the rounded x (see check_outputs)."""
    dev = _dev(V, b, z)
    d = np.asarray(x).shape[1]
    u = unit("float64")               # the contraction runs in float64 in both precisions (check_outputs)
    ell, scale, nug, D, psi = split_theta(th, d)
    xr = rounded(x, dtype)
    c0, e, cut = kernel_parts(xr, xr, ell, kernel, "float64", dev)
    n = c0.shape[0]
    s = _t(rounded(np.ones(n) if sr is None else sr, dtype), dev)
    ss = s[:, None] * s[None, :]
    nt = nug / (1.0 + nug)
    v, bb, zz = _t(V, dev), _t(b, dev), _t(z, dev)
    yr = _t(rounded(Y, dtype), dev)
    eye = torch.eye(n, dtype=torch.float64, device=dev)
    G = ss * (0.5 * D * v - 0.5 * zz[:, None] * zz[None, :])
    Ga = ss * (0.5 * abs(D) * v.abs() + 0.5 * zz.abs()[:, None] * zz.abs()[None, :])
    wgt = C * u * (n + d + e)
    fl = floor("float64", n)
    ref, bnd = [], []
    if dname(dtype) == "float32":
        # quad = D b^T (C o ss) z, gsig = D Y (C o ss) z: the cancellation-free forms the float32 path evaluates
        cm = ss * scale * ((1.0 - nt) * c0 + nt * eye)
        cz = cm @ zz
        cz_b = (wgt * cm.abs()) @ zz.abs()
        ref.append(D * torch.dot(bb, cz))
        bnd.append(abs(D) * torch.dot(bb.abs(), cz_b) + fl)
        gs_ref, gs_bnd = D * (yr @ cz), abs(D) * (yr.abs() @ cz_b) + fl
    else:
        ref.append(torch.dot(bb, bb - zz))
        bnd.append(C * n * u * torch.dot(bb.abs(), bb.abs() + zz.abs()) + fl)
        gs_ref = yr @ (bb - zz)
        gs_bnd = C * n * u * (yr.abs() @ (bb.abs() + zz.abs())) + fl
    for l, f in enumerate(dC0(xr, xr, ell, kernel, dev)):
        k = scale * (1.0 - nt) / ell[l]
        ref.append(k * (G * f).sum())
        bnd.append(abs(k) * (wgt * Ga * f).sum() + fl)
    sc0, trg = (G * c0).sum(), torch.trace(G)
    asc0, atrg = (wgt * Ga * c0).sum(), torch.trace(wgt * Ga)
    ref.append((1.0 - nt) * sc0 + nt * trg)
    bnd.append((1.0 - nt) * asc0 + nt * atrg + fl)
    ref.append(scale * (trg - sc0) / (1.0 + nug) ** 2)
    bnd.append(abs(scale) * (atrg + asc0) / (1.0 + nug) ** 2 + fl)
    ref = torch.cat([torch.stack(ref), gs_ref])
    bnd = torch.cat([torch.stack(bnd), gs_bnd])
    return ref, bnd


def output_names(d, p):
    return ["quad"] + ["g_ell%d" % l for l in range(d)] + ["g_scale", "g_nug"] + ["gsig%d" % a for a in range(p)]


def check_outputs(out_row, x, Y, sr, th, V, b, z, kernel, dtype) -> Check:
    """quad, gradients and gsig of one output row against the float64 contraction of the library's own V, b, z.

    Precision.  In BOTH storage types the library does this stage in float64: grad_kernel / grad_kernel_wide convert the
    stored x, sr, z and V to double, form x / ell, G, C0 and dC0 in double and accumulate in double; the c = (C o ss) z
    partials of float32, cvec_reduce_kernel, gsig_c_kernel, gsig_body and finalize_kernel are double as well.  The only
    float32 roundings are those of the stored inputs, and the reference uses exactly those (the fetched V, b, z and the
    rounded x, Y, sr).  So u is the float64 unit roundoff here whatever the storage type, E is kernel_parts' float64
    magnification and the floor is float64's.

    Gradients: G = ss o (D/2 V - z z^T / 2) contracted with dC/dtheta (formulas of finalize_kernel): each term carries
    (n + d + E_ij) u relative to |G|-with-absolute-values Ga = ss o (|D|/2 |V| + |z| |z|^T / 2) times |dC| (n: the
    reduction over the tiles, d: the dimensions, E: the kernel evaluation).  The d dimensions cover both forms of
    C0 S_l^2 / (1 + S_l): grad_kernel's prefix / suffix products (d - 1 products) and grad_kernel_wide's prod / (1 + S_l)
    (d products, the sum 1 + S_l and the quotient: d + 2 roundings, within d + E since E >= d + 3).  Matern52, C0 S_l^2
    (1 + S_l) / (3 f(S_l)) = exp(-sum S) m52_wl(S_l) prod_{i != l} f(S_i): m52_wl = (S S) fma(S, 1/3, 1/3) costs three
    roundings (the square, the fma, the product; the two constants 1/3 half a rounding each); every factor f(S_i) of a
    prefix / suffix product costs three (kernel_parts), so grad_kernel's pre_l suf has 3 (d - 1) and one more for the product
    of the two, and the products with ge and into the accumulator two: 3 d + 3 together, within d + E since E >= 3 d + 3.
    grad_kernel_wide (d > 32 only) has the whole product (3 d), m52_fm1 again (three), the sum 1 + fm1, the quotient, m52_wl
    (three) and the same two products: 3 d + 10, within d + E from d = 7 on, i.e. wherever that kernel runs.  quad and gsig:
    C n u (|b|^T (|b| + |z|)) in float64 storage; in float32 storage the library evaluates D b^T (C o ss) z and D Y (C o ss) z (finalize_kernel /
    gsig_c_kernel, the forms without the cancellation of b - z), bounded the same way as the gradients."""
    d, p = np.asarray(x).shape[1], np.asarray(Y).shape[0]
    ref, bnd = reference_outputs(x, Y, sr, th, V, b, z, kernel, dtype)
    o = np.asarray(out_row, np.float64)
    got = _t(np.concatenate([o[1:2], o[3:]]), ref.device)
    r = (got - ref).abs() / bnd
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    i = int(torch.argmax(r))
    return Check(float(r[i]), (output_names(d, p)[i],))


def check_predict(ghat, gvar, x0, x, sr, th, W, z, kernel, dtype, same=0) -> Check:
    """predictions at x0 against the float64 cross covariance X = scale ((1 - nt) C0(x0, x) + nt I[same]) o sr^T of the
    rounded inputs and the library's W, z:
        ghat = X z             C (n + d + E) u |X| |z|
        gvar = scale - D |W X_i^T|^2     C (n + d + E) u |D| || |W| |X_i| ||^2 + u scale
    `same` as in the C ABI (check_cov_cross): 0 = x0 are new inputs, no nugget term; else x0 row i is x row i + same - 1
    and X carries scale nt sr_j at that column j, two roundings more, within the same relative bound of |X_ij|."""
    dev = _dev(W, z)
    d = np.asarray(x).shape[1]
    u = unit(dtype)
    ell, scale, nug, D, _ = split_theta(th, d)
    nt = nug / (1.0 + nug)
    c0, e, cut = kernel_parts(rounded(x0, dtype), rounded(x, dtype), ell, kernel, dtype, dev)
    n0, n = c0.shape
    s = _t(rounded(np.ones(n) if sr is None else sr, dtype), dev)
    X = scale * (1.0 - nt) * c0 * s[None, :]
    Xa = X.abs() + torch.where(cut, X.abs(), torch.zeros_like(X))
    if same:
        i = torch.arange(n0, device=dev)
        j = i + same - 1
        assert int(j[-1]) < n, (same, n0, n)
        X[i, j] += scale * nt * s[j]
        Xa[i, j] += abs(scale * nt) * s[j].abs()
    wgt = C * u * (n + d + e.max(dim=1).values)
    w = torch.tril(_t(W, dev))
    zz = _t(z, dev)
    gref = X @ zz
    gb = wgt * (Xa @ zz.abs()) + floor(dtype, n)
    U = X @ w.T
    vref = scale - D * (U * U).sum(dim=1)
    Ua = Xa @ w.abs().T
    vb = wgt * abs(D) * (Ua * Ua).sum(dim=1) + u * abs(scale) + floor(dtype, n)
    return combine(worst((_t(ghat, dev) - gref).abs(), gb), worst((_t(gvar, dev) - vref).abs(), vb))


# ----------------------------------------------------------------------------------------------------------------------
# joint covariance over new inputs and correlated draws (lcgp_predict_cov, lcgp_potrf_logdet on the cov workspace,
# lcgp_sample_latent).  The factor of the cov workspace goes through check_cholesky_inverse_solve(Sigma + tau I, L).
# ----------------------------------------------------------------------------------------------------------------------
def _pad128(n) -> int:
    return -(-int(n) // (2 * TS)) * (2 * TS)


def check_cov_cross(X, x0, x, sr, th, kernel, dtype, same=0) -> Check:
    """X_k = scale ((1 - nt) C0(x0, x) + nt I[same]) o sr^T (n0 x n, the first slab of the lcgp_predict_cov scratch) against
    its float64 definition from the rounded x0, x, sr.  `same` as in the C ABI: 0 = no nugget term, else x0 row i is x row
    i + same - 1 and that entry carries scale nt sr.

    cross_kernel forms x / ell, the exponent and the polynomial, scales by scale (1 - nt) and sr and stores once: relative
    error (E + 4) u (E of kernel_parts: the evaluation; then the factors scale (1 - nt), sr and the store), entry by entry
    (C = 4 on top).  A nugget entry adds scale nt sr_j, two roundings more: C u scale nt sr_j.  Past the C0 cut-off the
    library may return any value in [0, C0]: the bound there is |X_ij| itself."""
    dev = _dev(X)
    d = np.asarray(x).shape[1]
    u = unit(dtype)
    ell, scale, nug, D, _ = split_theta(th, d)
    nt = nug / (1.0 + nug)
    c0, e, cut = kernel_parts(rounded(x0, dtype), rounded(x, dtype), ell, kernel, dtype, dev)
    n0, n = c0.shape
    s = _t(rounded(np.ones(n) if sr is None else sr, dtype), dev)
    off = (scale * (1.0 - nt) * c0 * s[None, :]).abs()
    dl = torch.zeros_like(c0)
    if same:
        i = torch.arange(n0, device=dev)
        dl[i, i + same - 1] = 1.0
    ref = scale * ((1.0 - nt) * c0 + nt * dl) * s[None, :]
    bound = C * (e + 4.0) * u * off + C * u * abs(scale * nt) * dl * s[None, :].abs() + floor(dtype, d)
    bound = bound + torch.where(cut, off, torch.zeros_like(off))
    return worst((_t(X, dev) - ref).abs(), bound, lower=False)


def check_cov_u(U, X, W, dtype) -> Check:
    """U_k = X_k W_k^T (n0 x n, the second slab of the scratch) against the float64 product of the library's own X and
    W = L^-1 (lower triangle of the fetched matrix): an inner product of K = npad terms (n rounded up to 128: the padding
    adds stored zeros), C (npad + 2) u (|X| |W|^T)_ij."""
    dev = _dev(U, X, W)
    xx = _t(X, dev)
    w = torch.tril(_t(W, dev))
    k = _pad128(w.shape[0])
    ref = xx @ w.T
    bound = C * (k + 2.0) * unit(dtype) * (xx.abs() @ w.abs().T) + floor(dtype, k)
    return worst((_t(U, dev) - ref).abs(), bound, lower=False)


def check_sigma(S, U, x0, th, jitter, kernel, dtype) -> Check:
    """Sigma_k + tau_k I (the matrix slot of the cov workspace after lcgp_predict_cov, lower triangle) against
    C00 - D U U^T + tau I in float64, built from the library's own U (n0 x n) and the rounded x0; tau = jitter scale.

    C00 = scale ((1 - nt) C0(x0, x0) + nt I) is evaluated like X in check_cov_cross: (E + 4) u relative.  The tile
    kernel accumulates C00_ij - D sum_k U_ik U_jk over K = npad terms in the storage type, alpha = -D_k applied to the
    product: (npad + 2) u (|C00| + |D| |U| |U|^T).  cov_diag_kernel adds tau to the stored diagonal in float64 and stores
    once: u |tau| plus a rounding of the sum, which the previous term covers (|Sigma| <= |C00| + |D| |U| |U|^T).  Together,
    with C = 4:  C (npad + d + E) u (|C00| + |D| |U| |U|^T) + u |tau|, and |C00| itself past the C0 cut-off.  The bound
    starts from the library's U, so no condition number enters."""
    dev = _dev(S, U)
    ell, scale, nug, D, _ = split_theta(th, np.asarray(x0).shape[1])
    ref, bound = sigma_ref_bound(U, x0, th, jitter * scale, kernel, dtype, dev)
    return worst((_t(S, dev) - ref).abs(), bound)


def sigma_ref_bound(U, x0, th, tau, kernel, dtype, dev):
    """(reference, bound) of check_sigma, float64 n0 x n0 tensors: C00 - D U U^T + diag(tau) from the library's own U and the
    rounded x0.  tau: a float (check_sigma's jitter scale) or a vector of n0 diagonal terms (check_cond_s: 1 / (D r_i)), which
    enter the bound as u |tau_i|."""
    d = np.asarray(x0).shape[1]
    u = unit(dtype)
    ell, scale, nug, D, _ = split_theta(th, d)
    nt = nug / (1.0 + nug)
    xr = rounded(x0, dtype)
    c0, e, cut = kernel_parts(xr, xr, ell, kernel, dtype, dev)
    n0 = c0.shape[0]
    uu = _t(U, dev)
    k = _pad128(uu.shape[1])
    eye = torch.eye(n0, dtype=torch.float64, device=dev)
    if not isinstance(tau, float):
        tau = _t(tau, dev)
    c00 = scale * ((1.0 - nt) * c0 + nt * eye)
    ref = c00 - D * (uu @ uu.T) + tau * eye
    ua = uu.abs()
    bound = C * (k + d + e) * u * (c00.abs() + abs(D) * (ua @ ua.T)) + u * abs(tau) * eye + floor(dtype, k)
    bound = bound + torch.where(cut, c00.abs(), torch.zeros_like(c00))
    return ref, bound


def check_draws(out, L, eps, ghat, dtype) -> Check:
    """draws out[s, i] = ghat_i + (L eps_s)_i (S x n0, float64, one component) against the float64 product of the library's
    factor (lower triangle of the fetched matrix), eps rounded to the storage type (the library uploads it so) and the
    library's ghat.  L eps_s is an inner product of at most n0 terms in the storage type, stored once: C (n0 + 1) u
    (|eps| |L|^T); the final add to ghat is float64: C u64 (|ghat| + |L eps|).  Locations are (draw block, input block)."""
    dev = _dev(out, L, ghat)
    l = torch.tril(_t(L, dev))
    n0 = l.shape[0]
    ep = _t(rounded(eps, dtype), dev)
    g = _t(ghat, dev)
    le = ep @ l.T
    ref = g[None, :] + le
    bound = C * (n0 + 1.0) * unit(dtype) * (ep.abs() @ l.abs().T) + C * unit("float64") * (g.abs()[None, :] + le.abs())
    return worst((_t(out, dev) - ref).abs(), bound + floor(dtype, n0), lower=False)


# ----------------------------------------------------------------------------------------------------------------------
# post-fit queries: input gradients of the prediction (lcgp_predict_grad), leave-one-out (lcgp_loo), k-fold cross-validation
# (lcgp_cv_gather -> lcgp_potrf_logdet / lcgp_potri on the fold workspace -> lcgp_cv_apply) and the integrated variance
# reduction (lcgp_variance_reduction_prepare / lcgp_variance_reduction).  The fold factor and inverse go through
# check_cholesky_inverse_solve, check_inverse_factor and check_inverse on the fetched slot.
# ----------------------------------------------------------------------------------------------------------------------
def predict_pad(n0) -> int:
    """rows of the lcgp_predict / lcgp_predict_grad scratch slabs: n0 rounded up to 128, or to 64 below 128"""
    return _pad128(n0) if n0 >= 2 * TS else -(-int(n0) // TS) * TS


def _worst_cols(err, bound, names) -> Check:
    """worst(err / bound) over an (rows x columns) table, located as (row block, column name)"""
    r = err / bound
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    if r.numel() == 0:
        return Check(0.0, ())
    idx = int(torch.argmax(r))
    i, j = divmod(idx, r.shape[1])
    return Check(float(r.view(-1)[idx]), (i // TS, names[j]))


def check_pgrad_v(V, U, W, dtype) -> Check:
    """V_k = U_k W_k (n0 x n; OP_PRED_V, written over the X slabs of the lcgp_predict_grad scratch) against the float64 product
    of the library's own U (the second slabs) and W = L^-1 (lower triangle of the fetched matrix).  Entry (i, j) is an inner
    product over m = j .. npad - 1 (W is lower triangular, the padding adds stored zeros), accumulated in the storage type and
    stored once: C (npad + 2) u (|U| |W|)_ij."""
    dev = _dev(V, U, W)
    uu = _t(U, dev)
    w = torch.tril(_t(W, dev))
    n = w.shape[0]
    k = _pad128(n)
    ref = uu @ w
    bound = C * (k + 2.0) * unit(dtype) * (uu.abs() @ w.abs()) + floor(dtype, k)
    return worst((_t(V, dev)[:, :n] - ref).abs(), bound, lower=False)


def pgrad_h(s, kernel):
    """h_l of check_pgrad from the signed scaled distance s (a float64 tensor): dC0 / dx0_l = -C0 h_l / ell_l"""
    _known(kernel)
    if kernel == "se":
        return s
    if kernel == "matern32":
        return s / (1.0 + s.abs())
    return s * (1.0 + s.abs()) / (3.0 + 3.0 * s.abs() + s * s)


def pgrad_psi(s, kernel):
    """psi = f'' / f of the 1-D factor f at the signed scaled distance s (a float64 tensor): d2 C0 / d x0_l^2 = C0 psi(s_l) /
    ell_l^2 (include/lcgp_hip.h).  Matern-3/2: (|s| - 1) / (1 + |s|), -1 at s = 0 with a kink there; SE: s^2 - 1; Matern-5/2:
    (s^2 - |s| - 1) / (3 + 3 |s| + s^2), -1/3 at s = 0."""
    _known(kernel)
    a = s.abs()
    if kernel == "se":
        return s * s - 1.0
    if kernel == "matern32":
        return (a - 1.0) / (1.0 + a)
    return (s * s - a - 1.0) / (3.0 + 3.0 * a + s * s)


def pgrad_psi_err(s, kernel):
    """(|d psi / d s|, k, abs) of the evaluation of psi in kern_psi, so that |d psi| <= u (|psi'| (m_l + |s|) + k |psi| + abs)
    with m_l = (|x0_il| + |x_jl|) / ell_l and |ds| <= u (m_l + |s|) as in check_pgrad.
      Matern-3/2: (a - 1) fast_rcp(1 + a): psi' = 2 / (1 + a)^2 (<= 2); the difference, the sum, fast_rcp within 2 u and the
        product are five roundings, each relative to psi: k = 5.
      SE: fma(s, s, -1): psi' = 2 s (NOT bounded by 1: the m_l weight is 2 |s|); one rounding: k = 1.
      Matern-5/2: fma(a, a - 1, -1) fast_rcp(fma(a, a + 3, 3)): psi' = 4 a (a + 2) / (3 + 3 a + a^2)^2 (<= 0.26); the two fmas,
        the sum a + 3, fast_rcp and the product are six roundings relative to psi (k = 6); the rounding of a - 1 is multiplied by
        a and is relative to a |a - 1|, not to the numerator a^2 - a - 1, which vanishes at a = 1.618: abs = a |a - 1| / q."""
    _known(kernel)
    a = s.abs()
    if kernel == "se":
        return 2.0 * a, 1.0, torch.zeros_like(a)
    if kernel == "matern32":
        return 2.0 / (1.0 + a) ** 2, 5.0, torch.zeros_like(a)
    q = 3.0 + 3.0 * a + a * a
    return 4.0 * a * (a + 2.0) / (q * q), 6.0, a * (a - 1.0).abs() / q


def check_pgrad(dghat, dgvar, x0, x, sr, th, z, V, kernel, dtype) -> Check:
    """dghat / dgvar (n0 x d) of lcgp_predict_grad against the contraction of include/lcgp_hip.h, in float64 from the rounded
    x0, x, sr and the library's own z (fetched) and V = U W (check_pgrad_v's stage):
        dghat[i, l] = -1/ell_l      sum_j c0_ij sr_j z_j    h_l(i, j)
        dgvar[i, l] =  2 D / ell_l  sum_j c0_ij sr_j V_ij   h_l(i, j)
        h_l = s / (1 + |s|) (Matern-3/2), s (SE), s (1 + |s|) / (3 + 3 |s| + s^2) (Matern-5/2),
        s = x0_il / ell_l - x_jl / ell_l,   c0 = scale (1 - nt) C0             (h is defined by dC0/dx0_l = -C0 h_l / ell_l).
    Precision.  pgrad_kernel converts the stored x0, x, sr, z and V to double and does everything else in double, in both
    storage types: u is the FLOAT64 unit roundoff for every factor below; the only storage-type roundings are those of the
    inputs, which the reference shares (and of V and z, which it takes from the library).
    Per term.  c0 carries kernel_parts' float64 magnification E (x / ell, the exponent, the polynomial; the cap and the
    cut-off as in check_predict) plus the products by c_off, sr and z or V (three roundings).  s carries u (|x0_il| + |x_jl|)
    / ell_l + u |s| (the two quotients and the difference); d h / d s = 1 / (1 + |s|)^2 <= 1 and h = s fast_rcp(1 + |s|)
    (v_rcp_f64 with two Newton steps: within 2 u of 1 / (1 + |s|)) adds four roundings: |dh| <= u (m_l + 5 |h|),
    m_l = (|x0_il| + |x_jl|) / ell_l.  Matern-5/2: h = fma(s, |s|, s) fast_rcp(fma(|s|, |s| + 3, 3)) -- two fmas, the add
    |s| + 3, fast_rcp within 2 u and the product: six roundings; d h / d s = (3 + 6 |s| + 2 s^2) / (3 + 3 |s| + s^2)^2 <= 1/3
    and |s| d h / d s <= |h|, so |dh| <= u (m_l / 3 + 7 |h|).  That is two roundings of |h| more than Matern-3/2 and a third
    of its m_l: with c0's E + 3, the n of the sum and the two of the scaling the library's count is (n + E + 12) |h| + m_l / 3,
    and twice that (the reference) sits within C = 4 times the existing (n + d + E + 4) |h| + m_l, since E >= 3 d + 3 >= 6.
    The sum over j (fma per slice, then the fixed-order slice reduction) adds n roundings
    of the absolute terms, the scaling by -1/ell_l or 2 D / ell_l two more.  Together, with C = 4 on top:
        C u / ell_l sum_j |c0_ij sr_j z_j| ((n + d + E_ij + 4) |h_l| + m_l)          (|V_ij| and 2 |D| for dgvar)
    plus the float64 floor.  m_l is not relative to |h_l|: x0 close to x_j (but not equal) leaves an absolute error of s.
    At dx = 0 (a training input among x0) both sides have s = 0 exactly, so h = 0.  Past the C0 cut-off the term itself is
    added (the library may return any c0 in [0, C0] there)."""
    dev = _dev(dghat, dgvar, z, V)
    n0, d = np.asarray(x0).shape
    gref, gbnd, vref, vbnd = _pgrad_tables(x0, x, sr, th, z, V, kernel, dtype, dev)
    names = ["l%d" % l for l in range(d)]
    cg = _worst_cols((_t(dghat, dev).reshape(n0, d) - gref).abs(), gbnd, ["dghat " + s for s in names])
    cv = _worst_cols((_t(dgvar, dev).reshape(n0, d) - vref).abs(), vbnd, ["dgvar " + s for s in names])
    return combine(cg, cv)


def check_pgrad_mean(dghat, x0, x, sr, th, z, kernel, dtype) -> Check:
    """the mean half of check_pgrad alone: dghat (n0 x d) of lcgp_predict_gradcov, whose pgrad_kernel<MEAN> launch runs the
    same contraction without V.  Reference, bound and locations are check_pgrad's (one table, _pgrad_tables)."""
    dev = _dev(dghat, z)
    n0, d = np.asarray(x0).shape
    gref, gbnd, _, _ = _pgrad_tables(x0, x, sr, th, z, None, kernel, dtype, dev)
    return _worst_cols((_t(dghat, dev).reshape(n0, d) - gref).abs(), gbnd, ["dghat l%d" % l for l in range(d)])


def _pgrad_tables(x0, x, sr, th, z, V, kernel, dtype, dev):
    """(reference, bound) of dghat and of dgvar as check_pgrad's docstring derives them: four n0 x d float64 tensors, the
    floor included in the bounds.  V = None leaves the variance half out (its two tensors are None)."""
    _known(kernel)
    u = unit("float64")
    a = _t(rounded(x0, dtype), dev)
    b = _t(rounded(x, dtype), dev)
    n0, d = a.shape
    n = b.shape[0]
    ell, scale, nug, D, _ = split_theta(th, d)
    nt = nug / (1.0 + nug)
    c0, e, cut = kernel_parts(a, b, ell, kernel, "float64", dev)
    c0 = scale * (1.0 - nt) * c0
    s = _t(rounded(np.ones(n) if sr is None else sr, dtype), dev)
    pz = c0 * (s * _t(z, dev)[:n])[None, :]
    pv = None if V is None else c0 * s[None, :] * _t(V, dev)[:n0, :n]
    cm = cut.to(torch.float64)
    wgt = n + d + e + 4.0
    gref, gbnd, vref, vbnd = (torch.zeros(n0, d, dtype=torch.float64, device=dev) for _ in range(4))
    for l in range(d):
        xa, xb = a[:, l] / ell[l], b[:, l] / ell[l]
        sl = xa[:, None] - xb[None, :]
        h = pgrad_h(sl, kernel)
        t = wgt * h.abs() + (xa.abs()[:, None] + xb.abs()[None, :])
        gref[:, l] = -(pz * h).sum(dim=1) / ell[l]
        gbnd[:, l] = (C * u * (pz.abs() * t).sum(dim=1) + (cm * (pz * h).abs()).sum(dim=1)) / ell[l]
        if pv is not None:
            vref[:, l] = 2.0 * D * (pv * h).sum(dim=1) / ell[l]
            vbnd[:, l] = 2.0 * abs(D) * (C * u * (pv.abs() * t).sum(dim=1) + (cm * (pv * h).abs()).sum(dim=1)) / ell[l]
    fl = floor("float64", n)
    if pv is None:
        return gref, gbnd + fl, None, None
    return gref, gbnd + fl, vref, vbnd + fl


def check_loo(ghat, gvar, V, b, z, sr, th, dtype, d) -> Check:
    """leave-one-out (lcgp_loo) against the closed form of lcgp_hip.h from the library's own a_ii (diagonal of the fetched
    A^-1), b and z and the rounded sr:
        ghat_i = (b_i - z_i / a_ii) / (D s_i),     gvar_i = (1 / a_ii - 1) / (D s_i^2).
    loo_kernel does this in double in both storage types, so u is float64's.  ghat: 1 / a_ii, the product with z_i, the
    difference, D s_i and the quotient are five roundings, |error| <= u (3 |b_i| + 5 |z_i / a_ii|) / |D s_i|; gvar: 1 / a_ii,
    the difference, D s_i, s_i once more and the quotient, |error| <= u (5 / |a_ii| + 4) / |D s_i^2|.  Bounds: 2 C u times
    (|b_i| + |z_i / a_ii|) / |D s_i| and (1 / |a_ii| + 1) / |D s_i^2| (2 C = 8 >= 5), plus the float64 floor.  d: the input
    dimension (it places D in the theta row)."""
    dev = _dev(ghat, gvar, V, b, z)
    u = unit("float64")
    a = torch.diagonal(_t(V, dev))
    n = a.shape[0]
    D = split_theta(th, d)[3]
    bb, zz = _t(b, dev)[:n], _t(z, dev)[:n]
    s = _t(rounded(np.ones(n) if sr is None else sr, dtype), dev)
    ia = 1.0 / a
    gref = (bb - zz * ia) / (D * s)
    gb = 2.0 * C * u * (bb.abs() + (zz * ia).abs()) / (abs(D) * s.abs()) + floor("float64", 1)
    vref = (ia - 1.0) / (D * s * s)
    vb = 2.0 * C * u * (ia.abs() + 1.0) / (abs(D) * s * s) + floor("float64", 1)
    return combine(worst((_t(ghat, dev)[:n] - gref).abs(), gb), worst((_t(gvar, dev)[:n] - vref).abs(), vb))


def check_cv_gather(M, V, fold_idx, mmax) -> Check:
    """the matrix slot of one fold (M: the raw mpad x mpad slot of the fold workspace, mpad = mmax rounded up to 128) after
    lcgp_cv_gather, BITWISE: on every lower 64-tile (whole tiles, the diagonal tiles' upper halves included, as the kernel
    writes them) M[i, j] = A^-1[idx_i, idx_j] for i, j < m (V: the fetched A^-1, whose upper triangle mirrors the lower
    storage the kernel reads at (max, min)) and the identity beyond m = len(fold_idx), up to mpad.  A copy has no rounding:
    ratio 0 when every entry matches, inf otherwise, located at the first wrong (row block, column block)."""
    dev = _dev(M, V)
    m_ = _t(M, dev)
    mpad = m_.shape[0]
    assert mpad == _pad128(mmax) and m_.shape[1] == mpad, (m_.shape, mmax)
    idx = torch.as_tensor(np.asarray(fold_idx, np.int64), device=dev)
    m = idx.shape[0]
    ref = torch.eye(mpad, dtype=torch.float64, device=dev)
    ref[:m, :m] = _t(V, dev)[idx][:, idx]
    blk = torch.arange(mpad, device=dev) // TS
    lower = blk[:, None] >= blk[None, :]
    bad = (m_.view(torch.int64) != ref.view(torch.int64)) & lower
    if not bool(bad.any()):
        return Check(0.0, ())
    i, j = (int(v) for v in torch.nonzero(bad)[0])
    return Check(math.inf, (i // TS, j // TS))


def check_cv_apply(ghat, gvar, Minv, b, z, sr, th, fold_idx, dtype, d) -> Check:
    """ghat / gvar at the positions of one fold (lcgp_cv_apply) against the closed form of lcgp_hip.h from the library's own
    M^-1 (the fetched V slot of the fold's slot; its upper triangle mirrors the lower storage), b and z:
        t = M^-1 z_B,   ghat_B = (b_B - t) / (D s_B),   gvar_B = (diag(M^-1) - 1) / (D s_B^2).
    cv_apply_kernel works in double in both storage types (u = float64's): t is an inner product of m terms, |dt| <=
    (m + 1) u (|M^-1| |z_B|); the difference, D s and the quotient add u (|b| + |t| + 2 |b - t|): together C u ((m + 2)
    |M^-1| |z_B| + 2 |b_B|) / |D s_B|.  gvar: four roundings, 2 C u (|M^-1_ii| + 1) / |D s_B^2|.  Every position of the fold
    is checked (locations: 64-blocks of the position within the fold).  d: the input dimension (places D in theta)."""
    dev = _dev(ghat, gvar, Minv, b, z)
    u = unit("float64")
    idx = torch.as_tensor(np.asarray(fold_idx, np.int64), device=dev)
    m = idx.shape[0]
    D = split_theta(th, d)[3]
    mi = _t(Minv, dev)[:m, :m]
    zb, bb = _t(z, dev)[idx], _t(b, dev)[idx]
    nfull = _t(b, dev).shape[0]
    s = _t(rounded(np.ones(nfull) if sr is None else sr, dtype), dev)[idx]
    t = mi @ zb
    gref = (bb - t) / (D * s)
    gb = C * u * ((m + 2.0) * (mi.abs() @ zb.abs()) + 2.0 * bb.abs()) / (abs(D) * s.abs()) + floor("float64", m)
    dg = torch.diagonal(mi)
    vref = (dg - 1.0) / (D * s * s)
    vb = 2.0 * C * u * (dg.abs() + 1.0) / (abs(D) * s * s) + floor("float64", 1)
    return combine(worst((_t(ghat, dev)[idx] - gref).abs(), gb), worst((_t(gvar, dev)[idx] - vref).abs(), vb))


def check_vr(out, x_ref, w, x_cand, match, r, x, sr, th, W, kernel, dtype) -> Check:
    """out[k, c] of lcgp_variance_reduction (one component, n_cand values) against its definition in float64 from the rounded
    x_ref, x_cand, x, sr, the weights w (float64, as given), the library's W = L^-1 (lower triangle of the fetched matrix):
        X_r = c_off C0(x_ref, x) o sr^T,   X_c = c_off C0(x_cand, x) o sr^T (+ scale nt sr_i at column i = match[c] >= 0)
        U = X W^T,   Sigma(t, c) = c_off C0(x_ref_t, x_cand_c) - D U_r(t) . U_c(c),   gvar_c = scale - D |U_c(c)|^2
        out_c = sum_t w_t Sigma(t, c)^2 / den_c,   den_c = max(gvar_c, 0) + 1 / (D r).
    Sigma.  U of either set is lcgp_predict's U (cross_kernel, then the product in the storage type over npad terms): |dU| <=
    g Ua with g = (npad + d + E) u and Ua = |X| |W|^T, |X| including the nugget entry (whose two extra roundings are within
    the same relative bound).  The product U_r U_c^T adds npad terms in the storage type, and C(t, c) is recomputed in double
    (E_tc).  Keeping the exact |U| on one side of each first-order term (|X| |W|^T alone is far larger than |U| where W
    cancels, which in float32 swamps the denominator below):
        |d(U_r . U_c)| <= g (Ua_t . |U_c| + |U_r| . Ua_c + |U_r| . |U_c|) + g^2 Ua_t . Ua_c
        delta_tc = C g_tc (|C_tc| + |D| (that bracket)),   g_tc = (npad + d + E_t + E_c + E_tc) u     (+ |C_tc| past the cut-off)
    with E_t, E_c the largest magnification of the row's cross covariance.  The nugget term never enters C(t, c): reference
    points are new inputs; it enters only U_c (and so gvar_c) through X_c.
    Denominator.  gvar_c = scale - D |U_c|^2 summed in double: delta_h = C |D| (g_c (2 |U_c| . Ua_c + |U_c|^2) + g_c^2
    |Ua_c|^2) + u scale; max(., 0) is 1-Lipschitz, so it passes delta_h on unchanged (a gvar_c that cancels to a tiny or
    negative value has den_c near 1 / (D r)); 1 / (D r) and the addition are three float64 roundings, C u64 den_c.
    out.  The library's den' = max(gvar', 0) + 1 / (D r) is never below 1 / (D r), whatever gvar' is, so den' >= lo_c =
    max(den_c - delta_h, 1 / (D r)) (the latter less a rounding).  With S = sum_t w_t Sigma^2, |S' - S| <= sum_t |w_t|
    (2 |Sigma| delta + delta^2) and |1/den' - 1/den| <= delta_h / (den lo):
        |out' - out| <= [sum_t |w_t| (2 |Sigma_tc| delta_tc + delta_tc^2) + |out_c| delta_h] / lo_c
                        + C (n_ref + 2) u64 sum_t |w_t| Sigma_tc^2 / den_c          (the double sums and the quotient)
    The clamp matters in float32 at large D: gvar_c of a candidate near the data cancels below its own error delta_h, and
    without it den' (so out) would have no bound at all.  Locations: 64-blocks of the candidate."""
    dev = _dev(out, W)
    d = np.asarray(x).shape[1]
    u, u64 = unit(dtype), unit("float64")
    ell, scale, nug, D, _ = split_theta(th, d)
    nt = nug / (1.0 + nug)
    coff = scale * (1.0 - nt)
    xr, xc, xt = (_t(rounded(a, dtype), dev) for a in (x_ref, x_cand, x))
    n = xt.shape[0]
    s = _t(rounded(np.ones(n) if sr is None else sr, dtype), dev)
    w_ = torch.tril(_t(W, dev))
    wa = w_.abs()
    npad = _pad128(n)

    def cross(x1, mt):
        c0, e, cut = kernel_parts(x1, xt, ell, kernel, dtype, dev)
        X = coff * c0 * s[None, :]
        Xa = X.abs() + torch.where(cut, X.abs(), torch.zeros_like(X))
        if mt is not None:
            mt = np.asarray(mt, np.int64)
            rows = np.nonzero(mt >= 0)[0]
            if rows.size:
                ri = torch.as_tensor(rows, device=dev)
                ci = torch.as_tensor(mt[rows], device=dev)
                X[ri, ci] += scale * nt * s[ci]
                Xa[ri, ci] = X[ri, ci].abs() + torch.where(cut[ri, ci], (coff * c0 * s[None, :])[ri, ci].abs(), 0.0)
        return X @ w_.T, Xa @ wa.T, e.max(dim=1).values

    Ur, Ura, er = cross(xr, None)
    Uc, Uca, ec = cross(xc, match)
    ctc, etc_, cut_tc = kernel_parts(xr, xc, ell, kernel, dtype, dev)
    ct = coff * ctc
    sig = ct - D * (Ur @ Uc.T)
    gt = (npad + d + er[:, None] + ec[None, :] + etc_) * u
    ura, uca = Ur.abs(), Uc.abs()
    prod = gt * (Ura @ uca.T + ura @ Uca.T + ura @ uca.T) + gt * gt * (Ura @ Uca.T)
    delta = C * (gt * ct.abs() + abs(D) * prod)
    delta = delta + torch.where(cut_tc, ct.abs(), torch.zeros_like(ct)) + floor(dtype, npad)
    del ctc, etc_, cut_tc, gt, prod, Ura, ura
    gc = (npad + d + ec) * u
    gv = scale - D * (Uc * Uc).sum(dim=1)
    den = torch.clamp(gv, min=0.0) + 1.0 / (D * r)
    dh = C * abs(D) * (gc * (2.0 * (uca * Uca).sum(dim=1) + (uca * uca).sum(dim=1)) + gc * gc * (Uca * Uca).sum(dim=1))
    dh = dh + u * abs(scale) + C * u64 * den + floor(dtype, npad)
    wt = _t(w, dev)
    ref = (wt[:, None] * sig * sig).sum(dim=0) / den
    num = (wt.abs()[:, None] * (2.0 * sig.abs() * delta + delta * delta)).sum(dim=0)
    lo = torch.clamp(den - dh, min=(1.0 - C * u64) / (D * r))
    bound = (num + ref.abs() * dh) / lo + C * (wt.shape[0] + 2.0) * u64 * (wt.abs()[:, None] * sig * sig).sum(dim=0) / den
    return worst((_t(out, dev) - ref).abs(), bound + floor("float64", wt.shape[0]))


# ----------------------------------------------------------------------------------------------------------------------
# the conditioned view (lcgp_condition_prepare / lcgp_condition_predict).  Per component, for m new unique inputs xn with
# latent observations t and replicate counts r, and n0 new inputs x0:
#     preparation   X_n, U_n = X_n W^T, ghat_n / gvar_n       check_cov_cross(same=0), check_cov_u, check_predict(same=0)
#                   L_S L_S^T = S                              check_cond_s
#                   L_S^-1 (W slot of the cond workspace), its dense copy in the state
#                                                              check_inverse_factor, check_cond_dense_inverse (bitwise)
#                   v = L_S^-1 (t - ghat_n)                    check_cond_v
#     prediction    X_0, U_0, ghat_0 / gvar_0                  check_cov_cross(same=0), check_cov_u, lcgp_predict's output
#                   Sigma_0n = C^x(x0, xn) - D U_0 U_n^T       check_cond_cross
#                   T = Sigma_0n L_S^-T                        check_cov_u(T, Sigma_0n, dense L_S^-1)
#                   ghat_0 + T v,  gvar_0 - rowsum(T o T)      check_cond_out
# Every check starts from the library's own input to its stage, so tau = 1 / (D r) -- which can make S ill-conditioned --
# enters no bound as a condition number.
# ----------------------------------------------------------------------------------------------------------------------
def cond_tau(th, r, m, d):
    """tau_i = 1 / (D r_i) (m values, float64 numpy; r = None: ones), as cond_diag_kernel forms it"""
    D = split_theta(th, d)[3]
    rr = np.ones(m) if r is None else np.asarray(r, np.float64)
    return 1.0 / (D * rr)


def cond_s_ref_bound(L, Un, xn, r, th, kernel, dtype):
    """(S_ref, bound, residual) of check_cond_s: float64 m x m tensors on the device of L / Un"""
    dev = _dev(L, Un)
    xn = np.asarray(xn)
    tau = cond_tau(th, r, xn.shape[0], xn.shape[1])
    ref, b1 = sigma_ref_bound(Un, xn, th, tau, kernel, dtype, dev)
    l = torch.tril(_t(L, dev))
    return ref, b1 + inverse_solve_bound(l, dtype), (ref - l @ l.T).abs()


def check_cond_s(L, Un, xn, r, th, kernel, dtype) -> Check:
    """L_S (the fetched matrix slot of the cond workspace after lcgp_condition_prepare, n = m) against
        S_ref = C(xn, xn) with the nugget on the diagonal - D U_n U_n^T + diag(tau),   tau_i = 1 / (D r_i),
    in float64 from the library's own U_n (m x n, the state's first slabs), the rounded xn and the counts r (float64, as given;
    None: ones).  S itself is factorised in place and cannot be read back, so the factor is held to S_ref directly:
        |L_S L_S^T - S_ref| <= |S - S_ref| + |L_S L_S^T - S|
    with the sum of two existing bounds (lower triangle):
      - check_sigma's for the first term.  cross_kernel (same = 1: the nugget on the diagonal), OP_PRED_COV over K = npad
        terms with alpha = -D on the product: C (npad + d + E) u (|C00| + |D| |U_n| |U_n|^T), |C00| itself past the C0 cut-off.
        cond_diag_kernel forms tau_i = 1 / (D r_i) in double (two roundings of u64), adds it to the stored diagonal in double
        and stores once: u |S_ii + tau_i| <= u |tau_i| + u |S_ii|; the second part is within the previous term, the first is
        the u |tau_i| on the diagonal.  (Operation count of the diagonal entry: npad products, the alpha product, the
        subtraction, the store, then one addition and one store more.  The double roundings of tau and the reference's own
        are within the margin of C on the first term as long as tau_i <= npad (|C00_ii| + |D| |U_n|_i^2), i.e. D r_i scale >=
        1 / npad: every case of the suite.)
      - check_cholesky_inverse_solve's for the second, on |L_S| |L_S|^T: min(i, j) + 2 terms per entry, plus the panel solve
        by the explicit inverse of the 64 x 64 diagonal block, which is what an ill-conditioned S (small tau, new inputs
        close together) needs -- that function's docstring.
    Both are independent of the condition number of S, so their sum is."""
    ref, bound, res = cond_s_ref_bound(L, Un, xn, r, th, kernel, dtype)
    return worst(res, bound)


def _first_bad(bad) -> Check:
    if not bool(bad.any()):
        return Check(0.0, ())
    i, j = (int(v) for v in torch.nonzero(bad)[0])
    return Check(math.inf, (i // TS, j // TS))


def cond_dense_mismatch(Wd, W, m):
    """the mask (mpad x mpad, bool) of the entries of the state's dense L_S^-1 that check_cond_dense_inverse rejects"""
    dev = _dev(Wd, W)
    wd = _t(Wd, dev).contiguous()
    mpad = wd.shape[0]
    assert mpad == _pad128(m) and wd.shape[1] == mpad, (wd.shape, m)
    ref = torch.eye(mpad, dtype=torch.float64, device=dev)
    ref[:m, :m] = torch.tril(_t(W, dev)[:m, :m])
    low = torch.zeros(mpad, mpad, dtype=torch.bool, device=dev)
    low[:m, :m] = torch.tril(torch.ones(m, m, dtype=torch.bool, device=dev))
    return torch.where(low, wd.view(torch.int64) != ref.view(torch.int64), wd != ref)


def check_cond_dense_inverse(Wd, W, m) -> Check:
    """the dense copy of L_S^-1 in the state (Wd: the raw mpad x mpad slab) after lcgp_condition_prepare, EXACTLY: bitwise equal to
    the fetched W slot of the cond workspace (W, m x m) on the lower triangle of the first m rows; zero above the diagonal over
    the whole mpad x mpad (the product that forms T reads whole tiles); the identity's rows from m on.  Off the copied triangle
    the comparison is by value: a NaN or any non-zero is rejected, a zero of either sign is a zero -- the triangular inverse of
    the identity padding leaves -0 = -(1 x 0 x w) below the diagonal of those rows, which adds nothing to any product.  A copy
    has no rounding: ratio 0 when every entry matches, inf otherwise, located at the first wrong (row block, column block)."""
    return _first_bad(cond_dense_mismatch(Wd, W, m))


def check_cond_v(v, Wd, t, ghat_n, m) -> Check:
    """v = L_S^-1 (t - ghat_n) (the state's m doubles) against the float64 product of the state's own dense L_S^-1 (lower
    triangle of its first m rows), the observations t (float64, as given) and ghat(xn) as the preparation left it in its
    scratch.  cond_v_kernel converts the stored row to double and accumulates in double in both storage types: per row the
    subtraction, at most m products and m - 1 additions (64 lanes, then the butterfly):
        C (m + 2) u64 (|L_S^-1| (|t| + |ghat_n|))_i + floor."""
    dev = _dev(v, Wd, ghat_n)
    w = torch.tril(_t(Wd, dev)[:m, :m])
    tt, gh = _t(t, dev)[:m], _t(ghat_n, dev)[:m]
    ref = w @ (tt - gh)
    bound = C * (m + 2.0) * unit("float64") * (w.abs() @ (tt.abs() + gh.abs())) + floor("float64", m)
    return worst((_t(v, dev)[:m] - ref).abs(), bound)


def check_cond_cross(Sg, U0, Un, x0, xn, th, kernel, dtype) -> Check:
    """Sigma_0n (n0 x m, the third slabs of the lcgp_condition_predict scratch) against
        scale (1 - nt) C0(x0, xn) - D U_0 U_n^T,
    never a nugget term (a row of x0 that equals a row of xn is still a new input of the continuous surface), in float64 from
    the library's own U_0 (n0 x n, the scratch's second slabs) and U_n (m x n, the state) and the rounded x0, xn.
    cross_kernel evaluates C^x like X in check_cov_cross ((E + 4) u relative, any value in [0, C0] past the cut-off);
    OP_COND_CROSS accumulates sum_k U_0[i, k] U_n[j, k] over K = npad terms in the storage type on 64 x 64 tiles, applies
    alpha = -D to the product, adds the C tile and stores once: npad products, the alpha product, the addition and the store,
        C (npad + d + E) u (|C^x| + |D| |U_0| |U_n|^T)  (+ |C^x| past the cut-off)  + floor,
    on ALL entries (the output is rectangular and has no symmetry to lean on)."""
    dev = _dev(Sg, U0, Un)
    d = np.asarray(x0).shape[1]
    u = unit(dtype)
    ell, scale, nug, D, _ = split_theta(th, d)
    nt = nug / (1.0 + nug)
    c0, e, cut = kernel_parts(rounded(x0, dtype), rounded(xn, dtype), ell, kernel, dtype, dev)
    u0, un = _t(U0, dev), _t(Un, dev)
    k = _pad128(un.shape[1])
    cx = scale * (1.0 - nt) * c0
    ref = cx - D * (u0 @ un.T)
    bound = C * (k + d + e) * u * (cx.abs() + abs(D) * (u0.abs() @ un.abs().T)) + floor(dtype, k)
    bound = bound + torch.where(cut, cx.abs(), torch.zeros_like(cx))
    return worst((_t(Sg, dev) - ref).abs(), bound, lower=False)


def check_cond_out(ghat, gvar, T, v, ghat0, gvar0, m) -> Check:
    """the outputs of lcgp_condition_predict (n0 doubles each, one component) against
        ghat_0 + T v,    gvar_0 - rowsum(T o T)
    in float64 from the library's own T (n0 x m, the scratch's fourth slabs), v (the state) and the ghat_0 / gvar_0 of a
    separate lcgp_predict(same = 0) call on the same rows, which the view's own first stage must equal bitwise.
    cond_reduce_kernel converts T to double and sums m terms in double (64 lanes, then the butterfly), then one addition to
    the stored output: m products, m additions:
        C (m + 2) u64 (|ghat_0| + |T| |v|) + floor,    C (m + 2) u64 (|gvar_0| + sum_j T_ij^2) + floor.
    The bound of gvar is relative to gvar_0 + sum T^2, not to the result: where a row of x0 equals a row of xn the result
    cancels to about tau."""
    dev = _dev(ghat, gvar, T, v)
    tm = _t(T, dev)[:, :m]
    vv = _t(v, dev)[:m]
    g0, v0 = _t(ghat0, dev), _t(gvar0, dev)
    w = C * (m + 2.0) * unit("float64")
    fl = floor("float64", m)
    gref = g0 + tm @ vv
    gb = w * (g0.abs() + tm.abs() @ vv.abs()) + fl
    t2 = (tm * tm).sum(dim=1)
    vref = v0 - t2
    vb = w * (v0.abs() + t2) + fl
    return combine(worst((_t(ghat, dev) - gref).abs(), gb), worst((_t(gvar, dev) - vref).abs(), vb))


# ----------------------------------------------------------------------------------------------------------------------
# second-order input queries: lcgp_predict_hess (pdx_kernel -> OP_PRED_U on n0 d rows -> phess_gram_kernel -> phess_kernel) and
# lcgp_predict_gradcov (pgrad_kernel<MEAN> -> pdx_kernel -> the same product -> gradcov_kernel -> gradcov_reduce_kernel).
# P = DX W^T goes through check_cov_u(P, DX, W): its inner dimension is npad whatever the number of rows, so the rows_pad rows
# of DX (n0 d rounded up to 64 / 128) need no wider count.  dghat of the second goes through check_pgrad_mean.
# ----------------------------------------------------------------------------------------------------------------------
def tri_names(d, prefix):
    """names of the packed lower triangle: entry (l, m <= l) at l (l + 1) / 2 + m"""
    return ["%s l%d m%d" % (prefix, l, m) for l in range(d) for m in range(l + 1)]


def _second_order_parts(x0, x, sr, th, kernel, dev):
    """shared float64 pieces from the ROUNDED x0, x, sr: c = c_off C0 (n0 x n), E, the cut-off mask (float64's: these kernels
    evaluate c0 in double in both storage types), sr, and per dimension the signed scaled distances S, the absolute terms
    Mx = (|x0_il| + |x_jl|) / ell_l and H = h(S): three n0 x n x d tensors (the largest objects; no n0 x n x d x d one)."""
    a, b = _t(x0, dev), _t(x, dev)
    n0, d = a.shape
    n = b.shape[0]
    ell, scale, nug, D, _ = split_theta(th, d)
    nt = nug / (1.0 + nug)
    c0, e, cut = kernel_parts(a, b, ell, kernel, "float64", dev)
    c0 = scale * (1.0 - nt) * c0
    s = _t(np.ones(n) if sr is None else sr, dev)
    le = _t(ell, dev)
    xa, xb = a / le, b / le
    S = xa[:, None, :] - xb[None, :, :]
    Mx = xa.abs()[:, None, :] + xb.abs()[None, :, :]
    return c0, e, cut.to(torch.float64), s, S, Mx, pgrad_h(S, kernel), ell, scale * (1.0 - nt), D


def check_pdx(DX, x0, x, sr, th, kernel, dtype) -> Check:
    """DX (n0 d x n, one slab of the lcgp_predict_hess / lcgp_predict_gradcov scratch, row i d + l) against
        DX[i d + l, j] = c_off C0_ij sr_j h_l(s_l),   s_l = x0_il / ell_l - x_jl / ell_l
    in float64 from the rounded x0, x, sr.  Precision: pdx_kernel converts the stored inputs to double, forms everything in
    double and rounds ONCE to the storage type at the store, in both storage types.  Counted from the source:
      v = c_off kern_c0(poly, ssum) cs_j: C0 carries kernel_parts' float64 magnification E; c_off = scale (1 - nug / (1 + nug))
        is four roundings, the two products two: (E + 6) u64 relative;
      h: u64 (m_l + 5 |h|) (Matern-3/2), u64 (m_l / 3 + 7 |h|) (Matern-5/2), u64 (m_l + |h|) (SE: h = s), m_l = (|x0_il| + |x_jl|)
        / ell_l the absolute term of check_pgrad (x0 close to x_j leaves an absolute error of s);
      the product v h in double: one more; the store (T): one rounding of the storage type.
    Library: u64 |v| ((E + 14) |h| + m_l) + u |DX|; the reference commits the float64 part again.  With C = 4 on top:
        C u64 |v| ((E + 14) |h| + m_l) + 2 u |DX_ref| + floor(dtype, d),      and |DX_ref| itself past the C0 cut-off.
    At a training input among x0, s = 0 exactly on both sides (the same two quotients), h = 0 and DX = 0 exactly: the bound
    there is the floor alone.  (The padding -- columns n .. npad, rows n0 d .. rows_pad -- is asserted bitwise zero by the GPU
    test: an exact statement, not a bound.)  Locations: (64-block of the row i d + l, 64-block of the column)."""
    _known(kernel)
    dev = _dev(DX)
    n0, d = np.asarray(x0).shape
    c0, e, cm, s, S, Mx, H, ell, _, _ = _second_order_parts(rounded(x0, dtype), rounded(x, dtype),
                                                            None if sr is None else rounded(sr, dtype), th, kernel, dev)
    n = c0.shape[1]
    v = c0 * s[None, :]
    ref = (v[:, :, None] * H).permute(0, 2, 1).reshape(n0 * d, n)
    t = (v.abs()[:, :, None] * ((e[:, :, None] + 14.0) * H.abs() + Mx)).permute(0, 2, 1).reshape(n0 * d, n)
    bound = C * unit("float64") * t + 2.0 * unit(dtype) * ref.abs() + floor(dtype, d)
    bound = bound + cm[:, None, :].expand(n0, d, n).reshape(n0 * d, n) * ref.abs()
    return worst((_t(DX, dev)[:n0 * d, :n] - ref).abs(), bound, lower=False)


def check_phess(d2ghat, d2gvar, x0, x, sr, th, z, V, P, kernel, dtype) -> Check:
    """d2ghat / d2gvar (n0 x d (d + 1) / 2, the packed lower triangles, entry (l, m <= l) at l (l + 1) / 2 + m) of
    lcgp_predict_hess against include/lcgp_hip.h, in float64 from the rounded x0, x, sr and the library's own z (fetched),
    V = U W (n0 x n, the first slabs of the scratch) and P = DX W^T (n0 d x n, row i d + l; the last slabs):
        d2ghat[i, lm] =        sum_j c_ij kap_lm(i, j) sr_j z_j                     / (ell_l ell_m)
        d2gvar[i, lm] = -2 D (sum_j c_ij kap_lm(i, j) sr_j V_ij + P_il . P_im)       / (ell_l ell_m)
        kap_lm = h(s_l) h(s_m)  (l != m),   psi(s_l)  (l == m);   c = c_off C0.
    Precision.  phess_kernel and phess_gram_kernel convert the stored x0, x, sr, z, V and P to double and compute in double in
    both storage types: u is the FLOAT64 unit roundoff throughout; the storage-type roundings are those of the inputs, which the
    reference shares or takes from the library.  Counted from the source, per term of the sum over j:
      c0 = c_off kern_c0: E (kernel_parts, float64) + 4 (c_off) + 1; times wz_j = sr_j z_j or wsr_j V_ij: 2 more: E + 7;
      l != m: kap = h_l h_m with |dh| <= u (m + 7 |h|) (check_pgrad; the largest of the three kernels) and the product:
          |d kap| <= u (m_l |h_m| + m_m |h_l| + 15 |kap|);
      l == m: kap = psi(s_l), |d psi| <= u (|psi'| (m_l + |s_l|) + k |psi| + abs), k <= 6 (pgrad_psi_err: the m_l weight of psi
          is |psi'|, which is 2 |s| for SE and not bounded by 1);
      the fma into the accumulator, the per-lane sums in ascending j, the half-wave shuffle and the four waves: at most n
      roundings of the absolute terms; 1 / (ell_l ell_m) two roundings and its product one; d2gvar adds the Gram term, -2 D and
      the same scaling: five.  Library: (n + E + 28) |term| + the m terms; the reference the same again; within C = 4 times
          (n + d + E + 16) |c kap w_j| + |c w_j| (m_l |h_m| + m_m |h_l|)                          (l != m)
          (n + d + E + 16) |c psi w_j| + |c w_j| (|psi'| (m_l + |s_l|) + abs)                     (l == m).
      Past the C0 cut-off the term itself is added, as in check_pgrad.
    The Gram term G_i[l, m] = P_il . P_im: n fmas in double from the storage-type P (16-byte loads and a tail, then the
    butterfly of wave_sum: any order) -- C (n + 2) u64 |P_il| . |P_im|, scaled by 2 |D| / (ell_l ell_m) like the rest (the five
    roundings behind it are within C (n + 2) for n >= 2 on top of the library's n + 6 and the reference's n).
    Locations: (64-block of the new input, "d2ghat l<l> m<m>" / "d2gvar l<l> m<m>").  Loops over l, vectorised over m <= l."""
    _known(kernel)
    dev = _dev(d2ghat, d2gvar, z, V, P)
    u = unit("float64")
    n0, d = np.asarray(x0).shape
    c0, e, cm, s, S, Mx, H, ell, _, D = _second_order_parts(rounded(x0, dtype), rounded(x, dtype),
                                                            None if sr is None else rounded(sr, dtype), th, kernel, dev)
    n = c0.shape[1]
    tri = d * (d + 1) // 2
    pz = c0 * (s * _t(z, dev)[:n])[None, :]
    pv = c0 * s[None, :] * _t(V, dev)[:n0, :n]
    Pr = _t(P, dev)[:n0 * d, :n].reshape(n0, d, n)
    Pa = Pr.abs()
    wgt = (n + d + e + 16.0)[:, :, None]
    Ha = H.abs()
    gref, gbnd, vref, vbnd = (torch.zeros(n0, tri, dtype=torch.float64, device=dev) for _ in range(4))
    for l in range(d):
        m1 = l + 1
        kap = H[:, :, l:m1] * H[:, :, :m1]
        t = wgt * kap.abs() + Mx[:, :, l:m1] * Ha[:, :, :m1] + Mx[:, :, :m1] * Ha[:, :, l:m1]
        sl = S[:, :, l]
        psi = pgrad_psi(sl, kernel)
        dpsi, _, apsi = pgrad_psi_err(sl, kernel)
        kap[:, :, l] = psi
        t[:, :, l] = wgt[:, :, 0] * psi.abs() + dpsi * (Mx[:, :, l] + sl.abs()) + apsi
        inv = 1.0 / (ell[l] * _t(ell[:m1], dev))
        o = slice(l * (l + 1) // 2, l * (l + 1) // 2 + m1)
        cz = torch.einsum("ij,ijm->im", pz, kap)
        bz = C * u * torch.einsum("ij,ijm->im", pz.abs(), t) + torch.einsum("ij,ijm->im", cm * pz.abs(), kap.abs())
        cv = torch.einsum("ij,ijm->im", pv, kap)
        bv = C * u * torch.einsum("ij,ijm->im", pv.abs(), t) + torch.einsum("ij,ijm->im", cm * pv.abs(), kap.abs())
        G = torch.einsum("ij,imj->im", Pr[:, l], Pr[:, :m1])
        Gb = C * (n + 2.0) * u * torch.einsum("ij,imj->im", Pa[:, l], Pa[:, :m1])
        gref[:, o] = cz * inv
        gbnd[:, o] = bz * inv
        vref[:, o] = -2.0 * D * (cv + G) * inv
        vbnd[:, o] = 2.0 * abs(D) * (bv + Gb) * inv
    fl = floor("float64", n)
    cg = _worst_cols((_t(d2ghat, dev).reshape(n0, tri) - gref).abs(), gbnd + fl, tri_names(d, "d2ghat"))
    cv = _worst_cols((_t(d2gvar, dev).reshape(n0, tri) - vref).abs(), vbnd + fl, tri_names(d, "d2gvar"))
    return combine(cg, cv)


GRADCOV_KAPPA = {"matern32": 1.0, "se": 1.0, "matern52": 1.0 / 3.0}      # -f''(0) of the 1-D factor


def check_gradcov(gamma, dghat, x0, x, sr, th, z, P, kernel, dtype) -> Check:
    """gamma (n0 x d (d + 1) / 2 packed as d2gvar is) and dghat (n0 x d) of lcgp_predict_gradcov.  dghat goes through
    check_pgrad_mean (the mean half of check_pgrad: the same launch without V).  gamma against
        Gamma[i, lm] = (delta_lm c_k kappa - D P_il . P_im) / (ell_l ell_m),   c_k = scale (1 - nt),   kappa = 1, 1, 1/3
    in float64 from the library's own P (n0 d x n, the second slabs of the scratch).  gradcov_kernel works in double from the
    storage-type P in both storage types (u = float64's).  Counted from the source: the dot product is n fmas and the
    butterfly (n roundings, any order); D s, the difference, ell_l ell_m and the quotient four more; the prior c_k kappa is
    scale (1 - nug / (1 + nug)) kappa, five roundings (the constant 1/3 half of one), and shares the last three.  Library:
    (n + 4) |D| |P_il| . |P_im| + 8 c_k kappa; the reference the same in float64; with C = 4:
        C u64 ((n + 2) |D| |P_il| . |P_im| + 5 delta_lm c_k kappa) / (ell_l ell_m) + floor.
    Locations: (64-block of the new input, "gamma l<l> m<m>"), or check_pgrad's for dghat."""
    _known(kernel)
    dev = _dev(gamma, dghat, z, P)
    u = unit("float64")
    n0, d = np.asarray(x0).shape
    n = np.asarray(x).shape[0]
    ell, scale, nug, D, _ = split_theta(th, d)
    prior = scale * (1.0 - nug / (1.0 + nug)) * GRADCOV_KAPPA[kernel]
    tri = d * (d + 1) // 2
    Pr = _t(P, dev)[:n0 * d, :n].reshape(n0, d, n)
    Pa = Pr.abs()
    ref, bnd = (torch.zeros(n0, tri, dtype=torch.float64, device=dev) for _ in range(2))
    for l in range(d):
        m1 = l + 1
        inv = 1.0 / (ell[l] * _t(ell[:m1], dev))
        dl = torch.zeros(m1, dtype=torch.float64, device=dev)
        dl[l] = 1.0
        o = slice(l * (l + 1) // 2, l * (l + 1) // 2 + m1)
        G = torch.einsum("ij,imj->im", Pr[:, l], Pr[:, :m1])
        Ga = torch.einsum("ij,imj->im", Pa[:, l], Pa[:, :m1])
        ref[:, o] = (dl * prior - D * G) * inv
        bnd[:, o] = C * u * ((n + 2.0) * abs(D) * Ga + 5.0 * dl * abs(prior)) * inv
    cg = _worst_cols((_t(gamma, dev).reshape(n0, tri) - ref).abs(), bnd + floor("float64", n), tri_names(d, "gamma"))
    return combine(cg, check_pgrad_mean(dghat, x0, x, sr, th, z, kernel, dtype))


def check_gradcov_sum(M_after, M_before, gamma, w) -> Check:
    """M (d (d + 1) / 2, one component) after lcgp_predict_gradcov with weights against M_before + sum_i w_i Gamma_i, from the
    library's OWN gamma (n0 x d (d + 1) / 2) and the weights w (n0 float64).  gradcov_kernel multiplies w_i Gamma_i (one
    rounding), sums the four waves of a workgroup, gradcov_reduce_kernel the workgroups in ascending order and adds the sum to
    M: n0 + 1 roundings of the absolute terms in any order, and the last addition, relative to |M_after| <= |M_before| + sum:
        C (n0 + 2) u64 sum_i |w_i Gamma_i| + u64 |M_before| + floor.
    The last term is ONE rounding, so the reference may not commit one of its own there: the sum is formed in float64 (its
    error is within the first term) and M_after - M_before by an error-free TwoSum, so only sum-sized quantities are rounded."""
    dev = _dev(M_after, M_before, gamma)
    u = unit("float64")
    g, ww = _t(gamma, dev), _t(w, dev)
    n0 = g.shape[0]
    ma, mb = _t(M_after, dev).reshape(-1), _t(M_before, dev).reshape(-1)
    sref = (ww[:, None] * g).sum(dim=0)
    sabs = (ww[:, None] * g).abs().sum(dim=0)
    hi = ma - mb                                   # TwoSum(ma, -mb): hi + lo = ma - mb exactly
    bv = hi - ma
    lo = (ma - (hi - bv)) + (-mb - bv)
    err = ((hi - sref) + lo).abs()
    bound = C * (n0 + 2.0) * u * sabs + u * mb.abs() + floor("float64", n0)
    r = err / bound
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    i = int(torch.argmax(r))
    d = int(round((math.sqrt(8 * r.numel() + 1) - 1) / 2))
    return Check(float(r[i]), (tri_names(d, "M")[i],))


# ----------------------------------------------------------------------------------------------------------------------
# box-averaged predictions (lcgp_predict_marginal, lcgp_condition_predict_marginal): marg_table_kernel -> the masked instance of
# cross_kernel -> U = X W^T (check_cov_u) -> marg_reduce_kernel; on a view the second table over xn, the masked rows against
# xn, OP_COND_CROSS, T (check_cov_u) and cond_reduce_kernel (check_cond_out, from an m = 0 call); marg_refcov_kernel (gcov).
#
# The table is the one stage of the library whose reference cannot be a float64 restatement: its formulas (a 20-term series
# below b = 1/2, closed forms with expm1 / erf / erfc above, three branches of I1) lose accuracy in places, and a restatement
# with the same switches loses it in the same places.  marg_exact / marg_exact2 are mpmath references with one formula per
# region and no switch; the bounds below FOLLOW the library's branches, the references do not.
# ----------------------------------------------------------------------------------------------------------------------
MARG_DPS = 50                   # digits of the mpmath references (guard digits are added where a closed form cancels)
MARG_ULP = 4.0                  # ASSUMED error of one device exp / expm1 / erf / erfc call, in ulp: no ulp table of ROCm's device
#                                 maths ships with the toolchain this suite runs on, so the largest figure the public tables of
#                                 comparable device libraries give for these four in double (1, 1, 2, 4..5) is taken for all
MARG_SERIES_BELOW = 0.5         # lcgp_hip.hip MARG_SERIES_BELOW / MARG_SERIES_TERMS: for the BOUND only (which terms are summed)
MARG_SERIES_TERMS = 20
# roundings of the closed forms beyond the special-function call, counted from marg_F / marg_G / marg_Fc:
#   Matern-3/2  F = 2 em - b e: the product b e, the difference (2 em is exact): 2, kept at 3 (one of margin)           3
#               G = 3 em - b (3 + b) e: 3 + b, two products, 3 em, the difference                                        5
#               Fc = (2 + b) e: the sum, the product                                                                      2
#   Matern-5/2  F = (8/3) em - b (5 + b) / 3 e: the constant (1/2), its product, 5 + b, b *, / 3, * e, the difference     7
#               G = 5 em - b (5 + b (2 + b / 3)) e: b / 3, 2 +, b *, 5 +, b *, * e, 5 em, the difference                   8
#               Fc = (8 + b (5 + b)) / 3 e: 5 + b, b *, 8 +, / 3, * e                                                     5
#   SE          F, Fc = c erf|erfc(b s): the constant c (1/2) and its product (the product b s and the constant s act on the
#               ARGUMENT: MARG_ARG)                                                                                        2
#               G = -expm1(-(b / 2) b): the product, whose error u b^2 / 2 moves G by at most u G (x e^-x <= 1 - e^-x)       1
# each on the sum of the absolute values of the terms of that form (_marg_terms)
MARG_ROUNDINGS = {("matern32", "F"): 3, ("matern32", "G"): 5, ("matern32", "Fc"): 2,
                  ("matern52", "F"): 7, ("matern52", "G"): 8, ("matern52", "Fc"): 5,
                  ("se", "F"): 2, ("se", "G"): 1, ("se", "Fc"): 2}
# the series: term m is t_m f(m) / (m + 1 | m + 2) with t_m = (-b)^m / m! built by m products and m quotients: 2 m + 3 roundings
# (the product with f, the quotient, f = (m - 1)(m - 3) / 3 itself for Matern-5/2) on a term that is below 1/2^m / m! of the
# first, so sum_m (2 m + 3) |term_m| <= 4 sum_m |term_m| (m = 0: 3; m = 2: 7/24; m = 3: 9/192; ...); the 20 additions add at most
# u times the largest partial sum each (<= sum |term_m|), the products b sf / b b sg one / two more: 4 + 20 + 2, and one of margin
MARG_SERIES_ROUNDINGS = 27.0
# roundings of the ARGUMENT b = |xv - lo| / ell (the difference and the quotient: 2), for SE also b s and the constant s (1.5),
# rounded up; they act through dF / db = kappa(b), dFc / db = -kappa(b): |dF| <= MARG_ARG u b kappa(b)
MARG_ARG = {"matern32": 2.0, "matern52": 2.0, "se": 4.0}
_MARG_CACHE = {}


def _kappa(kernel, b):
    """the 1-D factor of the product kernel at the scaled distance b >= 0 (float64 numpy)"""
    _known(kernel)
    if kernel == "se":
        return np.exp(-0.5 * b * b)
    if kernel == "matern32":
        return (1.0 + b) * np.exp(-b)
    return (1.0 + b + b * b / 3.0) * np.exp(-b)


def _marg_mp(kernel, which, b):
    """F(b) = int_0^b kappa, Fc(b) = int_b^inf kappa or G(b) = int_0^b u kappa(u) du in mpmath, MARG_DPS digits AFTER the
    cancellation of the closed form at small b (F ~ b, G ~ b^2 / 2 from terms of order one: two, three decimal guard digits
    per decade of 1 / b).  The tails go through erfc and the exact Matern tails, never through 1 - F."""
    _known(kernel)
    guard = 0 if (b == 0 or b >= 1) else 3 * (int(-mp.log10(b)) + 1)
    with mp.workdps(MARG_DPS + 10 + guard):
        if kernel == "se":
            if which == "F":
                return mp.sqrt(mp.pi / 2) * mp.erf(b / mp.sqrt(2))
            if which == "Fc":
                return mp.sqrt(mp.pi / 2) * mp.erfc(b / mp.sqrt(2))
            return -mp.expm1(-b * b / 2)
        e = mp.exp(-b)
        if kernel == "matern32":
            if which == "F":
                return -2 * mp.expm1(-b) - b * e
            if which == "Fc":
                return (2 + b) * e
            return -3 * mp.expm1(-b) - b * (3 + b) * e
        if which == "F":
            return -mp.mpf(8) / 3 * mp.expm1(-b) - b * (5 + b) / 3 * e
        if which == "Fc":
            return (8 + b * (5 + b)) / 3 * e
        return -5 * mp.expm1(-b) - b * (5 + b * (2 + b / 3)) * e


def marg_exact(kernel, x, lo, hi, ell):
    """I1 = (1 / w) int_lo^hi kappa(|t - x| / ell) dt, w = hi - lo, for every value of the float64 array x (lo, hi, ell: float64
    scalars, taken as exact), as an object array of mpmath numbers of MARG_DPS digits.  One formula per region:
        x inside [lo, hi] (ends included):   (ell / w) [F(b1) + F(b2)],      b1 = (x - lo) / ell, b2 = (hi - x) / ell
        x outside:                           (ell / w) [Fc(bn) - Fc(bf)],    bn < bf the scaled distances to the two ends
    with Fc through erfc (SE) or the exact Matern tails -- F(bf) - F(bn) is wrong in the far tails at ANY working precision that
    does not grow with b, which is how a 60-digit reference of that form went wrong in the SE tails.  No series, no switch at
    b = 1/2, none at bn = 1; nothing from tests/marginal_ref.py.  b1, b2 are formed exactly (the differences of floats are exact
    in mpmath).  Cached per (kernel, ell, lo, hi, x value): a case costs at most q d n evaluations."""
    _known(kernel)
    xs = np.asarray(x, np.float64)
    key = (kernel, float(ell), float(lo), float(hi))
    cache = _MARG_CACHE.setdefault(key, {})
    out = np.empty(xs.shape, object)
    flat = out.reshape(-1)
    with mp.workdps(MARG_DPS + 10):
        le, l0, h0 = mp.mpf(float(ell)), mp.mpf(float(lo)), mp.mpf(float(hi))
        w = h0 - l0
        for i, v in enumerate(xs.reshape(-1).tolist()):
            got = cache.get(v)
            if got is None:
                xv = mp.mpf(v)
                a1, a2 = xv - l0, h0 - xv
                b1, b2 = abs(a1) / le, abs(a2) / le
                if a1 >= 0 and a2 >= 0:
                    r = _marg_mp(kernel, "F", b1) + _marg_mp(kernel, "F", b2)
                else:
                    r = _marg_mp(kernel, "Fc", min(b1, b2)) - _marg_mp(kernel, "Fc", max(b1, b2))
                got = cache[v] = le / w * r
            flat[i] = got
    return out


def marg_exact2(kernel, w, ell):
    """I2 = (1 / w^2) int int kappa(|t - t'| / ell) dt dt' over [0, w]^2 = 2 [F(a) / a - G(a) / a^2], a = w / ell, in mpmath
    (MARG_DPS digits; w: a float or an mpmath number -- the exact hi - lo)"""
    _known(kernel)
    key = (kernel, float(ell), "i2", str(w))
    if key not in _MARG_CACHE:
        with mp.workdps(MARG_DPS + 10):
            a = mp.mpf(w) / mp.mpf(float(ell))
            _MARG_CACHE[key] = 2 * (_marg_mp(kernel, "F", a) / a - _marg_mp(kernel, "G", a) / (a * a))
    return _MARG_CACHE[key]


def _mp_err(got, exact):
    """|got - exact| as float64: got a float64 array, exact an object array of mpmath numbers (NaN in got: inf)"""
    g = np.asarray(got, np.float64)
    out = np.empty(g.shape, np.float64)
    with mp.workdps(MARG_DPS + 10):
        for i, (a, b) in enumerate(zip(g.reshape(-1).tolist(), np.asarray(exact, object).reshape(-1))):
            out.reshape(-1)[i] = float(abs(mp.mpf(a) - b)) if math.isfinite(a) else math.inf
    return out


def _marg_terms(kernel, which, b):
    """K A of one evaluation of marg_F / marg_G / marg_Fc at b (a float64 array) IN THE BRANCH THE LIBRARY TAKES: A the sum of the
    absolute values of the terms that form adds or subtracts, K its count of roundings in units of u (MARG_ULP per special
    function call plus MARG_ROUNDINGS, or MARG_SERIES_ROUNDINGS).  |error of the evaluation| <= u K A."""
    _known(kernel)
    b = np.asarray(b, np.float64)
    k = MARG_ULP + MARG_ROUNDINGS[kernel, which]
    if kernel == "se":
        s = math.sqrt(0.5)
        c = math.sqrt(0.5 * math.pi)
        if which == "G":
            return k * -np.expm1(-0.5 * b * b)
        return k * c * (scipy.special.erf(b * s) if which == "F" else scipy.special.erfc(b * s))
    e, em = np.exp(-b), -np.expm1(-b)
    if which == "Fc":
        return k * ((2.0 + b) * e if kernel == "matern32" else (8.0 + b * (5.0 + b)) / 3.0 * e)
    if kernel == "matern32":
        closed = 2.0 * em + b * e if which == "F" else 3.0 * em + b * (3.0 + b) * e
    else:
        closed = (8.0 / 3.0) * em + b * (5.0 + b) / 3.0 * e if which == "F" else 5.0 * em + b * (5.0 + b * (2.0 + b / 3.0)) * e
    bs = np.minimum(b, MARG_SERIES_BELOW)
    t, sa = np.ones_like(bs), np.zeros_like(bs)
    for m in range(MARG_SERIES_TERMS):
        f = abs(1.0 - m) if kernel == "matern32" else abs((m - 1.0) * (m - 3.0)) / 3.0
        sa = sa + t * f / (m + (1.0 if which == "F" else 2.0))
        t = t * bs / (m + 1.0)
    series = bs * sa if which == "F" else bs * bs * sa
    return np.where(b < MARG_SERIES_BELOW, MARG_SERIES_ROUNDINGS * series, k * closed)


def marg_table_bound(kernel, xv, lo, hi, ell):
    """the bound of check_marg_table on |I1 - exact| for the values xv (float64 array; lo, hi, ell float64 scalars), without C:
        u (ell / w) [ K1 A1 + K2 A2 + 3 (A1 + A2) + MARG_ARG (b1 kappa(b1) + b2 kappa(b2)) ]
    marg_I1 forms w = hi - lo, a1 = xv - lo, a2 = hi - xv, b = |a| / ell (one rounding each) and takes one of three branches:
    F(b1) + F(b2) inside (a1, a2 >= 0: the sign of a rounded difference is the exact one, so the library and the reference
    agree on it), otherwise with bn <= bf: Fc(bn) - Fc(bf) if bn > 1, else F(bf) - F(bn).  The b are recomputed here with the same
    three IEEE operations, so this follows the library's branch also at bn = 1 and b = 1/2 to the last bit.
      - K A: the evaluation of each of the two terms (_marg_terms).  The two are then added or subtracted and the result is
        scaled: the sum, w, ell / w and the product are four roundings of |r| <= A1 + A2, counted as 3 (w and ell / w act on the
        factor alone; half of each is in the margin of C).  Outside the box the result is (ell / w) kappa(.) (bf - bn) while the
        terms stay of order one: the error relative to the RESULT grows like ell / w -- the narrow-box loss, a property of the
        formula, which this bound admits and profiles/stage_bounds_marginal.txt records.
      - the argument: b carries two roundings and F' = kappa, Fc' = -kappa: u MARG_ARG b kappa(b) per end.  Relative to a tail
        Fc(b) ~ kappa(b) / b (SE) this is u MARG_ARG b^2: the argument magnification of the far SE tails."""
    _known(kernel)
    xv = np.asarray(xv, np.float64)
    lo, hi, ell = float(lo), float(hi), float(ell)
    w = hi - lo
    a1, a2 = xv - lo, hi - xv
    b1, b2 = np.abs(a1) / ell, np.abs(a2) / ell
    inside = (a1 >= 0.0) & (a2 >= 0.0)
    far = ~inside & (np.minimum(b1, b2) > 1.0)
    t1 = np.where(far, _marg_terms(kernel, "Fc", b1), _marg_terms(kernel, "F", b1))
    t2 = np.where(far, _marg_terms(kernel, "Fc", b2), _marg_terms(kernel, "F", b2))
    k1 = MARG_ULP + np.where(far, MARG_ROUNDINGS[kernel, "Fc"], MARG_ROUNDINGS[kernel, "F"])
    # 3 (A1 + A2) <= 3 (K1 A1 + K2 A2) / min K: expressed through the K A already formed
    extra = 3.0 * (t1 + t2) / np.minimum(k1, MARG_SERIES_ROUNDINGS)
    arg = MARG_ARG[kernel] * (b1 * _kappa(kernel, b1) + b2 * _kappa(kernel, b2))
    return unit("float64") * (ell / w) * (t1 + t2 + extra + arg)


def marg_i2_bound(kernel, w, ell):
    """the bound of check_marg_table on |I2 - exact|, without C.  marg_table_kernel: a = w / ell (w = hi - lo: two roundings),
    2 (F(a) / a - G(a) / (a a)): the evaluations (K_F A_F, K_G A_G of _marg_terms), one / two roundings for the quotients, one
    for the difference, and the argument through d/da [F / a - G / a^2] = -F / a^2 + 2 G / a^3 (the kappa terms cancel) with
    |da| <= 2 u a:      2 u [ (K_F A_F + F) / a + (K_G A_G + 2 G) / a^2 + (F / a + G / a^2) + 2 (F / a + 2 G / a^2) ]
    with F <= A_F, G <= A_G used for the values."""
    a = (float(w)) / float(ell)
    kf, kg = float(_marg_terms(kernel, "F", a)), float(_marg_terms(kernel, "G", a))
    kmin = MARG_ULP + 1.0
    f, g = kf / kmin, kg / kmin                      # upper bounds of A_F >= F and A_G >= G (every K is at least MARG_ULP + 1)
    return 2.0 * unit("float64") * ((kf + 4.0 * f) / a + (kg + 7.0 * g) / (a * a))


def check_marg_table(tab, i2, x, th, box, kernel, dtype, n, npad) -> Check:
    """the table of 1-D box averages (tab: q x d x npad doubles, i2: q x d doubles; double in BOTH storage types) after
    marg_table_kernel, entry by entry against marg_exact at the ROUNDED x (the library converts the stored x to double) and
    marg_exact2 at the exact hi - lo, for the theta rows th (q x tw) and box (2 x d):
        |tab - I1| <= C marg_table_bound + floor (1 + ell / w),        |i2 - I2| <= C marg_i2_bound + floor
    (the floor: the tails underflow to denormals and to zero where the exact value is 1e-320 or less; it scales with the factor
    ell / w that multiplies the underflowed difference).  Columns n .. npad - 1 must be BITWISE 1.0 (the masked cross_kernel
    multiplies whole 64-column tiles into poly; their products are discarded, but a NaN there must not be relied on to vanish).
    Locations: (component, dimension, 64-block of the column), or (component, dimension, "i2")."""
    _known(kernel)
    tb = np.asarray(tab.cpu() if isinstance(tab, torch.Tensor) else tab, np.float64)
    ii = np.asarray(i2.cpu() if isinstance(i2, torch.Tensor) else i2, np.float64)
    th = np.atleast_2d(np.asarray(th, np.float64))
    box = np.asarray(box, np.float64)
    q, d = ii.shape
    assert tb.shape == (q, d, npad) and th.shape[0] == q and box.shape == (2, d), (tb.shape, ii.shape, th.shape, box.shape)
    xr = rounded(x, dtype)[:n]
    one = np.float64(1.0).view(np.int64)
    best = Check(0.0, ())
    for k in range(q):
        for l in range(d):
            lo, hi, ell = box[0, l], box[1, l], th[k, l]
            pad = tb[k, l, n:].view(np.int64) != one
            if pad.any():
                return Check(math.inf, (k, l, (n + int(np.argmax(pad))) // TS))
            r = marg_table_ratios(kernel, tb[k, l, :n], xr[:, l], lo, hi, ell)
            j = int(np.argmax(r))
            if r[j] > best.ratio:
                best = Check(float(r[j]), (k, l, j // TS))
            with mp.workdps(MARG_DPS + 10):
                e2 = float(abs(mp.mpf(float(ii[k, l])) - marg_exact2(kernel, mp.mpf(float(hi)) - mp.mpf(float(lo)), ell))) \
                    if math.isfinite(ii[k, l]) else math.inf
            r2 = e2 / (C * marg_i2_bound(kernel, hi - lo, ell) + floor("float64", 1))
            if r2 > best.ratio:
                best = Check(float(r2), (k, l, "i2"))
    return best


def marg_table_ratios(kernel, got, xv, lo, hi, ell):
    """|got - I1| / (C marg_table_bound + floor (1 + ell / w)) per value of xv (float64 arrays; NaN counts as inf): the ratios of
    check_marg_table for one (component, dimension), also for a restatement evaluated on a grid"""
    err = _mp_err(got, marg_exact(kernel, xv, lo, hi, ell))
    bound = C * marg_table_bound(kernel, xv, lo, hi, ell) + floor("float64", 1) * (1.0 + float(ell) / (float(hi) - float(lo)))
    r = err / bound
    r[np.isnan(r)] = math.inf
    return r


def marg_floor_fraction(x, th, box, kernel, dtype):
    """the fraction of the table entries (n x d, one theta row) whose bound is set by the absolute floor, not by the terms of
    marg_table_bound (the CPU tests hold it below 1 % in the default-box and sub-box cases)"""
    xr = rounded(x, dtype)
    th = np.asarray(th, np.float64)
    cnt = 0
    for l in range(xr.shape[1]):
        lo, hi, ell = box[0][l], box[1][l], th[l]
        cnt += int(np.sum(C * marg_table_bound(kernel, xr[:, l], lo, hi, ell) < floor("float64", 1) * (1.0 + ell / (hi - lo))))
    return cnt / xr.size


def _marg_cross_ref(tab, x0, mask, x2, colscale, th, kernel, dtype, dev):
    """(ref, bound weight E', cut) of the masked rows: ref_ij = scale (1 - nt) C0_kept(x0_i, x2_j) prod_{l in mask_i} tab[l, j]
    cs_j in float64 from the LIBRARY'S table (d x n2pad) and the rounded x0, x2, colscale; E' = E of kernel_parts over the KEPT
    dimensions of the row + 4 + the number of masked dimensions.  x0 under the mask is never read (np.where first)."""
    mask = np.asarray(mask) != 0
    n0, d = mask.shape
    x2r = rounded(x2, dtype)
    n2 = x2r.shape[0]
    x0r = rounded(np.where(mask, 0.0, np.asarray(x0, np.float64)), dtype)
    ell, scale, nug, D, _ = split_theta(th, d)
    nt = nug / (1.0 + nug)
    tb = _t(tab, dev)[:, :n2]
    cs = _t(rounded(np.ones(n2) if colscale is None else colscale, dtype), dev)
    ref = torch.zeros(n0, n2, dtype=torch.float64, device=dev)
    ew = torch.zeros_like(ref)
    cut = torch.zeros(n0, n2, dtype=torch.bool, device=dev)
    pats, inv = np.unique(mask, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    for pi, pat in enumerate(pats):
        rows = np.nonzero(inv == pi)[0]
        keep = np.nonzero(~pat)[0]
        c0, e, ct = kernel_parts(x0r[rows][:, keep], x2r[:, keep], ell[keep], kernel, dtype, dev)
        prod = torch.ones(n2, dtype=torch.float64, device=dev)
        for l in np.nonzero(pat)[0]:
            prod = prod * tb[int(l)]
        ri = torch.as_tensor(rows, device=dev)
        ref[ri] = scale * (1.0 - nt) * c0 * (prod * cs)[None, :]
        ew[ri] = e + 4.0 + float(pat.sum())
        cut[ri] = ct
    return ref, ew, cut


def check_marg_cross(X, tab, x0, mask, x2, colscale, th, kernel, dtype, plain=None) -> Check:
    """the masked rows (X: n0 x n2, one component; the first slabs of the scratch against the training inputs with colscale = sr,
    or -- before OP_COND_CROSS overwrites them -- the view's rows against xn with colscale = None; never a nugget term) against
        X_ij = scale (1 - nt) [prod_{l kept} kappa(|x0_il - x2_jl| / ell_l)] [prod_{l in mask_i} tab[l, j]] cs_j
    in float64 from the library's OWN table tab (d x n2pad doubles of this component), the rounded x0, x2, colscale.  The kept
    dimensions go through kernel_parts restricted to them (E of its docstring with d := the number kept; the exponent is summed
    over kept dimensions only, and so is the cut-off); each masked dimension multiplies one table entry into poly: one rounding.
    Then scale (1 - nt), cs and the store as in check_cov_cross:      C (E_kept + 4 + #masked) u |X_ij|  (+ |X_ij| past the cut-off).
    Entries of x0 under the mask are never read here either: the tests pass NaN there, and a library that loads them returns NaN
    (ratio inf).  plain: the same rows from the plain path (lcgp_predict's X on x0 with zeros under the mask); every row with an
    EMPTY mask must equal it bitwise (ratio inf otherwise).  Locations: (row block, column block)."""
    dev = _dev(X)
    ref, ew, cut = _marg_cross_ref(tab, x0, mask, x2, colscale, th, kernel, dtype, dev)
    d = np.asarray(mask).shape[1]
    bound = C * ew * unit(dtype) * ref.abs() + torch.where(cut, ref.abs(), torch.zeros_like(ref)) + floor(dtype, d)
    got = _t(X, dev)
    c = worst((got - ref).abs(), bound, lower=False)
    if plain is not None:
        empty = torch.as_tensor(~(np.asarray(mask) != 0).any(axis=1), device=dev)
        a, b = got[empty].contiguous(), _t(plain, dev)[empty].contiguous()
        bad = a.view(torch.int64) != b.view(torch.int64)
        if bool(bad.any()):
            i, j = (int(v) for v in torch.nonzero(bad)[0])
            return Check(math.inf, (int(torch.nonzero(empty)[i]) // TS, j // TS))
    return c


def marg_prior(i2, mask, th):
    """the prior of marg_reduce_kernel per row (float64 numpy): scale (1 - nt) prod_{l in mask_i} i2[l] in ascending l from the
    library's own i2 (d doubles), or scale for a row with an empty mask"""
    mask = np.asarray(mask) != 0
    d = mask.shape[1]
    ell, scale, nug, D, _ = split_theta(th, d)
    pr = np.full(mask.shape[0], scale * (1.0 - nug / (1.0 + nug)))
    ii = np.asarray(i2, np.float64)
    for l in range(d):
        pr = np.where(mask[:, l], pr * ii[l], pr)
    return np.where(mask.any(axis=1), pr, scale)


def check_marg_out(ghat, gvar, X, U, z, i2, mask, th, dtype) -> Check:
    """ghat / gvar of lcgp_predict_marginal (n0 doubles each, one component) against
        ghat = X z,     gvar = prior - D rowsum(U o U),     prior = marg_prior (the nugget averages out; an empty mask: scale)
    in float64 from the library's own X, U (n0 x n), z (fetched) and i2.  marg_reduce_kernel converts the stored rows to double
    and sums n terms in double (64 lanes, then the butterfly); the prior is d products at most, the scaling by 1 - nug / (1 + nug)
    three roundings, D s2 and the difference two: gamma_{n + d} on the absolute terms, u = float64's in both storage types:
        C (n + d + 2) u64 (|X| |z|)_i + floor,      C (n + d + 2) u64 (|prior_i| + |D| |U_i|^2) + floor."""
    dev = _dev(ghat, gvar, X, U, z)
    xx, uu = _t(X, dev), _t(U, dev)
    n = xx.shape[1]
    zz = _t(z, dev)[:n]
    d = np.asarray(mask).shape[1]
    D = split_theta(th, d)[3]
    pr = _t(marg_prior(i2.cpu() if isinstance(i2, torch.Tensor) else i2, mask, th), dev)
    w = C * (n + d + 2.0) * unit("float64")
    fl = floor("float64", n)
    gref = xx @ zz
    gb = w * (xx.abs() @ zz.abs()) + fl
    u2 = (uu * uu).sum(dim=1)
    vref = pr - D * u2
    vb = w * (pr.abs() + abs(D) * u2) + fl
    return combine(worst((_t(ghat, dev) - gref).abs(), gb), worst((_t(gvar, dev) - vref).abs(), vb))


def check_marg_cond_cross(Sg, U0, Un, tabn, x0, mask, xn, th, kernel, dtype) -> Check:
    """check_cond_cross for the box-averaged view: Sigma_0n (n0 x m) after OP_COND_CROSS against
        Cbar^x(x0, xn) - D U_0 U_n^T
    with Cbar^x the reference of check_marg_cross from the FETCHED table over xn (tabn: d x mpad doubles), no colscale and no
    nugget, and the library's own U_0, U_n.  Bound as check_cond_cross with E' of the masked rows (E_kept + 4 + #masked):
        C (npad + d + E') u (|Cbar^x| + |D| |U_0| |U_n|^T)  (+ |Cbar^x| past the cut-off) + floor, on all entries."""
    dev = _dev(Sg, U0, Un)
    d = np.asarray(mask).shape[1]
    D = split_theta(th, d)[3]
    cx, ew, cut = _marg_cross_ref(tabn, x0, mask, xn, None, th, kernel, dtype, dev)
    u0, un = _t(U0, dev), _t(Un, dev)
    k = _pad128(un.shape[1])
    ref = cx - D * (u0 @ un.T)
    bound = C * (k + d + ew) * unit(dtype) * (cx.abs() + abs(D) * (u0.abs() @ un.abs().T)) + floor(dtype, k)
    bound = bound + torch.where(cut, cx.abs(), torch.zeros_like(cx))
    return worst((_t(Sg, dev) - ref).abs(), bound, lower=False)


def check_marg_refcov(gcov, U, T, ref, x0, mask, xr, mr, box, i2, th, kernel, dtype, n, m, ref_rows=None) -> Check:
    """gcov (n0 doubles, one component) of marg_refcov_kernel against
        gcov_i = prior(i, r) - D U_i . U_r - T_i . T_r,       [U_r | T_r] = ref (npad + mpad values; m = 0: no view, T ignored)
    in float64 from the library's own U (n0 x >= n), T (n0 x >= m), the widened row ref and i2 (d doubles), the rounded x0, xr
    (entries under their masks never read) and box (2 x d).  ref_rows = (U_r, T_r): the rows the widened row was copied from
    (padded as stored; T_r None without a view) -- ref must equal them BITWISE (ratio inf at ("ref",) otherwise).
    prior(i, r) = scale (1 - nt) prod_l f_l in ascending l: f_l = kappa(|x0_il - xr_l| / ell_l) where both rows keep l, the
    mpmath I1 (marg_exact) at the kept value where exactly one integrates l, the FETCHED i2[l] where both do.
    Counted from the source (double throughout): the two dot products are n and m fmas and the butterfly; D s1 and the two
    differences three; the prior d products and the three roundings of scale (1 - nt):
        C (n + m + d + 4) u64 (|prior| + |D| |U_i| . |U_r| + |T_i| . |T_r|)
    plus the factors' own errors, relative to |prior|: a mixed dimension carries marg_table_bound / I1 (the same marg_I1, on
    a query row's value); a kept-kept dimension the difference, the quotient, exp (MARG_ULP) and the polynomial (four), and the
    argument through b |kappa'(b)| / kappa(b) (b^2 / (1 + b), b^2, b^2 (1 + b) / (3 + 3 b + b^2)) with three roundings of b:
        C |prior| sum_l rel_l,     rel_l = u64 (MARG_ULP + 4 + 3 b |kappa'| / kappa)   or   marg_table_bound_l / I1_l.
    Locations: (64-block of the row,)."""
    _known(kernel)
    dev = _dev(gcov, U, T, ref)
    mask = np.asarray(mask) != 0
    mr = np.asarray(mr).reshape(-1) != 0
    n0, d = mask.shape
    npad = _pad128(n)
    rf = _t(ref, dev).reshape(-1)
    if ref_rows is not None:
        want = _t(ref_rows[0], dev).reshape(-1)[:npad]
        if m > 0:
            want = torch.cat([want, _t(ref_rows[1], dev).reshape(-1)[:_pad128(m)]])
        if want.shape != rf.shape or bool((want.contiguous().view(torch.int64) != rf.contiguous().view(torch.int64)).any()):
            return Check(math.inf, ("ref",))
    ell, scale, nug, D, _ = split_theta(th, d)
    u64 = unit("float64")
    x0r = rounded(np.where(mask, 0.0, np.asarray(x0, np.float64)), dtype)
    xrr = rounded(np.where(mr, 0.0, np.asarray(xr, np.float64).reshape(-1)), dtype)
    ii = np.asarray(i2.cpu() if isinstance(i2, torch.Tensor) else i2, np.float64)
    pr = np.full(n0, scale * (1.0 - nug / (1.0 + nug)))
    rel = np.zeros(n0)
    for l in range(d):
        both = mask[:, l] & mr[l]
        mixed = mask[:, l] ^ mr[l]
        kept = ~mask[:, l] & ~mr[l]
        f = np.ones(n0)
        f[both] = ii[l]
        if mixed.any():
            xv = np.full(n0, xrr[l]) if not mr[l] else x0r[:, l]
            i1 = marg_exact(kernel, xv[mixed], box[0][l], box[1][l], ell[l])
            f[mixed] = np.array([float(v) for v in i1])
            with np.errstate(divide="ignore", invalid="ignore"):
                r = marg_table_bound(kernel, xv[mixed], box[0][l], box[1][l], ell[l]) / f[mixed]
            rel[mixed] += np.where(np.isfinite(r), r, 0.0)
        if kept.any():
            b = np.abs(x0r[kept, l] - xrr[l]) / ell[l]
            f[kept] = _kappa(kernel, b)
            mag = b * b / (1.0 + b) if kernel == "matern32" else b * b if kernel == "se" \
                else b * b * (1.0 + b) / (3.0 + 3.0 * b + b * b)
            rel[kept] += u64 * (MARG_ULP + 4.0 + 3.0 * mag)
        pr = pr * f
    uu = _t(U, dev)[:, :n]
    ur = rf[:n]
    dots = uu @ ur
    adots = uu.abs() @ ur.abs()
    if m > 0:
        tt, tr = _t(T, dev)[:, :m], rf[npad:npad + m]
        tdot, atdot = tt @ tr, tt.abs() @ tr.abs()
    else:
        tdot = atdot = torch.zeros_like(dots)
    prt = _t(pr, dev)
    gref = prt - D * dots - tdot
    bound = C * (n + m + d + 4.0) * u64 * (prt.abs() + abs(D) * adots + atdot) + C * prt.abs() * _t(rel, dev) \
        + floor("float64", n + m)
    return worst((_t(gcov, dev) - gref).abs(), bound)


# ----------------------------------------------------------------------------------------------------------------------
# the two parameter-space queries: lcgp_nll_hess and lcgp_predict_paramgrad.  float64 only, so
# u = 2^-53 throughout.  Both leave every intermediate in their scratch (HessLay / PgradLay of lcgp_hip.hip, restated by
# hess_layout / pgrad_layout), so every stage is checked from the library's own input to it.  The references start from the
# library's own xs = x / ell (checked bitwise against one IEEE division in check_hess_prep).
#
# Evaluation constants, counted from the kernel text (units of u, relative unless stated):
#   C0 from xs (hess_c0, the row loop of pgrad_row_kernel): kernel_parts' E with the input-rounding term dropped -- xs is an
#     input here.  What is left: the difference df (one rounding of S_l, weight |d ln C0 / d ln S_l| <= S_l, S_l^2 for SE), the
#     d - 1 roundings of the exponent, the argument of exp and its ulp, the polynomial, the product:
#       matern32 (d + 1) sum S + d + 3,   matern52 (d + 1) sum S + 3 d + 3   (kernel_parts' counts),
#       se: 2 ssum (the differences) + d ssum (the fmas) + ssum + 1 (exp) <= (d + 3) ssum + 3,   ssum = 1/2 sum S^2.
#   phi (hess_phi), every factor positive, S carries the rounding of df with weight d ln phi / d ln S:
#       matern32  ie, S2, r = 1 / (1 + S) (2), S2 r ie (2), S (<= 2)                                              8
#       se        ie, S2, the product, S (2)                                                                      5
#       matern52  r = 1 / fma(fma) (3), N = S2 (1 + S) (3), N r ie (2), ie, S (<= 3)                             12
#   d phi (absolute, in units of u):
#       matern32  S2, fma, r r (5), ie ie (3), three products, S (<= 2)                         15 |dphi|
#       se        S2, 3 S2, ie ie (3), the product, S (2)                                         8 |dphi|
#       matern52  dphi = -(A + B) ie^2, A = S2 fma(3, S, 2) r > 0, B = N (3 - S2) r^2 changes sign at S = sqrt(3):
#                 A: S2, fma, r (4), two products, S (<= 3), the sum, ie ie and its product (4)        16 A ie^2
#                 B: N (3), its S (<= 3), r r (9) and its S (<= 4), 3 - S2 (absolute: 4 u (3 + S2)), two products, the
#                 sum, ie ie (4): 30 relative to N (3 + S2) r^2 -- the cancellation in 3 - S2 is not charged to B
#   d_iA = (D scale / (1 + nug)) (s_a s_b) C0 phi_i: the coefficient (3), s_a s_b, three products: E0 + PHI + 7.
# ----------------------------------------------------------------------------------------------------------------------
HS_B, HS_SLOTS, HS_JC, PP_DB = 4, 22, 8, 16            # lcgp_hip.hip
PHI_ROUND = {"matern32": 8.0, "se": 5.0, "matern52": 12.0}
DA_ROUND = 7.0
FLOOR_LOG = None          # a list while a test counts the entries whose bound the absolute floor sets: (stage, floored, entries)
_U64 = 2.0 ** -53


def gamma(k) -> float:
    """gamma_k = k u / (1 - k u) of the module docstring, u = 2^-53"""
    return k * _U64 / (1.0 - k * _U64)


def _align256(o) -> int:
    return (int(o) + 255) // 256 * 256


def _carve(sizes):
    """offsets in doubles, in order, each aligned to 256 bytes; 'total' in bytes"""
    lay, o = {}, 0
    for name, count in sizes:
        lay[name] = o // 8
        o = _align256(o + 8 * int(count))
    lay["total"] = o
    return lay


def hess_layout(n, d, p, qg):
    """hess_carve of lcgp_hip.hip: the element offsets of AI, E, G, xs, yv, uv, YP, Q, tp, cp, dot in the scratch of
    lcgp_nll_hess (doubles) and `total` in bytes (= lcgp_nll_hess_scratch_bytes)"""
    m, npad, ppad = d + 2, _pad128(n), _pad128(p)
    nb, nbk = npad // TS, -(-d // HS_B)
    npair, npb, mat = m * (m + 1) // 2, nbk * (nbk + 1) // 2, npad * npad
    lay = _carve([("ai", qg * mat), ("e", qg * mat), ("g", qg * m * mat), ("xs", qg * d * npad), ("yv", qg * m * npad),
                  ("uv", qg * m * npad), ("yp", ppad * npad), ("q", qg * ppad * npad), ("tp", qg * npair * nb),
                  ("cp", qg * npb * nb * HS_SLOTS), ("dot", qg * m * m)])
    lay.update(m=m, npad=npad, ppad=ppad, nb=nb, npair=npair, npb=npb, mat=mat)
    return lay


def pgrad_layout(n, d, p, qg, n0):
    """pgrad_carve of lcgp_hip.hip: X (then V), U (then T_j), E, xs, yv, YT, VY, rd, sums of lcgp_predict_paramgrad"""
    m, npad, ppad, n0p, n0r, nsum = d + 2, _pad128(n), _pad128(p), predict_pad(n0), _pad128(n0), 3 * d + 8
    lay = _carve([("x", qg * n0r * npad), ("u", qg * n0r * npad), ("e", qg * npad * npad), ("xs", qg * d * npad),
                  ("yv", qg * m * npad), ("yt", npad * ppad), ("vy", qg * n0r * ppad), ("rd", qg * d * n0r),
                  ("sum", qg * n0r * nsum)])
    lay.update(m=m, npad=npad, ppad=ppad, n0p=n0p, n0r=n0r, nsum=nsum, nb=npad // TS, mat=npad * npad, slab=n0r * npad)
    return lay


def tri_decode(t):
    r = int((math.sqrt(8.0 * t + 1.0) - 1.0) * 0.5)
    while (r + 1) * (r + 2) // 2 <= t:
        r += 1
    while r * (r + 1) // 2 > t:
        r -= 1
    return r, t - r * (r + 1) // 2


def _same_bits(a, b) -> bool:
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))


def _zero_bits(a) -> bool:
    return not bool(a.contiguous().view(torch.int64).any())


def _exact(ok, where) -> Check:
    return Check(0.0 if ok else math.inf, (where,))


def _blocks(pos):
    return tuple(int(v) // TS for v in pos)


def _pworst(stage, err, core, k, name=_blocks) -> Check:
    """worst err / (core + floor(k)) over every entry, located by name(index tuple)"""
    fl = floor("float64", k)
    if FLOOR_LOG is not None:
        FLOOR_LOG.append((stage, int((core < fl).sum()), int(core.numel())))
    if err.numel() == 0:
        return Check(0.0, ())
    r = err / (core + fl)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    idx = int(torch.argmax(r))
    return Check(float(r.reshape(-1)[idx]), name(np.unravel_index(idx, tuple(r.shape))))


def _phi_parts(S, ell, kernel):
    """phi = d log C0 / d ell, d phi / d ell of one dimension at S = |dx| / ell (hess_phi) and the ABSOLUTE error bounds of
    the library's evaluation of each in units of u (see the section comment)"""
    _known(kernel)
    ie, S2 = 1.0 / ell, S * S
    if kernel == "matern32":
        r = 1.0 / (1.0 + S)
        phi, dphi = S2 * r * ie, -S2 * (2.0 * S + 3.0) * r * r * ie * ie
        return phi, dphi, PHI_ROUND[kernel] * phi, 15.0 * dphi.abs()
    if kernel == "se":
        phi, dphi = S2 * ie, -3.0 * S2 * ie * ie
        return phi, dphi, PHI_ROUND[kernel] * phi, 8.0 * dphi.abs()
    r = 1.0 / (S2 + 3.0 * S + 3.0)
    N = S2 * (1.0 + S)
    A, B = S2 * (3.0 * S + 2.0) * r, N * (3.0 - S2) * r * r
    return N * r * ie, -(A + B) * ie * ie, PHI_ROUND[kernel] * N * r * ie, (16.0 * A + 30.0 * N * (3.0 + S2) * r * r) * ie * ie


def param_parts(xa, xb, ell, kernel):
    """C0 (na x nb), its evaluation magnification E0, and per dimension phi, dphi and their absolute error bounds (units of
    u), all from the SCALED inputs xa (d x na), xb (d x nb) -- the library's x / ell -- in float64 on their device"""
    _known(kernel)
    d = xa.shape[0]
    ssum = torch.zeros(xa.shape[1], xb.shape[1], dtype=torch.float64, device=xa.device)
    poly = torch.ones_like(ssum)
    S = []
    for l in range(d):
        s = (xa[l][:, None] - xb[l][None, :]).abs()
        S.append(s)
        if kernel == "se":
            ssum += 0.5 * s * s
        elif kernel == "matern32":
            ssum += s
            poly *= 1.0 + s
        else:
            ssum += s
            poly *= 1.0 + s + s * s / 3.0
    c0 = poly * torch.exp(-ssum)
    e0 = (d + 3.0) * ssum + 3.0 if kernel == "se" else (d + 1.0) * ssum + (d if kernel == "matern32" else 3.0 * d) + 3.0
    parts = [_phi_parts(S[l], float(ell[l]), kernel) for l in range(d)]
    return dict(c0=c0, e0=e0, phi=[q[0] for q in parts], dphi=[q[1] for q in parts], ephi=[q[2] for q in parts],
                edphi=[q[3] for q in parts])


def hess_parts(xs, sr, th, kernel, n):
    """what the checks of both queries share, from the library's xs (d x npad) of one component: param_parts on the n training
    inputs, s s^T, the coefficient of d_iA and dA(i) -> (d_iA, its relative evaluation error in units of u), n x n"""
    xs = _t(xs)
    d = xs.shape[0]
    ell, scale, nug, D, _ = split_theta(th, d)
    R = param_parts(xs[:, :n], xs[:, :n], ell, kernel)
    s = _t(np.ones(n) if sr is None else np.asarray(sr, np.float64), xs.device)
    R.update(n=n, d=d, npad=xs.shape[1], s=s, ss=s[:, None] * s[None, :], coef=D * scale / (1.0 + nug), kernel=kernel)
    R["dA"] = lambda i: (R["coef"] * R["ss"] * R["c0"] * R["phi"][i], R["e0"] + PHI_ROUND[kernel] + DA_ROUND)
    return R


def _padded(a, npad):
    out = torch.zeros(npad, npad, dtype=torch.float64, device=a.device)
    out[:a.shape[0], :a.shape[1]] = a
    return out


# ---- lcgp_nll_hess ---------------------------------------------------------------------------------------------------
def check_hess_prep(xs, yv, x, sr, th, b, z) -> Check:
    """hess_prep_kernel, from x, sr, theta and the fetched b, z of the component.  xs (d x npad): bitwise x / ell -- one IEEE
    division, so numpy gives the same bits -- dimension-major, bitwise zero on n .. npad.  yv rows d, d + 1:
        y_scale = (b - z) / scale: the difference and the quotient, 2 u (|b| + |z|) / scale;
        y_nug = (D scale s^2 z - (b - z)) / (1 + nug): D scale, s s, two products (4) on T1 = D scale s^2 |z|, the difference
        b - z (1) on |b| + |z|, then the subtraction, 1 + nug and the quotient (3) on both: u (7 T1 + 4 (|b| + |z|)) / (1 + nug);
    both bitwise zero on the padding.  Locations: the name of what failed, or (row, 64-block)."""
    x = np.asarray(x, np.float64)
    n, d = x.shape
    ell, scale, nug, D, _ = split_theta(th, d)
    xs, yv = _t(xs), _t(yv)
    dev, npad = xs.device, xs.shape[1]
    want = np.zeros((d, npad))
    want[:, :n] = (x / ell[None, :]).T
    if not _same_bits(xs.cpu(), torch.as_tensor(want)):
        return Check(math.inf, ("xs",))
    if not _zero_bits(yv[d:, n:]):
        return Check(math.inf, ("y padding",))
    bt, zt = _t(b, dev), _t(z, dev)
    s = _t(np.ones(n) if sr is None else np.asarray(sr, np.float64), dev)
    bz, mag = bt - zt, bt.abs() + zt.abs()
    t1 = D * scale * (s * s) * zt
    ref = torch.stack([bz / scale, (t1 - bz) / (1.0 + nug)])
    core = C * _U64 * torch.stack([2.0 * mag / scale, (7.0 * t1.abs() + 4.0 * mag) / (1.0 + nug)])
    return _pworst("hess_prep", (yv[d:, :n] - ref).abs(), core, 1, lambda pos: (("y_scale", "y_nug")[pos[0]], int(pos[1]) // TS))


def check_hess_mirror(AI, Gs, Gn, V, sr, th, n, d) -> Check:
    """hess_mirror_kernel.  AI (npad x npad): bitwise the mirror of the lower triangle of the fetched A^-1 (V, n x n), exactly
    symmetric, the identity on the padding.  From that AI, entry by entry (v = AI[a, b], dl = delta_ab):
        G_scale = (dl - v) / scale: two roundings, 2 u (dl + |v|) / scale;
        G_nug = (fma(c, v, v) - dl) / (1 + nug), c = D scale s_b^2 (three roundings), the fma, the subtraction, 1 + nug, the
        quotient: at most 7 u (dl + |v| (1 + c)) / (1 + nug) -- on the sum of the absolute terms, which does not shrink where
        A^-1 is close to I.  s_b is the COLUMN's s (G_nug = A^-1 d_nug A is not symmetric on the rep path).
    Both bitwise zero on the padding."""
    AI, Gs, Gn = _t(AI), _t(Gs), _t(Gn)
    dev, npad = AI.device, AI.shape[0]
    _, scale, nug, D, _ = split_theta(th, d)
    v = torch.tril(_t(V, dev))
    want = torch.eye(npad, dtype=torch.float64, device=dev)
    want[:n, :n] = v + torch.tril(v, -1).T
    if not _same_bits(AI, want) or not _same_bits(AI, AI.T):
        return Check(math.inf, ("AI",))
    for g in (Gs, Gn):
        if not (_zero_bits(g[n:, :]) and _zero_bits(g[:, n:])):
            return Check(math.inf, ("G padding",))
    v = AI[:n, :n]
    dl = torch.eye(n, dtype=torch.float64, device=dev)
    s = _t(np.ones(n) if sr is None else np.asarray(sr, np.float64), dev)
    c = (D * scale * s * s)[None, :]
    mag = dl + v.abs() * (1.0 + c)
    c1 = _pworst("hess_mirror", (Gs[:n, :n] - (dl - v) / scale).abs(), C * 2.0 * _U64 * (dl + v.abs()) / scale, 1,
                 lambda pos: ("G_scale",) + _blocks(pos))
    c2 = _pworst("hess_mirror", (Gn[:n, :n] - (c * v + v - dl) / (1.0 + nug)).abs(), C * 7.0 * _U64 * mag / (1.0 + nug), 1,
                 lambda pos: ("G_nug",) + _blocks(pos))
    return combine(c1, c2)


def check_hess_da(E, R, i) -> Check:
    """hess_da_kernel: E (npad x npad) = d_iA against coef s s^T o C0 o phi_i from xs, relative error (E0 + PHI + 7) u entry
    by entry over the FULL matrix; E exactly symmetric (df and -df give the same |df|; s_a s_b commutes) and bitwise zero on
    the padding.  (Its diagonal is exactly zero -- phi(0) = 0 -- and stands on the floor.)"""
    E = _t(E)
    n = R["n"]
    if not _same_bits(E, E.T):
        return Check(math.inf, ("E symmetry",))
    if not (_zero_bits(E[n:, :]) and _zero_bits(E[:, n:])):
        return Check(math.inf, ("E padding",))
    ref, e = R["dA"](i)
    return _pworst("hess_da", (E[:n, :n] - ref).abs(), C * _U64 * e * ref.abs(), 1)


def check_hess_y(yv, R, z, stage="hess_y") -> Check:
    """hess_matvec_kernel over d_iA: every y_i = d_iA z, i < d (yv: m x npad), against the reference d_iA from xs times the
    fetched z.  n fmas and the butterfly in some order (gamma_n, with the store n + 1) and the evaluation of d_iA:
        u sum_b (n + 1 + E0 + PHI + 7) |d_iA[a, b]| |z_b|.
    The rows n .. npad are bitwise zero (the rows of E there are).  Locations: (i, 64-block)."""
    yv = _t(yv)
    n, d = R["n"], R["d"]
    if not _zero_bits(yv[:d, n:]):
        return Check(math.inf, ("y padding",))
    zt = _t(z, yv.device)
    err, core = [], []
    for i in range(d):
        ref, e = R["dA"](i)
        err.append((yv[i, :n] - ref @ zt).abs())
        core.append(C * _U64 * (((n + 1.0) + e) * ref.abs()) @ zt.abs())
    return _pworst(stage, torch.stack(err), torch.stack(core), n, lambda pos: (int(pos[0]), int(pos[1]) // TS))


def check_hess_g(G, AI, E, R) -> Check:
    """OP_HESS_G: G_i = AI d_iA, i < d (G: >= d matrices npad x npad), entry by entry over the FULL matrix -- G is not symmetric.
    For i = d - 1 the operand is the fetched E (what the buffer holds after the call) and the bound is the product's alone,
    gamma_{n+1} |AI| |E| (the zero padding adds nothing, in any order of the k loop); for i < d - 1 the operand is the
    reference d_iA from xs and its evaluation error goes through |AI|: + u |AI| ((E0 + PHI + 7) |d_iA|).  The padding rows and
    columns are bitwise zero.  Locations: (i, row block, column block)."""
    G, AI, E = _t(G), _t(AI), _t(E)
    n, d, npad = R["n"], R["d"], R["npad"]
    worst_c = Check(0.0, ())
    aa = AI.abs()
    for i in range(d):
        if not (_zero_bits(G[i][n:, :]) and _zero_bits(G[i][:, n:])):
            return Check(math.inf, ("G padding", i))
        if i == d - 1:
            op, extra = E, None
        else:
            ref, e = R["dA"](i)
            op, extra = _padded(ref, npad), _padded(e * ref.abs(), npad)
        core = C * gamma(n + 1.0) * (aa @ op.abs())
        if extra is not None:
            core = core + C * _U64 * (aa @ extra)
        c = _pworst("hess_g", (G[i][:n, :n] - (AI @ op)[:n, :n]).abs(), core[:n, :n], n, lambda pos: (i,) + _blocks(pos))
        worst_c = combine(worst_c, c)
    return worst_c


def check_hess_trace(tp, G, n) -> Check:
    """hess_trace_kernel: every tp[pair(i, j <= i)][rb] = sum_{a in band rb} sum_b G_i[a, b] G_j[b, a] from the fetched G (all
    m matrices), pair(i, j) = i (i + 1) / 2 + j.  64 npad fmas and the workgroup sum in some order:
        gamma_{64 npad} sum_{a in rb, b} |G_i[a, b]| |G_j[b, a]|.
    A band entirely past n is exactly zero.  Locations: (i, j, rb)."""
    tp, G = _t(tp), _t(G)
    m, npad = G.shape[0], G.shape[1]
    nb, nlive = npad // TS, -(-n // TS)
    worst_c = Check(0.0, ())
    for i in range(m):
        prod = G[:i + 1].transpose(1, 2) * G[i][None]                     # [j, a, b] = G_i[a, b] G_j[b, a]
        ref = prod.reshape(i + 1, nb, TS * npad).sum(dim=2)
        ab = prod.abs().reshape(i + 1, nb, TS * npad).sum(dim=2)
        got = tp[i * (i + 1) // 2:i * (i + 1) // 2 + i + 1]
        if bool((got[:, nlive:] != 0).any()):
            return Check(math.inf, ("trace padding band", i))
        c = _pworst("hess_trace", (got - ref).abs()[:, :nlive], C * gamma(64.0 * npad) * ab[:, :nlive], 64 * npad,
                    lambda pos: (i, int(pos[0]), int(pos[1])))
        worst_c = combine(worst_c, c)
    return worst_c


def _bands(M, nb):
    """sums over the 64-row bands of an n x n matrix -> nb values (the bands past n are zero)"""
    out = torch.zeros(nb * TS, dtype=torch.float64, device=M.device)
    out[:M.shape[0]] = M.sum(dim=1)
    return out.reshape(nb, TS).sum(dim=1)


def check_hess_contract(cp, AI, R, z, th) -> Check:
    """hess_contract_kernel: the slots of cp (npb x nb x 22) per block pair pb = (bi, bj <= bi) and band rb, from AI, xs, the
    fetched z, sr and theta.  With g = s_a s_b (D/2 AI - z_a z_b / 2), |g|_abs = s_a s_b (D/2 |AI| + |z_a z_b| / 2) (the
    product s_a s_b, D/2 AI, z_a z_b, the subtraction: 4), w0 = g C0 (E0 + 1) and K = 64 n + 8 (the 64 n fmas of a band and
    the workgroup sum in some order, the 4 + 1 of w0, the product / fma of k2 and the fma into the accumulator):
        slot ii 4 + jj, i = 4 bi + ii, j = 4 bj + jj < d:   sum w0 (phi_i phi_j + [i = j] dphi_i)
            u sum |g|_abs C0 [ (K + E0) |phi_i phi_j| + ephi_i |phi_j| + |phi_i| ephi_j + [i = j] ((K + E0) |dphi_i| + edphi_i) ]
        slot 16 + ii (bj = 0, what hess_final_kernel reads), slot 20 (pb = 0): sum w0 phi_i, sum w0, likewise
        slot 21 (pb = 0): trace g, K u sum |g|_abs on the diagonal.
    On the diagonal block pair the slots jj > ii, which hess_final_kernel does not read, are checked all the same.  The
    second-order slots of a dimension past d are bitwise +0.  Locations: (pb, slot, rb)."""
    cp, AI = _t(cp), _t(AI)
    n, d, dev = R["n"], R["d"], AI.device
    _, scale, nug, D, _ = split_theta(th, d)
    npb, nb = cp.shape[0], cp.shape[1]
    nlive = -(-n // TS)
    zt = _t(z, dev)
    zz = zt[:, None] * zt[None, :]
    g = R["ss"] * (0.5 * D * AI[:n, :n] - 0.5 * zz)
    gabs = R["ss"] * (0.5 * D * AI[:n, :n].abs() + 0.5 * zz.abs())
    W0 = gabs * R["c0"]
    w0 = g * R["c0"]
    K = 64.0 * n + 8.0
    ke = K + R["e0"]
    phi, dphi, ephi, edphi = R["phi"], R["dphi"], R["ephi"], R["edphi"]
    refs, cores, names = [], [], []
    for pb in range(npb):
        bi, bj = tri_decode(pb)
        for ii in range(HS_B):
            for jj in range(HS_B):
                li, lj, slot = bi * HS_B + ii, bj * HS_B + jj, ii * HS_B + jj
                if li >= d or lj >= d:
                    if not _zero_bits(cp[pb, :, slot]):
                        return Check(math.inf, ("slot past d", pb, slot))
                    continue
                t = phi[li] * phi[lj]
                val, mag = t, ke * t.abs() + ephi[li] * phi[lj].abs() + phi[li].abs() * ephi[lj]
                if li == lj:
                    val, mag = t + dphi[li], mag + ke * dphi[li].abs() + edphi[li]
                refs.append(_bands(w0 * val, nb))
                cores.append(_bands(W0 * mag, nb))
                names.append((pb, slot))
        if bj == 0:
            for ii in range(HS_B):
                li = bi * HS_B + ii
                if li < d:
                    refs.append(_bands(w0 * phi[li], nb))
                    cores.append(_bands(W0 * (ke * phi[li].abs() + ephi[li]), nb))
                    names.append((pb, 16 + ii))
        if pb == 0:
            refs.append(_bands(w0, nb))
            cores.append(_bands(W0 * ke, nb))
            names.append((0, 20))
            refs.append(_bands(torch.diag(torch.diagonal(g)), nb))
            cores.append(K * _bands(torch.diag(torch.diagonal(gabs)), nb))
            names.append((0, 21))
    got = torch.stack([cp[pb, :, slot] for pb, slot in names])
    if bool((got[:, nlive:] != 0).any()):
        return Check(math.inf, ("contract padding band",))
    return _pworst("hess_contract", (got - torch.stack(refs)).abs()[:, :nlive], C * _U64 * torch.stack(cores)[:, :nlive], 64 * n,
                   lambda pos: names[int(pos[0])] + (int(pos[1]),))


def check_hess_vectors(uv, dot, YP, Q, AI, yv, Y, n) -> Check:
    """u_i = AI y_i for all m vectors (hess_matvec_kernel; gamma_{n+1} |AI| |y_i|, all npad rows), the m^2 dot[i, j] = y_i . u_j
    (hess_dot_kernel; gamma_{n+1} |y_i| . |u_j|), YP bitwise Y zero padded to ppad x npad (hess_pack_y_kernel) and Q = YP AI
    entry by entry (OP_HESS_G; gamma_{n+1} |YP| |AI|), each from the fetched operands.  Locations: (what, ...)."""
    uv, dot, YP, Q, AI, yv = _t(uv), _t(dot), _t(YP), _t(Q), _t(AI), _t(yv)
    dev = AI.device
    Yt = _t(Y, dev)
    p = Yt.shape[0]
    want = torch.zeros_like(YP)
    want[:p, :n] = Yt
    if not _same_bits(YP, want):
        return Check(math.inf, ("YP",))
    if bool((Q[p:, :] != 0).any()) or bool((Q[:, n:] != 0).any()) or bool((uv[:, n:] != 0).any()):
        return Check(math.inf, ("Q / u padding",))
    g = C * gamma(n + 1.0)
    c1 = _pworst("hess_vectors", (uv - yv @ AI.T).abs()[:, :n], g * (yv.abs() @ AI.abs().T)[:, :n], n,
                 lambda pos: ("u", int(pos[0]), int(pos[1]) // TS))
    c2 = _pworst("hess_vectors", (dot - yv @ uv.T).abs(), g * (yv.abs() @ uv.abs().T), n,
                 lambda pos: ("dot", int(pos[0]), int(pos[1])))
    c3 = _pworst("hess_vectors", (Q - YP @ AI).abs()[:p, :n], g * (YP.abs() @ AI.abs())[:p, :n], n,
                 lambda pos: ("Q", int(pos[0]), int(pos[1]) // TS))
    return combine(c1, c2, c3)


def hess_final_ref(tp, cp, dot, th, d):
    """hess_final_kernel term by term in float64 numpy from the fetched tp (npair x nb), cp (npb x nb x 22), dot (m x m):
    (hk (m x m, lower), the bound's sum of absolute terms |T| (m x m), 1/2 sum_rb |tp| (m x m))"""
    tp, cp, dot = (np.asarray(_t(a).cpu(), np.float64) for a in (tp, cp, dot))
    m = d + 2
    _, scale, nug, D, _ = split_theta(th, d)
    omw = 1.0 / (1.0 + nug)
    w1 = omw * omw
    ssum, sabs = cp.sum(axis=1), np.abs(cp).sum(axis=1)
    hk, Ta, tra = np.zeros((m, m)), np.zeros((m, m)), np.zeros((m, m))
    for i in range(m):
        for j in range(i + 1):
            if i < d:
                pb, slot = (i // HS_B) * (i // HS_B + 1) // 2 + j // HS_B, (i % HS_B) * HS_B + j % HS_B
                T, A = scale * omw * ssum[pb, slot], scale * omw * sabs[pb, slot]
            elif j < d:
                pb, slot = (j // HS_B) * (j // HS_B + 1) // 2, 16 + j % HS_B
                cf = omw if i == d else -scale * w1
                T, A = cf * ssum[pb, slot], abs(cf) * sabs[pb, slot]
            else:
                dd, da = ssum[0, 21] - ssum[0, 20], sabs[0, 21] + sabs[0, 20]
                cf = 0.0 if i == d else (w1 if j == d else -2.0 * scale * w1 * omw)
                T, A = cf * dd, abs(cf) * da
            t = i * (i + 1) // 2 + j
            hk[i, j] = (T - 0.5 * tp[t].sum()) + dot[i, j] / D
            Ta[i, j], tra[i, j] = A, 0.5 * np.abs(tp[t]).sum()
    return hk, Ta, tra


def check_hess_out(out_row, YP, uv, Q, b, z, tp, cp, dot, th, n, d, p) -> Check:
    """the row of `out` of one component, [hk (m x m) | hx (m x p) | hn (p x p)], from the fetched intermediates.
      hx[i, a] = psi_a (Y_a . u_i) / (2 D) (hess_cross_kernel): the dot product and three roundings,
          (n + 4) u |psi_a| |Y_a| . |u_i| / (2 D).
      hn[a, b] = -(delta_ab psi_a Y_a . (b - z) + psi_a psi_b Y_a . (Y_b - Q_b)) / (4 D) (hess_noise_kernel) from YP, Q, b, z: the
          differences are formed before the products, so the sums of absolute terms are |Y_a| . |Y_b - Q_b| and |Y_a| . |b - z|
          -- the cancellation of I - A^-1 is not charged; gamma_{n+2} and the five roundings of the combination: n + 6.
      hk[i, j] (hess_final_kernel) from tp, cp, dot: the band sums are nb roundings each; the coefficient of T at most 9 (omw two,
          w1 four, the products), the difference of slots 21 and 20 one, T - tr / 2, dot / D and the sum three:
          u [ (nb + 14) |T|_abs + (nb + 2) 1/2 sum_rb |tp| + 3 |dot| / D ],   |T|_abs = |coefficient| sum_rb |cp slot|.
      Both triangles of hk are bitwise equal.  Locations: (block, i, j)."""
    row = _t(out_row).reshape(-1)
    dev = row.device
    m = d + 2
    _, scale, nug, D, psi = split_theta(th, d)
    hk, hx, hn = row[:m * m].reshape(m, m), row[m * m:m * m + m * p].reshape(m, p), row[m * m + m * p:].reshape(p, p)
    if not _same_bits(hk, hk.T):
        return Check(math.inf, ("hk symmetry",))
    YP, uv, Q = _t(YP, dev)[:p, :n], _t(uv, dev)[:, :n], _t(Q, dev)[:p, :n]
    ps = _t(psi, dev)
    c1 = _pworst("hess_out", (hx - (uv @ YP.T) * ps[None, :] / (2.0 * D)).abs(),
                 C * _U64 * (n + 4.0) * (uv.abs() @ YP.abs().T) * ps.abs()[None, :] / (2.0 * D), n,
                 lambda pos: ("hx", int(pos[0]), int(pos[1])))
    bz = _t(b, dev) - _t(z, dev)
    dif = YP - Q
    pp = ps[:, None] * ps[None, :]
    ref = -(torch.diag(ps * (YP @ bz)) + pp * (YP @ dif.T)) / (4.0 * D)
    core = C * _U64 * (n + 6.0) * (torch.diag(ps.abs() * (YP.abs() @ bz.abs())) + pp.abs() * (YP.abs() @ dif.abs().T)) / (4.0 * D)
    c2 = _pworst("hess_out", (hn - ref).abs(), core, n, lambda pos: ("hn", int(pos[0]), int(pos[1])))
    nb = _t(tp).shape[1]
    kref, Ta, tra = hess_final_ref(tp, cp, dot, th, d)
    core = C * _U64 * ((nb + 14.0) * Ta + (nb + 2.0) * tra + 3.0 * np.abs(np.asarray(_t(dot).cpu())) / D)
    il = np.tril_indices(m)
    c3 = _pworst("hess_out", torch.as_tensor(np.abs(np.asarray(hk.cpu()) - kref)[il]), torch.as_tensor(core[il]), nb,
                 lambda pos: ("hk", int(il[0][pos[0]]), int(il[1][pos[0]])))
    return combine(c1, c2, c3)


# ---- lcgp_predict_paramgrad --------------------------------------------------------------------------------------------
# X, U, ghat, gvar, V are bitwise those of lcgp_predict_grad (check_cov_u, check_pgrad_v, check_predict cover them); xs, y_scale,
# y_nug, E and the y_j go through check_hess_prep, check_hess_da and check_hess_y.
def check_pp_y(yv, R, z) -> Check:
    """y_j = d_jA z for every j < d of lcgp_predict_paramgrad: check_hess_y (the same two launches per dimension)"""
    return check_hess_y(yv, R, z, "pp_y")


def check_pp_t(T, V, E, n0, n) -> Check:
    """the U slab after the call: T_{d-1} = V d_{d-1}A (OP_HESS_G) on the rows < n0, from the fetched V (n0 x >= n) and E:
    gamma_{n+1} |V| |E|.  Locations: (row block, column block)."""
    T, V, E = _t(T)[:n0, :n], _t(V)[:n0, :n], _t(E)[:n, :n]
    return _pworst("pp_t", (T - V @ E).abs(), C * gamma(n + 1.0) * (V.abs() @ E.abs()), n)


def check_pp_rowdot(rd, T, V, R, n0) -> Check:
    """rd[j][i] = V_i (d_jA) V_i^T (pgrad_rowdot_kernel over T_j = V d_jA).  For j = d - 1 from the fetched T and V:
    gamma_{n+1} |T_i| . |V_i|.  For the other j, whose T_j is overwritten, from V and the reference d_jA of xs: the product and
    the dot, n + 1 each, and the evaluation of d_jA: u sum_bc |V_ib| (2 n + 2 + E0 + PHI + 7) |d_jA_bc| |V_ic|.
    Locations: (j, 64-block of i)."""
    n, d = R["n"], R["d"]
    rd, V = _t(rd)[:, :n0], _t(V)[:n0, :n]
    T = _t(T, V.device)[:n0, :n]
    err, core = [], []
    for j in range(d):
        if j == d - 1:
            ref, bnd = (T * V).sum(dim=1), C * gamma(n + 1.0) * (T.abs() * V.abs()).sum(dim=1)
        else:
            dA, e = R["dA"](j)
            ref = ((V @ dA) * V).sum(dim=1)
            bnd = C * _U64 * ((V.abs() @ ((2.0 * n + 2.0 + e) * dA.abs())) * V.abs()).sum(dim=1)
        err.append((rd[j] - ref).abs())
        core.append(bnd)
    return _pworst("pp_rowdot", torch.stack(err), torch.stack(core), n * n, lambda pos: (int(pos[0]), int(pos[1]) // TS))


def pp_sum_names(d):
    return ["dz%d" % j for j in range(d)] + ["dv%d" % j for j in range(d)] + ["xz", "xv", "rz", "rv", "vv", "s2vv"] \
        + ["vy%d" % j for j in range(d)] + ["vy_scale", "vy_nug"]


def check_pp_sums(sums, x0, xs, z, V, yv, sr, th, kernel, same, n0, n) -> Check:
    """pgrad_row_kernel: all 3 d + 8 sums of every row i < n0, [dz_j | dv_j | Xc.z, Xc.v, rz, rv, |v|^2, sum s^2 v^2 | v.y_t],
    from x0, the library's xs, the fetched z, V (n0 x >= n), yv (m x npad), sr, theta.  x0 / ell is one IEEE division (the same
    bits here); Xc = (scale / (1 + nug)) C0 s: the coefficient two, C0 E0, two products: E0 + 4.  Every sum is n fmas and the
    workgroup sum in some order (n + 1 with the store) on the sum of its absolute terms:
        dz_j, dv_j: Xc phi_j and its product:  (n + 2 + E0 + 4) |Xc phi_j w| + |Xc| ephi_j |w|,   w = z, v
        Xc.z, Xc.v:  (n + 1 + E0 + 4) |Xc w|;     |v|^2, v.y_t:  n + 1;     sum s^2 v^2:  n + 3 (s s, its product with v)
        rz, rv: ONE rounding of s z, s v at c* = i + same - 1 (the other 255 threads add exact zeros), and exactly 0 with same = 0.
    Locations: (name of the sum, 64-block of i)."""
    sums, V, yv, xs = _t(sums)[:n0], _t(V)[:n0, :n], _t(yv)[:, :n], _t(xs)[:, :n]
    dev = sums.device
    x0 = np.asarray(x0, np.float64)
    d = x0.shape[1]
    ell, scale, nug, D, _ = split_theta(th, d)
    P = param_parts(_t((x0 / ell[None, :]).T.copy(), dev), xs, ell, kernel)
    s = _t(np.ones(n) if sr is None else np.asarray(sr, np.float64), dev)
    zt = _t(z, dev)
    xc = (scale / (1.0 + nug)) * P["c0"] * s[None, :]
    ex = P["e0"] + 4.0
    za, va = zt.abs()[None, :], V.abs()
    ref, core = [], []
    for w, wa in ((zt[None, :], za), (V, va)):
        for j in range(d):
            t = xc * P["phi"][j]
            ref.append((t * w).sum(dim=1))
            core.append((((n + 2.0) + ex) * t.abs() * wa + xc.abs() * P["ephi"][j] * wa).sum(dim=1))
    for w, wa in ((zt[None, :], za), (V, va)):
        ref.append((xc * w).sum(dim=1))
        core.append((((n + 1.0) + ex) * xc.abs() * wa).sum(dim=1))
    rz, rv = torch.zeros(n0, dtype=torch.float64, device=dev), torch.zeros(n0, dtype=torch.float64, device=dev)
    if same > 0:
        cs = torch.arange(n0, device=dev) + same - 1
        rz, rv = s[cs] * zt[cs], s[cs] * V[torch.arange(n0, device=dev), cs]
    ref += [rz, rv, (V * V).sum(dim=1), (s * s * V * V).sum(dim=1)]
    core += [rz.abs(), rv.abs(), (n + 1.0) * (V * V).sum(dim=1), (n + 3.0) * (s * s * V * V).sum(dim=1)]
    ref += [(V * yv[j][None, :]).sum(dim=1) for j in range(d + 2)]
    core += [(n + 1.0) * (va * yv[j].abs()[None, :]).sum(dim=1) for j in range(d + 2)]
    ref, core = torch.stack(ref, dim=1), C * _U64 * torch.stack(core, dim=1)
    if same <= 0 and not _zero_bits(sums[:, 2 * d + 2:2 * d + 4]):
        return Check(math.inf, ("rz / rv with same = 0",))
    names = pp_sum_names(d)
    keep = [c for c in range(3 * d + 8) if same > 0 or c not in (2 * d + 2, 2 * d + 3)]
    return _pworst("pp_sums", (sums - ref).abs()[:, keep], core[:, keep], n, lambda pos: (names[keep[int(pos[1])]], int(pos[0]) // TS))


def check_pp_vy(YT, VY, V, Y, n0, n) -> Check:
    """YT bitwise Y^T zero padded to npad x ppad (pgrad_pack_yt_kernel) and VY = V YT on the rows < n0 and columns < p
    (OP_HESS_G): gamma_{n+1} |V| |YT|.  Locations: (row block, column block)."""
    YT, VY, V = _t(YT), _t(VY), _t(V)[:n0, :n]
    Yt = _t(Y, YT.device)
    p = Yt.shape[0]
    want = torch.zeros_like(YT)
    want[:n, :p] = Yt.T
    if not _same_bits(YT, want):
        return Check(math.inf, ("YT",))
    return _pworst("pp_vy", (VY[:n0, :p] - V @ YT[:n, :p]).abs(), C * gamma(n + 1.0) * (V.abs() @ YT[:n, :p].abs()), n)


def check_pp_out(dghat, dgvar, dnoise, sums, rd, VY, th, d, p, n0) -> Check:
    """pgrad_final_kernel term by term from the fetched sums (n0 x nsum), rd (d x >= n0), VY (>= n0 x >= p); omw = 1 / (1 + nug)
    (two roundings), nt = nug omw (3), w1 = omw^2 (5); X.w = fma(scale nt, r_w, Xc.w) (5 on the nugget term):
        dghat_j = dz_j - v.y_j:                          u (|dz_j| + |v.y_j|)
        dgvar_j = -D (2 dv_j - rd_j):                    2 u D (2 |dv_j| + |rd_j|)
        dghat_scale = X.z / scale - v.y_scale:           8 u (|X.z|_abs / scale + |v.y_scale|)
        dgvar_scale = 1 - D (X.v + |v|^2) / scale:       9 u (1 + D (|X.v|_abs + |v|^2) / scale)
        dghat_nug = fma(scale w1, rz, -Xc.z omw) - v.y_nug:          8 u (|scale w1 rz| + |Xc.z omw| + |v.y_nug|)
        dgvar_nug = -D (2 A - B omw), A = fma(scale w1, rv, -Xc.v omw), B = D scale s2vv - (X.v - |v|^2):
                                                         13 u D (2 |A|_abs + (D scale |s2vv| + |X.v|_abs + |v|^2) omw)
        dghat_noise_a = -psi_a VY_a / 2:                 2 u |psi_a VY_a| / 2
    with C = 4 on top.  Locations: (output, column, 64-block of i)."""
    sums = _t(sums)[:n0]
    dev = sums.device
    m = d + 2
    _, scale, nug, D, psi = split_theta(th, d)
    omw = 1.0 / (1.0 + nug)
    nt, w1 = nug * omw, omw * omw
    rd, VY = _t(rd, dev)[:, :n0].T, _t(VY, dev)[:n0, :p]
    dg, dv, dn = _t(dghat, dev).reshape(n0, m), _t(dgvar, dev).reshape(n0, m), _t(dnoise, dev).reshape(n0, p)
    dz, dvs, vy = sums[:, :d], sums[:, d:2 * d], sums[:, 2 * d + 6:3 * d + 6]
    xcz, xcv, rz, rv, vv, s2vv = (sums[:, 2 * d + c] for c in range(6))
    vys, vyn = sums[:, 3 * d + 6], sums[:, 3 * d + 7]
    xz, xv = scale * nt * rz + xcz, scale * nt * rv + xcv
    xza, xva = abs(scale * nt) * rz.abs() + xcz.abs(), abs(scale * nt) * rv.abs() + xcv.abs()
    A = scale * w1 * rv - xcv * omw
    Aa = abs(scale * w1) * rv.abs() + xcv.abs() * omw
    rg = torch.cat([dz - vy, (xz / scale - vys)[:, None], (scale * w1 * rz - xcz * omw - vyn)[:, None]], dim=1)
    cg = torch.cat([dz.abs() + vy.abs(), 8.0 * (xza / scale + vys.abs())[:, None],
                    8.0 * (abs(scale * w1) * rz.abs() + xcz.abs() * omw + vyn.abs())[:, None]], dim=1)
    rv_ = torch.cat([-D * (2.0 * dvs - rd), (1.0 - D * (xv + vv) / scale)[:, None],
                     (-D * (2.0 * A - (D * scale * s2vv - (xv - vv)) * omw))[:, None]], dim=1)
    cv = torch.cat([2.0 * D * (2.0 * dvs.abs() + rd.abs()), 9.0 * (1.0 + D * (xva + vv.abs()) / scale)[:, None],
                    13.0 * D * (2.0 * Aa + (D * scale * s2vv.abs() + xva + vv.abs()) * omw)[:, None]], dim=1)
    ps = _t(psi, dev)
    c1 = _pworst("pp_out", (dg - rg).abs(), C * _U64 * cg, 1, lambda pos: ("dghat", int(pos[1]), int(pos[0]) // TS))
    c2 = _pworst("pp_out", (dv - rv_).abs(), C * _U64 * cv, 1, lambda pos: ("dgvar", int(pos[1]), int(pos[0]) // TS))
    c3 = _pworst("pp_out", (dn + 0.5 * ps[None, :] * VY).abs(), C * _U64 * 2.0 * (0.5 * ps[None, :] * VY).abs(), 1,
                 lambda pos: ("dghat_noise", int(pos[1]), int(pos[0]) // TS))
    return combine(c1, c2, c3)


# ----------------------------------------------------------------------------------------------------------------------
# Sobol pair sums (lcgp_sobol_pairs, lcgp_sobol_subset_pairs): sobol_table_kernel (the table is marg_I1:
# check_marg_table's bound; the box means) -> sobol_pair_kernel / sobol_pair_wide_kernel / sobol_subset_kernel (the tile sums
# part[pair, r, c, s]) -> sobol_reduce_kernel / sobol_subset_reduce_kernel (out).  Float64 only.
#
#   sobol_means    means[k] against sum_i w_ki prod_l tab from the LIBRARY'S table: gamma_(d + n) on the absolute sum
#   sobol_element  one-hot weights w_k = e_(i_k): the row of pair (k, k') is (M_u - M_0)[i_k, i_k'] of ONE element, every other
#                  element enters as fma(0, finite, acc); each column against mpmath (sobol_exact_J, marg_exact)
#   sobol_tile     every part[pair, r, c, s] against twice sum_tile wgt (M_u - M_0) from the library's table, the caller's w
#                  and J of tests/sobol_ref.py (which sobol_element's constants tie to mpmath)
#   sobol_reduce   out against the sum of the library's own part
#
# The bound of an element is relative to M_u + M_0, not to M_u - M_0: the kernel forms the two products and subtracts them, so
# what it can promise is u E_u M_u + u E_0 M_0 (E: the error constants of the factors and the multiplications), and the
# difference of two nearly equal products keeps that absolute error.  Constants:
#   a_l     the relative form of marg_table_bound (the 1-D average, against mpmath), per element
#   J_l SE  derived below from sobol_dim / sobol_J (_sobol_se_bound), with the input-conditioning terms
#   J_l Matern  SOBOL_KJ: no short derivation covers the 30-term chain, the two recurrences and the three segments, so the
#           constant is the worst error of the REFERENCE tests/sobol_ref.pair_integral against mpmath over sobol_cases, in units
#           of u relative to J, per kernel and per branch class (outer / middle segment x series / forward recurrence), measured
#           on the CPU (profiles/stage_bounds_sobol.txt, "reference against mpmath"; tests/test_sobol_bounds_cpu.py re-measures
#           and asserts the figures do not exceed the constants).  With the file's C = 4 that is four times the reference's error.
#           The device's own ratios go to the same file and set nothing.
#   products  M_0 is d multiplications (pa of sobol_pair_kernel, m0 of the wide kernel, sobol_subset_product(0): factors d .. DD - 1
#           are exactly 1).  M_u: sobol_pair_kernel forms a prefix of l, the factor, a suffix of d - 1 - l and their product:
#           d + 1 for a single input or its complement, d for all inputs; the wide kernel d; sobol_subset_product d.  All are at
#           most |u| + d, the count used.  One rounding for a_l a'_l per input, one for the difference, one for the fma.
# ----------------------------------------------------------------------------------------------------------------------
SOBOL_BATCH = 64                # lcgp_hip.hip: pairs per launch
SOBOL_CHUNK = 32                # sobol_subset.h sobol_subset_chunk(): masks per launch, both instances
SOBOL_SERIES_BELOW = 4.0        # lcgp_hip.hip: gamma L below it the 30-term series, from it on the forward recurrence
SOBOL_DPS = 40
# worst |pair_integral - exact| / (u exact) over sobol_cases on the two boxes [0, 1] and [0.3, 0.75], per (kernel, segment kind,
# branch), rounded up to an integer; the measured figures stand in profiles/stage_bounds_sobol.txt ("reference against mpmath").
# They are far above the handful of roundings of the formulas because they are relative to J and hold the input conditioning:
# with a length scale of 0.01 box widths the anchored exponent s0a + s0b reaches 50 to 100, and every rounding of a scaled
# distance moves e^(-s0) by s0 u.  No derived count is smaller over this table, so the measured ones stand.
SOBOL_KJ = {("matern32", "outer", "series"): 8.0, ("matern32", "outer", "forward"): 68.0,
            ("matern32", "middle", "series"): 183.0, ("matern32", "middle", "forward"): 26.0,
            ("matern52", "outer", "series"): 10.0, ("matern52", "outer", "forward"): 63.0,
            ("matern52", "middle", "series"): 190.0, ("matern52", "middle", "forward"): 27.0}
# The same measurement in units of u (1 + s0), s0 = s0a + s0b the anchored exponent of the element's DOMINANT segment (the smallest
# among its non-empty segments; (1 + s) e^-s falls with s, so the other segments' conditioning is covered): the derived
# conditioning term taken out, what is left is a constant of a few u in every class.  Both are measured bounds of the reference;
# an element's constant is the smaller of the two, so it is never above the flat one and an order of magnitude below it where the
# exponent is small -- which is where a wrong branch of sobol_moments shows (profiles/stage_bounds_sobol.txt, same section).
SOBOL_KJ0 = {("matern32", "outer", "series"): 7.0, ("matern32", "outer", "forward"): 3.0,
             ("matern32", "middle", "series"): 3.0, ("matern32", "middle", "forward"): 3.0,
             ("matern52", "outer", "series"): 6.0, ("matern52", "outer", "forward"): 3.0,
             ("matern52", "middle", "series"): 5.0, ("matern52", "middle", "forward"): 3.0}
# sum of a tile: 16 serial fmas per thread, six shuffle levels (sobol_wave_sum), two additions of the four waves
SOBOL_TILE_DEPTH = 24.0
_SOBOL_CACHE = {}


def sobol_layout(n, d, q_all, npairs, extra=0):
    """do_sobol_pairs' scratch: tab (q_all, d, n), means (q_all), part (min(npairs, 64), ntile, ntile, 2 d + 1 + extra) doubles
    (extra = 1: the matrix-weighted entries' S0); `total` in bytes (= lcgp_sobol_scratch_bytes / lcgp_sobol_matrix_scratch_bytes)"""
    ntile = (n + TS - 1) // TS
    nb = min(npairs, SOBOL_BATCH)
    cols = 2 * d + 1 + extra
    lay = dict(tab=0, means=q_all * d * n, part=q_all * d * n + q_all, ntile=ntile, nb=nb, cols=cols)
    lay["total"] = 8 * (lay["part"] + nb * ntile * ntile * cols)
    return lay


def sobol_subset_layout(n, d, q_all, npairs):
    """do_sobol_subset_pairs' scratch: tab, means, part (min(npairs, 64), ntile, ntile, SOBOL_CHUNK)"""
    ntile = (n + TS - 1) // TS
    nb = min(npairs, SOBOL_BATCH)
    lay = dict(tab=0, means=q_all * d * n, part=q_all * d * n + q_all, ntile=ntile, nb=nb, cols=SOBOL_CHUNK)
    lay["total"] = 8 * (lay["part"] + nb * ntile * ntile * SOBOL_CHUNK)
    return lay


def sobol_std_masks(d):
    """the 2 d + 1 columns of lcgp_sobol_pairs as bit masks: {l}, all but l, all"""
    full = (1 << d) - 1
    return [1 << l for l in range(d)] + [full ^ (1 << l) for l in range(d)] + [full]


def _np(a):
    return np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, np.float64)


def _mp_moment(n, g, L):
    """int_0^L tau^n e^(-g tau) dtau in mpmath for either sign of g: the series in g L below 1 (no cancellation), the closed
    form with guard digits from there on"""
    x = g * L
    if abs(x) < 1:
        s, t, j = mp.mpf(0), mp.mpf(1), 0
        while True:
            term = t / (n + 1 + j)
            s += term
            j += 1
            t = t * (-x) / j
            if abs(t) < mp.mpf(10) ** (-(SOBOL_DPS + 25)) or j > 400:
                break
        return L ** (n + 1) * s
    with mp.extradps(30):
        e = mp.exp(-x)
        part = sum(x ** j / mp.factorial(j) for j in range(n + 1))
        return +(mp.factorial(n) / g ** (n + 1) * (1 - e * part))


def sobol_exact_J(kernel, u, a, v, b, lo, hi):
    """J = (1 / (hi - lo)) int_lo^hi kappa(|t - u| / a) kappa(|t - v| / b) dt in mpmath (SOBOL_DPS digits) for float64 scalars
    taken as exact.  SE: the erf form, tails through erfc (_marg_mp).  Matern: the box split at the clipped centres; on a piece
    [p, r] neither t - u nor t - v changes sign, the integrand is a polynomial in tau = t - p times e^(-g tau) with g of either
    sign -- always anchored at the LEFT end, no switch on g L, no recurrence: nothing shared with sobol_J but the split."""
    _known(kernel)
    key = (kernel, float(u), float(a), float(v), float(b), float(lo), float(hi))
    got = _SOBOL_CACHE.get(key)
    if got is not None:
        return got
    with mp.workdps(SOBOL_DPS + 15):
        u_, a_, v_, b_, lo_, hi_ = (mp.mpf(float(t)) for t in (u, a, v, b, lo, hi))
        w = hi_ - lo_
        if kernel == "se":
            s2 = a_ * a_ + b_ * b_
            sig = a_ * b_ / mp.sqrt(s2)
            mu = (u_ * b_ * b_ + v_ * a_ * a_) / s2
            z1, z2 = (mu - lo_) / sig, (hi_ - mu) / sig
            if z1 >= 0 and z2 >= 0:
                r = _marg_mp("se", "F", z1) + _marg_mp("se", "F", z2)
            else:
                r = _marg_mp("se", "Fc", min(abs(z1), abs(z2))) - _marg_mp("se", "Fc", max(abs(z1), abs(z2)))
            got = mp.exp(-(u_ - v_) ** 2 / (2 * s2)) * sig * r / w
        else:
            cuts = sorted({lo_, hi_, min(max(u_, lo_), hi_), min(max(v_, lo_), hi_)})
            tot = mp.mpf(0)
            for p, r in zip(cuts[:-1], cuts[1:]):
                mid = (p + r) / 2
                polys, g, e0 = [], mp.mpf(0), mp.mpf(0)
                for c, ell in ((u_, a_), (v_, b_)):
                    sg = 1 if mid > c else -1
                    s0, al = abs(p - c) / ell, sg / ell         # s(tau) = s0 + al tau >= 0 on the piece
                    polys.append([1 + s0, al] if kernel == "matern32" else [1 + s0 + s0 * s0 / 3, al * (1 + 2 * s0 / 3), al * al / 3])
                    g += al
                    e0 += s0
                q = [mp.mpf(0)] * (len(polys[0]) + len(polys[1]) - 1)
                for i, ca in enumerate(polys[0]):
                    for j, cb in enumerate(polys[1]):
                        q[i + j] += ca * cb
                tot += mp.exp(-e0) * sum(qn * _mp_moment(n, g, r - p) for n, qn in enumerate(q))
            got = tot / w
    _SOBOL_CACHE[key] = got
    return got


def _sobol_matern_parts(u, a, v, b, lo, hi):
    """sobol_J's Matern branch variables in the library's float64 operations (arrays): the swap, the reciprocals, the clipped
    centres, per segment its length L and g L"""
    u, a, v, b, lo, hi = np.broadcast_arrays(*(np.asarray(t, np.float64) for t in (u, a, v, b, lo, hi)))
    swap = u > v
    ra, rb = np.where(swap, 1.0 / b, 1.0 / a), np.where(swap, 1.0 / a, 1.0 / b)
    uu, vv = np.where(swap, v, u), np.where(swap, u, v)
    cu, cv = np.minimum(np.maximum(uu, lo), hi), np.minimum(np.maximum(vv, lo), hi)
    L = np.stack([cu - lo, cv - cu, hi - cv])
    g1 = np.where(rb <= ra, ra + (-rb), (-ra) + rb)
    g = np.stack([ra + rb, g1, ra + rb])
    # s0 = s0a + s0b at each segment's anchor, as sobol_J passes them to sobol_segment (left: the anchor of the middle segment);
    # smin, the smallest among the non-empty segments, is the exponent SOBOL_KJ0 is normalised by: keep both in step with sobol_J
    left = rb <= ra
    s0 = np.stack([np.abs(uu - cu) * ra + np.abs(vv - cu) * rb,
                   np.where(left, np.abs(cu - uu) * ra + np.abs(vv - cu) * rb, np.abs(cv - uu) * ra + np.abs(vv - cv) * rb),
                   np.abs(cv - uu) * ra + np.abs(cv - vv) * rb])
    smin = np.min(np.where(L > 0.0, s0, np.inf), axis=0)
    return dict(swap=swap, ra=ra, rb=rb, u=uu, v=vv, cu=cu, cv=cv, L=L, g=g, x=g * L, s0=s0, smin=smin)


def _sobol_se_parts(u, a, v, b, lo, hi):
    """sobol_dim / sobol_J's SE variables in the library's float64 operations"""
    u, a, v, b, lo, hi = np.broadcast_arrays(*(np.asarray(t, np.float64) for t in (u, a, v, b, lo, hi)))
    s2 = a * a + b * b
    c0, c1 = -0.5 / s2, a * b / np.sqrt(s2)
    c2, c3, c4 = 1.0 / c1, b * b / s2, a * a / s2
    df = u - v
    arg = -(c0 * df * df)
    with np.errstate(under="ignore"):
        pref = np.exp(-arg)
    mu = c3 * u + c4 * v
    z1, z2 = (mu - lo) * c2, (hi - mu) * c2
    b1, b2 = np.abs(z1), np.abs(z2)
    inside = (z1 >= 0.0) & (z2 >= 0.0)
    return dict(c1=c1, c2=c2, c3=c3, c4=c4, arg=arg, pref=pref, mu=mu, z1=z1, z2=z2, b1=b1, b2=b2, inside=inside,
                bn=np.minimum(b1, b2), bf=np.maximum(b1, b2), rw=1.0 / (hi - lo), u=u, v=v)


def sobol_classes(kernel, u, a, v, b, lo, hi):
    """the branch classes of sobol_J / sobol_moments an element (u, a, v, b, lo, hi) falls into: name -> bool array.  Computed
    with the library's own float64 operations, so it follows the switches to the last bit."""
    _known(kernel)
    u, a, v, b, lo, hi = np.broadcast_arrays(*(np.asarray(t, np.float64) for t in (u, a, v, b, lo, hi)))
    if kernel == "se":
        p = _sobol_se_parts(u, a, v, b, lo, hi)
        return {"inside": p["inside"], "outside_bn_le_1": ~p["inside"] & (p["bn"] <= 1.0),
                "outside_bn_gt_1": ~p["inside"] & (p["bn"] > 1.0), "centre_on_end": (p["z1"] == 0.0) | (p["z2"] == 0.0),
                "prefactor_below_1e-300": p["pref"] < 1e-300}
    p = _sobol_matern_parts(u, a, v, b, lo, hi)
    L, x, g = p["L"], p["x"], p["g"]
    out = {}
    for s in range(3):
        out["seg%d_length0" % s] = L[s] == 0.0
        out["seg%d_series" % s] = (L[s] > 0.0) & (x[s] < SOBOL_SERIES_BELOW)
        out["seg%d_forward" % s] = (L[s] > 0.0) & (x[s] >= SOBOL_SERIES_BELOW)
    mid = L[1] > 0.0
    out["mid_gamma0"] = mid & (g[1] == 0.0)
    out["mid_just_below_4"] = mid & (x[1] < 4.0) & (x[1] > 4.0 - 1e-3)
    out["mid_just_above_4"] = mid & (x[1] >= 4.0) & (x[1] < 4.0 + 1e-3)
    out["mid_rb_le_ra"] = mid & (p["rb"] <= p["ra"])
    out["mid_rb_gt_ra"] = mid & (p["rb"] > p["ra"])
    out["swap"] = p["swap"]
    out["equal_centres"] = u == v
    out["centre_on_end"] = (u == lo) | (u == hi) | (v == lo) | (v == hi)
    ul, ur, vl, vr = u < lo, u > hi, v < lo, v > hi
    one = (ul | ur) ^ (vl | vr)
    out["one_outside_left"] = one & (ul | vl)
    out["one_outside_right"] = one & (ur | vr)
    out["both_outside_opposite"] = (ul & vr) | (ur & vl)
    out["both_outside_same"] = (ul & vl) | (ur & vr)
    out["scales_1e-12_apart"] = (a != b) & (np.abs(b / a - 1.0) < 1e-11)
    return out


def sobol_cases(kernel, lo, hi):
    """the 1-D case table of the element stage for the box [lo, hi]: rows (u, a, v, b), a few hundred, every class of
    sobol_classes at least 8 times per kernel over the two boxes of the tests (asserted by the CPU tests)"""
    _known(kernel)
    w = hi - lo
    at = lambda f: lo + f * w                              # noqa: E731
    S = [0.01 * w, w, 30.0 * w]
    rows = []
    centres = [(.2, .7), (.7, .2), (.5, .5), (0., .6), (.3, 1.), (-.3, .4), (.4, 1.3), (-.2, 1.3), (-.5, -.1), (1.1, 1.6),
               (.6, -.25), (1., 0.)]
    for a in S:
        for b in S:
            for fu, fv in centres:
                rows.append((at(fu), a, at(fv), b))
    if kernel == "se":
        for a in [0.01 * w, 0.1 * w, w, 3.0 * w, 30.0 * w]:        # a = b: c3 = c4 = 1/2, the product's centre lies on the end
            rows += [(lo, a, lo, a), (hi, a, hi, a)]
        for a in [0.0165 * w, 0.017 * w, 0.0175 * w, 0.01 * w]:    # e^(-df^2 / (2 s2)) below 1e-300 (the last: 0)
            rows += [(at(.05), a, at(.95), a), (at(.97), a, at(.06), a * 1.01), (at(-.02), a, at(.9), a)]
        for a, b in [(w, w), (3 * w, w), (w, 30 * w), (.3 * w, .3 * w)]:   # the centre outside within one sigma
            rows += [(at(-.1), a, at(-.15), b), (at(1.05), a, at(1.1), b)]
    else:
        # the middle segment around gamma L = 4: L = w / 2, 1 / a = 20 / w, gamma = 8 (1 + dl) / w
        for dl in (0.0, 3e-16, -3e-16, 1e-6, -1e-6, 1e-5, -1e-5, 5e-5, -5e-5, 1e-4, -1e-4, 2e-4, -2e-4):
            a, b = 0.05 * w, w / (12.0 - 8.0 * dl)
            rows += [(at(.25), a, at(.75), b), (at(.25), b, at(.75), a), (at(.75), a, at(.25), b)]
        # gamma L from 0.05 to 0.3 at moderate scales (s0 small: SOBOL_KJ0 applies), where a forward recurrence taken too early
        # loses most: the middle segment (1 / b = 1 / a + gamma) and, with both centres near an end, an outer one
        for gl in (0.05, 0.1, 0.2, 0.3):
            for fu, fv, ia in ((0., .7, 8.), (.3, 1., 8.), (0., 1., 3.), (.1, .8, 5.)):
                a, b = w / ia, w / (ia + gl / (fv - fu))
                rows += [(at(fu), a, at(fv), b), (at(fv), a, at(fu), b)]
            rows += [(at(gl / 4.0), 5.0 * w, at(gl / 4.0), 5.0 * w), (at(1.0 - gl / 2.0), 10.0 * w, at(1.0 - gl / 2.0), 10.0 * w)]
        for a in S + [0.1 * w]:                                    # b = a (1 + 1e-12), and gamma = 0 exactly
            for fu, fv in ((.2, .7), (.9, .1), (-.1, .5)):
                rows += [(at(fu), a, at(fv), a * (1.0 + 1e-12)), (at(fu), a, at(fv), a)]
    return np.array(rows, np.float64)


def _sobol_se_bound(u, a, v, b, lo, hi):
    """the absolute error of sobol_J<SE> in units of u, without C, counted from sobol_dim and sobol_J:
      s2 = a a + b b (2 relative), c0 = -1/2 / s2 (+1), c1 = a b / sqrt(s2) (1 + 2 + 1: 4, kept at 5), c2 = 1 / c1 (6),
      c3 = b b / s2, c4 = a a / s2 (4 each), rw = 1 / (hi - lo) (2)
      pref = exp(c0 df df): the argument carries c0 (3), df twice (2), two products (2): 7, kept at 8, each moving pref by
          |argument| u -- the input conditioning of e^(-z^2 / 2) -- plus the call's MARG_ULP
      mu = fma(c3, u, c4 v): (4 + 1) u on each term, one for the sum: |d mu| <= 6 u (|c3 u| + |c4 v|), which enters z = (mu - end) c2
          as an ABSOLUTE 6 u (|c3 u| + |c4 v|) c2 -- large against z where sigma is small against the centres: input conditioning
      z = (mu - end) c2: the difference, c2, the product: 8 u |z| more; marg_F<SE> / marg_Fc<SE>: _marg_terms and 2 u b kappa(b)
          for its own b s product; F' = kappa, Fc' = -kappa
      r = the sum or difference of the two (1 on |A1| + |A2|), J = pref c1 r rw: three products
    so |dJ| <= u [ J (MARG_ULP + 8 |arg| + 5 + 2 + 3) + pref c1 rw (K1 A1 + K2 A2 + A1 + A2 + sum_i kappa(b_i) (dz_i + 2 b_i)) ]"""
    p = _sobol_se_parts(u, a, v, b, lo, hi)
    far = ~p["inside"] & (p["bn"] > 1.0)
    b1, b2 = p["b1"], p["b2"]
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        t1 = np.where(far, _marg_terms("se", "Fc", b1), _marg_terms("se", "F", b1))
        t2 = np.where(far, _marg_terms("se", "Fc", b2), _marg_terms("se", "F", b2))
        k = MARG_ULP + MARG_ROUNDINGS["se", "F"]
        A1, A2 = t1 / k, t2 / k
        r = np.where(p["inside"], A1 + A2, np.abs(A1 - A2))
        dmu = 6.0 * (np.abs(p["c3"] * p["u"]) + np.abs(p["c4"] * p["v"])) * p["c2"]
        inner = t1 + t2 + A1 + A2 + _kappa("se", b1) * (dmu + 10.0 * b1) + _kappa("se", b2) * (dmu + 10.0 * b2)
        front = p["pref"] * p["c1"] * p["rw"]
        return front * r * (MARG_ULP + 8.0 * p["arg"] + 10.0) + front * inner


def sobol_j_bound(kernel, u, a, v, b, lo, hi, J):
    """the absolute error bound of ONE pair average J (arrays; J its value, float64) in units of u, without C: SE derived
    (_sobol_se_bound), Matern SOBOL_KJ of the worst branch among the element's non-empty segments, relative to J"""
    _known(kernel)
    if kernel == "se":
        return _sobol_se_bound(u, a, v, b, lo, hi)
    p = _sobol_matern_parts(u, a, v, b, lo, hi)
    K, K0 = np.zeros(np.shape(p["x"][0])), np.zeros(np.shape(p["x"][0]))
    for s, kind in ((0, "outer"), (1, "middle"), (2, "outer")):
        live = p["L"][s] > 0.0
        series = p["x"][s] < SOBOL_SERIES_BELOW
        K = np.maximum(K, np.where(live, np.where(series, SOBOL_KJ[kernel, kind, "series"], SOBOL_KJ[kernel, kind, "forward"]), 0.0))
        K0 = np.maximum(K0, np.where(live, np.where(series, SOBOL_KJ0[kernel, kind, "series"], SOBOL_KJ0[kernel, kind, "forward"]), 0.0))
    with np.errstate(invalid="ignore"):
        return np.minimum(K, K0 * (1.0 + np.where(np.isfinite(p["smin"]), p["smin"], 0.0))) * np.abs(J)


def sobol_j_measure(kernel, got, rows, lo, hi):
    """the error of `got` (float64 J per row of `rows` = (u, a, v, b)) against sobol_exact_J in units of u relative to the exact
    value (NaN where the exact value is below 1e-290: the floor's entries), and the exact values as float64"""
    rel, ex = np.full(len(rows), np.nan), np.zeros(len(rows))
    for i, (u, a, v, b) in enumerate(np.asarray(rows, np.float64).tolist()):
        e = sobol_exact_J(kernel, u, a, v, b, lo, hi)
        ex[i] = float(e)
        if ex[i] > 1e-290:
            with mp.workdps(SOBOL_DPS):
                rel[i] = float(abs(mp.mpf(float(got[i])) - e) / e) / _U64 if math.isfinite(got[i]) else math.inf
    return rel, ex


def check_sobol_means(means, tab, w) -> Check:
    """means[k] = sum_i w_ki prod_l tab[k, l, i] (sobol_table_kernel: d - 1 products and one fma per term, 64-lane shuffles, four
    waves) against the same sum from the library's table: |error| <= C gamma_(d + n) sum_i |w_ki| prod_l tab + floor"""
    mv, tb, wv = _np(means), _np(tab), _np(w)
    q, d, n = tb.shape
    pr = np.prod(tb, axis=1)
    ref, sab = np.sum(wv * pr, axis=1), np.sum(np.abs(wv) * np.abs(pr), axis=1)
    return worst(_t(np.abs(mv - ref)), _t(C * gamma(d + n) * sab + floor("float64", d + n)))


def sobol_element_exact(kernel, U, A, V, B, box):
    """per element e (rows of U, A, V, B: (m, d) centres and length scales of the two components) and input l the exact J and
    the two 1-D averages, as object arrays (m, d) of mpmath numbers"""
    U, A, V, B, box = (np.asarray(t, np.float64) for t in (U, A, V, B, box))
    m, d = U.shape
    Jx, ax, bx = (np.empty((m, d), object) for _ in range(3))
    for e in range(m):
        for l in range(d):
            lo, hi = box[0, l], box[1, l]
            Jx[e, l] = sobol_exact_J(kernel, U[e, l], A[e, l], V[e, l], B[e, l], lo, hi)
            ax[e, l] = marg_exact(kernel, U[e, l:l + 1], lo, hi, A[e, l])[0]
            bx[e, l] = marg_exact(kernel, V[e, l:l + 1], lo, hi, B[e, l])[0]
    return Jx, ax, bx


def check_sobol_element(rows, kernel, U, A, V, B, box, masks, detail=None) -> Check:
    """rows (m, len(masks)): the library's (M_u - M_0) of ONE element per row (one-hot weights) for the subsets `masks` (bit l:
    input l is in u), against the exact value from mpmath:
        |error| <= C u [ M_u (sum_(l in u) K_J,l + sum_(l not in u) (k_a,l + k_a',l + 1) + |u| + d)
                         + M_0 (sum_l (k_a,l + k_a',l + 1) + d) + |M_u - M_0| + (M_u + M_0) ] + floor
    K_J u J the bound of sobol_j_bound, k_a u a that of marg_table_bound; the last two terms are the difference's and the fma's
    rounding.  The empty mask must give exactly 0.0.  detail: a list that receives (row, column, |error| / (u (M_u + M_0)))."""
    _known(kernel)
    got = _np(rows)
    U, A, V, B, box = (np.asarray(t, np.float64) for t in (U, A, V, B, box))
    m, d = U.shape
    assert got.shape == (m, len(masks)), (got.shape, m, len(masks))
    Jx, ax, bx = sobol_element_exact(kernel, U, A, V, B, box)
    Jf, af, bf = (np.array(t.tolist(), np.float64).reshape(m, d) for t in (Jx, ax, bx))
    KJ, ka = np.zeros((m, d)), np.zeros((m, d))
    with np.errstate(divide="ignore", invalid="ignore"):
        for l in range(d):
            lo, hi = box[0, l], box[1, l]
            kj = sobol_j_bound(kernel, U[:, l], A[:, l], V[:, l], B[:, l], lo, hi, Jf[:, l]) / Jf[:, l]
            KJ[:, l] = np.where(Jf[:, l] > 0.0, kj, 0.0)
            for e in range(m):
                t = (marg_table_bound(kernel, U[e, l:l + 1], lo, hi, A[e, l])[0] / af[e, l] if af[e, l] > 0.0 else 0.0) + \
                    (marg_table_bound(kernel, V[e, l:l + 1], lo, hi, B[e, l])[0] / bf[e, l] if bf[e, l] > 0.0 else 0.0)
                ka[e, l] = t / _U64 + 1.0
    KJ = np.where(np.isfinite(KJ), KJ, 0.0)
    best = Check(0.0, ())
    fl = floor("float64", 2 * d)
    with mp.workdps(SOBOL_DPS):
        for e in range(m):
            m0x = mp.fprod(ax[e, l] * bx[e, l] for l in range(d))
            e0 = float(np.sum(ka[e])) + d
            for s, mask in enumerate(masks):
                if mask == 0:
                    r = 0.0 if (got[e, s] == 0.0 and not np.signbit(got[e, s])) else math.inf
                else:
                    mux = mp.fprod(Jx[e, l] if (mask >> l) & 1 else ax[e, l] * bx[e, l] for l in range(d))
                    eu = sum(KJ[e, l] if (mask >> l) & 1 else ka[e, l] for l in range(d)) + bin(mask).count("1") + d
                    mu_f, m0_f, ex = float(mux), float(m0x), mux - m0x
                    err = float(abs(mp.mpf(float(got[e, s])) - ex)) if math.isfinite(got[e, s]) else math.inf
                    bound = C * _U64 * (mu_f * eu + m0_f * e0 + float(abs(ex)) + mu_f + m0_f) + fl
                    r = err / bound
                    if detail is not None and mu_f + m0_f > 1e-290:
                        detail.append((e, s, err / (_U64 * (mu_f + m0_f))))
                if not r <= best.ratio:
                    best = Check(float(r) if r == r else math.inf, (e, s))
    return best


def sobol_tile_reference(kernel, x, w, ell, box, tab, k, kp, masks, Q=None, rows=None, cols=None):
    """per tile (r, c) and subset: ref = twice sum_tile wgt (M_u - M_0) and the bound's sum  u (E + SOBOL_TILE_DEPTH) |wgt| (M_u +
    M_0), elementwise E as in check_sobol_element without the a terms (the table is the library's own): (ref, bnd) of shape (ntile,
    ntile, len(masks) [+ 1 with Q: S0 = sum wgt M_0]).  J from tests/sobol_ref.pair_integral.  rows / cols: tile indices to form
    (default: all; for a pair k = k' only c <= r is formed, the rest stays NaN)."""
    from tests import sobol_ref
    x, w, ell, box, tab = (_np(t) for t in (x, w, ell, box, tab))
    n, d = x.shape
    ntile = (n + TS - 1) // TS
    ncol = len(masks) + (1 if Q is not None else 0)
    ref, bnd = np.full((ntile, ntile, ncol), np.nan), np.full((ntile, ntile, ncol), np.nan)
    for r in (range(ntile) if rows is None else rows):
        for c in (range(ntile) if cols is None else cols):
            if k == kp and c > r:
                continue
            ri, cj = slice(r * TS, min(n, (r + 1) * TS)), slice(c * TS, min(n, (c + 1) * TS))
            twice = 2.0 if (k == kp and c < r) else 1.0
            wgt = twice * (w[k, ri][:, None] * w[kp, cj][None, :])
            if Q is not None:
                wgt = wgt * _np(Q)[ri, cj]
            J = np.empty(wgt.shape + (d,))
            KJ = np.empty(wgt.shape + (d,))
            for l in range(d):
                args = (x[ri, l][:, None], ell[k, l], x[cj, l][None, :], ell[kp, l], box[0, l], box[1, l])
                J[..., l] = sobol_ref.pair_integral(kernel, box[0, l], box[1, l], args[0], args[1], args[2], args[3])
                with np.errstate(divide="ignore", invalid="ignore"):
                    kj = sobol_j_bound(kernel, *args, J[..., l]) / J[..., l]
                KJ[..., l] = np.where(np.isfinite(kj), kj, 0.0)
            Aa = tab[k][:, ri].T[:, None, :] * tab[kp][:, cj].T[None, :, :]
            M0 = np.prod(Aa, axis=-1)
            for s, mask in enumerate(masks):
                bits = np.array([(mask >> l) & 1 for l in range(d)], bool)
                Mu = np.prod(np.where(bits, J, Aa), axis=-1)
                E = np.sum(np.where(bits, KJ, 1.0), axis=-1) + float(bits.sum()) + d + 2.0
                E0 = 2.0 * d + 2.0
                ref[r, c, s] = np.sum(wgt * (Mu - M0))
                bnd[r, c, s] = _U64 * np.sum(np.abs(wgt) * ((E + SOBOL_TILE_DEPTH) * Mu + (E0 + SOBOL_TILE_DEPTH) * M0))
            if Q is not None:
                ref[r, c, -1] = np.sum(wgt * M0)
                bnd[r, c, -1] = _U64 * np.sum(np.abs(wgt) * (E0 + SOBOL_TILE_DEPTH) * M0)
    return ref, bnd


def check_sobol_tile(part, ref, bnd) -> Check:
    """part (ntile, ntile, cols) of one pair against sobol_tile_reference: |error| <= C bnd + floor wherever ref is formed (not
    NaN).  Location: (row tile, column tile, column)."""
    pv = _np(part)
    have = ~np.isnan(ref)
    if not have.any():
        return Check(0.0, ())
    r = np.where(have, np.abs(pv - np.where(have, ref, 0.0)) / (C * np.where(have, bnd, 1.0) + floor("float64", TS * TS)), 0.0)
    r = np.where(np.isnan(r), math.inf, r)
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return Check(float(r[i]), tuple(int(t) for t in i))


def check_sobol_reduce(out_row, part, same) -> Check:
    """out_row (cols) against the sum over the tiles of the library's own part (ntile, ntile, cols), in float64 on the host; for a
    pair k = k' (`same`) only the tiles c <= r -- whatever the others hold must not reach the sum:
        |error| <= C gamma_(ntile^2) sum |part| + floor
    (sobol_reduce_kernel / sobol_subset_reduce_kernel: a serial sum per thread, then a tree over 256 threads: any order)"""
    ov, pv = _np(out_row), _np(part)
    nt = pv.shape[0]
    keep = np.tril(np.ones((nt, nt), bool)) if same else np.ones((nt, nt), bool)
    sel = pv[keep]
    ref, sab = sel.sum(axis=0), np.abs(sel).sum(axis=0)
    r = np.abs(ov - ref) / (C * gamma(nt * nt) * sab + floor("float64", nt * nt))
    r = np.where(np.isnan(r), math.inf, r)
    i = int(np.argmax(r))
    return Check(float(r[i]), (i,))


def check_sobol_rows(out_row, ref, bnd) -> Check:
    """out_row (cols) of ANY batch against the tile references of sobol_tile_reference summed over the tiles it forms (NaN: none):
        |error| <= C (sum bnd + gamma_(ntile^2) sum |ref|) + floor
    the tile stage's bound and the reduction's together -- the one check that sees the rows of batches whose tile sums the next
    batch has overwritten (the p0 loop and the row offsets of do_sobol_pairs / do_sobol_subset_pairs)"""
    ov = _np(out_row)
    nt = ref.shape[0]
    r0, b0 = np.nansum(ref, axis=(0, 1)), np.nansum(bnd, axis=(0, 1))
    sab = np.nansum(np.abs(ref), axis=(0, 1))
    r = np.abs(ov[:r0.shape[0]] - r0) / (C * (b0 + gamma(nt * nt) * sab) + floor("float64", nt * nt * TS * TS))
    r = np.where(np.isnan(r), math.inf, r)
    i = int(np.argmax(r))
    return Check(float(r[i]), (i,))


# the matrix-weighted entries (lcgp_sobol_matrix_pairs: SOBOL_MAT) use sobol_layout(extra=1) and sobol_tile_reference(Q=...): the
# weight of an element is v_i v_i' Q[i, i'] (one more product: covered by the + 2 of E), one more sum per tile, S0.  The view
# (lcgp_condition_sobol_matrix_pairs: SOBOL_VIEW) prepares, per component, P and E in the scratch at cond_sobol_carve's offsets.
def cond_sobol_layout(n, d, q, m, subset=False):
    """cond_sobol_carve of lcgp_hip.hip: the offsets in doubles of tab (q, d, N), means, part (ONE pair: ntile^2 tiles of 2 d + 2
    sums, or of SOBOL_CHUNK for the subset form), neg (the word holding -1), T (mpad x npad), G (mpad x npad), P (Npad x mpad),
    E (Npad x Npad), each aligned to 256 bytes, and `total` in bytes"""
    N = n + m
    Npad, npad, mpad = -(-N // TS) * TS, _pad128(n), _pad128(m)
    nt = Npad // TS
    lay = _carve([("tab", q * d * N), ("means", q), ("part", nt * nt * (SOBOL_CHUNK if subset else 2 * d + 2)), ("neg", 1),
                  ("t", mpad * npad), ("g", mpad * npad), ("p", Npad * mpad), ("e", Npad * Npad)])
    lay.update(N=N, Npad=Npad, npad=npad, mpad=mpad, ntile=nt)
    return lay


def check_sobol_p(P, G, Wd, D, n, m) -> Check:
    """P (Npad x mpad) of cond_sobol_p_kernel: D G[a, i] for i < n (one rounding: |error| <= C u |D G| + floor), BITWISE the dense
    L_S^-1[a, i - n] for n <= i < n + m, bitwise zero on the rows from n + m on and on the columns from m on"""
    Pv, Gv, Wv = _np(P), _np(G), _np(Wd)
    if not (_same_bits(_t(Pv[n:n + m, :m].copy()), _t(Wv[:m, :m].T.copy())) and _zero_bits(_t(Pv[n + m:].copy()))
            and _zero_bits(_t(Pv[:, m:].copy()))):
        return Check(math.inf, ("copy",))
    ref = float(D) * Gv[:m, :n].T
    return worst(_t(np.abs(Pv[:n, :m] - ref)), _t(C * _U64 * np.abs(ref) + floor("float64", 1)), lower=False)


def check_sobol_e(E, P, m) -> Check:
    """the lower 64-tiles of E = P P^T (OP_PRED_COV on a zeroed E with alpha = -(-1)) against the library's own P:
    |error| <= C gamma_(m + 1) |P| |P|^T + floor on the lower triangle; the strictly upper tiles stay bitwise zero"""
    Ev, Pv = _np(E), _np(P)
    Np = Ev.shape[0]
    low = np.kron(np.tril(np.ones((Np // TS, Np // TS))), np.ones((TS, TS))) > 0
    if np.any(Ev[~low].view(np.int64) != 0):
        return Check(math.inf, ("upper",))
    ref, sab = Pv @ Pv.T, np.abs(Pv) @ np.abs(Pv).T
    err = np.tril(np.abs(Ev - ref))                        # (sobol_stage_q reads a diagonal tile's lower triangle only)
    return worst(_t(err), _t(C * gamma(m + 1) * sab + floor("float64", m)), lower=False)


def sobol_view_q(E, Ainv, D, nt, N):
    """Q' (N x N) as sobol_stage_q<SOBOL_VIEW> reads it: E from its lower triangle, mirrored, plus D A^-1 where both indices are
    below nt (one fma: within C)"""
    Ev = _np(E)[:N, :N]
    Q = np.tril(Ev) + np.tril(Ev, -1).T
    Q[:nt, :nt] += float(D) * _np(Ainv)[:nt, :nt]
    return Q


def check_sobol_t(T, Wd, Un, m) -> Check:
    """T = 0 - L_S^-1 U_n (mpad x npad; OP_COND_U on a zeroed slab with R := the dense L_S^-1, K = mpad) against the float64 product
    of the state's own dense L_S^-1 (mpad x mpad) and U_n (mpad x npad): an inner product of m terms (the padding adds stored
    zeros) and the subtraction from zero, |error| <= C gamma_(m + 1) |L_S^-1| |U_n| + floor.  G = T W, the launch that follows, is
    check_pgrad_v's (OP_PRED_V with W = L^-1)."""
    Tv, Wv, Uv = _np(T), _np(Wd), _np(Un)
    ref, sab = -(Wv @ Uv), np.abs(Wv) @ np.abs(Uv)
    return worst(_t(np.abs(Tv - ref)), _t(C * gamma(m + 1) * sab + floor("float64", m)), lower=False)
