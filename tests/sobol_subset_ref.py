"""float64 numpy restatement of the closed variances of arbitrary input subsets (LCGP.sobol_subsets, sobol_indices(order=2),
shapley_effects; lcgp_sobol_subset_pairs and its two matrix-weighted forms), written from the formulas of DESIGN.md 4.25 on top of
tests/sobol_ref.py (the pair integral, the conventions of pair_sums) and tests/sobol_uncertainty_ref.py (the matrix Q).

  mask_of / classical_masks   a subset as a bit mask (bit l: input l is in u); the 2 d + 1 subsets of lcgp_sobol_pairs in its order
  subset_product      P_u = prod_l (bit_l ? J_l : A_l), l ascending, multiplied one factor after the other as the device does
  subset_pair_sums    for one pair of components: D_u = sum w_i w'_i' (M_u - M_0) per mask, the two box means, and the size
                      sum |w_i| |w'_i'| (M_u + M_0) of what D_u adds up
  subset_matrix_sums  for one component and a dense symmetric Q: sum Q (M_u - M_0) per mask and the size sum |Q| (M_u + M_0)
  prior_products      prod over the inputs NOT in u of the double average I2_l per mask, and the product over all inputs
  shapley_by_permutations     the Shapley effects from their definition: the average over all orderings of the inputs

Shared by the CPU tests (tests/test_sobol_subset_host.py) and the GPU tests (tests/test_gpu_sobol_subsets.py)."""
import itertools

import numpy as np

from tests import marginal_ref as mref
from tests import sobol_ref as ref


def mask_of(u):
    return int(sum(1 << int(l) for l in u))


def classical_masks(d):
    """{l} (l = 0 .. d - 1), all but l, all inputs: the columns of lcgp_sobol_pairs"""
    full = (1 << d) - 1
    return [1 << l for l in range(d)] + [full & ~(1 << l) for l in range(d)] + [full]


def subset_product(mask, J, A):
    """J, A (..., d) -> prod_l (bit_l ? J_l : A_l), starting from 1.0 and multiplying l = 0, 1, ... in turn"""
    J, A = np.asarray(J, np.float64), np.asarray(A, np.float64)
    p = np.ones(J.shape[:-1])
    for l in range(J.shape[-1]):
        p = p * (J[..., l] if (int(mask) >> l) & 1 else A[..., l])
    return p


def _factors(kernel, x, ell1, ell2, box):
    x, box = np.asarray(x, np.float64), np.asarray(box, np.float64)
    lo, hi = box[0], box[1]
    a1 = mref.I1(kernel, x, lo[None, :], hi[None, :], np.asarray(ell1)[None, :])            # (n, d)
    a2 = mref.I1(kernel, x, lo[None, :], hi[None, :], np.asarray(ell2)[None, :])
    J = ref.pair_integral(kernel, lo, hi, x[:, None, :], np.asarray(ell1)[None, None, :], x[None, :, :], np.asarray(ell2)[None, None, :])
    return a1, a2, J, a1[:, None, :] * a2[None, :, :]


def subset_pair_sums(kernel, x, w1, ell1, w2, ell2, box, masks):
    """one pair of components over the inputs x (n, d) and box (2, d), standardised: D (nsub), the means (m1, m2), size (nsub)"""
    a1, a2, J, A = _factors(kernel, x, ell1, ell2, box)
    M0 = subset_product(0, J, A)
    ww = np.asarray(w1)[:, None] * np.asarray(w2)[None, :]
    D, size = np.zeros(len(masks)), np.zeros(len(masks))
    for s, mask in enumerate(masks):
        M = subset_product(mask, J, A)
        D[s] = np.sum(ww * (M - M0))
        size[s] = np.sum(np.abs(ww) * (M + M0))
    return D, (np.asarray(w1) @ np.prod(a1, axis=1), np.asarray(w2) @ np.prod(a2, axis=1)), size


def subset_matrix_sums(kernel, x, ell, box, Q, masks):
    """x (n, d), ell (d), box (2, d) standardised, Q (n, n): (sums (nsub), size (nsub))"""
    _, _, J, A = _factors(kernel, x, ell, ell, box)
    Q = np.asarray(Q, np.float64)
    M0 = subset_product(0, J, A)
    sums, size = np.zeros(len(masks)), np.zeros(len(masks))
    for s, mask in enumerate(masks):
        M = subset_product(mask, J, A)
        sums[s] = np.sum(Q * (M - M0))
        size[s] = np.sum(np.abs(Q) * (M + M0))
    return sums, size


def prior_products(kernel, ell, box, masks):
    """(P (nsub), P0): prod over the inputs NOT in u of the double average I2_l, and prod over all inputs"""
    box = np.asarray(box, np.float64)
    d = box.shape[1]
    i2 = mref.I2(kernel, box[1] - box[0], np.asarray(ell, np.float64))
    P = np.array([np.prod([i2[l] for l in range(d) if not (int(mask) >> l) & 1]) for mask in masks])
    return P, float(np.prod(i2))


def shapley_by_permutations(closed, d):
    """closed: a function mask -> V^c_u (scalar or array).  The effect of input l is the average, over all d! orders in which the
    inputs can be added, of what V^c gains when l joins the inputs before it"""
    perms = list(itertools.permutations(range(d)))
    eff = [0.0] * d
    for perm in perms:
        mask = 0
        for l in perm:
            eff[l] = eff[l] + (closed(mask | (1 << l)) - closed(mask))
            mask |= 1 << l
    return np.stack([np.asarray(e, np.float64) / len(perms) for e in eff], axis=-1)
