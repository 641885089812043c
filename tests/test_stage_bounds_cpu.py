"""The stage bounds of tests/stage_bounds.py have teeth (no GPU): an emulated path -- float64 stages, and float32 stages
emulated by rounding each stage's float64 result -- passes every check with a ratio far below 1, and each of the defects
the GPU tests are meant to catch (a perturbed tile, a missing panel update, a stale tile, a tile left out of a product, a
wrong tile in the gradient contraction, a poor pivot) fails the check of its stage.  The first defect also leaves the
end-to-end NLL within the 1e-6 parity bar: the bar the rest of the suite uses cannot see it.

The joint path (X, U, Sigma + tau I, its factor, the draws) gets the same treatment on an emulated path with q = 3
components: a perturbed tile of Sigma, a K-tile left out of D U U^T, tau of the wrong component, a draw through an
upper triangle that was not zeroed, draws shifted at a chunk split and a float32-accurate Sigma each fail their check.

At the input dimensions of the d-templated kernels (d = 17, 33, 126) the emulated path passes as well, and a last chunk
staged with the lengthscales of the chunk before it, stale padding dimensions, one lengthscale gradient 1e-8 off in the
fourth 32-dimension chunk (which the oracle's normwise bar passes) and swapped g_scale / g_nug accumulators each fail;
predictions at training rows fail check_predict when the nugget term sits one column off or is missing.

Matern-5/2.  The emulated paths build their matrices from sb.kernel_parts, so its Matern-5/2 branches are pinned without
going through them: C0 against tests/matern52_oracle.py, dC0 and h against torch autograd of a C0 restated here, and the
magnification E against an emulation of build_kernel's float32 operation order.  Three wrong-kernel defects (a far tile of
A, one g_ell slot, dghat: each with the Matern-3/2 formula) fail their stage.

The conditioned view (lcgp_condition_prepare / lcgp_condition_predict) is emulated in the storage type with q = 3 components,
the three kernels, the full and the replicated path: every stage from X_n to the corrected outputs is at or below 1, and tau of
the wrong component or without the replicate counts, a K-stage left out of a far tile of Sigma_0n, a nugget term where a row of
x0 equals a row of xn, an upper triangle of the dense L_S^-1 that was not zeroed, v of the wrong component, row sums over a
non-zero padding column of T and a float32-accurate Sigma_0n each fail their own stage and none upstream of it.  A far tile of
Sigma_0n off by 1e-6 relative, invisible in the units of the end-to-end test, fails cond_cross.

The second-order input queries (lcgp_predict_hess, lcgp_predict_gradcov) are emulated in the kernels' blocked order (4 x 4 blocks
of dimension pairs, 32-dimension chunks, four waves per workgroup), DX and P in the storage type: the three kernels, both
precisions, the full and the replicated path pass pdx, p, phess, gradcov and gradcov_sum at d = 6 and d = 33.  psi on an
off-diagonal block pair, a block past d written into a valid slot, a transposed packed index, the tail of the vector loads left
out of the Gram term, a stale 32-dimension chunk in DX, the Matern-3/2 psi or kappa under Matern-5/2, a float32 reciprocal, the D
of another component, M overwritten or a dead wave weighted, and a float32-accurate P each fail the check they name and no other.
One small off-diagonal Hessian entry off by 1e-3 relative, invisible to max|err| / max|ref|, fails check_phess.

The box-averaged predictions (lcgp_predict_marginal, lcgp_condition_predict_marginal) are emulated from the float64 restatement
tests/marginal_ref.py (the table), the masked rows, U, the outputs with the averaged prior, the view's stages and gcov: the three
kernels, both precisions, full and rep, d = 3 and 34, the default box and a sub-box pass every check, at most 1 % of the table
entries have a bound set by the absolute floor and the median ratio of the table stays above 1e-3.  The restatement itself -- which
shares its series, switches and closed forms with the kernel -- meets the table bound against mpmath on a grid that sits on every
switch.  A wrong Matern-5/2 coefficient, ten series terms, the near-branch formula (erf differences for SE) in the far tail, a
padding column that is not 1, the table row of the next dimension or component, a stale table chunk, x0 read under the mask, a
prior left at scale or with the nugget, I2 of the wrong dimension or T_i . T_r dropped in gcov and float32-accurate rows each fail
their stage.  Small table entries or one far tile of masked rows off by 1e-9, invisible to the normwise 1e-10, fail theirs.

The two parameter-space queries (lcgp_nll_hess, lcgp_predict_paramgrad) are emulated stage by stage in float64, every buffer of
their scratch layouts, in the kernels' blocked order (4 x 4 dimension block pairs, HS_JC chunks of j, 64-bands, PP_DB blocks): the
three kernels, full and rep, pass every check at d = 3 and d = 9 with at most 1 % of the bounds of any stage set by the floor, and
the final outputs agree with the closed forms of tests/test_nll_hess_host.py (tied there to tests/nll_hess_ref.py) and
tests/param_grad_ref.py at those files' bars.  Eleven defects of the Hessian path and six of the parameter-gradient path each fail
the stage they belong to and none upstream; one ell-ell entry of hk and one small dgvar column off by 1e-6 relative pass today's
normwise bars (1e-11, 1e-10) and fail check_hess_out / check_pp_out."""
import numpy as np
import pytest
import scipy.linalg
import torch

from tests import stage_bounds as sb

N, D_IN, P = 300, 3, 4
TS = sb.TS
KERNELS = ["matern32", "se", "matern52"]


def _problem(seed=0, ell=(0.3, 0.5, 0.8), n=N):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (n, D_IN))
    Y = rng.standard_normal((P, n))
    th = np.concatenate([np.asarray(ell, np.float64), [1.3, 0.01, 5.0], rng.standard_normal(P)])
    return x, Y, th


def _r(a, dtype):
    return sb.rounded(a, dtype)


def _emulate(x, Y, th, dtype, kernel="matern32"):
    """every stage computed in float64 from the previous stage's stored result and rounded to the storage type (any input
    dimension: d = x.shape[1] places psi in th)"""
    A = _r(sb.reference_A(x, None, th, kernel, dtype)[0].numpy(), dtype)
    L = _r(np.linalg.cholesky(A), dtype)
    W = _r(np.linalg.solve(L, np.eye(x.shape[0])), dtype)
    W = np.tril(W)
    V = _r(W.T @ W, dtype)
    psi = th[x.shape[1] + 3:]
    b = _r(_r(Y, dtype).T @ psi, dtype)
    z = _r(V @ b, dtype)
    ref, _ = sb.reference_outputs(x, Y, None, th, V, b, z, kernel, dtype)
    ref = ref.numpy()
    out = np.concatenate([[np.sum(np.log(np.diag(L))), ref[0], 0.0], ref[1:]])
    return dict(A=A, L=L, W=W, V=V, b=b, z=z, out=out)


def _checks(e, x, Y, th, dtype, kernel="matern32"):
    return dict(build=sb.check_build(e["A"], e["b"], x, Y, None, th, kernel, dtype),
                cholesky=sb.check_cholesky(e["A"], e["L"], dtype),
                half_logdet=sb.check_half_logdet(e["L"], e["out"][0], dtype),
                inverse_factor=sb.check_inverse_factor(e["L"], e["W"], dtype),
                inverse=sb.check_inverse(e["W"], e["V"], dtype),
                z=sb.check_z(e["V"], e["b"], e["z"], dtype),
                outputs=sb.check_outputs(e["out"], x, Y, None, th, e["V"], e["b"], e["z"], kernel, dtype))


def _tile(i, j):
    return slice(i * TS, (i + 1) * TS), slice(j * TS, (j + 1) * TS)


def _nll(L, b, D):
    """NLL_k = sum log L_ii - b^T (b - A^-1 b) / (2 D) from a factor L"""
    z = np.linalg.solve(L.T, np.linalg.solve(L, b))
    return np.sum(np.log(np.diag(L))) - b @ (b - z) / (2 * D)


@pytest.fixture(scope="module")
def prob():
    return _problem()


@pytest.fixture(scope="module")
def prob2048():
    return _problem(1, n=2048)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_emulated_path_passes_every_stage(prob, dtype, kernel):
    x, Y, th = prob
    e = _emulate(x, Y, th, dtype, kernel)
    for stage, c in _checks(e, x, Y, th, dtype, kernel).items():
        assert c.ratio < 0.5, (stage, c)


def test_predict_bound_passes(prob):
    x, Y, th = prob
    for dtype in ("float64", "float32"):
        e = _emulate(x, Y, th, dtype)
        x0 = np.random.default_rng(5).uniform(-0.2, 1.2, (37, D_IN))
        ell, scale, nug, Dk, _ = sb.split_theta(th, D_IN)
        c0 = sb.kernel_parts(_r(x0, dtype), _r(x, dtype), ell, "matern32", dtype)[0].numpy()
        X = scale * (1 - nug / (1 + nug)) * c0
        ghat = X @ e["z"]
        gvar = scale - Dk * np.sum((X @ e["W"].T) ** 2, axis=1)
        assert sb.check_predict(ghat, gvar, x0, x, None, th, e["W"], e["z"], "matern32", dtype).ratio < 0.05
        if dtype == "float64":          # (ghat cancels: |X| |z| ~ 2e3 |X z| here, so float32 has no teeth at 1e-2)
            bad = ghat.copy()
            bad[3] *= 1 + 1e-8
            assert sb.check_predict(bad, gvar, x0, x, None, th, e["W"], e["z"], "matern32", dtype).ratio > 1


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_mutation_1_perturbed_tile_of_L(prob, dtype):
    """one off-diagonal tile of L off by 1e-12 (float64) / 1e-5 (float32) relative: the Cholesky check fails at that
    tile, while the NLL moves by less than the suite's 1e-6 bar.  (In float32 the tile sits in block column 0: the
    bound of entry (i, j) grows with min(i, j), 1e-5 is within it from j ~ 40 on.)"""
    x, Y, th = prob
    e = _emulate(x, Y, th, dtype)
    L = e["L"].copy()
    tile = (3, 1) if dtype == "float64" else (3, 0)
    L[_tile(*tile)] *= 1 + (1e-12 if dtype == "float64" else 1e-5)
    c = sb.check_cholesky(e["A"], L, dtype)
    assert c.ratio > 1 and c.where == tile, c
    v0, v1 = _nll(e["L"], e["b"], th[D_IN + 2]), _nll(L, e["b"], th[D_IN + 2])
    assert abs(v1 - v0) < 1e-6 * abs(v0)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_mutation_2_far_tile_missing_a_panel_update(prob, dtype):
    """tile (4, 2) of L computed without the rank-64 update from block column 0"""
    x, Y, th = prob
    e = _emulate(x, Y, th, dtype)
    L = e["L"].copy()
    r, c, k = _tile(4, 2)[0], _tile(4, 2)[1], slice(0, TS)
    # L_rc = (A_rc - sum_j L_rj L_cj^T) L_cc^-T: leaving out panel k adds L_rk L_ck^T L_cc^-T
    L[r, c] = _r(L[r, c] + np.linalg.solve(L[c, c], (L[r, k] @ L[c, k].T).T).T, dtype)
    ch = sb.check_cholesky(e["A"], L, dtype)
    assert ch.ratio > 1 and ch.where[0] == 4, ch      # (row block 4 of the residual: tiles (4, 2) .. (4, 4))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_mutation_3_stale_tile_of_W(prob, dtype):
    """one tile of L^-1 left over from an evaluation at another theta (lengthscale 0.1 % off)"""
    x, Y, th = prob
    e = _emulate(x, Y, th, dtype)
    th2 = th.copy()
    th2[0] *= 1.001
    e2 = _emulate(x, Y, th2, dtype)
    W = e["W"].copy()
    W[_tile(3, 1)] = e2["W"][_tile(3, 1)]
    c = sb.check_inverse_factor(e["L"], W, dtype)
    assert c.ratio > 1 and c.where == (3, 1), c


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_mutation_4_tile_of_V_left_out_of_z(prob, dtype):
    x, Y, th = prob
    e = _emulate(x, Y, th, dtype)
    r, c = _tile(4, 1)
    z = e["z"].copy()
    z[r] = _r(z[r] - e["V"][r, c] @ e["b"][c], dtype)
    ch = sb.check_z(e["V"], e["b"], z, dtype)
    assert ch.ratio > 1 and ch.where == (4,), ch


@pytest.mark.parametrize("n", [N, 2048])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("defect", ["off_diagonal_dropped", "diagonal_twice"])
def test_mutation_5_gradient_contraction_tile(prob, prob2048, n, dtype, defect):
    """the gradient contraction with tile (3, 1) (and its mirror) dropped, or diagonal tile 2 counted twice -- also at
    n = 2048, where the contraction sums 4e6 entries: the float32 path contracts in float64, and so does its bound"""
    x, Y, th = prob if n == N else prob2048
    e = _emulate(x, Y, th, dtype)
    ell, scale, nug, Dk, _ = sb.split_theta(th, D_IN)
    V, z = torch.as_tensor(e["V"]), torch.as_tensor(e["z"])
    G = 0.5 * Dk * V - 0.5 * z[:, None] * z[None, :]
    mask = torch.ones_like(G)
    if defect == "off_diagonal_dropped":
        mask[_tile(3, 1)] = 0.0
        mask[_tile(1, 3)] = 0.0
    else:
        mask[_tile(2, 2)] = 2.0
    xr = sb.rounded(x, dtype)
    nt = nug / (1 + nug)
    out = e["out"].copy()
    for l, f in enumerate(sb.dC0(xr, xr, ell, "matern32")):
        out[3 + l] = scale * (1 - nt) / ell[l] * float((G * mask * f).sum())
    c = sb.check_outputs(out, x, Y, None, th, e["V"], e["b"], e["z"], "matern32", dtype)
    assert c.ratio > 1 and c.where[0].startswith("g_ell"), c


def test_mutation_6_pivot_rounded_to_float32_in_a_float64_factor(prob):
    """a diagonal entry of a float64 L carrying only float32 accuracy (a reciprocal on the pivot chain that is not
    refined to full precision)"""
    x, Y, th = prob
    e = _emulate(x, Y, th, "float64")
    L = e["L"].copy()
    j = 150
    L[j, j] = float(np.float32(L[j, j]))
    assert L[j, j] != e["L"][j, j]
    c = sb.check_cholesky(e["A"], L, "float64")
    assert c.ratio > 1 and c.where == (j // TS, j // TS), c


# ----------------------------------------------------------------------------------------------------------------------
# joint covariance and draws: an emulated path with q = 3 components that differ in every parameter
# ----------------------------------------------------------------------------------------------------------------------
N0, S_DRAWS = 300, 300
JOINT_TH = ((0.3, 0.5, 0.8), 1.3, 0.01, 5.0), ((0.6, 0.25, 0.4), 0.7, 0.002, 12.0), ((1.1, 0.9, 0.35), 2.1, 0.05, 2.5)
JITTER = {"float64": 1e-8, "float32": 1e-3}      # float32: Sigma cancels, the rounded Sigma needs tau to stay definite


def _emulate_joint(dtype, kernel="matern32"):
    """per component: W and z of the training factorisation (_emulate), then X, U, Sigma + tau I, its factor and the
    draws, each computed in float64 from the previous stage's stored result and rounded to the storage type"""
    x, Y, _ = _problem()
    x0 = np.random.default_rng(21).uniform(-0.1, 1.1, (N0, D_IN))
    jit = JITTER[dtype]
    comps = []
    for k, (ell, scale, nug, Dk) in enumerate(JOINT_TH):
        th = np.concatenate([ell, [scale, nug, Dk], np.random.default_rng(30 + k).standard_normal(P)])
        e = _emulate(x, Y, th, dtype, kernel)
        nt = nug / (1 + nug)
        c0 = sb.kernel_parts(_r(x0, dtype), _r(x, dtype), ell, kernel, dtype)[0].numpy()
        X = _r(scale * (1 - nt) * c0, dtype)
        U = _r(X @ e["W"].T, dtype)
        c00 = sb.kernel_parts(_r(x0, dtype), _r(x0, dtype), ell, kernel, dtype)[0].numpy()
        c00 = scale * ((1 - nt) * c00 + nt * np.eye(N0))
        sig = _r(c00 - Dk * U @ U.T + jit * scale * np.eye(N0), dtype)
        L = _r(np.linalg.cholesky(sig), dtype)
        eps = np.random.default_rng(40 + k).standard_normal((S_DRAWS, N0))
        ghat = X @ e["z"]
        draws = ghat[None, :] + _r(_r(eps, dtype) @ L.T, dtype)
        comps.append(dict(th=th, W=e["W"], X=X, U=U, sig=sig, L=L, eps=eps, ghat=ghat, draws=draws, c00=c00))
    return x, x0, jit, comps


@pytest.fixture(scope="module", params=["float64", "float32"])
def joint(request):
    return (request.param,) + _emulate_joint(request.param)


def _joint_checks(c, x, x0, jit, dtype, kernel="matern32"):
    return dict(cross=sb.check_cov_cross(c["X"], x0, x, None, c["th"], kernel, dtype),
                u=sb.check_cov_u(c["U"], c["X"], c["W"], dtype),
                sigma=sb.check_sigma(c["sig"], c["U"], x0, c["th"], jit, kernel, dtype),
                cov_factor=sb.check_cholesky_inverse_solve(c["sig"], c["L"], dtype),
                draws=sb.check_draws(c["draws"], c["L"], c["eps"], c["ghat"], dtype))


def test_emulated_joint_path_passes_every_stage(joint):
    dtype, x, x0, jit, comps = joint
    for k, c in enumerate(comps):
        for stage, ch in _joint_checks(c, x, x0, jit, dtype).items():
            assert ch.ratio < 0.5, (k, stage, ch)


def test_emulated_joint_path_se_kernel():
    x, x0, jit, comps = _emulate_joint("float64", "se")
    for k, c in enumerate(comps):
        for stage, ch in _joint_checks(c, x, x0, jit, "float64", "se").items():
            assert ch.ratio < 0.5, (k, stage, ch)


def test_emulated_joint_path_matern52_kernel():
    x, x0, jit, comps = _emulate_joint("float64", "matern52")
    for k, c in enumerate(comps):
        for stage, ch in _joint_checks(c, x, x0, jit, "float64", "matern52").items():
            assert ch.ratio < 0.5, (k, stage, ch)


def test_cov_cross_honours_the_nugget_of_the_training_set():
    """x0 = the training rows 10 .. 109 (same = 11): the nugget term belongs on the shifted diagonal and nowhere else"""
    x, _, _ = _problem()
    ell, scale, nug, Dk = JOINT_TH[0]
    th = np.concatenate([ell, [scale, nug, Dk]])
    nt = nug / (1 + nug)
    x0 = x[10:110]
    c0 = sb.kernel_parts(x0, x, ell, "matern32", "float64")[0].numpy()
    dl = np.zeros_like(c0)
    dl[np.arange(100), np.arange(100) + 10] = 1.0
    X = scale * ((1 - nt) * c0 + nt * dl)
    assert sb.check_cov_cross(X, x0, x, None, th, "matern32", "float64", same=11).ratio < 0.5
    assert sb.check_cov_cross(X, x0, x, None, th, "matern32", "float64", same=0).ratio > 1
    assert sb.check_cov_cross(X, x0, x, None, th, "matern32", "float64", same=1).ratio > 1


def test_joint_defect_1_perturbed_tile_of_sigma():
    """one strictly-lower 64-tile of Sigma off by 1e-9 relative (float64): far below any normwise bar the suite had"""
    _, x, x0, jit, comps = ("float64",) + _emulate_joint("float64")
    for k, c in enumerate(comps):
        sig = c["sig"].copy()
        sig[_tile(3, 1)] *= 1 + 1e-9
        ch = sb.check_sigma(sig, c["U"], x0, c["th"], jit, "matern32", "float64")
        assert ch.ratio > 1 and ch.where == (3, 1), (k, ch)


def test_joint_defect_2_k_tile_of_the_product_dropped(joint):
    """tile (4, 2) of Sigma misses the K-tile 1 of D U U^T"""
    dtype, x, x0, jit, comps = joint
    r, cc = _tile(4, 2)
    kt = slice(TS, 2 * TS)
    for k, c in enumerate(comps):
        Dk = c["th"][D_IN + 2]
        sig = c["sig"].copy()
        sig[r, cc] = _r(sig[r, cc] + Dk * c["U"][r, kt] @ c["U"][cc, kt].T, dtype)
        ch = sb.check_sigma(sig, c["U"], x0, c["th"], jit, "matern32", dtype)
        assert ch.ratio > 1 and ch.where == (4, 2), (k, ch)


def test_joint_defect_3_tau_from_the_wrong_component():
    """tau = jitter scale_j of another component j (float64: in float32 jitter (scale_j - scale_k) is within the bound
    of the cancelling diagonal at jitter 1e-3)"""
    _, x, x0, jit, comps = ("float64",) + _emulate_joint("float64")
    for k, c in enumerate(comps):
        other = comps[(k + 1) % len(comps)]["th"][D_IN]
        sig = c["sig"] + jit * (other - c["th"][D_IN]) * np.eye(N0)
        ch = sb.check_sigma(sig, c["U"], x0, c["th"], jit, "matern32", "float64")
        assert ch.ratio > 1 and ch.where[0] == ch.where[1], (k, ch)


def test_joint_defect_4_diagonal_block_upper_triangle_not_zeroed(joint):
    """the draws read the 128-tile diagonal block 1 whole, and its upper 64-tile (2, 3) still holds Sigma (what the
    factorisation leaves there): draws of inputs 128 .. 191 pick up Sigma[128:192, 192:256] eps"""
    dtype, x, x0, jit, comps = joint
    for k, c in enumerate(comps):
        Lb = c["L"].copy()
        Lb[_tile(2, 3)] = c["sig"][_tile(2, 3)]
        draws = c["ghat"][None, :] + _r(_r(c["eps"], dtype) @ Lb.T, dtype)
        ch = sb.check_draws(draws, c["L"], c["eps"], c["ghat"], dtype)
        assert ch.ratio > 1 and ch.where[1] == 2, (k, ch)


def test_joint_defect_5_draws_shifted_at_a_chunk_split(joint):
    """the chunk of draws from 128 on reads eps one draw late"""
    dtype, x, x0, jit, comps = joint
    for k, c in enumerate(comps):
        draws = c["draws"].copy()
        draws[128:-1] = draws[129:]
        ch = sb.check_draws(draws, c["L"], c["eps"], c["ghat"], dtype)
        assert ch.ratio > 1 and ch.where[0] >= 2, (k, ch)
        assert sb.check_draws(draws[:128], c["L"], c["eps"][:128], c["ghat"], dtype).ratio < 0.5


def test_joint_defect_6_float32_sigma_in_a_float64_check():
    _, x, x0, jit, comps = ("float64",) + _emulate_joint("float64")
    for k, c in enumerate(comps):
        sig = _r(c["sig"], "float32")
        ch = sb.check_sigma(sig, c["U"], x0, c["th"], jit, "matern32", "float64")
        assert ch.ratio > 1, (k, ch)


def _blocked_cholesky(A, inverse):
    """right-looking 64-column blocked Cholesky in float64; the panel below each diagonal block by substitution or, as
    the library does, by a product with the inverse of the diagonal block"""
    import scipy.linalg as sla
    A = A.copy()
    n = A.shape[0]
    L = np.zeros_like(A)
    for c in range(0, n, TS):
        lcc = np.linalg.cholesky(A[c:c + TS, c:c + TS])
        L[c:c + TS, c:c + TS] = lcc
        if inverse:
            L[c + TS:, c:c + TS] = A[c + TS:, c:c + TS] @ sla.solve_triangular(lcc, np.eye(lcc.shape[0]), lower=True).T
        else:
            L[c + TS:, c:c + TS] = sla.solve_triangular(lcc, A[c + TS:, c:c + TS].T, lower=True).T
        A[c + TS:, c + TS:] -= L[c + TS:, c:c + TS] @ L[c + TS:, c:c + TS].T
    return L


def test_cov_factor_bound_covers_the_inverse_panel_solve():
    """Sigma of a smooth prior over 1025 new inputs with one training point (ill-conditioned 64 x 64 diagonal blocks):
    the factor by the library's algorithm (panel = A' W_cc^T) exceeds check_cholesky's bound, which only a substitution
    meets; check_cholesky_inverse_solve holds for both and still catches a tile off by 1e-12 in a well-conditioned one"""
    x = np.array([[0.92281364, 0.95399568, 0.79189991]])
    x0 = np.random.default_rng(811).uniform(-0.1, 1.1, (1025, D_IN))
    ell, scale, nug, Dk = np.array([1.72214102, 1.23222954, 0.83902513]), 1.57160803, 4.97589362e-4, 9.84779725
    nt = nug / (1 + nug)
    c00 = scale * ((1 - nt) * sb.kernel_parts(x0, x0, ell, "matern32", "float64")[0].numpy() + nt * np.eye(1025))
    c0 = scale * (1 - nt) * sb.kernel_parts(x0, x, ell, "matern32", "float64")[0].numpy()
    sig = c00 - Dk * (c0 @ c0.T) / (1 + Dk * scale) + 1e-8 * scale * np.eye(1025)
    Li, Ls = _blocked_cholesky(sig, True), _blocked_cholesky(sig, False)
    assert sb.check_cholesky(sig, Li, "float64").ratio > 1
    assert sb.check_cholesky(sig, Ls, "float64").ratio < 0.5
    assert sb.check_cholesky_inverse_solve(sig, Li, "float64").ratio < 0.5
    assert sb.check_cholesky_inverse_solve(sig, Ls, "float64").ratio < 0.5
    _, x, x0, jit, comps = ("float64",) + _emulate_joint("float64")
    for k, c in enumerate(comps):
        L = _blocked_cholesky(c["sig"], True)
        assert sb.check_cholesky_inverse_solve(c["sig"], L, "float64").ratio < 0.5
        L[_tile(3, 1)] *= 1 + 1e-12
        ch = sb.check_cholesky_inverse_solve(c["sig"], L, "float64")
        assert ch.ratio > 1 and ch.where == (3, 1), (k, ch)


# ----------------------------------------------------------------------------------------------------------------------
# post-fit queries: predict_grad (V = U W, the input gradients), leave-one-out, k-fold cross-validation, the integrated
# variance reduction.  The emulated fit carries sr (the rep path) where a check depends on it; every post-fit stage is
# computed in float64 from the previous stored stage and rounded to the storage type where the library stores it.
# ----------------------------------------------------------------------------------------------------------------------
def _normwise(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.max(np.abs(got - ref)) / np.max(np.abs(ref))


def _fit(x, Y, sr, th, dtype, kernel="matern32"):
    """the fitted workspace of the emulated path with sr: W = L^-1, V = A^-1, b, z (storage type)"""
    d = x.shape[1]
    A = _r(sb.reference_A(x, sr, th, kernel, dtype)[0].numpy(), dtype)
    L = _r(np.linalg.cholesky(A), dtype)
    W = np.tril(_r(np.linalg.solve(L, np.eye(x.shape[0])), dtype))
    V = _r(W.T @ W, dtype)
    b = _r(_r(Y, dtype).T @ th[d + 3:], dtype)
    z = _r(V @ b, dtype)
    return dict(W=W, V=V, b=b, z=z)


def _theta(d, seed, ell=None, scale=1.3, nug=0.01, Dk=5.0):
    rng = np.random.default_rng(seed)
    ell = rng.uniform(0.3, 0.9, d) * np.sqrt(d) if ell is None else np.asarray(ell, np.float64)
    return np.concatenate([ell, [scale, nug, Dk], rng.standard_normal(P)])


def _cross(x0, x, sr, th, dtype, kernel="matern32", match=None):
    """X = c_off C0(x0, x) o sr^T (+ the nugget term at column match[c]) in float64 from the rounded inputs"""
    d = x.shape[1]
    ell, scale, nug, Dk, _ = sb.split_theta(th, d)
    nt = nug / (1 + nug)
    s = np.ones(x.shape[0]) if sr is None else _r(sr, dtype)
    X = scale * (1 - nt) * sb.kernel_parts(_r(x0, dtype), _r(x, dtype), ell, kernel, dtype)[0].numpy() * s[None, :]
    if match is not None:
        for c, i in enumerate(match):
            if i >= 0:
                X[c, i] += scale * nt * s[i]
    return X


def _h(sl, kernel, rcp=None):
    """h of the input gradient, every kernel spelled out (numpy; rcp: the reciprocal the library's fast_rcp stands for)"""
    rcp = (lambda v: 1.0 / v) if rcp is None else rcp
    a = np.abs(sl)
    if kernel == "se":
        return sl
    if kernel == "matern32":
        return sl * rcp(1.0 + a)
    if kernel == "matern52":
        return (sl * a + sl) * rcp(a * (a + 3.0) + 3.0)
    raise ValueError(kernel)


def _pgrad(x0, x, sr, th, z, V, dtype, kernel="matern32", rcp=None, chunk_l0=None, drop=None, h_kernel=None):
    """dghat, dgvar (n0 x d) of the contraction in float64; defects: rcp (the reciprocal in h), chunk_l0 (dimensions from
    chunk_l0 on computed with the s of dimension l - chunk_l0), drop (training inputs left out of dgvar), h_kernel (dghat
    formed with the h of another kernel)"""
    d = x.shape[1]
    ell, scale, nug, Dk, _ = sb.split_theta(th, d)
    s = np.ones(x.shape[0]) if sr is None else _r(sr, dtype)
    c0 = _cross(x0, x, None, th, dtype, kernel)
    a, b = _r(x0, dtype), _r(x, dtype)
    pz = c0 * (s * z)[None, :]
    pv = c0 * s[None, :] * V
    if drop is not None:
        pv = pv.copy()
        pv[:, drop] = 0.0
    gh, gv = np.zeros((x0.shape[0], d)), np.zeros((x0.shape[0], d))
    for l in range(d):
        ls = l - chunk_l0 if (chunk_l0 is not None and l >= chunk_l0) else l
        sl = a[:, ls][:, None] / ell[ls] - b[:, ls][None, :] / ell[ls]
        h = _h(sl, kernel, rcp)
        gh[:, l] = -(pz * (h if h_kernel is None else _h(sl, h_kernel, rcp))).sum(axis=1) / ell[l]
        gv[:, l] = 2 * Dk * (pv * h).sum(axis=1) / ell[l]
    return gh, gv


def _pgrad_problem(dtype, d=D_IN, n=N, n0=70, kernel="matern32", rep=False, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (n, d))
    Y = rng.standard_normal((P, n))
    sr = np.sqrt(rng.integers(1, 6, n).astype(np.float64)) if rep else None
    th = _theta(d, seed + 1)
    e = _fit(x, Y, sr, th, dtype, kernel)
    x0 = np.concatenate([x[:5], rng.uniform(-0.1, 1.1, (n0 - 5, d))])      # training inputs among x0: dx = 0
    U = _r(_r(_cross(x0, x, sr, th, dtype, kernel), dtype) @ e["W"].T, dtype)
    Vp = _r(U @ e["W"], dtype)                                               # V = U W of predict_grad (Vp here)
    gh, gv = _pgrad(x0, x, sr, th, e["z"], Vp, dtype, kernel)
    return dict(x=x, sr=sr, th=th, x0=x0, U=U, Vp=Vp, gh=gh, gv=gv, **e)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_emulated_predict_grad_passes(dtype, kernel):
    for rep in (False, True):
        g = _pgrad_problem(dtype, kernel=kernel, rep=rep)
        assert sb.check_pgrad_v(g["Vp"], g["U"], g["W"], dtype).ratio < 0.5
        c = sb.check_pgrad(g["gh"], g["gv"], g["x0"], g["x"], g["sr"], g["th"], g["z"], g["Vp"], kernel, dtype)
        assert c.ratio < 0.5, c


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_pgrad_defect_1_v_block_from_the_wrong_component(dtype):
    """rows 32 .. 63 of V (one PG_ROWS block) formed from the U of the next component"""
    g = _pgrad_problem(dtype)
    g2 = _pgrad_problem(dtype, seed=9)
    V = g["Vp"].copy()
    V[32:64] = g2["Vp"][32:64]
    c = sb.check_pgrad_v(V, g["U"], g["W"], dtype)
    assert c.ratio > 1 and c.where[0] == 0, c


def test_pgrad_defect_2_wide_chunk_with_l0_zero():
    """d = 40: the second 32-dimension chunk (blockIdx.z = 1) computed with l0 = 0 -- dimensions 32 .. 39 carry the scaled
    distances of 0 .. 7, divided by their own lengthscales"""
    for dtype in ("float64", "float32"):
        g = _pgrad_problem(dtype, d=40, n=150, n0=40)
        gh, gv = _pgrad(g["x0"], g["x"], None, g["th"], g["z"], g["Vp"], dtype, chunk_l0=32)
        c = sb.check_pgrad(gh, gv, g["x0"], g["x"], None, g["th"], g["z"], g["Vp"], "matern32", dtype)
        assert c.ratio > 1 and int(c.where[1].split("l")[-1]) >= 32, c


def test_pgrad_defect_3_float32_reciprocal_in_h():
    """h = s rcp(1 + |s|) with the reciprocal carrying float32 accuracy only (no Newton steps), in the float64 path"""
    g = _pgrad_problem("float64")
    gh, gv = _pgrad(g["x0"], g["x"], None, g["th"], g["z"], g["Vp"], "float64", rcp=lambda v: np.float32(1.0) / v.astype(np.float32))
    c = sb.check_pgrad(gh, gv, g["x0"], g["x"], None, g["th"], g["z"], g["Vp"], "matern32", "float64")
    assert c.ratio > 1, c


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_pgrad_defect_4_stage_of_training_inputs_left_out_of_dgvar(dtype):
    """one LDS stage of JT = 32 training inputs (64 .. 95) missing from the dgvar sum"""
    g = _pgrad_problem(dtype, rep=True)
    gh, gv = _pgrad(g["x0"], g["x"], g["sr"], g["th"], g["z"], g["Vp"], dtype, drop=slice(64, 96))
    c = sb.check_pgrad(g["gh"], gv, g["x0"], g["x"], g["sr"], g["th"], g["z"], g["Vp"], "matern32", dtype)
    assert c.ratio > 1 and c.where[1].startswith("dgvar"), c


# ---- leave-one-out -----------------------------------------------------------------------------------------------------
def _loo(V, b, z, sr, Dk):
    a = np.diag(V)
    s = np.ones_like(b) if sr is None else sr
    return (b - z / a) / (Dk * s), (1 / a - 1) / (Dk * s * s)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_emulated_loo_passes_and_defects_fail(dtype):
    for rep in (False, True):
        g = _pgrad_problem(dtype, rep=rep)
        sr = None if g["sr"] is None else _r(g["sr"], dtype)
        Dk = g["th"][D_IN + 2]
        gh, gv = _loo(g["V"], g["b"], g["z"], sr, Dk)
        assert sb.check_loo(gh, gv, g["V"], g["b"], g["z"], g["sr"], g["th"], dtype, D_IN).ratio < 0.5
        # defect 1: a_ii of component k + 1 (another theta, same inputs)
        g2 = _fit(g["x"], np.random.default_rng(4).standard_normal((P, N)), g["sr"], _theta(D_IN, 11), dtype)
        bad = _loo(np.diag(np.diag(g2["V"])), g["b"], g["z"], sr, Dk)
        c = sb.check_loo(bad[0], bad[1], g["V"], g["b"], g["z"], g["sr"], g["th"], dtype, D_IN)
        assert c.ratio > 1, c
        # defect 2 (rep path): gvar divided by s_i instead of s_i^2
        if rep:
            c = sb.check_loo(gh, gv * sr, g["V"], g["b"], g["z"], g["sr"], g["th"], dtype, D_IN)
            assert c.ratio > 1, c


# ---- k-fold --------------------------------------------------------------------------------------------------------------
FOLD_SIZES = (65, 129, 1, 105)          # mmax = 129: mpad = 256, four 64-tiles per side


def _folds(n, sizes, seed):
    perm = np.random.default_rng(seed).permutation(n)
    out, lo = [], 0
    for m in sizes:
        out.append(np.sort(perm[lo:lo + m]))
        lo += m
    assert lo == n
    return out


def _raw_V(V, seed):
    """lower storage of A^-1 as the library holds it: the strict upper triangle never written (garbage)"""
    g = np.random.default_rng(seed).uniform(-1e3, 1e3, V.shape)
    return np.tril(V) + np.triu(g, 1)


def _gather(Vraw, idx, mpad, upper_bug=False):
    M = np.eye(mpad)
    ii, jj = np.meshgrid(idx, idx, indexing="ij")
    m = len(idx)
    M[:m, :m] = Vraw[ii, jj] if upper_bug else Vraw[np.maximum(ii, jj), np.minimum(ii, jj)]
    return M


def _sym(M):
    return np.tril(M) + np.tril(M, -1).T


def _cv_emulate(dtype, rep=True):
    g = _pgrad_problem(dtype, rep=rep)
    folds = _folds(N, FOLD_SIZES, 5)
    mmax = max(FOLD_SIZES)
    mpad = sb._pad128(mmax)
    Vraw = _raw_V(g["V"], 6)
    sr = None if g["sr"] is None else _r(g["sr"], dtype)
    Dk = g["th"][D_IN + 2]
    res = []
    for idx in folds:
        slot = _gather(Vraw, idx, mpad)
        M = _sym(slot)[:mmax, :mmax]
        L = _r(np.linalg.cholesky(M), dtype)
        W = np.tril(_r(np.linalg.solve(L, np.eye(mmax)), dtype))
        Mi = _r(W.T @ W, dtype)
        m = len(idx)
        s = np.ones(m) if sr is None else sr[idx]
        t = Mi[:m, :m] @ g["z"][idx]
        res.append(dict(idx=idx, slot=slot, M=M, L=L, W=W, Mi=Mi, t=t, s=s,
                        gh=(g["b"][idx] - t) / (Dk * s), gv=(np.diag(Mi)[:m] - 1) / (Dk * s * s)))
    return g, Vraw, mmax, res


@pytest.fixture(scope="module", params=["float64", "float32"])
def cv(request):
    return (request.param,) + _cv_emulate(request.param)


def _scatter(res, n):
    gh, gv = np.full(n, np.nan), np.full(n, np.nan)
    for f in res:
        gh[f["idx"]], gv[f["idx"]] = f["gh"], f["gv"]
    return gh, gv


def test_emulated_cv_passes_every_stage(cv):
    dtype, g, Vraw, mmax, res = cv
    gh, gv = _scatter(res, N)
    for f in res:
        assert sb.check_cv_gather(f["slot"], g["V"], f["idx"], mmax).ratio == 0
        assert sb.check_cholesky_inverse_solve(f["M"], f["L"], dtype).ratio < 0.5
        assert sb.check_inverse_factor(f["L"], f["W"], dtype).ratio < 0.5
        assert sb.check_inverse(f["W"], f["Mi"], dtype).ratio < 0.5
        c = sb.check_cv_apply(gh, gv, f["Mi"], g["b"], g["z"], g["sr"], g["th"], f["idx"], dtype, D_IN)
        assert c.ratio < 0.5, c


def test_cv_defect_1_upper_tile_gathered_from_unwritten_storage(cv):
    dtype, g, Vraw, mmax, res = cv
    f = res[1]                                            # the 129-input fold: tiles (1, 0), (2, 0), (2, 1) and the diagonals
    slot = _gather(Vraw, f["idx"], sb._pad128(mmax), upper_bug=True)
    c = sb.check_cv_gather(slot, g["V"], f["idx"], mmax)
    assert c.ratio > 1, c
    slot = f["slot"].copy()
    slot[200, 200] = 0.0                                  # the identity padding beyond m_f not written
    assert sb.check_cv_gather(slot, g["V"], f["idx"], mmax).ratio > 1


def test_cv_defect_2_fold_scattered_one_position_off(cv):
    dtype, g, Vraw, mmax, res = cv
    gh, gv = _scatter(res, N)
    f = res[3]
    gh[f["idx"][1:]] = f["gh"][:-1]
    c = sb.check_cv_apply(gh, gv, f["Mi"], g["b"], g["z"], g["sr"], g["th"], f["idx"], dtype, D_IN)
    assert c.ratio > 1, c


def test_cv_defect_3_above_diagonal_tile_read_untransposed(cv):
    """the apply reads the stored tile (1, 0) of M^-1 for the block (0, 1) without transposing it: t of the fold's first 64
    positions is wrong"""
    dtype, g, Vraw, mmax, res = cv
    f = res[1]
    m = len(f["idx"])
    Mb = f["Mi"][:m, :m].copy()
    Mb[0:64, 64:128] = f["Mi"][64:128, 0:64]
    Dk = g["th"][D_IN + 2]
    t = Mb @ g["z"][f["idx"]]
    gh, gv = _scatter(res, N)
    gh[f["idx"]] = (g["b"][f["idx"]] - t) / (Dk * f["s"])
    c = sb.check_cv_apply(gh, gv, f["Mi"], g["b"], g["z"], g["sr"], g["th"], f["idx"], dtype, D_IN)
    assert c.ratio > 1 and c.where == (0,), c


# ---- integrated variance reduction -----------------------------------------------------------------------------------------
N_REF, N_CAND, VR_XBLK = 2100, 70, 2048


def _vr_out(Ur, Uc, xr, xc, w, th, r, dtype, kernel="matern32", den_r=None):
    d = xr.shape[1]
    ell, scale, nug, Dk, _ = sb.split_theta(th, d)
    ct = scale * (1 - nug / (1 + nug)) * sb.kernel_parts(_r(xr, dtype), _r(xc, dtype), ell, kernel, dtype)[0].numpy()
    sig = ct - Dk * _r(Ur @ Uc.T, dtype)
    gv = scale - Dk * np.sum(Uc * Uc, axis=1)
    den = np.maximum(gv, 0) + 1 / (Dk * (r if den_r is None else den_r))
    return (w[:, None] * sig * sig).sum(axis=0) / den


def _vr_emulate(dtype, kernel="matern32"):
    g = _pgrad_problem(dtype, rep=True, kernel=kernel)
    rng = np.random.default_rng(12)
    xr = rng.uniform(-0.1, 1.1, (N_REF, D_IN))
    xc = rng.uniform(-0.1, 1.1, (N_CAND, D_IN))
    xc[:4] = g["x"][[7, 20, 33, 298]]                  # matched candidates: replicates of training inputs
    match = -np.ones(N_CAND, np.int64)
    match[:4] = [7, 20, 33, 298]
    w = rng.uniform(0.0, 1.0, N_REF)
    w[::7] = 0.0
    w /= w.sum()
    Ur = _r(_r(_cross(xr, g["x"], g["sr"], g["th"], dtype, kernel), dtype) @ g["W"].T, dtype)
    Uc = _r(_r(_cross(xc, g["x"], g["sr"], g["th"], dtype, kernel, match), dtype) @ g["W"].T, dtype)
    r = 3
    out = _vr_out(Ur, Uc, xr, xc, w, g["th"], r, dtype, kernel)
    return dict(g=g, xr=xr, xc=xc, match=match, w=w, Ur=Ur, Uc=Uc, r=r, out=out, kernel=kernel)


@pytest.fixture(scope="module", params=["float64", "float32"])
def vr(request):
    return request.param, _vr_emulate(request.param)


@pytest.fixture(scope="module")
def vr64():
    """float64 only, for the defects of a size the float32 bound cannot resolve: Sigma = C - D U_r . U_c cancels (the
    posterior covariance is small against the prior), so in float32 its bound delta is of the size of Sigma itself and the
    bound on out of the size of out (a dropped tile of 52 reference rows, a 1 % change of a matched U_c, den with r = 1)"""
    return "float64", _vr_emulate("float64")


def _check_vr(v, out, dtype, match="same", r=None):
    g = v["g"]
    return sb.check_vr(out, v["xr"], v["w"], v["xc"], v["match"] if match == "same" else match, v["r"] if r is None else r,
                       g["x"], g["sr"], g["th"], g["W"], v["kernel"], dtype)


def test_emulated_vr_passes(vr):
    dtype, v = vr
    assert _check_vr(v, v["out"], dtype).ratio < 0.5
    for kernel in ("se", "matern52"):
        v2 = _vr_emulate(dtype, kernel)
        assert _check_vr(v2, v2["out"], dtype).ratio < 0.5, kernel


def test_vr_defect_1_last_reference_tile_left_out(vr64):
    dtype, v = vr64
    last = (N_REF - 1) // TS * TS
    w = v["w"].copy()
    w[last:] = 0.0
    out = _vr_out(v["Ur"], v["Uc"], v["xr"], v["xc"], w, v["g"]["th"], v["r"], dtype)
    assert _check_vr(v, out, dtype).ratio > 1


def test_vr_defect_2_reference_row_beyond_n_ref_weighted(vr):
    """a padding row of the last reference tile (x_ref staged as 0, U row 0) given the weight of row 1"""
    dtype, v = vr
    xr = np.concatenate([v["xr"], np.zeros((1, D_IN))])
    Ur = np.concatenate([v["Ur"], np.zeros((1, v["Ur"].shape[1]))])
    w = np.concatenate([v["w"], v["w"][1:2]])
    out = _vr_out(Ur, v["Uc"], xr, v["xc"], w, v["g"]["th"], v["r"], dtype)
    assert _check_vr(v, out, dtype).ratio > 1


def test_vr_defect_3_nugget_term_of_a_match_on_the_wrong_column(vr64):
    dtype, v = vr64
    g = v["g"]
    wrong = np.where(v["match"] >= 0, v["match"] + 1, -1)
    Uc = _r(_r(_cross(v["xc"], g["x"], g["sr"], g["th"], dtype, "matern32", wrong), dtype) @ g["W"].T, dtype)
    out = _vr_out(v["Ur"], Uc, v["xr"], v["xc"], v["w"], g["th"], v["r"], dtype)
    c = _check_vr(v, out, dtype)
    assert c.ratio > 1 and c.where == (0,), c


def test_vr_defect_4_r_ignored_in_the_denominator(vr64):
    dtype, v = vr64
    out = _vr_out(v["Ur"], v["Uc"], v["xr"], v["xc"], v["w"], v["g"]["th"], v["r"], dtype, den_r=1)
    assert _check_vr(v, out, dtype).ratio > 1


def test_vr_defect_5_second_pass_written_at_row_zero(vr):
    """n_ref = 2100 is formed in two passes of VR_XBLK = 2048 rows; the second pass's U lands on rows 0 .. 51 and rows
    2048 .. 2099 keep what the scratch held (zeros here)"""
    dtype, v = vr
    Ur = v["Ur"].copy()
    Ur[:N_REF - VR_XBLK] = v["Ur"][VR_XBLK:]
    Ur[VR_XBLK:] = 0.0
    out = _vr_out(Ur, v["Uc"], v["xr"], v["xc"], v["w"], v["g"]["th"], v["r"], dtype)
    assert _check_vr(v, out, dtype).ratio > 1


# ----------------------------------------------------------------------------------------------------------------------
# input dimensions: the bounds at the widths of for_dim's last bucket (d = 17) and of four wide chunks (d = 126), and the
# defects of the d-templated build and gradient kernels -- a chunk of lengthscales off by 32 dimensions, stale padding
# dimensions, one lengthscale gradient off in the fourth chunk, swapped accumulator slots -- and of predict at training rows
# ----------------------------------------------------------------------------------------------------------------------
N_WIDE = 200


def _wide_problem(d, seed=0, n=N_WIDE):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (n, d))
    Y = rng.standard_normal((P, n))
    return x, Y, _theta(d, seed + 1)


@pytest.fixture(scope="module")
def wide():
    """d -> (x, Y, th) at d = 17, 33 and 126 (ell uniform in [0.3, 0.9] sqrt(d): every dimension distinct)"""
    return {d: _wide_problem(d, seed=40 + d) for d in (17, 33, 126)}


def _contraction(e, x, th, dtype, kernel="matern32"):
    """the accumulators of grad_kernel in float64 from the emulated V, z: sum G F_l (l < d), sum G C0, trace G"""
    d = x.shape[1]
    ell, scale, nug, Dk, _ = sb.split_theta(th, d)
    V, z = torch.as_tensor(e["V"]), torch.as_tensor(e["z"])
    G = 0.5 * Dk * V - 0.5 * z[:, None] * z[None, :]
    xr = sb.rounded(x, dtype)
    c0 = sb.kernel_parts(xr, xr, ell, kernel, "float64")[0]
    return [float((G * f).sum()) for f in sb.dC0(xr, xr, ell, kernel)] + [float((G * c0).sum()), float(torch.trace(G))]


def _finalize(out, sums, th, d):
    """the gradient slots of an output row from the accumulators, as finalize_kernel forms them"""
    ell, scale, nug, Dk, _ = sb.split_theta(th, d)
    nt = nug / (1 + nug)
    out = out.copy()
    for l in range(d):
        out[3 + l] = scale * (1 - nt) / ell[l] * sums[l]
    out[3 + d] = (1 - nt) * sums[d] + nt * sums[d + 1]
    out[4 + d] = scale * (sums[d + 1] - sums[d]) / (1 + nug) ** 2
    return out


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_emulated_path_passes_at_wide_dimensions(wide, dtype, kernel):
    for d in (17, 126):
        x, Y, th = wide[d]
        e = _emulate(x, Y, th, dtype, kernel)
        for stage, c in _checks(e, x, Y, th, dtype, kernel).items():
            assert c.ratio < 0.5, (d, stage, c)
        x0 = np.random.default_rng(d).uniform(-0.1, 1.1, (37, d))
        X = _cross(x0, x, None, th, dtype, kernel)
        gvar = th[d] - th[d + 2] * np.sum((X @ e["W"].T) ** 2, axis=1)
        c = sb.check_predict(X @ e["z"], gvar, x0, x, None, th, e["W"], e["z"], kernel, dtype)
        assert c.ratio < 0.5, (d, "predict", c)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_wide_defect_1_last_chunk_with_the_lengthscales_of_the_previous_one(wide, dtype, kernel):
    """d = 126: the dimensions 96 .. 125 of A staged with ell[64 .. 93] (d0 off by 32 in the last chunk)"""
    x, Y, th = wide[126]
    bad = th.copy()
    bad[96:126] = th[64:94]
    A = _r(sb.reference_A(x, None, bad, kernel, dtype)[0].numpy(), dtype)
    b = _emulate(x, Y, th, dtype, kernel)["b"]
    assert sb.check_build(_r(sb.reference_A(x, None, th, kernel, dtype)[0].numpy(), dtype), b, x, Y, None, th, kernel,
                          dtype).ratio < 0.5
    c = sb.check_build(A, b, x, Y, None, th, kernel, dtype)
    assert c.ratio > 1, c


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_wide_defect_2_stale_padding_dimensions(wide, dtype, kernel):
    """d = 33: the second chunk holds dimension 32 and 31 padding columns, which keep the first chunk's staged columns 1 ..
    31 instead of zeros -- those dimensions count twice in the exponent (and in the Matern polynomial)"""
    x, Y, th = wide[33]
    ell, scale, nug, Dk, _ = sb.split_theta(th, 33)
    nt = nug / (1 + nug)
    xr = _r(x, dtype)
    c0 = sb.kernel_parts(xr, xr, ell, kernel, "float64")[0].numpy()
    extra = sb.kernel_parts(xr[:, 1:32], xr[:, 1:32], ell[1:32], kernel, "float64")[0].numpy()
    A = _r(np.eye(N_WIDE) + Dk * scale * ((1 - nt) * c0 * extra + nt * np.eye(N_WIDE)), dtype)
    b = _emulate(x, Y, th, dtype, kernel)["b"]
    c = sb.check_build(A, b, x, Y, None, th, kernel, dtype)
    assert c.ratio > 1, c


def test_wide_defect_3_one_lengthscale_gradient_off_in_the_fourth_chunk(wide):
    """d = 126, float64: g_ell_110 (fourth 32-dimension chunk) off by 1e-8 relative.  check_outputs names that entry; the
    oracle bar max|dg| <= 1e-5 max|g| of the parity tests passes it"""
    x, Y, th = wide[126]
    e = _emulate(x, Y, th, "float64")
    out = e["out"].copy()
    out[3 + 110] *= 1 + 1e-8
    c = sb.check_outputs(out, x, Y, None, th, e["V"], e["b"], e["z"], "matern32", "float64")
    assert c.ratio > 1 and c.where == ("g_ell110",), c
    g, gbad = e["out"][3:], out[3:]
    assert np.max(np.abs(gbad - g)) <= 1e-5 * np.max(np.abs(g))


@pytest.mark.parametrize("d", [5, 17, 126])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_wide_defect_4_swapped_accumulator_slots(wide, dtype, d):
    """g_scale / g_nug formed from the wrong accumulators of the partial row (grad_kernel's e = tid < d ? tid : DD + tid - d
    mapping): the two swapped, or each read one slot early (g_scale from the g_ell_{d-1} accumulator)"""
    x, Y, th = wide[d] if d in wide else _wide_problem(d, seed=40 + d)
    e = _emulate(x, Y, th, dtype)
    sums = _contraction(e, x, th, dtype)
    ok = _finalize(e["out"], sums, th, d)
    assert sb.check_outputs(ok, x, Y, None, th, e["V"], e["b"], e["z"], "matern32", dtype).ratio < 0.5
    swapped = sums[:d] + [sums[d + 1], sums[d]]
    early = sums[:d] + [sums[d - 1], sums[d]]
    for bad in (swapped, early):
        c = sb.check_outputs(_finalize(e["out"], bad, th, d), x, Y, None, th, e["V"], e["b"], e["z"], "matern32", dtype)
        assert c.ratio > 1 and c.where[0] in ("g_scale", "g_nug"), c


@pytest.mark.parametrize("rep", [False, True])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_predict_defect_nugget_one_row_off(dtype, rep):
    """x0 = the training rows 10 .. 109 (same = 11): check_predict(same = 11) passes the predictions and fails them with the
    nugget term one column early (same = 10), one late (12) or missing (0)"""
    g = _pgrad_problem(dtype, rep=rep)
    x, sr, th = g["x"], g["sr"], g["th"]
    lo, m = 10, 100
    x0 = x[lo:lo + m]
    X = _cross(x0, x, sr, th, dtype, match=np.arange(lo, lo + m))
    ghat = X @ g["z"]
    gvar = th[D_IN] - th[D_IN + 2] * np.sum((X @ g["W"].T) ** 2, axis=1)
    assert sb.check_predict(ghat, gvar, x0, x, sr, th, g["W"], g["z"], "matern32", dtype, same=lo + 1).ratio < 0.5
    for same in (lo, lo + 2, 0):
        c = sb.check_predict(ghat, gvar, x0, x, sr, th, g["W"], g["z"], "matern32", dtype, same=same)
        assert c.ratio > 1, (same, c)


# ----------------------------------------------------------------------------------------------------------------------
# Matern-5/2: pins of kernel_parts / dC0 / pgrad_h that do not go through them, the magnification E against build_kernel's
# float32 operation order, and the wrong-kernel defects
# ----------------------------------------------------------------------------------------------------------------------
M52_DIMS = (1, 3, 17, 40)


def _m52_points(d, seed):
    """x1 (23 x d) and x2 (31 x d) in the unit box; rows 0 .. 4 of x1 coincide with rows 7 .. 11 of x2"""
    rng = np.random.default_rng(seed)
    x1, x2 = rng.uniform(0.0, 1.0, (23, d)), rng.uniform(0.0, 1.0, (31, d))
    x1[:5] = x2[7:12]
    ell = rng.uniform(0.3, 0.9, d) * np.sqrt(d)
    return x1, x2, ell


def _c0_m52_torch(a, b, logell):
    """prod_l (1 + S_l + S_l^2 / 3) exp(-sum_l S_l) restated from the oracle's definition, differentiable in a and log ell"""
    s = ((a[:, None, :] - b[None, :, :]) / torch.exp(logell)).abs()
    return torch.prod(1.0 + s + s * s / 3.0, dim=2) * torch.exp(-s.sum(dim=2))


def test_unknown_kernel_name_is_an_error():
    x = np.zeros((2, 1))
    for name in ("matern", "matern12", "rbf", None):
        with pytest.raises(ValueError):
            sb.kernel_parts(x, x, [1.0], name, "float64")
        with pytest.raises(ValueError):
            sb.dC0(x, x, [1.0], name)
        with pytest.raises(ValueError):
            sb.pgrad_h(torch.zeros(2, dtype=torch.float64), name)
        with pytest.raises(ValueError):
            sb.check_pgrad(np.zeros((2, 1)), np.zeros((2, 1)), x, x, None, [1.0, 1.0, 0.01, 1.0], np.zeros(2), np.zeros((2, 2)),
                           name, "float64")


@pytest.mark.parametrize("d", M52_DIMS)
def test_matern52_c0_against_the_oracle(d):
    """kernel_parts' Matern-5/2 C0 against tests/matern52_oracle.c0_matern52 (pinned by the identities of
    tests/test_matern52_oracle.py), float64, 1e-14 relative: rectangular x1 != x2 with coincident rows, and x1 = x2"""
    from tests import matern52_oracle as m52
    x1, x2, ell = _m52_points(d, 60 + d)
    for a, b in ((x1, x2), (x2, x2)):
        c0, e, cut = sb.kernel_parts(a, b, ell, "matern52", "float64")
        ref = m52.c0_matern52(a / ell, b / ell)
        assert np.all(np.abs(c0.numpy() - ref) <= 1e-14 * np.abs(ref))
        assert not bool(cut.any())
    assert np.all(sb.kernel_parts(x1, x2, ell, "matern52", "float64")[0].numpy()[np.arange(5), np.arange(7, 12)] == 1.0)
    assert np.all(np.diag(sb.kernel_parts(x2, x2, ell, "matern52", "float64")[0].numpy()) == 1.0)
    # the restatement the autograd pins below differentiate is the same function
    t = _c0_m52_torch(torch.as_tensor(x1), torch.as_tensor(x2), torch.as_tensor(np.log(ell))).numpy()
    ref = m52.c0_matern52(x1 / ell, x2 / ell)
    assert np.all(np.abs(t - ref) <= 1e-14 * np.abs(ref))


@pytest.mark.parametrize("d", M52_DIMS)
def test_matern52_dc0_and_h_against_autograd(d):
    """dC0 = ell_l dC0 / d ell_l against autograd of C0 in log ell, and h, defined by dC0 / dx0_l = -C0 h_l / ell_l, against
    autograd of C0 in x0: float64, 1e-10 of the largest entry per dimension"""
    x1, x2, ell = _m52_points(d, 70 + d)
    a, b = torch.as_tensor(x1), torch.as_tensor(x2)
    le = torch.as_tensor(np.log(ell))
    J = torch.autograd.functional.jacobian(lambda t: _c0_m52_torch(a, b, t), le)             # (n1, n2, d)
    F = sb.dC0(x1, x2, ell, "matern52")
    assert len(F) == d
    for l in range(d):
        ref = J[:, :, l]
        assert float((F[l] - ref).abs().max()) <= 1e-10 * float(ref.abs().max()), l
    c0 = sb.kernel_parts(x1, x2, ell, "matern52", "float64")[0]
    Jx = torch.autograd.functional.jacobian(lambda t: _c0_m52_torch(t, b, le), a)            # (n1, n2, n1, d)
    i = torch.arange(a.shape[0])
    Jx = Jx[i, :, i, :]                                                                      # (n1, n2, d): row i by x0_i
    for l in range(d):
        sl = a[:, l][:, None] / ell[l] - b[:, l][None, :] / ell[l]
        got = -c0 * sb.pgrad_h(sl, "matern52") / ell[l]
        ref = Jx[:, :, l]
        assert float((got - ref).abs().max()) <= 1e-10 * float(ref.abs().max()), l
        assert float(sb.pgrad_h(sl, "matern52").abs().max()) < 1.0
        assert bool(torch.all(sb.pgrad_h(sl, "matern52")[:5][i[:5], i[:5] + 7] == 0.0))      # coincident points: h = 0


def _f32(v):
    return np.asarray(v, np.float32)


def _fma32(a, b, c):
    """fma in float32: the product of two float32 is exact in float64 (48 bits), the sum is rounded to float64 and then to
    float32 -- a single rounding but for the rare double-rounding ties"""
    with np.errstate(over="ignore", invalid="ignore"):
        return _f32(a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64))


def _build_kernel_f32_matern52(x, th):
    """A of build_kernel<float, DD, 2> (sr = 1), operation by operation in float32: x / ell formed in double and rounded;
    per dimension sd = |xa - xb|, m52_fm1 = fma(sd * (1/3), sd, sd), poly = fma(poly, fm1, poly), ssum -= sd; then
    c0 = min(poly, 1e38) exp(ssum) with __expf = exp2 of the float32 product with log2(e), v = (ss c_off) c0 and, on the
    diagonal, v += 1 + (c_diag - 1) ss.  Written from lcgp_hip.hip, independent of stage_bounds."""
    n, d = x.shape
    ell, scale, nug, Dk = th[:d], th[d], th[d + 1], th[d + 2]
    nt = nug / (1.0 + nug)
    xs = _f32(_f32(x).astype(np.float64) / ell)
    third = np.float32(1.0 / 3.0)
    poly = np.ones((n, n), np.float32)
    ssum = np.zeros((n, n), np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for l in range(d):
            sd = np.abs(xs[:, l][:, None] - xs[:, l][None, :])
            fm1 = _fma32(sd * third, sd, sd)
            poly = _fma32(poly, fm1, poly)
            ssum = ssum - sd
        arg = ssum * np.float32(1.4426950408889634)
        ex = _f32(np.exp2(arg.astype(np.float64)))
        c0 = np.fmin(poly, np.float32(1e38)) * ex
        c_off, c_diag = np.float32(Dk * scale * (1.0 - nt)), np.float32(1.0 + Dk * scale * nt)
        ss = np.float32(1.0) * np.float32(1.0)
        v = (ss * c_off) * c0
        v[np.diag_indices(n)] += np.float32(1.0) + (c_diag - np.float32(1.0)) * ss
    assert v.dtype == np.float32
    return v.astype(np.float64)


@pytest.mark.parametrize("ells", ["collapsed", "long"])
@pytest.mark.parametrize("d", [1, 6, 10, 33, 126])
def test_matern52_magnification_against_build_kernel_order(d, ells):
    """the constant 3 d + 3 of kernel_parts' Matern-5/2 E: an emulation of build_kernel's float32 operation order passes
    check_build below 0.5.  collapsed: the mean exponent at 0.9 times the float32 cut-off (entries on both sides of it, S_l
    up to ~ 250 / d per dimension); long: S_l ~ 0.03, the polynomial's roundings are all there is.  Past the cut-off
    check_build's bound is |A_ij| itself (the exponential is a denormal or zero there, whatever the polynomial): the whole
    matrix is held to ratio <= 1, and to < 0.5 with the entries past the cut-off taken from the reference, so that E alone
    is what the 0.5 measures."""
    rng = np.random.default_rng(80 + d)
    n = 130
    x = rng.uniform(0.0, 1.0, (n, d))
    Y = rng.standard_normal((P, n))
    if ells == "collapsed":
        ell = d / (3.0 * 0.9 * abs(sb.EXP_FLOOR["float32"])) * np.exp(rng.uniform(-0.15, 0.15, d))
    else:
        ell = 10.0 * np.exp(rng.uniform(-0.15, 0.15, d))
    th = _theta(d, 81 + d, ell=ell)
    A = _build_kernel_f32_matern52(x, th)
    assert np.all(np.isfinite(A))
    cut = sb.kernel_parts(_r(x, "float32"), _r(x, "float32"), ell, "matern52", "float32")[2].numpy()
    if ells == "collapsed":
        assert 0.05 < cut.mean() < 0.95, cut.mean()
        assert sb.check_build(A, None, x, Y, None, th, "matern52", "float32").ratio <= 1.0
        A = np.where(cut, _r(sb.reference_A(x, None, th, "matern52", "float32")[0].numpy(), "float32"), A)
    else:
        assert not cut.any()
    c = sb.check_build(A, None, x, Y, None, th, "matern52", "float32")
    assert c.ratio < 0.5, c
    # teeth: the same matrix with one far tile's polynomial evaluated as Matern-3/2 fails (long lengthscales: inside the cut)
    if ells == "long":
        bad = A.copy()
        bad[_tile(1, 0)] = _r(sb.reference_A(x, None, th, "matern32", "float32")[0].numpy(), "float32")[_tile(1, 0)]
        c = sb.check_build(bad, None, x, Y, None, th, "matern52", "float32")
        assert c.ratio > 1 and c.where == (1, 0), c


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_matern52_defect_1_far_tile_of_A_with_matern32_values(prob, dtype):
    """the far-off-diagonal 64-tile (4, 0) of A holds the Matern-3/2 kernel"""
    x, Y, th = prob
    e = _emulate(x, Y, th, dtype, "matern52")
    assert sb.check_build(e["A"], e["b"], x, Y, None, th, "matern52", dtype).ratio < 0.5
    A = e["A"].copy()
    A[_tile(4, 0)] = _emulate(x, Y, th, dtype, "matern32")["A"][_tile(4, 0)]
    c = sb.check_build(A, e["b"], x, Y, None, th, "matern52", dtype)
    assert c.ratio > 1 and c.where == (4, 0), c


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_matern52_defect_2_one_lengthscale_slot_with_the_matern32_weight(wide, dtype):
    """d = 126: g_ell_100 (fourth 32-dimension chunk) contracted with S^2 / (1 + S) in place of S^2 (1 + S) / (3 f(S))"""
    d, l = 126, 100
    x, Y, th = wide[d]
    e = _emulate(x, Y, th, dtype, "matern52")
    sums = _contraction(e, x, th, dtype, "matern52")
    ok = _finalize(e["out"], sums, th, d)
    assert sb.check_outputs(ok, x, Y, None, th, e["V"], e["b"], e["z"], "matern52", dtype).ratio < 0.5
    ell, scale, nug, Dk, _ = sb.split_theta(th, d)
    V, z = torch.as_tensor(e["V"]), torch.as_tensor(e["z"])
    G = 0.5 * Dk * V - 0.5 * z[:, None] * z[None, :]
    xr = torch.as_tensor(sb.rounded(x, dtype))
    c0 = sb.kernel_parts(xr, xr, ell, "matern52", "float64")[0]
    s = (xr[:, l][:, None] / ell[l] - xr[:, l][None, :] / ell[l]).abs()
    bad = list(sums)
    bad[l] = float((G * c0 * s * s / (1.0 + s)).sum())
    c = sb.check_outputs(_finalize(e["out"], bad, th, d), x, Y, None, th, e["V"], e["b"], e["z"], "matern52", dtype)
    assert c.ratio > 1 and c.where == ("g_ell%d" % l,), c


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_matern52_defect_3_dghat_with_the_matern32_h(dtype):
    """dghat formed with h = s / (1 + |s|); dgvar with the right one"""
    g = _pgrad_problem(dtype, kernel="matern52", rep=True)
    args = (g["x0"], g["x"], g["sr"], g["th"], g["z"], g["Vp"])
    assert sb.check_pgrad(g["gh"], g["gv"], *args, "matern52", dtype).ratio < 0.5
    gh, gv = _pgrad(*args, dtype, "matern52", h_kernel="matern32")
    assert np.array_equal(gv, g["gv"])
    c = sb.check_pgrad(gh, gv, *args, "matern52", dtype)
    assert c.ratio > 1 and c.where[1].startswith("dghat"), c


# ----------------------------------------------------------------------------------------------------------------------
# the conditioned view: an emulated lcgp_condition_prepare / lcgp_condition_predict with q = 3 components that differ in
# every parameter, in the storage type (numpy float32 / float64 arrays; the tile kernel's products in 64-stages on one
# accumulator, the reductions in double).  n = 300 (npad 384), m = 150 (mpad 256: 106 padding columns), n0 = 130 (n0pad
# 256).  Rows 0 .. 3 of x0 equal rows of xn; rows 64 .. 127 of x0 lie nine units outside the data, so the row block 1 of
# Sigma_0n is made of far tiles (entries ~1e-14 of the largest).
# ----------------------------------------------------------------------------------------------------------------------
COND_M, COND_N0 = 150, 130
COND_EQUAL = (0, 63, 64, 149)                 # x0 row i equals xn row COND_EQUAL[i]
COND_FAR = (1, 1)                             # a far tile of Sigma_0n: x0 rows 64 .. 127, xn rows 64 .. 127
COND_STAGES = ("cross_n", "u_n", "pred_n", "cond_s", "cond_winv", "cond_dense", "cond_v", "cross_0", "u_0", "cond_cross",
               "cond_t", "cond_out")


def _np_t(dtype):
    return np.float32 if dtype == "float32" else np.float64


def _mm(A, B, dtype):
    """A B^T as the tile kernel forms it: operands and accumulator in the storage type, K in 64-stages"""
    T = _np_t(dtype)
    A, B = np.asarray(A, T), np.asarray(B, T)
    acc = np.zeros((A.shape[0], B.shape[0]), T)
    for k in range(0, A.shape[1], TS):
        acc += A[:, k:k + TS] @ B[:, k:k + TS].T
    return acc


def _axpy(Cm, alpha, acc, dtype):
    """C + alpha acc in the storage type (the epilogue of OP_PRED_COV / OP_COND_CROSS), as float64"""
    T = _np_t(dtype)
    return np.asarray(np.asarray(Cm, T) + T(alpha) * np.asarray(acc, T), np.float64)


def _cond_problem(dtype, kernel="matern32", rep=False):
    import scipy.linalg  # noqa: F401  (the triangular solves of the emulation)
    rng = np.random.default_rng(50)
    x = rng.uniform(0.0, 1.0, (N, D_IN))
    Y = rng.standard_normal((P, N))
    sr = np.sqrt(rng.integers(1, 6, N).astype(np.float64)) if rep else None
    xn = rng.uniform(0.0, 1.0, (COND_M, D_IN))
    r = (1.0 + np.arange(COND_M) % 3) if rep else None
    x0 = rng.uniform(-0.1, 1.1, (COND_N0, D_IN))
    x0[:len(COND_EQUAL)] = xn[list(COND_EQUAL)]
    x0[64:128] += 9.0
    t = rng.standard_normal((len(JOINT_TH), COND_M))
    ths, fits = [], []
    for k, (ell, scale, nug, Dk) in enumerate(JOINT_TH):
        th = np.concatenate([ell, [scale, nug, Dk], np.random.default_rng(60 + k).standard_normal(P)])
        ths.append(th)
        fits.append(_fit(x, Y, sr, th, dtype, kernel))
    return dict(x=x, sr=sr, xn=xn, r=r, x0=x0, t=t, th=ths, fit=fits, dtype=dtype, kernel=kernel)


def _cond_prepare(p, k, tau_D=None, use_r=True, upper=None):
    """the preparation of component k.  Defects: tau_D (the D that tau is formed with), use_r = False (tau = 1 / D), upper (a
    value left above the diagonal of the dense L_S^-1)"""
    import scipy.linalg as sla
    dtype, kernel, th, f = p["dtype"], p["kernel"], p["th"][k], p["fit"][k]
    T = _np_t(dtype)
    ell, scale, nug, Dk, _ = sb.split_theta(th, D_IN)
    nt = nug / (1 + nug)
    m, mpad = COND_M, sb._pad128(COND_M)
    Xn = _r(_cross(p["xn"], p["x"], p["sr"], th, dtype, kernel), dtype)
    Un = np.asarray(_mm(Xn, f["W"], dtype), np.float64)
    ghat_n = Xn @ f["z"]
    gvar_n = scale - Dk * np.sum(Un * Un, axis=1)
    xr = _r(p["xn"], dtype)
    cnn = scale * ((1 - nt) * sb.kernel_parts(xr, xr, ell, kernel, dtype)[0].numpy() + nt * np.eye(m))
    S = _axpy(_r(cnn, dtype), -Dk, _mm(Un, Un, dtype), dtype)
    rr = p["r"] if (use_r and p["r"] is not None) else np.ones(m)
    tau = 1.0 / ((Dk if tau_D is None else tau_D) * rr)
    S[np.arange(m), np.arange(m)] = _r(np.diag(S) + tau, dtype)
    L = np.linalg.cholesky(np.asarray(S, T))
    Wn = np.tril(sla.solve_triangular(L, np.eye(m, dtype=T), lower=True))
    assert L.dtype == T and Wn.dtype == T
    L, Wn = np.asarray(L, np.float64), np.asarray(Wn, np.float64)
    Wd = np.eye(mpad)
    Wd[:m, :m] = Wn
    if upper is not None:
        Wd[np.triu_indices(mpad, 1)] = upper
    v = np.zeros(mpad)
    v[:m] = np.tril(Wd[:m, :m]) @ (p["t"][k] - ghat_n)         # (cond_v_kernel sums j <= i only)
    return dict(Xn=Xn, Un=Un, ghat_n=ghat_n, gvar_n=gvar_n, L=L, Wn=Wn, Wd=Wd, v=v)


def _cond_sigma(p, k, e, drop=None, nugget=False, as32=False):
    """Sigma_0n of component k, padded to n0pad x mpad with zeros, and what it is made from.  Defects: drop = (tile, stage): that
    64-tile misses that 64-wide K-stage of U_0 U_n^T; nugget: scale nt added where a row of x0 equals a row of xn; as32: the
    result carries float32 accuracy"""
    dtype, kernel, th, f = p["dtype"], p["kernel"], p["th"][k], p["fit"][k]
    ell, scale, nug, Dk, _ = sb.split_theta(th, D_IN)
    nt = nug / (1 + nug)
    n0, m = COND_N0, COND_M
    X0 = _r(_cross(p["x0"], p["x"], p["sr"], th, dtype, kernel), dtype)
    U0 = np.asarray(_mm(X0, f["W"], dtype), np.float64)
    g0 = X0 @ f["z"]
    v0 = scale - Dk * np.sum(U0 * U0, axis=1)
    cx = scale * (1 - nt) * sb.kernel_parts(_r(p["x0"], dtype), _r(p["xn"], dtype), ell, kernel, dtype)[0].numpy()
    if nugget:
        cx = cx.copy()
        cx[np.arange(len(COND_EQUAL)), list(COND_EQUAL)] += scale * nt
    acc = np.asarray(_mm(U0, e["Un"], dtype), np.float64)
    if drop is not None:
        (i, j), s = drop
        rows, cols = _tile(i, j)
        ks = slice(s * TS, (s + 1) * TS)
        acc[rows, cols] = _r(acc[rows, cols] - U0[rows, ks] @ e["Un"][cols, ks].T, dtype)[:n0 - rows.start]
    Sg = np.zeros((sb.predict_pad(n0), sb._pad128(m)))
    Sg[:n0, :m] = _axpy(_r(cx, dtype), -Dk, acc, dtype)
    if as32:
        Sg = _r(Sg, "float32")
    return dict(X0=X0, U0=U0, g0=g0, v0=v0, Sg=Sg)


def _cond_output(p, e, s, v=None, pad_column=False):
    """T and the corrected outputs from the dense L_S^-1 (read whole, as the tile kernel does), v and Sigma_0n.  Defects: v (the v
    of another component); pad_column: column m of T holds what column 0 does and the row sums run to mpad"""
    n0, m = COND_N0, COND_M
    Tm = np.asarray(_mm(s["Sg"], e["Wd"], p["dtype"]), np.float64)
    vv = e["v"] if v is None else v
    hi = m
    if pad_column:
        Tm[:, m] = Tm[:, 0]
        hi = Tm.shape[1]
    gh = s["g0"] + Tm[:n0, :hi] @ vv[:hi]
    gv = s["v0"] - np.sum(Tm[:n0, :hi] ** 2, axis=1)
    return dict(Tm=Tm, gh=gh, gv=gv)


def _cond_checks(p, k, e, s, o):
    dtype, kernel, th, f = p["dtype"], p["kernel"], p["th"][k], p["fit"][k]
    x, sr, xn, x0, n0, m = p["x"], p["sr"], p["xn"], p["x0"], COND_N0, COND_M
    return dict(
        cross_n=sb.check_cov_cross(e["Xn"], xn, x, sr, th, kernel, dtype),
        u_n=sb.check_cov_u(e["Un"], e["Xn"], f["W"], dtype),
        pred_n=sb.check_predict(e["ghat_n"], e["gvar_n"], xn, x, sr, th, f["W"], f["z"], kernel, dtype),
        cond_s=sb.check_cond_s(e["L"], e["Un"], xn, p["r"], th, kernel, dtype),
        cond_winv=sb.check_inverse_factor(e["L"], e["Wn"], dtype),
        cond_dense=sb.check_cond_dense_inverse(e["Wd"], e["Wn"], m),
        cond_v=sb.check_cond_v(e["v"], e["Wd"], p["t"][k], e["ghat_n"], m),
        cross_0=sb.check_cov_cross(s["X0"], x0, x, sr, th, kernel, dtype),
        u_0=sb.check_cov_u(s["U0"], s["X0"], f["W"], dtype),
        cond_cross=sb.check_cond_cross(s["Sg"][:n0, :m], s["U0"], e["Un"], x0, xn, th, kernel, dtype),
        cond_t=sb.check_cov_u(o["Tm"][:n0, :m], s["Sg"][:n0, :m], e["Wd"][:m, :m], dtype),
        cond_out=sb.check_cond_out(o["gh"], o["gv"], o["Tm"][:n0], e["v"], s["g0"], s["v0"], m))


def _cond_run(p, k, prepare=None, sigma=None, output=None):
    e = _cond_prepare(p, k, **(prepare or {}))
    s = _cond_sigma(p, k, e, **(sigma or {}))
    o = _cond_output(p, e, s, **(output or {}))
    return e, s, o, _cond_checks(p, k, e, s, o)


def _only(checks, *failing):
    """every stage listed in `failing` is above 1, every stage upstream of the first of them at or below 1"""
    assert tuple(checks) == COND_STAGES
    first = min(COND_STAGES.index(f) for f in failing)
    for stage in COND_STAGES[:first]:
        assert checks[stage].ratio <= 1.0, ("upstream", stage, checks[stage])
    for stage in failing:
        assert checks[stage].ratio > 1.0, (stage, checks[stage])


@pytest.fixture(scope="module", params=["float64", "float32"])
def cond(request):
    return _cond_problem(request.param)


@pytest.fixture(scope="module")
def cond64():
    return _cond_problem("float64")


@pytest.mark.parametrize("rep", [False, True], ids=["full", "rep"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_emulated_conditioned_view_passes_every_stage(dtype, kernel, rep):
    p = _cond_problem(dtype, kernel, rep)
    for k in range(len(JOINT_TH)):
        e, s, o, checks = _cond_run(p, k)
        print("conditioned view, emulated, %s %s %s k%d: %s"
              % (dtype, kernel, "rep" if rep else "full", k, "  ".join("%s %.2e" % (st, c.ratio) for st, c in checks.items())))
        for stage, c in checks.items():
            assert c.ratio <= 1.0, (k, stage, c)
        # the far tile is far: below 1e-8 of the largest entry, and not all zero in float64
        far = np.abs(s["Sg"][_tile(*COND_FAR)])
        assert far.max() < 1e-8 * np.abs(s["Sg"]).max()
        assert dtype == "float32" or kernel == "se" or far.min() > 0


def test_cond_defect_1_tau_of_the_next_component_or_without_r():
    """tau = 1 / (D_{k+1} r) and, on the rep path, tau = 1 / D_k: S, so its factor and everything behind it, belong to another
    problem; cond_s fails and nothing before it"""
    for dtype in ("float64", "float32"):
        p = _cond_problem(dtype, rep=True)
        for k in range(len(JOINT_TH)):
            other = p["th"][(k + 1) % len(JOINT_TH)][D_IN + 2]
            _only(_cond_run(p, k, prepare=dict(tau_D=other))[3], "cond_s")
            _only(_cond_run(p, k, prepare=dict(use_r=False))[3], "cond_s")


def test_cond_defect_2_k_stage_left_out_of_a_far_tile(cond):
    """the far tile (1, 1) of Sigma_0n misses the 64-wide K-stage 2 of U_0 U_n^T"""
    for k in range(len(JOINT_TH)):
        checks = _cond_run(cond, k, sigma=dict(drop=(COND_FAR, 2)))[3]
        _only(checks, "cond_cross")
        assert checks["cond_cross"].where == COND_FAR, checks["cond_cross"]


def test_cond_defect_3_nugget_where_a_row_of_x0_equals_a_row_of_xn(cond):
    for k in range(len(JOINT_TH)):
        checks = _cond_run(cond, k, sigma=dict(nugget=True))[3]
        _only(checks, "cond_cross")
        assert checks["cond_cross"].where[0] == 0, checks["cond_cross"]


def test_cond_defect_4_upper_triangle_of_the_dense_inverse_not_zeroed(cond):
    """the strict upper triangle of the state's L_S^-1 holds 0.25: the bitwise check sees it, and T, which the tile kernel forms
    from whole tiles of it, fails cond_t; the stages between (v sums j <= i only) and Sigma_0n do not"""
    for k in range(len(JOINT_TH)):
        checks = _cond_run(cond, k, prepare=dict(upper=0.25))[3]
        _only(checks, "cond_dense", "cond_t")
        for stage in ("cond_winv", "cond_v", "cross_0", "u_0", "cond_cross"):
            assert checks[stage].ratio <= 1.0, (stage, checks[stage])


def test_cond_defect_5_v_of_the_next_component(cond):
    for k in range(len(JOINT_TH)):
        v = _cond_prepare(cond, (k + 1) % len(JOINT_TH))["v"]
        _only(_cond_run(cond, k, output=dict(v=v))[3], "cond_out")


def test_cond_defect_6_row_sums_over_a_nonzero_padding_column_of_t(cond):
    for k in range(len(JOINT_TH)):
        _only(_cond_run(cond, k, output=dict(pad_column=True))[3], "cond_out")


def test_cond_defect_7_float32_sigma0n_in_the_float64_check(cond64):
    for k in range(len(JOINT_TH)):
        _only(_cond_run(cond64, k, sigma=dict(as32=True))[3], "cond_cross")


def test_cond_gap_far_tile_off_by_1e_6_is_invisible_end_to_end(cond64):
    """what the stage bound closes: the far tile (1, 1) of Sigma_0n off by 1e-6 relative.  In the units of tests/test_gpu_condition.py
    -- the largest gvar of the base model and the largest |ghat| over the 130 points -- the outputs move by far less than its
    1e-10; cond_cross is above 1 at that tile"""
    p = cond64
    for k in range(len(JOINT_TH)):
        e, s, o, checks = _cond_run(p, k)
        assert checks["cond_cross"].ratio <= 1.0
        bad = dict(s, Sg=s["Sg"].copy())
        tile = _tile(*COND_FAR)
        assert np.abs(bad["Sg"][tile]).max() < 1e-8 * np.abs(s["Sg"]).max()
        bad["Sg"][tile] *= 1 + 1e-6
        ob = _cond_output(p, e, bad)
        eh = np.max(np.abs(ob["gh"] - o["gh"])) / np.max(np.abs(o["gh"]))
        ev = np.max(np.abs(ob["gv"] - o["gv"])) / np.max(s["v0"])
        print("gap k%d: end-to-end change ghat %.3e gvar %.3e (bar 1e-10)" % (k, eh, ev))
        assert eh < 1e-10 and ev < 1e-10
        c = _cond_checks(p, k, e, bad, ob)["cond_cross"]
        assert c.ratio > 1 and c.where == COND_FAR, c


# ----------------------------------------------------------------------------------------------------------------------
# second-order input queries (lcgp_predict_hess, lcgp_predict_gradcov): DX, P = DX W^T, the packed Hessians, Gamma and its
# weighted sum M, emulated in the kernels' blocked order -- PH_B x PH_B block pairs (lb >= mb) with psi where lb == mb and
# a == b, the DMAX chunks of pdx_kernel, four waves per workgroup and the workgroups ascending for M.  DX and P are stored in
# the storage type (the product through _mm), everything else is float64, as in the library.  n = 303: odd (VN = 2 leaves a
# tail of one column in float64) and 3 mod 4 (VN = 4 leaves three in float32).
# ----------------------------------------------------------------------------------------------------------------------
SO_N, SO_N0 = 303, 21                         # 21 = 5 workgroups of four waves + one: three dead waves in the last
PH_B, DMAX = 4, 32
SO_STAGES = ("pdx", "p", "phess", "gradcov", "gradcov_sum")
_SO_CACHE = {}


def _psi(sl, kernel, rcp=None):
    """psi of the input Hessian, every kernel spelled out (numpy; rcp as in _h)"""
    rcp = (lambda v: 1.0 / v) if rcp is None else rcp
    a = np.abs(sl)
    if kernel == "se":
        return sl * sl - 1.0
    if kernel == "matern32":
        return (a - 1.0) * rcp(1.0 + a)
    if kernel == "matern52":
        return (a * (a - 1.0) - 1.0) * rcp(a * (a + 3.0) + 3.0)
    raise ValueError(kernel)


def _so_problem(dtype, d=6, kernel="matern32", rep=False, n0=SO_N0, seed=11, far=False):
    key = (dtype, d, kernel, rep, n0, seed, far)
    if key in _SO_CACHE:
        return _SO_CACHE[key]
    rng = np.random.default_rng(seed + d)
    n = SO_N
    x = rng.uniform(0.0, 1.0, (n, d))
    Y = rng.standard_normal((P, n))
    sr = np.sqrt(rng.integers(1, 6, n).astype(np.float64)) if rep else None
    th = _theta(d, seed + 1)
    e = _fit(x, Y, sr, th, dtype, kernel)
    x0 = np.concatenate([x[:3], rng.uniform(-0.1, 1.1, (n0 - 3, d))])      # training inputs among x0: s = 0
    if far:
        x0[-1] = 12.0                                                         # one new input far outside the data
    U = _r(_r(_cross(x0, x, sr, th, dtype, kernel), dtype) @ e["W"].T, dtype)
    Vp = _r(U @ e["W"], dtype)
    w = rng.uniform(0.0, 1.0, n0)
    w[::4] = 0.0
    w[1] = -0.3
    Mb = rng.standard_normal(d * (d + 1) // 2)
    p = dict(x=x, sr=sr, th=th, x0=x0, Vp=Vp, w=w, Mb=Mb, dtype=dtype, kernel=kernel, d=d, n=n, n0=n0, **e)
    _SO_CACHE[key] = p
    return p


def _so_s(p, l, ell_of=None):
    ell = sb.split_theta(p["th"], p["d"])[0]
    le = ell[l if ell_of is None else ell_of]
    a, b = _r(p["x0"], p["dtype"]), _r(p["x"], p["dtype"])
    return a[:, l][:, None] / le - b[:, l][None, :] / le


def _so_pdx(p, rcp=None, stale_chunk=False):
    """DX (n0 d x n), rounded once to the storage type.  Defects: rcp (the reciprocal in h), stale_chunk (the chunks of DMAX
    dimensions after the first are staged with the lengthscales of the chunk before them)"""
    d, n0, n, dtype, kernel = p["d"], p["n0"], p["n"], p["dtype"], p["kernel"]
    X = _cross(p["x0"], p["x"], p["sr"], p["th"], dtype, kernel)
    DX = np.zeros((n0, d, n))
    for d0 in range(0, d, DMAX):
        for l in range(d0, min(d0 + DMAX, d)):
            s = _so_s(p, l, l - DMAX if (stale_chunk and d0 > 0) else None)
            DX[:, l, :] = X * _h(s, kernel, rcp)
    return _r(DX.reshape(n0 * d, n), dtype)


def _so_p(p, DX, as32=False):
    """P = DX W^T on the tile kernel (storage type); defect as32: stored with float32 accuracy"""
    Pm = np.asarray(_mm(DX, p["W"], p["dtype"]), np.float64)
    return _r(Pm, "float32") if as32 else Pm


def _so_pairs(d):
    nblk = -(-d // PH_B)
    return [(lb, mb) for lb in range(nblk) for mb in range(lb + 1)]


def _so_gram(p, P, i_l, i_m, drop_tail):
    """P_il . P_im for row-index arrays; drop_tail: the n % VN columns behind the 16-byte loads left out"""
    n = p["n"]
    vn = 4 if p["dtype"] == "float32" else 2
    cols = n - n % vn if drop_tail else n
    return np.einsum("ij,ij->i", P[i_l, :cols], P[i_m, :cols])


def _so_phess(p, P, diag_ignored=False, past_d=False, transposed=False, drop_tail=False, psi_kernel=None, rcp=None):
    """d2ghat, d2gvar (n0 x tri) block pair by block pair.  Defects: diag_ignored (psi on a == b of every block pair),
    past_d (the guard l < d missing: the dimensions beyond d, which re-read row d - 1, are written at l (l + 1) / 2 + m, which
    lies in the next input's row), transposed (the packed index m (m + 1) / 2 + l), drop_tail, psi_kernel (psi of another
    kernel), rcp (the reciprocal in h and psi)"""
    d, n0, dtype, kernel, th = p["d"], p["n0"], p["dtype"], p["kernel"], p["th"]
    ell, scale, nug, Dk, _ = sb.split_theta(th, d)
    s = np.ones(p["n"]) if p["sr"] is None else _r(p["sr"], dtype)
    c0 = _cross(p["x0"], p["x"], None, th, dtype, kernel)
    pz, pv = c0 * (s * p["z"])[None, :], c0 * s[None, :] * p["Vp"]
    S = [_so_s(p, l) for l in range(d)]
    Hh = [_h(S[l], kernel, rcp) for l in range(d)]
    Ps = [_psi(S[l], psi_kernel or kernel, rcp) for l in range(d)]
    tri = d * (d + 1) // 2
    gh, gv = np.full((n0, tri), np.nan), np.full((n0, tri), np.nan)
    rows = np.arange(n0) * d

    def entry(l, m, use_psi):
        kap = Ps[l] if use_psi else Hh[l] * Hh[m]
        inv = 1.0 / (ell[l] * ell[m])
        G = _so_gram(p, P, rows + l, rows + m, drop_tail)
        return (pz * kap).sum(axis=1) * inv, -2.0 * Dk * ((pv * kap).sum(axis=1) + G) * inv

    for lb, mb in _so_pairs(d):
        for a in range(PH_B):
            for b in range(PH_B):
                l, m = lb * PH_B + a, mb * PH_B + b
                use_psi = a == b and (lb == mb or diag_ignored)
                if l < d and m <= l:
                    o = m * (m + 1) // 2 + l if transposed else l * (l + 1) // 2 + m
                    gh[:, o], gv[:, o] = entry(l, m, use_psi)
                elif past_d and l >= d and m <= l:
                    o = l * (l + 1) // 2 + m - tri
                    if o < tri:
                        vh, vv = entry(d - 1, min(m, d - 1), use_psi and m >= d - 1)
                        gh[1:, o], gv[1:, o] = vh[:-1], vv[:-1]
    return gh, gv


def _so_gradcov(p, P, kappa=None, Dk=None, drop_tail=False):
    """Gamma (n0 x tri); defects: kappa, Dk (the D of another component), drop_tail"""
    d, n0, th = p["d"], p["n0"], p["th"]
    ell, scale, nug, D, _ = sb.split_theta(th, d)
    D = D if Dk is None else Dk
    prior = scale * (1.0 - nug / (1.0 + nug)) * (sb.GRADCOV_KAPPA[p["kernel"]] if kappa is None else kappa)
    g = np.zeros((n0, d * (d + 1) // 2))
    rows = np.arange(n0) * d
    for lb, mb in _so_pairs(d):
        for a in range(PH_B):
            for b in range(PH_B):
                l, m = lb * PH_B + a, mb * PH_B + b
                if l < d and m <= l:
                    G = _so_gram(p, P, rows + l, rows + m, drop_tail)
                    g[:, l * (l + 1) // 2 + m] = ((prior if l == m else 0.0) - D * G) / (ell[l] * ell[m])
    return g


def _so_sum(p, gamma, overwrite=False, dead_weight=False):
    """M after the weighted call: four waves per workgroup, the workgroups ascending, then M += sum.  Defects: overwrite,
    dead_weight (a wave beyond n0 in the last workgroup adds the last input once more, with weight 1)"""
    n0, w = p["n0"], p["w"]
    s = np.zeros(gamma.shape[1])
    for g0 in range(0, n0, 4):
        red = []
        for i in range(g0, g0 + 4):
            if i < n0:
                red.append(w[i] * gamma[i])
            else:
                red.append(1.0 * gamma[n0 - 1] if dead_weight else 0.0 * gamma[0])
        s = s + (((red[0] + red[1]) + red[2]) + red[3])
    return s if overwrite else p["Mb"] + s


def _so_run(p, pdx=None, pp=None, phess=None, gradcov=None, gsum=None):
    dtype, kernel = p["dtype"], p["kernel"]
    a = (p["x0"], p["x"], p["sr"], p["th"])
    DX = _so_pdx(p, **(pdx or {}))
    Pm = _so_p(p, DX, **(pp or {}))
    gh, gv = _so_phess(p, Pm, **(phess or {}))
    gamma = _so_gradcov(p, Pm, **(gradcov or {}))
    dghat = _pgrad(p["x0"], p["x"], p["sr"], p["th"], p["z"], p["Vp"], dtype, kernel)[0]
    Ma = _so_sum(p, gamma, **(gsum or {}))
    checks = dict(pdx=sb.check_pdx(DX, *a, kernel, dtype),
                  p=sb.check_cov_u(Pm, DX, p["W"], dtype),
                  phess=sb.check_phess(gh, gv, *a, p["z"], p["Vp"], Pm, kernel, dtype),
                  gradcov=sb.check_gradcov(gamma, dghat, *a, p["z"], Pm, kernel, dtype),
                  gradcov_sum=sb.check_gradcov_sum(Ma, p["Mb"], gamma, p["w"]))
    return dict(DX=DX, P=Pm, gh=gh, gv=gv, gamma=gamma, dghat=dghat, Ma=Ma), checks


def _so_only(checks, *failing):
    """the stages listed in `failing` are above 1 and EVERY other stage is at or below 1"""
    assert tuple(checks) == SO_STAGES
    for stage in SO_STAGES:
        if stage in failing:
            assert checks[stage].ratio > 1.0, (stage, checks[stage])
        else:
            assert checks[stage].ratio <= 1.0, ("not named", stage, checks[stage])


@pytest.mark.parametrize("d", [6, 33])
@pytest.mark.parametrize("rep", [False, True], ids=["full", "rep"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_emulated_second_order_paths_pass_every_stage(dtype, kernel, rep, d):
    p = _so_problem(dtype, d=d, kernel=kernel, rep=rep, n0=SO_N0 if d == 6 else 10)
    r, checks = _so_run(p)
    print("second order, emulated, %s %s %s d=%d: %s"
          % (dtype, kernel, "rep" if rep else "full", d, "  ".join("%s %.2e" % (st, c.ratio) for st, c in checks.items())))
    for stage, c in checks.items():
        assert c.ratio <= 1.0, (stage, c)
    for i in range(3):                                       # x0 row i IS x row i: s = 0 and DX = 0 exactly at column i
        assert np.all(r["DX"][i * d:(i + 1) * d, i] == 0.0)


@pytest.mark.parametrize("kernel", KERNELS)
def test_psi_and_h_against_autograd_of_the_1d_factor(kernel):
    """pgrad_psi = f'' / f and pgrad_h = -f' / f of the 1-D factor f(s) = g(|s|), against torch autograd of g in a = |s| (g is
    smooth on a >= 0; f'' (s) = g''(|s|) away from 0 and psi(0) is its one-sided limit: -1 for Matern-3/2, where f has a kink
    in its second derivative), and the |psi'| of pgrad_psi_err against autograd of psi: float64, 1e-12"""
    g = {"matern32": lambda a: (1.0 + a) * torch.exp(-a), "se": lambda a: torch.exp(-0.5 * a * a),
         "matern52": lambda a: (1.0 + a + a * a / 3.0) * torch.exp(-a)}[kernel]
    s = torch.as_tensor(np.concatenate([[0.0, 1e-300, -1e-300, 1.0, -1.0, 1.618033988749895],
                                        np.random.default_rng(5).uniform(-9.0, 9.0, 200)]))
    a = s.abs().clone().requires_grad_(True)
    f = g(a)
    f1, = torch.autograd.grad(f.sum(), a, create_graph=True)
    f2, = torch.autograd.grad(f1.sum(), a)
    psi, h = sb.pgrad_psi(s, kernel), sb.pgrad_h(s, kernel)
    assert float((psi - (f2 / f).detach()).abs().max()) <= 1e-12
    assert float((h + torch.sign(s) * (f1 / f).detach()).abs().max()) <= 1e-12
    assert float(psi[0]) == {"matern32": -1.0, "se": -1.0, "matern52": -1.0 / 3.0}[kernel]
    assert float((psi[1:3] - psi[0]).abs().max()) <= 1e-15    # continuous at 0 from both sides
    sv = s.clone().requires_grad_(True)
    dpsi, = torch.autograd.grad(sb.pgrad_psi(sv, kernel).sum(), sv)
    got, k, ab = sb.pgrad_psi_err(s, kernel)
    nz = s != 0
    assert float((got - dpsi.abs())[nz].abs().max()) <= 1e-12
    assert 1.0 <= k <= 6.0 and float(ab.min()) >= 0.0


def test_unknown_kernel_name_is_an_error_in_the_second_order_checks():
    p = _so_problem("float64")
    r, _ = _so_run(p)
    a = (p["x0"], p["x"], p["sr"], p["th"])
    with pytest.raises(ValueError):
        sb.pgrad_psi(torch.zeros(1, dtype=torch.float64), "matern")
    with pytest.raises(ValueError):
        sb.check_pdx(r["DX"], *a, "matern", "float64")
    with pytest.raises(ValueError):
        sb.check_phess(r["gh"], r["gv"], *a, p["z"], p["Vp"], r["P"], "matern", "float64")
    with pytest.raises(ValueError):
        sb.check_gradcov(r["gamma"], r["dghat"], *a, p["z"], r["P"], "matern", "float64")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_second_order_defect_1_psi_on_an_off_diagonal_block_pair(dtype):
    """the diag flag ignored: block pair (1, 0) at d = 6 puts psi(s_4), psi(s_5) at (4, 0) and (5, 1)"""
    checks = _so_run(_so_problem(dtype), phess=dict(diag_ignored=True))[1]
    _so_only(checks, "phess")
    assert checks["phess"].where[1].split(" ", 1)[1] in ("l4 m0", "l5 m1"), checks["phess"]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_second_order_defect_2_block_past_d_written_into_a_valid_slot(dtype):
    """d = 6: block 1 reaches dimensions 6 and 7, which re-read row 5; without l < d they land in the next input's row"""
    _so_only(_so_run(_so_problem(dtype), phess=dict(past_d=True))[1], "phess")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_second_order_defect_3_transposed_packed_index(dtype):
    _so_only(_so_run(_so_problem(dtype), phess=dict(transposed=True))[1], "phess")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_second_order_defect_4_vector_load_tail_left_out_of_the_gram_term(dtype):
    """n = 303: the last column (float64, VN = 2) or the last three (float32, VN = 4) missing from P_il . P_im"""
    assert SO_N % 2 == 1 and SO_N % 4 == 3
    p = _so_problem(dtype)
    checks = _so_run(p, phess=dict(drop_tail=True), gradcov=dict(drop_tail=True))[1]
    _so_only(checks, "phess", "gradcov")
    assert checks["phess"].where[1].startswith("d2gvar") and checks["gradcov"].where[1].startswith("gamma")
    _so_only(_so_run(p, phess=dict(drop_tail=True))[1], "phess")
    _so_only(_so_run(p, gradcov=dict(drop_tail=True))[1], "gradcov")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_second_order_defect_5_second_pdx_chunk_with_the_lengthscales_of_the_first(dtype):
    checks = _so_run(_so_problem(dtype, d=33, n0=10), pdx=dict(stale_chunk=True))[1]
    _so_only(checks, "pdx")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_second_order_defect_6_matern52_with_the_matern32_psi_or_kappa(dtype):
    p = _so_problem(dtype, kernel="matern52")
    checks = _so_run(p, phess=dict(psi_kernel="matern32"))[1]
    _so_only(checks, "phess")
    l, m = (int(v[1:]) for v in checks["phess"].where[1].split(" ")[1:])
    assert l == m, checks["phess"]
    checks = _so_run(p, gradcov=dict(kappa=1.0))[1]
    _so_only(checks, "gradcov")
    assert checks["gradcov"].where[1].startswith("gamma"), checks["gradcov"]


def test_second_order_defect_7_float32_reciprocal_in_h_and_psi():
    """fast_rcp without its Newton steps, in the float64 path: in pdx_kernel (DX, and nothing behind it: P, G and Gamma are
    checked from the library's own DX and P), and in phess_kernel"""
    rcp32 = lambda v: np.float32(1.0) / v.astype(np.float32)      # noqa: E731
    p = _so_problem("float64")
    _so_only(_so_run(p, pdx=dict(rcp=rcp32))[1], "pdx")
    _so_only(_so_run(p, phess=dict(rcp=rcp32))[1], "phess")
    p = _so_problem("float64", kernel="matern52")
    _so_only(_so_run(p, pdx=dict(rcp=rcp32))[1], "pdx")
    _so_only(_so_run(p, phess=dict(rcp=rcp32))[1], "phess")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_second_order_defect_8_gamma_with_the_d_of_the_next_component(dtype):
    p = _so_problem(dtype)
    other = sb.split_theta(p["th"], p["d"])[3] * 1.7
    _so_only(_so_run(p, gradcov=dict(Dk=other))[1], "gradcov")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_second_order_defect_9_m_overwritten_or_a_dead_wave_weighted(dtype):
    p = _so_problem(dtype)
    assert p["n0"] % 4 != 0 and np.any(p["Mb"] != 0)
    _so_only(_so_run(p, gsum=dict(overwrite=True))[1], "gradcov_sum")
    _so_only(_so_run(p, gsum=dict(dead_weight=True))[1], "gradcov_sum")


def test_second_order_defect_10_float32_p_in_the_float64_check():
    _so_only(_so_run(_so_problem("float64"), pp=dict(as32=True))[1], "p")


def test_second_order_gap_small_hessian_entry_is_invisible_normwise():
    """what the entry-by-entry bound closes: tests/test_gpu_predict_hess.py measures max|err| / max|ref| over the whole output
    against LATENT_BAR = 1e-10.  An off-diagonal entry (l = 3, m = 1) of the Hessians of a new input far from the data, off by
    1e-3 RELATIVE, stays far below that bar; check_phess is above 1 at that entry"""
    LATENT_BAR = 1e-10
    p = _so_problem("float64", far=True)
    r, checks = _so_run(p)
    for c in checks.values():
        assert c.ratio <= 1.0, checks
    i, o = p["n0"] - 1, 3 * 4 // 2 + 1
    a = (p["x0"], p["x"], p["sr"], p["th"])
    for name in ("gh", "gv"):
        bad = dict(r, **{name: r[name].copy()})
        assert abs(bad[name][i, o]) < 1e-8 * np.abs(r[name]).max() and bad[name][i, o] != 0
        bad[name][i, o] *= 1 + 1e-3
        nw = _normwise(bad[name], r[name])
        print("gap %s: normwise %.3e (bar %.0e)" % (name, nw, LATENT_BAR))
        assert nw < 1e-3 * LATENT_BAR
        c = sb.check_phess(bad["gh"], bad["gv"], *a, p["z"], p["Vp"], r["P"], "matern32", "float64")
        assert c.ratio > 1 and c.where == (i // TS, "%s l3 m1" % ("d2ghat" if name == "gh" else "d2gvar")), c


# ----------------------------------------------------------------------------------------------------------------------
# box-averaged predictions (lcgp_predict_marginal, lcgp_condition_predict_marginal): the table of 1-D averages (the restatement
# tests/marginal_ref.py in float64: the same series, switches and closed forms as marg_table_kernel), the masked rows, U, the
# outputs with the averaged prior, the view's stages (the table over xn, the masked rows against xn, Sigma_0n, T, the corrected
# outputs) and gcov, emulated with q = 2 components whose lengthscales run from 0.02 to 30 within a row.  n = 130 (npad 256:
# 126 padding columns of the table), n0 = 70, m = 70; d = 3 and d = 34 (two 32-dimension chunks of the masked cross_kernel).
# The inputs are float32-representable so that both precisions share the mpmath values (stage_bounds caches them per value).
# ----------------------------------------------------------------------------------------------------------------------
from tests import marginal_ref as mref  # noqa: E402

MG_N, MG_N0, MG_M, MG_Q = 130, 70, 70, 2
MG_BOXES = {"default": (0.0, 1.0), "sub": (0.3, 0.75)}
MG_STAGES = ("table", "cross", "u", "out", "table_n", "cross_n", "cond_cross", "cond_t", "cond_out", "gcov")
MG_REF_ROWS = (0, 3, 4)                       # rows of _mg_rows with an empty, a full and a random mask: the reference rows of gcov
_MG_CACHE = {}


def _mg_rows(d, n0, seed, shift=0):
    """x0 (NaN under the mask) and masks of the kinds tests/test_gpu_marginal.py::_rows makes: empty, one dimension, all but one,
    all, random (never empty); with d > 32 the single / kept dimension walks over 30 .. 33 and the random masks straddle 31 / 32.
    Row i is of kind (i + shift) % 5"""
    rng = np.random.default_rng(seed)
    x0 = np.asarray(rng.uniform(-0.1, 1.1, (n0, d)), np.float32).astype(np.float64)
    mask = np.zeros((n0, d), bool)
    edge = [l for l in (0, 30, 31, 32, 33, d - 1) if l < d]
    for i in range(n0):
        l = edge[(i // 5) % len(edge)]
        kind = (i + shift) % 5
        if kind == 1:
            mask[i, l] = True
        elif kind == 2:
            mask[i] = True
            mask[i, l] = False
        elif kind == 3:
            mask[i] = True
        elif kind == 4:
            mask[i] = rng.uniform(0, 1, d) < 0.5
            if d > 32:
                mask[i, 31], mask[i, 32] = True, False
            if not mask[i].any() or (mask[i].all() and d > 1):
                mask[i, d - 1], mask[i, 0] = False, True
    x0[mask] = np.nan
    return x0, mask


def _mg_theta(d, kernel, k):
    """theta row of component k: lengthscales from 0.02 (0.1 for SE at d > 3, whose C0 would otherwise be past its cut-off for
    nearly every pair) to 30 within the row, 0.7 in between so that b straddles 1/2 and 1 at the box edges; the components
    share the other lengthscales at d > 3 (the mpmath cache is keyed on them)"""
    rng = np.random.default_rng(900 + d)
    ell = np.sqrt(d) * rng.uniform(0.3, 0.9, d)
    small = 0.02 if (kernel != "se" or d <= 3) else 0.1
    if d <= 3:
        ell = np.array([[small, 0.7, 30.0], [30.0, 0.3, small]][k][:d])
    else:
        ell[0], ell[1], ell[d // 2], ell[d - 1] = (small, 30.0, 0.7, 2.0) if k == 0 else (30.0, small, 0.7, 2.0)
    rk = np.random.default_rng(910 + k)
    return np.concatenate([ell, [(1.3, 0.7)[k], (0.01, 0.002)[k], (5.0, 12.0)[k]], rk.standard_normal(P)])


def _mg_problem(dtype, kernel="matern32", rep=False, d=3, box="default", sort0=False):
    key = (dtype, kernel, rep, d, box, sort0)
    if key in _MG_CACHE:
        return _MG_CACHE[key]
    rng = np.random.default_rng(70 + d)
    x = np.asarray(rng.uniform(0.0, 1.0, (MG_N, d)), np.float32).astype(np.float64)
    if sort0:
        x = x[np.argsort(x[:, 0])]
    Y = rng.standard_normal((P, MG_N))
    sr = np.sqrt(rng.integers(1, 6, MG_N).astype(np.float64)) if rep else None
    xn = np.asarray(rng.uniform(-0.2, 1.2, (MG_M, d)), np.float32).astype(np.float64)       # inside and outside the box
    r = (1.0 + np.arange(MG_M) % 3) if rep else None
    x0, mask = _mg_rows(d, MG_N0, 71 + d)
    for i, j in ((0, 5), (6, 64), (9, 69)):                    # rows of x0 equal to rows of xn where they keep the dimension
        x0[i] = np.where(mask[i], np.nan, xn[j])
    if sort0:
        x0[:64, 0] = np.where(mask[:64, 0], np.nan, 0.5 * np.abs(np.nan_to_num(x0[:64, 0])) / 1.1)
        x0 = np.where(mask, np.nan, np.asarray(np.nan_to_num(x0), np.float32).astype(np.float64))
    t = rng.standard_normal((MG_Q, MG_M))
    lo, hi = MG_BOXES[box]
    bx = np.stack([np.full(d, lo), np.full(d, hi)])
    ths = [_mg_theta(d, kernel, k) for k in range(MG_Q)]
    fits = [_fit(x, Y, sr, th, dtype, kernel) for th in ths]
    p = dict(x=x, sr=sr, xn=xn, r=r, x0=x0, mask=mask, t=t, th=ths, fit=fits, dtype=dtype, kernel=kernel, d=d, box=bx)
    _MG_CACHE[key] = p
    return p


def _mg_table(p, k, x2, n2pad, i1=None, pad=1.0, shift=0):
    """the table (d x n2pad doubles, padding 1.0) and i2 (d) of component k over the inputs x2 from the restatement.  Defects:
    i1 (another I1), pad (the padding value), shift (row l holds the values of dimension l + shift)"""
    d, th, kernel = p["d"], p["th"][k], p["kernel"]
    x2r = _r(x2, p["dtype"])
    f = mref.I1 if i1 is None else i1
    tab = np.full((d, n2pad), pad)
    for l in range(d):
        ls = (l + shift) % d
        tab[l, :x2r.shape[0]] = f(kernel, x2r[:, ls], p["box"][0][ls], p["box"][1][ls], th[ls])
    i2 = np.array([float(mref.I2(kernel, p["box"][1][l] - p["box"][0][l], th[l])) for l in range(d)])
    return tab, i2


def _mg_X(p, k, tab, x2, cs, stale_chunk=False, read_masked=False):
    """the masked rows of component k against x2 (float64 from the rounded inputs, rounded once to the storage type): kept
    dimensions kappa(|x0 - x2| / ell), masked ones the table entry.  Defects: stale_chunk (the dimensions of the second
    32-dimension chunk take the table rows of the first), read_masked (x0 is loaded under the mask)"""
    d, th, kernel, dtype, mask = p["d"], p["th"][k], p["kernel"], p["dtype"], p["mask"]
    ell, scale, nug, Dk, _ = sb.split_theta(th, d)
    x2r = _r(x2, dtype)
    n2 = x2r.shape[0]
    x0r = _r(np.where(mask & (not read_masked), 0.0, p["x0"]), dtype)
    s = np.ones(n2) if cs is None else _r(cs, dtype)
    poly = np.ones((x0r.shape[0], n2))
    for l in range(d):
        ls = l - 32 if (stale_chunk and l >= 32) else l
        kept = mref.kappa(kernel, np.abs(x0r[:, l][:, None] - x2r[:, l][None, :]) / ell[l])
        use_tab = mask[:, l] & (not read_masked)
        poly = poly * np.where(use_tab[:, None], tab[ls, :n2][None, :], kept)
    return _r(scale * (1.0 - nug / (1.0 + nug)) * poly * s[None, :], dtype)


def _mg_prior(p, k, i2, keep_scale=False, nugget=False):
    d, th, mask = p["d"], p["th"][k], p["mask"]
    ell, scale, nug, Dk, _ = sb.split_theta(th, d)
    pr = np.full(mask.shape[0], scale if nugget else scale * (1.0 - nug / (1.0 + nug)))
    for l in range(d):
        pr = np.where(mask[:, l], pr * i2[l], pr)
    return np.where(mask.any(axis=1) & (not keep_scale), pr, scale)


def _mg_view(p, k):
    """a valid state of the view for component k (U_n, the dense L_S^-1, v), as lcgp_condition_prepare leaves it; its own stages are
    held by the conditioned-view tests above"""
    import scipy.linalg as sla
    dtype, kernel, th, f, d = p["dtype"], p["kernel"], p["th"][k], p["fit"][k], p["d"]
    T = _np_t(dtype)
    ell, scale, nug, Dk, _ = sb.split_theta(th, d)
    nt = nug / (1 + nug)
    m, mpad = MG_M, sb._pad128(MG_M)
    Xn = _r(_cross(p["xn"], p["x"], p["sr"], th, dtype, kernel), dtype)
    Un = np.asarray(_mm(Xn, f["W"], dtype), np.float64)
    xr = _r(p["xn"], dtype)
    cnn = scale * ((1 - nt) * sb.kernel_parts(xr, xr, ell, kernel, dtype)[0].numpy() + nt * np.eye(m))
    S = _axpy(_r(cnn, dtype), -Dk, _mm(Un, Un, dtype), dtype)
    rr = p["r"] if p["r"] is not None else np.ones(m)
    S[np.arange(m), np.arange(m)] = _r(np.diag(S) + 1.0 / (Dk * rr), dtype)
    L = np.linalg.cholesky(np.asarray(S, T))
    Wn = np.asarray(np.tril(sla.solve_triangular(L, np.eye(m, dtype=T), lower=True)), np.float64)
    Wd = np.eye(mpad)
    Wd[:m, :m] = Wn
    v = np.zeros(mpad)
    v[:m] = Wn @ (p["t"][k] - Xn @ f["z"])
    return dict(Un=Un, Wd=Wd, v=v)


def _mg_gcov(p, k, e, r, wrong_i2=False, drop_t=False):
    """gcov of every row against the reference row r of the same pass: the widened row [U_r | T_r] and the prior from the
    restatement.  Defects: wrong_i2 (I2 of dimension l + 1 where both rows integrate l), drop_t (T_i . T_r left out)"""
    d, th, kernel, dtype, mask = p["d"], p["th"][k], p["kernel"], p["dtype"], p["mask"]
    ell, scale, nug, Dk, _ = sb.split_theta(th, d)
    n, m, npad, mpad = MG_N, MG_M, sb._pad128(MG_N), sb._pad128(MG_M)
    ref = np.zeros(npad + mpad)
    ref[:n] = e["U"][r]
    ref[npad:npad + mpad] = e["Tm"][r]
    x0r = _r(np.where(mask, 0.0, p["x0"]), dtype)
    xr, mr = x0r[r], mask[r]
    pr = np.full(mask.shape[0], scale * (1.0 - nug / (1.0 + nug)))
    for l in range(d):
        lo, hi = p["box"][0][l], p["box"][1][l]
        kept = mref.kappa(kernel, np.abs(x0r[:, l] - xr[l]) / ell[l])
        if mr[l]:
            f = np.where(mask[:, l], e["i2"][(l + 1) % d if wrong_i2 else l], mref.I1(kernel, x0r[:, l], lo, hi, ell[l]))
        else:
            f = np.where(mask[:, l], float(mref.I1(kernel, xr[l], lo, hi, ell[l])), kept)
        pr = pr * f
    g = pr - Dk * (e["U"] @ e["U"][r])
    if not drop_t:
        g = g - e["Tm"][:, :m] @ e["Tm"][r, :m]
    return dict(ref=ref, xr=p["x0"][r], mr=mr, gcov=g)


def _mg_emulate(p, k, table=None, cross=None, prior=None, tab_of=None, as32=False):
    """every stage of component k.  Defects: table / cross / prior (keywords of _mg_table / _mg_X / _mg_prior), tab_of (the masked
    rows read the table of that component), as32 (X carries float32 accuracy)"""
    dtype, th, f, d = p["dtype"], p["th"][k], p["fit"][k], p["d"]
    Dk = sb.split_theta(th, d)[3]
    n0, n, m = MG_N0, MG_N, MG_M
    npad, mpad, n0pad = sb._pad128(n), sb._pad128(m), sb.predict_pad(n0)
    tab, i2 = _mg_table(p, k, p["x"], npad, **(table or {}))
    rd = tab if tab_of is None else _mg_table(p, tab_of, p["x"], npad)[0]
    X = _mg_X(p, k, rd, p["x"], p["sr"], **(cross or {}))
    if as32:
        X = _r(X, "float32")
    U = np.asarray(_mm(X, f["W"], dtype), np.float64)
    pr = _mg_prior(p, k, i2, **(prior or {}))
    gh, gv = X @ f["z"], pr - Dk * np.sum(U * U, axis=1)
    v = _mg_view(p, k)
    tabn, _ = _mg_table(p, k, p["xn"], mpad)
    Cn = _mg_X(p, k, tabn, p["xn"], None, **(cross or {}))
    Sg = np.zeros((n0pad, mpad))
    Sg[:n0, :m] = _axpy(Cn, -Dk, _mm(U, v["Un"], dtype), dtype)
    Tm = np.asarray(_mm(Sg, v["Wd"], dtype), np.float64)[:n0]
    gh1 = gh + Tm[:, :m] @ v["v"][:m]
    gv1 = gv - np.sum(Tm[:, :m] ** 2, axis=1)
    return dict(tab=tab, i2=i2, X=X, U=U, gh=gh, gv=gv, tabn=tabn, Cn=Cn, Sg=Sg[:n0, :m], Tm=Tm, gh1=gh1, gv1=gv1, **v)


def _mg_checks(p, k, e, gc=None, r=MG_REF_ROWS[2], stages=MG_STAGES):
    dtype, kernel, th, f, d = p["dtype"], p["kernel"], p["th"][k], p["fit"][k], p["d"]
    x, sr, xn, x0, mask, box = p["x"], p["sr"], p["xn"], p["x0"], p["mask"], p["box"]
    n, m, npad, mpad = MG_N, MG_M, sb._pad128(MG_N), sb._pad128(MG_M)
    out = {}
    for st in stages:
        if st == "table":
            out[st] = sb.check_marg_table(e["tab"][None], e["i2"][None], x, th[None], box, kernel, dtype, n, npad)
        elif st == "cross":
            out[st] = sb.check_marg_cross(e["X"], e["tab"], x0, mask, x, sr, th, kernel, dtype)
        elif st == "u":
            out[st] = sb.check_cov_u(e["U"], e["X"], f["W"], dtype)
        elif st == "out":
            out[st] = sb.check_marg_out(e["gh"], e["gv"], e["X"], e["U"], f["z"], e["i2"], mask, th, dtype)
        elif st == "table_n":
            out[st] = sb.check_marg_table(e["tabn"][None], e["i2"][None], xn, th[None], box, kernel, dtype, m, mpad)
        elif st == "cross_n":
            out[st] = sb.check_marg_cross(e["Cn"], e["tabn"], x0, mask, xn, None, th, kernel, dtype)
        elif st == "cond_cross":
            out[st] = sb.check_marg_cond_cross(e["Sg"], e["U"], e["Un"], e["tabn"], x0, mask, xn, th, kernel, dtype)
        elif st == "cond_t":
            out[st] = sb.check_cov_u(e["Tm"][:, :m], e["Sg"], e["Wd"][:m, :m], dtype)
        elif st == "cond_out":
            out[st] = sb.check_cond_out(e["gh1"], e["gv1"], e["Tm"], e["v"], e["gh"], e["gv"], m)
        elif st == "gcov":
            g = _mg_gcov(p, k, e, r) if gc is None else gc
            out[st] = sb.check_marg_refcov(g["gcov"], e["U"], e["Tm"], g["ref"], x0, mask, g["xr"], g["mr"], box, e["i2"], th,
                                           kernel, dtype, n, m, ref_rows=(np.pad(e["U"][r], (0, npad - n)), e["Tm"][r]))
    return out


def _mg_only(checks, *failing):
    first = min(MG_STAGES.index(f) for f in failing)
    for stage in MG_STAGES[:first]:
        if stage in checks:
            assert checks[stage].ratio <= 1.0, ("upstream", stage, checks[stage])
    for stage in failing:
        assert checks[stage].ratio > 1.0, (stage, checks[stage])


def _mg_table_ratios(p, k, e):
    """every ratio of the table entries of component k (n d values)"""
    xr = _r(p["x"], p["dtype"])
    return np.concatenate([sb.marg_table_ratios(p["kernel"], e["tab"][l, :MG_N], xr[:, l], p["box"][0][l], p["box"][1][l], p["th"][k][l])
                           for l in range(p["d"])])


@pytest.mark.parametrize("d,box", [(3, "default"), (3, "sub"), (34, "default"), (34, "sub")])
@pytest.mark.parametrize("rep", [False, True], ids=["full", "rep"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_emulated_marginal_path_passes_every_stage(dtype, kernel, rep, d, box):
    """every stage at or below 1, with every kind of reference row for gcov; and the two conditions that keep the table bound
    honest: at most 1 % of its entries have a bound set by the absolute floor, and the median ratio of the emulation is above
    1e-3 (the bound is within three orders of what correct code does)"""
    p = _mg_problem(dtype, kernel, rep, d, box)
    for k in range(MG_Q):
        e = _mg_emulate(p, k)
        checks = _mg_checks(p, k, e)
        for r in MG_REF_ROWS[:2]:
            checks["gcov r%d" % r] = _mg_checks(p, k, e, r=r, stages=("gcov",))["gcov"]
        med = float(np.median(_mg_table_ratios(p, k, e)))
        fl = sb.marg_floor_fraction(p["x"], p["th"][k], p["box"], kernel, dtype)
        print("marginal, emulated, %s %s %s d=%d %s k%d: %s  table median %.2e floor fraction %.4f"
              % (dtype, kernel, "rep" if rep else "full", d, box, k, "  ".join("%s %.2e" % (s, c.ratio) for s, c in checks.items()),
                 med, fl))
        for stage, c in checks.items():
            assert c.ratio <= 1.0, (k, stage, c)
        assert med > 1e-3, (k, med)
        assert fl <= 0.01, (k, fl)


# the restatement against mpmath, on every switch: b = 1/2 and bn = 1 with their float64 neighbours, x on lo, on hi and one ulp
# either side, w / ell from 1e-4 to 50, ell from 0.02 to 30.  With lo = 0 the difference x - lo is exact and b = x / ell sits on the
# switch (ell = 1: exactly, with both neighbours); with lo = 0.25 it is rounded first.  The neighbours are taken in x and b is
# recomputed from x as the library does
MG_GRID_ELL = (0.02, 0.3, 1.0, 7.0, 30.0)
MG_GRID_WL = (1e-4, 1e-3, 1e-2, 0.1, 0.5, 1.0, 3.0, 50.0)


def _mg_grid(ell, w, lo):
    hi = lo + w
    xs = []
    for b in (0.0, 1e-9, 1e-3, 0.1, 0.25, 0.5, 0.75, 1.0, 1.5, 3.0, 8.0, 20.0, 40.0):
        for base in (lo - b * ell, hi + b * ell, lo + b * ell, hi - b * ell):
            xs += [np.nextafter(base, -np.inf), base, np.nextafter(base, np.inf)]
    for base in (lo, hi):
        xs += [np.nextafter(base, -np.inf), base, np.nextafter(base, np.inf)]
    return lo, hi, np.unique(np.asarray(xs, np.float64))


@pytest.mark.parametrize("kernel", KERNELS)
def test_marginal_restatement_meets_the_table_bound_against_mpmath(kernel):
    """tests/marginal_ref.py's I1 (through its F and Fc in all three branches) and I2 (F and G) against marg_exact / marg_exact2
    within the bound of check_marg_table: the structure the restatement shares with the kernel is itself held to an
    independent reference.  The worst relative error per class is printed (the narrow-box loss ~ u ell / w among them)"""
    worst, relw = 0.0, {}
    for ell in MG_GRID_ELL:
        for wl, lo0 in [(w_, l_) for w_ in MG_GRID_WL for l_ in (0.0, 0.25)]:
            lo, hi, xs = _mg_grid(ell, wl * ell, lo0)
            got = mref.I1(kernel, xs, lo, hi, ell)
            r = sb.marg_table_ratios(kernel, got, xs, lo, hi, ell)
            assert np.all(r <= 1.0), (kernel, ell, wl, float(r.max()), float(xs[int(np.argmax(r))]))
            worst = max(worst, float(r.max()))
            ex = np.array([float(v) for v in sb.marg_exact(kernel, xs, lo, hi, ell)])
            ok = ex > 1e-300
            relw[wl] = max(relw.get(wl, 0.0), float(np.max(np.abs(got[ok] - ex[ok]) / ex[ok])) / sb.unit("float64"))
            i2 = float(mref.I2(kernel, hi - lo, ell))
            with sb.mp.workdps(60):
                e2 = float(abs(sb.mp.mpf(i2) - sb.marg_exact2(kernel, sb.mp.mpf(hi) - sb.mp.mpf(lo), ell)))
            r2 = e2 / (sb.C * sb.marg_i2_bound(kernel, hi - lo, ell) + sb.floor("float64", 1))
            assert r2 <= 1.0, (kernel, ell, wl, r2)
            for which in ("F", "G", "Fc"):
                for b in (np.nextafter(0.5, 0), 0.5, np.nextafter(0.5, 1), np.nextafter(1.0, 0), 1.0, np.nextafter(1.0, 2), wl):
                    g = float(getattr(mref, which)(kernel, b))
                    with sb.mp.workdps(60):
                        eb = float(abs(sb.mp.mpf(g) - sb._marg_mp(kernel, which, sb.mp.mpf(float(b)))))
                    assert eb <= sb.C * sb.unit("float64") * float(sb._marg_terms(kernel, which, b)), (kernel, which, b, eb)
    print("restatement against mpmath, %s: worst ratio %.3f; worst relative error of I1 in u per w / ell: %s"
          % (kernel, worst, "  ".join("%g: %.3g" % kv for kv in sorted(relw.items()))))


def _i1_variant(near_always=False, erf_tail=False):
    """I1 of the restatement with a wrong branch: the near-branch formula F(bf) - F(bn) also beyond bn = 1"""
    def i1(kernel, x, lo, hi, ell):
        x, lo, hi, ell = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (x, lo, hi, ell)))
        a1, a2 = x - lo, hi - x
        b1, b2 = np.abs(a1) / ell, np.abs(a2) / ell
        inside = (a1 >= 0.0) & (a2 >= 0.0)
        bn, bf = np.minimum(b1, b2), np.maximum(b1, b2)
        r = np.where(inside, mref.F(kernel, b1) + mref.F(kernel, b2), mref.F(kernel, bf) - mref.F(kernel, bn))
        return ell / (hi - lo) * r
    return i1


def test_marginal_defects_of_the_table(monkeypatch):
    """a wrong Matern-5/2 coefficient in F; 10 series terms at b just below 1/2; the near-branch formula far out in the tail
    (Matern) and erf differences in place of erfc (SE: the same mistake in its kernel); a padding column that is not 1; the row
    of the next dimension.  Each fails check_marg_table, and the untouched table passes"""
    # (1) 8/3 -> 8/3 (1 + 1e-12) in the closed form of F
    p = _mg_problem("float64", "matern52", False, 3, "default")
    good = _mg_emulate(p, 0)
    assert _mg_checks(p, 0, good, stages=("table",))["table"].ratio <= 1.0
    closed = mref._closed

    def wrong_closed(kernel, b):
        f, g = closed(kernel, b)
        return f + (8.0 / 3.0) * 1e-12 * -np.expm1(-b), g
    monkeypatch.setattr(mref, "_closed", wrong_closed)
    _mg_only(_mg_checks(p, 0, _mg_emulate(p, 0), stages=("table",)), "table")
    monkeypatch.setattr(mref, "_closed", closed)
    # (2) ten terms of the series: seen on the grid, at the first b below 1/2
    for kernel in ("matern32", "matern52"):
        lo, hi, ell = 0.0, 1.0, 1.0
        xs = np.array([np.nextafter(0.5, 0), 0.49])
        monkeypatch.setattr(mref, "SERIES_TERMS", 10)
        bad = mref.I1(kernel, xs, lo, hi, ell)
        monkeypatch.setattr(mref, "SERIES_TERMS", 20)
        assert np.all(sb.marg_table_ratios(kernel, bad, xs, lo, hi, ell) > 1.0)
        assert np.all(sb.marg_table_ratios(kernel, mref.I1(kernel, xs, lo, hi, ell), xs, lo, hi, ell) <= 1.0)
    # (3), (4) the near-branch formula beyond bn = 1, in the sub-box problem whose inputs lie up to 15 lengthscales outside
    for kernel in KERNELS:
        p = _mg_problem("float64", kernel, False, 3, "sub")
        c = _mg_checks(p, 0, _mg_emulate(p, 0, table=dict(i1=_i1_variant())), stages=("table",))["table"]
        assert c.ratio > 1.0 and c.where[1] == 0, (kernel, c)                  # (dimension 0: ell = 0.02)
    # (5) the padding, (6) the next dimension's row
    p = _mg_problem("float32", "matern32", True, 3, "sub")
    for defect in (dict(pad=0.0), dict(pad=np.nextafter(1.0, 2.0)), dict(pad=np.nan), dict(shift=1)):
        _mg_only(_mg_checks(p, 1, _mg_emulate(p, 1, table=defect), stages=("table",)), "table")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_marginal_defects_of_the_masked_rows_and_outputs(dtype):
    """the table of the next component read; the second 32-dimension chunk staged with the first chunk's table rows; x0 read under
    the mask (NaN there); the prior of a masked row left at scale; the nugget kept in the prior; I2 of the wrong dimension and
    T_i . T_r dropped in gcov: each fails its own stage and nothing upstream"""
    front = ("table", "cross", "u", "out")
    p = _mg_problem(dtype, "matern52", True, 3, "sub")
    _mg_only(_mg_checks(p, 0, _mg_emulate(p, 0, tab_of=1), stages=front), "cross")
    p34 = _mg_problem(dtype, "matern32", False, 34, "default")
    c = _mg_checks(p34, 0, _mg_emulate(p34, 0, cross=dict(stale_chunk=True)), stages=front + ("table_n", "cross_n"))
    _mg_only(c, "cross", "cross_n")
    for q in (p, p34):
        c = _mg_checks(q, 1, _mg_emulate(q, 1, cross=dict(read_masked=True)), stages=("table", "cross"))
        _mg_only(c, "cross")
        assert c["cross"].ratio == np.inf
    _mg_only(_mg_checks(p, 0, _mg_emulate(p, 0, prior=dict(keep_scale=True)), stages=front), "out")
    _mg_only(_mg_checks(p, 0, _mg_emulate(p, 0, prior=dict(nugget=True)), stages=front), "out")
    e = _mg_emulate(p, 0)
    for r in (MG_REF_ROWS[1], MG_REF_ROWS[2]):
        for defect in (dict(wrong_i2=True), dict(drop_t=True)):
            assert _mg_checks(p, 0, e, r=r, stages=("gcov",))["gcov"].ratio <= 1.0
            c = _mg_checks(p, 0, e, gc=_mg_gcov(p, 0, e, r, **defect), r=r, stages=("gcov",))["gcov"]
            assert c.ratio > 1.0, (r, defect, c)
    g = _mg_gcov(p, 0, e, 4)
    g["ref"] = g["ref"].copy()
    g["ref"][1] = np.nextafter(g["ref"][1], 1.0)
    assert _mg_checks(p, 0, e, gc=g, r=4, stages=("gcov",))["gcov"] == sb.Check(np.inf, ("ref",))


def test_marginal_defect_float32_rows_in_the_float64_check():
    p = _mg_problem("float64", "se", False, 3, "default")
    _mg_only(_mg_checks(p, 0, _mg_emulate(p, 0, as32=True), stages=("table", "cross")), "cross")


def test_marginal_gap_small_table_entries_and_a_far_tile_are_invisible_normwise():
    """what the stage bounds close.  (a) the table entries of the inputs far outside the sub-box (below 1e-3 of the row's largest)
    off by 1e-9 relative; (b) one 64-tile of the masked rows, whose entries are small, off by 1e-9 relative.  Both leave ghat and
    gvar within the 1e-10 of max|err| / max|ref| that tests/test_gpu_marginal.py holds them to -- computed here -- and both fail
    their stage check.  The training inputs are sorted along dimension 0 (lengthscale 0.02) and rows 0 .. 63 of x0 keep to its
    lower half where they keep it, so the last column tile is far from the first row tile"""
    p = _mg_problem("float64", "matern32", False, 3, "sub", sort0=True)
    k = 0
    e = _mg_emulate(p, k)
    assert all(c.ratio <= 1.0 for c in _mg_checks(p, k, e, stages=("table", "cross", "u", "out")).values())
    f, Dk = p["fit"][k], p["th"][k][p["d"] + 2]

    def outputs(X):
        U = np.asarray(_mm(X, f["W"], "float64"), np.float64)
        return X @ f["z"], _mg_prior(p, k, e["i2"]) - Dk * np.sum(U * U, axis=1)
    # (a)
    tab = e["tab"].copy()
    small = tab[0, :MG_N] < 1e-3 * tab[0, :MG_N].max()
    assert 10 <= small.sum() < MG_N
    tab[0, :MG_N][small] *= 1 + 1e-9
    gh, gv = outputs(_mg_X(p, k, tab, p["x"], p["sr"]))
    eh, ev = _normwise(gh, e["gh"]), _normwise(gv, e["gv"])
    print("gap (a): end-to-end change ghat %.3e gvar %.3e (bar 1e-10)" % (eh, ev))
    assert eh < 1e-10 and ev < 1e-10
    c = sb.check_marg_table(tab[None], e["i2"][None], p["x"], p["th"][k][None], p["box"], "matern32", "float64", MG_N, 256)
    assert c.ratio > 1.0 and c.where[:2] == (0, 0), c
    # (b)
    rows, cols = _tile(0, (MG_N - 1) // TS)
    X = e["X"].copy()
    assert np.abs(X[rows, cols]).max() < 1e-2 * np.abs(X).max() and np.abs(X[rows, cols]).max() > 0
    X[rows, cols] *= 1 + 1e-9
    gh, gv = outputs(X)
    eh, ev = _normwise(gh, e["gh"]), _normwise(gv, e["gv"])
    print("gap (b): end-to-end change ghat %.3e gvar %.3e (bar 1e-10)" % (eh, ev))
    assert eh < 1e-10 and ev < 1e-10
    c = sb.check_marg_cross(X, e["tab"], p["x0"], p["mask"], p["x"], p["sr"], p["th"][k], "matern32", "float64")
    assert c.ratio > 1.0 and c.where == (0, (MG_N - 1) // TS), c


# ======================================================================================================================
# the two parameter-space queries (lcgp_nll_hess, lcgp_predict_paramgrad), emulated stage by stage in float64: each stage from
# the previous stage's stored result, in the kernels' blocked order (4 x 4 dimension block pairs, HS_JC chunks of j, 64-bands,
# PP_DB blocks of dimensions).  n = 150: npad = 256, four bands, the third ragged, the fourth all padding.
# ======================================================================================================================
PH_N, PH_P, PH_N0 = 150, 3, 70
PH_STAGES = ("hess_prep", "hess_mirror", "hess_da", "hess_y", "hess_g", "hess_trace", "hess_contract", "hess_vectors", "hess_out")
PP_STAGES = ("hess_prep", "hess_da", "pp_y", "pp_t", "pp_rowdot", "pp_sums", "pp_vy", "pp_out")
_PH_CACHE = {}


def _ph_problem(d, kernel="matern32", rep=False, seed=21, n=PH_N):
    """x in the unit box; lengthscales sqrt(d) exp(U(-1, 0.3)): sum_l S_l stays below ~10, so C0 is far from the cut-off and
    from underflow and the only entries whose bound the floor sets are exact zeros (the diagonal of d_iA: phi(0) = 0).  D in
    (0.2, 2): cond(A) <= 1 + D scale sum s^2 stays near that of the problems of the host files whose bars the ties below use"""
    key = (d, kernel, rep, seed, n)
    if key not in _PH_CACHE:
        rng = np.random.default_rng(seed + d)
        x, Y = rng.uniform(0.0, 1.0, (n, d)), rng.standard_normal((PH_P, n))
        sr = np.sqrt(rng.integers(1, 6, n).astype(np.float64)) if rep else None
        th = np.zeros((2, d + 3 + PH_P))
        for k in range(2):
            th[k, :d] = np.sqrt(d) * np.exp(rng.uniform(-1.0, 0.3, d))
            th[k, d:d + 3] = rng.uniform(0.5, 2.0), 10.0 ** rng.uniform(-4.0, -2.0), rng.uniform(0.2, 2.0)
            th[k, d + 3:] = rng.standard_normal(PH_P) / np.sqrt(PH_P)
        x0 = rng.uniform(-0.1, 1.1, (PH_N0, d))
        x0[:3] = x[:3]
        _PH_CACHE[key] = dict(x=x, Y=Y, sr=sr, th=th, kernel=kernel, n=n, d=d, p=PH_P, x0=x0, fit={})
    return _PH_CACHE[key]


def _ph_phi(S, ell, kernel):
    """hess_phi of lcgp_hip.hip"""
    ie, S2 = 1.0 / ell, S * S
    if kernel == "matern32":
        r = 1.0 / (1.0 + S)
        return S2 * r * ie, -S2 * (2.0 * S + 3.0) * (r * r) * (ie * ie)
    if kernel == "se":
        return S2 * ie, -3.0 * S2 * (ie * ie)
    assert kernel == "matern52"
    r = 1.0 / (S * S + (3.0 * S + 3.0))
    N = S2 * (1.0 + S)
    return N * r * ie, -(S2 * (3.0 * S + 2.0) * r + N * (3.0 - S2) * (r * r)) * (ie * ie)


def _ph_c0(xa, xb, kernel):
    """hess_c0 / the row loop of pgrad_row_kernel: C0 from scaled inputs (d x na), (d x nb)"""
    poly, ssum = np.ones((xa.shape[1], xb.shape[1])), np.zeros((xa.shape[1], xb.shape[1]))
    for l in range(xa.shape[0]):
        df = xa[l][:, None] - xb[l][None, :]
        sd = np.abs(df)
        if kernel == "matern32":
            poly, ssum = poly * sd + poly, ssum - sd
        elif kernel == "se":
            ssum = -0.5 * df * df + ssum
        else:
            poly, ssum = poly * (sd * (1.0 / 3.0) * sd + sd) + poly, ssum - sd
    return np.exp(ssum) if kernel == "se" else poly * np.exp(ssum)


def _ph_fit(P, k):
    """the workspace of component k: A^-1 as the library stores it (lower triangle written, the upper one not), its fetched
    (mirrored) form, b and z"""
    if k not in P["fit"]:
        n, d = P["n"], P["d"]
        ell, scale, nug, D, psi = sb.split_theta(P["th"][k], d)
        s = np.ones(n) if P["sr"] is None else P["sr"]
        xs = (P["x"] / ell[None, :]).T
        nt = nug / (1.0 + nug)
        A = np.eye(n) + D * scale * np.outer(s, s) * ((1.0 - nt) * _ph_c0(xs, xs, P["kernel"]) + nt * np.eye(n))
        low = np.tril(scipy.linalg.cho_solve((np.linalg.cholesky(A), True), np.eye(n)))
        V = low + np.tril(low, -1).T
        raw = low + np.triu(np.random.default_rng(5).standard_normal((n, n)), 1)
        b = P["Y"].T @ psi
        P["fit"][k] = dict(V=V, raw=raw, b=b, z=V @ b)
    return P["fit"][k]


def _ph_prep(P, k, npad, bug=None):
    n, d = P["n"], P["d"]
    f = _ph_fit(P, k)
    ell, scale, nug, D, _ = sb.split_theta(P["th"][k], d)
    s = np.ones(n) if P["sr"] is None else P["sr"]
    xs, yv = np.zeros((d, npad)), np.zeros((d + 2, npad))
    xs[:, :n] = (P["x"] / ell[None, :]).T
    bz = f["b"] - f["z"]
    yv[d, :n] = bz / scale
    yv[d + 1, :n] = (D * scale * (1.0 if bug == "ynug_no_s2" else s * s) * f["z"] - bz) / (1.0 + nug)
    return xs, yv


def _ph_da(P, k, xs, i):
    """hess_da_kernel: d_iA as a full npad x npad matrix, zero on the padding"""
    n, d, npad = P["n"], P["d"], xs.shape[1]
    ell, scale, nug, D, _ = sb.split_theta(P["th"][k], d)
    s = np.ones(n) if P["sr"] is None else P["sr"]
    E = np.zeros((npad, npad))
    phi = _ph_phi(np.abs(xs[i, :n, None] - xs[i, None, :n]), ell[i], P["kernel"])[0]
    E[:n, :n] = (D * scale / (1.0 + nug)) * np.outer(s, s) * _ph_c0(xs[:, :n], xs[:, :n], P["kernel"]) * phi
    return E


def _ph_final(tp, cp, dot, th, d, bug=None):
    """hess_final_kernel"""
    m, B = d + 2, sb.HS_B
    _, scale, nug, D, _ = sb.split_theta(th, d)
    omw = 1.0 / (1.0 + nug)
    w1 = 1.0 / ((1.0 + nug) * (1.0 + nug))
    slot_sum = lambda pb, slot: cp[pb, :, slot].sum()
    hk = np.zeros((m, m))
    for i in range(m):
        for j in range(i + 1):
            if i < d:
                bi, bj = i // B, j // B
                T = scale * omw * slot_sum(bi * (bi + 1) // 2 + bj, (i % B) * B + j % B)
            elif j < d:
                bj = j // B
                s1 = slot_sum(bj if bug == "first_order_pair_bj" else bj * (bj + 1) // 2, 16 + j % B)
                T = omw * s1 if i == d else -scale * w1 * s1
            else:
                dd = slot_sum(0, 21) - slot_sum(0, 20)
                T = 0.0 if i == d else (w1 * dd if j == d else -2.0 * scale * w1 * omw * dd)
            hk[i, j] = hk[j, i] = (T - 0.5 * tp[i * (i + 1) // 2 + j].sum()) + dot[i, j] / D
    return hk


def _ph_emulate(P, k, bug=None):
    """lcgp_nll_hess on component k: every buffer of HessLay and the row of `out`.  `bug` plants one defect"""
    n, d, p, kernel = P["n"], P["d"], P["p"], P["kernel"]
    th = P["th"][k]
    ell, scale, nug, D, psi = sb.split_theta(th, d)
    L = sb.hess_layout(n, d, p, 1)
    m, npad, nb, ppad, npair, npb = L["m"], L["npad"], L["nb"], L["ppad"], L["npair"], L["npb"]
    f = _ph_fit(P, k)
    s = np.ones(n) if P["sr"] is None else P["sr"]
    spad = np.ones(npad)
    spad[:n] = s
    xs, yv = _ph_prep(P, k, npad, bug)
    # hess_mirror_kernel
    AI = np.eye(npad)
    raw = f["raw"]
    AI[:n, :n] = np.triu(raw) + np.triu(raw, 1).T if bug == "mirror_upper" else np.tril(raw) + np.tril(raw, -1).T
    G = np.zeros((m, npad, npad))
    v, dl = AI[:n, :n], np.eye(n)
    G[d][:n, :n] = (dl - v) / scale
    c = D * scale * (s * s)
    G[d + 1][:n, :n] = ((c[:, None] if bug == "gnug_sa" else c[None, :]) * v + v - dl) / (1.0 + nug)
    # per dimension: d_iA, y_i, G_i
    for i in range(d):
        E = _ph_da(P, k, xs, i)
        yv[i] = E @ np.concatenate([f["z"], np.zeros(npad - n)])
        G[i] = AI @ E
    # hess_trace_kernel: one workgroup per (band, i, chunk of HS_JC values of j)
    tp = np.full((npair, nb), np.nan)
    njc, late = -(-m // sb.HS_JC), []
    for i in range(m):
        for jc in range(njc):
            j0 = jc * sb.HS_JC
            if j0 > i:
                continue
            for jj in range(sb.HS_JC):
                j = j0 + jj
                if j >= m or not (j <= i or (bug == "chunk2_all" and jc > 0)):
                    continue
                vals = (G[i] * G[j].T).reshape(nb, TS * npad).sum(axis=1)
                idx = i * m + j if bug == "pair_im" else i * (i + 1) // 2 + j
                if j > i:
                    late.append((idx, vals))
                elif idx < npair:
                    tp[idx] = vals
    for idx, vals in late:
        if idx < npair:
            tp[idx] = vals
    # hess_contract_kernel: one workgroup per (band, block pair)
    lim = npad if bug == "band_past_n" else n
    zp = np.concatenate([f["z"], np.zeros(npad - n)])[:lim]
    g = np.outer(spad[:lim], spad[:lim]) * (0.5 * D * AI[:lim, :lim] - 0.5 * np.outer(zp, zp))
    w0 = g * _ph_c0(xs[:, :lim], xs[:, :lim], kernel)
    ph = [_ph_phi(np.abs(xs[l, :lim, None] - xs[l, None, :lim]), ell[l], kernel) for l in range(d)]
    if bug == "dphi_m32":
        ph = [(ph[l][0], _ph_phi(np.abs(xs[l, :lim, None] - xs[l, None, :lim]), ell[l], "matern32")[1]) for l in range(d)]

    def bands(M):
        out = np.zeros(npad)
        out[:lim] = M.sum(axis=1)
        return out.reshape(nb, TS).sum(axis=1)

    cp = np.full((npb, nb, sb.HS_SLOTS), np.nan)
    B = sb.HS_B
    for pb in range(npb):
        bi, bj = sb.tri_decode(pb)
        for ii in range(B):
            li = bi * B + ii
            pi = ph[li][0] if li < d else 0.0
            cp[pb, :, 16 + ii] = bands(w0 * pi)
            for jj in range(B):
                lj = bj * B + jj
                pj = ph[lj][0] if lj < d else 0.0
                k2 = pi * pj
                if li < d and ii == jj and (bi == bj or bug == "dphi_offdiag"):
                    k2 = k2 + ph[li][1]
                slot = jj * B + ii if (bug == "a2_transposed" and bi != bj) else ii * B + jj
                cp[pb, :, slot] = bands(w0 * k2) if (li < d and lj < d) else 0.0
        cp[pb, :, 20], cp[pb, :, 21] = bands(w0), bands(np.diag(np.diag(g)))
    # u_i, dot, YP, Q
    uv = yv @ AI.T
    dot = yv @ uv.T
    YP = np.zeros((ppad, npad))
    YP[:p, :n] = P["Y"]
    Q = YP @ AI
    # the three output blocks
    hx = (uv[:, :n] @ YP[:p, :n].T) * psi[None, :] / (2.0 * D)
    sdot = YP[:p, :n] @ (YP[:p, :n] - Q[:p, :n]).T
    tdot = np.zeros(p) if bug == "hn_no_diag" else YP[:p, :n] @ (f["b"] - f["z"])
    hn = -(np.diag(psi * tdot) + np.outer(psi, psi) * sdot) / (4.0 * D)
    hk = _ph_final(tp, cp, dot, th, d, bug)
    out = np.concatenate([hk.reshape(-1), hx.reshape(-1), hn.reshape(-1)])
    return dict(xs=xs, yv=yv, AI=AI, G=G, E=E, tp=tp, cp=cp, uv=uv, dot=dot, YP=YP, Q=Q, out=out)


def _ph_checks(P, k, e, stages=PH_STAGES):
    n, d, p, th, f = P["n"], P["d"], P["p"], P["th"][k], _ph_fit(P, k)
    R = sb.hess_parts(e["xs"], P["sr"], th, P["kernel"], n)
    fns = dict(hess_prep=lambda: sb.check_hess_prep(e["xs"], e["yv"], P["x"], P["sr"], th, f["b"], f["z"]),
               hess_mirror=lambda: sb.check_hess_mirror(e["AI"], e["G"][d], e["G"][d + 1], f["V"], P["sr"], th, n, d),
               hess_da=lambda: sb.check_hess_da(e["E"], R, d - 1),
               hess_y=lambda: sb.check_hess_y(e["yv"], R, f["z"]),
               hess_g=lambda: sb.check_hess_g(e["G"], e["AI"], e["E"], R),
               hess_trace=lambda: sb.check_hess_trace(e["tp"], e["G"], n),
               hess_contract=lambda: sb.check_hess_contract(e["cp"], e["AI"], R, f["z"], th),
               hess_vectors=lambda: sb.check_hess_vectors(e["uv"], e["dot"], e["YP"], e["Q"], e["AI"], e["yv"], P["Y"], n),
               hess_out=lambda: sb.check_hess_out(e["out"], e["YP"], e["uv"], e["Q"], f["b"], f["z"], e["tp"], e["cp"], e["dot"],
                                                  th, n, d, p))
    return {s: fns[s]() for s in stages}


def _stage_only(order, checks, *failing):
    """every stage listed in `failing` is above 1, every stage upstream of the first of them at or below 1"""
    first = min(order.index(f) for f in failing)
    for stage in order[:first]:
        if stage in checks:
            assert checks[stage].ratio <= 1.0, ("upstream", stage, checks[stage])
    for stage in failing:
        assert checks[stage].ratio > 1.0, (stage, checks[stage])


def _floor_condition(log):
    """at most 1 % of the entries of any stage have their bound set by the absolute floor"""
    tot = {}
    for stage, floored, entries in log:
        a, b = tot.get(stage, (0, 0))
        tot[stage] = (a + floored, b + entries)
    for stage, (floored, entries) in tot.items():
        assert floored <= 0.01 * entries, (stage, floored, entries)
    return tot


def _normwise_blocks(got, want):
    return max(float(np.max(np.abs(g - w)) / np.max(np.abs(w))) for g, w in zip(got, want))


@pytest.mark.parametrize("d", [3, 9])
@pytest.mark.parametrize("rep", [False, True], ids=["full", "rep"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_emulated_nll_hess_passes_every_stage(kernel, rep, d, monkeypatch):
    """every stage at or below 1, the floor sets at most 1 % of the bounds of any stage, and the emulated output blocks agree
    with the numpy closed form of tests/test_nll_hess_host.py -- which that file ties to the autograd Hessian of
    tests/nll_hess_ref.py -- at its bar (EPS_REF = 1e-14 of the largest entry per block), on the same A^-1"""
    import types
    from tests import test_nll_hess_host as host
    P = _ph_problem(d, kernel, rep)
    log = []
    monkeypatch.setattr(sb, "FLOOR_LOG", log)
    for k in range(2):
        e = _ph_emulate(P, k)
        checks = _ph_checks(P, k, e)
        print(kernel, rep, d, k, {s: "%.2e" % c.ratio for s, c in checks.items()})
        for stage, c in checks.items():
            assert c.ratio <= 1.0, (stage, c)
        m, p = d + 2, P["p"]
        got = e["out"][:m * m].reshape(m, m), e["out"][m * m:m * m + m * p].reshape(m, p), e["out"][m * m + m * p:].reshape(p, p)
        # (the closed form takes the emulation's A^-1 -- the mirrored lower triangle, the input of both -- in place of its own
        # solve: the two inverses differ by eps cond(A), which the noise corner's I - A^-1 magnifies past the bar)
        monkeypatch.setattr(host, "sla", types.SimpleNamespace(cho_solve=lambda c, b, V=_ph_fit(P, k)["V"]: V))
        assert _normwise_blocks(got, host.component_blocks(P["x"], P["Y"], P["sr"], P["th"][k], kernel)) <= host.EPS_REF
    _floor_condition(log)


HESS_DEFECTS = [("dphi_offdiag", "hess_contract"), ("a2_transposed", "hess_contract"), ("first_order_pair_bj", "hess_out"),
                ("chunk2_all", "hess_trace"), ("pair_im", "hess_trace"), ("band_past_n", "hess_contract"),
                ("gnug_sa", "hess_mirror"), ("ynug_no_s2", "hess_prep"), ("mirror_upper", "hess_mirror"),
                ("hn_no_diag", "hess_out"), ("dphi_m32", "hess_contract")]


@pytest.mark.parametrize("bug,stage", HESS_DEFECTS)
def test_nll_hess_defect_fails_its_stage_and_none_upstream(bug, stage):
    """d = 9 (three blocks of four dimensions, six block pairs, m = 11: two HS_JC chunks), the replicated path (s_a against s_b,
    s^2 in y_nug); Matern-5/2 for the wrong d phi: dphi on an off-diagonal block pair, a2 transposed there, a first-order slot
    read from pair bj (2 instead of 3 for the third block), a second chunk that also sums j > i, a trace pair written at
    i m + j, a band past n included (the identity padding of AI reaches slots 20 and 21), G_nug with the row's s, y_nug without
    s^2, the mirror from the unwritten triangle, hn without its diagonal term, the Matern-3/2 d phi under Matern-5/2"""
    P = _ph_problem(9, "matern52" if bug == "dphi_m32" else "matern32", True)
    checks = _ph_checks(P, 0, _ph_emulate(P, 0, bug))
    print(bug, {s: "%.2e" % c.ratio for s, c in checks.items()})
    _stage_only(PH_STAGES, checks, stage)


def test_nll_hess_gap_small_ell_ell_entry_is_invisible_normwise():
    """the smallest ell-ell entry of hk off by 1e-6 relative: max|H - H_ref| / max|H_ref| of the kernel block stays below the 1e-11
    of tests/test_gpu_nll_hess.py, and check_hess_out fails at that entry"""
    P = _ph_problem(9, "matern32", False)
    d, m = 9, 11
    e = _ph_emulate(P, 0)
    hk = e["out"][:m * m].reshape(m, m).copy()
    sub = np.abs(hk[:d, :d]) + np.triu(np.full((d, d), np.inf), 1)
    i, j = np.unravel_index(int(np.argmin(sub)), sub.shape)
    bad = hk.copy()
    bad[i, j] = bad[j, i] = hk[i, j] * (1.0 + 1e-6)
    nw = np.max(np.abs(bad - hk)) / np.max(np.abs(hk))
    print("hk[%d, %d] = %.3e of max %.3e: normwise %.3e (bar 1e-11)" % (i, j, hk[i, j], np.max(np.abs(hk)), nw))
    assert 0 < nw <= 1e-11
    out = e["out"].copy()
    out[:m * m] = bad.reshape(-1)
    e2 = dict(e, out=out)
    c = _ph_checks(P, 0, e2, stages=("hess_out",))["hess_out"]
    assert c.ratio > 1.0 and c.where == ("hk", i, j), c


# ---- lcgp_predict_paramgrad --------------------------------------------------------------------------------------------
def _pp_x0(P, same, n0=PH_N0):
    """same = 0: new inputs, the first three of them training inputs (phi = 0 at distance 0); same = lo + 1: rows lo .. lo + n0
    of the training set, as a chunked caller passes them"""
    return P["x0"][:n0] if same == 0 else P["x"][same - 1:same - 1 + n0]


def _pp_emulate(P, k, same=0, bug=None, n0=PH_N0):
    """lcgp_predict_paramgrad on component k: every buffer of PgradLay after the call and the three outputs"""
    n, d, p, kernel = P["n"], P["d"], P["p"], P["kernel"]
    th = P["th"][k]
    ell, scale, nug, D, psi = sb.split_theta(th, d)
    L = sb.pgrad_layout(n, d, p, 1, n0)
    m, npad, ppad, n0r, nsum = L["m"], L["npad"], L["ppad"], L["n0r"], L["nsum"]
    f = _ph_fit(P, k)
    s = np.ones(n) if P["sr"] is None else P["sr"]
    x0 = _pp_x0(P, same, n0)
    xs, yv = _ph_prep(P, k, npad)
    omw = 1.0 / (1.0 + nug)
    nt, w1 = nug * omw, omw * omw
    x0l = (x0 / ell[None, :]).T
    xc = (scale / (1.0 + nug)) * _ph_c0(x0l, xs[:, :n], kernel) * s[None, :]
    X = xc.copy()
    rows = np.arange(n0)
    if same > 0:
        X[rows, rows + same - 1] += scale * nt * s[rows + same - 1]
    V = np.zeros((n0r, npad))
    V[:n0, :n] = X @ f["V"]                                  # (the library: U = X W^T, V = U W; an input of every check here)
    zp = np.concatenate([f["z"], np.zeros(npad - n)])
    rd = np.zeros((d, n0r))
    per_dim = []
    for j in range(d):
        E = _ph_da(P, k, xs, j)
        yv[j] = E @ zp
        T = V @ E
        per_dim.append((T * V).sum(axis=1))
    for j in range(d):
        rd[j] = per_dim[max(j - 1, 0)] if bug == "rd_prev" else per_dim[j]
    v, z = V[:n0, :n], f["z"]
    sums = np.zeros((n0r, nsum))
    for j0 in range(0, d, sb.PP_DB):                          # one workgroup per (row, block of PP_DB dimensions)
        for j in range(j0, min(j0 + sb.PP_DB, d)):
            lj = ell[j - sb.PP_DB] if (bug == "stale_block" and j0 > 0) else ell[j]
            t = xc * _ph_phi(np.abs(x0l[j][:, None] - xs[j][None, :n]), lj, kernel)[0]
            sums[:n0, j], sums[:n0, d + j], sums[:n0, 2 * d + 6 + j] = (t * z).sum(axis=1), (t * v).sum(axis=1), (v * yv[j, :n]).sum(axis=1)
        if j0 == 0:
            s2 = 1.0 if bug == "s2vv_no_s2" else s * s
            sums[:n0, 2 * d], sums[:n0, 2 * d + 1] = (xc * z).sum(axis=1), (xc * v).sum(axis=1)
            sums[:n0, 2 * d + 4], sums[:n0, 2 * d + 5] = (v * v).sum(axis=1), (s2 * v * v).sum(axis=1)
            sums[:n0, 3 * d + 6], sums[:n0, 3 * d + 7] = (v * yv[d, :n]).sum(axis=1), (v * yv[d + 1, :n]).sum(axis=1)
            if same > 0:
                cs = rows + same - 1 + (1 if bug == "cstar_off" else 0)
                sums[:n0, 2 * d + 2], sums[:n0, 2 * d + 3] = s[cs] * z[cs], s[cs] * v[rows, cs]
    YT = np.zeros((npad, ppad))
    YT[:n, :p] = P["Y"].T
    VY = V @ YT
    # pgrad_final_kernel
    S = sums[:n0]
    dg, dv = np.zeros((n0, m)), np.zeros((n0, m))
    dg[:, :d] = S[:, :d] - S[:, 2 * d + 6:3 * d + 6]
    dv[:, :d] = -D * (2.0 * S[:, d:2 * d] - rd[:, :n0].T)
    xcz, xcv, rz, rv, vv, s2vv = (S[:, 2 * d + c] for c in range(6))
    xz, xv = scale * nt * rz + xcz, scale * nt * rv + xcv
    dg[:, d] = xz / scale - S[:, 3 * d + 6]
    dv[:, d] = 1.0 - D * (xv + vv) / scale
    dg[:, d + 1] = (scale * w1 * rz - xcz * omw) - S[:, 3 * d + 7]
    sg = -1.0 if bug == "nug_sign" else 1.0
    dv[:, d + 1] = -D * (2.0 * (sg * scale * w1 * rv - xcv * omw) - (D * scale * s2vv - (xv - vv)) * omw)
    ps = sb.split_theta(P["th"][1 - k], d)[4] if bug == "noise_psi_other" else psi
    dn = -0.5 * ps[None, :] * VY[:n0, :p]
    return dict(xs=xs, yv=yv, E=E, V=V, T=T, rd=rd, sums=sums, YT=YT, VY=VY, dg=dg, dv=dv, dn=dn, ghat=X @ z,
                gvar=scale - D * (X * v).sum(axis=1))


def _pp_checks(P, k, e, same, n0=PH_N0, stages=PP_STAGES):
    n, d, p, th, f = P["n"], P["d"], P["p"], P["th"][k], _ph_fit(P, k)
    R = sb.hess_parts(e["xs"], P["sr"], th, P["kernel"], n)
    fns = dict(hess_prep=lambda: sb.check_hess_prep(e["xs"], e["yv"], P["x"], P["sr"], th, f["b"], f["z"]),
               hess_da=lambda: sb.check_hess_da(e["E"], R, d - 1),
               pp_y=lambda: sb.check_pp_y(e["yv"], R, f["z"]),
               pp_t=lambda: sb.check_pp_t(e["T"], e["V"], e["E"], n0, n),
               pp_rowdot=lambda: sb.check_pp_rowdot(e["rd"], e["T"], e["V"], R, n0),
               pp_sums=lambda: sb.check_pp_sums(e["sums"], _pp_x0(P, same, n0), e["xs"], f["z"], e["V"], e["yv"], P["sr"], th,
                                                P["kernel"], same, n0, n),
               pp_vy=lambda: sb.check_pp_vy(e["YT"], e["VY"], e["V"], P["Y"], n0, n),
               pp_out=lambda: sb.check_pp_out(e["dg"], e["dv"], e["dn"], e["sums"], e["rd"], e["VY"], th, d, p, n0))
    return {s: fns[s]() for s in stages}


@pytest.mark.parametrize("d", [3, 9])
@pytest.mark.parametrize("rep", [False, True], ids=["full", "rep"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_emulated_predict_paramgrad_passes_every_stage(kernel, rep, d, monkeypatch):
    """new inputs (same = 0), the training set itself (same = 1) and a middle slice of it (same = 21): every stage at or below
    1, the floor sets at most 1 % of the bounds of any stage, and the outputs agree with the dense restatement
    tests/param_grad_ref.py:latent at the bar of tests/test_param_grad_host.py (1e-12 of the largest entry per output)"""
    import types
    from tests import param_grad_ref as pref
    from tests.test_param_grad_host import EPS_REF
    P = _ph_problem(d, kernel, rep)
    log = []
    monkeypatch.setattr(sb, "FLOOR_LOG", log)
    for k, same in ((0, 0), (1, 1), (0, 21)):
        e = _pp_emulate(P, k, same)
        checks = _pp_checks(P, k, e, same)
        print(kernel, rep, d, k, same, {s: "%.2e" % c.ratio for s, c in checks.items()})
        for stage, c in checks.items():
            assert c.ratio <= 1.0, (stage, c)
        if same <= 1:
            # (on the emulation's A^-1, as in the Hessian's tie: gvar = scale - D X.V cancels to eps cond(A) of its terms)
            monkeypatch.setattr(pref, "sla", types.SimpleNamespace(cho_solve=lambda c, b, V=_ph_fit(P, k)["V"]: V))
            want = pref.latent(_pp_x0(P, same), bool(same), P["x"], P["Y"], P["sr"], P["th"][k], kernel)
            # (gvar, lcgp_predict_grad's output and none of this pass's stages, is left out: scale - D X.V cancels)
            assert _normwise_blocks((e["ghat"], e["dg"], e["dv"], e["dn"]), want[:1] + want[2:]) <= EPS_REF
    _floor_condition(log)


PP_DEFECTS = [("cstar_off", "pp_sums", 9), ("rd_prev", "pp_rowdot", 9), ("s2vv_no_s2", "pp_sums", 9), ("stale_block", "pp_sums", 17),
              ("noise_psi_other", "pp_out", 9), ("nug_sign", "pp_out", 9)]


@pytest.mark.parametrize("bug,stage,d", PP_DEFECTS)
def test_predict_paramgrad_defect_fails_its_stage_and_none_upstream(bug, stage, d):
    """the replicated path, a middle slice of the training set (same = 21): c* one column off, rd of dimension j - 1, sum s^2 V^2
    without s^2, the second PP_DB block (d = 17) with the first block's lengthscales, dghat_noise with psi of the other component,
    d_nug gvar with the wrong sign on the nugget term"""
    P = _ph_problem(d, "matern32", True)
    checks = _pp_checks(P, 0, _pp_emulate(P, 0, 21, bug), 21)
    print(bug, {s: "%.2e" % c.ratio for s, c in checks.items()})
    _stage_only(PP_STAGES, checks, stage)


def test_predict_paramgrad_gap_small_dgvar_column_is_invisible_normwise():
    """one lengthscale 50 times longer than the others: its dgvar column is small, and off by 1e-6 relative it stays within the
    1e-10 of max|err| / max|ref| of tests/test_gpu_param_grad.py while check_pp_out fails at that column"""
    base = _ph_problem(9, "matern32", False)
    P = dict(base, th=base["th"].copy(), fit={})
    P["th"][:, 0] *= 50.0
    e = _pp_emulate(P, 0, 0)
    assert all(c.ratio <= 1.0 for c in _pp_checks(P, 0, e, 0).values())
    bad = e["dv"].copy()
    bad[:, 0] *= 1.0 + 1e-6
    nw = np.max(np.abs(bad - e["dv"])) / np.max(np.abs(e["dv"]))
    print("dgvar column 0: max %.3e of %.3e, normwise %.3e (bar 1e-10)" % (np.max(np.abs(e["dv"][:, 0])), np.max(np.abs(e["dv"])), nw))
    assert 0 < nw <= 1e-10
    c = _pp_checks(P, 0, dict(e, dv=bad), 0, stages=("pp_out",))["pp_out"]
    assert c.ratio > 1.0 and c.where[:2] == ("dgvar", 0), c
