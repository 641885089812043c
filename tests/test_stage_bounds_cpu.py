"""The stage bounds of tests/stage_bounds.py have teeth (no GPU): an emulated path -- float64 stages, and float32 stages
emulated by rounding each stage's float64 result -- passes every check with a ratio far below 1, and each of the defects
the GPU tests are meant to catch (a perturbed tile, a missing panel update, a stale tile, a tile left out of a product, a
wrong tile in the gradient contraction, a poor pivot) fails the check of its stage.  The first defect also leaves the
end-to-end NLL within the 1e-6 parity bar: the bar the rest of the suite uses cannot see it.

The joint path (X, U, Sigma + tau I, its factor, the draws) gets the same treatment on an emulated path with q = 3
components: a perturbed tile of Sigma, a K-tile left out of D U U^T, tau of the wrong component, a draw through an
upper triangle that was not zeroed, draws shifted at a chunk split and a float32-accurate Sigma each fail their check."""
import numpy as np
import pytest
import torch

from tests import stage_bounds as sb

N, D_IN, P = 300, 3, 4
TS = sb.TS


def _problem(seed=0, ell=(0.3, 0.5, 0.8), n=N):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (n, D_IN))
    Y = rng.standard_normal((P, n))
    th = np.concatenate([np.asarray(ell, np.float64), [1.3, 0.01, 5.0], rng.standard_normal(P)])
    return x, Y, th


def _r(a, dtype):
    return sb.rounded(a, dtype)


def _emulate(x, Y, th, dtype, kernel="matern32"):
    """every stage computed in float64 from the previous stage's stored result and rounded to the storage type"""
    A = _r(sb.reference_A(x, None, th, kernel, dtype)[0].numpy(), dtype)
    L = _r(np.linalg.cholesky(A), dtype)
    W = _r(np.linalg.solve(L, np.eye(x.shape[0])), dtype)
    W = np.tril(W)
    V = _r(W.T @ W, dtype)
    psi = th[D_IN + 3:]
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


@pytest.mark.parametrize("kernel", ["matern32", "se"])
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
