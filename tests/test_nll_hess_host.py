"""CPU tests of the Hessian of the objective in the parameters (LCGP.loss_hessian / LCGP.laplace): the torch restatement of the
objective (tests/nll_hess_ref.py) against the oracle, its autograd Hessian against central differences of the oracle's analytic
gradient, a plain-numpy implementation of the closed-form blocks lcgp_nll_hess computes against autograd, the SoftClip second
derivative, the constrained -> unconstrained map, laplace() through a numpy stand-in of the engine, and the C entries of the
library (tests/test_gpu_nll_hess.py runs the same through liblcgp_hip.so on the GPU).

eps_ref -- the largest deviation of the numpy closed form from autograd, max |H - H_ref| / max |H_ref| per block type, measured
on the shapes below (n = 150 / 50 x 3, d = 2, p = 4, q = 2; and d = 1, and the error structure [1, 3]):
    kernel block 2.3e-15, border 2.2e-15, noise corner 5.5e-16, over the three kernels, full and rep.
Central differences take the step 1e-5 max(1, |c_i|): a step relative to the VALUE of a nugget of 5e-5 is 5e-10, where the
rounding of the oracle's gradient divided by the step (1e-7 of the largest entry and growing as the step shrinks) is all that
is left of the comparison; with this step the differences agree with autograd to 7e-9.
The GPU test's bound is 10 x max(eps_ref, 1e-12) = 1e-11."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from lcgp_amd import LCGP, synth
from lcgp_amd import dist as _dist
from lcgp_amd.params import SoftClip, softclip_flat2
from oracle import lcgp_oracle as orc
from tests import matern52_oracle as m52
from tests import nll_hess_ref as ref
from tests.helpers import OracleEngine

EPS_REF = 1e-14            # asserted for the closed form below; measured: see the module docstring


# ---------------------------------------------------------------------------------------------------------------------------
# the closed form of the issue in plain numpy: what lcgp_nll_hess computes, per component
# ---------------------------------------------------------------------------------------------------------------------------
def phi_and_dphi(S, ell, kernel):
    """phi = d log C0 / d ell and d phi / d ell of one dimension at S = |dx| / ell"""
    if kernel == 'matern32':
        return S * S / ((1.0 + S) * ell), -S * S * (3.0 + 2.0 * S) / ((1.0 + S) ** 2 * ell * ell)
    if kernel == 'se':
        return S * S / ell, -3.0 * S * S / (ell * ell)
    assert kernel == 'matern52'
    q = 3.0 + 3.0 * S + S * S
    N = S * S * (1.0 + S)
    return N / (ell * q), -(S * S * (2.0 + 3.0 * S) / q + N * (3.0 - S * S) / q ** 2) / (ell * ell)


def component_blocks(x, Y, sr, th, kernel):
    """(hk (m, m), hx (m, p), hn (p, p)) of one component from its theta row [ell | scale | nug | D | psi], m = d + 2:
        hk[i, j] = 1/2 sum (A^-1 o d_ijA) - 1/2 tr(G_i G_j) - z^T d_ijA z / (2 D) + y_i^T A^-1 y_j / D
        hx[i, a] = c_a^T A^-1 y_i / (2 D)
        hn[a, b] = -[ delta_ab c_a^T (b - z) + c_a^T (I - A^-1) c_b ] / (4 D)"""
    n, d = x.shape
    ell, scale, nug, D, psi = th[:d], th[d], th[d + 1], th[d + 2], th[d + 3:]
    s = np.ones(n) if sr is None else np.asarray(sr, np.float64)
    a = x / ell
    S = np.abs(a.T[:, :, None] - a.T[:, None, :])                      # (d, n, n)
    if kernel == 'se':
        c0 = np.exp(-0.5 * (S * S).sum(axis=0))
    elif kernel == 'matern32':
        c0 = np.prod(1.0 + S, axis=0) * np.exp(-S.sum(axis=0))
    else:
        c0 = np.prod(1.0 + S + S * S / 3.0, axis=0) * np.exp(-S.sum(axis=0))
    w, w1, w2 = nug / (1.0 + nug), 1.0 / (1.0 + nug) ** 2, -2.0 / (1.0 + nug) ** 3
    eye = np.eye(n)
    ss = s[:, None] * s[None, :]
    A = eye + D * ss * scale * ((1.0 - w) * c0 + w * eye)
    ainv = sla.cho_solve((np.linalg.cholesky(A), True), eye)
    b = Y.T @ psi
    z = ainv @ b
    ph, dph = np.empty((d, n, n)), np.empty((d, n, n))
    for i in range(d):
        ph[i], dph[i] = phi_and_dphi(S[i], ell[i], kernel)
    m = d + 2
    dA = np.empty((m, n, n))
    for i in range(d):
        dA[i] = D * ss * scale * (1.0 - w) * c0 * ph[i]
    dA[d] = (A - eye) / scale
    dA[d + 1] = D * ss * scale * w1 * (eye - c0)
    G = np.stack([ainv @ dA[i] for i in range(m)])
    yv = np.stack([dA[i] @ z for i in range(m)])
    uv = yv @ ainv
    gmat = ss * (0.5 * D * ainv - 0.5 * np.outer(z, z))               # 1/2 sum A^-1 o d_ijA - z^T d_ijA z / (2 D) = sum gmat o d_ijC
    T = np.zeros((m, m))
    for i in range(d):
        for j in range(i + 1):
            T[i, j] = T[j, i] = np.sum(gmat * scale * (1.0 - w) * c0 * (ph[i] * ph[j] + (dph[i] if i == j else 0.0)))
        T[i, d] = T[d, i] = np.sum(gmat * (1.0 - w) * c0 * ph[i])
        T[i, d + 1] = T[d + 1, i] = -np.sum(gmat * scale * w1 * c0 * ph[i])
    T[d, d + 1] = T[d + 1, d] = w1 * np.sum(gmat * (eye - c0))
    T[d + 1, d + 1] = scale * w2 * np.sum(gmat * (eye - c0))
    hk = np.empty((m, m))
    for i in range(m):
        for j in range(m):
            hk[i, j] = T[i, j] - 0.5 * np.sum(G[i] * G[j].T) + yv[i] @ uv[j] / D
    cm = psi[:, None] * Y
    hx = (uv @ cm.T) / (2.0 * D)
    hn = -(np.diag(cm @ (b - z)) + cm @ (cm - cm @ ainv).T) / (4.0 * D)
    return hk, hx, hn


class HessOracleEngine(OracleEngine):
    """OracleEngine plus nll_hess_block: the rows of lcgp_nll_hess from the numpy closed form"""

    def nll_hess_block(self):
        rows = []
        for th, _, _, _ in self._state:
            rows.append(np.concatenate([blk.reshape(-1) for blk in component_blocks(self.x, self.Y, self.sr, th, self.kernel)]))
        return torch.as_tensor(np.stack(rows))


def patch_engine(model):
    """this file's copy of tests.helpers.patch_engine, installing HessOracleEngine"""
    def _make(dtype=None):
        rank, world = _dist.rank_world(model._group)
        model._local_ks = _dist.local_components(model.q, rank, world)
        if not model._local_ks:
            return None
        if model.submethod == 'rep':
            sr = np.sqrt(model.r.numpy().astype(float))
            yb = (model.ybar_s if model.rep_standardize_ybar else model.ybar).numpy()
            return HessOracleEngine(model.x_unique_s.numpy(), yb * sr[None, :], sr, len(model._local_ks),
                                    comp_ids=model._local_ks, q_total=model.q, kernel=model.kernel)
        return HessOracleEngine(model.x.numpy(), model.y.numpy(), None, len(model._local_ks),
                                comp_ids=model._local_ks, q_total=model.q, kernel=model.kernel)
    model._make_engine = _make
    return model


CASES = [('full', 'matern32', {}), ('rep', 'matern32', {}), ('full', 'se', {}), ('rep', 'se', {}), ('full', 'matern52', {}),
         ('rep', 'matern52', {}), ('full', 'matern32', {'d': 1}), ('full', 'matern32', {'diag_error_structure': [1, 3]})]
_cache = {}
NFULL, NREP = 150, 50


def _case(mode, kernel, kw):
    """(model through the stand-in, oracle, flat unconstrained point, reference problem, autograd Hessian), built once per case"""
    key = (mode, kernel, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _cache:
        kw = dict(kw)
        d = kw.pop('d', 2)
        x, y = synth.make_full(7, NFULL, d, 4, 2) if mode == "full" else synth.make_rep(7, NREP, 3, d, 4, 2)
        with m52.patched():
            o = orc.OracleLCGP(y=y, x=x, q=2, submethod=mode, kernel=kernel, **kw)
            m = patch_engine(LCGP(y=y, x=x, q=2, submethod=mode, kernel=kernel, **kw))
            o.phi = m.phi.numpy().copy()
            u = synth.param_points(7, o.get_unconstrained())[1]
            o.set_unconstrained(u)
            val, g = o._value_and_constrained_grad(True)
        gflat = np.concatenate([g['lLmb'].reshape(-1), g['lLmb0'], g['lnugGPs'], g['lsigma2s']])
        prob = ref.problem(o)
        H = ref.hessian(ref.flat_constrained(o), prob)
        H.setflags(write=False)
        _cache[key] = (m, o, u, prob, H, val, gflat)
    return _cache[key]


@pytest.mark.parametrize('mode,kernel,kw', CASES)
def test_restatement_matches_the_oracle_in_value_and_gradient(mode, kernel, kw):
    m, o, u, prob, H, val, gflat = _case(mode, kernel, kw)
    v, g = ref.value_and_grad(ref.flat_constrained(o), prob)
    ev, eg = abs(v - val) / abs(val), np.max(np.abs(g - gflat)) / np.max(np.abs(gflat))
    print('value %.2e gradient %.2e' % (ev, eg))
    assert ev <= 1e-12 and eg <= 1e-12


@pytest.mark.parametrize('mode,kernel,kw', CASES)
def test_autograd_hessian_matches_central_differences_of_the_oracle_gradient(mode, kernel, kw):
    m, o, u, prob, H, _, _ = _case(mode, kernel, kw)
    c = ref.flat_constrained(o)
    q, d = prob['q'], prob['d']

    def grad_at(cv):
        a = q * d
        with m52.patched():
            if mode == 'full':
                _, g = orc.nll_grad_full_chol(o.x, o.y, o.phi, o.diag_D, o.diag_error_structure, cv[:a].reshape(q, d), cv[a:a + q],
                                              cv[a + 2 * q:], cv[a + q:a + 2 * q], kernel=kernel)
            else:
                yb = o.ybar_s if o.rep_standardize_ybar else o.ybar
                _, g = orc.nll_grad_rep_chol(o.x_unique_s, yb, o.ybar_std, o.rep_standardize_ybar, o.r, o.phi, o.diag_D,
                                             o.diag_error_structure, cv[:a].reshape(q, d), cv[a:a + q], cv[a + 2 * q:],
                                             cv[a + q:a + 2 * q], kernel=kernel)
        return np.concatenate([g['lLmb'].reshape(-1), g['lLmb0'], g['lnugGPs'], g['lsigma2s']])

    fd = np.empty_like(H)
    for i in range(len(c)):
        h = 1e-5 * max(1.0, abs(c[i]))
        e = np.zeros_like(c)
        e[i] = h
        fd[:, i] = (grad_at(c + e) - grad_at(c - e)) / (2.0 * h)
    err = np.max(np.abs(H - fd)) / np.max(np.abs(H))
    sym = np.max(np.abs(H - H.T)) / np.max(np.abs(H))
    print('autograd vs central differences %.2e, asymmetry %.2e' % (err, sym))
    assert err <= 1e-7 and sym <= 1e-13
    idx = ref.kernel_index(q, d)
    assert np.all(H[np.ix_(idx[0], idx[1])] == 0.0)          # kernel blocks of different components: exactly zero


@pytest.mark.parametrize('mode,kernel,kw', CASES)
def test_numpy_closed_form_matches_autograd(mode, kernel, kw):
    """the formulas lcgp_nll_hess implements, assembled by LCGP.loss_hessian(space='constrained') through the stand-in"""
    m, o, u, prob, H, _, _ = _case(mode, kernel, kw)
    Hc = m.loss_hessian(u, space='constrained')
    assert Hc.shape == H.shape and Hc.dtype == np.float64
    errs = ref.block_errors(Hc, H, prob['q'], prob['d'])
    print('eps_ref', errs)
    assert max(errs.values()) <= EPS_REF
    np.testing.assert_array_equal(Hc, Hc.T)
    idx = ref.kernel_index(prob['q'], prob['d'])
    assert np.all(Hc[np.ix_(idx[0], idx[1])] == 0.0)
    assert m._aux_valid


def test_softclip_second_derivative_matches_central_differences_of_dforward():
    for lo, hi in ((1e-6, 1e4), (1e-10, 1e4), (-2.0, 3.0)):
        tr = SoftClip(lo, hi)
        u = np.concatenate([np.linspace(lo - 8.0, lo + 8.0, 41), np.linspace(hi - 8.0, hi + 8.0, 41)]) if hi - lo > 100 \
            else np.linspace(lo - 6.0, hi + 6.0, 61)
        h = 1e-5
        fd = (tr.dforward(u + h) - tr.dforward(u - h)) / (2.0 * h)
        got = tr.d2forward(u)
        assert np.max(np.abs(got - fd)) <= 1e-8 * max(1.0, np.max(np.abs(fd)))
        w = np.full_like(u, hi - lo)
        j, j2 = softclip_flat2(u, np.full_like(u, lo), np.full_like(u, hi), w, np.full_like(u, tr._c))
        np.testing.assert_array_equal(j, tr.dforward(u))
        np.testing.assert_array_equal(j2, got)


@pytest.mark.parametrize('mode,kernel,kw', [CASES[0], CASES[1], CASES[7]])
def test_unconstrained_hessian_matches_autograd_through_the_transform(mode, kernel, kw):
    m, o, u, prob, H, _, _ = _case(mode, kernel, kw)
    q, d = prob['q'], prob['d']
    bounds = [orc.LLMB_BOUNDS] * (q * d) + [orc.LLMB0_BOUNDS] * q + [orc.LNUG_BOUNDS] * q
    lo = torch.tensor([b[0] for b in bounds], dtype=torch.float64)
    hi = torch.tensor([b[1] for b in bounds], dtype=torch.float64)
    sp = torch.nn.functional.softplus

    def through(uv):
        nb = len(bounds)
        w = hi - lo
        c = hi - w / sp(w) * sp(w - sp(uv[:nb] - lo))
        return ref.objective(torch.cat([c, uv[nb:]]), prob)

    want = torch.autograd.functional.hessian(through, torch.tensor(u)).numpy()
    got = m.loss_hessian(u)                                  # space='unconstrained' is the default
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print('unconstrained vs autograd through the transform %.2e' % err)
    assert err <= 1e-12
    np.testing.assert_array_equal(got, got.T)


def test_a_replaced_transform_without_second_derivative_raises():
    m = _case(*CASES[0])[0]

    class Exp:
        low, high = 0.0, np.inf
        forward = staticmethod(np.exp)
        inverse = staticmethod(np.log)
        dforward = staticmethod(np.exp)

    keep = m.lLmb0.transform
    m.lLmb0.transform = Exp()
    try:
        with pytest.raises(NotImplementedError, match='d2forward'):
            m.loss_hessian()
    finally:
        m.lLmb0.transform = keep


def test_loss_hessian_exists_and_refuses_an_unknown_space():
    m = _case(*CASES[0])[0]
    with pytest.raises(ValueError, match='space'):
        m.loss_hessian(space='natural')


def test_laplace_on_the_stand_in():
    x, y = synth.make_full(3, 60, 2, 4, 2)
    m = patch_engine(LCGP(y=y, x=x, q=2, diag_error_structure=[1, 3]))
    m.fit()
    res = m.laplace()
    print('eigenvalues %.3e .. %.3e' % (res.eigenvalues[0], res.eigenvalues[-1]))
    P = m._get_flat().size
    assert res.hessian.shape == res.cov.shape == (P, P) and res.eigenvalues.shape == (P,)
    assert np.all(res.eigenvalues > 0) and np.all(np.diff(res.eigenvalues) >= 0)
    # (the fit leaves a nugget near its lower bound: cond(H) ~ 1e8, so H^-1 H = I to eps cond(H) ~ 2e-8; two orders of margin)
    assert np.max(np.abs(res.cov @ res.hessian - np.eye(P))) <= 1e-6
    np.testing.assert_array_equal(res.cov, res.cov.T)
    for se, par in zip(res.stderr, m.get_param()):
        assert tuple(se.shape) == tuple(par.shape) and bool(torch.all(se > 0))
    # the delta method: |d forward / d u| sqrt(diag cov), lsigma2s repeated over its groups
    sd = np.sqrt(np.diag(res.cov))
    q, d = 2, 2
    np.testing.assert_allclose(res.stderr[0].numpy(), (m.lLmb.transform.dforward(m.lLmb.unconstrained) * sd[:q * d].reshape(q, d)),
                               rtol=1e-14)
    np.testing.assert_allclose(res.stderr[2].numpy(), np.repeat(sd[q * d + 2 * q:], [1, 3]), rtol=1e-14)
    np.testing.assert_allclose(res.stderr[3].numpy(), m.lnugGPs.transform.dforward(m.lnugGPs.unconstrained) * sd[q * d + q:q * d + 2 * q],
                               rtol=1e-14)
    # away from the optimum the Hessian is indefinite: LinAlgError naming the smallest eigenvalue, nothing jittered
    u = m._get_flat().copy()
    u[:q * d] -= 3.0
    m._set_flat(u)
    ev = np.linalg.eigvalsh(m.loss_hessian())
    assert ev[0] < 0
    with pytest.raises(np.linalg.LinAlgError, match='smallest eigenvalue -'):
        m.laplace()


def test_c_abi_of_the_hessian_entries():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() >= 600
    for name in ('lcgp_nll_hess', 'lcgp_nll_hess_scratch_bytes', 'lcgp_nll_hess_width'):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    assert lib.lcgp_nll_hess_width(6, 64) == 8 * 8 + 8 * 64 + 64 * 64
    nb = C.c_size_t(0)
    # n = 1000 -> npad 1024; d = 3: A^-1, d_iA and 5 G_i per component
    assert lib.lcgp_nll_hess_scratch_bytes(0, 1000, 3, 5, 2, C.byref(nb)) == 0
    assert 2 * 7 * 1024 * 1024 * 8 <= nb.value <= 2 * 7 * 1024 * 1024 * 8 * 1.05
    assert lib.lcgp_nll_hess_scratch_bytes(1, 1000, 3, 5, 2, C.byref(nb)) < 0
    assert b'float64 only' in lib.lcgp_last_error()
    assert lib.lcgp_nll_hess_scratch_bytes(0, 1000, 127, 5, 2, C.byref(nb)) < 0
    assert b'd must be' in lib.lcgp_last_error()
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything

    def call(dtype=0, kern=0, d=2, k0=0, qg=1, x=dummy, scratch=dummy, out=dummy):
        return lib.lcgp_nll_hess(None, dtype, kern, 100, d, 3, 2, x, dummy, None, dummy, dummy, k0, qg, scratch, out)

    assert call(dtype=1) < 0 and b'float64 only' in lib.lcgp_last_error()
    assert call(dtype=2) < 0 and b'dtype' in lib.lcgp_last_error()
    assert call(kern=7) < 0 and b'kernel_id' in lib.lcgp_last_error()
    assert call(d=127) < 0 and b'd must be' in lib.lcgp_last_error()
    assert call(k0=1, qg=2) < 0 and b'q_group' in lib.lcgp_last_error()
    assert call(qg=0) < 0 and b'q_group' in lib.lcgp_last_error()
    assert call(x=None) < 0 and b'NULL' in lib.lcgp_last_error()
    assert call(scratch=None) < 0 and b'NULL' in lib.lcgp_last_error()
    assert call(out=None) < 0 and b'NULL' in lib.lcgp_last_error()
