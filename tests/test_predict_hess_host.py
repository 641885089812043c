"""CPU tests of the input Hessians of the prediction (LCGP.predict_hess / predict_differentiable(order=2)): the host layer --
unpacking of the packed lower triangles, chain rule to the raw input and output scales through _output_map, full and rep
paths, the three kernels, the second-order autograd wrapper -- through a numpy stand-in of HotPathEngine.predict_hess_block
built from the oracle's kernels and dense solves, against central differences of the stand-in's predict_grad; and the C
entries of the library (tests/test_gpu_predict_hess.py runs the same through liblcgp_hip.so on the GPU)."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from lcgp_amd import LCGP, synth
from lcgp_amd import dist as _dist
from oracle import lcgp_oracle as orc
from tests import matern52_oracle as m52
from tests.test_predict_grad_host import LO, SPAN, GradOracleEngine


def _cross(x0s, x, ell, scale, nug, kernel):
    """the cross covariance without nugget term (x0s is not the training set), any of the three kernels"""
    if kernel == 'matern52':
        return m52.kernel_matrix(x0s, x, ell, scale, nug, same=False)
    return orc.matern32(x0s, x, ell, scale, nug, kernel=kernel)


def latent_hessians(x0s, x, sr, th, low, z, kernel):
    """float64 numpy restatement for one component: ghat, gvar (n0), Jm, Jv (n0, d), Hm, Hv (n0, d, d) with respect to the
    standardised x0s.  With c the cross covariance, s = (x0s - x) / ell, a = |s|, V = (c o sr) A^-1, u = L^-1 (d_l X)^T:
        d_l c = -c h(s_l) / ell_l,   d2_lm c = c h(s_l) h(s_m) / (ell_l ell_m)  (l != m),   d2_ll c = c psi(s_l) / ell_l^2
        Hm[i, l, m] = sum_j d2_lm c sr_j z_j,   Hv[i, l, m] = -2 D (sum_j d2_lm c sr_j V[i, j] + u_il . u_im)"""
    d = x.shape[1]
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    c = _cross(x0s, x, ell, scale, nug, kernel)
    s = (x0s[:, None, :] - x[None, :, :]) / ell                     # (n0, n, d) signed scaled distances
    a = np.abs(s)
    if kernel == 'matern32':
        h, psi = s / (1.0 + a), -(1.0 - a) / (1.0 + a)
    elif kernel == 'se':
        h, psi = s, s * s - 1.0
    else:
        assert kernel == 'matern52'
        h, psi = s * (1.0 + a) / (3.0 + 3.0 * a + a * a), -(1.0 + a - a * a) / (3.0 + 3.0 * a + a * a)
    dc = -c[:, :, None] * h / ell                                   # (n0, n, d)
    kap = h[:, :, :, None] * h[:, :, None, :]
    idx = np.arange(d)
    kap[:, :, idx, idx] = psi
    d2c = c[:, :, None, None] * kap / (ell[:, None] * ell[None, :])  # (n0, n, d, d)
    X = c * sr[None, :]
    V = sla.cho_solve((low, True), X.T).T
    u = sla.solve_triangular(low, X.T, lower=True)
    gh, gv = X @ z, scale - D * np.sum(u * u, axis=0)
    jm = np.einsum('ijl,j->il', dc, sr * z)
    jv = -2.0 * D * np.einsum('ijl,ij->il', dc, sr[None, :] * V)
    n0 = x0s.shape[0]
    dX = (dc * sr[None, :, None]).transpose(0, 2, 1).reshape(n0 * d, -1)        # row i d + l
    P = sla.solve_triangular(low, dX.T, lower=True).T.reshape(n0, d, -1)
    hm = np.einsum('ijlm,j->ilm', d2c, sr * z)
    hv = -2.0 * D * (np.einsum('ijlm,ij->ilm', d2c, sr[None, :] * V) + np.einsum('ilj,imj->ilm', P, P))
    return gh, gv, jm, jv, hm, hv


def pack_lower(h):
    """(..., d, d) -> (..., d (d + 1) / 2): entry (l, m <= l) at l (l + 1) / 2 + m"""
    il, im = np.tril_indices(h.shape[-1])
    return h[..., il, im]


class HessOracleEngine(GradOracleEngine):
    """GradOracleEngine plus predict_hess_block, in numpy float64; Matern-5/2 through tests/matern52_oracle.py"""

    def evaluate(self, theta_rows):
        if self.kernel == 'matern52':
            with m52.patched():
                return super().evaluate(theta_rows)
        return super().evaluate(theta_rows)

    def _all(self, x0s):
        x0s = np.asarray(x0s, np.float64)
        sr = np.ones(self.n) if self.sr is None else self.sr
        return [latent_hessians(x0s, self.x, sr, th, low, z, self.kernel) for th, low, z, b in self._state]

    def predict(self, x0s, same=False):
        if self.kernel != 'matern52':
            return super().predict(x0s, same)
        assert not same
        res = self._all(x0s)
        return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])

    def predict_grad_block(self, x0s):
        if self.kernel != 'matern52':
            return super().predict_grad_block(x0s)          # the tested first-order restatement
        res = self._all(x0s)
        return (torch.as_tensor(np.stack([[r[0] for r in res], [r[1] for r in res]])),
                torch.as_tensor(np.stack([[r[2] for r in res], [r[3] for r in res]])))

    def predict_hess_block(self, x0s):
        blk, jac = self.predict_grad_block(x0s)
        res = self._all(x0s)
        hess = np.stack([[pack_lower(r[4]) for r in res], [pack_lower(r[5]) for r in res]])
        return blk, jac, torch.as_tensor(hess)


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


def _model(mode, kernel='matern32', **kw):
    """model through the stand-in and its raw training inputs; p = 3 outputs, q = 2 components, non-unit input ranges"""
    if mode == 'full':
        x, y = synth.make_full(71, 40, 2, 3, 2)
    else:
        x, y = synth.make_rep(72, 16, 3, 2, 3, 2)
    x = LO + SPAN * x
    m = patch_engine(LCGP(y=y, x=x, q=2, submethod=mode, kernel=kernel, **kw))
    o = orc.OracleLCGP(y=y, x=x, q=2, submethod=mode, **kw)         # (only for the shape of the parameter vector)
    m._set_flat(synth.param_points(71, o.get_unconstrained())[1])
    assert int(m.p) == 3 and int(m.q) == 2
    return m, x


def central_differences_of_predict_grad(m, x0, h):
    """(3, p, n0, d, d): [..., l, c] = d/dx0[i, c] of predict_grad's [..., l], every row perturbed at once"""
    n0, d = x0.shape
    out = np.zeros((3, int(m.p), n0, d, d))
    for c in range(d):
        e = np.zeros_like(x0)
        e[:, c] = h[c]
        plus, minus = m.predict_grad(x0 + e), m.predict_grad(x0 - e)
        for w in range(3):
            out[w, ..., c] = (plus[w].numpy() - minus[w].numpy()) / (2 * h[c])
    return out


def assert_clear_of_kinks(x0, x, h):
    """Matern-3/2: psi has a kink where a coordinate of x0 equals a training input's; a central difference across it is
    wrong to O(step), so every |x0_il - x_jl| is at least two steps"""
    gap = np.min(np.abs(x0[:, None, :] - x[None, :, :]) / h)
    assert gap >= 2.0, gap


@pytest.mark.parametrize('mode,kw', [('full', {}), ('rep', {}), ('rep', {'rep_standardize_ybar': False}),
                                     ('full', {'kernel': 'se'}), ('full', {'kernel': 'matern52'})])
def test_predict_hess_equals_central_differences_of_predict_grad(mode, kw):
    kw = dict(kw)
    kernel = kw.pop('kernel', 'matern32')
    m, x = _model(mode, kernel, **kw)
    x0 = LO + SPAN * np.random.default_rng(4).uniform(0.05, 0.95, (11, 2))
    h = 1e-5 * SPAN
    if kernel == 'matern32':
        assert_clear_of_kinks(x0, x, h)
    got = [t.numpy() for t in m.predict_hess(x0)]
    for g in got:
        assert g.shape == (3, 11, 2, 2) and g.dtype == np.float64
        assert np.array_equal(g, np.swapaxes(g, -1, -2))            # exactly symmetric
    np.testing.assert_array_equal(got[1], got[2])                   # the noise variance does not depend on x0
    fd = central_differences_of_predict_grad(m, x0, h)
    for g, f in zip(got, fd):
        err = np.max(np.abs(g - f))
        print(mode, kernel, err / np.max(np.abs(f)))
        assert err <= 1e-6 * np.max(np.abs(f)), (err, np.max(np.abs(f)))
    assert m.d2ghat.shape == m.d2gvar.shape == (2, 11, 2, 2)
    assert m.dghat.shape == (2, 11, 2) and m.ghat.shape == (2, 11)


def test_latent_hessians_are_the_engine_block_and_chain_through_the_output_map():
    m, x = _model('rep')
    x0 = LO + SPAN * np.random.default_rng(5).uniform(0.1, 0.9, (6, 2))
    d2yp, d2ypv, d2ycv = [t.numpy() for t in m.predict_hess(x0)]
    assert m._local_ks == [0, 1]
    x0s, _ = m._standardise_x0(x0)
    blk, jac, hess = m._get_engine().predict_hess_block(x0s)
    assert blk.shape == (2, 2, 6) and jac.shape == (2, 2, 6, 2) and hess.shape == (2, 2, 6, 3)
    for full, packed in ((m.d2ghat.numpy(), hess[0].numpy()), (m.d2gvar.numpy(), hess[1].numpy())):
        assert full.shape == (2, 6, 2, 2) and m.d2ghat.dtype == torch.float64
        np.testing.assert_array_equal(pack_lower(full), packed)
        np.testing.assert_array_equal(full, np.swapaxes(full, -1, -2))
    np.testing.assert_array_equal(m.dghat.numpy(), jac[0].numpy())
    np.testing.assert_array_equal(m.ghat.numpy(), blk[0].numpy())
    W, _, scale, _ = m._output_map()
    rng = (m.x_max - m.x_min).numpy().reshape(-1)          # the standardisation's range, not SPAN itself
    rr = rng[:, None] * rng[None, :]
    want = np.einsum('ka,kilm->ailm', W, m.d2ghat.numpy()) * scale[:, None, None, None] / rr
    np.testing.assert_allclose(d2yp, want, rtol=1e-13, atol=0)
    want = np.einsum('ka,kilm->ailm', W ** 2, m.d2gvar.numpy()) * (scale ** 2)[:, None, None, None] / rr
    np.testing.assert_allclose(d2ycv, want, rtol=1e-13, atol=0)
    np.testing.assert_array_equal(d2ypv, d2ycv)


@pytest.mark.parametrize('kernel', ['matern32', 'matern52'])
def test_order_two_gradgradcheck_and_hessian(kernel):
    m, x = _model('full', kernel)
    x0 = LO + SPAN * np.random.default_rng(6).uniform(0.1, 0.9, (4, 2))
    assert_clear_of_kinks(x0, x, 1e-6 * np.ones(2))                # gradgradcheck's step
    outs = m.predict_differentiable(torch.as_tensor(x0), order=2)
    for a, b in zip(outs, m.predict(x0)):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    xt = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
    for which in range(3):
        fn = lambda t: m.predict_differentiable(t, order=2)[which]          # noqa: E731
        assert torch.autograd.gradcheck(fn, (xt,), eps=1e-6, atol=1e-7, rtol=1e-5)
        assert torch.autograd.gradgradcheck(fn, (xt,), eps=1e-6, atol=1e-6, rtol=1e-4)
    want = m.predict_hess(x0)
    for which in (0, 2):
        for a in range(3):
            H = torch.autograd.functional.hessian(lambda t: m.predict_differentiable(t, order=2)[which][a].sum(), xt)
            assert H.shape == (4, 2, 4, 2)
            for i in range(4):
                for j in range(4):
                    blk = want[which][a, i] if i == j else torch.zeros(2, 2, dtype=torch.float64)
                    torch.testing.assert_close(H[i, :, j, :], blk, rtol=1e-13, atol=0)
    # a first-order use of order=2 equals order=1
    (g2,) = torch.autograd.grad(m.predict_differentiable(xt, order=2)[0].sum(), xt)
    (g1,) = torch.autograd.grad(m.predict_differentiable(xt, order=1)[0].sum(), xt)
    assert torch.equal(g1, g2) and not g2.requires_grad


def test_order_one_still_refuses_double_backward_and_third_order_is_refused():
    m, x = _model('full')
    xt = torch.tensor(LO + SPAN * np.array([[0.3, 0.6], [0.7, 0.2]]), requires_grad=True)
    with pytest.raises(RuntimeError, match='double backward'):
        torch.autograd.grad(m.predict_differentiable(xt)[0].sum(), xt, create_graph=True)
    with pytest.raises(RuntimeError, match='double backward'):
        torch.autograd.grad(m.predict_differentiable(xt, order=1)[0].sum(), xt, create_graph=True)
    (g,) = torch.autograd.grad(m.predict_differentiable(xt, order=2)[0].sum(), xt, create_graph=True)
    assert g.requires_grad
    (gg,) = torch.autograd.grad(g.pow(2).sum(), xt)                # a plain double backward works
    assert gg.shape == xt.shape and torch.all(torch.isfinite(gg))
    (g,) = torch.autograd.grad(m.predict_differentiable(xt, order=2)[0].sum(), xt, create_graph=True)
    with pytest.raises(RuntimeError, match='triple backward'):
        torch.autograd.grad(g.pow(2).sum(), xt, create_graph=True)
    with pytest.raises(ValueError, match='order'):
        m.predict_differentiable(xt, order=3)


def test_c_abi_of_the_hessian_entry():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() >= 580
    for name in ('lcgp_predict_hess', 'lcgp_predict_hess_scratch_bytes'):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    nb = C.c_size_t(0)
    # n = 1000 -> npad 1024; n0 = 100 -> 128 rows of X and of U; n0 d = 300 -> 384 rows of dX and of P; q = 2, float64
    assert lib.lcgp_predict_hess_scratch_bytes(0, 1000, 3, 2, 100, C.byref(nb)) == 0
    assert nb.value == 2 * 2 * (128 + 384) * 1024 * 8
    assert lib.lcgp_predict_hess_scratch_bytes(1, 1000, 1, 2, 50, C.byref(nb)) == 0
    assert nb.value == 2 * 2 * (64 + 64) * 1024 * 4
    assert lib.lcgp_predict_hess_scratch_bytes(2, 1000, 3, 2, 100, C.byref(nb)) < 0
    assert b'dtype' in lib.lcgp_last_error()
    assert lib.lcgp_predict_hess_scratch_bytes(0, 1000, 127, 2, 100, C.byref(nb)) < 0
    assert b'd must be' in lib.lcgp_last_error()
    assert lib.lcgp_predict_hess_scratch_bytes(0, 1000, 100, 2, 50000, C.byref(nb)) < 0
    assert b'n0 * d' in lib.lcgp_last_error()
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything
    head = (dummy, None, dummy, dummy)                              # x, sr, theta, workspace
    outs = (dummy,) * 6

    def call(dtype=0, kern=0, d=2, n0=10, x0=dummy, scratch=dummy, outs=outs, stride=0):
        return lib.lcgp_predict_hess(None, dtype, kern, 100, d, 3, 1, *head, n0, x0, scratch, *outs, stride)

    assert call(dtype=2) < 0 and b'dtype' in lib.lcgp_last_error()
    assert call(kern=7) < 0 and b'kernel_id' in lib.lcgp_last_error()
    assert call(d=127) < 0 and b'd must be' in lib.lcgp_last_error()
    assert call(d=0) < 0 and b'd must be' in lib.lcgp_last_error()
    assert call(n0=0) < 0 and b'n0' in lib.lcgp_last_error()
    assert call(d=100, n0=50000) < 0 and b'n0 * d' in lib.lcgp_last_error()
    for miss in range(6):
        o = tuple(None if i == miss else dummy for i in range(6))
        assert call(outs=o) < 0 and b'NULL' in lib.lcgp_last_error(), miss
    assert call(x0=None) < 0 and b'NULL' in lib.lcgp_last_error()
    assert call(scratch=None) < 0 and b'NULL' in lib.lcgp_last_error()
    assert call(stride=5) < 0 and b'out_stride' in lib.lcgp_last_error()
