"""CPU tests of the input gradients of the prediction (LCGP.predict_grad / predict_differentiable): the host layer -- chain
rule to the raw input and output scales through _output_map, full and rep paths, p != q, the autograd wrapper -- through a
numpy stand-in of HotPathEngine.predict_grad_block built from the oracle's kernel and dense solves, against central
differences of the oracle's predict; and the C entries of the library (tests/test_gpu_predict_grad.py runs the same through
liblcgp_hip.so on the GPU)."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from lcgp_amd import LCGP, synth
from lcgp_amd import dist as _dist
from oracle import lcgp_oracle as orc
from tests.helpers import OracleEngine


def latent_jacobians(x0s, x, sr, th, low, z, kernel):
    """float64 numpy restatement for one component: ghat, gvar (n0) and Jm, Jv (n0, d) with respect to the standardised x0s,
        Jm[i, l] = sum_j dc_l(i, j) sr_j z_j,   Jv[i, l] = -2 D sum_j dc_l(i, j) sr_j V[i, j],   V = (c o sr) A^-1
    with c from the oracle's kernel (no nugget: x0s is not the training set) and A^-1 from the factor `low`"""
    d = x.shape[1]
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    c = orc.matern32(x0s, x, ell, scale, nug, kernel=kernel)
    s = (x0s[:, None, :] - x[None, :, :]) / ell                     # (n0, n, d) signed scaled distances
    h = s / (1.0 + np.abs(s)) if kernel == 'matern32' else s
    dc = -c[:, :, None] * h / ell                                   # d c / d x0s_l
    X = c * sr[None, :]
    V = sla.cho_solve((low, True), X.T).T
    u = sla.solve_triangular(low, X.T, lower=True)
    gh, gv = X @ z, scale - D * np.sum(u * u, axis=0)
    jm = np.einsum('ijl,j->il', dc, sr * z)
    jv = -2.0 * D * np.einsum('ijl,ij->il', dc, sr[None, :] * V)
    return gh, gv, jm, jv


class GradOracleEngine(OracleEngine):
    """OracleEngine plus predict_grad_block, in numpy float64"""

    def predict_grad_block(self, x0s):
        x0s = np.asarray(x0s, np.float64)
        n0, d = x0s.shape
        sr = np.ones(self.n) if self.sr is None else self.sr
        blk = np.zeros((2, self.q_local, n0))
        jac = np.zeros((2, self.q_local, n0, d))
        for i, (th, low, z, b) in enumerate(self._state):
            gh, gv, jm, jv = latent_jacobians(x0s, self.x, sr, th, low, z, self.kernel)
            blk[0, i], blk[1, i], jac[0, i], jac[1, i] = gh, gv, jm, jv
        # ghat / gvar exactly as predict_block(same=False) forms them (the GPU entry point shares predict's launches)
        blk[0], blk[1] = self.predict(x0s, False)
        return torch.as_tensor(blk), torch.as_tensor(jac)


def patch_engine(model):
    """this file's copy of tests.helpers.patch_engine, installing GradOracleEngine"""
    def _make(dtype=None):
        rank, world = _dist.rank_world(model._group)
        model._local_ks = _dist.local_components(model.q, rank, world)
        if not model._local_ks:
            return None
        if model.submethod == 'rep':
            sr = np.sqrt(model.r.numpy().astype(float))
            yb = (model.ybar_s if model.rep_standardize_ybar else model.ybar).numpy()
            return GradOracleEngine(model.x_unique_s.numpy(), yb * sr[None, :], sr, len(model._local_ks),
                                    comp_ids=model._local_ks, q_total=model.q, kernel=model.kernel)
        return GradOracleEngine(model.x.numpy(), model.y.numpy(), None, len(model._local_ks),
                                comp_ids=model._local_ks, q_total=model.q, kernel=model.kernel)
    model._make_engine = _make
    return model


LO, SPAN = np.array([1.0, -2.0]), np.array([3.0, 0.5])           # a non-unit input range, different per dimension


def _pair(mode, kernel='matern32', **kw):
    """(model through the stand-in, oracle at the same parameters, raw training inputs); p = 3 outputs, q = 2 components"""
    if mode == 'full':
        x, y = synth.make_full(71, 40, 2, 3, 2)
    else:
        x, y = synth.make_rep(72, 16, 3, 2, 3, 2)
    x = LO + SPAN * x
    m = patch_engine(LCGP(y=y, x=x, q=2, submethod=mode, kernel=kernel, **kw))
    o = orc.OracleLCGP(y=y, x=x, q=2, submethod=mode, kernel=kernel, **kw)
    o.phi = m.phi.numpy().copy()
    u = synth.param_points(71, o.get_unconstrained())[1]
    m._set_flat(u)
    o.set_unconstrained(u)
    assert int(m.p) == 3 and int(m.q) == 2
    return m, o, x


def _central_differences(o, x0, h):
    """(3, p, n0, d): d/dx0[i, l] of the oracle's (ypred, ypredvar, yconfvar), every row perturbed at once (row i of the
    outputs depends on row i of x0 only)"""
    n0, d = x0.shape
    out = None
    for l in range(d):
        e = np.zeros_like(x0)
        e[:, l] = h[l]
        o._aux = None
        plus = o.predict(x0 + e)
        o._aux = None
        minus = o.predict(x0 - e)
        diff = np.stack([(a - b) / (2 * h[l]) for a, b in zip(plus[:3], minus[:3])])
        if out is None:
            out = np.zeros(diff.shape + (d,))
        out[..., l] = diff
    return out


@pytest.mark.parametrize('mode,kw', [('full', {}), ('rep', {}), ('rep', {'rep_standardize_ybar': False}),
                                     ('full', {'kernel': 'se'})])
def test_predict_grad_equals_central_differences_of_the_oracle(mode, kw):
    kernel = kw.pop('kernel', 'matern32')
    m, o, x = _pair(mode, kernel, **kw)
    x0 = LO + SPAN * np.random.default_rng(4).uniform(0.05, 0.95, (11, 2))
    dyp, dypv, dycv = [t.numpy() for t in m.predict_grad(x0)]
    assert dyp.shape == dypv.shape == dycv.shape == (3, 11, 2)
    assert dyp.dtype == np.float64
    fd = _central_differences(o, x0, 1e-5 * SPAN)
    for got, want in zip((dyp, dypv, dycv), fd):
        assert np.max(np.abs(got - want)) <= 1e-6 * np.max(np.abs(want)), (np.max(np.abs(got - want)), np.max(np.abs(want)))
    np.testing.assert_array_equal(dypv, dycv)           # the noise variance does not depend on x0
    assert m.dghat.shape == m.dgvar.shape == (2, 11, 2)
    assert m.ghat.shape == (2, 11)


def test_latent_jacobians_are_kept_and_chain_through_the_output_map():
    m, o, x = _pair('full')
    x0 = LO + SPAN * np.random.default_rng(5).uniform(0.1, 0.9, (6, 2))
    dyp, _, dycv = [t.numpy() for t in m.predict_grad(x0)]
    W, _, scale, _ = m._output_map()
    rng = (m.x_max - m.x_min).numpy().reshape(-1)          # the standardisation's range, not SPAN itself
    want = np.einsum('ka,kil->ail', W, m.dghat.numpy()) * scale[:, None, None] / rng
    np.testing.assert_allclose(dyp, want, rtol=1e-13, atol=0)
    want = np.einsum('ka,kil->ail', W ** 2, m.dgvar.numpy()) * (scale ** 2)[:, None, None] / rng
    np.testing.assert_allclose(dycv, want, rtol=1e-13, atol=0)


def test_gradient_at_training_inputs_is_that_of_the_continuous_surface():
    """at a training input the nugget is a point mass (added only when x0 IS the training set): the gradient there is the
    limit of the gradients around it"""
    m, o, x = _pair('full')
    x0 = x[:3]
    near = x0 + 1e-7 * SPAN
    a = m.predict_grad(x0)[0].numpy()
    b = m.predict_grad(near)[0].numpy()
    assert np.max(np.abs(a - b)) <= 1e-4 * np.max(np.abs(a))


@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_predict_differentiable_forward_equals_predict_and_passes_gradcheck(mode):
    m, o, x = _pair(mode)
    x0 = LO + SPAN * np.random.default_rng(6).uniform(0.1, 0.9, (5, 2))
    outs = m.predict_differentiable(torch.as_tensor(x0))
    ref = m.predict(x0)
    for a, b in zip(outs, ref):
        assert not a.requires_grad
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    xt = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
    for which in range(3):
        assert torch.autograd.gradcheck(lambda t: m.predict_differentiable(t)[which], (xt,), eps=1e-6, atol=1e-7, rtol=1e-5)
    yp, ypv, ycv = m.predict_differentiable(xt)
    (yp.sum() + (ypv * ycv).sum()).backward()
    assert xt.grad.shape == xt.shape and torch.all(torch.isfinite(xt.grad))


def test_predict_differentiable_refuses_double_backward_and_keeps_predict_detached():
    m, o, x = _pair('full')
    xt = torch.tensor(LO + SPAN * np.array([[0.3, 0.6], [0.7, 0.2]]), requires_grad=True)
    yp = m.predict_differentiable(xt)[0]
    assert yp.requires_grad
    with pytest.raises(RuntimeError, match='double backward'):
        torch.autograd.grad(yp.sum(), xt, create_graph=True)
    (g,) = torch.autograd.grad(m.predict_differentiable(xt)[0].sum(), xt)
    assert g.shape == xt.shape and not g.requires_grad
    assert not any(t.requires_grad for t in m.predict(xt) if t is not None)


def test_latent_jacobians_on_the_model_are_the_engine_block():
    """the (q, n0, d) latent Jacobians kept as dghat / dgvar are the engine's block, unpacked from the one gathered row per
    component (tests/test_gpu_predict_grad.py checks two ranks against one on the GPU)"""
    m, o, x = _pair('rep')
    x0 = LO + SPAN * np.random.default_rng(8).uniform(0.1, 0.9, (4, 2))
    want = [t.numpy() for t in m.predict_grad(x0)]
    assert m._local_ks == [0, 1]
    x0s, _ = m._standardise_x0(x0)
    blk, jac = m._get_engine().predict_grad_block(x0s)
    assert blk.shape == (2, 2, 4) and jac.shape == (2, 2, 4, 2)
    np.testing.assert_array_equal(m.dghat.numpy(), jac[0].numpy())
    np.testing.assert_array_equal(m.dgvar.numpy(), jac[1].numpy())
    np.testing.assert_array_equal(want[0].shape, (3, 4, 2))


def test_c_abi_argument_checks_of_the_gradient_entry():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() >= 530
    for name in ('lcgp_predict_grad', 'lcgp_predict_grad_scratch_bytes'):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    nb, nb2 = C.c_size_t(0), C.c_size_t(0)
    assert lib.lcgp_predict_grad_scratch_bytes(0, 1000, 2, 100, C.byref(nb)) == 0
    assert lib.lcgp_predict_scratch_bytes(0, 1000, 2, 100, C.byref(nb2)) == 0
    assert nb.value == nb2.value == 2 * 2 * 128 * 1024 * 8
    assert lib.lcgp_predict_grad_scratch_bytes(2, 1000, 2, 100, C.byref(nb)) < 0
    assert b'dtype' in lib.lcgp_last_error()
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything
    args = (None, 0, 0, 100, 2, 3, 1, dummy, None, dummy, dummy)
    assert lib.lcgp_predict_grad(*args, 0, dummy, dummy, dummy, dummy, dummy, dummy, 0) < 0
    assert b'n0' in lib.lcgp_last_error()
    assert lib.lcgp_predict_grad(*args, 10, dummy, dummy, dummy, dummy, None, dummy, 0) < 0
    assert b'NULL' in lib.lcgp_last_error()
    assert lib.lcgp_predict_grad(*args, 10, dummy, dummy, dummy, dummy, dummy, dummy, 5) < 0
    assert b'out_stride' in lib.lcgp_last_error()
    assert lib.lcgp_predict_grad(None, 0, 7, 100, 2, 3, 1, dummy, None, dummy, dummy, 10, dummy, dummy, dummy, dummy, dummy,
                                 dummy, 0) < 0
    assert b'kernel_id' in lib.lcgp_last_error()
    assert lib.lcgp_predict_grad(None, 0, 0, 100, 127, 3, 1, dummy, None, dummy, dummy, 10, dummy, dummy, dummy, dummy, dummy,
                                 dummy, 0) < 0
    assert b'd must be' in lib.lcgp_last_error()
