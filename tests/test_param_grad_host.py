"""CPU tests of the parameter derivatives of the prediction (LCGP.predict_param_grad / predict_laplace, the host side of
lcgp_predict_paramgrad): the numpy restatement of the latent formulas and the host map against torch autograd of a torch
restatement of predict(), that restatement against the oracle, central differences of OracleLCGP.predict, the pure host map on
random latent Jacobians, predict_laplace's assembly on a stub latent pass, and the C ABI of the two new entries.

Bound of the restatement: 1e-12 of the largest entry per block.  Measured here (float64, n = 40): at most 3e-14 over all cases."""
import ctypes as C

import numpy as np
import pytest
import torch

import lcgp_amd.lcgp as lcgp_mod
from lcgp_amd import LCGP, synth
from oracle import lcgp_oracle as orc
from tests import matern52_oracle as m52
from tests import param_grad_ref as ref

EPS_REF = 1e-12
N, N0, D, P, Q = 40, 7, 2, 4, 3
CASES = [(mode, kernel, es) for mode in ('full', 'rep') for kernel in ('matern32', 'se', 'matern52') for es in (None,)] + \
        [('full', 'matern32', [1, 3]), ('rep', 'matern52', [2, 2])]
_cache = {}


def _case(mode, kernel, es):
    """(model on the stand-in engine, oracle, flat unconstrained point, torch problem), built once per case"""
    key = (mode, kernel, None if es is None else tuple(es))
    if key not in _cache:
        x, y = synth.make_full(11, N, D, P, Q) if mode == 'full' else synth.make_rep(11, N, 2, D, P, Q)
        kw = dict(q=Q, submethod=mode, kernel=kernel, diag_error_structure=es)
        with m52.patched():
            o = orc.OracleLCGP(y=y, x=x, **kw)
            m = ref.patch_engine(LCGP(y=y, x=x, **kw))
            o.phi = m.phi.numpy().copy()
            u = synth.param_points(11, o.get_unconstrained())[1]
            o.set_unconstrained(u)
        m._set_flat(u)
        _cache[key] = (m, o, u, ref.problem(o), x)
    return _cache[key]


def _x0(m, x, same):
    """raw-scale new inputs: the training set (same) or N0 points inside its box, two of them training inputs"""
    xtr = np.asarray(m.x_unique.numpy() if m.submethod == 'rep' else m.x_orig.numpy()) if same else None
    if same:
        return xtr
    lo, hi = x.min(axis=0), x.max(axis=0)
    x0 = lo + (hi - lo) * np.random.default_rng(5).uniform(0.05, 0.95, (N0, x.shape[1]))
    x0[:2] = x[[0, 3]]
    return x0


def _rel(got, want):
    return float(np.max(np.abs(np.asarray(got) - want)) / np.max(np.abs(want)))


@pytest.mark.parametrize('same', [False, True])
@pytest.mark.parametrize('mode,kernel,es', CASES)
def test_restatement_and_host_map_match_autograd(mode, kernel, es, same):
    m, o, u, pr, x = _case(mode, kernel, es)
    x0 = _x0(m, x, same)
    x0s, same_found = m._standardise_x0(x0)
    assert same_found == same
    with m52.patched():
        want_val = o.predict(x0)
        got = m.predict_param_grad(x0, space='constrained')
    c = ref.flat_constrained(o)
    vals = ref.predict(torch.as_tensor(c), pr, torch.as_tensor(x0s), same)
    # the torch restatement IS the oracle's predict: two routes through the factorisation, apart by cond(A) eps -- the
    # project's first-order bar of 1e-10 on the full path; the oracle's rep path forms the explicit inverse and subtracts
    # (c0 T) . c0 from the prior, which loses cond(A) eps once more: 1e-8 there
    for v, w in zip(vals, want_val[:3]):
        assert _rel(v.numpy(), np.asarray(w)) <= (1e-8 if mode == 'rep' else 1e-10)
    want = ref.jacobians(c, pr, x0s, same)
    for g, w, what in zip(got, want, ('dypred', 'dypredvar', 'dyconfvar')):
        assert tuple(g.shape) == w.shape == (P, len(x0), len(u))
        print(mode, kernel, es, same, what, _rel(g.numpy(), w))
        assert _rel(g.numpy(), w) <= EPS_REF, what
    # the unconstrained space: the chain rule with d constrained / d unconstrained
    jac = m._flat_jacobians()[0]
    for g, w in zip(m.predict_param_grad(x0), want):
        assert _rel(g.numpy(), w * jac) <= EPS_REF
    # latent=True: the components' own Jacobians, zero in the other components' kernel parameters
    lg, lv = (a.numpy() for a in m.predict_param_grad(x0, space='constrained', latent=True))
    W, _, scale, _ = m._output_map()
    o_ = Q * (D + 2)
    assert _rel(np.einsum('ka,kip->aip', W, lg[:, :, :o_]) * scale[:, None, None], want[0][:, :, :o_]) <= EPS_REF
    assert np.all(lv[:, :, o_:] == 0.0)
    for k in range(Q):
        other = np.setdiff1d(np.arange(o_), np.r_[k * D + np.arange(D), Q * D + k, Q * D + Q + k])
        assert np.all(lg[k][:, other] == 0.0) and np.all(lv[k][:, other] == 0.0)


@pytest.mark.parametrize('mode,es', [('full', None), ('rep', None), ('full', [1, 3])])
def test_central_differences_of_the_oracle_predict(mode, es):
    """step 1e-5 max(1, |u_i|); bound: 10 x the error the torch restatement's OWN central differences have at that step against
    its autograd Jacobian.  The oracle's rep path evaluates predict() through the explicit inverse, whose rounding noise (its
    distance from the Cholesky restatement, two references, measured here) divided by 2 h enters its differences on top of
    that: there the bound is 10 x (own error + noise / (2 h_min) relative to the largest entry)."""
    m, o, u, pr, x = _case(mode, 'matern32', es)
    x0 = _x0(m, x, False)
    x0s = torch.as_tensor(m._standardise_x0(x0)[0])
    got = [g.numpy() for g in m.predict_param_grad(x0)]
    jac = m._flat_jacobians()[0]
    auto = [w * jac for w in ref.jacobians(ref.flat_constrained(o), pr, x0s.numpy(), False)]
    fd_o, fd_r = [np.empty_like(g) for g in got], [np.empty_like(g) for g in got]
    noise = [0.0, 0.0, 0.0]
    try:
        for i in range(len(u)):
            h = 1e-5 * max(1.0, abs(u[i]))
            e = np.zeros_like(u)
            e[i] = h
            sides = []
            for sgn in (1.0, -1.0):
                o.set_unconstrained(u + sgn * e)
                with torch.no_grad():
                    sides.append(([np.asarray(v) for v in o.predict(x0)[:3]],
                                  [v.numpy() for v in ref.predict(torch.as_tensor(ref.flat_constrained(o)), pr, x0s, False)]))
            for b in range(3):
                noise[b] = max(noise[b], max(float(np.max(np.abs(sd[0][b] - sd[1][b]))) for sd in sides))
                fd_o[b][:, :, i] = (sides[0][0][b] - sides[1][0][b]) / (2.0 * h)
                fd_r[b][:, :, i] = (sides[0][1][b] - sides[1][1][b]) / (2.0 * h)
    finally:
        o.set_unconstrained(u)
    for b, what in enumerate(('dypred', 'dypredvar', 'dyconfvar')):
        own = _rel(fd_r[b], auto[b])
        err = _rel(got[b], fd_o[b])
        if mode == 'rep':
            own += noise[b] / (2.0 * 1e-5) / float(np.max(np.abs(auto[b])))
        print(mode, es, what, 'own central-difference error %.2e, predict_param_grad vs oracle differences %.2e' % (own, err))
        assert err <= 10.0 * own, what


@pytest.mark.parametrize('rep', [False, True])
@pytest.mark.parametrize('es', [[1, 1, 1, 1, 1], [2, 3], [1, 3, 1]])
def test_pure_host_map_against_autograd_of_the_same_map(es, rep):
    """random latent Jacobians; the latent values are made LINEAR in the parameters with exactly those Jacobians, W and the
    noise keep their true dependence on the noise parameters: autograd of that map must give param_jacobians"""
    rng = np.random.default_rng(len(es) + 10 * rep)
    q, d, p, n0 = 3, 2, 5, 6
    m_, ns = d + 2, len(es)
    Pn = q * m_ + ns
    g0, v0 = rng.normal(size=(q, n0)), rng.uniform(0.5, 2.0, (q, n0))
    dg, dv, dn = rng.normal(size=(q, n0, m_)), rng.normal(size=(q, n0, m_)), rng.normal(size=(q, n0, p))
    phi, ls2 = rng.normal(size=(p, q)), rng.normal(size=ns)
    scale = rng.uniform(0.5, 2.0, p)
    offset = rng.normal(size=p)
    jac = rng.uniform(0.2, 1.5, Pn)
    T = torch.as_tensor
    esr = torch.as_tensor(es)

    def maps(ls2b):
        if rep:                                                 # LCGP._output_map(), rep path: the output scale divides W
            return (T(phi) * (torch.exp(0.5 * ls2b) / T(scale))[:, None]).T, torch.exp(ls2b) / T(scale) ** 2
        return T(phi).T * torch.exp(0.5 * ls2b), torch.exp(ls2b)

    c0 = np.concatenate([rng.normal(size=q * m_), ls2])

    def f(u):
        c = T(c0) + T(jac) * u                                  # constrained = linear in the "unconstrained" u, slope jac
        ls2b = torch.repeat_interleave(c[q * m_:], esr)
        dlt = torch.repeat_interleave(c[q * m_:] - T(ls2), esr)
        gh, gv = [], []
        for k in range(q):
            th = torch.cat([c[k * d:(k + 1) * d], c[q * d + k:q * d + k + 1], c[q * d + q + k:q * d + q + k + 1]]) - \
                T(np.r_[c0[k * d:(k + 1) * d], c0[q * d + k], c0[q * d + q + k]])
            gh.append(T(g0[k]) + T(dg[k]) @ th + T(dn[k]) @ dlt)
            gv.append(T(v0[k]) + T(dv[k]) @ th)
        gh, gv = torch.stack(gh), torch.stack(gv)
        W, noise = maps(ls2b)
        conf = (W ** 2).T @ gv
        sc = T(scale)
        return (W.T @ gh) * sc[:, None] + T(offset)[:, None], (conf + noise[:, None]) * (sc ** 2)[:, None], conf * (sc ** 2)[:, None]

    want = [j.numpy() for j in torch.autograd.functional.jacobian(f, torch.zeros(Pn, dtype=torch.float64))]
    W, noise = (a.numpy() for a in maps(torch.repeat_interleave(T(ls2), esr)))
    got_u = lcgp_mod.param_jacobians(g0, v0, dg, dv, dn, W, noise, scale, offset, es, jac)
    got_c = lcgp_mod.param_jacobians(g0, v0, dg, dv, dn, W, noise, scale, offset, es, None)
    for gu, gc, w in zip(got_u, got_c, want):
        assert gu.shape == (p, n0, Pn)
        assert _rel(gu, w) <= 1e-13 and _rel(gc, w / jac) <= 1e-13
    np.testing.assert_array_equal(lcgp_mod.param_jacobians(g0, v0, dg, dv, dn, W, noise, scale, offset, es, jac, mean_only=True), got_u[0])
    lg, lv = lcgp_mod.param_jacobians(g0, v0, dg, dv, dn, W, noise, scale, offset, es, jac, latent=True)
    assert lg.shape == lv.shape == (q, n0, Pn)
    assert _rel(np.einsum('ka,kip->aip', W, lg[:, :, :q * m_]) * scale[:, None, None], want[0][:, :, :q * m_]) <= 1e-13


def test_predict_laplace_assembly_on_a_stub_latent_pass(monkeypatch):
    m, o, u, pr, x = _case('full', 'matern32', [1, 3])
    rng = np.random.default_rng(3)
    n0, Pn = 23, len(u)
    stub = (rng.normal(size=(Q, n0)), rng.uniform(0.5, 2, (Q, n0)), rng.normal(size=(Q, n0, D + 2)), rng.normal(size=(Q, n0, D + 2)),
            rng.normal(size=(Q, n0, P)))
    base = tuple(torch.as_tensor(rng.uniform(1, 2, (P, n0))) for _ in range(3))
    monkeypatch.setattr(m, '_latent_param_grad', lambda x0: stub)
    monkeypatch.setattr(m, 'predict', lambda x0: base)
    monkeypatch.setattr(lcgp_mod, 'LAPLACE_CHUNK', 5)            # five passes, the last one ragged
    B = rng.normal(size=(Pn, Pn))
    cov = B @ B.T
    J = m.predict_param_grad(None)[0].numpy()
    dense = np.einsum('aip,pq,aiq->ai', J, cov, J)
    yp, ypv, ycv, pv = m.predict_laplace(None, cov=cov)
    assert yp is base[0]
    assert _rel(pv.numpy(), dense) <= 1e-13 and np.all(pv.numpy() >= 0)
    np.testing.assert_array_equal(ypv.numpy(), base[1].numpy() + pv.numpy())
    np.testing.assert_array_equal(ycv.numpy(), base[2].numpy() + pv.numpy())
    # cov = None: laplace().cov
    monkeypatch.setattr(m, 'laplace', lambda: lcgp_mod.LaplaceResult(None, None, 2.0 * cov, None))
    assert _rel(m.predict_laplace(None)[3].numpy(), 2.0 * dense) <= 1e-13
    with pytest.raises(ValueError, match='cov must be'):
        m.predict_laplace(None, cov=np.eye(3))

    def indefinite():
        raise np.linalg.LinAlgError('the Hessian of the objective is not positive definite at the current parameters: smallest eigenvalue -1')
    monkeypatch.setattr(m, 'laplace', indefinite)
    with pytest.raises(np.linalg.LinAlgError, match='smallest eigenvalue -'):
        m.predict_laplace(None)
    with pytest.raises(ValueError, match='space'):
        m.predict_param_grad(None, space='natural')


def test_c_abi_of_the_paramgrad_entries():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() == 610
    for name in ('lcgp_predict_paramgrad', 'lcgp_predict_paramgrad_scratch_bytes'):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    nb = C.c_size_t(0)
    # n = 1000 -> npad 1024, n0 = 200 -> 256 rows: X / V, U / T_j and d_jA per component
    assert lib.lcgp_predict_paramgrad_scratch_bytes(0, 1000, 3, 5, 2, 200, C.byref(nb)) == 0
    mats = 2 * (2 * 256 * 1024 + 1024 * 1024) * 8
    assert mats <= nb.value <= 1.1 * mats
    assert lib.lcgp_predict_paramgrad_scratch_bytes(1, 1000, 3, 5, 2, 200, C.byref(nb)) < 0
    assert b'float64 only' in lib.lcgp_last_error()
    assert lib.lcgp_predict_paramgrad_scratch_bytes(0, 1000, 127, 5, 2, 200, C.byref(nb)) < 0
    assert b'd must be' in lib.lcgp_last_error()
    assert lib.lcgp_predict_paramgrad_scratch_bytes(0, 1000, 3, 5, 2, 0, C.byref(nb)) < 0
    assert b'n0' in lib.lcgp_last_error()
    assert lib.lcgp_predict_paramgrad_scratch_bytes(0, 1000, 3, 5, 2, 200, None) < 0
    assert b'NULL' in lib.lcgp_last_error()
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything

    def call(dtype=0, kern=0, d=2, k0=0, qg=1, n0=10, same=0, x=dummy, x0=dummy, scratch=dummy, out=dummy, stride=0):
        return lib.lcgp_predict_paramgrad(None, dtype, kern, 100, d, 3, 2, x, dummy, None, dummy, dummy, k0, qg, n0, x0, same, scratch,
                                          dummy, dummy, dummy, dummy, out, stride)

    assert call(dtype=1) < 0 and b'float64 only' in lib.lcgp_last_error()
    assert call(dtype=2) < 0 and b'dtype' in lib.lcgp_last_error()
    assert call(kern=7) < 0 and b'kernel_id' in lib.lcgp_last_error()
    assert call(d=127) < 0 and b'd must be' in lib.lcgp_last_error()
    assert call(k0=1, qg=2) < 0 and b'q_group' in lib.lcgp_last_error()
    assert call(n0=0) < 0 and b'n0' in lib.lcgp_last_error()
    assert call(same=95) < 0 and b'same' in lib.lcgp_last_error()
    assert call(stride=5) < 0 and b'out_stride' in lib.lcgp_last_error()
    for kw in ({'x': None}, {'x0': None}, {'scratch': None}, {'out': None}):
        assert call(**kw) < 0 and b'NULL' in lib.lcgp_last_error()
