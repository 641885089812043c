"""Pins the Matern-5/2 helper oracle (tests/matern52_oracle.py) by identities, as tests/test_oracle_identities.py pins 'se',
and checks the host side of the C ABI for LCGP_KERNEL_MATERN52.

PARITY UNPINNED: the reference has no Matern-5/2 kernel.  The committed oracle cannot learn one (its kernel switches fall
through to Matern-3/2 for unknown names), so the helper patches the three kernel-specific functions; these tests tie that
helper to the definition and to itself: closed-form gradient = central finite differences, eigendecomposition form =
Cholesky form, replicated literal form = Cholesky form, kernel value = the textbook Matern-5/2 at lengthscale sqrt(5) ell."""
import ctypes as C

import numpy as np
import pytest

from lcgp_amd import synth
from oracle import lcgp_oracle as orc
from tests import matern52_oracle as m52
from tests.test_oracle_identities import _fd_grad, _full_model, _rep_model


@pytest.fixture
def oracle52(monkeypatch):
    m52.patch(monkeypatch)
    return orc


def test_kernel_value_is_the_textbook_matern52_at_sqrt5_ell():
    rng = np.random.default_rng(3)
    a, b = rng.uniform(size=(7, 3)), rng.uniform(size=(5, 3))
    ell = np.array([0.6, 1.1, 0.3])
    r = np.abs(a[:, None, :] - b[None, :, :])
    lt = np.sqrt(5.0) * ell                                   # textbook lengthscale
    t = np.sqrt(5.0) * r / lt
    textbook = np.prod((1.0 + t + t * t / 3.0) * np.exp(-t), axis=2)      # (1 + sqrt5 r/l + 5 r^2 / (3 l^2)) exp(-sqrt5 r/l)
    want = 1.7 * (1 - 0.02 / 1.02) * textbook
    np.testing.assert_allclose(m52.matern32(a, b, ell, 1.7, 0.02, kernel='matern52'), want, rtol=1e-14)
    same = m52.matern32(a, a, ell, 1.7, 0.02, kernel='matern52')
    np.testing.assert_allclose(np.diag(same), 1.7, rtol=1e-14)            # (1 - nt) + nt on the diagonal
    np.testing.assert_allclose(m52.matern32(a, a, ell, 1.7, 0.02, diag_only=True, kernel='matern52'), 1.7)
    # the other names are the oracle's own
    for kernel in ('matern32', 'se'):
        np.testing.assert_array_equal(m52.matern32(a, b, ell, 1.7, 0.02, kernel=kernel),
                                      orc.matern32(a, b, ell, 1.7, 0.02, kernel=kernel))
    c0, s_all = m52.matern32_c0_and_s(a, ell, 'matern52')
    np.testing.assert_allclose(s_all, np.abs(a[:, None, :] - a[None, :, :]).transpose(2, 0, 1) / ell[:, None, None], rtol=1e-13,
                               atol=1e-15)      # (|a - b| / ell against |a / ell - b / ell|: a few ulps)
    np.testing.assert_allclose(1.7 * ((1 - 0.02 / 1.02) * c0 + 0.02 / 1.02 * np.eye(7)), same, rtol=1e-14)


def test_lengthscale_derivative_weight_matches_central_differences():
    rng = np.random.default_rng(5)
    a = rng.uniform(size=(9, 3))
    ell = np.array([0.6, 1.1, 0.3])
    c0, s_all = m52.matern32_c0_and_s(a, ell, 'matern52')
    for j in range(3):
        h = 1e-6 * ell[j]
        e = np.zeros(3)
        e[j] = h
        fd = (m52.matern32_c0_and_s(a, ell + e, 'matern52')[0] - m52.matern32_c0_and_s(a, ell - e, 'matern52')[0]) / (2 * h)
        s = s_all[j]
        np.testing.assert_allclose(c0 * s * s * (1 + s) / ((3 + 3 * s + s * s) * ell[j]), fd, rtol=1e-7, atol=1e-9)


def test_the_patch_is_in_force_and_is_undone(monkeypatch):
    """the unpatched oracle silently computes Matern-3/2 for kernel='matern52': a test that forgot to patch must not pass"""
    m = _full_model(kernel='matern52')
    m32 = _full_model()
    u = synth.param_points(11, m.get_unconstrained())[1]
    m.set_unconstrained(u)
    m32.set_unconstrained(u)
    unpatched = m.loss()
    assert unpatched == m32.loss()
    with m52.patched():
        patched = m.loss()
    assert abs(patched - m32.loss()) > 1e-3 * abs(m32.loss())
    assert m.loss() == unpatched                     # restored
    m52.patch(monkeypatch)
    assert m.loss() == patched


def test_eigh_form_equals_cholesky_form(oracle52):
    m = _full_model(diag_error_structure=[2, 1, 1], kernel='matern52')
    for u in synth.param_points(11, m.get_unconstrained()):
        m.set_unconstrained(u)
        a, b = m.loss_reference_form(), m.loss()
        assert abs(a - b) <= 1e-11 * max(1.0, abs(a))


def test_rep_literal_equals_cholesky_form(oracle52):
    for use_std in (True, False):
        m = _rep_model(rep_standardize_ybar=use_std, kernel='matern52')
        for u in synth.param_points(12, m.get_unconstrained()):
            m.set_unconstrained(u)
            a, b = m.loss_reference_form(), m.loss()
            assert abs(a - b) <= 1e-10 * max(1.0, abs(a))


@pytest.mark.parametrize("kind", ["full", "full_grouped", "rep_std", "rep_raw"])
def test_closed_form_gradient_matches_finite_differences(oracle52, kind):
    if kind == "full":
        m = _full_model(kernel='matern52')
    elif kind == "full_grouped":
        m = _full_model(diag_error_structure=[1, 3], robust_mean=False, kernel='matern52')
    elif kind == "rep_std":
        m = _rep_model(kernel='matern52')
    else:
        m = _rep_model(rep_standardize_ybar=False, kernel='matern52')
    m32 = _full_model() if kind == "full" else None
    for u in synth.param_points(14, m.get_unconstrained(), count=2):
        val, g = m.loss_and_grad_unconstrained(u)
        assert abs(val - m.loss()) < 1e-12 * max(1, abs(val))
        if m32 is not None:             # (guards against a fixture that did not patch)
            v32, _ = m32.loss_and_grad_unconstrained(u)
            assert abs(val - v32) > 1e-3 * abs(v32)
        fd = _fd_grad(m, u)
        np.testing.assert_allclose(g, fd, rtol=2e-5, atol=2e-6 * max(1.0, np.max(np.abs(fd))))


def test_gradient_matches_torch_autograd_of_literal_form(oracle52):
    """Independent check: autograd through the eigendecomposition form with the kernel written out in torch."""
    torch = pytest.importorskip("torch")
    m = _full_model(n=40, kernel='matern52')
    u = synth.param_points(15, m.get_unconstrained())[1]
    _, g = m.loss_and_grad_unconstrained(u)
    lLmb, lLmb0, ls2b, lnug = m.get_param()
    t = dict(l=torch.tensor(lLmb, requires_grad=True), s=torch.tensor(lLmb0, requires_grad=True),
             v=torch.tensor(lnug, requires_grad=True), e=torch.tensor(np.asarray(m.lsigma2s), requires_grad=True))
    x, y, phi, n = torch.tensor(m.x), torch.tensor(m.y), torch.tensor(m.phi), m.n
    psi_c = phi.T / torch.sqrt(torch.exp(t['e']))
    nlp = 0.0
    for k in range(m.q):
        a = x / t['l'][k]
        S = (a[:, None, :] - a[None, :, :]).abs()
        c0 = torch.prod(1 + S + S * S / 3, dim=2) * torch.exp(-S.sum(dim=2))
        nt = t['v'][k] / (1 + t['v'][k])
        ck = t['s'][k] * ((1 - nt) * c0 + nt * torch.eye(n, dtype=torch.float64))
        wk, uk = torch.linalg.eigh(ck)
        qk = uk @ torch.diag(1 / (m.diag_D[k] + 1 / wk)) @ uk.T
        nlp = nlp + 0.5 * torch.sum(torch.log(1 + m.diag_D[k] * wk))
        nlp = nlp - 0.5 * torch.sum((y @ qk) * (torch.outer(psi_c[k], psi_c[k]) @ y))
    nlp = nlp + n / 2 * t['e'].sum() + 0.5 * torch.sum((y.T / torch.sqrt(torch.exp(t['e']))) ** 2)
    nlp.backward()
    u1, u2, u3, _ = m._split(u)
    ref = np.concatenate([
        (t['l'].grad.numpy() * orc.softclip_grad(u1, *orc.LLMB_BOUNDS)).reshape(-1),
        t['s'].grad.numpy() * orc.softclip_grad(u2, *orc.LLMB0_BOUNDS),
        t['v'].grad.numpy() * orc.softclip_grad(u3, *orc.LNUG_BOUNDS),
        t['e'].grad.numpy()])
    assert abs(float(nlp.detach()) - m.loss()) < 1e-10 * abs(m.loss())
    np.testing.assert_allclose(g, ref, rtol=1e-8, atol=1e-9 * np.max(np.abs(ref)))


# ---- the host side of the C ABI (runs without a GPU, as tests/test_joint_host.py does) ----
def test_python_names_the_three_kernels():
    import lcgp_amd
    from lcgp_amd import _hip, LCGP
    assert _hip.KERNELS == {'matern32': 0, 'se': 1, 'matern52': 2}
    assert callable(lcgp_amd.Matern52) and callable(lcgp_amd.covmat.Matern52)
    x, y = synth.make_full(5, 30, 2, 3, 3)
    assert LCGP(y=y, x=x, q=3, kernel='matern52').kernel == 'matern52'
    with pytest.raises(ValueError, match="'matern32'.*'se'.*'matern52'"):
        LCGP(y=y, x=x, q=3, kernel='rbf')
    # diag_only needs no device
    np.testing.assert_allclose(lcgp_amd.Matern52(x, x, [0.5, 0.7], 1.7, 1e-3, diag_only=True).numpy(), 1.7)


def test_c_abi_accepts_kernel_id_2_and_refuses_unknown_ids_by_name():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() >= 570
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything

    def head(kernel_id):
        return (None, 0, kernel_id, 100, 2, 3, 1, dummy, None, dummy, dummy)
    # kernel_id = 2 passes the kernel check (which comes first): the refusal names n0
    assert lib.lcgp_predict_cov(*head(2), 0, dummy, 0, dummy, dummy, 0.0) < 0
    err = lib.lcgp_last_error()
    assert b'n0' in err and b'kernel_id' not in err, err
    assert lib.lcgp_predict_grad(*head(2), 0, dummy, dummy, dummy, dummy, dummy, dummy, 0) < 0
    err = lib.lcgp_last_error()
    assert b'n0' in err and b'kernel_id' not in err, err
    # an unknown id is still refused by name, and the message lists the three kernels
    for bad in (7, 3, -1):
        assert lib.lcgp_predict_cov(*head(bad), 10, dummy, 0, dummy, dummy, 0.0) < 0
        err = lib.lcgp_last_error()
        assert b'kernel_id' in err and b'Matern-3/2' in err and b'squared exponential' in err and b'Matern-5/2' in err, err
        assert lib.lcgp_predict_grad(*head(bad), 10, dummy, dummy, dummy, dummy, dummy, dummy, 0) < 0
        assert b'kernel_id' in lib.lcgp_last_error()
    # the second validation site: lcgp_covmat (n1 = 0 is refused for its sizes, not for the kernel)
    ell = (C.c_double * 2)(1.0, 1.0)
    assert lib.lcgp_covmat(None, 0, 7, 10, 10, 2, dummy, dummy, ell, 1.0, 0.0, 0, dummy) < 0
    assert b'kernel_id' in lib.lcgp_last_error() and b'Matern-5/2' in lib.lcgp_last_error()
    assert lib.lcgp_covmat(None, 0, 2, 0, 10, 2, dummy, dummy, ell, 1.0, 0.0, 0, dummy) < 0
    assert b'kernel_id' not in lib.lcgp_last_error()
