"""The Hessian of the calibration target on the GPU (lcgp_calib_hess_rows, CalibrationTarget.loglik_hess): the row entry alone on
synthetic inputs against the np.longdouble evaluation of the same formulas (every q path of the first launch, one wavefront per
row in the second; gvar = 0 and slightly negative, a rank-deficient M, rows of a strided block, a wide d), ll / dll / sens
bitwise lcgp_calib_rows', bitwise independence of the optional outputs, of how the rows are split and of what the outputs held;
then the model: d2ll against the Hessian of the dense p-space density fed with the GPU's own latent Hessians and against
central differences of the GPU's loglik_grad, a view's target against an engine on the augmented data, a float32 model, two
ranks against one, autograd to second order on a device tensor, the headline shape.

Measured on an MI355X (largest error / tolerance over all cases; the tolerances are calib_hess_ref.row_tolerances2's and the
model-level bound stated at _dense_bound): see DESIGN.md 4.21."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lcgp_amd import LCGP, _hip, synth
from lcgp_amd.engine import calib_hess_rows_device
from tests import calib_hess_ref as href
from tests import calib_ref as ref
from tests.test_gpu_calibration import DEV, EPS, _dev, _free_port, _p
from tests.test_gpu_calibration import _run as _run_first_order
from tests.test_predict_hess_host import assert_clear_of_kinks

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N0, D = href.N0, href.D
NAMES = ('ll', 'dll', 'd2ll', 's', 'v', 'B')

_CACHE = {}


def _reference(q, deficient):
    """(inputs, longdouble reference, tolerances) of the whole synthetic block: computed once, only read"""
    key = (q, deficient)
    if key not in _CACHE:
        inp = href.wide_inputs() if q == 'wide' else href.hess_inputs(q, deficient)
        r64, rld = href.rows2_of(inp), href.rows2_of(inp, dtype=np.longdouble)
        _CACHE[key] = (inp, rld, href.row_tolerances2(r64, rld))
    return _CACHE[key]


def _run(inp, q, n0, d, row0=0, sens=True, want_B=True, want_d2=True, fill=0x00, stride=N0):
    """lcgp_calib_hess_rows on rows row0 .. row0 + n0 of the block, read in place (in_stride = the block's rows >= n0), with the
    first d input dimensions (their Jacobians and the leading d (d + 1) / 2 entries of the packed triangles, repacked); outputs
    pre-filled with the byte `fill`.  Returns numpy (ll, dll, d2ll, s, v, B), None where not requested."""
    lib = _hip.load()
    tri = d * (d + 1) // 2
    t = {k: _dev(v) for k, v in (('ghat', inp['ghat']), ('gvar', inp['gvar']), ('dghat', inp['dghat'][:, :, :d]),
                                 ('dgvar', inp['dgvar'][:, :, :d]), ('d2ghat', inp['d2ghat'][:, :, :tri]),
                                 ('d2gvar', inp['d2gvar'][:, :, :tri]), ('M', inp['M']), ('b', inp['b']),
                                 ('ir', inp['inv_range'][:d]))}
    assert row0 + n0 <= stride == inp['ghat'].shape[1]
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=DEV)        # noqa: E731
    ll, dll = new(n0), new(n0, d)
    d2ll = new(n0, tri) if want_d2 else None
    sv = new(2, q, n0) if sens else None
    B = new(n0, q, q) if want_B else None
    for o in (ll, dll, d2ll, sv, B):
        if o is not None:
            o.view(torch.uint8).fill_(fill)
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    _hip.check(lib.lcgp_calib_hess_rows(st, q, d, n0, _p(t['ghat'], row0), _p(t['gvar'], row0), _p(t['dghat'], row0 * d),
                                        _p(t['dgvar'], row0 * d), _p(t['d2ghat'], row0 * tri), _p(t['d2gvar'], row0 * tri), stride,
                                        _p(t['M']), _p(t['b']), inp['c0'], inp['lognorm'], _p(t['ir']), _p(ll), _p(dll), _p(d2ll),
                                        _p(sv), _p(B)), 'lcgp_calib_hess_rows')
    torch.cuda.synchronize()
    n = lambda o: None if o is None else o.cpu().numpy()                             # noqa: E731
    sv = n(sv)
    return n(ll), n(dll), n(d2ll), None if sv is None else sv[0], None if sv is None else sv[1], n(B)


WORST = {}


def _check(got, rld, tol, rows, d, what):
    tri = d * (d + 1) // 2
    ll, dll, d2ll, s, v, B = got
    for name, g, want, t in (('ll', ll, rld['ll'][rows], tol['ll'][rows]), ('s', s, rld['s'][:, rows], tol['s'][:, rows]),
                             ('v', v, rld['v'][:, rows], tol['v'][:, rows]), ('dll', dll, rld['dll'][rows, :d], tol['dll'][rows, :d]),
                             ('B', B, rld['B'][rows], tol['B'][rows]),
                             ('d2ll', d2ll, rld['d2ll'][rows, :tri], tol['d2ll'][rows, :tri])):
        if g is None:
            continue
        assert np.all(np.isfinite(g)), (what, name)
        err = np.abs(g.astype(np.longdouble) - want)
        worst = np.unravel_index(np.argmax(err / t), err.shape)
        ratio = float(err[worst] / t[worst])
        WORST[name] = max(WORST.get(name, 0.0), ratio)
        print('%s %s: largest error / tolerance %.3g' % (what, name, ratio))
        assert np.all(err <= t), (what, name, worst, float(err[worst]), float(t[worst]))


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nlcgp_calib_hess_rows: largest error / tolerance per quantity over all row cases: '
          + ', '.join('%s %.3g' % kv for kv in sorted(WORST.items())))


@pytest.mark.parametrize('deficient', [False, True], ids=['full-rank', 'rank-deficient'])
@pytest.mark.parametrize('q', href.ROW_QS)
def test_row_entry_against_longdouble_and_bitwise_the_first_order_entry(q, deficient):
    """every n0 is a part of the block of N0 = 257 rows read in place: in_stride > n0 except at n0 = 257"""
    inp, rld, tol = _reference(q, int(deficient))
    for n0 in (1, 63, 64, 65, 257):
        for d in (1, 6):
            got = _run(inp, q, n0, d)
            _check(got, rld, tol, slice(0, n0), d, 'q=%d n0=%d d=%d' % (q, n0, d))
            first = _run_first_order(inp, q, n0, d)                 # lcgp_calib_rows: (ll, dll, s, v)
            for a, b in zip(first, (got[0], got[1], got[3], got[4])):
                assert np.array_equal(a, b), (q, n0, d)
            assert np.array_equal(got[5], np.swapaxes(got[5], 1, 2))            # B is bitwise symmetric
            if d == 1 and n0 != 65:
                continue
            # with and without the optional outputs: the same bits in what remains
            for sens, want_B, want_d2 in ((False, False, True), (True, False, True), (False, True, True), (True, True, False),
                                          (False, False, False)):
                part = _run(inp, q, n0, d, sens=sens, want_B=want_B, want_d2=want_d2, fill=0xFF)
                for name, a, b in zip(NAMES, part, got):
                    assert a is None or np.array_equal(a, b), (q, n0, d, sens, want_B, want_d2, name)
    # rows in the middle of the block: a strided block that does not start at the block's first row
    got = _run(inp, q, 70, 6, row0=130)
    _check(got, rld, tol, slice(130, 200), 6, 'q=%d rows 130..200' % q)


def test_row_entry_wide_d():
    """d = 40 at q = 9, n0 = 5: tri = 820"""
    inp, rld, tol = _reference('wide', 0)
    w = href.WIDE
    got = _run(inp, w['q'], w['n0'], w['d'], stride=w['n0'])
    _check(got, rld, tol, slice(0, w['n0']), w['d'], 'wide')
    first = _run_wide_first_order(inp)
    for a, b in zip(first, (got[0], got[1], got[3], got[4])):
        assert np.array_equal(a, b)


def _run_wide_first_order(inp):
    from lcgp_amd.engine import calib_rows_device
    blk = _dev(np.stack([inp['ghat'], inp['gvar']]))
    jac = _dev(np.stack([inp['dghat'], inp['dgvar']]))
    ll, dll, sens = calib_rows_device(blk, jac, _dev(inp['M']), _dev(inp['b']), inp['c0'], inp['lognorm'], _dev(inp['inv_range']),
                                      True)
    sens = sens.cpu().numpy()
    return ll.cpu().numpy(), dll.cpu().numpy(), sens[0], sens[1]


@pytest.mark.parametrize('q', [1, 8, 9, 64])
def test_rows_are_bitwise_independent_of_the_split_and_of_the_outputs_content(q):
    inp = _reference(q, 0)[0]
    whole = _run(inp, q, N0, D, fill=0x00)
    for fill in (0xFF, 0x5A):
        again = _run(inp, q, N0, D, fill=fill)
        for a, b in zip(whole, again):
            assert np.array_equal(a, b), fill
    cut = 128
    first, second = _run(inp, q, cut, D, fill=0xFF), _run(inp, q, N0 - cut, D, row0=cut, fill=0x5A)
    for w, axis in ((0, 0), (1, 0), (2, 0), (3, 1), (4, 1), (5, 0)):
        assert np.array_equal(np.concatenate([first[w], second[w]], axis=axis), whole[w]), NAMES[w]


# ------------------------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------------------------
def _dense_bound(m, src, theta, y_obs, obs_var):
    """(d2ll of the dense p-space density from the GPU's own latents of `src` (the model or a view), its error bound): the
    bound tests/test_gpu_calibration.py uses for loglik, 64 p eps cond(Sigma_i) x magnitude, with the sum of the absolute
    values of the Hessian's six dense terms (calib_hess_ref.dense_hess) in the place of |quad| + |logdet| + p"""
    ghat, gvar, dghat, dgvar, d2ghat, d2gvar = src._latent_predict_hess(theta)
    _, phi_s, t, lam = ref.observation(m, y_obs, obs_var)
    inv_range = 1.0 / (m.x_max.numpy() - m.x_min.numpy()).reshape(-1)
    want, mag = href.dense_hess(phi_s, t, lam, ghat, gvar, dghat, dgvar, d2ghat, d2gvar, inv_range)
    cov = ref.dense_loglik(phi_s, t, lam, ghat, gvar)[1]
    cond = np.array([np.linalg.cond(c) for c in cov])
    assert np.all(cond <= 1e6), cond.max()
    return want, 64 * int(m.p) * EPS * cond[:, None, None] * mag


def _central_differences_of_loglik_grad(tgt, theta, h):
    out = np.zeros(theta.shape + (theta.shape[1],))
    for c in range(theta.shape[1]):
        e = np.zeros_like(theta)
        e[:, c] = h[c]
        out[..., c] = (tgt.loglik_grad(theta + e)[1].numpy() - tgt.loglik_grad(theta - e)[1].numpy()) / (2 * h[c])
    return out


def _clear_rows(theta, knots, h):
    """the rows of theta whose every coordinate is at least two steps from every knot's (Matern-3/2's kinks)"""
    return np.flatnonzero(np.min(np.abs(theta[:, None, :] - knots[None, :, :]) / h, axis=(1, 2)) >= 2.0)


def _model_checks(tgt, m, src, theta, y_obs, obs_var, knots, what):
    n0, d = theta.shape
    q = int(m.q)
    ll, dll, d2ll, s, v, B = tgt.loglik_hess(theta, latent=True)
    assert d2ll.shape == (n0, d, d) and B.shape == (n0, q, q) and s.shape == v.shape == (q, n0)
    assert d2ll.dtype == torch.float64 and d2ll.device.type == 'cpu' and torch.all(torch.isfinite(d2ll))
    assert torch.equal(d2ll, d2ll.transpose(-1, -2))
    for a, b in zip((ll, dll, s, v), tgt.loglik_grad(theta, latent=True)):
        assert np.array_equal(a.numpy(), b.numpy())                 # bitwise loglik_grad's, kink rows included
    want, tol = _dense_bound(m, src, theta, y_obs, obs_var)
    ratio = np.max(np.abs(d2ll.numpy() - want) / tol)
    print('%s: largest d2ll error / bound against the dense Hessian %.3g' % (what, ratio))
    assert ratio <= 1.0, (what, ratio)
    h = 1e-5 * (m.x_max.numpy() - m.x_min.numpy()).reshape(-1)
    rows = _clear_rows(theta, knots, h) if m.kernel == 'matern32' else np.arange(n0)
    assert len(rows) >= n0 - 4
    if m.kernel == 'matern32':
        assert_clear_of_kinks(theta[rows], knots, h)
    fd = _central_differences_of_loglik_grad(tgt, theta[rows], h)
    err = np.max(np.abs(d2ll.numpy()[rows] - fd)) / np.max(np.abs(fd))
    print('%s: d2ll against central differences of loglik_grad %.3g of the largest entry' % (what, err))
    assert err <= 1e-6, (what, err)


@pytest.mark.parametrize('name', list(ref.MODEL_CASES))
def test_loglik_hess_against_the_dense_hessian_and_central_differences(name):
    m, x, y = ref.model_case(name)
    knots = np.unique(x, axis=0)
    for form, drop in (('dense', None), ('diag', 2)):
        theta, y_obs, obs_var = ref.case_observation(name, x, y, form)
        if drop is not None:
            y_obs = y_obs.copy()
            y_obs[drop] = np.nan
        _model_checks(m.calibration(y_obs, obs_var), m, m, theta, y_obs, obs_var, knots, '%s %s' % (name, form))


@pytest.mark.parametrize('mode,kernel', [('full', 'matern32'), ('rep', 'se')])
def test_view_target_against_the_augmented_engine(mode, kernel):
    from tests.test_gpu_condition_grad import _augmented_engine, _box_model, _new_runs
    m, x = _box_model(mode, kernel)
    xn, yn = _new_runs(m, x, 5, 14)
    view = m.condition(xn, yn)
    rng = np.random.default_rng(15)
    sd = yn.std(axis=1)
    y_obs = yn[:, 3] + 0.1 * sd * rng.standard_normal(4)
    obs_var = (sd * rng.uniform(0.2, 0.4, 4)) ** 2
    tgt = view.calibration(y_obs, obs_var)
    lo, hi = x.min(0), x.max(0)
    theta = lo + (hi - lo) * rng.uniform(0.05, 0.95, (17, 3))
    theta[:2] = x[[3, 11]]
    theta[2] = xn[0]
    _model_checks(tgt, m, view, theta, y_obs, obs_var, np.vstack([np.unique(x, axis=0), xn]), 'view %s %s' % (mode, kernel))
    # calib_hess_rows_device on the augmented engine's predict_hess_block with the same M, b, c0, lognorm
    got = tgt.loglik_hess(theta, latent=True)
    aug = _augmented_engine(m, xn, yn)
    blk, jac, hess = aug.predict_hess_block(m._standardise_x0(theta)[0])
    M, b, inv_range = tgt._device_consts(blk.device)
    ll, dll, packed, sens, B = [u.cpu().numpy() for u in calib_hess_rows_device(blk, jac, hess, M, b, tgt.c0, tgt.lognorm, inv_range,
                                                                               True, True)]
    for nm, g, w in (('ll', got[0], ll), ('dll', got[1], dll), ('d2ll', got[2], href.unpack_lower(packed, 3)), ('B', got[5], B)):
        err = np.max(np.abs(g.numpy() - w)) / np.max(np.abs(w))
        print('view %s %s: %s against the augmented engine %.3e (bound 1e-9)' % (mode, kernel, nm, err))
        assert err <= 1e-9, (nm, err)
    m._set_flat(m._get_flat() + 0.01)
    with pytest.raises(RuntimeError, match='stale'):
        tgt.loglik_hess(theta)


def test_float32_model_row_entry_on_its_own_latent_blocks():
    """a float32 model's engine writes its latents, Jacobians and Hessians in double: the float64 row entry on them against the
    longdouble formulas fed with the same arrays, at the row entry's tolerance"""
    name = 'full-matern32-q3'
    m, x, y = ref.model_case(name, dtype='float32')
    theta, y_obs, obs_var = ref.case_observation(name, x, y, 'dense')
    tgt = m.calibration(y_obs, obs_var)
    eng = m._ensure_aux()
    assert eng.dtype_name == 'float32'
    blk, jac, hess = eng.predict_hess_block(m._x0_2d(theta, 'theta'))
    M, b, inv_range = tgt._device_consts(blk.device)
    ll, dll, packed, sens, B = [t.cpu().numpy() for t in calib_hess_rows_device(blk, jac, hess, M, b, tgt.c0, tgt.lognorm,
                                                                               inv_range, True, True)]
    n = lambda t: t.cpu().numpy()                                                   # noqa: E731
    args = (n(blk[0]), n(blk[1]), n(jac[0]), n(jac[1]), n(hess[0]), n(hess[1]), tgt.M, tgt.b, tgt.c0, tgt.lognorm, n(inv_range))
    r64, rld = href.rows2(*args), href.rows2(*args, dtype=np.longdouble)
    _check((ll, dll, packed, sens[0], sens[1], B), rld, href.row_tolerances2(r64, rld), slice(0, 17), 3, 'float32 model')
    got = tgt.loglik_hess(theta, latent=True)
    for a, b_ in zip(got, (ll, dll, href.unpack_lower(packed, 3), sens[0], sens[1], B)):
        assert np.array_equal(a.numpy(), b_)
    for a, b_ in zip(got[:2], tgt.loglik_grad(theta)):
        assert torch.equal(a, b_)


def test_two_ranks_equal_one_rank_bitwise():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_calibration_hess_gpu_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


def test_loglik_differentiable_order_two_on_the_device():
    name = 'rep-se-q3'
    m, x, y = ref.model_case(name)
    theta, y_obs, obs_var = ref.case_observation(name, x, y, 'diag')
    tgt = m.calibration(y_obs, obs_var)
    th = theta[2:6]
    tt = torch.tensor(th, dtype=torch.float64, device=DEV, requires_grad=True)
    out = tgt.loglik_differentiable(tt, order=2)
    assert out.device == tt.device and torch.equal(out.cpu(), tgt.loglik(th))
    (g,) = torch.autograd.grad(out.sum(), tt, create_graph=True)
    assert g.device == tt.device and g.requires_grad and torch.equal(g.detach().cpu(), tgt.loglik_grad(th)[1])
    H = torch.autograd.functional.hessian(lambda t: tgt.loglik_differentiable(t, order=2).sum(), tt.detach())
    assert H.device == tt.device and H.shape == (4, 3, 4, 3)
    want = tgt.loglik_hess(th)[2]
    for i in range(4):
        for j in range(4):
            assert torch.equal(H[i, :, j, :].cpu(), want[i] if i == j else torch.zeros(3, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='double backward'):
        torch.autograd.grad(tgt.loglik_differentiable(tt).sum(), tt, create_graph=True)


def test_headline_shape():
    """n = 4096, d = 6, p = 64, q = 8, n0 = 2000, parameters set, no fit: the whole call, then central differences of
    loglik_grad on a sample of kink-clear rows.  Timing is reported by tools/calib_hess_bench.py, not asserted here."""
    x, y, cfg = synth.make_config(3)
    m = LCGP(y=y, x=x, q=cfg['q'], device=DEV)
    d = cfg['d']
    rng = np.random.default_rng(12)
    theta = rng.uniform(0, 1, (2000, d))
    sd = y.std(axis=1)
    y_obs = y[:, 100] + 0.1 * sd * rng.standard_normal(cfg['p'])
    tgt = m.calibration(y_obs, (0.1 * sd) ** 2)
    ll, dll, d2ll = [t.numpy() for t in tgt.loglik_hess(theta)]
    assert ll.shape == (2000,) and dll.shape == (2000, d) and d2ll.shape == (2000, d, d) and np.all(np.isfinite(d2ll))
    assert np.array_equal(d2ll, np.swapaxes(d2ll, 1, 2))
    for a, b in zip((ll, dll), tgt.loglik_grad(theta)):
        assert np.array_equal(a, b.numpy())
    h = 1e-5 * (x.max(0) - x.min(0))
    clear = _clear_rows(theta, x, h)
    assert len(clear) >= 3
    rows = [int(clear[0]), int(clear[len(clear) // 2]), int(clear[-1])]
    assert_clear_of_kinks(theta[rows], x, h)
    fd = _central_differences_of_loglik_grad(tgt, theta[rows], h)
    err = np.max(np.abs(d2ll[rows] - fd)) / np.max(np.abs(fd))
    print('headline: d2ll against central differences %.3g of the largest entry' % err)
    assert err <= 1e-6, err
