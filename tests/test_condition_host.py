"""CPU tests of conditioning on new runs (LCGP.condition / ConditionedLCGP): a numpy stand-in of
HotPathEngine.condition_begin / condition_predict_block written in the closed form of include/lcgp_hip.h, checked against
brute force (augment the training set, refactor I + D (C o s s^T), predict); the host layer -- standardisation of y_new, rep
grouping, the output map, the gather over ranks, staleness, every ValueError -- through that stand-in; and the symbols,
argument checks and sizes of the new C entries (tests/test_gpu_condition.py runs the same through liblcgp_hip.so)."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from lcgp_amd import LCGP, synth
from lcgp_amd import dist as _dist
from lcgp_amd.lcgp import ConditionedLCGP
from oracle import lcgp_oracle as orc
from tests.test_predict_hess_host import HessOracleEngine, _cross

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = ('matern32', 'se', 'matern52')


def closed_form_begin(th, low, z, x, sr, kernel, xn, t, r):
    """(U_n, L_S, v) of one component in the closed form of include/lcgp_hip.h; raises LinAlgError when S is not PD"""
    d = x.shape[1]
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    Xn = _cross(xn, x, ell, scale, nug, kernel) * sr[None, :]
    Un = sla.solve_triangular(low, Xn.T, lower=True).T
    Cnn = _cross(xn, xn, ell, scale, nug, kernel)
    Cnn[np.arange(len(xn)), np.arange(len(xn))] = scale             # the nugget on the diagonal
    S = Cnn - D * Un @ Un.T + np.diag(1.0 / (D * r))
    LS = np.linalg.cholesky(S)
    v = sla.solve_triangular(LS, t - Xn @ z, lower=True)
    return Un, LS, v


def closed_form_predict(th, low, z, x, sr, kernel, xn, Un, LS, v, x0):
    d = x.shape[1]
    ell, scale, nug, D = th[:d], th[d], th[d + 1], th[d + 2]
    X0 = _cross(x0, x, ell, scale, nug, kernel) * sr[None, :]
    U0 = sla.solve_triangular(low, X0.T, lower=True).T
    Sg = _cross(x0, xn, ell, scale, nug, kernel) - D * U0 @ Un.T
    T = sla.solve_triangular(LS, Sg.T, lower=True).T
    return X0 @ z + T @ v, scale - D * np.sum(U0 * U0, axis=1) - np.sum(T * T, axis=1)


class CondOracleEngine(HessOracleEngine):
    """HessOracleEngine plus condition_begin / condition_predict_block in the closed form of include/lcgp_hip.h, in numpy"""
    dtype_name = 'float64'

    @property
    def _theta_last(self):
        return None if self._state is None else np.stack([s[0] for s in self._state])

    def is_current(self, rows):
        return self._state is not None and np.array_equal(self._theta_last, np.asarray(rows))

    def condition_begin(self, xn_s, t, r=None):
        xn = np.asarray(xn_s, np.float64)
        r = np.ones(len(xn)) if r is None else np.asarray(r, np.float64)
        sr = np.ones(self.n) if self.sr is None else self.sr
        parts, info = [], np.zeros(self.q_local, np.int64)
        for i, (th, low, z, b) in enumerate(self._state):
            try:
                parts.append(closed_form_begin(th, low, z, self.x, sr, self.kernel, xn, np.asarray(t)[i], r))
            except np.linalg.LinAlgError:
                info[i] = 1
                parts.append(None)
        if np.any(info):
            err = np.linalg.LinAlgError('S_k not positive definite')
            err.info = info
            raise err
        return {'m': len(xn), 'xn': xn, 'state': parts, 'theta': self._theta_last.copy()}

    def condition_predict_block(self, state, x0s):
        assert self.is_current(state['theta'])
        x0 = np.asarray(x0s, np.float64)
        sr = np.ones(self.n) if self.sr is None else self.sr
        out = np.zeros((2, self.q_local, len(x0)))
        for i, (th, low, z, b) in enumerate(self._state):
            out[0, i], out[1, i] = closed_form_predict(th, low, z, self.x, sr, self.kernel, state['xn'], *state['state'][i], x0)
        return torch.as_tensor(out)


def patch_cond(model, engine_cls=CondOracleEngine):
    def _make(dtype=None):
        rank, world = _dist.rank_world(model._group)
        model._local_ks = _dist.local_components(model.q, rank, world)
        if not model._local_ks:
            return None
        if model.submethod == 'rep':
            sr = np.sqrt(model.r.numpy().astype(float))
            yb = (model.ybar_s if model.rep_standardize_ybar else model.ybar).numpy()
            e = engine_cls(model.x_unique_s.numpy(), yb * sr[None, :], sr, len(model._local_ks),
                           comp_ids=model._local_ks, q_total=model.q, kernel=model.kernel)
        else:
            e = engine_cls(model.x.numpy(), model.y.numpy(), None, len(model._local_ks),
                           comp_ids=model._local_ks, q_total=model.q, kernel=model.kernel)
        e.dtype_name = model._dtype if dtype is None else dtype     # (the arithmetic of the stand-in is float64 either way)
        return e
    model._make_engine = _make
    model._engine = None
    model._invalidate()
    return model


def make_model(mode, kernel='matern32', d=2, group=None, q=2, **kw):
    """a model through the stand-in on non-unit input ranges, its raw training data, and new runs: the full path gets 5 new
    rows, the rep path 4 new unique inputs with 1 to 3 replicates in shuffled order"""
    if mode == 'full':
        x, y = synth.make_full(81 + d, 30, d, 3, 2)
    else:
        x, y = synth.make_rep(82 + d, 14, 3, d, 3, 2)
    x = -1.5 + 4.0 * x
    m = patch_cond(LCGP(y=y, x=x, q=q, submethod=mode, kernel=kernel, process_group=group, **kw))
    o = orc.OracleLCGP(y=y, x=x, q=q, submethod=mode)               # (only for the shape of the parameter vector)
    m._set_flat(synth.param_points(81, o.get_unconstrained())[1])
    rng = np.random.default_rng(17 + d)
    if mode == 'full':
        xn = -1.5 + 4.0 * rng.uniform(0, 1, (5, d))
    else:
        xu = -1.5 + 4.0 * rng.uniform(0, 1, (4, d))
        xn = xu[[0, 1, 1, 2, 2, 2, 3, 0]][rng.permutation(8)]
    yn = rng.standard_normal((3, len(xn))) + 0.3
    return m, x, y, xn, yn


def new_columns(m, xn, yn):
    """what the augmented training set gains: the new unique inputs (standardised), their sqrt(r) and their columns of the
    engine's Y (standardised outputs; sqrt(r) o standardised replicate means on the rep path), from the model's stored data"""
    if m.submethod == 'rep':
        xu, inverse, counts = np.unique(xn, axis=0, return_inverse=True, return_counts=True)
        ybar = np.stack([yn[:, np.asarray(inverse).reshape(-1) == j].mean(axis=1) for j in range(len(xu))], axis=1)
        if m.rep_standardize_ybar:
            ybar = (ybar - m.ybar_mean.numpy()) / m.ybar_std.numpy()
        snew = np.sqrt(counts.astype(float))
        return m._standardise_x0(xu)[0], snew, ybar * snew[None, :]
    return m._standardise_x0(xn)[0], np.ones(len(xn)), (yn - m.ymean.numpy()) / m.ystd.numpy()


def dense_augmented(rows, x, s, Y, kernel, xn_s, snew, ycol, x0s):
    """(ghat, gvar) (q, n0) from first principles in float64 numpy: the training set (x, s, Y) augmented by the new columns, b
    and A = I + D (C o s s^T) rebuilt and solved at the theta rows, lcgp_predict's formulas with same = 0"""
    xa, sa, Ya = np.vstack([x, xn_s]), np.r_[s, snew], np.hstack([Y, ycol])
    d = x.shape[1]
    gh, gv = np.zeros((len(rows), len(x0s))), np.zeros((len(rows), len(x0s)))
    for i, th in enumerate(rows):
        ell, scale, nug, D, psi = th[:d], th[d], th[d + 1], th[d + 2], th[d + 3:]
        Cm = _cross(xa, xa, ell, scale, nug, kernel)
        Cm[np.arange(len(xa)), np.arange(len(xa))] = scale
        low = np.linalg.cholesky(np.eye(len(xa)) + D * Cm * np.outer(sa, sa))
        c = _cross(x0s, xa, ell, scale, nug, kernel) * sa[None, :]
        u = sla.solve_triangular(low, c.T, lower=True)
        gh[i] = u.T @ sla.solve_triangular(low, Ya.T @ psi, lower=True)
        gv[i] = scale - D * np.sum(u * u, axis=0)
    return gh, gv


def brute_force(m, xn, yn, x0):
    eng = m._aux_engine
    s = np.ones(eng.n) if eng.sr is None else eng.sr
    return dense_augmented(eng._theta_last, eng.x, s, eng.Y, eng.kernel, *new_columns(m, xn, yn), m._standardise_x0(x0)[0])


def test_a_nearly_duplicate_pair_keeps_s_positive_definite():
    """S = Sigma_nn + diag(1 / (D r)) with Sigma_nn positive semi-definite: its smallest eigenvalue is at least 1 / D, its
    largest at most m scale, so its condition number is bounded by 1 + m scale D -- about 1e8 at the SoftClip ceiling of the
    scale (1e4), far from 1e16.  Two new inputs 1e-13 apart with the smallest nugget the model allows, on the smoothest kernel
    and at that ceiling, still factor in float64: no VALID input makes S numerically indefinite there, which is why the GPU
    suite has no such case."""
    m, x, _, xn, yn = make_model('full', 'se')
    u = m._get_flat().copy()
    q, d = 2, 2
    u[q * d:q * d + q] = 1e6                # lLmb0 -> its upper bound
    u[q * d + q:q * d + 2 * q] = -50.0      # lnugGPs -> its lower bound
    m._set_flat(u)
    pair = np.vstack([xn[:1], xn[:1] + 1e-13 * np.abs(xn[:1]), xn[1:3]])
    assert not np.array_equal(pair[0], pair[1])
    view = m.condition(pair, yn[:, :4])
    rows = m._aux_engine._theta_last
    assert np.all(rows[:, d] > 9e3) and np.all(rows[:, d + 1] < 2e-7)
    gh, gv = [t.numpy() for t in view.predict(xn, latent=True)]
    assert np.all(np.isfinite(gh)) and np.all(np.isfinite(gv))


@pytest.mark.parametrize('d', [1, 6])
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('mode', ['full', 'rep'])
def test_view_equals_brute_force_augmentation(mode, kernel, d):
    m, x, _, xn, yn = make_model(mode, kernel, d)
    x0 = np.vstack([-1.5 + 4.0 * np.random.default_rng(3).uniform(0, 1, (9, d)), x[:2]])      # training inputs among them
    view = m.condition(xn, yn)
    assert isinstance(view, ConditionedLCGP) and view.base is m
    assert view.m == (5 if mode == 'full' else 4) and tuple(view.x_new.shape) == (view.m, d)
    gh, gv = [t.numpy() for t in view.predict(x0, latent=True)]
    rh, rv = brute_force(m, xn, yn, x0)
    assert gh.shape == (2, 11) and gv.shape == (2, 11)
    np.testing.assert_allclose(gh, rh, rtol=0, atol=1e-9 * np.max(np.abs(rh)))
    np.testing.assert_allclose(gv, rv, rtol=0, atol=1e-9 * np.max(np.abs(rv)))
    # the new runs did something, and the variance never grows
    bh, bv = m._aux_engine.predict(m._standardise_x0(x0)[0])
    assert np.max(np.abs(gh - bh)) > 1e-3 * np.max(np.abs(bh))
    assert np.all(gv <= bv + 1e-12 * np.max(bv))


@pytest.mark.parametrize('mode,kw', [('full', {}), ('full', {'robust_mean': False}), ('rep', {}),
                                     ('rep', {'rep_standardize_ybar': False})])
def test_host_layer_standardisation_grouping_and_output_map(mode, kw):
    m, x, _, xn, yn = make_model(mode, **kw)
    calls = []
    eng = m._get_engine()
    orig = eng.condition_begin
    eng.condition_begin = lambda xs, t, r=None: (calls.append((np.array(xs), np.array(t), None if r is None else np.array(r))),
                                                orig(xs, t, r))[1]
    view = m.condition(torch.as_tensor(xn), torch.as_tensor(yn))
    xs, t, r = calls[0]
    rows = m._aux_engine._theta_last
    d = 2
    if mode == 'full':
        assert r is None
        np.testing.assert_array_equal(xs, (xn - m.x_min.numpy()) / (m.x_max.numpy() - m.x_min.numpy()))
        ys = (yn - m.ymean.numpy()) / m.ystd.numpy()
    else:
        xu = np.unique(xn, axis=0)
        np.testing.assert_array_equal(view.x_new.numpy(), xu)
        np.testing.assert_array_equal(xs, (xu - m.x_min.numpy()) / (m.x_max.numpy() - m.x_min.numpy()))
        assert sorted(r.tolist()) == [1.0, 2.0, 2.0, 3.0] and r.sum() == 8
        ybar = np.stack([yn[:, np.all(xn == u[None, :], axis=1)].mean(axis=1) for u in xu], axis=1)
        ys = (ybar - m.ybar_mean.numpy()) / m.ybar_std.numpy() if m.rep_standardize_ybar else ybar
    np.testing.assert_allclose(t, (rows[:, d + 3:] @ ys) / rows[:, d + 2][:, None], rtol=1e-13)
    # outputs: the unchanged output map on the view's latent rows
    x0 = -1.5 + 4.0 * np.random.default_rng(5).uniform(0, 1, (6, 2))
    gh, gv = [a.numpy() for a in view.predict(x0, latent=True)]
    res = view.predict(x0)
    ref = m._outputs(gh, gv)
    assert len(res) == 3
    for a, b, c in zip(res, ref, m.predict(x0)):
        assert a.dtype == c.dtype and a.shape == c.shape == (3, 6) and not a.requires_grad
        np.testing.assert_array_equal(a.numpy(), b.numpy())
    # the base model is only read
    assert m.ghat.shape[1] == 6 and m._aux_engine is eng
    assert repr(view).startswith('ConditionedLCGP(m=%d' % view.m)


def test_view_goes_stale_when_the_parameters_change():
    m, x, _, xn, yn = make_model('full')
    view = m.condition(xn, yn)
    x0 = x[:3] + 0.01
    view.predict(x0)
    u = m._get_flat().copy()
    m._set_flat(u + 0.01)
    with pytest.raises(RuntimeError, match='stale'):
        view.predict(x0)
    m.predict(x0)                                        # the workspace now holds another factorisation
    with pytest.raises(RuntimeError, match='stale'):
        view.predict(x0)
    m._set_flat(u)                                       # the old parameters again, but the workspace is not theirs
    with pytest.raises(RuntimeError, match='stale'):
        view.predict(x0)
    m.condition(xn, yn).predict(x0)


def test_argument_errors():
    m, x, y, xn, yn = make_model('full')
    cases = [((xn[:, :1], yn), 'x_new must have shape'), ((xn, yn[:2]), 'y_new must have shape'),
             ((xn, yn[:, :4]), 'y_new must have shape'), ((xn[:0], yn[:, :0]), 'N = 0'),
             ((np.where(np.arange(10).reshape(5, 2) == 3, np.nan, xn), yn), 'finite'),
             ((xn, np.where(np.arange(15).reshape(3, 5) == 7, np.inf, yn)), 'finite'),
             ((np.vstack([xn[:4], x[7:8]]), yn), 'equals a training input'),
             ((np.vstack([xn[:4], xn[1:2]]), yn), 'duplicate rows'), ((xn, yn[0]), 'y_new must have shape')]
    for (a, b), msg in cases:
        with pytest.raises(ValueError, match=msg):
            m.condition(a, b)
    for (a, b), msg in cases[-3:-1]:
        with pytest.raises(ValueError, match='refit'):
            m.condition(a, b)
    mr, xr, _, xnr, ynr = make_model('rep')
    with pytest.raises(ValueError, match='equals a training input'):
        mr.condition(np.vstack([xnr, mr.x_unique.numpy()[3:4]]), np.hstack([ynr, ynr[:, :1]]))
    assert mr.condition(xnr, ynr).m == 4                 # duplicate rows are replicates there
    view = m.condition(xn, yn)
    with pytest.raises(ValueError, match='x0 must have shape'):
        view.predict(np.zeros((3, 3)))


def test_non_positive_definite_s_raises_linalgerror_on_every_component_named():
    class Fails(CondOracleEngine):
        def condition_begin(self, xn_s, t, r=None):
            err = np.linalg.LinAlgError('S_k')
            err.info = np.array([0, 3])
            raise err
    m, x, _, xn, yn = make_model('full')
    patch_cond(m, Fails)
    with pytest.raises(np.linalg.LinAlgError, match=r'component\(s\) \[1\].*info \[3\]'):
        m.condition(xn, yn)


def test_float32_model_builds_the_view_on_its_float64_engine_when_float32_fails():
    """a stand-in whose float32 engine reports a non-PD S: the view is built once on the float64 engine; the model's own
    state (engine that answers, flags, last gradient) is what it was, predict() of the base model is unchanged and comes from
    the float32 engine, and the view's staleness check runs on the float64 engine"""
    calls = []

    class F32Fails(CondOracleEngine):
        def condition_begin(self, xn_s, t, r=None):
            calls.append(self.dtype_name)
            if self.dtype_name == 'float32':
                err = np.linalg.LinAlgError('S_k')
                err.info = np.array([0, 2])
                raise err
            return super().condition_begin(xn_s, t, r)

        def predict_block(self, x0s, same=0):
            calls.append('predict ' + self.dtype_name)
            return super().predict_block(x0s, same)
    m, x, _, xn, yn = make_model('full', dtype='float32')
    patch_cond(m, F32Fails)
    x0 = x[:4] + 0.01
    p0 = [t.numpy().copy() for t in m.predict(x0)]
    e32 = m._aux_engine
    assert e32.dtype_name == 'float32' and m._engine64 is None
    before = (m._last_eval_float64, m._float64_only, m._gc_last.copy(), m.float32_fallbacks)
    del calls[:]
    view = m.condition(xn, yn)
    assert calls == ['float32', 'float64']
    assert view._engine is m._engine64 and view._engine.dtype_name == 'float64'
    assert m._aux_engine is e32 and m._aux_valid
    assert (m._last_eval_float64, m._float64_only) == before[:2] and np.array_equal(m._gc_last, before[2])
    assert m.float32_fallbacks == before[3] + 1          # the one thing it counts on the model
    ref = patch_cond(make_model('full')[0])              # the same model through a stand-in that does not fail
    want = ref.condition(xn, yn).predict(x0)
    got = view.predict(x0)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    del calls[:]
    p1 = [t.numpy() for t in m.predict(x0)]
    assert calls == ['predict float32'] and all(np.array_equal(a, b) for a, b in zip(p0, p1))
    view.predict(x0)                                     # still current
    m._set_flat(m._get_flat() + 0.01)
    with pytest.raises(RuntimeError, match='stale'):
        view.predict(x0)
    m.predict(x0)                                        # the float32 engine moved on, the float64 engine did not ...
    with pytest.raises(RuntimeError, match='stale'):     # ... and the view is stale all the same
        view.predict(x0)
    # float64 models and float32_fallback=False do not try again
    m2 = patch_cond(make_model('full', dtype='float32')[0], F32Fails)
    m2.float32_fallback = False
    with pytest.raises(np.linalg.LinAlgError, match=r'component\(s\) \[1\].*info \[2\]'):
        m2.condition(xn, yn)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_gather_what_one_rank_computes():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "_condition_host_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANK 0 OK" in res.stdout and "RANK 1 OK" in res.stdout


NEW_SYMBOLS = ('lcgp_condition_scratch_bytes', 'lcgp_condition_state_bytes', 'lcgp_condition_prepare', 'lcgp_condition_predict')


def test_new_symbols_version_and_sizes():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() == 610
    for name in NEW_SYMBOLS:
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    from lcgp_amd.engine import HotPathEngine
    assert hasattr(HotPathEngine, 'condition_begin') and hasattr(HotPathEngine, 'condition_predict_block')
    nb = C.c_size_t(0)

    def sb(m, n0, dtype=0, n=4096, q=8):
        assert lib.lcgp_condition_scratch_bytes(dtype, n, q, m, n0, C.byref(nb)) == 0, lib.lcgp_last_error()
        return nb.value

    def st(m, dtype=0, n=4096, q=8):
        assert lib.lcgp_condition_state_bytes(dtype, n, 6, q, m, C.byref(nb)) == 0, lib.lcgp_last_error()
        return nb.value

    ms, n0s = (1, 64, 128, 129, 256, 1000, 1024, 4096), (0, 1, 64, 127, 128, 129, 1000, 2048)
    for dtype in (0, 1):
        for a, b in zip(ms, ms[1:]):
            assert st(a, dtype) <= st(b, dtype)
            for n0 in n0s:
                assert sb(a, n0, dtype) <= sb(b, n0, dtype)
        for m in ms:
            for a, b in zip(n0s, n0s[1:]):
                assert sb(m, a, dtype) <= sb(m, b, dtype)
    # the documented sizes: mpad (npad + mpad) elements and mpad doubles per component; 2 n0pad (npad + mpad) elements
    assert st(1000) == 8 * (1024 * (4096 + 1024) * 8 + 1024 * 8)
    assert sb(1000, 2048) == 2 * 8 * 2048 * (4096 + 1024) * 8
    assert st(1000, 1) < st(1000) and sb(1000, 2048, 1) < sb(1000, 2048)
    for args, msg in (((0, 4096, 8, 0, 1), b'm < 1'), ((0, 4096, 8, 5, -1), b'n0 < 0'), ((2, 4096, 8, 5, 1), b'dtype'),
                      ((0, 0, 8, 5, 1), b'n, q_local')):
        assert lib.lcgp_condition_scratch_bytes(*args, C.byref(nb)) < 0
        assert msg in lib.lcgp_last_error()
    assert lib.lcgp_condition_scratch_bytes(0, 4096, 8, 5, 1, None) < 0
    assert lib.lcgp_condition_state_bytes(0, 4096, 6, 8, 0, C.byref(nb)) < 0 and b'm < 1' in lib.lcgp_last_error()
    assert lib.lcgp_condition_state_bytes(0, 4096, 6, 8, 5, None) < 0


def test_c_abi_argument_checks():
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    dummy = C.c_void_p(16)          # never dereferenced: every call below is refused before it enqueues anything
    big = 1 << 40

    def prep(dtype=0, kern=0, n=50, d=2, q=2, m=4, x=dummy, theta=dummy, ws=dummy, xn=dummy, t=dummy, scratch=dummy, nsc=big,
             cws=dummy, state=dummy, info=dummy):
        return lib.lcgp_condition_prepare(None, dtype, kern, n, d, 3, q, x, None, theta, ws, m, xn, t, None, scratch, nsc, cws,
                                          state, info)

    def pred(dtype=0, kern=0, n=50, d=2, q=2, m=4, n0=3, x=dummy, theta=dummy, ws=dummy, state=dummy, xn=dummy, x0=dummy,
             scratch=dummy, nsc=big, ghat=dummy, gvar=dummy, stride=0):
        return lib.lcgp_condition_predict(None, dtype, kern, n, d, 3, q, x, None, theta, ws, state, m, xn, n0, x0, scratch, nsc,
                                          ghat, gvar, stride)

    nb = C.c_size_t(0)
    assert lib.lcgp_condition_scratch_bytes(0, 50, 2, 4, 0, C.byref(nb)) == 0
    need_prep = nb.value
    assert lib.lcgp_condition_scratch_bytes(0, 50, 2, 4, 3, C.byref(nb)) == 0
    need_pred = nb.value
    common = [(dict(m=0), 'm < 1'), (dict(kern=3), 'kernel_id'), (dict(dtype=2), 'dtype'), (dict(d=0), 'd must be'),
              (dict(d=127), 'd must be'), (dict(n=0), 'n < 1'), (dict(q=0), 'q_local'), (dict(x=None), 'NULL'),
              (dict(theta=None), 'NULL'), (dict(ws=None), 'NULL'), (dict(xn=None), 'NULL'), (dict(scratch=None), 'NULL'),
              (dict(state=None), 'NULL')]
    for kw, msg in common + [(dict(t=None), 'NULL'), (dict(cws=None), 'NULL'), (dict(info=None), 'NULL'),
                             (dict(nsc=need_prep - 1), 'scratch is smaller'), (dict(nsc=0), 'scratch is smaller')]:
        assert prep(**kw) == -1, kw
        assert msg.encode() in lib.lcgp_last_error(), (kw, lib.lcgp_last_error())
    for kw, msg in common + [(dict(n0=0), 'n0 < 1'), (dict(x0=None), 'NULL'), (dict(ghat=None), 'NULL'), (dict(gvar=None), 'NULL'),
                             (dict(stride=2), 'out_stride'), (dict(nsc=need_pred - 1), 'scratch is smaller')]:
        assert pred(**kw) == -1, kw
        assert msg.encode() in lib.lcgp_last_error(), (kw, lib.lcgp_last_error())
