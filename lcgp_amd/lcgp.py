"""LCGP with the reference's Python surface, hot path on MI355X.

Host-side mirror of `lcgp.LCGP` (reference `src/lcgp/lcgp.py:19-930`): same constructor, attributes, methods,
exceptions and return shapes, so a caller of the reference can switch imports.  The one-off preprocessing
(standardisation, replicate grouping, SVD basis, initial parameters; lcgp.py:295-513) is host numpy; what
`fit()` loops over and what `predict()` consumes -- covariance build, factorisation, NLL, its gradient, the
prediction caches -- runs in liblcgp_hip.so (include/lcgp_hip.h).  There is no CPU fallback for that part.

Deliberate differences from the reference, all documented in DESIGN.md:
  * gradients are closed-form instead of a TensorFlow tape; the Cholesky form of the objective
    replaces the eigendecomposition (identical value);
  * prediction caches are invalidated by `fit()`/parameter changes (the reference reuses stale ones);
  * the (q,n,n) cache tensors `Ths`/`Tks` are materialised only when read, never at construction;
  * results are CPU float64 torch tensors (the reference returns TF tensors; both have .numpy()/.shape);
  * the unconditional "VARIANCE OF G" print (lcgp.py:482-483) happens only with verbose=True;
  * keyword-only extras: device, dtype ('float64' | 'float32'), process_group (component-parallel multi-GPU).
"""
from __future__ import annotations

import math
import zlib

import numpy as np
import scipy.optimize as sopt
import torch

from . import dist as _dist
from .params import Parameter, SoftClip
from .params import softclip_flat, softclip_flat2

F64 = np.float64


def _t(a):
    """numpy -> CPU float64 torch tensor (what the public surface hands out)."""
    return torch.as_tensor(np.asarray(a, dtype=F64))


def _np(a):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().numpy().astype(F64)
    if isinstance(a, Parameter):
        return a.numpy()
    return np.asarray(a, dtype=F64)


def _box_double_average(kernel, a):
    """I2 = (1 / w^2) int int kappa(|t - t'| / ell) dt dt' over [0, w]^2 = 2 [F(a) / a - G(a) / a^2], a = w / ell, of the 1-D
    factor of the product kernel (a scalar, host side: q d values per call).  Matern below a = 1/2: F and G from
    the Taylor series of kappa, as the device does, because their closed forms cancel there."""
    import math
    if kernel == 'se':
        Fa, Ga = math.sqrt(0.5 * math.pi) * math.erf(a * math.sqrt(0.5)), -math.expm1(-0.5 * a * a)
    elif a < 0.5:
        t, sf, sg = 1.0, 0.0, 0.0
        for m in range(20):
            f = 1.0 - m if kernel == 'matern32' else (m - 1.0) * (m - 3.0) / 3.0
            sf += t * f / (m + 1.0)
            sg += t * f / (m + 2.0)
            t *= -a / (m + 1.0)
        Fa, Ga = a * sf, a * a * sg
    else:
        e, em = math.exp(-a), -math.expm1(-a)
        if kernel == 'matern32':
            Fa, Ga = 2.0 * em - a * e, 3.0 * em - a * (3.0 + a) * e
        else:
            Fa, Ga = (8.0 / 3.0) * em - a * (5.0 + a) / 3.0 * e, 5.0 * em - a * (5.0 + a * (2.0 + a / 3.0)) * e
    return 2.0 * (Fa / a - Ga / (a * a))


def _percentile50_nearest(a):
    """tfp.stats.percentile(a, 50.0, axis=1, keepdims=True) with its default 'nearest' interpolation
    (lcgp.py:317-318, 388-389): ascending sort, index round-half-even(0.5 (m-1)).  Not np.median."""
    a = np.asarray(a, F64)
    idx = int(np.round(0.5 * (a.shape[1] - 1)))
    return np.sort(a, axis=1)[:, idx:idx + 1]


class _PredictFn(torch.autograd.Function):
    """LCGP.predict_differentiable: forward = predict()'s outputs from one lcgp_predict_grad pass, backward = the per-point
    vector-Jacobian product with the saved output Jacobians"""

    @staticmethod
    def forward(ctx, x0, model):
        ghat, gvar, dghat, dgvar = model._latent_predict_grad(x0.detach().cpu().to(torch.float64))
        outs = model._outputs(ghat, gvar)
        dyp, dycv = model._output_jacobians(dghat, dgvar)
        ctx.x0_dtype, ctx.x0_device, ctx.x0_shape = x0.dtype, x0.device, x0.shape
        ctx.jac = (torch.as_tensor(dyp), torch.as_tensor(dycv))
        return tuple(o.to(x0.device) for o in outs[:3])

    @staticmethod
    def backward(ctx, g_ypred, g_ypredvar, g_yconfvar):
        if torch.is_grad_enabled():         # create_graph=True: the saved Jacobians are constants, not a graph
            raise RuntimeError('LCGP.predict_differentiable supports first derivatives only: double backward '
                               '(create_graph=True) is not available; use predict_grad() for the Jacobians')
        dyp, dycv = ctx.jac
        gx = torch.zeros(dyp.shape[1:], dtype=torch.float64)
        if g_ypred is not None:
            gx += torch.einsum('ai,ail->il', g_ypred.detach().cpu().to(torch.float64), dyp)
        gv = [g.detach().cpu().to(torch.float64) for g in (g_ypredvar, g_yconfvar) if g is not None]
        if gv:
            gx += torch.einsum('ai,ail->il', sum(gv), dycv)
        return gx.reshape(ctx.x0_shape).to(device=ctx.x0_device, dtype=ctx.x0_dtype), None


def _vjp_first(g_ypred, g_ypredvar, g_yconfvar, dyp, dycv):
    """(n0, d) CPU float64: sum_a g_ypred[a, i] dyp[a, i, l] + (g_ypredvar + g_yconfvar)[a, i] dycv[a, i, l]"""
    gp, gv = _cpu64(g_ypred), _cpu64(g_ypredvar) + _cpu64(g_yconfvar)
    return torch.einsum('ai,ail->il', gp, dyp) + torch.einsum('ai,ail->il', gv, dycv)


def _cpu64(t):
    return t.detach().cpu().to(torch.float64)


class _PredictFn2(torch.autograd.Function):
    """LCGP.predict_differentiable(order=2): _PredictFn whose backward pass is itself a differentiable function
    (_PredictVjpFn) of x0 and of the incoming gradients"""

    @staticmethod
    def forward(ctx, x0, model):
        x0c = _cpu64(x0)
        host = getattr(model, 'base', model)        # (a ConditionedLCGP: the output map is its base model's)
        ghat, gvar, dghat, dgvar = model._latent_predict_grad(x0c)
        outs = host._outputs(ghat, gvar)
        dyp, dycv = host._output_jacobians(dghat, dgvar)
        ctx.model, ctx.x0c = model, x0c
        ctx.jac = (torch.as_tensor(dyp), torch.as_tensor(dycv))
        ctx.save_for_backward(x0)
        return tuple(o.to(x0.device) for o in outs[:3])

    @staticmethod
    def backward(ctx, g_ypred, g_ypredvar, g_yconfvar):
        (x0,) = ctx.saved_tensors
        return _PredictVjpFn.apply(x0, g_ypred, g_ypredvar, g_yconfvar, ctx.model, ctx.x0c, ctx.jac), None


class _PredictVjpFn(torch.autograd.Function):
    """gx[i, l] = sum_a g_ypred[a, i] dypred[a, i, l] + (g_ypredvar + g_yconfvar)[a, i] dyconfvar[a, i, l] as a function of x0
    (through the Jacobians) and of the three incoming gradients.  Its backward contracts the Hessians of predict_hess(), fetched
    by ONE lcgp_predict_hess pass, and only here: a first-order use of predict_differentiable(order=2) never pays for them."""

    @staticmethod
    def forward(ctx, x0, g_ypred, g_ypredvar, g_yconfvar, model, x0c, jac):
        ctx.model, ctx.x0c, ctx.jac = model, x0c, jac
        ctx.x0_meta = (x0.dtype, x0.device, x0.shape)
        ctx.g_meta = [(g.dtype, g.device) for g in (g_ypred, g_ypredvar, g_yconfvar)]
        ctx.save_for_backward(g_ypred, g_ypredvar, g_yconfvar)
        gx = _vjp_first(g_ypred, g_ypredvar, g_yconfvar, *jac)
        return gx.reshape(x0.shape).to(device=x0.device, dtype=x0.dtype)

    @staticmethod
    def backward(ctx, gg):
        if torch.is_grad_enabled():         # a third derivative: the Hessians are constants, not a graph
            raise RuntimeError('LCGP.predict_differentiable(order=2) supports first and second derivatives only: triple '
                               'backward is not available; use predict_hess() for the Hessians')
        g_ypred, g_ypredvar, g_yconfvar = ctx.saved_tensors
        dyp, dycv = ctx.jac
        ggc = _cpu64(gg).reshape(dyp.shape[1:])
        gx0 = None
        if ctx.needs_input_grad[0]:
            d2yp, _, d2ycv = ctx.model.predict_hess(ctx.x0c)
            gp, gv = _cpu64(g_ypred), _cpu64(g_ypredvar) + _cpu64(g_yconfvar)
            gx0 = torch.einsum('ai,ailm,im->il', gp, d2yp, ggc) + torch.einsum('ai,ailm,im->il', gv, d2ycv, ggc)
            dt, dev, shape = ctx.x0_meta
            gx0 = gx0.reshape(shape).to(device=dev, dtype=dt)
        gp = torch.einsum('ail,il->ai', dyp, ggc)
        gv = torch.einsum('ail,il->ai', dycv, ggc)
        gouts = [v.to(device=dev, dtype=dt) for v, (dt, dev) in zip((gp, gv, gv), ctx.g_meta)]
        return (gx0, *gouts, None, None, None)


class _VrFn(torch.autograd.Function):
    """LCGP.variance_reduction_differentiable: forward = variance_reduction_grad()'s gain, backward = the per-candidate
    vector-Jacobian product with the saved gradient"""

    @staticmethod
    def forward(ctx, x_cand, model, kwargs):
        gain, dgain = model.variance_reduction_grad(x_cand.detach().cpu().to(torch.float64), **kwargs)
        ctx.meta = (x_cand.dtype, x_cand.device, x_cand.shape)
        ctx.dgain = dgain
        return gain.to(x_cand.device)

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():         # create_graph=True: the saved gradient is a constant, not a graph
            raise RuntimeError('LCGP.variance_reduction_differentiable supports first derivatives only: double backward '
                               '(create_graph=True) is not available; use variance_reduction_grad() for the gradient')
        dt, dev, shape = ctx.meta
        gx = torch.einsum('ac,acl->cl', _cpu64(g), ctx.dgain)
        return gx.reshape(shape).to(device=dev, dtype=dt), None, None


# rows of new inputs per pass of param_variance: bounds the (p, rows, P) Jacobian it holds (p P LAPLACE_CHUNK doubles)
LAPLACE_CHUNK = 256


def param_jacobians(ghat, gvar, dghat, dgvar, dnoise, W, noise, scale, offset, error_structure, jac=None, latent=False,
                    mean_only=False):
    """The host map of predict_param_grad, a pure function of the latent arrays: ghat, gvar (q, n0); dghat, dgvar (q, n0, d + 2)
    in each component's constrained [ell_0 .. ell_{d-1}, scale, nug]; dnoise (q, n0, p) = d ghat / d built noise parameters t_b;
    (W, noise, scale, offset) of LCGP._output_map() (W[k, a] ~ exp(t_a / 2), noise_a ~ exp(t_a)); error_structure: the sizes of
    the groups of outputs that share one lsigma2s.  Returns (dypred, dypredvar, dyconfvar), each (p, n0, P), P = q (d + 2) +
    groups, in the flat order [ell (q d, component-major), scale (q), nug (q), lsigma2s]:
        d ypred_a / d theta_k = scale_a W[k, a] d ghat_k       d yconfvar_a / d theta_k = scale_a^2 W[k, a]^2 d gvar_k
        d ypred_a / d t_b     = scale_a sum_k W[k, a] d_tb ghat_k + delta_ab (ypred_a - offset_a) / 2
        d yconfvar_a / d t_b  = delta_ab yconfvar_a            d ypredvar_a / d t_b adds delta_ab scale_a^2 noise_a
    the t_b folded through the groups.  jac (P,): d constrained / d unconstrained, multiplied onto the last axis (None: the
    constrained space).  latent=True: (dghat, dgvar) (q, n0, P) instead.  mean_only=True: dypred alone."""
    ghat, gvar, dghat, dgvar, dnoise = (np.asarray(a, F64) for a in (ghat, gvar, dghat, dgvar, dnoise))
    q, n0, m = dghat.shape
    d = m - 2
    es = np.asarray(error_structure, int)
    starts = np.r_[0, np.cumsum(es)[:-1]]
    o = q * m
    P = o + len(es)
    p = W.shape[1]
    cols = [np.r_[k * d + np.arange(d), q * d + k, q * d + q + k] for k in range(q)]

    def finish(*arrays):
        return tuple(a if jac is None else a * jac for a in arrays)

    if latent:
        lg, lv = np.zeros((q, n0, P), F64), np.zeros((q, n0, P), F64)
        for k in range(q):
            lg[k][:, cols[k]] = dghat[k]
            lv[k][:, cols[k]] = dgvar[k]
        lg[:, :, o:] = np.add.reduceat(dnoise, starts, axis=2)
        return finish(lg, lv)
    dyp = np.zeros((p, n0, P), F64)
    for k in range(q):
        dyp[:, :, cols[k]] = (scale * W[k])[:, None, None] * dghat[k][None]
    tb = np.einsum('ka,kib->aib', W, dnoise) * scale[:, None, None]
    half = 0.5 * scale[:, None] * (W.T @ ghat)                       # (ypred - offset) / 2
    tb[np.arange(p), :, np.arange(p)] += half
    dyp[:, :, o:] = np.add.reduceat(tb, starts, axis=2)
    if mean_only:
        return finish(dyp)[0]
    dyc = np.zeros((p, n0, P), F64)
    for k in range(q):
        dyc[:, :, cols[k]] = (scale * W[k])[:, None, None] ** 2 * dgvar[k][None]
    yconfvar = (W.T ** 2 @ gvar) * (scale ** 2)[:, None]
    group = np.repeat(np.arange(len(es)), es)                        # the group of output a
    dyv = dyc.copy()
    dyc[np.arange(p), :, o + group] = yconfvar
    dyv[np.arange(p), :, o + group] = yconfvar + (scale ** 2 * noise)[:, None]
    return finish(dyp, dyv, dyc)


def param_variance(ghat, dghat, dnoise, W, scale, error_structure, jac, cov):
    """yparamvar (p, n0) of predict_laplace: J cov J^T per output and new input, J = d ypred / d unconstrained vector
    (param_jacobians), formed over LAPLACE_CHUNK new inputs at a time"""
    p, n0 = W.shape[1], np.shape(ghat)[1]
    out = np.empty((p, n0), F64)
    zero = np.zeros(p, F64)
    for lo in range(0, n0, LAPLACE_CHUNK):
        hi = min(n0, lo + LAPLACE_CHUNK)
        # (gvar, dgvar, noise and offset do not enter the mean's Jacobian)
        J = param_jacobians(ghat[:, lo:hi], ghat[:, lo:hi], dghat[:, lo:hi], dghat[:, lo:hi], dnoise[:, lo:hi], W, zero, scale, zero,
                            error_structure, jac, mean_only=True)
        out[:, lo:hi] = np.einsum('aip,aip->ai', J @ cov, J)
    return out


class LaplaceResult:
    """What LCGP.laplace() returns: `hessian` (the unconstrained Hessian of the objective), its `eigenvalues` (ascending),
    `cov` = hessian^-1 and `stderr`, the delta-method standard errors of the constrained parameters shaped like get_param()."""

    def __init__(self, hessian, eigenvalues, cov, stderr):
        self.hessian, self.eigenvalues, self.cov, self.stderr = hessian, eigenvalues, cov, stderr

    def __repr__(self):
        return "LaplaceResult(P=%d, eigenvalues in [%.3e, %.3e])" % (len(self.eigenvalues), self.eigenvalues[0], self.eigenvalues[-1])


class ActiveSubspace:
    """What LCGP.active_subspace() returns, per selected output a (CPU float64 tensors): `matrix` (p_sel, d, d), the posterior
    expectation of sum_i w_i grad f_a grad f_a^T over the reference points, = `mean_part` (the gradients of the predictive
    mean) + `cov_part` (the emulator's own uncertainty about the gradient); `activity` (p_sel, d), its diagonal: the
    posterior-expected derivative-based sensitivity nu_l = E[(d f_a / d x_l)^2]; `eigenvalues` (p_sel, d), descending, and
    `eigenvectors` (p_sel, d, d) in columns, the largest-magnitude entry of each positive."""

    def __init__(self, matrix, mean_part, cov_part, activity, eigenvalues, eigenvectors):
        self.matrix, self.mean_part, self.cov_part = matrix, mean_part, cov_part
        self.activity, self.eigenvalues, self.eigenvectors = activity, eigenvalues, eigenvectors

    def __repr__(self):
        return "ActiveSubspace(outputs=%d, d=%d)" % tuple(self.activity.shape)


class MainEffects:
    """main_effects(): grid (d, G) on the raw input scale; mean, var (p_sel, d, G), the output as a function of input l alone,
    averaged over the others, and the posterior variance of that average; overall, overall_var (p_sel,), the average over all
    inputs (the Bayesian-quadrature mean of the output over the box); effect = mean - overall, the curve of a main-effect plot;
    effect_var (p_sel, d, G) its posterior variance var + overall_var - 2 cov(row, overall row) -- mean and overall are strongly
    correlated, so this is far below var + overall_var -- or None when main_effects() was not asked for it.  Small negative
    values from rounding are not clamped."""

    def __init__(self, grid, mean, var, overall, overall_var, effect_var=None):
        self.grid, self.mean, self.var, self.overall, self.overall_var = grid, mean, var, overall, overall_var
        self.effect = mean - overall[:, None, None]
        self.effect_var = effect_var

    def __repr__(self):
        return 'MainEffects(outputs=%d, d=%d, grid=%d)' % (self.mean.shape[0], self.mean.shape[1], self.mean.shape[2])


class SobolIndices:
    """sobol_indices(): first, total (p_sel, d), the first-order and total Sobol indices of every selected output (latent=True:
    of every latent component) for each input, of the posterior mean surface under the uniform measure on the box; variance
    (p_sel,), the variance V of that surface over the box, and mean (p_sel,), its average (main_effects().overall), on the raw
    output scale; first_variance = V_l (p_sel, d), the variance of the main effect of input l (first = V_l / V), and
    closed_variance = V_~l, the variance explained by all inputs but l (total = 1 - V_~l / V).  A surface that is constant over
    the box (V exactly 0) has NaN indices.  Rounding is not clamped: an index may leave [0, 1] by rounding error.
    With uncertainty=True also (None otherwise) the posterior EXPECTATIONS of the same variances under the emulator's own
    uncertainty at the fitted parameters: expected_variance (p_sel,) = E[V], expected_first_variance = E[V_l] and
    expected_closed_variance = E[V_~l] (p_sel, d), each the plug-in value plus a correction >= 0; first_expected = E[V_l] /
    E[V] and total_expected = 1 - E[V_~l] / E[V], ratios of expectations (NaN where E[V] is exactly 0); and
    integrated_variance (p_sel,), the posterior variance of the continuous surface averaged over the box.
    With order=2 also (None otherwise) the second-order terms: second_variance (p_sel, d, d), the variance
    V_lm = V^c_{lm} - V_l - V_m of the interaction of inputs l and m alone, and second = V_lm / V; both symmetric with a NaN
    diagonal.  With order=2 and uncertainty=True: expected_second_variance = E[V^c_{lm}] - E[V_l] - E[V_m] and second_expected,
    its ratio to E[V]."""

    def __init__(self, first, total, variance, mean, first_variance, closed_variance, expected_variance=None,
                 expected_first_variance=None, expected_closed_variance=None, first_expected=None, total_expected=None,
                 integrated_variance=None):
        self.first, self.total, self.variance, self.mean = first, total, variance, mean
        self.first_variance, self.closed_variance = first_variance, closed_variance
        self.expected_variance, self.integrated_variance = expected_variance, integrated_variance
        self.expected_first_variance, self.expected_closed_variance = expected_first_variance, expected_closed_variance
        self.first_expected, self.total_expected = first_expected, total_expected
        self.second = self.second_variance = self.expected_second_variance = self.second_expected = None

    def __repr__(self):
        return 'SobolIndices(outputs=%d, d=%d)' % tuple(self.first.shape)


class SobolSubsets:
    """sobol_subsets(): for the list `subsets` (tuples of input indices, as asked for) closed_variance (p_sel, S), the closed
    variance V^c_u = Var_{x_u} E[f | x_u] of the posterior mean surface over the box under the uniform measure -- what the
    inputs in u explain together, their interactions among themselves included -- and closed = V^c_u / V (NaN where V is
    exactly 0); variance (p_sel,) = V and mean (p_sel,), as in SobolIndices.  The empty subset has V^c exactly 0, the full one V.
    The total index of a group u is 1 - closed of its complement.  Rounding is not clamped.
    With uncertainty=True also (None otherwise) the posterior expectations expected_closed_variance = E[V^c_u] (p_sel, S),
    expected_variance = E[V] (p_sel,) and closed_expected = E[V^c_u] / E[V], a ratio of expectations."""

    def __init__(self, subsets, closed_variance, closed, variance, mean, expected_closed_variance=None, closed_expected=None,
                 expected_variance=None):
        self.subsets, self.closed_variance, self.closed, self.variance, self.mean = subsets, closed_variance, closed, variance, mean
        self.expected_closed_variance, self.closed_expected = expected_closed_variance, closed_expected
        self.expected_variance = expected_variance

    def __repr__(self):
        return 'SobolSubsets(outputs=%d, subsets=%d)' % tuple(self.closed_variance.shape)


class ShapleyEffects:
    """shapley_effects(): effects (p_sel, d), the Shapley effect of every input on every selected output: the average over all
    orders in which the inputs can be added of the closed variance input l adds, sum_{u without l} |u|! (d - |u| - 1)! / d!
    (V^c_{u + l} - V^c_u).  Unlike first and total indices the effects of an output add up to its variance V (variance,
    (p_sel,)), interactions shared equally among their inputs, and first_variance <= effect <= V - closed_variance of the
    others; shares = effects / V (NaN where V is exactly 0).  From the closed variances of all 2^d subsets, exact.
    With uncertainty=True also (None otherwise) effects_expected, the same sum over the posterior expectations E[V^c_u], which
    add up to expected_variance = E[V], and shares_expected = effects_expected / E[V]."""

    def __init__(self, effects, shares, variance, effects_expected=None, shares_expected=None, expected_variance=None):
        self.effects, self.shares, self.variance = effects, shares, variance
        self.effects_expected, self.shares_expected, self.expected_variance = effects_expected, shares_expected, expected_variance

    def __repr__(self):
        return 'ShapleyEffects(outputs=%d, d=%d)' % tuple(self.effects.shape)


class ConditionedLCGP:
    """What LCGP.condition() returns: a read-only view of the fitted model `base` conditioned on `m` new unique inputs
    `x_new` (raw scale, (m, d)) at the FIXED parameters, basis and standardisation of the fit.  It holds device state only
    (per local component U_n, L_S^-1 and v of DESIGN.md 4.13); the fitted model, its workspace and its plans are only read.
    predict(x0) equals, to rounding, predict(x0) of a model built on the augmented data at the same parameters.  The view
    goes stale when the base model's parameters change or the model is evaluated elsewhere: using it then raises RuntimeError."""

    def __init__(self, base, x_new, engine, state, ys=None, counts=None, float64=None):
        self.base, self.x_new, self.m = base, x_new, int(x_new.shape[0])
        self._engine, self._state = engine, state
        # what the float64 queries (sobol_indices, integrated_variance) rebuild a float32 view from: the standardised outputs
        # (p, m) and the counts (None: ones) condition() formed; float64: whether `state` is a float64 engine's (None: the base
        # model's dtype says)
        self._ys, self._counts = ys, counts
        self._float64 = (base._dtype == 'float64') if float64 is None else bool(float64)
        self._companion = None       # (state on the base model's float64 engine, built on first use) of a float32 view
        # (the view of a float32 model may live on its float64 engine, which does not follow the model's later evaluations:
        # the parameter vector itself is part of the check)
        self._u = base._get_flat().copy()

    def __repr__(self):
        return "ConditionedLCGP(m=%d, d=%d, base=%s n=%d)" % (self.m, int(self.base.d), self.base.submethod, int(self.base.n))

    def _require_current(self):
        base = self.base
        ok = base._aux_valid and np.array_equal(self._u, base._get_flat()) and \
            (self._engine is None or self._engine.is_current(self._state['theta']))
        if not ok:
            raise RuntimeError('this ConditionedLCGP is stale: the parameters of its base model changed (or the model was refit) '
                               'after condition(); call condition() again')

    def predict(self, x0, latent=False):
        """(ypred, ypredvar, yconfvar), each (p, n0) CPU float64 as LCGP.predict returns them, of the conditioned model at the
        raw-scale inputs x0; latent=True: (ghat, gvar), each (q, n0).  Rows of x0 that equal training inputs follow
        predict_grad()'s rule: the continuous prediction surface, no nugget term in the cross covariance (same = 0), also
        when x0 IS the training set.  Computed on the GPU in the dtype of the engine that holds the view's state (float32
        models: float32 products, ghat / gvar in double)."""
        base = self.base
        x0s = base._x0_2d(x0, 'x0')
        self._require_current()
        eng = self._engine
        loc = None if eng is None else eng.condition_predict_block(self._state, x0s).permute(1, 0, 2)      # (q_local, 2, n0)
        both = base._gather_components(loc, (2, x0s.shape[0]))
        ghat, gvar = both[:, 0], both[:, 1]
        if latent:
            return _t(ghat.copy()), _t(gvar.copy())
        return tuple(r.detach() for r in base._outputs(ghat, gvar))

    def _latent_predict_grad(self, x0):
        """ghat, gvar (q, n0) of the view and their Jacobians dghat, dgvar (q, n0, d) with respect to the STANDARDISED inputs,
        for raw-scale x0: LCGP._latent_predict_grad on the view (one reduction gathers the components over the ranks)"""
        base = self.base
        x0s = base._x0_2d(x0, 'x0')
        self._require_current()
        eng, st = self._engine, self._state
        return base._latent_grad_result(x0s, None if eng is None else lambda: eng.condition_predict_grad_block(st, x0s))

    def predict_grad(self, x0, latent=False):
        """LCGP.predict_grad() of the conditioned model: (dypred, dypredvar, dyconfvar), each (p, n0, d) CPU float64 on the raw
        input and output scales, the Jacobians of predict()'s outputs per point; dypredvar = dyconfvar.  latent=True:
        (ghat, gvar, dghat, dgvar), (q, n0) and (q, n0, d), on the standardised scale (ghat / gvar are predict(latent=True)'s).
        Equal, to rounding, to predict_grad() of a model built on the augmented data at the same parameters; nothing is
        refactorised.  The gradient of the continuous prediction surface (same = 0), also at training inputs
        and at the view's own new inputs.  RuntimeError when the view is stale."""
        ghat, gvar, dghat, dgvar = self._latent_predict_grad(x0)
        if latent:
            return _t(ghat.copy()), _t(gvar.copy()), _t(dghat.copy()), _t(dgvar.copy())
        dyp, dycv = self.base._output_jacobians(dghat, dgvar)
        return _t(dyp), _t(dycv.copy()), _t(dycv)

    def predict_differentiable(self, x0, order=1):
        """(ypred, ypredvar, yconfvar) (p, n0) as predict() returns them, float64 on x0's device, differentiable with respect to
        a requires_grad x0 (any device) through torch.autograd, as LCGP.predict_differentiable: the backward pass multiplies
        with the Jacobians of predict_grad() saved by the forward pass.  order=1: a double backward (create_graph=True)
        raises.  order=2: the backward pass is itself differentiable (torch.autograd.functional.hessian, gradgradcheck); the
        Hessians come from one predict_hess() pass of this view, made only when a double backward runs.  A third derivative
        raises."""
        if order not in (1, 2):
            raise ValueError('predict_differentiable: order must be 1 or 2, got %r' % (order,))
        x0 = x0 if isinstance(x0, torch.Tensor) else torch.as_tensor(np.asarray(x0, F64))
        return (_ViewPredictFn if order == 1 else _PredictFn2).apply(x0, self)

    def _latent_predict_hess(self, x0):
        """ghat, gvar, dghat, dgvar and the Hessians d2ghat, d2gvar (q, n0, d, d) of the view with respect to the STANDARDISED
        inputs, exactly symmetric: LCGP._latent_predict_hess on the view (lcgp_condition_predict_hess)"""
        base = self.base
        x0s = base._x0_2d(x0, 'x0')
        self._require_current()
        eng, st = self._engine, self._state
        return base._latent_hess_result(x0s, None if eng is None else lambda: eng.condition_predict_hess_block(st, x0s))

    def predict_hess(self, x0):
        """LCGP.predict_hess() of the conditioned model: (d2ypred, d2ypredvar, d2yconfvar), each (p, n0, d, d) CPU float64,
        exactly symmetric, on the raw input and output scales; d2ypredvar = d2yconfvar.  Equal, to rounding, to predict_hess()
        of a model built on the augmented data at the same parameters; nothing is refactorised.  The Hessian
        of the continuous prediction surface (same = 0), also at training inputs and at the view's own new inputs; the
        Matern-3/2 kernel has its kinks where a coordinate of x0 equals a training input's or one of the view's inputs'.
        RuntimeError when the view is stale."""
        _, _, _, _, d2ghat, d2gvar = self._latent_predict_hess(x0)
        d2yp, d2ycv = self.base._output_hessians(d2ghat, d2gvar)
        return _t(d2yp), _t(d2ycv.copy()), _t(d2ycv)

    def predict_grad_cov(self, x0, latent=False):
        """LCGP.predict_grad_cov() of the conditioned model: (p, n0, d, d) CPU float64, exactly symmetric, the posterior
        covariance of the gradient of the noise-free output at each new input GIVEN the base model's data and this view's new
        runs; latent=True: Gamma' (q, n0, d, d) in standardised inputs,
            Gamma'_k[i, l, m] = delta_lm c_k kappa / ell_l^2 - D_k (P'_il . P'_im) / (ell_l ell_m)
        with the rows P' of predict_hess() widened by the view's m columns (lcgp_condition_predict_gradcov).
        Gamma of the base model minus Gamma' is positive semidefinite: conditioning cannot add gradient uncertainty.
        RuntimeError when the view is stale."""
        base = self.base
        x0s = base._x0_2d(x0, 'x0')
        self._require_current()
        eng, st = self._engine, self._state
        return base._grad_cov_result(x0s, None if eng is None else lambda: eng.condition_grad_cov_block(st, x0s), latent)[1]

    def active_subspace(self, x_ref, weights=None, outputs=None):
        """LCGP.active_subspace() of the conditioned model: the ActiveSubspace over x_ref after the view's new runs; cov_part
        shrinks by what the runs settled.  Arguments, defaults, checks and the result are the model's."""
        def engine():
            self._require_current()
            return self._engine
        st = self._state
        return self.base._active_subspace(x_ref, weights, outputs, engine,
                                          lambda eng, x0s, w: eng.condition_grad_cov_block(st, x0s, w, per_point=False))

    def calibration(self, y_obs, obs_var, include_noise=True):
        """LCGP.calibration() of the conditioned model: a CalibrationTarget for one field observation whose loglik(theta),
        loglik_grad(theta), loglik_hess(theta) and loglik_differentiable(theta) draw ghat, gvar, their Jacobians and their
        Hessians from this view.  The output
        map is the base model's, so arguments, checks, errors and the folding into M, b, c0 and lognorm are exactly
        LCGP.calibration()'s.  The target is stale when the view is."""
        self._require_current()
        target = self.base.calibration(y_obs, obs_var, include_noise)
        target._view = self
        return target

    def predict_latent_cov(self, x0):
        """LCGP.predict_latent_cov() of the conditioned model: (q, n0, n0) CPU float64, the posterior covariance of the latent
        components over the raw-scale inputs x0 GIVEN the base model's data and this view's new runs,
            Sigma'_k = C00_k - D_k U_0 U_0^T - T T^T,   diag(Sigma'_k) = gvar'[k] of predict(latent=True)
        (the base model's kernels on rows widened by the view's m columns; nothing is refactorised).  Equal, to
        rounding, to predict_latent_cov() of a model built on the augmented data at the same parameters.  Rows of x0 that equal
        training inputs or the view's own inputs follow predict()'s rule (same = 0).  RuntimeError when the view is stale;
        ValueError when the buffers do not fit.  GPU memory: the base method's plus q_local n0pad K' elements, K' = npad + mpad."""
        base = self.base
        x0s = base._x0_2d(x0, 'x0')
        self._require_current()
        st = self._state
        return base._latent_cov(x0s, lambda: self._engine, lambda eng: eng.condition_predict_cov(st, x0s))

    def predict_jointcov(self, x0, outputs=None, include_noise=True):
        """LCGP.predict_jointcov() of the conditioned model: (len(outputs), n0, n0) CPU float64 on the raw output scale, with
        the base model's output map; its diagonal is this view's ypredvar (include_noise=True) or yconfvar (False).
        RuntimeError when the view is stale.  Memory as predict_latent_cov."""
        base = self.base
        x0s = base._x0_2d(x0, 'x0')
        self._require_current()
        st = self._state
        return base._jointcov(x0s, outputs, include_noise, lambda: self._engine, lambda eng: eng.condition_predict_cov(st, x0s))

    def sample(self, x0, size=1, seed=None, include_noise=True, jitter=1e-10):
        """LCGP.sample() of the conditioned model: (size, p, n0) CPU float64 draws of the outputs at x0 from the joint posterior
        given the base model's data and this view's new runs, g_k = ghat'_k + L_k eps_k with L_k L_k^T = Sigma'_k + jitter scale_k I.
        Seeding, the noise, the LinAlgError for a Sigma'_k + tau I that is not numerically positive definite and the memory
        beyond predict_latent_cov's are LCGP.sample()'s: the draws do not depend on how the components are spread over ranks.
        The factorisation runs in the dtype of the engine that holds the view's state.  RuntimeError when the view is stale."""
        base = self.base
        x0s = base._x0_2d(x0, 'x0')
        self._require_current()
        st = self._state
        return base._sample(x0s, size, seed, include_noise, jitter, lambda: self._engine,
                            lambda eng, S, seeds: eng.condition_sample_latent(st, x0s, S, seeds, jitter))

    def predict_marginal(self, x0, integrate, box=None, latent=False, cov_with=None):
        """LCGP.predict_marginal() of the conditioned model: (ypred, yconfvar[, ycov]), each (p, n0) CPU float64 (latent=True:
        (q, n0)), the box averages of the outputs GIVEN the base model's data and this view's new runs.  Averaging is linear, so
        it commutes with conditioning: the pass is predict()'s of this view with both row kernels replaced by their box-averaged
        instances (lcgp_condition_predict_marginal); nothing is refactorised.  Equal, to rounding, to
        predict_marginal() of a model built on the augmented data at the same parameters.  Arguments, defaults, checks, errors
        and shapes are LCGP.predict_marginal()'s; the default box is the bounding box of the BASE model's training inputs (the
        view's inputs may lie outside it).  RuntimeError when the view is stale."""
        base = self.base
        x0s, mask, bs, ref = base._marginal_arguments(x0, integrate, box, cov_with)
        self._require_current()
        eng = self._engine
        loc = None if eng is None else eng.predict_marginal_block(x0s, mask, bs, state=self._state, ref=ref).permute(1, 0, 2)
        return base._marginal_result(loc, x0s.shape[0], latent, ref is not None)

    def main_effects(self, grid=33, box=None, outputs=None, effect_var=False):
        """LCGP.main_effects() of the conditioned model: the main-effect curves after the view's new runs, from one
        predict_marginal() pass of this view.  Arguments, defaults, checks and the MainEffects returned are the model's."""
        return self.base._main_effects(self.predict_marginal, grid, box, outputs, effect_var)

    def _float64_state(self):
        """(engine, state) of this view in float64 (engine None on a rank without components): its own where that is a float64
        engine's; otherwise a companion state on the base model's float64 engine (one evaluation there when its factorisation
        is not current), built once from the same new inputs, standardised outputs and counts and kept with the view.  The
        view is stale when either engine no longer holds the parameters of its state."""
        self._require_current()
        if self._float64:
            return self._engine, self._state
        base = self.base
        if self._ys is None:
            raise RuntimeError('this ConditionedLCGP was built without the outputs of its new runs: a float32 view needs them for '
                               'its float64 queries; call condition() again')
        eng = base._ensure_aux64()
        if self._companion is None:
            xs = base._standardise_x0(_np(self.x_new))[0]
            self._companion = (base._agree(lambda: base._condition_state(eng, xs, self._ys, self._counts),
                                           failure='the conditioning matrix S_k of latent component(s) %s is not numerically positive '
                                                   'definite in float64 (info %s)', what='the float64 state of the view'),)
        state = self._companion[0]
        if eng is not None and not eng.is_current(state['theta']):
            raise RuntimeError('this ConditionedLCGP is stale: its float64 state belongs to other parameters; call condition() again')
        return eng, state

    def _mean_weights(self, eng, state):
        """(xa (N, d), w (q, N)): the N = n + m centres [x; xn] (standardised) and the weights of every component's mean surface
        over them, c sr_i z'_i on the training inputs and c w_a on the new ones.  Every rank gathers all q rows."""
        base = self.base
        n, m = int(base.n), self.m
        rows = np.zeros((len(base._local_ks), n + m), F64)
        if eng is not None:
            rows[:, :n], rows[:, n:] = eng.condition_mean_vectors(state)
        allv = _dist.gather_rows(rows, int(base.q), base._group, None if eng is None else eng.device)
        sr = np.sqrt(_np(base.r)) if base.submethod == 'rep' else np.ones(n, F64)
        scale_k, nug = base.lLmb0.numpy(), base.lnugGPs.numpy()
        c = scale_k * (1.0 - nug / (1.0 + nug))
        w = c[:, None] * np.concatenate([sr[None, :] * allv[:, :n], allv[:, n:]], axis=1)
        return np.vstack([base._x_train(), base._standardise_x0(_np(self.x_new))[0]]), w

    def _sobol_matrix(self, bs, eng, state):
        """LCGP._sobol_matrix with the view's covariance correction Q' over the n + m centres (lcgp_condition_sobol_matrix_pairs)"""
        base = self.base
        n, m = int(base.n), self.m

        def local_sums(loc, c, Dk, sr, ell):
            v = c[loc][:, None] * np.concatenate([np.broadcast_to(sr[None, :], (len(loc), n)), np.ones((len(loc), m), F64)], axis=1)
            return eng.condition_sobol_matrix_sums(state, v, ell[loc], bs, np.arange(len(loc)))

        return base._sobol_matrix(bs, eng, local_sums)

    def _sobol_context(self, box):
        """LCGP._sobol_context of the conditioned model: the centres [x; x_new], the view's mean weights and its matrix Q'"""
        base = self.base
        bs = base._marginal_box(box)
        eng, state = self._float64_state()
        xa, w = self._mean_weights(eng, state)
        n, m = int(base.n), self.m

        def matrix(masks):
            def local_sums(loc, c, Dk, sr, ell):
                v = c[loc][:, None] * np.concatenate([np.broadcast_to(sr[None, :], (len(loc), n)), np.ones((len(loc), m), F64)], axis=1)
                return eng.condition_sobol_matrix_subset_sums(state, v, ell[loc], bs, np.arange(len(loc)), masks)
            return base._sobol_subset_matrix(bs, masks, eng, local_sums)

        return eng, xa, w, bs, matrix

    def sobol_subsets(self, subsets, box=None, outputs=None, latent=False, uncertainty=False):
        """LCGP.sobol_subsets() of the conditioned model: the SobolSubsets GIVEN the base model's data and this
        view's new runs, equal to rounding to those of a model built on the augmented data at the same parameters.  The
        plug-in part is the vector pass on the n + m centres, uncertainty=True adds the matrix-weighted pass with the view's
        Q' (lcgp_condition_sobol_matrix_subset_pairs; E is formed once per component).  Arguments, checks, errors and fields
        are the model's.  RuntimeError when the view is stale."""
        base = self.base
        outputs = base._sobol_rows(outputs, latent)
        subsets, masks = base._subset_masks(subsets)
        return base._sobol_subsets_result(self._sobol_context(box), subsets, masks, outputs, latent, uncertainty)

    def shapley_effects(self, box=None, outputs=None, latent=False, uncertainty=False):
        """LCGP.shapley_effects() of the conditioned model; arguments, checks, errors and fields are the
        model's.  RuntimeError when the view is stale."""
        base = self.base
        outputs = base._sobol_rows(outputs, latent)
        base._shapley_check()
        return base._shapley_result(self._sobol_context(box), outputs, latent, uncertainty)

    def sobol_indices(self, box=None, outputs=None, latent=False, uncertainty=False, order=1):
        """LCGP.sobol_indices() of the conditioned model: the SobolIndices GIVEN the base model's data and this view's new runs,
        equal to rounding to those of a model built on the augmented data at the same parameters; nothing of size n is
        factorised.  The mean surface is a kernel expansion over the n + m centres [x; x_new], so the plug-in
        part is lcgp_sobol_pairs on them; uncertainty=True adds one matrix-weighted pass over the (n + m)^2 pairs per
        component, weighted by A^-1 in place plus the view's rank-m term (lcgp_condition_sobol_matrix_pairs).  Arguments,
        defaults, checks, errors, shapes and the fields are the model's; the default box is the base model's (main_effects()).
        Always float64: the view of a float32 model builds a float64 state once on the base model's float64 engine and keeps
        it.  Any number of ranks, the result does not depend on it.  RuntimeError when the view is stale.
        order=2 adds the second-order fields by one more pass over the d (d - 1) / 2 pair masks."""
        base = self.base
        base._sobol_order(order)
        outputs = base._sobol_rows(outputs, latent)
        bs = base._marginal_box(box)
        eng, state = self._float64_state()
        xa, w = self._mean_weights(eng, state)
        V, mean = base._sobol_mean(eng, xa, w, bs, latent)
        res = base._sobol_result(V, mean, outputs, latent, (lambda: self._sobol_matrix(bs, eng, state)) if uncertainty else None)
        if order == 2:
            base._sobol_second(res, self._sobol_context(box), outputs, latent, uncertainty)
        return res

    def integrated_variance(self, box=None, outputs=None, latent=False):
        """LCGP.integrated_variance() of the conditioned model: (p_sel,) the exact IMSPE after the view's new runs, what a
        sequential design is judged by, without a model on the augmented data.  The matrix-weighted pass of
        sobol_indices(uncertainty=True) alone and bitwise that call's integrated_variance; never above the base model's.
        RuntimeError when the view is stale."""
        base = self.base
        outputs = base._sobol_rows(outputs, latent)
        bs = base._marginal_box(box)
        eng, state = self._float64_state()
        _, iv, _ = self._sobol_matrix(bs, eng, state)
        return _t(base._latent_variance_to_rows(iv, latent)[outputs])

    def _design_arguments(self, xc_s, match):
        """what the design queries check beyond the base model's: the view is current, and on the rep path no candidate equals
        one of the view's new inputs"""
        self._require_current()
        base = self.base
        if match is not None:
            new = {row.tobytes() for row in np.ascontiguousarray(base._standardise_x0(_np(self.x_new))[0])}
            if any(row.tobytes() in new for row in np.ascontiguousarray(xc_s)):
                raise ValueError('a candidate equals one of the new inputs of this view (bitwise after standardisation): it would '
                                 'have to share a nugget with that run, and the view has no column to add replicates to; refit '
                                 'with the new runs instead')

    def variance_reduction(self, x_cand, x_ref=None, weights=None, outputs=None, replicates=1, latent=False):
        """LCGP.variance_reduction() of the conditioned model: for each candidate the drop of the weighted predictive variance
        over the reference set if the simulator ran there once more, GIVEN the base model's data and this view's new runs, at
        the fixed parameters.  Equal, to rounding, to variance_reduction() of a model built on the augmented data at the same
        parameters; nothing is refactorised (the base model's kernels on rows widened by the view's m columns).
        Arguments, checks, the output map and the full / rep rules are exactly LCGP.variance_reduction()'s; on the rep path a
        candidate equal to a BASE training input adds `replicates` runs to it.  A candidate bitwise equal (after
        standardisation) to one of the view's new inputs raises ValueError on the rep path (it would share a nugget with that
        run; refit for it); on the full path it is one more new row with its own nugget.  RuntimeError when the view is stale.
        GPU memory: the base method's with rows of K' = npad + mpad instead of npad (mpad = m rounded up to 128)."""
        base = self.base
        xc_s, xr_s, w, outputs, r, match = base._vr_arguments(x_cand, x_ref, weights, outputs, replicates)
        self._design_arguments(xc_s, match)
        eng = self._engine
        loc = base._agree(lambda: None if eng is None else
                          eng.condition_variance_reduction_block(self._state, xc_s, xr_s, w, match, r))
        R = base._gather_components(loc, (xc_s.shape[0],))
        if latent:
            return _t(R)
        W, _, scale, _ = base._output_map()
        delta = (W[:, outputs] ** 2).T @ R * (scale[outputs] ** 2)[:, None]
        return _t(delta)

    def variance_reduction_grad(self, x_cand, x_ref=None, weights=None, outputs=None, replicates=1, latent=False):
        """LCGP.variance_reduction_grad() of the conditioned model: (gain, dgain), CPU float64, this view's variance_reduction()
        and its gradient with respect to the candidates' locations on the RAW input scale -- what a continuous ALC search needs
        after condition().  Equal, to rounding, to variance_reduction_grad() of a model built on the augmented data at the same
        parameters; nothing of size n is factorised (lcgp_condition_vr_grad).  Arguments, checks, shapes, the
        output map and the full / rep rule for `replicates` are LCGP.variance_reduction_grad()'s.  x_ref and weights are
        CONSTANTS, also with x_ref=None.  Every candidate is a NEW input (predict_grad()'s rule): on the rep path a candidate
        equal to a base training input or to one of this view's own inputs gets the value and gradient of the continuous
        surface and is not refused; away from such candidates gain is bitwise variance_reduction()'s.  RuntimeError when the
        view is stale.  GPU memory: this view's variance_reduction()'s plus q_local min(n_cand, 2048) (n_ref + K' + 2 npad + 2 mpad)
        elements, K' = npad + mpad -- ValueError when it does not fit."""
        base = self.base
        xc_s, xr_s, w, outputs, r, _ = base._vr_arguments(x_cand, x_ref, weights, outputs, replicates)
        self._require_current()
        n_cand, d = xc_s.shape
        eng, st = self._engine, self._state
        return base._vr_grad_result(None if eng is None else
                                    lambda: eng.condition_variance_reduction_grad_block(st, xc_s, xr_s, w, r),
                                    n_cand, d, outputs, latent)

    def variance_reduction_differentiable(self, x_cand, x_ref=None, weights=None, outputs=None, replicates=1, latent=False):
        """LCGP.variance_reduction_differentiable() of the conditioned model: variance_reduction_grad()'s gain as a tensor on
        x_cand's device, differentiable with respect to a requires_grad x_cand through torch.autograd to first order (the
        backward pass multiplies with the gradient the forward pass saved); x_ref and weights are constants.  A double backward
        (create_graph=True) raises."""
        x_cand = x_cand if isinstance(x_cand, torch.Tensor) else torch.as_tensor(np.asarray(x_cand, F64))
        kwargs = dict(x_ref=x_ref, weights=weights, outputs=outputs, replicates=replicates, latent=latent)
        return _VrFn.apply(x_cand, self, kwargs)

    def select_batch(self, x_cand, size, x_ref=None, weights=None, outputs=None, replicates=1, return_scores=False):
        """LCGP.select_batch() of the conditioned model: the next batch GIVEN the base model's data and this view's new runs --
        same contract, same returns (idx, gain[, scores]), same checks as there and as variance_reduction() of this view.  On
        one rank the whole loop runs on the device; on several ranks each step is gathered and rank 0's argmax broadcast, as
        on the base model.  To go on after the batch has been run, condition the base model on all new runs so far."""
        base = self.base
        xc_s, xr_s, w, r, match, size, omega = base._select_arguments(x_cand, size, x_ref, weights, outputs, replicates)
        self._design_arguments(xc_s, match)
        eng, st = self._engine, self._state
        return base._select_run(
            eng, xc_s.shape[0], size, omega, return_scores,
            block=lambda: eng.condition_select_batch_block(st, xc_s, xr_s, w, match, r, size, omega[base._local_ks]),
            begin=lambda: eng.condition_select_begin(st, xc_s, xr_s, w, match, r, size),
            rows=lambda: eng.condition_select_rows(), condition=lambda j: eng.condition_select_condition(j))


class _ViewPredictFn(torch.autograd.Function):
    """ConditionedLCGP.predict_differentiable: _PredictFn on the view's latents -- forward = view.predict()'s outputs from one
    lcgp_condition_predict_grad pass, backward = the per-point vector-Jacobian product with the saved output Jacobians"""

    @staticmethod
    def forward(ctx, x0, view):
        base = view.base
        ghat, gvar, dghat, dgvar = view._latent_predict_grad(x0.detach().cpu().to(torch.float64))
        outs = base._outputs(ghat, gvar)
        dyp, dycv = base._output_jacobians(dghat, dgvar)
        ctx.x0_dtype, ctx.x0_device, ctx.x0_shape = x0.dtype, x0.device, x0.shape
        ctx.jac = (torch.as_tensor(dyp), torch.as_tensor(dycv))
        return tuple(o.to(x0.device) for o in outs[:3])

    @staticmethod
    def backward(ctx, g_ypred, g_ypredvar, g_yconfvar):
        if torch.is_grad_enabled():         # create_graph=True: the saved Jacobians are constants, not a graph
            raise RuntimeError('ConditionedLCGP.predict_differentiable supports first derivatives only: double backward '
                               '(create_graph=True) is not available; use predict_grad() for the Jacobians')
        return _PredictFn.backward(ctx, g_ypred, g_ypredvar, g_yconfvar)


class _CalibFn(torch.autograd.Function):
    """CalibrationTarget.loglik_differentiable: forward = loglik_grad()'s log likelihood, backward = the per-row product with
    the saved gradient"""

    @staticmethod
    def forward(ctx, theta, target):
        ll, dll = target.loglik_grad(theta.detach().cpu().to(torch.float64))
        ctx.meta = (theta.dtype, theta.device, theta.shape)
        ctx.dll = dll
        return ll.to(theta.device)

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():         # create_graph=True: the saved gradient is a constant, not a graph
            raise RuntimeError('CalibrationTarget.loglik_differentiable supports first derivatives only: double backward '
                               '(create_graph=True) is not available; use loglik_grad() for the gradient')
        dt, dev, shape = ctx.meta
        gx = _cpu64(g)[:, None] * ctx.dll
        return gx.reshape(shape).to(device=dev, dtype=dt), None


class _CalibFn2(torch.autograd.Function):
    """CalibrationTarget.loglik_differentiable(order=2): _CalibFn whose backward pass is itself a differentiable function
    (_CalibVjpFn) of theta and of the incoming gradient"""

    @staticmethod
    def forward(ctx, theta, target):
        thc = _cpu64(theta)
        ll, dll = target.loglik_grad(thc)
        ctx.target, ctx.thc, ctx.dll = target, thc, dll
        ctx.save_for_backward(theta)
        return ll.to(theta.device)

    @staticmethod
    def backward(ctx, g):
        (theta,) = ctx.saved_tensors
        return _CalibVjpFn.apply(theta, g, ctx.target, ctx.thc, ctx.dll), None


class _CalibVjpFn(torch.autograd.Function):
    """gx[i, l] = g[i] dll[i, l] as a function of theta (through the gradient) and of the incoming gradient g.  Its backward
    contracts the Hessian of loglik_hess(), fetched by ONE lcgp_predict_hess + lcgp_calib_hess_rows pass, and only here: a
    first-order use of loglik_differentiable(order=2) never pays for it."""

    @staticmethod
    def forward(ctx, theta, g, target, thc, dll):
        ctx.target, ctx.thc, ctx.dll = target, thc, dll
        ctx.meta = (theta.dtype, theta.device, theta.shape)
        ctx.g_meta = (g.dtype, g.device)
        ctx.save_for_backward(g)
        gx = _cpu64(g)[:, None] * dll
        return gx.reshape(theta.shape).to(device=theta.device, dtype=theta.dtype)

    @staticmethod
    def backward(ctx, gg):
        if torch.is_grad_enabled():         # a third derivative: the Hessian is a constant, not a graph
            raise RuntimeError('CalibrationTarget.loglik_differentiable(order=2) supports first and second derivatives only: '
                               'triple backward is not available; use loglik_hess() for the Hessian')
        (g,) = ctx.saved_tensors
        ggc = _cpu64(gg).reshape(ctx.dll.shape)
        gth = None
        if ctx.needs_input_grad[0]:
            d2ll = ctx.target.loglik_hess(ctx.thc)[2]
            dt, dev, shape = ctx.meta
            gth = (_cpu64(g)[:, None] * torch.einsum('ilm,im->il', d2ll, ggc)).reshape(shape).to(device=dev, dtype=dt)
        dt, dev = ctx.g_meta
        return gth, torch.einsum('il,il->i', ctx.dll, ggc).to(device=dev, dtype=dt), None, None, None


class CalibrationTarget:
    """What LCGP.calibration() returns: the log likelihood of ONE field observation y_obs of the p outputs as a function of the
    inputs theta, under the fitted emulator `model` at its current parameters,
        log p(y_obs | theta) = log N(y_obs; ypred(theta), Phi_s diag(gvar(theta)) Phi_s^T + noise + Sigma_obs),
    over the observed outputs.  Read-only: it holds the q x q matrix M, the q-vector b and two scalars into
    which everything output-sized was folded once, and a reference to the model, whose factorisation it reads.  It goes stale
    when the model's parameters change: every method then raises RuntimeError.  Nugget convention: predict_grad()'s (the
    continuous prediction surface, same = 0, training inputs included)."""

    def __init__(self, model, observed, M, b, c0, lognorm):
        self.model, self.observed = model, observed
        self.M, self.b, self.c0, self.lognorm = M, b, float(c0), float(lognorm)
        self._u = model._get_flat().copy()
        self._consts = {}               # device -> (M, b, 1 / input range) as tensors there
        self._view = None               # the ConditionedLCGP the latents are drawn from (ConditionedLCGP.calibration)

    def __repr__(self):
        return "CalibrationTarget(observed=%d of p=%d, q=%d)" % (int(self.observed.sum()), int(self.model.p), int(self.model.q))

    def _require_current(self):
        if self._view is not None:
            self._view._require_current()
        if not np.array_equal(self._u, self.model._get_flat()):
            raise RuntimeError('this CalibrationTarget is stale: the parameters of its model changed (or the model was refit) '
                               'after calibration(); call calibration() again')

    def _device_consts(self, dev):
        hit = self._consts.get(dev)
        if hit is None:
            m = self.model
            inv_range = 1.0 / (_np(m.x_max) - _np(m.x_min)).reshape(-1)
            hit = self._consts[dev] = tuple(torch.as_tensor(np.ascontiguousarray(a, F64)).to(dev)
                                            for a in (self.M, self.b, inv_range))
        return hit

    def _rows(self, theta, grad, want_sens=False):
        m = self.model
        x0s = m._x0_2d(theta, 'theta')
        self._require_current()
        blk, jac = m._calib_latent(x0s, grad, view=self._view)
        return m._calib_rows_device(blk, jac, *self._device_consts(blk.device), self.c0, self.lognorm, want_sens)

    def loglik(self, theta):
        """(n0,) CPU float64: log p(y_obs | theta[i]) for the rows of theta (n0, d) on the raw input scale"""
        return _t(self._rows(theta, False)[0])

    def loglik_grad(self, theta, latent=False):
        """(ll (n0,), dll (n0, d)), CPU float64: dll[i, l] = d ll[i] / d theta[i, l] on the raw input scale; ll is bitwise
        loglik(theta).  latent=True: additionally s, v (q, n0), the sensitivities d ll / d ghat and d ll / d gvar."""
        ll, dll, sens = self._rows(theta, True, latent)
        if latent:
            return _t(ll), _t(dll), _t(sens[0]), _t(sens[1])
        return _t(ll), _t(dll)

    def loglik_hess(self, theta, latent=False):
        """(ll (n0,), dll (n0, d), d2ll (n0, d, d)), CPU float64 on the raw input scale: d2ll[i, l, m] = d^2 ll[i] / d theta[i, l]
        d theta[i, m], exact and EXACTLY symmetric (the packed triangle of lcgp_calib_hess_rows, mirrored
        here); ll and dll are bitwise loglik_grad(theta)'s.  One lcgp_predict_hess pass (of the view for a view's target) and
        the row kernels.  latent=True: additionally s, v (q, n0) and B (n0, q, q) = Phi_s^T Sigma_i^-1 Phi_s, minus the Hessian
        of ll in ghat.  Nugget convention of predict_hess(): the continuous surface, also at training inputs and at a view's
        own inputs; the Matern-3/2 kernel has its kinks there."""
        m = self.model
        x0s = m._x0_2d(theta, 'theta')
        self._require_current()
        blk, jac, hess = m._calib_latent(x0s, 2, view=self._view)
        ll, dll, packed, sens, B = m._calib_hess_rows_device(blk, jac, hess, *self._device_consts(blk.device), self.c0,
                                                             self.lognorm, latent, latent)
        d2ll = m._unpack_lower(packed, x0s.shape[1])
        if latent:
            return _t(ll), _t(dll), _t(d2ll), _t(sens[0]), _t(sens[1]), _t(B)
        return _t(ll), _t(dll), _t(d2ll)

    def loglik_differentiable(self, theta, order=1):
        """(n0,) float64 on theta's device, differentiable with respect to a requires_grad theta (any device) through
        torch.autograd: the backward pass multiplies with the gradient of loglik_grad() saved by the forward pass.
        order=1: first derivatives only; a double backward (create_graph=True) raises.  order=2: the backward pass is itself
        differentiable (torch.autograd.functional.hessian, gradgradcheck); the Hessian comes from one loglik_hess() pass, made
        only when a double backward actually runs.  A third derivative raises."""
        if order not in (1, 2):
            raise ValueError('loglik_differentiable: order must be 1 or 2, got %r' % (order,))
        theta = theta if isinstance(theta, torch.Tensor) else torch.as_tensor(np.asarray(theta, F64))
        return (_CalibFn if order == 1 else _CalibFn2).apply(theta, self)


class LCGP:
    """
    Latent Component Gaussian Process (LCGP), MI355X hot path.

      - submethod='full': uses all observations (x, y)
      - submethod='rep' : groups replicated x rows, uses (x_unique, ybar) structures
    """

    # =============================================================================================
    # constructor (lcgp.py:31-222)
    # =============================================================================================
    def __init__(self, y=None, x=None, q=None, var_threshold=None, diag_error_structure=None,
                 parameter_clamp_flag=False, robust_mean=True, submethod='full', rep_standardize_ybar=True,
                 verbose=False, *, device=None, dtype='float64', process_group=None, kernel='matern32'):
        self.verbose = verbose
        # covariance kernel of the latent components: 'matern32' is the reference's only kernel (covmat.py:5-55); 'se', the
        # squared-exponential product kernel, is an extension (BASELINE.json's north star names it; parity unpinned), and so is
        # 'matern52': prod_j (1 + S_j + S_j^2 / 3) exp(-sum_j S_j) in the reference's convention for Matern-3/2 (no sqrt(5):
        # the textbook Matern-5/2 at lengthscale sqrt(5) ell_j), whose predictions are twice differentiable in x0
        if kernel not in ('matern32', 'se', 'matern52'):
            raise ValueError("kernel must be 'matern32', 'se' or 'matern52', got %r" % (kernel,))
        self.kernel = kernel
        self.robust_mean = robust_mean
        self.rep_standardize_ybar = rep_standardize_ybar
        self.parameter_clamp_flag = parameter_clamp_flag
        self._device = device
        # arithmetic of the device path: the reference is float64 only (lcgp.py:16); aliases are normalised ONCE here, every
        # later test compares with the normalised name
        try:
            self._dtype = {'float64': 'float64', 'f64': 'float64', 'float32': 'float32', 'f32': 'float32'}[str(dtype)]
        except KeyError:
            raise ValueError("dtype must be 'float64' or 'float32' (aliases 'f64', 'f32'), got %r" % (dtype,))
        self._engine64 = None            # float32 models: float64 engine for points where the float32 factorisation fails
        self.float32_fallback = True
        self.float32_fallbacks = 0
        # float32 models: after this many CONSECUTIVE evaluations that had to be repeated in float64 the model stops trying
        # float32 (every such point pays a wasted float32 evaluation first): the run continues on the float64 engine alone and
        # the float32 workspace is released.  info is all-reduced, so every rank counts the same and switches together.
        self.float32_switch_after = 3
        self._f32_consecutive = 0
        self._float64_only = False
        self._last_eval_float64 = False
        self._aux_engine = None          # the engine whose workspace holds the factorisation of _u_last
        self._group = process_group
        self._engine = None
        self._u_last = None          # unconstrained vector the factorisation in the workspace belongs to
        self._aux_override = {}
        self._np_cache = {}          # name -> ((id, version), numpy copy) of constant tensor attributes (_const_np)
        self._bounds_cache = None    # flat bounds of the three SoftClip blocks (_flat_transform)
        self._es_cache = None        # diag_error_structure as arrays (_run_path)
        self._jac_flat = None        # d constrained / d unconstrained of the evaluation in flight

        self.x = self._verify_data_types(x)
        self.y = self._verify_data_types(y)

        self.method = 'LCGP'
        if submethod not in ['full', 'rep']:
            raise ValueError('Invalid submethod. Choices are \'full\' or \'rep\'.')
        self.submethod = submethod
        self.submethod_loss_map = {'full': self.neglpost, 'rep': self.neglpost_rep}
        self.submethod_predict_map = {'full': self.predict_full, 'rep': self.predict_rep}

        if (q is not None) and (var_threshold is not None):
            raise ValueError('Include only q or var_threshold but not both.')
        self.q = q
        self.var_threshold = var_threshold

        self.n, self.d, self.p = self.verify_dim(self.y, self.x)
        self.x_orig = self.x
        self.y_orig = self.y

        self.x, self.x_min, self.x_max, _, self.xnorm = self.init_standard_x(self.x)

        self._rep_initialized = False
        if self.submethod == 'rep':
            (self.x_unique, self.x_unique_s, self.group_ids, self.r, self.R, self.ybar, self.ybar_s,
             self.ybar_mean, self.ybar_std, self.n, self.d, self.p) = self.preprocess()
            self._rep_initialized = True
        else:
            self.y, self.ymean, self.ystd, _ = self.init_standard_y(self.y)

        self.g, self.phi, self.diag_D, self.q = self.init_phi(var_threshold=var_threshold)
        if _dist.use_collectives(self._group):
            # the SVD basis is only defined up to column signs: all ranks must use rank 0's
            dev = torch.device(device) if device is not None else None
            self.phi = _t(_dist.broadcast_array(_np(self.phi), 0, self._group, dev))
            self.g = _t(_dist.broadcast_array(_np(self.g), 0, self._group, dev))
            self.diag_D = _t(_dist.broadcast_array(_np(self.diag_D), 0, self._group, dev))

        if diag_error_structure is None:
            self.diag_error_structure = [1] * int(self.p)
        else:
            self.diag_error_structure = diag_error_structure
        self.verify_error_structure(self.diag_error_structure, self.y)

        d_in = self.x.shape[1]
        self.lLmb = Parameter(np.ones((self.q, d_in)), 'Latent GP log-scale', SoftClip(1e-6, 1e4))
        self.lLmb0 = Parameter(np.ones(self.q), 'Latent GP log-lengthscale', SoftClip(1e-4, 1e4))
        self.lsigma2s = Parameter(np.ones(len(self.diag_error_structure)), 'Diagonal error log-variance')
        self.lnugGPs = Parameter(np.ones(self.q) * 1e-6, 'Latent GP nugget scale',
                                 SoftClip(np.exp(-16.0), np.exp(-2.0)))
        self.init_params()
        self.ghat = None
        self.gvar = None
        self.psi_c = None

    # =============================================================================================
    # display (lcgp.py:227-243)
    # =============================================================================================
    def __repr__(self):
        rows = []
        for par in (self.lLmb, self.lLmb0, self.lsigma2s, self.lnugGPs):
            tr = type(par.transform).__name__
            rows.append('\t\t%-32s %-9s shape=%-10s value=%s' % (
                par.name, tr, str(tuple(par.shape)), np.array2string(par.numpy(), precision=5, threshold=8)))
        return ('LCGP(\n'
                '\tsubmethod:\t{:s}\n'
                '\toutput dimension:\t{:d}\n'
                '\tnumber of latent components:\t{:d}\n'
                '\tparameter_clamping:\t{:s}\n'
                '\trobust_standardization:\t{:s}\n'
                '\tdiagonal_error structure:\t{:s}\n'
                '\tparameters:\t\n{}\n)').format(self.submethod, int(self.p), int(self.q),
                                                 str(self.parameter_clamp_flag), str(self.robust_mean),
                                                 str(self.diag_error_structure), '\n'.join(rows))

    # =============================================================================================
    # validation / transforms (lcgp.py:248-290)
    # =============================================================================================
    @staticmethod
    def _verify_data_types(t):
        if isinstance(t, torch.Tensor):
            t = t.detach().to('cpu', torch.float64)
        else:
            t = torch.as_tensor(np.asarray(t, dtype=F64))
        if t.ndim < 2:
            t = t.unsqueeze(1)
        return t

    def verify_dim(self, y, x):
        p, ny = y.shape[0], y.shape[1]
        nx, d = x.shape[0], x.shape[1]
        assert ny == nx, 'Number of inputs (x) differs from number of outputs (y), y.shape[1] != x.shape[0]'
        return (torch.tensor(nx, dtype=torch.int32), torch.tensor(d, dtype=torch.int32),
                torch.tensor(p, dtype=torch.int32))

    @staticmethod
    def verify_error_structure(diag_error_structure, y):
        assert sum(diag_error_structure) == y.shape[0], \
            'Sum of error_structure should equal the output dimension.'

    def tx_x(self, xs):
        return _t(_np(xs) * (_np(self.x_max) - _np(self.x_min)) + _np(self.x_min))

    def tx_y(self, ys):
        return _t(_np(ys) * _np(self.ystd) + _np(self.ymean))

    # =============================================================================================
    # standardisation (lcgp.py:295-324)
    # =============================================================================================
    @staticmethod
    def init_standard_x(x):
        xn = _np(x)
        x_max = xn.max(axis=0)
        x_min = xn.min(axis=0)
        xs = (xn - x_min) / (x_max - x_min)
        # mean of the strictly positive |x_i - x_i'| over ordered pairs (lcgp.py:304-309), from a sort:
        # sum_{i,i'} |x_i - x_i'| = 2 sum_k (2k - n + 1) x_(k);  #positive pairs = n^2 - sum_v count_v^2
        n = xn.shape[0]
        xnorm = np.zeros(xn.shape[1], F64)
        coef = 2.0 * np.arange(n) - n + 1.0
        for j in range(xn.shape[1]):
            s = np.sort(xn[:, j])
            _, cnt = np.unique(s, return_counts=True)
            npos = float(n) * n - float(np.sum(cnt.astype(F64) ** 2))
            xnorm[j] = 2.0 * float(coef @ s) / npos if npos > 0 else np.nan
        return _t(xs), _t(x_min), _t(x_max), x, _t(xnorm)

    def init_standard_y(self, y):
        yn = _np(y)
        if self.robust_mean:
            ycenter = _percentile50_nearest(yn)
            yspread = _percentile50_nearest(np.abs(yn - ycenter))
        else:
            ycenter = yn.mean(axis=1, keepdims=True)
            yspread = yn.std(axis=1, keepdims=True)
        ys = (yn - ycenter) / yspread
        return _t(ys), _t(ycenter), _t(yspread), y

    # =============================================================================================
    # replication preprocessing (lcgp.py:329-434)
    # =============================================================================================
    def _get_raw_xy(self, x_raw=None, y_raw=None):
        xr = _np(self.x_orig if x_raw is None else x_raw)
        yr = _np(self.y_orig if y_raw is None else y_raw)
        assert xr.ndim == 2, "x_raw must be (N, d)"
        assert yr.ndim == 2, "y_raw must be (p, N)"
        N, d = xr.shape
        p, Ny = yr.shape
        assert Ny == N, "y_raw columns must match x_raw rows"
        return xr, yr, N, d, p

    def _group_unique_rows_np(self, xr):
        x_unique, inverse, counts = np.unique(xr, axis=0, return_inverse=True, return_counts=True)
        return x_unique, np.asarray(inverse).reshape(-1), counts

    def _compute_ybar_np(self, yr, inverse, n):
        p, N = yr.shape
        sums = np.zeros((p, n), F64)
        np.add.at(sums.T, inverse, yr.T)
        return sums / np.bincount(inverse, minlength=n).astype(F64)[None, :]

    def _pack_replication_tensors(self, x_unique_np, inverse_np, r_np, ybar_np):
        x_unique_s = (x_unique_np - _np(self.x_min)) / (_np(self.x_max) - _np(self.x_min))
        r_t = torch.as_tensor(np.asarray(r_np, np.int32))
        return (_t(x_unique_np), _t(x_unique_s), torch.as_tensor(np.asarray(inverse_np, np.int32)), r_t,
                torch.diag(r_t.to(torch.float64)), _t(ybar_np))

    def _compute_center_spread_tf(self, Y):
        """(center, spread) per output row; non-positive spread -> 1 (lcgp.py:383-395).  Name kept for
        drop-in compatibility; nothing here is TensorFlow."""
        yn = _np(Y)
        if self.robust_mean:
            c = _percentile50_nearest(yn)
            s = _percentile50_nearest(np.abs(yn - c))
        else:
            c = yn.mean(axis=1, keepdims=True)
            s = yn.std(axis=1, keepdims=True)
        s = np.where(s > 0, s, 1.0)
        return _t(c), _t(s)

    def preprocess(self, y_raw=None, x_raw=None):
        """12-tuple of replication structures (lcgp.py:397-426)."""
        xr, yr, N, d, p = self._get_raw_xy(x_raw=x_raw, y_raw=y_raw)
        x_unique_np, inverse_np, counts_np = self._group_unique_rows_np(xr)
        n_unique = int(x_unique_np.shape[0])
        r_np = counts_np.astype(np.int32)
        ybar_np = self._compute_ybar_np(yr, inverse_np, n_unique)
        x_unique, x_unique_s, group_ids, r_t, R_t, ybar = self._pack_replication_tensors(
            x_unique_np, inverse_np, r_np, ybar_np)
        ybar_mean, ybar_std = self._compute_center_spread_tf(ybar)
        ybar_s = (ybar - ybar_mean) / ybar_std
        return (x_unique, x_unique_s, group_ids, r_t, R_t, ybar, ybar_s, ybar_mean, ybar_std,
                torch.tensor(n_unique, dtype=torch.int32), torch.tensor(d, dtype=torch.int32),
                torch.tensor(p, dtype=torch.int32))

    def _ensure_replication(self):
        if not self._rep_initialized:
            self.preprocess()
            self._rep_initialized = True

    # =============================================================================================
    # basis (lcgp.py:439-485)
    # =============================================================================================
    def _get_phi_input(self):
        if self.submethod != "rep":
            return self.y
        if getattr(self, "rep_standardize_ybar", True) and hasattr(self, "ybar_s"):
            return self.ybar_s
        if hasattr(self, "ybar"):
            return self.ybar
        return self.y

    def init_phi(self, var_threshold=None):
        y = _np(self._get_phi_input())
        n = int(self.n)
        p = int(self.p)
        left_u, singvals, _ = np.linalg.svd(y, full_matrices=False)
        if (self.q is None) and (var_threshold is None):
            q = p
        elif (self.q is None) and (var_threshold is not None):
            cumvar = np.cumsum(singvals ** 2) / np.sum(singvals ** 2)
            q = int(np.argmax(cumvar > var_threshold) + 1) if np.any(cumvar > var_threshold) else p
        else:
            q = int(self.q)
        assert left_u.shape[1] == min(n, p)
        phi = left_u[:, :q] * np.sqrt(float(n)) / singvals[:q]
        diag_D = np.sum(phi ** 2, axis=0)
        g = phi.T @ y
        if self.verbose:
            print("======= VARIANCE OF G ======")
            print(np.var(g, axis=1))
        return _t(g), _t(phi), _t(diag_D), q

    # =============================================================================================
    # parameters (lcgp.py:490-532)
    # =============================================================================================
    def init_params(self):
        x = _np(self.x)
        d = int(self.d)
        llmb = np.exp(0.5 * np.log(d) + np.log(np.std(x, axis=0)))
        y = _np(self.y)
        err_struct = self.diag_error_structure
        lsigma2_diag = np.zeros(len(err_struct), F64)
        col = 0
        for k in range(len(err_struct)):
            lsigma2_diag[k] = np.log(np.var(y[col:(col + err_struct[k])]))
            col += err_struct[k]
        self.lLmb.assign(np.tile(llmb, self.q).reshape((self.q, d)))
        self.lLmb0.assign(np.ones(self.q, F64))
        self.lnugGPs.assign(np.exp(-10.) * np.ones(self.q, F64))
        self.lsigma2s.assign(lsigma2_diag)
        self._invalidate()

    def get_param(self):
        """(lLmb (q,d), lLmb0 (q,), built_lsigma2s (p,), lnugGPs (q,)) -- constrained values."""
        built = np.repeat(self.lsigma2s.numpy(), np.asarray(self.diag_error_structure, int))
        return _t(self.lLmb.numpy()), _t(self.lLmb0.numpy()), _t(built), _t(self.lnugGPs.numpy())

    @property
    def trainable_variables(self):
        # tf.Module order: attribute names sorted -> lLmb, lLmb0, lnugGPs, lsigma2s
        return tuple(par.variable() for par in (self.lLmb, self.lLmb0, self.lnugGPs, self.lsigma2s))

    def _get_flat(self):
        return np.concatenate([self.lLmb.unconstrained.reshape(-1), self.lLmb0.unconstrained,
                               self.lnugGPs.unconstrained, self.lsigma2s.unconstrained])

    def _set_flat(self, u):
        u = np.asarray(u, F64)
        q, d, ns = self.q, int(self.d), len(self.diag_error_structure)
        a = q * d
        self.lLmb.unconstrained = u[:a].reshape(q, d).copy()
        self.lLmb0.unconstrained = u[a:a + q].copy()
        self.lnugGPs.unconstrained = u[a + q:a + 2 * q].copy()
        self.lsigma2s.unconstrained = u[a + 2 * q:a + 2 * q + ns].copy()
        self._aux_override = {}

    def _invalidate(self):
        self._u_last = None
        self._aux_override = {}

    @property
    def _aux_valid(self):
        """True when the workspace holds L, L^-1, A^-1, z of the CURRENT parameter vector (so `predict()` right after
        `fit()` does not pay another evaluation: L-BFGS-B's last evaluation normally is its final iterate)."""
        return self._u_last is not None and not self._aux_override and np.array_equal(self._u_last, self._get_flat())

    # =============================================================================================
    # the hot path (lcgp.py:537-666 + the gpflow/TF gradient tape)
    # =============================================================================================
    def _make_engine(self, dtype=None):
        """One rank's share of the path on the GPU (raises without a GPU: no CPU fallback)."""
        from .engine import HotPathEngine
        dtype = self._dtype if dtype is None else dtype
        rank, world = _dist.rank_world(self._group)
        self._local_ks = _dist.local_components(self.q, rank, world)
        if not self._local_ks:
            return None
        if self.submethod == 'rep':
            sr = np.sqrt(_np(self.r))
            ybar_used = _np(self.ybar_s if self.rep_standardize_ybar else self.ybar)
            return HotPathEngine(_np(self.x_unique_s), ybar_used * sr[None, :], sr, len(self._local_ks),
                                 dtype, self._device, comp_ids=self._local_ks, q_total=self.q, kernel=self.kernel)
        return HotPathEngine(_np(self.x), _np(self.y), None, len(self._local_ks), dtype, self._device,
                             comp_ids=self._local_ks, q_total=self.q, kernel=self.kernel)

    def _get_engine(self):
        if self._float64_only:           # a float32 model that has given up on float32 (float32_switch_after)
            return self._engine64
        if self._engine is None:
            self._engine = self._make_engine()
            self._path_consts()
        return self._engine

    def _ensure_engine64(self):
        """creates the float64 engine behind a float32 model's fallback if it is missing (none on a rank without components)"""
        if self._engine64 is None and self._get_engine() is not None:
            self._engine64 = self._make_engine('float64')

    def _path_consts(self):
        """Parameter-independent pieces of the objective."""
        rank, world = _dist.rank_world(self._group)
        self._local_ks = _dist.local_components(self.q, rank, world)
        if self.submethod == 'rep':
            r = _np(self.r)
            ybar_used = _np(self.ybar_s if self.rep_standardize_ybar else self.ybar)
            yeff = ybar_used * np.sqrt(r)[None, :]
            self._ysq = np.sum(yeff * yeff, axis=1)
            self._std = _np(self.ybar_std)[:, 0] if self.rep_standardize_ybar else np.ones(int(self.p), F64)
            self._sum_log_r = float(np.sum(np.log(r)))
        else:
            yn = _np(self.y)
            self._ysq = np.sum(yn * yn, axis=1)
            self._std = np.ones(int(self.p), F64)
            self._sum_log_r = 0.0

    def _const_np(self, name):
        """numpy view of a constant public attribute (a torch tensor: phi, diag_D), converted once per tensor VERSION -- the
        evaluation loop reads these at every step, and an in-place change by a caller (torch bumps `_version`) or a new
        tensor object invalidates the cached copy."""
        t = getattr(self, name)
        ver = getattr(t, '_version', None)
        hit = self._np_cache.get(name)
        # (the entry holds the tensor itself: an id() alone could be that of a freed tensor's successor)
        if hit is None or hit[0] is not t or hit[1] != ver:
            hit = (t, ver, _np(t))
            self._np_cache[name] = hit
        return hit[2]

    def _flat_transform(self):
        """constrained values and d constrained / d unconstrained of the three bounded blocks (lLmb, lLmb0, lnugGPs) in flat order,
        in ONE vectorised pass (the per-parameter `transform.forward` / `.dforward` calls cost ~40 us of numpy dispatch per
        evaluation, a tenth of a small configuration's step); same arithmetic element by element"""
        q, d = int(self.q), int(self.d)
        if not all(type(par.transform) is SoftClip for par in (self.lLmb, self.lLmb0, self.lnugGPs)):
            return None                  # (a caller has replaced a transform: the per-parameter path serves any bijector)
        trs = tuple(par.transform for par in (self.lLmb, self.lLmb0, self.lnugGPs))
        key = tuple((tr.low, tr.high) for tr in trs)
        if self._bounds_cache is None or self._bounds_cache[0] != key or any(a is not b for a, b in zip(self._bounds_cache[5], trs)):
            lo = np.concatenate([np.full(n_, par.transform.low, F64) for par, n_ in ((self.lLmb, q * d), (self.lLmb0, q), (self.lnugGPs, q))])
            hi = np.concatenate([np.full(n_, par.transform.high, F64) for par, n_ in ((self.lLmb, q * d), (self.lLmb0, q), (self.lnugGPs, q))])
            cc = np.concatenate([np.full(n_, par.transform._c, F64) for par, n_ in ((self.lLmb, q * d), (self.lLmb0, q), (self.lnugGPs, q))])
            self._bounds_cache = (key, lo, hi, hi - lo, cc, trs)        # (holds the transforms: no id() reuse)
        _, lo, hi, w, cc, _ = self._bounds_cache
        u = np.concatenate([self.lLmb.unconstrained.reshape(-1), self.lLmb0.unconstrained, self.lnugGPs.unconstrained])
        return softclip_flat(u, lo, hi, w, cc)

    def _theta_rows(self, sig_eff, constrained=None):
        if constrained is None:
            lLmb, lLmb0, lnug = self.lLmb.numpy(), self.lLmb0.numpy(), self.lnugGPs.numpy()
        else:
            q_, d_ = int(self.q), int(self.d)
            lLmb, lLmb0, lnug = constrained[:q_ * d_].reshape(q_, d_), constrained[q_ * d_:q_ * d_ + q_], constrained[q_ * d_ + q_:]
        phi, D = self._const_np('phi'), self._const_np('diag_D')
        ks = self._local_ks
        d = int(self.d)
        rows = np.empty((len(ks), d + 3 + int(self.p)), F64)
        if len(ks):
            rows[:, :d] = lLmb[ks]
            rows[:, d] = lLmb0[ks]
            rows[:, d + 1] = lnug[ks]
            rows[:, d + 2] = D[ks]
            rows[:, d + 3:] = phi[:, ks].T / sig_eff
        return rows

    def _zeros_on_device(self, shape):
        """A zero tensor where this rank's collectives run (a rank without components has no engine)."""
        if self._engine is not None:
            dev = self._engine.device
        elif _dist.backend_is_nccl(self._group):
            dev = torch.device(self._device) if self._device is not None else torch.device('cuda', torch.cuda.current_device())
        else:
            dev = torch.device('cpu')
        return torch.zeros(shape, dtype=torch.float64, device=dev)

    def _run_path(self):
        """One evaluation at the current parameters: returns (value, gradient w.r.t. the CONSTRAINED
        parameters in flat order lLmb, lLmb0, lnugGPs, lsigma2s).  Rep values already carry the 1/n.

        The rank's share [nll, info, g_lLmb (q d), g_lLmb0 (q), g_lnug (q), g_ls2_built (p)] is assembled ON THE
        DEVICE (lcgp_pack_partial), all-reduced in place (RCCL when the group's backend is nccl) and copied to
        the host once."""
        eng = self._get_engine()
        u_now = self._get_flat().copy()
        self._u_last = None
        n, d, p, q = int(self.n), int(self.d), int(self.p), int(self.q)
        es_key = tuple(self.diag_error_structure)
        if self._es_cache is None or self._es_cache[0] != es_key:
            es_arr = np.asarray(es_key, int)
            self._es_cache = (es_key, es_arr, np.r_[0, np.cumsum(es_arr)[:-1]])
        es, es_starts = self._es_cache[1], self._es_cache[2]
        ls2_b = np.repeat(self.lsigma2s.numpy(), es)
        flat = self._flat_transform()
        self._jac_flat = None if flat is None else flat[1]
        # a line-search trial may push lsigma2s far out: exp() overflowing to inf (psi / inf = 0) gives a huge finite value
        # that the optimiser rejects, as it does in the reference -- without numpy's warnings
        with np.errstate(over='ignore', divide='ignore'):
            sig_eff = np.exp(0.5 * ls2_b) / self._std
            rows = self._theta_rows(sig_eff, None if flat is None else flat[0]) if eng is not None else None
        # Lock-step guard: every rank runs its own L-BFGS-B on the all-reduced numbers, no iterate is ever broadcast.
        # A hash of the parameter vector this rank is evaluating rides in the last slot of the vector; after the sum it must
        # equal world_size x the local one (integers below 2^32: exact in float64), or some rank has drifted -- then
        # EVERY rank raises here, after the same collective, instead of waiting forever in a later one.
        guard = float(zlib.crc32(u_now.tobytes()))
        world = _dist.rank_world(self._group)[1]

        def reduced(engine):
            if engine is not None:
                part = engine.evaluate_partial(rows, guard)
            else:
                part = self._zeros_on_device(3 + q * d + 2 * q + p)
                part[-1] = guard
            v = _dist.reduce_to_host(part, self._group)
            if v[-1] != world * guard:
                raise RuntimeError('lcgp_amd: the ranks are no longer in lock-step (the parameter vectors they evaluated '
                                   'differ: guard sum %.17g != %d x %.17g); every rank stops here' % (v[-1], world, guard))
            return v[:-1]

        if self._float64_only:
            eng = self._engine64
        vec = reduced(eng)
        if self._float64_only:
            self._last_eval_float64 = True
        elif (vec[1] != 0 or not np.isfinite(vec[0])) and self._dtype == 'float32' and self.float32_fallback:
            # The float32 factorisation broke down (I + D_k C_k has a condition number beyond single precision somewhere
            # along a line search; the reference is float64 only).  The point is evaluated again in float64 -- on every
            # rank: info was all-reduced -- so the optimiser sees the objective there instead of an artificial value.
            self._ensure_engine64()
            self.float32_fallbacks += 1
            vec = reduced(self._engine64)
            self._last_eval_float64 = True
            # only a point that float64 CAN evaluate says something about float32: one that is not positive definite in
            # either precision (a line-search trial at a SoftClip edge) leaves the counter alone
            if vec[1] == 0 and np.isfinite(vec[0]):
                self._f32_consecutive += 1
            if self.float32_switch_after and self._f32_consecutive >= self.float32_switch_after:
                # float32 is not carrying this model: stay on the float64 engine, give the float32 workspace back
                self._float64_only = True
                self._engine = None
        else:
            self._last_eval_float64 = False
            self._f32_consecutive = 0
        if vec[1] != 0 or not np.isfinite(vec[0]):
            raise np.linalg.LinAlgError(
                'I + D_k C_k is not numerically positive definite at the current parameters (info=%g)' % vec[1])
        # the workspace of the engine that ran now holds L, L^-1, A^-1, z at these parameters
        self._u_last = u_now
        self._aux_engine = self._engine64 if self._last_eval_float64 else eng
        nll = vec[0] + 0.5 * np.sum(self._ysq / sig_eff ** 2) + n / 2.0 * np.sum(ls2_b - 2.0 * np.log(self._std)) \
            - 0.5 * p * self._sum_log_r
        g_b = vec[2 + q * d + 2 * q:] + n / 2.0 - 0.5 * self._ysq / sig_eff ** 2
        g_ls2 = np.add.reduceat(g_b, es_starts)
        grad = np.concatenate([vec[2:2 + q * d + 2 * q], g_ls2])
        if self.submethod == 'rep':
            nll, grad = nll / n, grad / n
        self._gc_last = grad             # (the constrained gradient at _u_last: the curvature term of loss_hessian's chain rule)
        return float(nll), grad

    def loss_and_grad(self, u=None):
        """NLL and d NLL / d unconstrained flat vector (what gpflow's Scipy wrapper hands L-BFGS-B)."""
        if u is not None:
            self._set_flat(u)
        val, g = self._run_path()
        if self._jac_flat is not None:       # the evaluation has formed it together with the constrained values (_flat_transform)
            g = g.copy()
            g[:self._jac_flat.size] *= self._jac_flat
            return val, g
        jac = np.concatenate([self.lLmb.transform.dforward(self.lLmb.unconstrained).reshape(-1),
                              self.lLmb0.transform.dforward(self.lLmb0.unconstrained),
                              self.lnugGPs.transform.dforward(self.lnugGPs.unconstrained),
                              np.ones(self.lsigma2s.size, F64)])
        return val, g * jac

    # =============================================================================================
    # exact Hessian of the objective in the parameters (beyond the reference, which would nest two tapes around neglpost)
    # =============================================================================================
    def _ensure_aux64(self):
        """the engine whose workspace holds the FLOAT64 factorisation of the current parameters (None on a rank without
        components): the one in the workspace when it is current and float64, otherwise one evaluation runs first (a float32
        model: on its float64 engine)"""
        eng = self._get_engine()
        if not (self._aux_valid and (self._dtype == 'float64' or self._last_eval_float64)):
            if self._dtype == 'float64' or self._float64_only:
                self._run_path()
            else:
                self._ensure_engine64()
                self._float64_only = True          # one evaluation on the float64 engine at the current parameters
                try:
                    self._run_path()
                finally:
                    self._float64_only = False
        return self._aux_engine if eng is not None else None

    def _hessian_blocks(self):
        """((q, (d + 2)^2 + (d + 2) p + p^2) numpy array of the per-component blocks of lcgp_nll_hess, constrained gradient)
        at the current parameters.  The factorisation in the workspace is reused when it is the current one and float64;
        otherwise one evaluation runs first (a float32 model: on its float64 engine).  Every rank computes its components'
        rows; one reduction of the zero-padded block gathers them (_gather_components), failures go through _agree."""
        aux = self._ensure_aux64()
        d, p = int(self.d), int(self.p)
        width = (d + 2) * (d + 2) + (d + 2) * p + p * p
        blocks = self._gather_components(self._agree(lambda: None if aux is None else aux.nll_hess_block()), (width,))
        return np.asarray(blocks, F64), self._gc_last

    def _hessian_constrained(self, blocks):
        """(P, P) Hessian in the constrained parameters from the per-component blocks: the q dense kernel blocks, the border
        and the noise corner (a sum over the components in ascending order, plus the term of the objective outside the
        components), both noise blocks folded through the error-structure groups; rep: the 1 / n of the objective."""
        n, d, p, q = int(self.n), int(self.d), int(self.p), int(self.q)
        m = d + 2
        es = np.asarray(self.diag_error_structure, int)
        starts = np.r_[0, np.cumsum(es)[:-1]]
        ns = len(es)
        o = q * m
        H = np.zeros((o + ns, o + ns), F64)
        sig_eff = np.exp(0.5 * np.repeat(self.lsigma2s.numpy(), es)) / self._std
        corner = np.diag(0.5 * self._ysq / sig_eff ** 2)
        for k in range(q):
            row = blocks[k]
            idx = np.r_[k * d + np.arange(d), q * d + k, q * d + q + k]
            H[np.ix_(idx, idx)] = row[:m * m].reshape(m, m)
            H[idx, o:] = border = np.add.reduceat(row[m * m:m * m + m * p].reshape(m, p), starts, axis=1)
            H[o:, idx] = border.T
            corner = corner + row[m * m + m * p:].reshape(p, p)
        H[o:, o:] = np.add.reduceat(np.add.reduceat(corner, starts, axis=0), starts, axis=1)
        if self.submethod == 'rep':
            H /= n
        return H

    def _flat_jacobians(self):
        """d constrained / d unconstrained and its derivative, in flat order (1 and 0 on lsigma2s, which has no bijector)"""
        pars = (self.lLmb, self.lLmb0, self.lnugGPs)
        ns = self.lsigma2s.size
        if self._flat_transform() is not None:
            _, lo, hi, w, cc, _ = self._bounds_cache
            u = np.concatenate([par.unconstrained.reshape(-1) for par in pars])
            j, j2 = softclip_flat2(u, lo, hi, w, cc)
        else:
            for par in pars:
                if not hasattr(par.transform, 'd2forward'):
                    raise NotImplementedError(
                        "loss_hessian(space='unconstrained') needs the second derivative of the bijector of %s: give %s a "
                        "d2forward(u) beside dforward(u), or ask for space='constrained'" % (par.name, type(par.transform).__name__))
            j = np.concatenate([par.transform.dforward(par.unconstrained).reshape(-1) for par in pars])
            j2 = np.concatenate([np.asarray(par.transform.d2forward(par.unconstrained), F64).reshape(-1) for par in pars])
        return np.concatenate([j, np.ones(ns, F64)]), np.concatenate([j2, np.zeros(ns, F64)])

    def loss_hessian(self, u=None, space='unconstrained'):
        """Exact Hessian of the objective (`loss()`) in the parameters: a (P, P) float64 numpy array in the flat order of
        loss_and_grad (lLmb, lLmb0, lnugGPs, lsigma2s), evaluated at `u` if given (the parameters are set to it, as
        loss_and_grad does).  space='unconstrained' (default): in the vector the optimiser sees, H_u = J H_c J + diag(g_c o
        d2forward), the matrix that goes with loss_and_grad's gradient; space='constrained': in the constrained values
        get_param() returns (lsigma2s per error-structure group).
        One GPU pass (lcgp_nll_hess) behind the factorisation of the current parameters, which is reused when the workspace
        holds it (right after fit() or loss_and_grad(u)) and only read: predict() stays valid.  Always float64: a
        dtype='float32' model evaluates once on its float64 engine at the current parameters and computes there, so its
        result is the float64 model's.  The result is exactly symmetric (one triangle mirrored, not averaged); kernel
        blocks of different components are exactly zero.  Multi-rank: each rank computes its components, one reduction
        assembles them, every rank returns the same matrix.  GPU memory: (d + 4) npad^2 doubles per component processed at a
        time -- ValueError when not even one fits."""
        if space not in ('unconstrained', 'constrained'):
            raise ValueError("space must be 'unconstrained' or 'constrained', not %r" % (space,))
        if u is not None:
            self._set_flat(u)
        if space == 'unconstrained':
            jac, jac2 = self._flat_jacobians()          # (before the GPU pass: a bijector without d2forward fails at once)
        blocks, g_c = self._hessian_blocks()
        H = self._hessian_constrained(blocks)
        if space == 'unconstrained':
            H = jac[:, None] * H * jac[None, :]
            H[np.diag_indices_from(H)] += g_c * jac2
        low = np.tril(H)
        return low + np.tril(H, -1).T

    def laplace(self):
        """Laplace approximation at the current parameters (call it after fit()): a LaplaceResult with
            hessian      (P, P) loss_hessian() in the unconstrained vector       eigenvalues  (P,) ascending
            cov          (P, P) its inverse, the covariance of the unconstrained vector
            stderr       standard errors of the CONSTRAINED parameters by the delta method (|d forward| sqrt(diag cov)), a
                         tuple shaped like get_param(): (lLmb (q, d), lLmb0 (q,), built lsigma2s (p,), lnugGPs (q,))
        On the rep path the objective carries 1 / n, so cov is n times the covariance of the parameters' posterior mode
        approximation of the unnormalised objective.  Raises numpy.linalg.LinAlgError naming the smallest eigenvalue when the
        Hessian is not positive definite (a flat valley or a point that is no minimum); nothing is jittered."""
        H = self.loss_hessian(space='unconstrained')
        ev, vec = np.linalg.eigh(H)
        if not np.all(np.isfinite(ev)) or ev[0] <= 0.0:
            raise np.linalg.LinAlgError('the Hessian of the objective is not positive definite at the current parameters: '
                                        'smallest eigenvalue %.6e (largest %.6e)' % (ev[0], ev[-1]))
        cov = (vec / ev[None, :]) @ vec.T
        cov = np.tril(cov) + np.tril(cov, -1).T
        jac, _ = self._flat_jacobians()
        se = np.abs(jac) * np.sqrt(np.diag(cov))
        q, d = int(self.q), int(self.d)
        es = np.asarray(self.diag_error_structure, int)
        stderr = (_t(se[:q * d].reshape(q, d)), _t(se[q * d:q * d + q]), _t(np.repeat(se[q * d + 2 * q:], es)),
                  _t(se[q * d + q:q * d + 2 * q]))
        return LaplaceResult(H, ev, cov, stderr)

    # =============================================================================================
    # parameter derivatives of the prediction and the Laplace-propagated parameter uncertainty (the reference: a gradient tape
    # around predict over the trainable variables)
    # =============================================================================================
    def _latent_param_grad(self, x0):
        """(ghat, gvar (q, n0), dghat, dgvar (q, n0, d + 2), dnoise (q, n0, p)) for raw-scale x0: the latent prediction and its
        derivatives in each component's CONSTRAINED kernel parameters [ell, scale, nug] and in the built noise parameters, from
        the float64 factorisation of the current parameters (lcgp_predict_paramgrad on the local components, ONE reduction of
        the zero-padded block gathers them, failures go through _agree).  x0 equal to the training set carries predict()'s
        nugget entry."""
        x0s, same = self._standardise_x0(x0)
        n0, m, p = x0s.shape[0], int(self.d) + 2, int(self.p)
        aux = self._ensure_aux64()

        def local():
            if aux is None:
                return None
            blk, dk, dn = aux.predict_paramgrad_block(x0s, same)
            return torch.cat([blk.permute(1, 2, 0), dk.permute(1, 2, 0, 3).reshape(blk.shape[1], n0, 2 * m), dn], dim=2)

        both = np.asarray(self._gather_components(self._agree(local), (n0, 2 + 2 * m + p)), F64)
        return both[:, :, 0], both[:, :, 1], both[:, :, 2:2 + m], both[:, :, 2 + m:2 + 2 * m], both[:, :, 2 + 2 * m:]

    def _param_grad_space(self, space):
        """d constrained / d unconstrained in flat order for space='unconstrained', None for 'constrained'"""
        if space not in ('unconstrained', 'constrained'):
            raise ValueError("space must be 'unconstrained' or 'constrained', not %r" % (space,))
        return self._flat_jacobians()[0] if space == 'unconstrained' else None

    def predict_param_grad(self, x0, space='unconstrained', latent=False):
        """Jacobians of predict()'s outputs with respect to the parameters, per new input:
            dypred[a, i, :] = d ypred[a, i] / d flat vector,   dypredvar, dyconfvar likewise      each (p, n0, P), CPU float64
        in the flat order of loss_and_grad (lLmb, lLmb0, lnugGPs, lsigma2s) and with loss_hessian's `space` convention:
        'unconstrained' (default) is the vector the optimiser sees, 'constrained' the values get_param() returns (lsigma2s per
        error-structure group).  latent=True: (dghat, dgvar) (q, n0, P) of the latent components instead, zero in the kernel
        parameters of the other components.
        One GPU pass (lcgp_predict_paramgrad) behind the factorisation of the current parameters, which is reused when the
        workspace holds it (right after fit() no extra evaluation) and only read.  Always float64: a dtype='float32' model
        evaluates once on its float64 engine and computes there.  x0 equal to the training set follows predict()'s branch
        (the nugget entry of the cross covariance).  Multi-rank: each rank computes its components, one reduction assembles
        them, every rank returns the same arrays.  GPU memory: one n x n matrix and two of min(n0, 2048) x n per component
        processed at a time -- ValueError when not even one fits."""
        jac = self._param_grad_space(space)
        ghat, gvar, dghat, dgvar, dnoise = self._latent_param_grad(x0)
        W, noise, scale, offset = self._output_map()
        out = param_jacobians(ghat, gvar, dghat, dgvar, dnoise, W, noise, scale, offset, self.diag_error_structure, jac, latent)
        return tuple(_t(a) for a in out)

    def predict_laplace(self, x0, cov=None):
        """predict() with the uncertainty of the fitted parameters propagated to first order:
            (ypred, ypredvar, yconfvar, yparamvar), each (p, n0), CPU float64
        yparamvar[a, i] = J Sigma J^T with J = d ypred[a, i] / d unconstrained vector (predict_param_grad) and Sigma the
        covariance of that vector: laplace().cov by default, or `cov`, a symmetric (P, P) array in the unconstrained space
        (from MCMC, say).  yparamvar is ADDED to both variances -- the first-order law of total variance, Var ~ E[var | theta] +
        Var[E | theta]; ypred is predict()'s, bit for bit.  A Hessian that is not positive definite raises laplace()'s
        LinAlgError.  The quadratic form is taken over chunks of new inputs: the (p, n0, P) Jacobian is never held whole."""
        ypred, ypredvar, yconfvar = self.predict(x0)          # (first: a float32 model predicts on its own engine)
        if cov is None:
            cov = self.laplace().cov
        cov = np.asarray(cov, F64)
        jac = self._param_grad_space('unconstrained')
        if cov.shape != (jac.size, jac.size):
            raise ValueError('predict_laplace: cov must be (%d, %d) in the unconstrained space, not %r' % (jac.size, jac.size, cov.shape))
        ghat, gvar, dghat, dgvar, dnoise = self._latent_param_grad(x0)
        W, noise, scale, offset = self._output_map()
        yparamvar = param_variance(ghat, dghat, dnoise, W, scale, self.diag_error_structure, jac, cov)
        pv = _t(yparamvar)
        return ypred, ypredvar + pv, yconfvar + pv, pv

    def fit(self, verbose=False):
        """scipy L-BFGS-B with default options on the unconstrained vector (lcgp.py:537-540).

        A trial point at which some I + D_k C_k is not numerically positive definite (possible in float32 or at the
        SoftClip edges) does not abort the fit: the reference's eigendecomposition form returns a non-finite value there,
        which leaves the line search nothing to interpolate with.  Here the closure reports a value clearly ABOVE the
        last successful one (f_last + 1 + |f_last|, zero gradient): the line search's interpolation then shortens the
        step and tries again (a far larger penalty would shrink the step to nothing and end the run with a spurious
        "converged").  `loss()` / `neglpost()` called directly still raise, and so does a failure at the very first
        evaluation (nothing to back off to).  (info is all-reduced, so every rank takes the same branch.)"""
        if self.submethod not in self.submethod_loss_map:
            raise ValueError("Invalid submethod. Choices are 'full' or 'rep'.")
        u0 = self._get_flat()
        last = []
        self._f32_consecutive = 0          # (a run of float64 repeats does not carry over from an earlier fit)
        if self._dtype == 'float32' and self.float32_fallback and not self._float64_only:
            # the float64 engine behind the fallback is created BEFORE the optimiser starts: if its workspace does not fit,
            # that surfaces here, on every rank, and not in the middle of a run that has already made progress
            self._ensure_engine64()

        def fun(u):
            try:
                val, g = self.loss_and_grad(u)
            except np.linalg.LinAlgError:
                if not last:
                    raise
                return last[0] + 1.0 + abs(last[0]), np.zeros_like(u)
            last[:] = [val]
            return val, g

        res = sopt.minimize(fun, u0, jac=True, method='L-BFGS-B')
        runs = [dict(nit=int(res.nit), nfev=int(res.nfev), fun=float(res.fun), success=bool(res.success), message=str(res.message))]
        if self._dtype == 'float32':
            # The float32 objective carries rounding noise of ~3e-7 relative, far above L-BFGS-B's default relative-reduction
            # test (2.2e-9): a run ends when one line search returns a step inside the noise.  Restarting from the point it
            # stopped at (fresh curvature memory) until a whole run gains less than 1e-6 relative carries on to where the
            # float64 run ends (tests/test_gpu_configs.py: final losses within 1e-3 relative on the configs[3] prefix).
            # `opt_result.restarts` keeps every run (iterations, evaluations, value, message); `nit` / `nfev` of the result are the
            # TOTALS over all runs, everything else describes the accepted (best) run.  The restarts stop after 30 runs or after
            # 15000 evaluations in all (SciPy's own default budget for one run).  A model that has switched to float64 on the
            # way (float32_switch_after) is restarted by the same rule: its curvature memory was built on float32 values.
            total_nit, total_nfev = res.nit, res.nfev
            for _ in range(30):
                if total_nfev >= 15000:
                    break
                last[:] = [res.fun]
                nxt = sopt.minimize(fun, res.x, jac=True, method='L-BFGS-B')
                runs.append(dict(nit=int(nxt.nit), nfev=int(nxt.nfev), fun=float(nxt.fun), success=bool(nxt.success),
                                 message=str(nxt.message)))
                total_nit += nxt.nit
                total_nfev += nxt.nfev
                gained = res.fun - nxt.fun
                if nxt.fun <= res.fun:
                    res = nxt
                if not gained > 1e-6 * abs(res.fun):
                    break
            if not self._float64_only and str(runs[-1]['message']).startswith('ABNORMAL') and self._engine64 is not None:
                # The last float32 run ended because its line search found no decrease -- the signature of the float32 noise
                # floor on a flat valley (the 4096-point prefix of configs[3]: float32 stops 1.5 % above the float64 optimum
                # with a projected gradient fifteen times larger).  The run carries on in float64 from there, on the engine
                # the repeats use; a float32 run that ends by a convergence test is accepted as it is (configs[3] at full
                # size: 0 repeats, final loss 3e-6 from the float64 fit's, 0.73 x its wall-clock).
                self._float64_only = True
                self._engine = None
                nxt = sopt.minimize(fun, res.x, jac=True, method='L-BFGS-B')
                runs.append(dict(nit=int(nxt.nit), nfev=int(nxt.nfev), fun=float(nxt.fun), success=bool(nxt.success),
                                 message=str(nxt.message), float64=True))
                total_nit += nxt.nit
                total_nfev += nxt.nfev
                if nxt.fun <= res.fun + 1e-6 * abs(res.fun):
                    res = nxt
            res.nit, res.nfev = total_nit, total_nfev
        res.restarts = runs
        res.float32_fallbacks = int(self.float32_fallbacks)
        res.float64_only = bool(self._float64_only)
        self._set_flat(res.x)
        self.opt_result = res
        return

    def loss(self):
        try:
            return self.submethod_loss_map[self.submethod]()
        except KeyError:
            raise ValueError("Invalid submethod. Choices are 'full' or 'rep'.")

    def neglpost(self):
        """lcgp.py:635-666 (value only; a 0-d float64 tensor)."""
        self._require_mode('full')
        val, _ = self._run_path()
        return torch.tensor(val, dtype=torch.float64)

    def neglpost_rep(self):
        """lcgp.py:554-630."""
        self._require_mode('rep')
        val, _ = self._run_path()
        return torch.tensor(val, dtype=torch.float64)

    def _require_mode(self, mode):
        built = 'rep' if hasattr(self, 'x_unique') and hasattr(self, 'ybar') else 'full'
        if mode != built:
            raise ValueError('model was preprocessed for submethod=%r' % built)

    # =============================================================================================
    # prediction (lcgp.py:671-930)
    # =============================================================================================
    def predict(self, x0, return_fullcov=False):
        x0 = self._verify_data_types(x0)
        try:
            predict_call = self.submethod_predict_map[self.submethod]
        except KeyError as e:
            print(e)
            raise KeyError('Invalid submethod.  Choices are \'full\' or \'rep\'.')
        result = predict_call(x0=x0, return_fullcov=return_fullcov)
        return tuple(r.detach() if r is not None else None for r in result)

    def compute_aux_predictive_quantities(self):
        """Factorise at the current parameters so that predict() can reuse L^-1, A^-1 and z (replaces the
        eigendecomposition caches of lcgp.py:685-726 / the Cholesky caches of 728-803)."""
        if hasattr(self, 'x_unique') and hasattr(self, 'ybar'):
            self._compute_aux_predictive_quantities_rep()
            return
        self._aux_override = {}
        self._run_path()

    def _compute_aux_predictive_quantities_rep(self):
        self._aux_override = {}
        self._run_path()
        ls2_b = _np(self.get_param()[2])
        sis = np.exp(-0.5 * ls2_b) * self._std
        phi = _np(self.phi)
        # the reference writes phi^T / sigma_inv_sqrt_used[:, None] (lcgp.py:754), which broadcasts only
        # when q == p (or 1); keep that expression there and fall back to the per-output scaling otherwise
        try:
            self.psi_c = _t(phi.T / sis[:, None])
        except ValueError:
            self.psi_c = _t(phi.T / sis[None, :])

    def _ensure_aux(self):
        eng = self._get_engine()
        # rank-independent test (all ranks must enter the collective together): is the factorisation in the
        # workspace the one of the current parameter vector?
        if not self._aux_valid:
            self.compute_aux_predictive_quantities()
        # (a float32 model whose factorisation failed at these parameters was evaluated by its float64 engine)
        return self._aux_engine if eng is not None else None

    def _latent_predict(self, x0):
        """ghat, gvar (q, n0) for raw-scale x0 (lcgp.py:822-838 / 877-900): the local components' rows are computed
        on the device, ONE reduction of the zero-padded block gathers them (_gather_components)."""
        x0s, same = self._standardise_x0(x0)
        eng = self._ensure_aux()
        loc = None if eng is None else eng.predict_block(x0s, same).permute(1, 0, 2)      # (q_local, 2, n0)
        both = self._gather_components(loc, (2, x0s.shape[0]))
        ghat, gvar = both[:, 0], both[:, 1]
        self.ghat, self.gvar = _t(ghat), _t(gvar)
        return ghat, gvar

    def predict_full(self, x0, return_fullcov=False):
        """lcgp.py:808-859."""
        return self._outputs(*self._latent_predict(x0), return_fullcov)

    def predict_rep(self, x0, return_fullcov=False):
        """lcgp.py:864-930."""
        return self._outputs(*self._latent_predict(x0), return_fullcov)

    def _outputs(self, ghat, gvar, return_fullcov=False):
        """latent (ghat, gvar) (q, n0) -> (ypred, ypredvar, yconfvar[, cov]) through _output_map(); cov is the (n0, p, p)
        output covariance on the full path and None on the rep path (lcgp.py:840-858 / 906-930)"""
        W, noise, scale, offset = self._output_map()
        predmean = W.T @ ghat
        confvar = gvar.T @ W ** 2
        predvar = confvar + noise
        ypred = predmean * scale[:, None] + offset[:, None]
        yconfvar = confvar.T * (scale ** 2)[:, None]
        ypredvar = predvar.T * (scale ** 2)[:, None]
        if not return_fullcov:
            return _t(ypred), _t(ypredvar), _t(yconfvar)
        if self.submethod == 'rep':
            return _t(ypred), _t(ypredvar), _t(yconfvar), None
        ch = np.einsum('kn,kp->npk', np.sqrt(gvar), W)
        cov = ch @ np.transpose(ch, (0, 2, 1)) + np.diag(noise)[None, ...]
        cov = cov * (scale[:, None] * scale[None, :])[None, ...]
        return _t(ypred), _t(ypredvar), _t(yconfvar), _t(cov)

    # the map's names per path, kept for callers of the earlier two-function form
    _outputs_full = _outputs_rep = _outputs

    # =============================================================================================
    # joint posterior covariance over new inputs and correlated draws (beyond the reference: its predict is marginal only)
    # =============================================================================================
    def _standardise_x0(self, x0):
        """x0 on the raw scale -> standardised x0 and whether it IS the training set (the nugget of the cross covariance)"""
        x0n = _np(self._verify_data_types(x0))
        x0s = (x0n - _np(self.x_min)) / (_np(self.x_max) - _np(self.x_min))
        xtrain = self._x_train()
        same = (x0s.shape == xtrain.shape) and bool(np.all(x0s == xtrain))
        return x0s, same

    def _x_train(self):
        """the standardised training inputs the engine holds: the unique inputs on the rep path"""
        return _np(self.x_unique_s if self.submethod == 'rep' else self.x)

    def _output_map(self):
        """(W, noise, scale, offset) with which _outputs turns latent (ghat, gvar) into outputs, the one place that knows the
        full / rep difference: mean_a = offset_a + scale_a sum_k W[k, a] g_k, noise variance scale_a^2 noise_a"""
        ls2_b = _np(self.get_param()[2])
        phi = _np(self.phi)
        p = int(self.p)
        if self.submethod == 'rep':
            use_std = getattr(self, "rep_standardize_ybar", True)
            scale = _np(self.ybar_std)[:, 0] if use_std else np.ones(p, F64)
            W = (phi * (np.sqrt(np.exp(ls2_b)) / scale)[:, None]).T
            noise = np.exp(ls2_b) / scale ** 2
            offset = _np(self.ybar_mean)[:, 0] if use_std else np.zeros(p, F64)
        else:
            W = phi.T * np.sqrt(np.exp(ls2_b))
            noise = np.exp(ls2_b)
            scale, offset = _np(self.ystd)[:, 0], _np(self.ymean)[:, 0]
        return W, np.broadcast_to(noise, (p,)).astype(F64), scale, offset

    def _agree(self, fn, jitter=None, failure=None, what='the joint covariance'):
        """runs this rank's share `fn()` and makes every rank raise together when any rank's share failed (a rank that raised
        alone would leave the others waiting in the next collective): the q info words of the factorisations and a
        ValueError flag are all-reduced first.  Returns fn()'s value.  `failure`: the message of the LinAlgError, formatted
        with the failing components and their info words (default: that of the joint covariance); `what`: what a rank that
        reports another rank's memory refusal says could not be allocated."""
        q = int(self.q)
        status = np.zeros(q + 1, F64)
        res, err = None, None
        try:
            res = fn()
        except np.linalg.LinAlgError as e:
            err = e
            for i, v in enumerate(e.info):
                status[self._local_ks[i]] = v
        except ValueError as e:
            err = e
            status[q] = 1.0
        if _dist.use_collectives(self._group):
            status = _dist.all_reduce_sum(status, self._group, None if self._engine is None else self._engine.device)
        if status[q] != 0:
            raise err if err is not None else ValueError('another rank could not allocate %s' % what)
        bad = [k for k in range(q) if status[k] != 0]
        if bad and failure is not None:
            raise np.linalg.LinAlgError(failure % (bad, [int(status[k]) for k in bad]))
        if bad:
            raise np.linalg.LinAlgError(
                'the posterior covariance Sigma_k + jitter scale_k I of latent component(s) %s is not numerically positive '
                'definite with jitter=%g (info %s): pass a larger jitter' % (bad, jitter, [int(status[k]) for k in bad]))
        return res

    def _gather_components(self, loc, shape):
        """(q, *shape) numpy array from this rank's (q_local, *shape) device tensor: ONE reduction of a zero-padded block
        (disjoint components: a sum is a gather)"""
        if not _dist.use_collectives(self._group):
            return loc.cpu().numpy()
        full = self._zeros_on_device((int(self.q),) + tuple(shape))
        if loc is not None:
            idx = torch.as_tensor(self._local_ks, dtype=torch.long, device=full.device)
            full.index_copy_(0, idx, loc.to(full.device))
        return _dist.reduce_to_host(full, self._group)

    def predict_latent_cov(self, x0):
        """(q, n0, n0) posterior covariance of the latent components over the new inputs x0 (raw scale):
            Sigma_k = C00_k - D_k (c0_k o sr) A_k^-1 (c0_k o sr)^T,   diag(Sigma_k) = gvar[k] of predict()
        formed on the GPU from the factorisation of the current parameters (right after fit() no extra evaluation).
        Memory: a second workspace of 3 q_local n0pad^2 elements per GPU (n0pad = n0 rounded up to 128; 3.2 GB at n0 = 4096,
        8 local components, float64) -- ValueError when it does not fit.  float32 models compute in float32."""
        x0s, same = self._standardise_x0(x0)
        return self._latent_cov(x0s, self._ensure_aux, lambda eng: eng.predict_cov(x0s, same))

    def _latent_cov(self, x0s, engine, cov):
        """predict_latent_cov of this model or of a view of it: engine() is the engine that answers (None on a rank without
        components), cov(engine) this rank's (q_local, n0, n0) share"""
        eng = engine()
        loc = self._agree(lambda: None if eng is None else cov(eng))
        return _t(self._gather_components(loc, (x0s.shape[0], x0s.shape[0])))

    def predict_jointcov(self, x0, outputs=None, include_noise=True):
        """(len(outputs), n0, n0) posterior covariance of each selected output over the new inputs x0, on the raw output scale:
            Cov(y_a(x0_i), y_a(x0_j)) = scale_a^2 (sum_k W[k, a]^2 Sigma_k[i, j] + [include_noise] noise_a delta_ij)
        with W, noise, scale what predict() uses (psi / exp(lsigma2s) / ystd on the full path, Psi / s_var / ybar_std on
        the rep path).  Its diagonal is predict()'s ypredvar (include_noise=True) or yconfvar (False).  outputs: indices
        (default: all p).  Memory as predict_latent_cov."""
        x0s, same = self._standardise_x0(x0)
        return self._jointcov(x0s, outputs, include_noise, self._ensure_aux, lambda eng: eng.predict_cov(x0s, same))

    def _jointcov(self, x0s, outputs, include_noise, engine, cov):
        """predict_jointcov of this model or of a view of it (engine, cov: as _latent_cov takes them): the output projection of
        the local components' covariances, one all-reduce, the noise on the diagonal"""
        n0 = x0s.shape[0]
        outputs = list(range(int(self.p))) if outputs is None else [int(a) for a in np.atleast_1d(outputs)]
        W, noise, scale, _ = self._output_map()
        w2 = W[:, outputs] ** 2                                  # (q, P)
        eng = engine()
        sig = self._agree(lambda: None if eng is None else cov(eng))
        part = self._zeros_on_device((len(outputs), n0, n0))
        if sig is not None:
            wl = torch.as_tensor(w2[self._local_ks].T.copy(), device=sig.device)       # (P, q_local)
            part = part.to(sig.device)
            part += torch.tensordot(wl, sig, dims=1)
            del sig
        cov = _dist.reduce_to_host(part, self._group)           # one all-reduce: the sum over the ranks' components
        if include_noise:
            idx = np.arange(n0)
            cov[:, idx, idx] += noise[outputs][:, None]
        cov *= (scale[outputs] ** 2)[:, None, None]
        return _t(cov)

    def sample(self, x0, size=1, seed=None, include_noise=True, jitter=1e-10):
        """(size, p, n0) draws of the outputs at the new inputs x0 (raw scale) from the joint posterior:
            g_k = ghat_k + L_k eps_k,   L_k L_k^T = Sigma_k + jitter scale_k I,   y = offset + scale (W^T g + [include_noise] sqrt(noise) eta)
        The normals of latent component k come from numpy's default_rng((seed, k)) with k the GLOBAL index, the observation
        noise from default_rng((seed, q)): the draws do not depend on how the components are spread over ranks.  seed=None:
        a fresh seed (rank 0's, on every rank).  A Sigma_k + tau I that is not numerically positive definite raises
        numpy.linalg.LinAlgError naming the component and the jitter (never NaNs); a larger jitter helps, in float32 models
        in particular (the factorisation runs in the dtype of the engine that holds the model's factorisation).
        Memory as predict_latent_cov, plus 2 q_local min(size, 4096) n0pad elements of scratch."""
        x0s, same = self._standardise_x0(x0)
        return self._sample(x0s, size, seed, include_noise, jitter, self._ensure_aux,
                            lambda eng, S, seeds: eng.sample_latent(x0s, S, seeds, jitter, same))

    def _sample(self, x0s, size, seed, include_noise, jitter, engine, draw):
        """sample of this model or of a view of it: engine() as _latent_cov takes it, draw(engine, S, seeds) this rank's
        (q_local, S, n0) latent draws; the seed broadcast, the seeding by GLOBAL component, the output map and the noise"""
        n0, q, p, S = x0s.shape[0], int(self.q), int(self.p), int(size)
        if S < 1:
            raise ValueError('size must be >= 1')
        if seed is None:
            fresh = float(int(np.random.SeedSequence().generate_state(1, np.uint64)[0]) >> 12)     # exact in float64
            seed = int(_dist.broadcast_array(np.array([fresh]), 0, self._group,
                                             None if self._engine is None else self._engine.device)[0])
        seed = int(seed)
        W, noise, scale, offset = self._output_map()
        eng = engine()
        seeds = [(seed, k) for k in self._local_ks] if eng is not None else []
        loc = self._agree(lambda: None if eng is None else draw(eng, S, seeds), jitter)
        g = self._gather_components(loc, (S, n0))
        ys = np.einsum('ka,ksi->sai', W, g)
        if include_noise:
            eta = np.random.default_rng((seed, q)).standard_normal((S, p, n0))
            ys += np.sqrt(noise)[None, :, None] * eta
        return _t(ys * scale[None, :, None] + offset[None, :, None])

    # =============================================================================================
    # conditioning on new runs without refactorising (beyond the reference)
    # =============================================================================================
    def condition(self, x_new, y_new):
        """A read-only view of this model conditioned on new runs: x_new (N, d) on the raw input scale, y_new (p, N) on the raw
        output scale.  Returns a ConditionedLCGP whose predict(x0) equals, to rounding, predict(x0) of a model built on the
        augmented data at the same parameters, basis phi and standardisation (no refit, no factorisation of size n): per
        latent component a rank-m correction from a block factorisation.  y_new goes through the stored
        standardisation (on the rep path the one of the replicate means).  Full path: every row is one run.  Rep path:
        bitwise-equal rows of x_new are grouped into m unique inputs with their counts and means.
        Raises ValueError for wrong shapes, non-finite values, N = 0, a new input bitwise equal (after standardisation) to a
        training input -- it would have to share a nugget with it -- and, on the full path, bitwise-duplicate rows inside
        x_new: refit for those.  A conditioning matrix S_k that is not numerically positive definite raises
        numpy.linalg.LinAlgError naming the component (nothing is jittered); a float32 model builds the view once more on
        its float64 engine first (counted in float32_fallbacks, the one thing condition() changes on the model).  The fitted model, its workspace and its plans are only read: every other query keeps
        working on the base model, and predict() of the base model is bitwise unchanged."""
        self._require_mode(self.submethod)
        d, p = int(self.d), int(self.p)
        xn = _np(self._verify_data_types(x_new))
        if isinstance(y_new, torch.Tensor):
            yn = y_new.detach().to('cpu', torch.float64).numpy()
        else:
            yn = np.asarray(y_new, F64)
        if xn.ndim != 2 or xn.shape[1] != d:
            raise ValueError('x_new must have shape (N, %d), got %s' % (d, tuple(xn.shape)))
        if xn.shape[0] < 1:
            raise ValueError('x_new holds no rows (N = 0)')
        if yn.ndim != 2 or yn.shape != (p, xn.shape[0]):
            raise ValueError('y_new must have shape (%d, N = %d), got %s' % (p, xn.shape[0], tuple(yn.shape)))
        if not np.all(np.isfinite(xn)) or not np.all(np.isfinite(yn)):
            raise ValueError('x_new and y_new must be finite')
        if self.submethod == 'rep':
            xu, inverse, counts = self._group_unique_rows_np(xn)
            ybar = self._compute_ybar_np(yn, inverse, xu.shape[0])
            if self.rep_standardize_ybar:
                ybar = (ybar - _np(self.ybar_mean)) / _np(self.ybar_std)
            ys, r = ybar, counts.astype(F64)
        else:
            xu, r = xn, None
            ys = (yn - _np(self.ymean)) / _np(self.ystd)
        xu_s = self._standardise_x0(xu)[0]
        if r is None and len({row.tobytes() for row in np.ascontiguousarray(xu_s)}) != xu_s.shape[0]:
            raise ValueError('x_new holds duplicate rows (bitwise equal after standardisation): two copies of one input would '
                             'have to share a nugget; refit with the new runs instead')
        train = {row.tobytes() for row in np.ascontiguousarray(self._x_train())}
        if any(row.tobytes() in train for row in np.ascontiguousarray(xu_s)):
            raise ValueError('a row of x_new equals a training input (bitwise after standardisation): it would have to share a '
                             'nugget with it; refit with the new runs instead')
        eng = self._ensure_aux()
        failure = ('condition(): the conditioning matrix S_k of latent component(s) %s is not numerically positive definite at '
                   'the current parameters (info %s)')

        def begin(e):
            return self._condition_state(e, xu_s, ys, r)
        float64 = self._dtype == 'float64' or bool(self._last_eval_float64)      # (the same on every rank)
        try:
            state = self._agree(lambda: begin(eng), failure=failure, what='the conditioned view')
        except np.linalg.LinAlgError:
            if not (self._dtype == 'float32' and self.float32_fallback) or self._last_eval_float64:
                raise
            # float32 gave up (every rank: the failure was agreed on): the view is built once on the float64 engine, evaluated
            # at the current parameters; the base model keeps answering from its own float32 factorisation
            keep = (self._aux_engine, self._last_eval_float64, self._gc_last, self._float64_only)
            self._ensure_engine64()
            self.float32_fallbacks += 1
            self._float64_only = True
            try:
                self._run_path()
                eng = self._aux_engine if self._engine64 is not None else None
            finally:
                self._aux_engine, self._last_eval_float64, self._gc_last, self._float64_only = keep
            state = self._agree(lambda: begin(eng), failure=failure + ', in float64 either', what='the conditioned view')
            float64 = True
        return ConditionedLCGP(self, _t(xu), eng, state, ys=ys, counts=r, float64=float64)

    def _condition_state(self, e, xu_s, ys, r):
        """this rank's state of a view on the engine e (None: a rank without components) for the standardised new inputs xu_s,
        their standardised outputs ys (p, m) and counts r (None: ones)"""
        if e is None:
            return None
        d = int(self.d)
        rows = e._theta_last
        # the latent observation of each new input: the entry of b_k the evaluation would form for it, over D_k sr_i
        # (one product per component: a row's sum must not depend on how many components the rank holds)
        t = np.stack([(row[d + 3:] @ ys) / row[d + 2] for row in rows])
        return e.condition_begin(xu_s, t, r)

    # =============================================================================================
    # closed-form cross-validation at fixed parameters (beyond the reference)
    # =============================================================================================
    def _cv_labels(self, folds, seed):
        """fold labels (n,) over the training inputs (the unique inputs on the rep path) -> (labels, fold_ptr, fold_idx)"""
        n = self._cv_n()
        if np.ndim(folds) == 0:
            if isinstance(folds, (bool, np.bool_)) or not float(folds).is_integer():
                raise ValueError('folds must be an int F or an array of %d integer labels' % n)
            F = int(folds)
            if F < 1 or F > n:
                raise ValueError('the number of folds must be in [1, %d], got %d' % (n, F))
            labels = np.random.default_rng(seed).permutation(n) % F
        else:
            labels = np.asarray(folds)
            if labels.shape != (n,):
                raise ValueError('fold labels must have shape (%d,) (one per %s), got %s'
                                 % (n, 'unique input' if self.submethod == 'rep' else 'training input', labels.shape))
            if labels.dtype.kind not in 'iu' and not (labels.dtype.kind == 'f' and np.all(np.isfinite(labels))
                                                      and np.all(labels == np.round(labels))):
                raise ValueError('fold labels must be integers')
            labels = labels.astype(np.int64)
        _, inv = np.unique(labels, return_inverse=True)
        inv = inv.reshape(-1)
        F = int(inv.max()) + 1
        if F * int(self.q) > 65535:
            raise ValueError('at most %d folds with q = %d latent components' % (65535 // int(self.q), int(self.q)))
        order = np.argsort(inv, kind='stable')          # ascending input index within each fold
        fold_ptr = np.r_[0, np.cumsum(np.bincount(inv, minlength=F))]
        return labels, fold_ptr, order

    def _cv_latent(self, fn):
        """runs the engine call `fn(eng)` -> (2, q_local, n) [ghat; gvar] (and extras) on the factorisation of the current
        parameters, with the ranks agreeing on failures; a float32 model whose fold factorisation fails is evaluated again on
        its float64 engine, as a failed float32 evaluation is"""
        eng = self._ensure_aux()
        failure = ('cross-validation: a fold matrix a_k[B, B] of latent component(s) %s is not numerically positive definite '
                   'at the current parameters (info %s)')
        try:
            return self._agree(lambda: None if eng is None else fn(eng), failure=failure), eng
        except np.linalg.LinAlgError:
            if not (self._dtype == 'float32' and self.float32_fallback) or self._last_eval_float64:
                raise
        # float32 gave up: the float64 engine evaluates the current parameters (every rank: the failure was agreed on)
        self._ensure_engine64()
        self.float32_fallbacks += 1
        only = self._float64_only
        self._float64_only = True
        try:
            self._run_path()
        finally:
            self._float64_only = only
        eng = self._aux_engine if self._engine64 is not None else None
        return self._agree(lambda: None if eng is None else fn(eng), failure=failure + ', in float64 either'), eng

    def predict_loo(self):
        """Leave-one-out predictions (ypred, ypredvar, yconfvar), each (p, n) -- (p, n_unique) on the rep path -- at FIXED
        parameters: column i is what predict(x[i:i+1]) returns from the model conditioned on every other input, with the same
        hyper-parameters, noise, basis phi and standardisation (no nugget in the cross covariance, as for a new input).  In
        closed form from the factorisation of the current parameters (lcgp_loo; right after fit() or predict() no extra
        evaluation), in the engine's dtype: ghat_i = (b_i - z_i / a_ii) / (D s_i), gvar_i = (1 / a_ii - 1) / (D s_i^2).
        On the rep path input i is a unique input with all its replicates left out, and ypredvar is the variance of ONE new
        replicate, as in predict(): compare against ybar[:, i] with yconfvar + noise / r_i.  On the full path duplicated rows
        are left out one at a time (the copy stays in): group them with predict_cv labels, or use submethod='rep'.
        self.ghat / self.gvar are left untouched."""
        n = self._cv_n()
        blk, _ = self._cv_latent(lambda e: e.loo_block())
        loc = None if blk is None else blk.permute(1, 0, 2)              # (q_local, 2, n)
        both = self._gather_components(loc, (2, n))
        return self._outputs(both[:, 0], both[:, 1])

    def _cv_n(self):
        return self._x_train().shape[0]

    def predict_cv(self, folds, seed=0, return_latent_cov=False):
        """k-fold cross-validation predictions (ypred, ypredvar, yconfvar), each (p, n) -- (p, n_unique) on the rep path --
        at FIXED parameters: the inputs of each fold are predicted by the model conditioned on all other folds, as
        predict_loo() does for single inputs (same hyper-parameters, basis and standardisation; no refit).
          folds: an int F (labels default_rng(seed).permutation(n) % F) or an array of n integer labels, one per training
                 input (per unique input on the rep path).  The labels used are kept as self.cv_labels.
          return_latent_cov: also a list of F tensors (q, m_f, m_f), the latent posterior covariance of each fold over its
                 inputs in ascending order (the prior variance, nugget included, on the diagonal, as predict_latent_cov).
        Folds of one input each reproduce predict_loo(); one fold holding every input gives the prior.  GPU memory: 3 q_local
        F mpad^2 elements (mpad = the largest fold rounded up to 128) -- ValueError when it does not fit.  A float32 model
        computes in float32 and repeats the call in float64 if a fold matrix is not numerically positive definite there.
        self.ghat / self.gvar are left untouched."""
        labels, fold_ptr, fold_idx = self._cv_labels(folds, seed)
        n, q = len(labels), int(self.q)
        sizes = np.diff(fold_ptr)
        res, _ = self._cv_latent(lambda e: e.cv_block(fold_ptr, fold_idx, return_latent_cov))
        loc = None
        if res is not None:
            blk, covs = res if return_latent_cov else (res, [])
            # predictions and every fold's covariance in ONE reduction: (q_local, 2 n + sum m_f^2)
            loc = torch.cat([blk.permute(1, 0, 2).reshape(blk.shape[1], -1)] + [c.reshape(c.shape[0], -1) for c in covs], dim=1)
        width = 2 * n + (int(np.sum(sizes * sizes)) if return_latent_cov else 0)
        flat = self._gather_components(loc, (width,))
        self.cv_labels = labels
        both = flat[:, :2 * n].reshape(q, 2, n)
        outs = self._outputs(both[:, 0], both[:, 1])
        if not return_latent_cov:
            return outs
        lat, off = [], 2 * n
        for m in sizes:
            lat.append(_t(flat[:, off:off + m * m].reshape(q, m, m)))
            off += m * m
        return (*outs, lat)

    # =============================================================================================
    # integrated variance reduction for choosing new design points (beyond the reference)
    # =============================================================================================
    def _vr_arguments(self, x_cand, x_ref, weights, outputs, replicates):
        """the checks and conventions variance_reduction() and select_batch() share: standardised candidates and reference points
        (None: the candidates), normalised weights, output indices, r and the rep path's match of candidates to training inputs"""
        d = int(self.d)
        xc = _np(self._verify_data_types(x_cand))
        if xc.ndim != 2 or xc.shape[1] != d or xc.shape[0] < 1:
            raise ValueError('x_cand must have shape (n_cand, %d), got %s' % (d, tuple(xc.shape)))
        xc_s, _ = self._standardise_x0(xc)
        xr_s = None
        n_ref = xc.shape[0]
        if x_ref is not None:
            xr = _np(self._verify_data_types(x_ref))
            if xr.ndim != 2 or xr.shape[1] != d or xr.shape[0] < 1:
                raise ValueError('x_ref must have shape (n_ref, %d), got %s' % (d, tuple(xr.shape)))
            xr_s, _ = self._standardise_x0(xr)
            n_ref = xr.shape[0]
        if weights is None:
            w = np.full(n_ref, 1.0 / n_ref)
        else:
            w = np.asarray(weights, F64).reshape(-1)
            if w.shape != (n_ref,):
                raise ValueError('weights must have length n_ref = %d, got %d' % (n_ref, w.size))
            if not np.all(np.isfinite(w)) or np.any(w < 0):
                raise ValueError('weights must be finite and non-negative')
            if not np.any(w > 0):
                raise ValueError('weights must not all be zero')
            w = w / np.sum(w)
        p = int(self.p)
        outputs = list(range(p)) if outputs is None else [int(a) for a in np.atleast_1d(outputs)]
        if any(a < 0 or a >= p for a in outputs):
            raise ValueError('outputs must be indices in [0, %d)' % p)
        if isinstance(replicates, (bool, np.bool_)) or int(replicates) != replicates or replicates < 1:
            raise ValueError('replicates must be an integer >= 1')
        r = int(replicates)
        match = None
        if self.submethod == 'rep':
            xt = self._x_train()
            lookup = {row.tobytes(): i for i, row in enumerate(np.ascontiguousarray(xt))}
            match = np.array([lookup.get(row.tobytes(), -1) for row in np.ascontiguousarray(xc_s)], np.int32)
        elif r != 1:
            raise ValueError("replicates must be 1 on the full path (submethod='full'): a candidate is one new training row")
        return xc_s, xr_s, w, outputs, r, match

    def variance_reduction(self, x_cand, x_ref=None, weights=None, outputs=None, replicates=1, latent=False):
        """Integrated variance reduction (the active-learning-Cohn criterion, ALC / IMSPE reduction): for each candidate input
        the drop of the weighted predictive variance over a reference set if the simulator ran once more there, at FIXED
        parameters (hyper-parameters, noise, basis phi, standardisation; no refit).  It does not depend on the simulator output.
        With latent component k, reference point t, candidate c (standardised) and U_k as in predict():
            R_k(c)     = sum_t w_t Sigma_k(t, c)^2 / (max(Sigma_k^h(c, c), 0) + 1 / (D_k r))
            Sigma_k(t, c)   = C_k(t, c) - D_k U_k(t) . U_k(c)     (no nugget: reference points are new inputs)
            Sigma_k^h(c, c) = scale_k - D_k |U_k(c)|^2           (predict()'s gvar at c, with the candidate's own cross row)
            Delta_a(c) = scale_a^2 sum_k W[k, a]^2 R_k(c)         (W, scale: those of predict())
        R_k(c) is gvar_k summed over the reference set before minus after adding the run to the training set; Delta_a(c) is the
        drop of yconfvar, and of ypredvar (the noise does not change).
          x_cand: (n_cand, d) raw-scale candidates.  x_ref: (n_ref, d) raw-scale reference points (default: x_cand).
          weights: n_ref non-negative weights, normalised to sum 1 (default uniform).  outputs: output indices (default all p).
          replicates: r runs at the candidate.  Full path: the candidate is one new training row with its own nugget, r = 1
                 only; its cross row has no nugget term even where it equals a training input.  Rep path: a candidate equal
                 (after standardisation, bitwise) to a unique training input adds r replicates to it (its cross row carries
                 the nugget term at that input, as predict() does at the training set); otherwise it is a new unique input.
          latent: return R (q, n_cand) instead of Delta (len(outputs), n_cand).
        Computed on the GPU from the factorisation of the current parameters (right after fit() no extra evaluation), in the
        engine's dtype (float32 models: float32 products, double sums).  GPU memory: q_local (n_ref + min(n_cand, 2048)) npad
        elements of scratch and q_local ceil(n_ref / 64) min(n_cand, 2048) doubles (npad = n_train rounded up to 128); the
        n_ref x n_cand matrix is never formed -- ValueError when it does not fit.  self.ghat / self.gvar are left untouched."""
        xc_s, xr_s, w, outputs, r, match = self._vr_arguments(x_cand, x_ref, weights, outputs, replicates)
        eng = self._ensure_aux()
        loc = self._agree(lambda: None if eng is None else eng.variance_reduction_block(xc_s, xr_s, w, match, r))
        R = self._gather_components(loc, (xc_s.shape[0],))
        if latent:
            return _t(R)
        W, _, scale, _ = self._output_map()
        delta = (W[:, outputs] ** 2).T @ R * (scale[outputs] ** 2)[:, None]
        return _t(delta)

    def integrated_variance_reduction(self, x_cand, box=None, outputs=None, replicates=1, latent=False):
        """Exact box ALC: for each candidate input, how much integrated_variance(box) would drop if the simulator ran once more
        there, at FIXED parameters -- variance_reduction() with the weighted sum over a reference set replaced by the exact
        integral over `box` (uniform measure), so the score carries no sampling noise and needs no reference set.  In closed
        form for the product kernels.  With c_k = scale_k (1 - nt_k), X_c the candidate's cross-covariance row
        as variance_reduction() forms it, b_c = D_k c_k sr o (A_k^-1 X_c^T), and M, m_c, m_cc the box averages of products of two
        kernel factors (between training inputs, between the candidate and a training input, of the candidate with itself):
            R_k(c)     = [ c_k^2 m_cc - 2 c_k b_c . m_c + b_c^T M b_c ] / (max(Sigma_k^h(c, c), 0) + 1 / (D_k r))
            Delta_a(c) = scale_a^2 sum_k W[k, a]^2 R_k(c)
        R_k(c) is the latent integrated variance before minus after r runs at c; Delta_a(c) is that of integrated_variance().
        Returns (len(outputs), n_cand), or R (q, n_cand) with latent=True, CPU float64.
          x_cand, outputs, replicates and the rep path's matching of candidates to training inputs: as in variance_reduction().
          box: as in integrated_variance() ((2, d) raw scale, default the training inputs' bounding box).  Candidates may lie
                 outside the box.
        Conditioning: the three terms cancel -- their absolute sum is tens to hundreds of c_k where the gain is 1e-5 to 1e-3 of
        c_k -- so the result carries an ABSOLUTE error of a few ulps of that sum (as integrated_variance() does), fewer
        relative digits than variance_reduction()'s quadrature of squares.  It is not clamped: a gain at rounding level may come
        out slightly negative.  float64 always (a float32 model uses its float64 engine), any number of ranks.  GPU memory: per
        local component processed at once one npad^2 matrix and two min(n_cand, 2048) x npad slabs of doubles (npad = n_train
        rounded up to 128); the components go in groups that fit -- ValueError when one does not."""
        xc_s, _, _, outputs, r, match = self._vr_arguments(x_cand, None, None, outputs, replicates)
        bs = self._marginal_box(box)
        eng = self._ensure_aux64()
        loc = self._agree(lambda: None if eng is None else eng.box_alc_block(xc_s, bs, match, r), what='the exact box ALC')
        R = self._gather_components(loc, (xc_s.shape[0],))
        if latent:
            return _t(R)
        W, _, scale, _ = self._output_map()
        delta = (W[:, outputs] ** 2).T @ R * (scale[outputs] ** 2)[:, None]
        return _t(delta)

    def variance_reduction_grad(self, x_cand, x_ref=None, weights=None, outputs=None, replicates=1, latent=False):
        """variance_reduction() and its gradient with respect to the candidates' locations (the analytic derivative a continuous
        ALC / IMSPE search needs; laGP's alcopt): returns (gain, dgain), CPU float64,
            gain[a, c]     = Delta_a(c)  (latent=True: R_k(c)),   shape (len(outputs) | q, n_cand)
            dgain[a, c, l] = d gain[a, c] / d x_cand[c, l]        on the RAW input scale, shape (len(outputs) | q, n_cand, d)
        Arguments, checks and the full / rep rules for `replicates` exactly as in variance_reduction().  x_ref and weights are
        CONSTANTS: the gradient is with respect to the candidate's location only, also when x_ref=None makes the reference set a
        copy of the candidates.
        Every candidate is a NEW input: on the rep path a candidate bitwise equal to a unique training input gets the value and
        gradient of the continuous surface (a new unique input at that location), NOT variance_reduction()'s
        add-replicates-to-that-input value -- the rule of predict_grad() / predict_differentiable(); the point mass of the nugget
        has no derivative.  Away from such candidates gain is bitwise variance_reduction()'s.  All three kernels have a continuous
        first derivative everywhere, so there is no kink convention.
        Computed on the GPU from the factorisation of the current parameters (lcgp_variance_reduction_grad), in the engine's
        dtype (float32 models: float32 products; Sigma, sums and contractions in double).  GPU memory: variance_reduction()'s plus
        q_local min(n_cand, 2048) (n_ref + 2 npad) elements -- ValueError when it does not fit.  self.ghat / self.gvar are left
        untouched."""
        xc_s, xr_s, w, outputs, r, _ = self._vr_arguments(x_cand, x_ref, weights, outputs, replicates)
        n_cand, d = xc_s.shape
        eng = self._ensure_aux()

        return self._vr_grad_result(None if eng is None else lambda: eng.variance_reduction_grad_block(xc_s, xr_s, w, r),
                                    n_cand, d, outputs, latent)

    def _vr_grad_result(self, block, n_cand, d, outputs, latent):
        """(gain, dgain) of variance_reduction_grad() from block() = (R, dR) of the local components (None: a rank without any):
        one reduction gathers both, the gradient goes to the raw input scale, the output map folds the components"""
        def local():
            if block is None:
                return None
            R, dR = block()
            return torch.cat([R, dR.reshape(dR.shape[0], -1)], dim=1)
        both = self._gather_components(self._agree(local), (n_cand + n_cand * d,))
        rng = (_np(self.x_max) - _np(self.x_min)).reshape(-1)
        R = both[:, :n_cand]
        dR = both[:, n_cand:].reshape(-1, n_cand, d) / rng[None, None, :]
        if latent:
            return _t(R.copy()), _t(dR)
        W, _, scale, _ = self._output_map()
        delta = (W[:, outputs] ** 2).T @ R * (scale[outputs] ** 2)[:, None]
        ddelta = np.einsum('ka,kcl->acl', W[:, outputs] ** 2, dR) * (scale[outputs] ** 2)[:, None, None]
        return _t(delta), _t(ddelta)

    def variance_reduction_differentiable(self, x_cand, x_ref=None, weights=None, outputs=None, replicates=1, latent=False):
        """variance_reduction_grad()'s gain as a tensor on x_cand's device, differentiable with respect to a requires_grad x_cand
        through torch.autograd (the backward pass is the vector-Jacobian product with the gradient the forward pass saved: no
        second GPU pass), so any torch or SciPy optimiser can search a box for the best next run.  x_ref and weights are
        constants (no gradient flows to them, nor through the reference copy of the candidates made by x_ref=None).  First
        derivatives only: a double backward (create_graph=True) raises."""
        x_cand = x_cand if isinstance(x_cand, torch.Tensor) else torch.as_tensor(np.asarray(x_cand, F64))
        kwargs = dict(x_ref=x_ref, weights=weights, outputs=outputs, replicates=replicates, latent=latent)
        return _VrFn.apply(x_cand, self, kwargs)

    def select_batch(self, x_cand, size, x_ref=None, weights=None, outputs=None, replicates=1, return_scores=False):
        """Greedy batch design by sequential ALC: `size` of the candidates, chosen one after the other -- the candidate with the
        largest integrated variance reduction is picked, the posterior variance is conditioned on `replicates` runs there (ALC
        does not depend on the runs' outputs, so no simulator call is needed), and the remaining candidates are scored again.
        Taking the `size` best candidates of ONE variance_reduction() call instead picks neighbours that duplicate information.
            score_t(c) = sum_k omega_k R_k^t(c),   omega_k = mean over a in outputs of scale_a^2 W[k, a]^2
        (the mean over the chosen outputs of variance_reduction()'s Delta), R_k^t: R_k of variance_reduction() for the model
        conditioned on the t picks made so far, at FIXED parameters (hyper-parameters, noise, phi, standardisation; no refit).
          x_cand, x_ref, weights, outputs, replicates: exactly as in variance_reduction() (same checks, same full / rep
                 conventions, same matching of candidates to training inputs on the rep path).
          size: 1 <= size <= n_cand; each candidate is picked at most once.
        Bitwise-duplicate candidate rows (after standardisation) raise ValueError: two copies of one input would have to share
        a nugget, a convention variance_reduction() does not define.
        Returns idx (size,) int64, the picks in order, and gain (size,) float64, gain[t] = score_t(idx[t]); gain is
        non-increasing up to rounding (ALC is submodular at fixed parameters).  With return_scores=True also scores
        (size, n_cand) float64: the whole score row of every step, -inf at candidates already picked.  Ties go to the lowest index.
        The posterior over the candidates is carried as a lazily evaluated pivoted Cholesky factor on the GPU:
        per step two passes over U of the reference set and of the candidates; on one rank all steps are enqueued without a host
        synchronisation.  GPU memory: q_local (n_ref + n_cand) npad elements (ALL candidates resident) plus q_local size
        (n_ref + n_cand) doubles of history -- ValueError when it does not fit.  The model is left unchanged (ghat, gvar, the
        factorisation and n untouched)."""
        xc_s, xr_s, w, r, match, size, omega = self._select_arguments(x_cand, size, x_ref, weights, outputs, replicates)
        eng = self._ensure_aux()
        return self._select_run(
            eng, xc_s.shape[0], size, omega, return_scores,
            block=lambda: eng.select_batch_block(xc_s, xr_s, w, match, r, size, omega[self._local_ks]),
            begin=lambda: eng.select_begin(xc_s, xr_s, w, match, r, size),
            rows=lambda: eng.select_rows(), condition=lambda j: eng.select_condition(j))

    def _select_arguments(self, x_cand, size, x_ref, weights, outputs, replicates):
        """_vr_arguments plus what select_batch() of the model and of a conditioned view check and form beyond it: size, no
        duplicate candidates, the score weights omega (q,)"""
        xc_s, xr_s, w, outputs, r, match = self._vr_arguments(x_cand, x_ref, weights, outputs, replicates)
        n_cand = xc_s.shape[0]
        if isinstance(size, (bool, np.bool_)) or int(size) != size or size < 1 or size > n_cand:
            raise ValueError('size must be an integer in [1, n_cand = %d]' % n_cand)
        size = int(size)
        if len({row.tobytes() for row in np.ascontiguousarray(xc_s)}) != n_cand:
            raise ValueError('x_cand holds duplicate rows (bitwise equal after standardisation): two copies of one input would '
                             'have to share a nugget; pass each candidate once')
        W, _, scale, _ = self._output_map()
        omega = np.mean((W[:, outputs] ** 2) * (scale[outputs] ** 2)[None, :], axis=1)
        return xc_s, xr_s, w, r, match, size, omega

    def _select_run(self, eng, n_cand, size, omega, return_scores, block, begin, rows, condition):
        """the greedy loop of select_batch(), of the model and of a conditioned view: `block` runs it whole on the device,
        `begin` / `rows` / `condition` are its steps on this rank's engine (eng = None: a rank without components)"""
        q = int(self.q)
        if not _dist.use_collectives(self._group):
            # one rank holds every component: the whole loop on the device, one copy back
            idx_d, sc_d = self._agree(block)
            idx = idx_d.cpu().numpy().astype(np.int64)
            scores = sc_d.cpu().numpy()
        else:
            # components sharded over ranks: per step the local rows are gathered (disjoint components: the sum is a gather, so
            # every rank adds the q terms in the order one rank does), rank 0's argmax is broadcast
            self._agree(lambda: None if eng is None else begin())
            dev = None if eng is None else eng.device
            idx = np.zeros(size, np.int64)
            scores = np.empty((size, n_cand), F64)
            picked = np.zeros(n_cand, bool)
            for t in range(size):
                R = self._gather_components(None if eng is None else rows(), (n_cand,))
                s = np.zeros(n_cand, F64)
                for k in range(q):
                    s = s + omega[k] * R[k]
                s[picked] = -np.inf
                j = int(_dist.broadcast_array(np.array([np.argmax(s)], F64), 0, self._group, dev)[0])
                idx[t], scores[t], picked[j] = j, s, True
                if eng is not None and t + 1 < size:
                    condition(j)
        gain = scores[np.arange(size), idx].copy()
        if return_scores:
            return torch.as_tensor(idx), _t(gain), _t(scores)
        return torch.as_tensor(idx), _t(gain)

    # =============================================================================================
    # input gradients of the prediction (the reference: a tf.GradientTape around predict)
    # =============================================================================================
    def _latent_predict_grad(self, x0):
        """ghat, gvar (q, n0) and their Jacobians dghat, dgvar (q, n0, d) with respect to the STANDARDISED inputs, for raw-scale
        x0: the local components on the device (lcgp_predict_grad), ONE reduction of the zero-padded block gathers them.
        No nugget term (same = 0 even at training inputs): the gradient of the continuous prediction surface."""
        x0s, _ = self._standardise_x0(x0)
        eng = self._ensure_aux()
        res = self._latent_grad_result(x0s, None if eng is None else lambda: eng.predict_grad_block(x0s))
        ghat, gvar, dghat, dgvar = res
        self.ghat, self.gvar = _t(ghat), _t(gvar)
        self.dghat, self.dgvar = _t(dghat), _t(dgvar)
        return res

    def _latent_grad_result(self, x0s, block):
        """_latent_predict_grad's gather for this rank's (blk, jac) = block() (None on a rank without components): shared with
        ConditionedLCGP"""
        n0, d = x0s.shape
        loc = None
        if block is not None:
            blk, jac = block()
            loc = torch.cat([t.movedim(1, 0).reshape(t.shape[1], -1) for t in (blk, jac)], dim=1)
        both = self._gather_components(loc, (2 * n0 + 2 * n0 * d,))
        jac = both[:, 2 * n0:].reshape(int(self.q), 2, n0, d)
        return both[:, :n0], both[:, n0:2 * n0], jac[:, 0], jac[:, 1]

    def _output_jacobians(self, dghat, dgvar):
        """latent Jacobians (q, n0, d) on the standardised scale -> (dypred, dyconfvar) (p, n0, d) on the raw input and output
        scales, through _output_map():  dypred = scale_a sum_k W[k, a] dghat_k / range,  dyconfvar = scale_a^2 sum_k W[k, a]^2
        dgvar_k / range  (range = x_max - x_min, x0s = (x0 - x_min) / range)"""
        W, _, scale, _ = self._output_map()
        rng = (_np(self.x_max) - _np(self.x_min)).reshape(-1)
        dyp = np.einsum('ka,kil->ail', W, dghat) * scale[:, None, None] / rng[None, None, :]
        dycv = np.einsum('ka,kil->ail', W ** 2, dgvar) * (scale ** 2)[:, None, None] / rng[None, None, :]
        return dyp, dycv

    def predict_grad(self, x0):
        """Jacobians of predict()'s outputs with respect to the new inputs, per point (output row i depends only on x0[i]):
            dypred[a, i, l] = d ypred[a, i] / d x0[i, l],   dypredvar, dyconfvar likewise      each (p, n0, d), CPU float64
        on the raw input and output scales.  dypredvar = dyconfvar (the noise variance does not depend on x0).  Computed on
        the GPU from the factorisation of the current parameters (lcgp_predict_grad; right after fit() no extra evaluation),
        in the engine's dtype.  Nugget convention: the reference adds the nugget to the cross covariance only when x0 IS the
        training set; that point mass has no derivative, so this is the gradient of the continuous prediction surface, also
        at training inputs.  The latent Jacobians stay on the model as dghat / dgvar (q, n0, d), next to ghat / gvar."""
        _, _, dghat, dgvar = self._latent_predict_grad(x0)
        dyp, dycv = self._output_jacobians(dghat, dgvar)
        return _t(dyp), _t(dycv.copy()), _t(dycv)

    def predict_differentiable(self, x0, order=1):
        """(ypred, ypredvar, yconfvar) (p, n0) as predict() returns them, float64 on x0's device, differentiable with respect to
        a requires_grad x0 (any device) through torch.autograd: the backward pass is the vector-Jacobian product with the
        Jacobians of predict_grad() saved by the forward pass (no second GPU pass).  The values equal predict(x0) whenever x0 is
        not the training set (here the nugget term is never added: see predict_grad).
        order=1: first derivatives only; a double backward (create_graph=True) raises.  order=2: the backward pass is itself
        differentiable, so torch.autograd.grad(..., create_graph=True), torch.autograd.functional.hessian and gradgradcheck
        work; the Hessians come from one predict_hess() pass, made only when a double backward actually runs.  A third
        derivative raises."""
        if order not in (1, 2):
            raise ValueError('predict_differentiable: order must be 1 or 2, got %r' % (order,))
        x0 = x0 if isinstance(x0, torch.Tensor) else torch.as_tensor(np.asarray(x0, F64))
        return (_PredictFn if order == 1 else _PredictFn2).apply(x0, self)

    # =============================================================================================
    # calibration: the log likelihood of a field observation as a function of the inputs (beyond the reference)
    # =============================================================================================
    def calibration(self, y_obs, obs_var, include_noise=True):
        """A CalibrationTarget for one field observation: y_obs (p,) on the raw output scale, NaN marking an output that was not
        observed (at least one must be; fewer than q is fine), and obs_var, the observation (plus discrepancy) covariance on
        the raw output scale as a scalar, (p,) variances or a symmetric (p, p) matrix; rows and columns of unobserved outputs
        are ignored.  include_noise=True adds the fitted noise variance, as ypredvar does.  The target's loglik(theta) is
            log N(y_obs; ypred(theta), Phi_s diag(gvar(theta)) Phi_s^T + noise + Sigma_obs)
        restricted to the observed outputs, exactly (no diagonal approximation of the emulator's covariance), on the full and
        rep paths; loglik_grad(theta) adds its gradient in theta, loglik_hess(theta) its Hessian.  Everything p-sized is folded here, once, into a q x q
        matrix and a q-vector (host float64; a diagonal obs_var never forms a p x p matrix); per row of theta the GPU then
        factorises a q x q matrix on top of lcgp_predict_grad's outputs (lcgp_calib_rows).
        Raises ValueError for wrong shapes, non-finite observed values, negative variances and an asymmetric (p, p) obs_var,
        numpy.linalg.LinAlgError when noise + Sigma_obs over the observed outputs is not positive definite."""
        p = int(self.p)
        y = _np(y_obs)
        if y.shape != (p,):
            raise ValueError('y_obs must have shape (%d,), got %s' % (p, tuple(y.shape)))
        obs = ~np.isnan(y)
        if not obs.any():
            raise ValueError('y_obs holds no observed output (all NaN)')
        if not np.all(np.isfinite(y[obs])):
            raise ValueError('the observed entries of y_obs must be finite')
        ov = _np(obs_var)
        if ov.ndim == 0:
            ov = np.full(p, float(ov), F64)
        if ov.shape not in ((p,), (p, p)):
            raise ValueError('obs_var must be a scalar, (%d,) variances or a (%d, %d) covariance, got shape %s'
                             % (p, p, p, tuple(ov.shape)))
        W, noise, scale, offset = self._output_map()
        phi_s = (W[:, obs] * scale[obs][None, :]).T                          # (|O|, q)
        t = (y - offset)[obs]
        lam = (scale ** 2 * noise)[obs] if include_noise else np.zeros(int(obs.sum()), F64)
        if ov.ndim == 1:
            var = ov[obs]
            if not np.all(np.isfinite(var)) or np.any(var < 0):
                raise ValueError('obs_var must be finite and non-negative on the observed outputs')
            lam = lam + var
            if not np.all(lam > 0):
                raise np.linalg.LinAlgError('noise + obs_var is not positive on every observed output')
            M = phi_s.T @ (phi_s / lam[:, None])
            b = phi_s.T @ (t / lam)
            c0 = float(t @ (t / lam))
            logdet = float(np.sum(np.log(lam)))
        else:
            S = ov[np.ix_(obs, obs)]
            if not np.all(np.isfinite(S)) or np.any(np.diag(S) < 0):
                raise ValueError('obs_var must be finite with a non-negative diagonal on the observed outputs')
            if np.max(np.abs(S - S.T)) > 1e-12 * max(np.max(np.abs(S)), np.finfo(F64).tiny):
                raise ValueError('a (p, p) obs_var must be symmetric')
            low = np.linalg.cholesky(0.5 * (S + S.T) + np.diag(lam))         # LinAlgError when not positive definite
            import scipy.linalg as sla
            A = sla.solve_triangular(low, phi_s, lower=True)
            z = sla.solve_triangular(low, t, lower=True)
            M, b, c0 = A.T @ A, A.T @ z, float(z @ z)
            logdet = 2.0 * float(np.sum(np.log(np.diag(low))))
        lognorm = logdet + int(obs.sum()) * float(np.log(2.0 * np.pi))
        return CalibrationTarget(self, obs, 0.5 * (M + M.T), b, c0, lognorm)

    def _calib_latent(self, x0s, grad, view=None):
        """(blk (2, q, n0), jac (2, q, n0, d) or None): [ghat; gvar] and [dghat; dgvar] of ALL q components at the standardised
        inputs x0s, float64 tensors where the row kernel runs; view: a ConditionedLCGP of this model whose latents are taken
        instead of the fitted model's.  grad=2 (second order): (blk, jac, hess), hess (2, q, n0, d (d + 1) / 2) = [d2ghat;
        d2gvar] as packed lower triangles, from predict_hess_block / condition_predict_hess_block, whose blk and jac are
        bitwise the first-order ones.  One rank: the engine's blocks, read in place.  Several ranks: the zero-padded blocks
        are summed over the ranks (disjoint components: exact) and copied back to every rank's device."""
        if view is None:
            eng = self._ensure_aux()
            hess_block = lambda x: eng.predict_hess_block(x)
            grad_block = lambda x: eng.predict_grad_block(x)
            block = lambda x: eng.predict_block(x, False)
        else:
            eng, st = view._engine, view._state
            hess_block = lambda x: eng.condition_predict_hess_block(st, x)
            grad_block = lambda x: eng.condition_predict_grad_block(st, x)
            block = lambda x: eng.condition_predict_block(st, x)
        if not _dist.use_collectives(self._group):
            if grad == 2:
                return hess_block(x0s)
            return grad_block(x0s) if grad else (block(x0s), None)
        n0, d = x0s.shape
        q = int(self.q)
        tri = d * (d + 1) // 2
        widths = [2 * n0] + ([2 * n0 * d] if grad else []) + ([2 * n0 * tri] if grad == 2 else [])
        loc = None
        if eng is not None and grad:
            parts = hess_block(x0s) if grad == 2 else grad_block(x0s)
            loc = torch.cat([t.movedim(1, 0).reshape(t.shape[1], -1) for t in parts], dim=1)
        elif eng is not None:
            loc = block(x0s).permute(1, 0, 2).reshape(-1, 2 * n0)
        both = self._gather_components(loc, (sum(widths),))
        if eng is not None:
            dev = eng.device
        else:
            dev = torch.device(self._device) if self._device is not None else torch.device('cuda', torch.cuda.current_device())
        both = torch.as_tensor(np.ascontiguousarray(both, F64)).to(dev)
        blk = both[:, :2 * n0].reshape(q, 2, n0).permute(1, 0, 2).contiguous()
        jac = both[:, 2 * n0:2 * n0 * (1 + d)].reshape(q, 2, n0, d).permute(1, 0, 2, 3).contiguous() if grad else None
        if grad == 2:
            return blk, jac, both[:, 2 * n0 * (1 + d):].reshape(q, 2, n0, tri).permute(1, 0, 2, 3).contiguous()
        return blk, jac

    def _calib_rows_device(self, blk, jac, M, b, inv_range, c0, lognorm, want_sens):
        """the one call into the row kernel (lcgp_calib_rows; there is no other implementation in the package): device
        tensors in, numpy (ll (n0,), dll (n0, d) or None, sens (2, q, n0) or None) out"""
        from .engine import calib_rows_device
        out = calib_rows_device(blk, jac, M, b, c0, lognorm, inv_range, want_sens)
        return tuple(None if t is None else t.cpu().numpy() for t in out)

    def _calib_hess_rows_device(self, blk, jac, hess, M, b, inv_range, c0, lognorm, want_sens, want_B):
        """the one call into the second-order row entry (lcgp_calib_hess_rows; there is no other implementation in the
        package): device tensors in, numpy (ll (n0,), dll (n0, d), d2ll (n0, d (d + 1) / 2) packed, sens (2, q, n0) or None,
        B (n0, q, q) or None) out"""
        from .engine import calib_hess_rows_device
        out = calib_hess_rows_device(blk, jac, hess, M, b, c0, lognorm, inv_range, want_sens, want_B)
        return tuple(None if t is None else t.cpu().numpy() for t in out)

    # =============================================================================================
    # input Hessians of the prediction (the reference: two nested tf.GradientTapes around predict)
    # =============================================================================================
    def _latent_predict_hess(self, x0):
        """ghat, gvar (q, n0), dghat, dgvar (q, n0, d) and the Hessians d2ghat, d2gvar (q, n0, d, d) with respect to the
        STANDARDISED inputs, for raw-scale x0: the local components on the device (lcgp_predict_hess), ONE reduction of the
        zero-padded block gathers them; the packed lower triangles are mirrored here, so the Hessians are exactly symmetric.
        No nugget term, as in _latent_predict_grad."""
        x0s, _ = self._standardise_x0(x0)
        eng = self._ensure_aux()
        res = self._latent_hess_result(x0s, None if eng is None else lambda: eng.predict_hess_block(x0s))
        ghat, gvar, dghat, dgvar, d2ghat, d2gvar = res
        self.ghat, self.gvar = _t(ghat), _t(gvar)
        self.dghat, self.dgvar = _t(dghat), _t(dgvar)
        self.d2ghat, self.d2gvar = _t(d2ghat), _t(d2gvar)
        return res

    def _latent_hess_result(self, x0s, block):
        """_latent_predict_hess's gather and mirroring for this rank's (blk, jac, hess) = block() (None on a rank without
        components): shared with ConditionedLCGP"""
        n0, d = x0s.shape
        tri = d * (d + 1) // 2
        loc = None
        if block is not None:
            blk, jac, hess = block()
            loc = torch.cat([t.movedim(1, 0).reshape(t.shape[1], -1) for t in (blk, jac, hess)], dim=1)
        both = self._gather_components(loc, (2 * n0 * (1 + d + tri),))
        q = int(self.q)
        ghat, gvar = both[:, :n0], both[:, n0:2 * n0]
        jac = both[:, 2 * n0:2 * n0 * (1 + d)].reshape(q, 2, n0, d)
        packed = both[:, 2 * n0 * (1 + d):].reshape(q, 2, n0, tri)
        il, im = np.tril_indices(d)                       # row-major over the lower triangle: entry (l, m) at l (l + 1) / 2 + m
        full = np.empty((q, 2, n0, d, d), F64)
        full[..., il, im] = packed
        full[..., im, il] = packed
        return ghat, gvar, jac[:, 0], jac[:, 1], full[:, 0], full[:, 1]

    def _output_hessians(self, d2ghat, d2gvar):
        """latent Hessians (q, n0, d, d) on the standardised scale -> (d2ypred, d2yconfvar) (p, n0, d, d) on the raw input and
        output scales, as _output_jacobians:  d2ypred = scale_a sum_k W[k, a] d2ghat_k / (range_l range_m),  d2yconfvar with
        W^2, scale_a^2"""
        W, _, scale, _ = self._output_map()
        rng = (_np(self.x_max) - _np(self.x_min)).reshape(-1)
        rr = rng[:, None] * rng[None, :]
        d2yp = np.einsum('ka,kilm->ailm', W, d2ghat) * scale[:, None, None, None] / rr
        d2ycv = np.einsum('ka,kilm->ailm', W ** 2, d2gvar) * (scale ** 2)[:, None, None, None] / rr
        return d2yp, d2ycv

    def predict_hess(self, x0):
        """Hessians of predict()'s outputs with respect to the new inputs, per point (output row i depends only on x0[i]):
            d2ypred[a, i, l, m] = d^2 ypred[a, i] / d x0[i, l] d x0[i, m],   d2ypredvar, d2yconfvar likewise
        each (p, n0, d, d), CPU float64, exactly symmetric in the last two axes, on the raw input and output scales;
        d2ypredvar = d2yconfvar.  One pass on the GPU from the factorisation of the current parameters (lcgp_predict_hess),
        in the engine's dtype; every kernel has them (Matern-3/2: continuous, with a kink where x0[i, l] equals a training
        input's coordinate).  Nugget convention of predict_grad: the Hessian of the continuous prediction surface, also at
        training inputs.  The latent Hessians stay on the model as d2ghat / d2gvar (q, n0, d, d), beside dghat / dgvar (which,
        like ghat / gvar, this call sets to what predict_grad(x0) sets)."""
        _, _, _, _, d2ghat, d2gvar = self._latent_predict_hess(x0)
        d2yp, d2ycv = self._output_hessians(d2ghat, d2gvar)
        return _t(d2yp), _t(d2ycv.copy()), _t(d2ycv)

    # =============================================================================================
    # posterior covariance of the gradient and active subspaces (no counterpart in the reference)
    # =============================================================================================
    @staticmethod
    def _unpack_lower(packed, d):
        """(..., d (d + 1) / 2) packed lower triangles -> (..., d, d), mirrored: exactly symmetric"""
        il, im = np.tril_indices(d)
        full = np.empty(packed.shape[:-1] + (d, d), F64)
        full[..., il, im] = packed
        full[..., im, il] = packed
        return full

    def _x0_2d(self, x0, name):
        x0n = _np(self._verify_data_types(x0))
        if x0n.ndim != 2 or x0n.shape[1] != int(self.d) or x0n.shape[0] < 1:
            raise ValueError('%s must have shape (n, %d), got %s' % (name, int(self.d), tuple(x0n.shape)))
        return self._standardise_x0(x0n)[0]

    def predict_grad_cov(self, x0, latent=False):
        """Posterior covariance of the gradient of the noise-free output at each new input, the counterpart of yconfvar for
        predict_grad()'s dypred:
            cov[a, i, l, m] = Cov(d y_a / d x0[i, l], d y_a / d x0[i, m])
                            = scale_a^2 sum_k W[k, a]^2 Gamma_k[i, l, m] / (range_l range_m)          (p, n0, d, d)
            Gamma_k[i, l, m] = delta_lm c_k kappa / ell_l^2 - D_k (P_il . P_im) / (ell_l ell_m)
        on the raw input and output scales (W, scale: those of predict(); range = x_max - x_min), CPU float64, exactly
        symmetric.  Gamma_k is the posterior covariance function of latent component k differentiated once in each argument:
        c_k = scale_k (1 - nug_k / (1 + nug_k)) is the continuous part of the prior variance (the nugget is a point mass with
        no derivative: the convention of predict_grad), kappa = 1 (Matern-3/2, SE) or 1 / 3 (Matern-5/2), P_il the rows of
        predict_hess().  latent=True returns Gamma (q, n0, d, d) in standardised inputs.  One pass on the GPU from the
        factorisation of the current parameters (lcgp_predict_gradcov), in the engine's dtype.  Sets self.dghat to what
        predict_grad(x0) sets."""
        x0s = self._x0_2d(x0, 'x0')
        eng = self._ensure_aux()
        dghat, cov = self._grad_cov_result(x0s, None if eng is None else lambda: eng.grad_cov_block(x0s), latent)
        self.dghat = _t(dghat)
        return cov

    def _grad_cov_result(self, x0s, block, latent):
        """predict_grad_cov's gather and output map for this rank's (dghat, gamma, _) = block() (None on a rank without
        components) -> (dghat (q, n0, d), the result): shared with ConditionedLCGP"""
        n0, d = x0s.shape
        tri = d * (d + 1) // 2
        loc = None
        if block is not None:
            dghat, gamma, _ = block()
            loc = torch.cat([dghat.reshape(dghat.shape[0], -1), gamma.reshape(gamma.shape[0], -1)], dim=1)
        both = self._gather_components(loc, (n0 * (d + tri),))
        q = int(self.q)
        dghat = both[:, :n0 * d].reshape(q, n0, d)
        G = self._unpack_lower(both[:, n0 * d:].reshape(q, n0, tri), d)
        if latent:
            return dghat, _t(G)
        W, _, scale, _ = self._output_map()
        rng = (_np(self.x_max) - _np(self.x_min)).reshape(-1)
        cov = np.einsum('ka,kilm->ailm', W ** 2, G) * (scale ** 2)[:, None, None, None] / (rng[:, None] * rng[None, :])
        return dghat, _t(cov)

    def active_subspace(self, x_ref, weights=None, outputs=None):
        """Active-subspace matrix of each selected output over a reference sample, with the emulator's uncertainty included:
            C_a = sum_i w_i E[grad y_a grad y_a^T at x_ref[i]] = sum_i w_i grad ypred_a grad ypred_a^T + sum_i w_i predict_grad_cov
        (the posterior expectation of an outer product is the outer product of the means plus the covariance).  Returns an
        ActiveSubspace: matrix = mean_part + cov_part (p_sel, d, d), activity = its diagonal (the expected derivative-based
        global sensitivity measures nu_l, which bound the total Sobol indices from above), eigenvalues (descending) and
        eigenvectors (columns).  A cov_part that is not small beside mean_part says more runs may change the ranking.
          x_ref: (n_ref, d) raw-scale sample of the input distribution.  weights: n_ref non-negative weights, normalised to
          sum 1 (default uniform), as in variance_reduction().  outputs: output indices (default all p).
        The weighted sum of the covariances is reduced on the GPU (the n_ref x d x d tensor is never formed); the mean part is
        formed on the host from the gathered latent gradients, n_ref x d per component."""
        return self._active_subspace(x_ref, weights, outputs, self._ensure_aux,
                                     lambda eng, x0s, w: eng.grad_cov_block(x0s, w, per_point=False))

    def _active_subspace(self, x_ref, weights, outputs, engine, block):
        """active_subspace's checks, gather and assembly; engine() is called behind the checks and gives this rank's engine
        (None on a rank without components), block(engine, x0s, w) its (dghat, _, M): shared with ConditionedLCGP"""
        x0s = self._x0_2d(x_ref, 'x_ref')
        n0, d = x0s.shape
        if weights is None:
            w = np.full(n0, 1.0 / n0)
        else:
            w = np.asarray(weights, F64).reshape(-1)
            if w.shape != (n0,):
                raise ValueError('weights must have length n_ref = %d, got %d' % (n0, w.size))
            if not np.all(np.isfinite(w)) or np.any(w < 0):
                raise ValueError('weights must be finite and non-negative')
            if not np.any(w > 0):
                raise ValueError('weights must not all be zero')
            w = w / np.sum(w)
        p = int(self.p)
        outputs = list(range(p)) if outputs is None else [int(a) for a in np.atleast_1d(outputs)]
        if any(a < 0 or a >= p for a in outputs):
            raise ValueError('outputs must be indices in [0, %d)' % p)
        tri = d * (d + 1) // 2
        eng = engine()
        loc = None
        if eng is not None:
            dghat, _, M = block(eng, x0s, w)
            loc = torch.cat([dghat.reshape(dghat.shape[0], -1), M], dim=1)
        both = self._gather_components(loc, (n0 * d + tri,))
        q = int(self.q)
        dghat = both[:, :n0 * d].reshape(q, n0, d)
        Mk = self._unpack_lower(both[:, n0 * d:], d)
        W, _, scale, _ = self._output_map()
        W, scale = W[:, outputs], scale[outputs]
        rng = (_np(self.x_max) - _np(self.x_min)).reshape(-1)
        grad = np.einsum('ka,kil->ail', W, dghat) * scale[:, None, None] / rng[None, None, :]
        mean_part = np.einsum('i,ail,aim->alm', w, grad, grad)
        mean_part = 0.5 * (mean_part + np.swapaxes(mean_part, -1, -2))
        cov_part = np.einsum('ka,klm->alm', W ** 2, Mk) * (scale ** 2)[:, None, None] / (rng[:, None] * rng[None, :])
        matrix = mean_part + cov_part
        lam, vec = np.linalg.eigh(matrix)
        lam, vec = lam[:, ::-1].copy(), vec[:, :, ::-1].copy()
        big = np.argmax(np.abs(vec), axis=1)                            # (p_sel, d): row of the largest entry per column
        sign = np.sign(np.take_along_axis(vec, big[:, None, :], axis=1))
        vec = vec * np.where(sign == 0, 1.0, sign)
        activity = np.diagonal(matrix, axis1=-2, axis2=-1).copy()
        return ActiveSubspace(_t(matrix), _t(mean_part), _t(cov_part), _t(activity), _t(lam), _t(vec))

    # =============================================================================================
    # box-averaged predictions (beyond the reference): closed-form averages of the product kernels
    # =============================================================================================
    def _marginal_box(self, box):
        """box (2, d) on the raw scale (default: the training inputs' bounding box) -> standardised [lo; hi]"""
        d = int(self.d)
        if box is None:
            return np.stack([np.zeros(d, F64), np.ones(d, F64)])
        b = np.asarray(_np(self._verify_data_types(box)), F64)
        if b.shape != (2, d):
            raise ValueError('box must have shape (2, %d) = [lower; upper], got %s' % (d, tuple(b.shape)))
        xmin, xmax = _np(self.x_min).reshape(-1), _np(self.x_max).reshape(-1)
        bs = (b - xmin[None, :]) / (xmax - xmin)[None, :]
        if not np.all(np.isfinite(bs)) or not np.all(bs[1] > bs[0]):
            raise ValueError('box must be finite with upper > lower in every dimension')
        return bs

    def _marginal_rows(self, x0, integrate, name='x0'):
        """x0 (n0, d) raw scale and `integrate` (dimension indices for every row, or a boolean (n0, d) array) -> (x0n, mask): a
        float64 copy and the boolean mask of integrated entries, after predict_marginal()'s shape and index checks"""
        x0n = np.array(_np(self._verify_data_types(x0)), F64)
        d = int(self.d)
        if x0n.ndim != 2 or x0n.shape[1] != d or x0n.shape[0] < 1:
            raise ValueError('%s must have shape (n, %d), got %s' % (name, d, tuple(x0n.shape)))
        n0 = x0n.shape[0]
        integ = np.asarray(integrate)
        if integ.dtype == bool and integ.ndim == 2:
            if integ.shape != (n0, d):
                raise ValueError('a boolean integrate must have shape (%d, %d), got %s' % (n0, d, tuple(integ.shape)))
            mask = integ.copy()
        else:
            idx = integ.reshape(-1)
            if idx.size and not np.issubdtype(idx.dtype, np.integer):
                raise ValueError('integrate must be dimension indices or a boolean (n0, d) array')
            if np.any(idx < 0) or np.any(idx >= d):
                raise ValueError('integrate must hold dimension indices in [0, %d)' % d)
            mask = np.zeros((n0, d), bool)
            mask[:, idx.astype(int)] = True
        return x0n, mask

    def _marginal_arguments(self, x0, integrate, box, cov_with):
        """predict_marginal()'s checks, for the model and its views: (x0s (n0, d) standardised with zeros under the mask, mask,
        box (2, d) standardised, ref) with ref = None or (x_ref_s (d,), mask_ref (d,)) from cov_with"""
        x0n, mask = self._marginal_rows(x0, integrate)
        row = None
        if cov_with is not None:
            if not isinstance(cov_with, (tuple, list)) or len(cov_with) != 2:
                raise ValueError('cov_with must be (x_row, integrate_row): one raw-scale row (d,) and its integrated dimensions')
            xr = np.array(_np(cov_with[0]), F64)                  # (a vector: _verify_data_types would make it a column)
            d = int(self.d)
            if xr.shape != (d,):
                raise ValueError('the row of cov_with must have shape (%d,), got %s' % (d, tuple(xr.shape)))
            ir = np.asarray(cov_with[1])
            if ir.dtype == bool and ir.ndim == 1:
                if ir.shape != (d,):
                    raise ValueError('a boolean integrate_row of cov_with must have shape (%d,), got %s' % (d, tuple(ir.shape)))
                ir = ir[None, :]
            row = self._marginal_rows(xr[None, :], ir, 'the row of cov_with')
        bs = self._marginal_box(box)
        if not np.all(np.isfinite(x0n[~mask])):
            raise ValueError('x0 must be finite in the columns that are kept')
        x0n[mask] = 0.0                                  # (never read: the engine passes zeros under the mask)
        x0s = self._standardise_x0(x0n)[0]
        ref = None
        if row is not None:
            xr, mr = row
            if not np.all(np.isfinite(xr[~mr])):
                raise ValueError('the row of cov_with must be finite in the columns that are kept')
            xr[mr] = 0.0
            ref = (self._standardise_x0(xr)[0][0], mr[0])
        return x0s, mask, bs, ref

    def _marginal_result(self, loc, n0, latent, with_cov):
        """this rank's (q_local, 2 or 3, n0) block [ghat; gvar[; gcov]] (None without components) -> what predict_marginal()
        returns; a covariance maps to the outputs as a variance does (W^2, scale^2, no additive term)"""
        both = self._gather_components(loc, (3 if with_cov else 2, n0))
        ghat, gvar = both[:, 0], both[:, 1]
        if latent:
            return (_t(ghat), _t(gvar)) + ((_t(both[:, 2]),) if with_cov else ())
        ypred, _, yconfvar = self._outputs(ghat, gvar)
        if not with_cov:
            return ypred, yconfvar
        W, _, scale, _ = self._output_map()
        return ypred, yconfvar, _t((both[:, 2].T @ W ** 2).T * (scale ** 2)[:, None])

    def predict_marginal(self, x0, integrate, box=None, latent=False, cov_with=None):
        """Predictions AVERAGED over some of the inputs: (ypred, yconfvar), each (p, n0), the output at the kept inputs of each
        row of x0 averaged over the integrated inputs, uniformly over `box`, and the posterior variance of that average (of
        the noise-free surface; no ypredvar: observation noise does not average).
          integrate: a sequence of dimension indices, the same for every row, or a boolean (n0, d) array, one mask per row
                     (True = integrated out).  Values of x0 in integrated columns are ignored; NaN is allowed there.
          box:       (2, d) = [lower; upper] on the raw input scale (default: the training inputs' bounding box).  Training
                     inputs may lie outside it.
          latent:    return (ghat, gvar), each (q, n0), of the latent components instead.
          cov_with:  (x_row, integrate_row): one more raw-scale row (d,) with its dimension indices or boolean (d,) mask, checked
                     as x0 and integrate are (NaN allowed under the mask).  A third result ycov (p, n0) is appended (latent:
                     gcov (q, n0)): the posterior covariance of each row's average with that row's average, for the same
                     output, of the continuous surface (no nugget term, also for two rows that integrate nothing).  The first
                     two results are bitwise those without it.
        For the product kernels the average is exact: a prediction whose cross-covariance row holds the box average of the
        1-D kernel factor in the integrated dimensions and whose prior variance holds its double average (the nugget, white
        noise, averages to zero).  One pass on the GPU at the cost of predict() on n0 rows (lcgp_predict_marginal); a row that
        integrates nothing is predict()'s at a new input.  Rows are treated one by one: beyond cov_with's row their covariance
        is not formed."""
        x0s, mask, bs, ref = self._marginal_arguments(x0, integrate, box, cov_with)
        eng = self._ensure_aux()
        extra = {} if ref is None else {'ref': ref}
        loc = None if eng is None else eng.predict_marginal_block(x0s, mask, bs, **extra).permute(1, 0, 2)      # (q_local, 2 | 3, n0)
        return self._marginal_result(loc, x0s.shape[0], latent, ref is not None)

    def main_effects(self, grid=33, box=None, outputs=None, effect_var=False):
        """Main effects of every input: the output as a function of input l alone, averaged over all the others uniformly over
        `box` ((2, d) raw scale, default the training inputs' bounding box), on `grid` equally spaced values of input l
        between the box's ends, with the posterior variance of each average; and the average over all inputs.  One
        predict_marginal() pass of d grid + 1 rows.  Returns a MainEffects (grid, mean, var, overall, overall_var, effect,
        effect_var); outputs: output indices (default all p).  effect_var=True: the same pass takes the overall row as
        cov_with's and fills MainEffects.effect_var, the variance of the plotted curve `effect` (otherwise None; the other
        fields are bitwise the same either way)."""
        return self._main_effects(self.predict_marginal, grid, box, outputs, effect_var)

    def _main_effects(self, marginal, grid, box, outputs, effect_var):
        """main_effects() through `marginal`, the model's predict_marginal or a view's"""
        d, G = int(self.d), int(grid)
        if G < 1:
            raise ValueError('grid must be at least 1')
        p = int(self.p)
        outputs = list(range(p)) if outputs is None else [int(a) for a in np.atleast_1d(outputs)]
        if any(a < 0 or a >= p for a in outputs):
            raise ValueError('outputs must be indices in [0, %d)' % p)
        self._marginal_box(box)                                 # (its checks, before any work)
        xmin, xmax = _np(self.x_min).reshape(-1), _np(self.x_max).reshape(-1)
        raw = np.stack([xmin, xmax]) if box is None else np.asarray(_np(self._verify_data_types(box)), F64)
        t = np.linspace(0.0, 1.0, G) if G > 1 else np.array([0.5])
        grid_raw = raw[0][:, None] + (raw[1] - raw[0])[:, None] * t[None, :]                   # (d, G)
        x0 = np.full((d * G + 1, d), np.nan)
        mask = np.ones((d * G + 1, d), bool)
        for l in range(d):
            x0[l * G:(l + 1) * G, l] = grid_raw[l]
            mask[l * G:(l + 1) * G, l] = False
        ns = len(outputs)
        if effect_var:
            ypred, yconfvar, ycov = marginal(x0, mask, box=box, cov_with=(x0[-1], mask[-1]))
            ycov = _np(ycov)[outputs]
        else:
            ypred, yconfvar = marginal(x0, mask, box=box)
        ypred, yconfvar = _np(ypred)[outputs], _np(yconfvar)[outputs]
        ev = None
        if effect_var:
            ev = _t((yconfvar[:, :-1] + yconfvar[:, -1:] - 2.0 * ycov[:, :-1]).reshape(ns, d, G))
        return MainEffects(_t(grid_raw), _t(ypred[:, :-1].reshape(ns, d, G)), _t(yconfvar[:, :-1].reshape(ns, d, G)),
                           _t(ypred[:, -1]), _t(yconfvar[:, -1]), ev)

    # =============================================================================================
    # Sobol indices of the posterior mean surface in closed form (beyond the reference)
    # =============================================================================================
    def sobol_indices(self, box=None, outputs=None, latent=False, uncertainty=False, order=1):
        """First-order and total Sobol indices of every output with respect to every input: the share of the output's variance
        over `box` ((2, d) raw scale, default the training inputs' bounding box; uniform measure) that input l explains alone
        (first) and together with all its interactions (total).  They are those of the posterior mean surface at the fitted
        parameters (the plug-in estimator; the emulator's own uncertainty does not enter), exact for the product kernels: no
        sampling, so an index that is zero comes out as rounding error, not as Monte Carlo noise.  Returns a SobolIndices
        (first, total, variance, mean, first_variance, closed_variance); outputs: output indices (default all p); latent=True:
        the same for the q latent components (outputs then selects components).
        One pass on the GPU over the n x n pairs of training inputs per pair of components k <= k' (lcgp_sobol_pairs; latent=True:
        the q pairs k = k' only), always in float64 -- a float32 model evaluates once on its float64 engine for the weight
        vectors.  With several ranks the pairs are dealt round-robin over the ranks that hold components and one reduction
        assembles them: the result does not depend on the number of ranks.
        uncertainty=True: the SobolIndices also carries the posterior expectations of the variances (Oakley and O'Hagan 2004)
        and the integrated variance (expected_variance, expected_first_variance, expected_closed_variance, first_expected,
        total_expected, integrated_variance): with few runs the plug-in indices understate the variance, and an
        input the data say nothing about gets a plug-in index of exactly zero.  One more pass over the pairs k = k' (on the rank
        that owns the component, weighted by its A^-1 in place: lcgp_sobol_matrix_pairs) and one more reduction; the fields
        above are bitwise the same with and without it.
        order=2: the SobolIndices also carries the second-order terms second_variance[l, m] = V^c_{lm} - V_l - V_m and second
        = second_variance / V, (p_sel, d, d), symmetric with a NaN diagonal -- which inputs interact -- and with
        uncertainty=True their expectations expected_second_variance and second_expected: one more pass over the d (d - 1) / 2
        pair masks (lcgp_sobol_subset_pairs; d <= 16).  order=1 (the default) leaves them None and every other
        field bitwise what it is without the argument; any other order raises ValueError."""
        self._sobol_order(order)
        outputs = self._sobol_rows(outputs, latent)
        bs = self._marginal_box(box)
        eng = self._ensure_aux64()
        n = int(self.n)
        sr = np.sqrt(_np(self.r)) if self.submethod == 'rep' else np.ones(n, F64)
        z = self._fetch_all(lambda e, i: e.fetch_vector(1, i), n)
        scale_k, nug = self.lLmb0.numpy(), self.lnugGPs.numpy()
        w = (scale_k * (1.0 - nug / (1.0 + nug)))[:, None] * sr[None, :] * z
        V, mean = self._sobol_mean(eng, self._x_train(), w, bs, latent)
        res = self._sobol_result(V, mean, outputs, latent, (lambda: self._sobol_matrix(bs)) if uncertainty else None)
        if order == 2:
            self._sobol_second(res, (eng, self._x_train(), w, bs, lambda masks: self._sobol_subset_matrix(bs, masks)), outputs,
                               latent, uncertainty)
        return res

    # =============================================================================================
    # Closed variances of arbitrary input subsets: groups, second-order indices, Shapley effects
    # =============================================================================================
    def sobol_subsets(self, subsets, box=None, outputs=None, latent=False, uncertainty=False):
        """The closed variance V^c_u = Var_{x_u} E[f | x_u] of every subset u in `subsets` (a sequence of sequences of input
        indices; the empty and the full set are allowed) for every selected output: what a group of inputs explains together,
        exact for the product kernels as sobol_indices is (same box, measure, outputs= and latent=).  Returns a SobolSubsets
        (subsets, closed_variance (p_sel, S), closed = V^c_u / V, variance, mean).  The call appends the full set itself, so V
        and the ratios come from the same pass: lcgp_sobol_subset_pairs, lcgp_sobol_subset_chunk(d) subsets per launch over
        the pair integrals of an element, further subsets in further launches.  Float64 always; the pairs of components are
        dealt over the ranks as in sobol_indices and the result does not depend on their number.
        uncertainty=True adds expected_closed_variance = V^c_u + C_u, closed_expected and expected_variance (4.23's formula
        holds for any u; one matrix-weighted pass on the owner of each component and one more reduction).
        ValueError: an index outside [0, d), an index repeated inside a subset, d > 16."""
        outputs = self._sobol_rows(outputs, latent)
        subsets, masks = self._subset_masks(subsets)
        return self._sobol_subsets_result(self._sobol_context(box), subsets, masks, outputs, latent, uncertainty)

    def shapley_effects(self, box=None, outputs=None, latent=False, uncertainty=False):
        """Shapley effects of every input on every selected output: an attribution of the output's variance V over the box to
        the inputs whose shares ADD UP to V, interactions (and, with correlated effects, overlaps) shared equally -- between
        the first-order and the total variance of each input.  They need the closed variances of all 2^d subsets, which
        sampling cannot afford and the closed form gets from 2^d / lcgp_sobol_subset_chunk(d) passes.  Returns a
        ShapleyEffects (effects (p_sel, d), shares = effects / V, variance); the weights |u|! (d - |u| - 1)! / d! are applied
        on the host in float64.  box, outputs, latent and the ranks as in sobol_subsets.  uncertainty=True adds
        effects_expected, shares_expected and expected_variance from the posterior expectations E[V^c_u].
        ValueError: d > 10 (more than 1024 subsets)."""
        outputs = self._sobol_rows(outputs, latent)
        self._shapley_check()
        return self._shapley_result(self._sobol_context(box), outputs, latent, uncertainty)

    @staticmethod
    def _sobol_order(order):
        if order not in (1, 2) or isinstance(order, bool):
            raise ValueError('order must be 1 (first-order and total indices) or 2 (also the second-order indices), not %r' % (order,))

    def _shapley_check(self):
        if int(self.d) > 10:
            raise ValueError('shapley_effects needs the closed variances of all 2^d subsets: d = %d > 10 is refused (more than '
                             '1024 subsets)' % int(self.d))

    def _subset_masks(self, subsets):
        """the checked subsets as a list of tuples (in the order given) and their bit masks (uint64; bit l: input l is in u)"""
        d = int(self.d)
        if d > 16:
            raise ValueError('the subset pass takes at most 16 inputs (d = %d); sobol_indices() has no such limit' % d)
        if isinstance(subsets, (str, bytes)) or not hasattr(subsets, '__iter__'):
            raise ValueError('subsets must be a sequence of sequences of input indices')
        out, masks = [], []
        for u in subsets:
            if isinstance(u, (str, bytes)) or not hasattr(u, '__iter__'):
                raise ValueError('subsets must be a sequence of sequences of input indices')
            u = tuple(int(l) for l in u)
            if any(l < 0 or l >= d for l in u):
                raise ValueError('a subset holds an input index outside [0, %d): %r' % (d, u))
            if len(set(u)) != len(u):
                raise ValueError('a subset repeats an input index: %r' % (u,))
            out.append(u)
            masks.append(sum(1 << l for l in u))
        return out, np.array(masks, np.uint64)

    def _sobol_context(self, box):
        """what a subset pass works on: (float64 engine or None, centres (N, d) standardised, weights w (q, N) of the mean
        surface of ALL components, the standardised box, matrix(masks) -> C (q, nsub) of _sobol_subset_matrix)"""
        bs = self._marginal_box(box)
        eng = self._ensure_aux64()
        n = int(self.n)
        sr = np.sqrt(_np(self.r)) if self.submethod == 'rep' else np.ones(n, F64)
        z = self._fetch_all(lambda e, i: e.fetch_vector(1, i), n)
        scale_k, nug = self.lLmb0.numpy(), self.lnugGPs.numpy()
        w = (scale_k * (1.0 - nug / (1.0 + nug)))[:, None] * sr[None, :] * z
        return eng, self._x_train(), w, bs, lambda masks: self._sobol_subset_matrix(bs, masks)

    def _sobol_subset_matrix(self, bs, masks, eng=None, local_sums=None):
        """_sobol_matrix's first line for the subsets `masks`, per latent component: C (q, nsub) with
            C_u = c (prod_{l not in u} I2_l - prod_l I2_l) - sum Q (M_u - M_0)            E[V^c_u] - V^c_u(mean)
        (4.23's formula holds for any u).  Every rank evaluates the components it holds (lcgp_sobol_matrix_subset_pairs) and one
        reduction completes the array; a conditioned view passes its engine and local_sums(loc, c, Dk, sr, ell) -> sums."""
        d, q, nsub = int(self.d), int(self.q), len(masks)
        c, ell, full = self._sobol_matrix_shares(
            nsub, False, 'the matrix-weighted Sobol subset sums', eng, local_sums,
            lambda eng, v, ell, ks: eng.sobol_matrix_subset_sums(self._x_train(), v, ell, bs, ks, masks))
        width = bs[1] - bs[0]
        inside = ((np.asarray(masks, np.uint64)[:, None] >> np.arange(d, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
        prior = np.ones((q, nsub), F64)                        # prod of I2 over the inputs NOT in u, l ascending
        i2all = np.ones(q, F64)
        for k in range(q):
            for l in range(d):
                i2 = _box_double_average(self.kernel, float(width[l] / ell[k, l]))
                prior[k] = np.where(inside[:, l], prior[k], prior[k] * i2)
                i2all[k] *= i2
        return c[:, None] * (prior - i2all[:, None]) - full

    def _sobol_subset_pass(self, ctx, masks, latent, uncertainty):
        """(V (rows, nsub), mean (rows,), E (rows, nsub) or None) of ALL rows (the p outputs; latent: the q components)"""
        eng, xc, w, bs, matrix = ctx
        V, mean = self._sobol_mean(eng, xc, w, bs, latent, masks)
        E = V + self._latent_variance_to_rows(matrix(masks), latent) if uncertainty else None
        return V, mean, E

    @staticmethod
    def _ratio(num, den):
        """num / den along the first axis, NaN where den is exactly 0"""
        den = den.reshape((-1,) + (1,) * (num.ndim - 1))
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(den == 0.0, np.nan, num / den)

    def _sobol_subsets_result(self, ctx, subsets, masks, outputs, latent, uncertainty):
        d = int(self.d)
        masks = np.concatenate([masks, np.array([(1 << d) - 1], np.uint64)])           # (the full set: V from the same pass)
        V, mean, E = self._sobol_subset_pass(ctx, masks, latent, uncertainty)
        V, mean = V[outputs], mean[outputs]
        plug = (subsets, _t(V[:, :-1].copy()), _t(self._ratio(V[:, :-1], V[:, -1])), _t(V[:, -1].copy()), _t(mean.copy()))
        if not uncertainty:
            return SobolSubsets(*plug)
        E = E[outputs]
        return SobolSubsets(*plug, _t(E[:, :-1].copy()), _t(self._ratio(E[:, :-1], E[:, -1])), _t(E[:, -1].copy()))

    def _sobol_second(self, res, ctx, outputs, latent, uncertainty):
        """fills the second-order fields of the SobolIndices res from one pass over the pair masks"""
        d = int(self.d)
        il, im = np.triu_indices(d, 1)
        masks = np.array([(1 << int(l)) | (1 << int(m)) for l, m in zip(il, im)], np.uint64)

        def spread(Vc, first, var):
            sv = np.full((len(outputs), d, d), np.nan, F64)
            if len(masks):
                sv[:, il, im] = sv[:, im, il] = Vc - first[:, il] - first[:, im]
            return _t(sv), _t(self._ratio(sv, var))

        V = E = np.zeros((len(outputs), 0), F64)
        if len(masks):
            V, _, E = self._sobol_subset_pass(ctx, masks, latent, uncertainty)
            V, E = V[outputs], (E[outputs] if uncertainty else None)
        res.second_variance, res.second = spread(V, _np(res.first_variance), _np(res.variance))
        if uncertainty:
            res.expected_second_variance, res.second_expected = spread(E, _np(res.expected_first_variance), _np(res.expected_variance))

    def _shapley_result(self, ctx, outputs, latent, uncertainty):
        d = int(self.d)
        masks = np.arange(1 << d, dtype=np.uint64)             # (mask s IS the index of its column)
        V, _, E = self._sobol_subset_pass(ctx, masks, latent, uncertainty)
        size = np.array([bin(s).count('1') for s in range(1 << d)])
        fact = [float(math.factorial(j)) for j in range(d + 1)]
        wt = np.array([fact[j] * fact[d - j - 1] / fact[d] if j < d else 0.0 for j in range(d + 1)], F64)

        def effects(Vc):
            Vc = Vc[outputs]
            eff = np.zeros((len(outputs), d), F64)
            for l in range(d):
                without = np.array([s for s in range(1 << d) if not (s >> l) & 1])
                eff[:, l] = (Vc[:, without | (1 << l)] - Vc[:, without]) @ wt[size[without]]
            var = Vc[:, -1]
            return _t(eff), _t(self._ratio(eff, var)), _t(var.copy())

        if not uncertainty:
            return ShapleyEffects(*effects(V))
        return ShapleyEffects(*effects(V), *effects(E))

    def _sobol_mean(self, eng, xc, w, bs, latent, masks=None):
        """The variances of the conditional means and the box mean of a mean surface given as a kernel expansion: centres xc
        (N, d) standardised, weights w (q, N) of ALL components, on the float64 engine eng (None on a rank without components).
        Returns (V (rows, 2 d + 1), mean (rows,)) for all p outputs (latent: the q components), columns as lcgp_sobol_pairs
        orders the subsets; with masks (V (rows, nsub), mean) for those subsets (lcgp_sobol_subset_pairs).  The pairs are dealt
        round-robin over the ranks that hold an engine; one reduction assembles them."""
        q = int(self.q)
        width = 2 * int(self.d) + 1 if masks is None else len(masks)
        ell = self.lLmb.numpy()
        pairs = np.array([(k, k) for k in range(q)] if latent else [(k, kp) for k in range(q) for kp in range(k, q)], np.int32)
        rank, world = _dist.rank_world(self._group)
        mine = np.arange(rank, len(pairs), min(world, q)) if eng is not None else np.zeros(0, int)
        full = np.zeros((len(pairs), width + 1), F64)

        def share():
            if len(mine):
                full[mine, :width], full[mine, width] = (eng.sobol_pairs(xc, w, ell, bs, pairs[mine]) if masks is None else
                                                         eng.sobol_subset_pairs(xc, w, ell, bs, pairs[mine], masks))

        self._agree(share, what='the Sobol pair sums' if masks is None else 'the Sobol subset sums')
        if _dist.use_collectives(self._group):
            full = _dist.all_reduce_sum(full.reshape(-1), self._group, None if eng is None else eng.device).reshape(full.shape)
        D = np.zeros((q, q, width), F64)
        means = np.zeros(q, F64)
        for (k, kp), row in zip(pairs, full):
            D[k, kp] = D[kp, k] = row[:width]
            if k == kp:
                means[k] = row[width]
        if latent:
            V, mean = D[np.arange(q), np.arange(q)], means
        else:
            W, _, scale, offset = self._output_map()
            V = np.einsum('ka,la,klu->au', W, W, D) * (scale ** 2)[:, None]
            mean = offset + scale * (W.T @ means)
        return V, mean

    def _sobol_result(self, V, mean, outputs, latent, matrix):
        """the SobolIndices of the rows `outputs` of _sobol_mean's (V, mean); matrix: None, or a callable that returns
        _sobol_matrix's tuple (uncertainty=True: the expectations and the integrated variance are added)"""
        d = int(self.d)
        uncertainty = matrix is not None
        V, mean = V[outputs], mean[outputs]
        var = V[:, 2 * d]
        with np.errstate(divide='ignore', invalid='ignore'):
            first = np.where(var[:, None] == 0.0, np.nan, V[:, :d] / var[:, None])
            total = np.where(var[:, None] == 0.0, np.nan, 1.0 - V[:, d:2 * d] / var[:, None])
        plug = (_t(first), _t(total), _t(var.copy()), _t(mean.copy()), _t(V[:, :d].copy()), _t(V[:, d:2 * d].copy()))
        if not uncertainty:
            return SobolIndices(*plug)
        corr, iv, _ = matrix()
        E = V + self._latent_variance_to_rows(corr, latent)[outputs]
        ev = E[:, 2 * d]
        with np.errstate(divide='ignore', invalid='ignore'):
            first_e = np.where(ev[:, None] == 0.0, np.nan, E[:, :d] / ev[:, None])
            total_e = np.where(ev[:, None] == 0.0, np.nan, 1.0 - E[:, d:2 * d] / ev[:, None])
        return SobolIndices(*plug, _t(ev.copy()), _t(E[:, :d].copy()), _t(E[:, d:2 * d].copy()), _t(first_e), _t(total_e),
                            _t(self._latent_variance_to_rows(iv, latent)[outputs]))

    def integrated_variance(self, box=None, outputs=None, latent=False):
        """(p_sel,) the posterior variance of every selected output averaged over `box` ((2, d) raw scale, default the training
        inputs' bounding box; uniform measure), exact for the product kernels: IMSPE, the number a design is judged by, without
        a Monte Carlo mean of predict().  It is the variance of the CONTINUOUS surface (no nugget, as in predict_marginal): the
        box mean of predict()'s yconfvar at new inputs exceeds it by the constant scale_a^2 sum_k W_ka^2 scale_k nt_k.
        outputs: output indices (default all p); latent=True: per latent component (outputs then selects components).  The
        matrix-weighted pass of sobol_indices(uncertainty=True) alone -- none of the q (q + 1) / 2 pairs of the mean surface
        -- and bitwise that call's integrated_variance; float64 always, any number of ranks."""
        outputs = self._sobol_rows(outputs, latent)
        _, iv, _ = self._sobol_matrix(self._marginal_box(box))
        return _t(self._latent_variance_to_rows(iv, latent)[outputs])

    def _sobol_rows(self, outputs, latent):
        """the checked list of rows `outputs` selects: of the p outputs, latent: of the q components"""
        rows = int(self.q) if latent else int(self.p)
        outputs = list(range(rows)) if outputs is None else [int(a) for a in np.atleast_1d(outputs)]
        if any(a < 0 or a >= rows for a in outputs):
            raise ValueError('outputs must be indices in [0, %d)' % rows)
        return outputs

    def _latent_variance_to_rows(self, lat, latent):
        """per-component variances lat (q, ...) -> per output: scale_a^2 sum_k W_ka^2 lat[k] (latent: unchanged)"""
        if latent:
            return lat
        W, _, scale, _ = self._output_map()
        return np.tensordot((W ** 2).T, lat, axes=(1, 0)) * (scale ** 2).reshape((-1,) + (1,) * (lat.ndim - 1))

    def _sobol_matrix_shares(self, width, with_s0, what, eng, local_sums, engine_sums):
        """What _sobol_matrix and _sobol_subset_matrix begin with: (c (q,), ell (q, d), full (q, width; with_s0: S0 in one more
        column)), the matrix-weighted sums of all components.  Every rank evaluates the components it holds -- engine_sums(eng,
        v, ell, ks) on the fitted model's float64 engine, local_sums(loc, c, Dk, sr, ell) on the engine eng of a conditioned
        view -- fills their rows of a zero array, and one reduction completes it (`what` names the pass if the ranks disagree)."""
        q, n = int(self.q), int(self.n)
        if local_sums is None:
            eng = self._ensure_aux64()
        sr = np.sqrt(_np(self.r)) if self.submethod == 'rep' else np.ones(n, F64)
        ell, scale_k, nug = self.lLmb.numpy(), self.lLmb0.numpy(), self.lnugGPs.numpy()
        c = scale_k * (1.0 - nug / (1.0 + nug))
        Dk = _np(self.diag_D).reshape(-1)
        full = np.zeros((q, width + with_s0), F64)

        def share():
            if eng is not None:
                loc = [int(k) for k in self._local_ks]
                if local_sums is not None:
                    got = local_sums(loc, c, Dk, sr, ell)
                else:
                    v = (c[loc] * np.sqrt(Dk[loc]))[:, None] * sr[None, :]
                    got = engine_sums(eng, v, ell[loc], np.arange(len(loc)))
                if with_s0:
                    full[loc, :width], full[loc, width] = got
                else:
                    full[loc] = got

        self._agree(share, what=what)
        if _dist.use_collectives(self._group):
            full = _dist.all_reduce_sum(full.reshape(-1), self._group, None if eng is None else eng.device).reshape(full.shape)
        return c, ell, full

    def _sobol_matrix(self, bs, eng=None, local_sums=None):
        """What the posterior covariance of the continuous surface adds, per latent component, over the standardised box bs
        (DESIGN.md 4.23): (C (q, 2 d + 1), IV (q,), overall_var (q,)) with
            C_u = c (prod_{l not in u} I2_l - prod_l I2_l) - sum Q (M_u - M_0)      E[V_u] - V_u(mean), u as in sobol_indices
            IV  = c - S0 - sum Q (M_all - M_0)                                        the box mean of the posterior variance
            overall_var = c prod_l I2_l - S0                                          the variance of the box mean
        c = scale (1 - nt), Q = D c^2 sr sr^T o A^-1.  Every rank evaluates the components it holds on its float64 engine
        (lcgp_sobol_matrix_pairs), fills their rows of a zero array, and one reduction completes it.
        A conditioned view passes its float64 engine and local_sums(loc, c, Dk, sr, ell) -> (sums, s0) of the local
        components loc with ITS matrix Q' over n + m centres; the prior terms and the three lines above are
        the same."""
        d, q = int(self.d), int(self.q)
        c, ell, full = self._sobol_matrix_shares(
            2 * d + 1, True, 'the matrix-weighted Sobol pair sums', eng, local_sums,
            lambda eng, v, ell, ks: eng.sobol_matrix_sums(self._x_train(), v, ell, bs, ks))
        width = bs[1] - bs[0]
        prior = np.zeros((q, 2 * d + 1), F64)                  # prod of I2 over the inputs NOT in u (u = all: the empty product)
        i2all = np.ones(q, F64)
        for k in range(q):
            i2 = [_box_double_average(self.kernel, float(width[l] / ell[k, l])) for l in range(d)]
            for l in range(d):
                prior[k, l] = float(np.prod([i2[m] for m in range(d) if m != l]))
                prior[k, d + l] = i2[l]
            prior[k, 2 * d] = 1.0
            i2all[k] = float(np.prod(i2))
        sums, s0 = full[:, :2 * d + 1], full[:, 2 * d + 1]
        C = c[:, None] * (prior - i2all[:, None]) - sums
        return C, c - s0 - sums[:, 2 * d], c * i2all - s0

    # ---- cache views the reference keeps as attributes (materialised from the device only when read) ----
    def _fetch_all(self, fn, width):
        """(q, width) from per-component rows: every rank computes `fn` for the components IT holds (also any host-side
        work hidden in `fn`, e.g. the eigendecomposition behind `Ths`), then one all_gather assembles the rows."""
        eng = self._aux_engine
        rows = np.zeros((len(self._local_ks), width), F64)
        if eng is not None:
            for i in range(len(self._local_ks)):
                rows[i] = np.asarray(fn(eng, i), F64).reshape(-1)
        return _dist.gather_rows(rows, int(self.q), self._group, None if eng is None else eng.device)

    def _cache_get(self, name):
        if name in self._aux_override:
            return self._aux_override[name]
        # rank-independent decision (a rank without components has no engine but must still enter the gather):
        # only the validity of the factorisation counts, never whether THIS rank holds an engine
        if not self._aux_valid:
            n = int(self.n)
            if name in ('CinvMs', 'mks'):
                return torch.full((int(self.q), n), float('nan'), dtype=torch.float64)
            return None
        n = int(self.n)
        sr = np.sqrt(_np(self.r)) if self.submethod == 'rep' else np.ones(n, F64)
        D = _np(self.diag_D)
        if name == 'CinvMs':      # (I + D_k C_k)^-1 B_k (full, lcgp.py:708);  b_k - D_k R m_k = sqrt(r) o z_k (rep, 781)
            return _t(self._fetch_all(lambda e, i: e.fetch_vector(1, i), n) * sr[None, :])
        if name == 'mks':         # (C_k^-1 + D_k R)^-1 b_k = (beta - z) / (D_k sqrt(r))      (lcgp.py:779)
            b = self._fetch_all(lambda e, i: e.fetch_vector(0, i), n)
            z = self._fetch_all(lambda e, i: e.fetch_vector(1, i), n)
            return _t((b - z) / (D[:, None] * sr[None, :]))
        if name == 'Tks':         # C^-1 - C^-1 (C^-1 + D R)^-1 C^-1 = D R^1/2 A^-1 R^1/2      (lcgp.py:783-788)
            if self.submethod != 'rep':
                return None
            ainv = self._fetch_all(lambda e, i: e.fetch_matrix(2, i), n * n).reshape(int(self.q), n, n)
            return _t(D[:, None, None] * ainv * sr[None, :, None] * sr[None, None, :])
        if name == 'Ths':         # the reference's matrix (lcgp.py:709-715): U diag(sqrt(D / (1 + D w))) U^T, i.e. the SYMMETRIC
            # square root of D_k A_k^-1 (unique: symmetric positive definite).  predict() never needs it (it works from
            # L^-1 on the device); this view exists for callers of the reference that read the attribute, and pays an
            # eigendecomposition of A^-1 per component on the host when -- and only when -- it is read.
            if self.submethod != 'full':
                return None
            # Each rank takes the square root of the components it OWNS (one eigendecomposition per owned component, not q
            # on every rank) and the finished rows are gathered.
            def sqrt_owned(e, i):
                ainv = e.fetch_matrix(2, i)
                lam, vec = np.linalg.eigh(0.5 * (ainv + ainv.T))
                return (vec * np.sqrt(D[self._local_ks[i]] * np.maximum(lam, 0.0))[None, :]) @ vec.T
            return _t(self._fetch_all(sqrt_owned, n * n).reshape(int(self.q), n, n))
        raise AttributeError(name)

    def _cache_set(self, name, value):
        self._aux_override[name] = value

    CinvMs = property(lambda self: self._cache_get('CinvMs'), lambda self, v: self._cache_set('CinvMs', v))
    mks = property(lambda self: self._cache_get('mks'), lambda self, v: self._cache_set('mks', v))
    Tks = property(lambda self: self._cache_get('Tks'), lambda self, v: self._cache_set('Tks', v))
    Ths = property(lambda self: self._cache_get('Ths'), lambda self, v: self._cache_set('Ths', v))
