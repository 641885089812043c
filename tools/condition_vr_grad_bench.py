"""Timing of the ALC gradient on a conditioned view (ConditionedLCGP.variance_reduction_grad) at the headline shape (n = 4096,
d = 6, p = 64, q = 8), n_ref = n_cand = --cands, m in --ms new runs, float64 and float32, next to the base model's gradient and
to the two routes that exist without it, in the same process on the same sets.

Per dtype and m, median of --reps after a warm-up, each window bracketed by device events on the current stream (the windows
also hold the host-to-device copies of the inputs):
  (a) view grad: HotPathEngine.condition_variance_reduction_grad_block (reference set given explicitly);
  (b) base grad: HotPathEngine.variance_reduction_grad_block on the same sets;
  (c) the refit route: on an engine built on the n + m points, one evaluation (refactorisation) and its
      variance_reduction_grad_block; its construction (allocation and uploads) is left out of the window, in the view's favour it
      would only add;
  (d) the central differences the gradient replaces: 2 d condition_variance_reduction_block calls on the same sets.
Reported beside them: (a) / (b) and the flop ratio of the two calls from the shapes (include/lcgp_hip.h) -- per component, the
row formers of both sets (npad^2 per row against npad^2 + 2 mpad npad + mpad^2), the fused product 2 n_ref64 n_cand64 K, P and G
(4 C n_refpad K), Q and V (2 C npad^2), and on the view Q_n, R_c (2 C mpad^2) and the two products with U_n (4 C mpad npad), with
K = npad against K' = npad + mpad; whether (a) < (c) and (a) < (d); and the clock the chip held in the A^-1 launch of the model's
evaluation before and after the measurements (lcgp_lauum_clock), as bench.py reports it.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lcgp_amd import LCGP, synth  # noqa: E402
from lcgp_amd.engine import HotPathEngine  # noqa: E402
from tools.vr_bench import device_ms, pad, upad, wall_ms  # noqa: E402


def flops(n, m, n_ref, n_cand):
    """flops per component of one gradient call (m = 0: the fitted model's)"""
    npad, mpad = pad(n, 128), pad(m, 128) if m else 0
    kp = npad + mpad
    c, rp = upad(n_cand), pad(n_ref, 128)
    rows = (upad(n_ref) + c) * (npad ** 2 + 2.0 * mpad * npad + mpad ** 2)
    fused = 2.0 * pad(n_ref, 64) * pad(n_cand, 64) * kp
    return rows + fused + 4.0 * c * rp * kp + 2.0 * c * npad ** 2 + 2.0 * c * mpad ** 2 + 4.0 * c * mpad * npad


def clock_mhz(eng):
    """the clock the chip held in the A^-1 launch of the engine's last evaluation (lcgp_lauum_clock), as bench.py reports it"""
    clk = torch.zeros(2, dtype=torch.int64, device='cuda:0')
    eng.lib.lcgp_lauum_clock(eng._stream(), eng.dtype, eng.n, eng.d, eng.p, eng.q_local, eng._p(eng.workspace), eng._p(clk))
    c = clk.cpu().numpy()
    return 100.0 * c[0] / c[1] if c[1] else float('nan')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ms', default='32,256,1024')
    ap.add_argument('--cands', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtypes', default='float64,float32')
    a = ap.parse_args()
    x, y, cfg = synth.make_config(3)
    x = np.asarray(x)
    d = cfg['d']
    lo, hi = x.min(axis=0), x.max(axis=0)
    rng = np.random.default_rng(1)
    xc = lo + (hi - lo) * rng.random((a.cands, d))
    w = np.full(a.cands, 1.0 / a.cands)
    out = dict(n=cfg['n'], d=d, p=cfg['p'], q=cfg['q'], n_ref=a.cands, n_cand=a.cands, device=torch.cuda.get_device_name(0))
    for dt in a.dtypes.split(','):
        m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0', dtype=dt)
        m.loss_and_grad(m._get_flat())
        eng = m._aux_engine
        xc_s, xt = m._standardise_x0(xc)[0], m._x_train()
        th = eng._theta_last.copy()
        res = dict(engine=eng.dtype_name, clock_mhz_before=clock_mhz(eng),
                   base_grad_ms=device_ms(lambda: eng.variance_reduction_grad_block(xc_s, xc_s, w, 1), a.reps),
                   base_vr_ms=device_ms(lambda: eng.variance_reduction_block(xc_s, xc_s, w, None, 1), a.reps))
        for k in [int(v) for v in a.ms.split(',')]:
            xn = lo + (hi - lo) * rng.random((k, d))
            yn = rng.standard_normal((cfg['p'], k))
            xn_s = m._standardise_x0(xn)[0]
            ys = (yn - m.ymean.numpy()) / m.ystd.numpy()
            t = (th[:, d + 3:] @ ys) / th[:, d + 2][:, None]
            state = eng.condition_begin(xn_s, t, None)
            steps = [np.eye(d)[l] * s * 1e-5 for l in range(d) for s in (1.0, -1.0)]

            def central_differences():
                for e in steps:
                    eng.condition_variance_reduction_block(state, xc_s + e[None, :], xc_s, w, None, 1)

            r = dict(view_grad_ms=device_ms(lambda: eng.condition_variance_reduction_grad_block(state, xc_s, xc_s, w, 1), a.reps),
                     view_vr_ms=device_ms(lambda: eng.condition_variance_reduction_block(state, xc_s, xc_s, w, None, 1), a.reps),
                     central_differences_ms=device_ms(central_differences, a.reps))
            aug = HotPathEngine(np.vstack([xt, xn_s]), np.hstack([m.y.numpy(), ys]), None, q_local=eng.q_local, kernel=m.kernel,
                                dtype=dt)
            aug.evaluate(th)

            def refit_grad():
                aug.upload_theta(th)
                aug.enqueue()
                aug.variance_reduction_grad_block(xc_s, xc_s, w, 1)

            r['refit_eval_ms'] = device_ms(aug.enqueue, a.reps)
            r['refit_grad_ms'] = device_ms(refit_grad, a.reps)
            r['grad_ratio_view_over_base'] = r['view_grad_ms'] / res['base_grad_ms']
            r['flop_ratio'] = flops(cfg['n'], k, a.cands, a.cands) / flops(cfg['n'], 0, a.cands, a.cands)
            r['ratio_over_flop_ratio'] = r['grad_ratio_view_over_base'] / r['flop_ratio']
            r['view_grad_over_refit'] = r['view_grad_ms'] / r['refit_grad_ms']
            r['view_grad_over_central_differences'] = r['view_grad_ms'] / r['central_differences_ms']
            r['view_grad_below_refit'] = bool(r['view_grad_ms'] < r['refit_grad_ms'])
            r['view_grad_below_central_differences'] = bool(r['view_grad_ms'] < r['central_differences_ms'])
            view = m.condition(xn, yn)
            r['api_view_grad_ms'] = wall_ms(lambda: view.variance_reduction_grad(xc, x_ref=xc), 3)
            res['m=%d' % k] = r
            del state, aug, view
            torch.cuda.empty_cache()
        m.loss_and_grad(m._get_flat())
        res['clock_mhz_after'] = clock_mhz(m._aux_engine)
        out[dt] = res
        del m, eng
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
