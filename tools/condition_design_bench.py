"""Timing of the design queries on a conditioned view (ConditionedLCGP.variance_reduction / select_batch) at the headline shape
(n = 4096, d = 6, p = 64, q = 8), n_ref = n_cand = --cands, m in --ms new runs, float64 and float32, next to the base model's
queries and to the route that exists without the view, in the same process on the same sets.

Per dtype and m, median of --reps after a warm-up, each window bracketed by device events on the current stream (the windows
also hold the host-to-device copies of the inputs):
  (a) view vr: HotPathEngine.condition_variance_reduction_block (reference set given explicitly);
  (b) base vr: HotPathEngine.variance_reduction_block on the same sets;
  (c) the route the view replaces: on an engine built on the n + m points, one evaluation (refactorisation) and its
      variance_reduction_block; its construction (allocation and uploads) is left out of the window, in the view's favour it
      would only add;
  (d) select: condition_select_batch_block(size) next to select_batch_block of the base model and to evaluation +
      select_batch_block of the engine of (c).
  prepare: condition_begin, what the view costs before its first query.
Reported beside them: (a) / (b) and the flop ratio of the two from the shapes -- per component and row of either set npad^2 (U)
against npad^2 + 2 mpad npad + mpad^2 (U, Sigma_an, T), and the fused product 2 n_ref64 n_cand64 npad against the same with
K' = npad + mpad; whether (a) < (c) and view select < (c)'s select; and the clock the chip held in the A^-1 launch of the
model's evaluation (lcgp_lauum_clock), as bench.py reports it.  Prints one JSON line."""
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


def flop_ratio(n, m, n_ref, n_cand):
    npad, mpad = pad(n, 128), pad(m, 128)
    rows = upad(n_ref) + upad(n_cand)
    fused = 2.0 * pad(n_ref, 64) * pad(n_cand, 64)
    base = rows * npad ** 2 + fused * npad
    view = rows * (npad ** 2 + 2.0 * mpad * npad + mpad ** 2) + fused * (npad + mpad)
    return view / base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ms', default='32,256,1024')
    ap.add_argument('--cands', type=int, default=2000)
    ap.add_argument('--size', type=int, default=32)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtypes', default='float64,float32')
    a = ap.parse_args()
    x, y, cfg = synth.make_config(3)
    x = np.asarray(x)
    lo, hi = x.min(axis=0), x.max(axis=0)
    rng = np.random.default_rng(1)
    xc = lo + (hi - lo) * rng.random((a.cands, x.shape[1]))
    w = np.full(a.cands, 1.0 / a.cands)
    out = dict(n=cfg['n'], d=cfg['d'], p=cfg['p'], q=cfg['q'], n_ref=a.cands, n_cand=a.cands, size=a.size,
               device=torch.cuda.get_device_name(0))
    for dt in a.dtypes.split(','):
        m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0', dtype=dt)
        m.loss_and_grad(m._get_flat())
        eng = m._aux_engine
        clk = torch.zeros(2, dtype=torch.int64, device='cuda:0')
        eng.lib.lcgp_lauum_clock(eng._stream(), eng.dtype, eng.n, eng.d, eng.p, eng.q_local, eng._p(eng.workspace), eng._p(clk))
        c = clk.cpu().numpy()
        xc_s, xt = m._standardise_x0(xc)[0], m._x_train()
        th = eng._theta_last.copy()
        W, _, scale, _ = m._output_map()
        om = np.mean(W ** 2 * (scale ** 2)[None, :], axis=1)
        res = dict(engine=eng.dtype_name, clock_mhz=100.0 * c[0] / c[1] if c[1] else float('nan'),
                   base_vr_ms=device_ms(lambda: eng.variance_reduction_block(xc_s, xc_s, w, None, 1), a.reps),
                   base_select_ms=device_ms(lambda: eng.select_batch_block(xc_s, xc_s, w, None, 1, a.size, om), a.reps))
        for k in [int(v) for v in a.ms.split(',')]:
            xn = lo + (hi - lo) * rng.random((k, x.shape[1]))
            yn = rng.standard_normal((cfg['p'], k))
            xn_s = m._standardise_x0(xn)[0]
            ys = (yn - m.ymean.numpy()) / m.ystd.numpy()
            t = (th[:, cfg['d'] + 3:] @ ys) / th[:, cfg['d'] + 2][:, None]
            state = eng.condition_begin(xn_s, t, None)
            r = dict(prepare_ms=device_ms(lambda: eng.condition_begin(xn_s, t, None), a.reps),
                     view_vr_ms=device_ms(lambda: eng.condition_variance_reduction_block(state, xc_s, xc_s, w, None, 1), a.reps),
                     view_select_ms=device_ms(lambda: eng.condition_select_batch_block(state, xc_s, xc_s, w, None, 1, a.size, om),
                                              a.reps))
            aug = HotPathEngine(np.vstack([xt, xn_s]), np.hstack([m.y.numpy(), ys]), None, q_local=eng.q_local, kernel=m.kernel,
                                dtype=dt)
            aug.evaluate(th)

            def refit_vr():
                aug.upload_theta(th)
                aug.enqueue()
                aug.variance_reduction_block(xc_s, xc_s, w, None, 1)

            def refit_select():
                aug.upload_theta(th)
                aug.enqueue()
                aug.select_batch_block(xc_s, xc_s, w, None, 1, a.size, om)

            r['refit_eval_ms'] = device_ms(aug.enqueue, a.reps)
            r['refit_vr_ms'] = device_ms(refit_vr, a.reps)
            r['refit_select_ms'] = device_ms(refit_select, a.reps)
            r['vr_ratio_view_over_base'] = r['view_vr_ms'] / res['base_vr_ms']
            r['flop_ratio'] = flop_ratio(cfg['n'], k, a.cands, a.cands)
            r['select_ratio_view_over_base'] = r['view_select_ms'] / res['base_select_ms']
            r['row_ratio'] = (pad(cfg['n'], 128) + pad(k, 128)) / float(pad(cfg['n'], 128))
            r['view_vr_below_refit'] = bool(r['view_vr_ms'] < r['refit_vr_ms'])
            r['prepare_plus_view_vr_below_refit'] = bool(r['prepare_ms'] + r['view_vr_ms'] < r['refit_vr_ms'])
            r['view_select_below_refit'] = bool(r['view_select_ms'] < r['refit_select_ms'])
            view = m.condition(xn, yn)
            r['api_view_vr_ms'] = wall_ms(lambda: view.variance_reduction(xc, x_ref=xc), 3)
            r['api_view_select_ms'] = wall_ms(lambda: view.select_batch(xc, a.size, x_ref=xc), 3)
            res['m=%d' % k] = r
            del state, aug, view
            torch.cuda.empty_cache()
        out[dt] = res
        del m, eng
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
