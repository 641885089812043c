"""Timing of conditioning on new runs (LCGP.condition / ConditionedLCGP.predict) at the headline shape (n = 4096, d = 6, p = 64,
q = 8), m in --ms new runs and --rows new inputs, float64 and float32, next to the route that exists without it, in the same
process on the same sets.

Per dtype and m, median of --reps after a warm-up, each window bracketed by device events on the current stream:
  (a) prepare: HotPathEngine.condition_begin (U_n, S, its factorisation and inverse, v; the window also holds the
      host-to-device copies and the read-back of the info words);
  (b) view predict: HotPathEngine.condition_predict_block on --rows rows;
  (c) predict: HotPathEngine.predict_block on as many rows;
  (d) the parent route: a HotPathEngine built on the n + m points, one evaluation and one predict_block.  The construction
      (allocation, zero fill and uploads) is timed by the wall clock, evaluation + predict by device events; (d) is their sum.
Conditions, stated in the output: (a) + (b) < (d); (b) / (c) beside the flop ratio 1 + m (2 npad + mpad) / npad^2 (mpad = m
rounded up to 128), and whether it is within 1.5 x that ratio.  --only view: just (a) and (b), for a kernel trace.  Prints one
JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lcgp_amd import LCGP, synth  # noqa: E402
from lcgp_amd.engine import HotPathEngine  # noqa: E402
from tools.vr_bench import device_ms, pad, wall_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ms', default='32,256,1024')
    ap.add_argument('--rows', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtypes', default='float64,float32')
    ap.add_argument('--only', default='all', choices=['all', 'view'])
    a = ap.parse_args()
    x, y, cfg = synth.make_config(3)
    x = np.asarray(x)
    lo, hi = x.min(axis=0), x.max(axis=0)
    rng = np.random.default_rng(1)
    x0 = lo + (hi - lo) * rng.random((a.rows, x.shape[1]))
    out = dict(n=cfg['n'], d=cfg['d'], p=cfg['p'], q=cfg['q'], n0=a.rows)
    npad = pad(cfg['n'], 128)
    for dt in a.dtypes.split(','):
        m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0', dtype=dt)
        m.loss_and_grad(m._get_flat())
        eng = m._aux_engine
        x0s, xt = m._standardise_x0(x0)[0], m._x_train()
        th = eng._theta_last.copy()
        res = dict(engine=eng.dtype_name)
        if a.only == 'all':
            res['predict_ms'] = device_ms(lambda: eng.predict_block(x0s), a.reps)
        for k in [int(v) for v in a.ms.split(',')]:
            xn = lo + (hi - lo) * rng.random((k, x.shape[1]))
            yn = rng.standard_normal((cfg['p'], k))
            xn_s = m._standardise_x0(xn)[0]
            ys = (yn - m.ymean.numpy()) / m.ystd.numpy()
            t = (th[:, cfg['d'] + 3:] @ ys) / th[:, cfg['d'] + 2][:, None]
            state = eng.condition_begin(xn_s, t, None)
            r = dict(prepare_ms=device_ms(lambda: eng.condition_begin(xn_s, t, None), a.reps),
                     view_predict_ms=device_ms(lambda: eng.condition_predict_block(state, x0s), a.reps))
            if a.only == 'all':
                xa, Ya = np.vstack([xt, xn_s]), np.hstack([m.y.numpy(), ys])
                made = []

                def construct():
                    made.clear()
                    made.append(HotPathEngine(xa, Ya, None, q_local=eng.q_local, kernel=m.kernel, dtype=dt))

                r['parent_construct_ms'] = wall_ms(construct, 3)
                aug = made[0]

                def parent():
                    aug.upload_theta(th)
                    aug.enqueue()
                    aug.predict_block(x0s)

                r['parent_eval_predict_ms'] = device_ms(parent, a.reps)
                r['parent_route_ms'] = r['parent_construct_ms'] + r['parent_eval_predict_ms']
                r['view_route_ms'] = r['prepare_ms'] + r['view_predict_ms']
                r['condition_view_below_parent'] = bool(r['view_route_ms'] < r['parent_route_ms'])
                r['condition_view_below_parent_without_construction'] = bool(r['view_route_ms'] < r['parent_eval_predict_ms'])
                r['predict_ratio'] = r['view_predict_ms'] / res['predict_ms']
                r['flop_ratio'] = 1.0 + k * (2.0 * npad + pad(k, 128)) / float(npad) ** 2
                r['within_1p5_of_flop_ratio'] = bool(r['predict_ratio'] <= 1.5 * r['flop_ratio'])
                r['api_condition_ms'] = wall_ms(lambda: m.condition(xn, yn), 3)
                view = m.condition(xn, yn)
                r['api_view_predict_ms'] = wall_ms(lambda: view.predict(x0), 3)
                del aug, made, view
            res['m=%d' % k] = r
            del state
            torch.cuda.empty_cache()
        out[dt] = res
        del m, eng
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
