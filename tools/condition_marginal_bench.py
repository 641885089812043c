"""Timing of the box averages on a conditioned view and of the covariance with a reference row
(HotPathEngine.predict_marginal_block(x0s, mask, box, state, ref)) at the headline shape (n = 4096, d = 6, p = 64, q = 8), --rows
rows that keep one dimension each, m in --ms new runs, float64 and float32, next to the queries it is built from and to the
route that exists without it, in the same process on the same sets.

Per dtype and m the windows below are taken ALTERNATELY, --reps rounds after a warm-up round, each window bracketed by device
events on the current stream (it also holds the host-to-device copies of the rows, masks and box); medians:
  (a) the view's marginal pass;                       (a_ref) the same with a reference row (the overall row)
  (b) the base model's marginal pass;                 (b_ref) the same with a reference row
  (c) HotPathEngine.condition_predict_block on as many rows;
  (d) the route without this query: a HotPathEngine built on the n + m points (construction by the wall clock), one
      evaluation and its marginal pass (device events); (d) is their sum, beside prepare + (a) of the view.
Reported, not asserted: (a) / (b) beside the flop ratio 1 + m (2 npad + mpad) / npad^2 (mpad = m rounded up to 128) and whether it
is within 1.5 x that ratio; (a_ref) - (a) and (b_ref) - (b) beside the bytes the reference row makes the pass read again (the U
and T rows: q rows (n + m) elements, and the one-row pass in front).  --only view: just (a) and (a_ref), for a kernel trace.
Prints one JSON line."""
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


def alternating_ms(fns, reps):
    """median device-event time of every fns[name](), the windows taken in turn: one warm-up round, then reps rounds"""
    ts = {k: [] for k in fns}
    for rnd in range(reps + 1):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if rnd:
                ts[k].append(a.elapsed_time(b))
    return {k: float(np.median(v)) for k, v in ts.items()}


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
    d, q = cfg['d'], cfg['q']
    lo, hi = x.min(axis=0), x.max(axis=0)
    rng = np.random.default_rng(1)
    x0s = rng.random((a.rows, d))                                   # standardised: the training inputs' bounding box
    mask = np.ones((a.rows, d), bool)
    mask[np.arange(a.rows), np.arange(a.rows) % d] = False          # every row keeps one dimension
    box = np.stack([np.zeros(d), np.ones(d)])
    ref = (np.zeros(d), np.ones(d, bool))                           # the overall row
    out = dict(n=cfg['n'], d=d, p=cfg['p'], q=q, n0=a.rows)
    npad = pad(cfg['n'], 128)
    for dt in a.dtypes.split(','):
        m = LCGP(y=y, x=x, q=q, device='cuda:0', dtype=dt)
        m.loss_and_grad(m._get_flat())
        eng = m._aux_engine
        xt = m._x_train()
        th = eng._theta_last.copy()
        esz = 8 if eng.dtype_name == 'float64' else 4
        res = dict(engine=eng.dtype_name)
        for k in [int(v) for v in a.ms.split(',')]:
            xn = lo + (hi - lo) * rng.random((k, d))
            yn = rng.standard_normal((cfg['p'], k))
            xn_s = m._standardise_x0(xn)[0]
            ys = (yn - m.ymean.numpy()) / m.ystd.numpy()
            t = (th[:, d + 3:] @ ys) / th[:, d + 2][:, None]
            state = eng.condition_begin(xn_s, t, None)
            fns = {'view_marginal_ms': lambda: eng.predict_marginal_block(x0s, mask, box, state=state),
                   'view_marginal_ref_ms': lambda: eng.predict_marginal_block(x0s, mask, box, state=state, ref=ref)}
            if a.only == 'all':
                fns.update({'marginal_ms': lambda: eng.predict_marginal_block(x0s, mask, box),
                            'marginal_ref_ms': lambda: eng.predict_marginal_block(x0s, mask, box, ref=ref),
                            'view_predict_ms': lambda: eng.condition_predict_block(state, x0s)})
            r = alternating_ms(fns, a.reps)
            r['ref_bytes_view'] = q * (a.rows + 1) * (cfg['n'] + k) * esz
            r['ref_bytes_model'] = q * (a.rows + 1) * cfg['n'] * esz
            r['ref_cost_view_ms'] = r['view_marginal_ref_ms'] - r['view_marginal_ms']
            if a.only == 'all':
                r['ref_cost_model_ms'] = r['marginal_ref_ms'] - r['marginal_ms']
                r['prepare_ms'] = device_ms(lambda: eng.condition_begin(xn_s, t, None), a.reps)
                xa, Ya = np.vstack([xt, xn_s]), np.hstack([m.y.numpy(), ys])
                made = []

                def construct():
                    made.clear()
                    made.append(HotPathEngine(xa, Ya, None, q_local=eng.q_local, kernel=m.kernel, dtype=dt))

                r['parent_construct_ms'] = wall_ms(construct, 3)
                aug = made[0]

                def parent():
                    aug.evaluate(th)
                    aug.predict_marginal_block(x0s, mask, box)

                r['parent_eval_marginal_ms'] = device_ms(parent, a.reps)
                r['parent_route_ms'] = r['parent_construct_ms'] + r['parent_eval_marginal_ms']
                r['view_route_ms'] = r['prepare_ms'] + r['view_marginal_ms']
                r['marginal_ratio'] = r['view_marginal_ms'] / r['marginal_ms']
                r['view_marginal_over_view_predict'] = r['view_marginal_ms'] / r['view_predict_ms']
                r['flop_ratio'] = 1.0 + k * (2.0 * npad + pad(k, 128)) / float(npad) ** 2
                r['within_1p5_of_flop_ratio'] = bool(r['marginal_ratio'] <= 1.5 * r['flop_ratio'])
                del aug, made
            res['m=%d' % k] = r
            del state
            torch.cuda.empty_cache()
        out[dt] = res
        del m, eng
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
