"""Timing of the input Hessians and the gradient covariance of a conditioned view (ConditionedLCGP.predict_hess /
predict_grad_cov) at the headline shape (n = 4096, d = 6, p = 64, q = 8), m in --ms new runs and --rows new inputs, float64 and
float32, next to the fitted model's own queries and to the route that exists without the feature, in the same process on the
same sets.

Per dtype and m, median of --reps after a warm-up, each window bracketed by device events on the current stream:
  (a) the view's passes: HotPathEngine.condition_predict_hess_block and condition_grad_cov_block on --rows rows (grad state in
      place);
  (b) predict_hess_block / grad_cov_block of the fitted model on as many rows;
  (c) the route without the feature: a HotPathEngine built on the n + m points, one evaluation plus its own block.
Stated in the output: (a) / (b) beside the flop ratio 1 + m (2 npad + mpad) / npad^2 (mpad = m rounded up to 128) and whether
it is within 1.5 x that ratio; whether (a) is below (c); the clock the chip held (lcgp_lauum_clock of an evaluation before and
after).  --only view: just (a), for a kernel trace.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lcgp_amd import LCGP, synth  # noqa: E402
from lcgp_amd.engine import HotPathEngine  # noqa: E402
from tools.condition_grad_bench import clock_mhz  # noqa: E402
from tools.vr_bench import device_ms, pad  # noqa: E402


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
    out = dict(n=cfg['n'], d=cfg['d'], p=cfg['p'], q=cfg['q'], n0=a.rows, reps=a.reps)
    npad = pad(cfg['n'], 128)
    for dt in a.dtypes.split(','):
        m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0', dtype=dt)
        m.loss_and_grad(m._get_flat())
        eng = m._aux_engine
        x0s, xt = m._standardise_x0(x0)[0], m._x_train()
        th = eng._theta_last.copy()
        res = dict(engine=eng.dtype_name)
        res['clock_mhz_before'] = clock_mhz(eng)
        if a.only == 'all':
            res['predict_hess_ms'] = device_ms(lambda: eng.predict_hess_block(x0s), a.reps)
            res['grad_cov_ms'] = device_ms(lambda: eng.grad_cov_block(x0s), a.reps)
        for k in [int(v) for v in a.ms.split(',')]:
            xn = lo + (hi - lo) * rng.random((k, x.shape[1]))
            yn = rng.standard_normal((cfg['p'], k))
            xn_s = m._standardise_x0(xn)[0]
            ys = (yn - m.ymean.numpy()) / m.ystd.numpy()
            t = (th[:, cfg['d'] + 3:] @ ys) / th[:, cfg['d'] + 2][:, None]
            state = eng.condition_begin(xn_s, t, None)
            eng.condition_predict_grad_block(state, x0s[:64])            # (builds the grad state)
            r = dict(view_hess_ms=device_ms(lambda: eng.condition_predict_hess_block(state, x0s), a.reps),
                     view_grad_cov_ms=device_ms(lambda: eng.condition_grad_cov_block(state, x0s), a.reps))
            if a.only == 'all':
                xa, Ya = np.vstack([xt, xn_s]), np.hstack([m.y.numpy(), ys])
                aug = HotPathEngine(xa, Ya, None, q_local=eng.q_local, kernel=m.kernel, dtype=dt)

                def parent(block):
                    aug.upload_theta(th)
                    aug.enqueue()
                    block(x0s)

                r['parent_eval_hess_ms'] = device_ms(lambda: parent(aug.predict_hess_block), a.reps)
                r['parent_eval_grad_cov_ms'] = device_ms(lambda: parent(aug.grad_cov_block), a.reps)
                r['flop_ratio'] = 1.0 + k * (2.0 * npad + pad(k, 128)) / float(npad) ** 2
                for what, base in (('hess', 'predict_hess_ms'), ('grad_cov', 'grad_cov_ms')):
                    r[what + '_ratio'] = r['view_%s_ms' % what] / res[base]
                    r[what + '_within_1p5_of_flop_ratio'] = bool(r[what + '_ratio'] <= 1.5 * r['flop_ratio'])
                    r[what + '_below_parent_route'] = bool(r['view_%s_ms' % what] < r['parent_eval_%s_ms' % what])
                del aug
            res['m=%d' % k] = r
            del state
            torch.cuda.empty_cache()
        m.loss_and_grad(m._get_flat())
        res['clock_mhz_after'] = clock_mhz(m._aux_engine)
        out[dt] = res
        del m, eng
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
