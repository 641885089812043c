"""Timing of the input gradients and the calibration target of a conditioned view (ConditionedLCGP.predict_grad /
calibration) at the headline shape (n = 4096, d = 6, p = 64, q = 8), m in --ms new runs and --rows new inputs, float64 and
float32, next to the route that exists without them, in the same process on the same sets.

Per dtype and m, median of --reps after a warm-up, each window bracketed by device events on the current stream:
  (a) grad prepare: lcgp_condition_grad_prepare (w and z' of the view; three bandwidth-bound products);
  (b) view gradient pass: HotPathEngine.condition_predict_grad_block on --rows rows (grad state in place);
  (c) predict_grad_block of the fitted model on as many rows;
  (d) the route without the feature: a HotPathEngine built on the n + m points (construction by the wall clock), one
      evaluation and its predict_grad_block (device events); (d) is their sum.
Stated in the output: (b) / (c) beside the flop ratio 1 + m (2 npad + mpad) / npad^2 (mpad = m rounded up to 128) and whether
it is within 1.5 x that ratio; view.calibration(...).loglik_grad for 64 and --rows rows beside the base target's (wall clock,
host layer included); the clock the chip held (lcgp_lauum_clock of an evaluation before and after).  --only view: just (a)
and (b), for a kernel trace.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lcgp_amd import LCGP, _hip, synth  # noqa: E402
from lcgp_amd.engine import HotPathEngine  # noqa: E402
from tools.vr_bench import device_ms, pad, wall_ms  # noqa: E402


def grad_prepare(eng, state):
    """lcgp_condition_grad_prepare into the view's existing grad state (what condition_predict_grad_block does on first use)"""
    _hip.check(eng.lib.lcgp_condition_grad_prepare(
        eng._stream(), eng.dtype, eng.n, eng.d, eng.p, eng.q_local, eng._p(eng.theta_dev), eng._p(eng.workspace),
        eng._p(state['state']), state['m'], eng._p(state['grad'])), "lcgp_condition_grad_prepare")


def clock_mhz(eng):
    """the clock the chip held in the A^-1 launch of the engine's last evaluation (lcgp_lauum_clock), as bench.py reports it"""
    clk = torch.zeros(2, dtype=torch.int64, device='cuda:0')
    eng.lib.lcgp_lauum_clock(eng._stream(), eng.dtype, eng.n, eng.d, eng.p, eng.q_local, eng._p(eng.workspace), eng._p(clk))
    c = clk.cpu().numpy()
    return 100.0 * c[0] / c[1] if c[1] else float('nan')


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
        y_obs = np.asarray(y)[:, 7] + 0.1 * np.asarray(y).std(axis=1)
        if a.only == 'all':
            res['predict_grad_ms'] = device_ms(lambda: eng.predict_grad_block(x0s), a.reps)
            base_t = m.calibration(y_obs, 0.1)
            for rows in (64, a.rows):
                res['base_loglik_grad_%d_ms' % rows] = wall_ms(lambda: base_t.loglik_grad(x0[:rows]), a.reps)
        for k in [int(v) for v in a.ms.split(',')]:
            xn = lo + (hi - lo) * rng.random((k, x.shape[1]))
            yn = rng.standard_normal((cfg['p'], k))
            xn_s = m._standardise_x0(xn)[0]
            ys = (yn - m.ymean.numpy()) / m.ystd.numpy()
            t = (th[:, cfg['d'] + 3:] @ ys) / th[:, cfg['d'] + 2][:, None]
            state = eng.condition_begin(xn_s, t, None)
            eng.condition_predict_grad_block(state, x0s[:64])            # (builds the grad state)
            r = dict(grad_prepare_ms=device_ms(lambda: grad_prepare(eng, state), a.reps),
                     view_grad_ms=device_ms(lambda: eng.condition_predict_grad_block(state, x0s), a.reps))
            if a.only == 'all':
                r['view_predict_ms'] = device_ms(lambda: eng.condition_predict_block(state, x0s), a.reps)
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
                    aug.predict_grad_block(x0s)

                r['parent_eval_grad_ms'] = device_ms(parent, a.reps)
                r['parent_route_ms'] = r['parent_construct_ms'] + r['parent_eval_grad_ms']
                r['grad_ratio'] = r['view_grad_ms'] / res['predict_grad_ms']
                r['flop_ratio'] = 1.0 + k * (2.0 * npad + pad(k, 128)) / float(npad) ** 2
                r['within_1p5_of_flop_ratio'] = bool(r['grad_ratio'] <= 1.5 * r['flop_ratio'])
                view = m.condition(xn, yn)
                tgt = view.calibration(y_obs, 0.1)
                tgt.loglik_grad(x0[:64])
                for rows in (64, a.rows):
                    r['view_loglik_grad_%d_ms' % rows] = wall_ms(lambda: tgt.loglik_grad(x0[:rows]), a.reps)
                del aug, made, view, tgt
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
