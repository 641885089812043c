"""Timing of the joint covariance and the draws on a conditioned view (ConditionedLCGP.predict_latent_cov / sample) at the
headline shape (n = 4096, d = 6, p = 64, q = 8), n0 = --n0 new inputs, m in --ms new runs, float64 and float32, next to the base
model's queries and to the route that exists without the view, in the same process on the same inputs.

Per dtype and m, median of --reps after a warm-up, each window bracketed by device events on the current stream (the windows
also hold the host-to-device copy of the inputs, and for the draws the host-side normals):
  (a) view cov: HotPathEngine._form_cov(state, ...) -- lcgp_condition_predict_cov, the covariance into the cov workspace;
  (b) base cov: HotPathEngine.form_cov -- lcgp_predict_cov of the base model on as many rows;
  (c) the route the view replaces: on an engine built on the n + m points, one evaluation (refactorisation) and its form_cov;
      its construction (allocation and uploads) is left out of the window, in the view's favour it would only add;
  the same three for --draws latent draws (condition_sample_latent / sample_latent: the prediction, the covariance, its
  factorisation, the normals and the product), at the jitter tests/test_gpu_joint_bounds.py takes at this shape.
  prepare: condition_begin, what the view costs before its first query.
Reported beside them: (a) / (b) and the flop ratio of the two from the shapes,
    (n0pad^2 K' + n0pad (npad^2 + 2 mpad npad + mpad^2)) / (n0pad^2 npad + n0pad npad^2),
whether prepare + (a) < (c), and the clock the chip held in the A^-1 launch of the model's evaluation (lcgp_lauum_clock), as
bench.py reports it.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lcgp_amd import LCGP, synth  # noqa: E402
from lcgp_amd.engine import HotPathEngine  # noqa: E402
from tools.vr_bench import device_ms, pad  # noqa: E402

JITTER = {'float64': 1e-8, 'float32': 1e-2}


def flop_ratio(n, m, n0):
    npad, mpad, n0pad = pad(n, 128), pad(m, 128), pad(n0, 128)
    view = n0pad ** 2 * (npad + mpad) + n0pad * (npad ** 2 + 2.0 * mpad * npad + mpad ** 2)
    return view / (n0pad ** 2 * npad + n0pad * float(npad) ** 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ms', default='32,256,1024')
    ap.add_argument('--n0', type=int, default=2000)
    ap.add_argument('--draws', type=int, default=100)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtypes', default='float64,float32')
    a = ap.parse_args()
    x, y, cfg = synth.make_config(3)
    x = np.asarray(x)
    lo, hi = x.min(axis=0), x.max(axis=0)
    rng = np.random.default_rng(1)
    x0 = lo + (hi - lo) * rng.random((a.n0, x.shape[1]))
    out = dict(n=cfg['n'], d=cfg['d'], p=cfg['p'], q=cfg['q'], n0=a.n0, draws=a.draws, device=torch.cuda.get_device_name(0))
    for dt in a.dtypes.split(','):
        m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0', dtype=dt)
        m.loss_and_grad(m._get_flat())
        eng = m._aux_engine
        clk = torch.zeros(2, dtype=torch.int64, device='cuda:0')
        eng.lib.lcgp_lauum_clock(eng._stream(), eng.dtype, eng.n, eng.d, eng.p, eng.q_local, eng._p(eng.workspace), eng._p(clk))
        c = clk.cpu().numpy()
        x0s, xt = m._standardise_x0(x0)[0], m._x_train()
        th = eng._theta_last.copy()
        seeds = [(0, k) for k in range(eng.q_local)]
        jit = JITTER[eng.dtype_name]
        res = dict(engine=eng.dtype_name, clock_mhz=100.0 * c[0] / c[1] if c[1] else float('nan'), jitter=jit,
                   base_cov_ms=device_ms(lambda: eng.form_cov(x0s, False, 0.0), a.reps),
                   base_sample_ms=device_ms(lambda: eng.sample_latent(x0s, a.draws, seeds, jit), a.reps))
        for k in [int(v) for v in a.ms.split(',')]:
            xn = lo + (hi - lo) * rng.random((k, x.shape[1]))
            yn = rng.standard_normal((cfg['p'], k))
            xn_s = m._standardise_x0(xn)[0]
            ys = (yn - m.ymean.numpy()) / m.ystd.numpy()
            t = (th[:, cfg['d'] + 3:] @ ys) / th[:, cfg['d'] + 2][:, None]
            state = eng.condition_begin(xn_s, t, None)
            r = dict(prepare_ms=device_ms(lambda: eng.condition_begin(xn_s, t, None), a.reps),
                     view_cov_ms=device_ms(lambda: eng._form_cov(state, x0s, False, 0.0), a.reps),
                     view_sample_ms=device_ms(lambda: eng.condition_sample_latent(state, x0s, a.draws, seeds, jit), a.reps))
            aug = HotPathEngine(np.vstack([xt, xn_s]), np.hstack([m.y.numpy(), ys]), None, q_local=eng.q_local, kernel=m.kernel,
                                dtype=dt)
            aug.evaluate(th)

            def refit_cov():
                aug.upload_theta(th)
                aug.enqueue()
                aug.form_cov(x0s, False, 0.0)

            def refit_sample():
                aug.upload_theta(th)
                aug.enqueue()
                aug.sample_latent(x0s, a.draws, seeds, jit)

            r['refit_eval_ms'] = device_ms(aug.enqueue, a.reps)
            r['refit_cov_ms'] = device_ms(refit_cov, a.reps)
            r['refit_sample_ms'] = device_ms(refit_sample, a.reps)
            r['cov_ratio_view_over_base'] = r['view_cov_ms'] / res['base_cov_ms']
            r['flop_ratio'] = flop_ratio(cfg['n'], k, a.n0)
            r['sample_ratio_view_over_base'] = r['view_sample_ms'] / res['base_sample_ms']
            r['prepare_plus_view_cov_below_refit'] = bool(r['prepare_ms'] + r['view_cov_ms'] < r['refit_cov_ms'])
            r['prepare_plus_view_sample_below_refit'] = bool(r['prepare_ms'] + r['view_sample_ms'] < r['refit_sample_ms'])
            res['m=%d' % k] = r
            del state, aug
            torch.cuda.empty_cache()
        out[dt] = res
        del m, eng
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
