"""Timing of the calibration target's Hessian (CalibrationTarget.loglik_hess, lcgp_calib_hess_rows) at the headline shape
(n = 4096, d = 6, p = 64, q = 8, fp64) and at one q = 16 model of the same data shape, for n0 = 64 and n0 = 2000 rows of theta.

Four things, alternated in ONE process (each window: a number of calls between two device synchronisations, sized so that a
window lasts a few tenths of a second; median of --reps windows after a warm-up of every shape), per call:
  a. HotPathEngine.predict_hess_block alone: the latent pass the Hessian rests on, the yardstick;
  b. CalibrationTarget.loglik_hess end to end (the same device pass, the two row launches, the copies to the host, the mirror);
  c. the row entry alone (lcgp_calib_hess_rows on the device blocks, d2ll only: two launches), and lcgp_calib_rows alone on the
     same blocks for the cost of the second launch;
  d. the 2 d loglik_grad calls of the central differences the Hessian replaces (their difference quotient is not timed).
Nothing is gated: the tool records what the machine gives.  Before timing, d2ll is compared with the central differences of (d)
on the rows that are clear of Matern-3/2's kinks.  Prints text; profiles/calib_hess_bench.txt is its output."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def window(fn, inner):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--window', type=float, default=0.3, help='seconds a timed window should last')
    a = ap.parse_args()
    import torch
    from lcgp_amd import LCGP, synth
    from lcgp_amd.engine import calib_hess_rows_device, calib_rows_device
    _, _, cfg = synth.make_config(3)
    d = cfg['d']
    print('# calib_hess_bench: n = %d, d = %d, p = %d, fp64; per call, median of %d windows of about %.1f s, alternated in one '
          'process' % (cfg['n'], d, cfg['p'], a.reps, a.window))
    for q in (cfg['q'], 16):
        x, y = synth.make_full(3, cfg['n'], d, cfg['p'], q)
        m = LCGP(y=y, x=x, q=q, device='cuda:0')
        m.loss_and_grad(m._get_flat())
        eng = m._aux_engine
        rng = np.random.default_rng(0)
        sd = y.std(axis=1)
        tgt = m.calibration(y[:, 100] + 0.1 * sd * rng.standard_normal(cfg['p']), (0.1 * sd) ** 2)
        h = 1e-5 * (x.max(0) - x.min(0))
        for n0 in (64, 2000):
            theta = rng.uniform(0, 1, (n0, d))
            x0s = m._x0_2d(theta, 'theta')
            blk, jac, hess = eng.predict_hess_block(x0s)
            M, b, inv_range = tgt._device_consts(blk.device)
            steps = [theta + sgn * h[c] * np.eye(d)[c] for c in range(d) for sgn in (1.0, -1.0)]

            def central():
                return [tgt.loglik_grad(t)[1] for t in steps]
            fns = {
                'a predict_hess_block': lambda: eng.predict_hess_block(x0s),
                'b loglik_hess': lambda: tgt.loglik_hess(theta),
                'c hess_rows (2 launches)': lambda: calib_hess_rows_device(blk, jac, hess, M, b, tgt.c0, tgt.lognorm, inv_range),
                'c calib_rows (1 launch)': lambda: calib_rows_device(blk, jac, M, b, tgt.c0, tgt.lognorm, inv_range),
                'd 2d x loglik_grad': central,
            }
            d2ll = tgt.loglik_hess(theta)[2].numpy()
            g = [t.numpy() for t in central()]
            fd = np.stack([(g[2 * c] - g[2 * c + 1]) / (2 * h[c]) for c in range(d)], axis=-1)
            clear = np.flatnonzero(np.min(np.abs(theta[:, None, :] - x[None, :, :]) / h, axis=(1, 2)) >= 2.0)
            diff = np.max(np.abs(d2ll[clear] - fd[clear])) / np.max(np.abs(fd[clear])) if len(clear) else float('nan')
            inner = {}
            for k, fn in fns.items():                                 # warm-up of every shape, and the window's size
                window(fn, 2)
                inner[k] = max(2, int(round(a.window / window(fn, 3))))
            ts = {k: [] for k in fns}
            for _ in range(a.reps):
                for k, fn in fns.items():
                    ts[k].append(window(fn, inner[k]))
            med = {k: float(np.median(v)) for k, v in ts.items()}
            print('q = %2d  n0 = %4d' % (q, n0))
            for k in fns:
                print('    %-26s %10.1f us   (min %.1f, max %.1f; %d calls per window)'
                      % (k, 1e6 * med[k], 1e6 * min(ts[k]), 1e6 * max(ts[k]), inner[k]))
            print('    b over a: +%.1f us (x%.3f);  d over b: x%.2f;  second row launch: %.1f us'
                  % (1e6 * (med['b loglik_hess'] - med['a predict_hess_block']), med['b loglik_hess'] / med['a predict_hess_block'],
                     med['d 2d x loglik_grad'] / med['b loglik_hess'],
                     1e6 * (med['c hess_rows (2 launches)'] - med['c calib_rows (1 launch)'])))
            print('    d2ll against the central differences of (d) on the %d kink-clear rows: %.1e of the largest entry'
                  % (len(clear), diff))
        del m, eng, tgt
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
