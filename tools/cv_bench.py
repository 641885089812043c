"""Timing of closed-form cross-validation (LCGP.predict_loo / predict_cv) at the headline shape (n = 4096, d = 6, p = 64,
q = 8), float64 and float32, next to one lcgp_nll_grad in the same process.

Per dtype, median of --reps after a warm-up, each window bracketed by device events on the current stream:
  - nll_grad: one evaluation (HotPathEngine.enqueue);
  - loo: HotPathEngine.loo_block (lcgp_loo, one launch);
  - cv: HotPathEngine.cv_block with F = --folds (lcgp_cv_gather, lcgp_potrf_logdet + lcgp_potri of the q F fold matrices,
    lcgp_cv_apply).  The window also holds the host-side checks of the folds and one synchronising read of the info words,
    so it bounds the device time from above; rocprofv3 --kernel-trace --stats gives the kernels on their own.
  - the public calls end to end (wall clock: the gather, the host output map).
Gate of the feature: cv below one nll_grad.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lcgp_amd import LCGP, synth  # noqa: E402


def device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--folds', type=int, default=10)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtypes', default='float64,float32')
    a = ap.parse_args()
    x, y, cfg = synth.make_config(3)
    out = dict(n=cfg['n'], d=cfg['d'], p=cfg['p'], q=cfg['q'], folds=a.folds)
    for dt in a.dtypes.split(','):
        m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0', dtype=dt)
        m.loss_and_grad(m._get_flat())
        eng = m._aux_engine
        _, ptr, idx = m._cv_labels(a.folds, 0)
        t_nll = device_ms(eng.enqueue, a.reps)          # (the workspace keeps the same parameters' factorisation)
        t_loo = device_ms(eng.loo_block, a.reps)
        t_cv = device_ms(lambda: eng.cv_block(ptr, idx), a.reps)
        mpad = (int(np.diff(ptr).max()) + 127) // 128 * 128
        out[dt] = dict(engine=eng.dtype_name, nll_grad_ms=t_nll, loo_ms=t_loo, cv_ms=t_cv, cv_over_nll=t_cv / t_nll,
                       cv_mpad=mpad, cv_flop=eng.q_local * a.folds * mpad ** 3 * 1.0,
                       predict_loo_wall_ms=wall_ms(m.predict_loo, a.reps),
                       predict_cv_wall_ms=wall_ms(lambda: m.predict_cv(a.folds), a.reps))
        del m, eng
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
