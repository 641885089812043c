"""Timing of the integrated variance reduction (LCGP.variance_reduction) at the headline shape (n = 4096, d = 6, p = 64,
q = 8), float64 and float32, next to one lcgp_nll_grad in the same process.

Per dtype and shape, median of --reps after a warm-up, each window bracketed by device events on the current stream:
  - nll_grad: one evaluation (HotPathEngine.enqueue);
  - vr: HotPathEngine.variance_reduction_block (lcgp_variance_reduction_prepare: U of the reference set; then per chunk of
    candidates lcgp_variance_reduction: U of the candidates unless the sets are one, the fused OP_VR launch, the reduction).
    The window also holds the host-to-device copies of the inputs, so it bounds the device time from above; rocprofv3
    --kernel-trace --stats gives the kernels on their own;
  - the public call end to end (wall clock: standardisation, the gather, the output map).
Shapes: n_ref = n_cand = --cands (x_ref = x_cand: one U serves both), and n_ref = n, n_cand = --cands.
Flops from the shapes, per component: U of a set of m points m_pad npad^2 (2 flops per multiply-add over the lower triangle
of W; m_pad: m rounded up to 128, or to 64 below 128), the fused product 2 n_ref64 n_cand64 npad (n64: rounded up to 64).
Prints one JSON line."""
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


def pad(m, b):
    return (m + b - 1) // b * b


def upad(m):
    return pad(m, 128) if m >= 128 else pad(m, 64)


def flops(q, n, n_ref, n_cand, shared):
    npad = pad(n, 128)
    u = upad(n_ref) * npad ** 2 + (0 if shared else upad(n_cand) * npad ** 2)
    fused = 2.0 * pad(n_ref, 64) * pad(n_cand, 64) * npad
    return q * u, q * fused


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cands', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtypes', default='float64,float32')
    a = ap.parse_args()
    x, y, cfg = synth.make_config(3)
    x = np.asarray(x)
    lo, hi = x.min(axis=0), x.max(axis=0)
    xc = lo + (hi - lo) * np.random.default_rng(1).random((a.cands, x.shape[1]))
    out = dict(n=cfg['n'], d=cfg['d'], p=cfg['p'], q=cfg['q'], cands=a.cands)
    for dt in a.dtypes.split(','):
        m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0', dtype=dt)
        m.loss_and_grad(m._get_flat())
        eng = m._aux_engine
        n = eng.n
        xc_s = m._standardise_x0(xc)[0]
        xr_s = m._standardise_x0(x)[0]
        t_nll = device_ms(eng.enqueue, a.reps)          # (the workspace keeps the same parameters' factorisation)
        res = dict(engine=eng.dtype_name, nll_grad_ms=t_nll)
        for name, ref, n_ref in (('shared', None, a.cands), ('ref_n', xr_s, n)):
            w = np.full(n_ref, 1.0 / n_ref)
            t = device_ms(lambda: eng.variance_reduction_block(xc_s, ref, w, None, 1), a.reps)
            fu, ff = flops(eng.q_local, n, n_ref, a.cands, ref is None)
            res[name] = dict(n_ref=n_ref, vr_ms=t, vr_over_nll=t / t_nll, flop_u=fu, flop_fused=ff,
                             tflops=(fu + ff) / (t * 1e-3) / 1e12,
                             wall_ms=wall_ms(lambda: m.variance_reduction(xc, x_ref=None if ref is None else x), a.reps))
        out[dt] = res
        del m, eng
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
