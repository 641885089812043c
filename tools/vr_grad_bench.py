"""Timing of the gradient of the integrated variance reduction (LCGP.variance_reduction_grad) at the headline shape
(n = 4096, d = 6, p = 64, q = 8; n_ref = n_cand = --cands, an explicit reference set), float64 and float32.

Per dtype, median of --reps after a warm-up, each window bracketed by device events on the current stream, all in ONE process:
  - vr_grad: one HotPathEngine.variance_reduction_grad_block (value and gradient);
  - vr: one HotPathEngine.variance_reduction_block (the value alone);
  - central: the route to the same information without the analytic gradient: 2 d calls of variance_reduction_block (one per
    shifted copy of the candidates; the differences themselves are not timed).
The windows also hold the host-to-device copies of the inputs, so they bound the device time from above; rocprofv3
--kernel-trace --stats gives the kernels on their own.
Flops of the new products from the shapes, per component (2 per multiply-add; m128: rounded up to 128): P = U_cand U_ref^T and
G = S U_ref 2 n_cand128 n_ref128 npad each; Q = G W and V = U_cand W n_cand128 npad^2 each (W lower triangular).
Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lcgp_amd import LCGP, synth  # noqa: E402
from tools.vr_bench import device_ms, pad  # noqa: E402


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
    xr = lo + (hi - lo) * np.random.default_rng(2).random((a.cands, x.shape[1]))
    out = dict(n=cfg['n'], d=cfg['d'], p=cfg['p'], q=cfg['q'], cands=a.cands, n_ref=a.cands)
    for dt in a.dtypes.split(','):
        m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0', dtype=dt)
        m.loss_and_grad(m._get_flat())
        eng = m._aux_engine
        n, d = eng.n, eng.d
        xc_s, xr_s = m._standardise_x0(xc)[0], m._standardise_x0(xr)[0]
        w = np.full(a.cands, 1.0 / a.cands)
        shifted = []
        for l in range(d):
            for sgn in (1.0, -1.0):
                xs = xc_s.copy()
                xs[:, l] += sgn * 1e-4
                shifted.append(xs)
        t_grad = device_ms(lambda: eng.variance_reduction_grad_block(xc_s, xr_s, w, 1), a.reps)
        t_vr = device_ms(lambda: eng.variance_reduction_block(xc_s, xr_s, w, None, 1), a.reps)
        t_cd = device_ms(lambda: [eng.variance_reduction_block(xs, xr_s, w, None, 1) for xs in shifted], a.reps)
        npad, c128, r128 = pad(n, 128), pad(a.cands, 128), pad(a.cands, 128)
        out[dt] = dict(engine=eng.dtype_name, vr_grad_ms=t_grad, vr_ms=t_vr, central_2d_calls_ms=t_cd,
                       grad_over_vr=t_grad / t_vr, grad_over_central=t_grad / t_cd,
                       flop_P=eng.q_local * 2.0 * c128 * r128 * npad, flop_G=eng.q_local * 2.0 * c128 * r128 * npad,
                       flop_Q=eng.q_local * 1.0 * c128 * npad ** 2, flop_V=eng.q_local * 1.0 * c128 * npad ** 2)
        del m, eng
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
