"""Timing of the input gradients of the prediction (LCGP.predict_grad) at the headline shape.

Reports, with device synchronisation around each timed window (median of --reps after a warm-up), at n = 4096, d = 6, q = 8,
n0 = 2000 (fp64; --dtype float32 for the other precision):
  - HotPathEngine.predict_block (lcgp_predict) and predict_grad_block (lcgp_predict_grad, the same launches plus V = U W and
    the contraction) and their ratio;
  - the end-to-end LCGP.predict_grad (device pass, gather, output map on the host).
Flop count of the V product from the shapes (n0pad = n0 rounded up to 128, nb = npad / 128 tile columns of W):
  q * (n0pad / 128) * nb (nb + 1) / 2 * 128^3 * 2   (2 flops per multiply-add; the k tiles from the diagonal of W down).
The per-launch times of the V product (tile_gemm<..., 7, 128, 8>) and of the contraction (pgrad_kernel) come from a
rocprofv3 --kernel-trace --stats run of this tool; `--stats <kernel_stats.csv>` turns that file into the same JSON fields.
Prints one JSON line."""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

FP64_PEAK = 78.6e12


def v_flops(n, q, n0):
    npad, n0pad = (n + 127) // 128 * 128, (n0 + 127) // 128 * 128
    nb = npad // 128
    return q * (n0pad // 128) * nb * (nb + 1) / 2 * 128.0 ** 3 * 2


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def from_stats(path, n, q, n0):
    """the V launch and the contraction kernel from rocprofv3's kernel_stats.csv (average duration per launch, ns)"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name, avg = row['Name'], float(row['AverageNs'])
            if 'tile_gemm' in name and ', 7, ' in name:
                out['v_launch'] = name
                out['v_ms'] = avg / 1e6
                out['v_tflops'] = v_flops(n, q, n0) / (avg * 1e-9) / 1e12
                out['v_frac_fp64_peak'] = v_flops(n, q, n0) / (avg * 1e-9) / FP64_PEAK
            elif 'pgrad_kernel' in name:
                out['contraction_launch'] = name
                out['contraction_ms'] = avg / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n0', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', default='float64')
    ap.add_argument('--stats', default=None, help='kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool')
    a = ap.parse_args()
    from lcgp_amd import synth
    _, _, cfg = synth.make_config(3)
    if a.stats:
        print(json.dumps(dict(n=cfg['n'], q=cfg['q'], n0=a.n0, **from_stats(a.stats, cfg['n'], cfg['q'], a.n0))))
        return
    from lcgp_amd import LCGP
    x, y, cfg = synth.make_config(3)
    m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0', dtype=a.dtype)
    m.loss_and_grad(m._get_flat())
    eng = m._aux_engine
    rng = np.random.default_rng(0)
    x0s = rng.uniform(0, 1, (a.n0, cfg['d']))
    t_pred = timed(lambda: eng.predict_block(x0s, False), a.reps)
    t_grad = timed(lambda: eng.predict_grad_block(x0s), a.reps)
    x0 = x0s * (m.x_max.numpy() - m.x_min.numpy()) + m.x_min.numpy()
    t_api = timed(lambda: m.predict_grad(x0), max(3, a.reps // 3))
    out = dict(n=int(eng.n), d=int(eng.d), q=int(eng.q_local), n0=a.n0, dtype=a.dtype,
               predict_ms=1e3 * t_pred, predict_grad_ms=1e3 * t_grad, ratio=t_grad / t_pred,
               grad_extra_ms=1e3 * (t_grad - t_pred), v_flop=v_flops(eng.n, eng.q_local, a.n0),
               predict_grad_api_ms=1e3 * t_api)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
