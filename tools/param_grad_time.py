"""Timing of the parameter derivatives of the prediction (LCGP.predict_param_grad) at the headline shape.

Reports, in device-event windows (median of --reps after a warm-up), at n = 4096, d = 6, p = 64, q = 8, n0 = 2000, float64, one
process:
  - HotPathEngine.predict_paramgrad_block (lcgp_predict_paramgrad: the whole latent pass);
  - what it replaces: central differences of predict() over the P parameters, 2 P passes, each one evaluation of the objective
    (the refactorisation at the shifted parameters) followed by predict_block; one such pass is timed (median) and multiplied by
    2 P;
  - the ratio of the two, the gate of the feature: the pass must be faster (exit status 1 otherwise);
  - the flops of the d products T_j = V d_jA from the shapes, 2 d q n0pad npad^2, and the time they take at the rate the tile
    kernel holds on dense products (70 TFLOP/s) as a share of the pass;
  - the end-to-end LCGP.predict_param_grad (device pass, gather and the host map; wall clock);
  - the scratch of the call and the clock the chip held in the evaluation's A^-1 launch (lcgp_lauum_clock), as bench.py reports it.
The per-launch times come from a rocprofv3 --kernel-trace --stats run of this tool with --only-pass; `--stats
<kernel_stats.csv>` turns that file into the measured share of the products (tile_gemm<..., 11, ...>) and of the new kernels.
Prints one JSON line."""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

DENSE_RATE = 70e12


def timed_events(fn, reps):
    """median over reps of the device time of fn() between two events on the current stream (ms)"""
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def from_stats(path):
    """shares of the dense products and of the new kernels from rocprofv3's kernel_stats.csv"""
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r['TotalDurationNs']) for r in rows)
    out = {}
    for r in rows:
        name, tot, calls = r['Name'], float(r['TotalDurationNs']), int(r['Calls'])
        key = None
        if 'tile_gemm' in name and ', 11, ' in name:
            key = 'dense_products'
        for k in ('pgrad_row_kernel', 'pgrad_rowdot_kernel', 'hess_da_kernel', 'hess_matvec_kernel'):
            if k in name:
                key = k
        if key:
            out[key + '_share'] = out.get(key + '_share', 0.0) + tot / total
            out[key + '_avg_ms'] = tot / calls / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n0', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--only-pass', action='store_true', help='time predict_paramgrad_block alone (for a rocprofv3 trace)')
    ap.add_argument('--stats', default=None, help='kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool')
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(from_stats(a.stats)))
        return 0
    import torch
    from lcgp_amd import LCGP, synth
    x, y, cfg = synth.make_config(3)
    m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0', dtype='float64')
    u = m._get_flat().copy()
    m.loss_and_grad(u)
    eng = m._aux_engine
    d, q, p, n = int(eng.d), int(eng.q_local), int(eng.p), int(eng.n)
    x0s = np.random.default_rng(0).uniform(0, 1, (a.n0, d))
    t_pass = timed_events(lambda: eng.predict_paramgrad_block(x0s), a.reps)
    if a.only_pass:
        print(json.dumps(dict(predict_paramgrad_ms=t_pass)))
        return 0
    rows = eng._theta_last.copy()

    def one_difference_pass():
        eng.upload_theta(rows)
        eng.enqueue()
        eng.predict_block(x0s)

    t_one = timed_events(one_difference_pass, a.reps)
    clk = torch.zeros(2, dtype=torch.int64, device=eng.device)
    eng.lib.lcgp_lauum_clock(eng._stream(), eng.dtype, n, d, p, q, eng._p(eng.workspace), eng._p(clk))
    cyc, ticks = (int(v) for v in clk.cpu().numpy())
    P = u.size
    x0 = x0s * (m.x_max.numpy() - m.x_min.numpy()) + m.x_min.numpy()
    m.predict_param_grad(x0[:8])
    t0 = time.perf_counter()
    m.predict_param_grad(x0)
    t_api = time.perf_counter() - t0
    npad, n0pad = (n + 127) // 128 * 128, (a.n0 + 127) // 128 * 128
    flop = 2.0 * d * q * n0pad * npad * npad
    out = dict(n=n, d=d, p=p, q=q, n0=a.n0, P=int(P), predict_paramgrad_ms=t_pass, one_difference_pass_ms=t_one,
               central_differences_ms=2 * P * t_one, ratio=2 * P * t_one / t_pass, gate_ok=bool(t_pass < 2 * P * t_one),
               products_flop=flop, products_ms_at_70_tflops=1e3 * flop / DENSE_RATE, products_share_at_70_tflops=1e3 * flop / DENSE_RATE / t_pass,
               clock_mhz=(100.0 * cyc / ticks if ticks else None), scratch_bytes=int(eng._scratch.numel()),
               predict_param_grad_api_ms=1e3 * t_api)
    print(json.dumps(out))
    return 0 if out['gate_ok'] else 1


if __name__ == '__main__':
    sys.exit(main())
