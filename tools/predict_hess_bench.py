"""Timing of the input Hessians of the prediction (LCGP.predict_hess) at the headline shape.

Reports, in device-event windows (median of --reps after a warm-up), at n = 4096, d = 6, q = 8, n0 = 2000 (fp64; --dtype
float32 for the other precision):
  - HotPathEngine.predict_grad_block (lcgp_predict_grad) and predict_hess_block (lcgp_predict_hess: the same launches, then
    the rows d_l X, P = dX W^T, the Gram terms and the fused contraction), their ratio, and the only other route to a
    Hessian, 2 d predict_grad_block calls (central differences);
  - the gate of the feature: predict_hess_block < 2 d x predict_grad_block (exit status 1 otherwise);
  - the end-to-end LCGP.predict_hess (device passes, gather, unpacking and output map on the host; wall clock);
  - the scratch of the call.
Flop count of the P product from the shapes, per pass of `chunk` new inputs (rpad = chunk d rounded up to 128, nb = npad / 128
tile columns of W):   q * (rpad / 128) * nb (nb + 1) / 2 * 128^3 * 2   (2 flops per multiply-add; the k tiles up to the diagonal).
The per-launch times of the new kernels come from a rocprofv3 --kernel-trace --stats run of this tool; `--stats
<kernel_stats.csv>` turns that file into JSON fields: the share of pdx_kernel, phess_gram_kernel and phess_kernel in the run
and the rate of the U-type products (tile_gemm<..., 5, ...>: U of lcgp_predict and P, which share a kernel name; P is d / (d +
1) of their flops).  Prints one JSON line."""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

FP64_PEAK = 78.6e12


def pad128(r):
    return (r + 127) // 128 * 128 if r >= 128 else (r + 63) // 64 * 64


def passes(n0, d, predict_chunk):
    """sizes of the passes of HotPathEngine.predict_hess_block"""
    chunk = min(n0, max(128, predict_chunk // d))
    out = []
    for lo in range(0, n0, chunk):
        m = min(chunk, n0 - lo)
        out.append(128 if m < 128 <= n0 else m)
    return out


def u_flops(n, q, rows):
    npad = (n + 127) // 128 * 128
    nb = npad // 128
    return q * (pad128(rows) // 128) * nb * (nb + 1) / 2 * 128.0 ** 3 * 2


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


def from_stats(path, n, d, q, n0, predict_chunk):
    """shares of the new kernels and the rate of the U-type products from rocprofv3's kernel_stats.csv"""
    out, total = {}, 0.0
    rows = list(csv.DictReader(open(path)))
    for row in rows:
        total += float(row['TotalDurationNs'])
    for row in rows:
        name, tot, calls = row['Name'], float(row['TotalDurationNs']), int(row['Calls'])
        for key in ('pdx_kernel', 'phess_gram_kernel', 'phess_kernel', 'pgrad_kernel'):
            if ('::' + key + '<') in name or name.startswith(key + '<'):
                out[key + '_share'] = tot / total
                out[key + '_avg_ms'] = tot / calls / 1e6
        if 'tile_gemm' in name and ', 5, ' in name:
            ps = passes(n0, d, predict_chunk)
            per_call = sum(u_flops(n, q, m) + u_flops(n, q, m * d) for m in ps)      # U of X and P, per predict_hess_block
            out['u_products_share'] = tot / total
            out['u_products_avg_ms'] = tot / calls / 1e6
            # (calls per predict_hess_block: 2 per pass; predict_grad_block's own U launches are in the same row when the
            # traced run also times it, so the rate is taken per launch from the flops of an average launch)
            out['u_products_tflops_if_only_hess_ran'] = per_call / (2 * len(ps)) / (tot / calls * 1e-9) / 1e12
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n0', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', default='float64')
    ap.add_argument('--only-hess', action='store_true', help='time predict_hess_block alone (for a rocprofv3 trace)')
    ap.add_argument('--stats', default=None, help='kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool')
    a = ap.parse_args()
    from lcgp_amd import synth
    from lcgp_amd import engine as engine_mod
    _, _, cfg = synth.make_config(3)
    if a.stats:
        print(json.dumps(dict(n=cfg['n'], q=cfg['q'], n0=a.n0,
                              **from_stats(a.stats, cfg['n'], cfg['d'], cfg['q'], a.n0, engine_mod.PREDICT_CHUNK))))
        return 0
    from lcgp_amd import LCGP
    x, y, cfg = synth.make_config(3)
    m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0', dtype=a.dtype)
    m.loss_and_grad(m._get_flat())
    eng = m._aux_engine
    d = int(eng.d)
    x0s = np.random.default_rng(0).uniform(0, 1, (a.n0, d))
    t_hess = timed_events(lambda: eng.predict_hess_block(x0s), a.reps)
    if a.only_hess:
        print(json.dumps(dict(predict_hess_ms=t_hess)))
        return 0
    t_grad = timed_events(lambda: eng.predict_grad_block(x0s), a.reps)
    x0 = x0s * (m.x_max.numpy() - m.x_min.numpy()) + m.x_min.numpy()
    t0 = time.perf_counter()
    m.predict_hess(x0)
    t_api = time.perf_counter() - t0
    ps = passes(a.n0, d, engine_mod.PREDICT_CHUNK)
    p_flop = sum(u_flops(eng.n, eng.q_local, mm * d) for mm in ps)
    out = dict(n=int(eng.n), d=d, q=int(eng.q_local), n0=a.n0, dtype=a.dtype, passes=ps,
               predict_grad_ms=t_grad, predict_hess_ms=t_hess, ratio=t_hess / t_grad,
               central_differences_ms=2 * d * t_grad, gate_ok=bool(t_hess < 2 * d * t_grad),
               p_flop=p_flop, scratch_bytes=int(eng._scratch.numel()), predict_hess_api_ms=1e3 * t_api)
    print(json.dumps(out))
    return 0 if out['gate_ok'] else 1


if __name__ == '__main__':
    sys.exit(main())
