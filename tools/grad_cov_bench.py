"""Timing of the posterior covariance of the gradient (LCGP.predict_grad_cov / active_subspace) at the headline shape.

Reports, in device-event windows (median of --reps after a warm-up, one process), at n = 4096, d = 6, q = 8, n0 = 2000 (fp64;
--dtype float32 for the other precision):
  - HotPathEngine.grad_cov_block per point (dghat and the packed Gamma of every new input) and reduce-only (weights given,
    the per-point tensor never written);
  - HotPathEngine.predict_hess_block beside them (the pass this one is cut from: it also forms U, V = U W and the two
    contractions over the training inputs), and the ratio grad_cov / predict_hess, which has to be below 1;
  - the end-to-end LCGP.predict_grad_cov and LCGP.active_subspace (device passes, gather and output map on the host; wall
    clock);
  - the scratch of the call.
`--only per_point|reduce|hess` times one of the three alone, for a rocprofv3 --kernel-trace --stats run of this tool; `--stats
<kernel_stats.csv>` turns that run's file into JSON fields: time per call and share of every kernel of the pass.  Prints one
JSON line."""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tools.predict_hess_bench import passes, timed_events, u_flops  # noqa: E402

KERNELS = ('pgrad_kernel', 'pdx_kernel', 'tile_gemm', 'gradcov_kernel', 'gradcov_reduce_kernel', 'cross_kernel',
           'pred_reduce_kernel', 'phess_gram_kernel', 'phess_kernel')


def from_stats(path):
    """per-kernel total, calls, average and share from rocprofv3's kernel_stats.csv"""
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r['TotalDurationNs']) for r in rows)
    out = {}
    for r in rows:
        name, tot, calls = r['Name'], float(r['TotalDurationNs']), int(r['Calls'])
        for key in KERNELS:
            if ('::' + key + '<') in name or name.startswith(key + '<') or name.startswith(key + '('):
                label = key
                if key == 'tile_gemm':
                    label = 'tile_gemm_op' + name.split('<', 1)[1].split(',')[1].strip()
                out[label] = dict(calls=calls, avg_ms=tot / calls / 1e6, share=tot / total)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n0', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', default='float64')
    ap.add_argument('--only', default=None, choices=('per_point', 'reduce', 'hess'))
    ap.add_argument('--stats', default=None, help='kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool')
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(from_stats(a.stats)))
        return 0
    from lcgp_amd import LCGP, synth
    from lcgp_amd import engine as engine_mod
    x, y, cfg = synth.make_config(3)
    m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0', dtype=a.dtype)
    m.loss_and_grad(m._get_flat())
    eng = m._aux_engine
    d = int(eng.d)
    x0s = np.random.default_rng(0).uniform(0, 1, (a.n0, d))
    w = np.full(a.n0, 1.0 / a.n0)
    runs = dict(per_point=lambda: eng.grad_cov_block(x0s), reduce=lambda: eng.grad_cov_block(x0s, w, per_point=False),
                hess=lambda: eng.predict_hess_block(x0s))
    if a.only:
        print(json.dumps({a.only + '_ms': timed_events(runs[a.only], a.reps)}))
        return 0
    t = {k: timed_events(f, a.reps) for k, f in runs.items()}
    scratch = int(eng._scratch.numel())
    x0 = x0s * (m.x_max.numpy() - m.x_min.numpy()) + m.x_min.numpy()
    t0 = time.perf_counter()
    m.predict_grad_cov(x0)
    t_api = time.perf_counter() - t0
    t0 = time.perf_counter()
    m.active_subspace(x0)
    t_as = time.perf_counter() - t0
    ps = passes(a.n0, d, engine_mod.PREDICT_CHUNK)
    out = dict(n=int(eng.n), d=d, q=int(eng.q_local), n0=a.n0, dtype=a.dtype, passes=ps,
               grad_cov_per_point_ms=t['per_point'], grad_cov_reduce_only_ms=t['reduce'], predict_hess_ms=t['hess'],
               ratio=t['per_point'] / t['hess'], ratio_reduce_only=t['reduce'] / t['hess'],
               faster_than_predict_hess=bool(t['per_point'] < t['hess']),
               p_flop=sum(u_flops(eng.n, eng.q_local, mm * d) for mm in ps), scratch_bytes_with_hess=scratch,
               predict_grad_cov_api_ms=1e3 * t_api, active_subspace_api_ms=1e3 * t_as)
    print(json.dumps(out))
    return 0 if out['faster_than_predict_hess'] else 1


if __name__ == '__main__':
    sys.exit(main())
