"""Timing of the box-averaged predictions (LCGP.predict_marginal / main_effects) at the headline shape.

Reports, in device-event windows (one process, the two passes ALTERNATING --rounds times, --reps calls each; medians over all
windows of a pass), at n = 4096, d = 6, q = 8 and 2000 rows (fp64; --dtype float32 for the other precision):
  - HotPathEngine.predict_marginal_block on rows that keep one dimension and integrate the others (the rows of main_effects),
    on the default box;
  - HotPathEngine.predict_block on the same number of rows (the pass this one is made of), and the ratio marginal / predict,
    which the flop counts put within 1.10;
  - the end-to-end LCGP.predict_marginal and LCGP.main_effects (device pass, gather and output map on the host; wall clock).
`--only marginal|predict` times one of the two alone, for a rocprofv3 --kernel-trace --stats run of this tool; `--stats
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

from tools.predict_hess_bench import timed_events  # noqa: E402

KERNELS = ('marg_table_kernel', 'cross_kernel', 'tile_gemm', 'marg_reduce_kernel', 'pred_reduce_kernel')


def from_stats(path):
    """per-kernel calls, average and share from rocprofv3's kernel_stats.csv (cross_kernel: the row kernel)"""
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
                if key == 'cross_kernel' and 'unsigned char' in name:
                    label = 'cross_kernel_marginal'
                out[label] = dict(calls=calls, avg_ms=tot / calls / 1e6, share=tot / total)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n0', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--dtype', default='float64')
    ap.add_argument('--only', default=None, choices=('marginal', 'predict'))
    ap.add_argument('--stats', default=None, help='kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool')
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(from_stats(a.stats)))
        return 0
    from lcgp_amd import LCGP, synth
    x, y, cfg = synth.make_config(3)
    m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0', dtype=a.dtype)
    m.loss_and_grad(m._get_flat())
    eng = m._aux_engine
    d = int(eng.d)
    x0s = np.random.default_rng(0).uniform(0, 1, (a.n0, d))
    mask = np.ones((a.n0, d), bool)
    mask[np.arange(a.n0), np.arange(a.n0) % d] = False           # row i keeps dimension i mod d
    box = np.stack([np.zeros(d), np.ones(d)])
    runs = dict(marginal=lambda: eng.predict_marginal_block(x0s, mask, box), predict=lambda: eng.predict_block(x0s))
    if a.only:
        print(json.dumps({a.only + '_ms': timed_events(runs[a.only], a.reps)}))
        return 0
    ts = dict(marginal=[], predict=[])
    for _ in range(a.rounds):
        for k in ('marginal', 'predict'):
            ts[k].append(timed_events(runs[k], a.reps))
    t = {k: float(np.median(v)) for k, v in ts.items()}
    x0 = x0s * (m.x_max.numpy() - m.x_min.numpy()) + m.x_min.numpy()
    t0 = time.perf_counter()
    m.predict_marginal(x0, mask)
    t_api = time.perf_counter() - t0
    G = (a.n0 - 1) // d
    t0 = time.perf_counter()
    m.main_effects(grid=G)
    t_me = time.perf_counter() - t0
    out = dict(n=int(eng.n), d=d, q=int(eng.q_local), n0=a.n0, dtype=a.dtype, predict_marginal_ms=t['marginal'],
               predict_ms=t['predict'], ratio=t['marginal'] / t['predict'], rounds_marginal_ms=ts['marginal'],
               rounds_predict_ms=ts['predict'], within_1p10=bool(t['marginal'] <= 1.10 * t['predict']),
               predict_marginal_api_ms=1e3 * t_api, main_effects_grid=G, main_effects_api_ms=1e3 * t_me)
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
