"""Timing of the closed-form Sobol indices (LCGP.sobol_indices) at the headline shape, beside what they replace.

At n = 4096, d = 6, p = 64, q = 8 in fp64 (synth.make_config(3); 36 pairs of components) one process times, by the wall clock
around calls that end in a device-to-host copy (median, minimum and maximum over --reps calls after one warm-up call):
  - HotPathEngine.sobol_pairs on all 36 pairs (three launches: the table, the 64 x 64 pair tiles, the reduction);
  - LCGP.sobol_indices end to end (the gather of the weight vectors, the pass, the output map on the host);
  - LCGP.sobol_indices(latent=True): the 8 pairs k = k' alone;
  - for context LCGP.predict on --saltelli (d + 2) rows, the design of a Saltelli estimator of --saltelli base points (its
    estimates themselves are not formed).
Prints one JSON line.  Nothing is gated: the figures are recorded in profiles/sobol_bench.txt."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def timed(fn, reps):
    """[median, min, max] in ms of reps calls of fn after one warm-up call"""
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--saltelli', type=int, default=10000)
    ap.add_argument('--only', default=None, choices=('pairs',), help='the engine pass alone, for a kernel trace of this tool')
    a = ap.parse_args()
    from lcgp_amd import LCGP, synth
    x, y, cfg = synth.make_config(3)
    m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0')
    m.loss_and_grad(m._get_flat())
    eng = m._ensure_aux64()
    n, d, q = int(eng.n), int(eng.d), int(m.q)
    z = np.stack([eng.fetch_vector(1, k) for k in range(q)])
    scale, nug = m.lLmb0.numpy(), m.lnugGPs.numpy()
    w = (scale * (1.0 - nug / (1.0 + nug)))[:, None] * z
    pairs = np.array([(k, kp) for k in range(q) for kp in range(k, q)])
    box = np.stack([np.zeros(d), np.ones(d)])
    xs = np.asarray(m._x_train(), np.float64)
    out = dict(n=n, d=d, p=int(m.p), q=q, pairs=len(pairs), reps=a.reps)
    out['sobol_pairs_ms'] = timed(lambda: eng.sobol_pairs(xs, w, m.lLmb.numpy(), box, pairs), a.reps)
    if a.only:
        print(json.dumps(out))
        return 0
    out['sobol_indices_ms'] = timed(lambda: m.sobol_indices(), a.reps)
    out['sobol_indices_latent_ms'] = timed(lambda: m.sobol_indices(latent=True), a.reps)
    rows = a.saltelli * (d + 2)
    x0 = np.random.default_rng(0).uniform(0, 1, (rows, d)) * (m.x_max.numpy() - m.x_min.numpy()) + m.x_min.numpy()
    out['saltelli_rows'] = rows
    out['predict_ms'] = timed(lambda: m.predict(x0), max(1, a.reps // 2))
    s = m.sobol_indices()
    out['first_sum_range'] = [float(s.first.numpy().sum(axis=1).min()), float(s.first.numpy().sum(axis=1).max())]
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
