"""Timing of the expected Sobol variances and the exact integrated variance (LCGP.sobol_indices(uncertainty=True),
LCGP.integrated_variance) at the headline shape, beside the calls they extend.

At n = 4096, d = 6, p = 64, q = 8 in fp64 (synth.make_config(3)) one process times, by the wall clock around calls that end in a
device-to-host copy (median, minimum and maximum over --reps calls after one warm-up call):
  - LCGP.sobol_indices() against LCGP.sobol_indices(uncertainty=True): the 36 pairs of the mean surface, then the 8 pairs k = k'
    once more, weighted by A^-1 in place;
  - LCGP.integrated_variance() (the matrix-weighted pass alone) against LCGP.sobol_indices(latent=True), the vector-weighted
    pass over the same 8 pairs;
  - HotPathEngine.sobol_matrix_sums on the 8 components (three launches: the table, the 64 x 64 pair tiles, the reduction).
Prints one JSON line.  Nothing is gated: the figures are recorded in profiles/sobol_uncertainty_bench.txt."""
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
    ap.add_argument('--only', default=None, choices=('matrix',), help='the engine pass alone, for a kernel trace of this tool')
    a = ap.parse_args()
    from lcgp_amd import LCGP, synth
    x, y, cfg = synth.make_config(3)
    m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0')
    m.loss_and_grad(m._get_flat())
    eng = m._ensure_aux64()
    n, d, q = int(eng.n), int(eng.d), int(m.q)
    scale, nug = m.lLmb0.numpy(), m.lnugGPs.numpy()
    v = (scale * (1.0 - nug / (1.0 + nug)) * np.sqrt(m.diag_D.numpy().reshape(-1)))[:, None] * np.ones((1, n))
    box = np.stack([np.zeros(d), np.ones(d)])
    xs = np.asarray(m._x_train(), np.float64)
    out = dict(n=n, d=d, p=int(m.p), q=q, reps=a.reps)
    out['sobol_matrix_sums_ms'] = timed(lambda: eng.sobol_matrix_sums(xs, v, m.lLmb.numpy(), box, np.arange(q)), a.reps)
    if a.only:
        print(json.dumps(out))
        return 0
    out['sobol_indices_ms'] = timed(lambda: m.sobol_indices(), a.reps)
    out['sobol_indices_uncertainty_ms'] = timed(lambda: m.sobol_indices(uncertainty=True), a.reps)
    out['sobol_indices_latent_ms'] = timed(lambda: m.sobol_indices(latent=True), a.reps)
    out['integrated_variance_ms'] = timed(lambda: m.integrated_variance(), a.reps)
    s = m.sobol_indices(uncertainty=True)
    out['expected_over_plug_in_variance_range'] = [float((s.expected_variance / s.variance).min()),
                                                   float((s.expected_variance / s.variance).max())]
    out['integrated_variance_range'] = [float(s.integrated_variance.min()), float(s.integrated_variance.max())]
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
