"""Timing of the subset pass (LCGP.sobol_indices(order=2), LCGP.shapley_effects) at the headline shape, beside
the pass it extends.

At n = 4096, d = 6, p = 64, q = 8 in fp64 (synth.make_config(3); 36 pairs of components) one process times, by the wall clock
around calls that end in a device-to-host copy (median, minimum and maximum over --reps calls after one warm-up call):
  - LCGP.sobol_indices(): the pass of 4.22 (what tools/sobol_bench.py times, for a run of the parent revision on the same box);
  - LCGP.sobol_indices(order=2): that pass and one subset pass over the d (d - 1) / 2 = 15 pair masks (one chunk);
  - HotPathEngine.sobol_subset_pairs on all 36 pairs for one chunk of masks and for two chunks;
  - LCGP.shapley_effects(): all 2^d = 64 masks (two chunks) over the 36 pairs;
  - LCGP.sobol_indices(uncertainty=True) and LCGP.shapley_effects(uncertainty=True): with the matrix-weighted passes over the 8
    pairs k = k'.
Prints one JSON line.  Nothing is gated: the figures are recorded in profiles/sobol_subset_bench.txt."""
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
    a = ap.parse_args()
    from lcgp_amd import LCGP, _hip, synth
    x, y, cfg = synth.make_config(3)
    m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0')
    m.loss_and_grad(m._get_flat())
    eng = m._ensure_aux64()
    n, d, q = int(eng.n), int(eng.d), int(m.q)
    chunk = _hip.load().lcgp_sobol_subset_chunk(d)
    z = np.stack([eng.fetch_vector(1, k) for k in range(q)])
    scale, nug = m.lLmb0.numpy(), m.lnugGPs.numpy()
    w = (scale * (1.0 - nug / (1.0 + nug)))[:, None] * z
    pairs = np.array([(k, kp) for k in range(q) for kp in range(k, q)])
    box = np.stack([np.zeros(d), np.ones(d)])
    xs = np.asarray(m._x_train(), np.float64)
    ell = m.lLmb.numpy()
    out = dict(n=n, d=d, p=int(m.p), q=q, pairs=len(pairs), reps=a.reps, chunk=chunk)
    out['sobol_indices_ms'] = timed(lambda: m.sobol_indices(), a.reps)
    out['sobol_pairs_ms'] = timed(lambda: eng.sobol_pairs(xs, w, ell, box, pairs), a.reps)
    for name, nsub in (('one_mask', 1), ('one_chunk', chunk), ('two_chunks', 2 * chunk)):
        masks = np.arange(nsub, dtype=np.uint64) % np.uint64(1 << d)
        out['sobol_subset_pairs_%s_ms' % name] = timed(lambda: eng.sobol_subset_pairs(xs, w, ell, box, pairs, masks), a.reps)
    out['sobol_indices_order2_ms'] = timed(lambda: m.sobol_indices(order=2), a.reps)
    out['shapley_effects_ms'] = timed(lambda: m.shapley_effects(), a.reps)
    out['sobol_indices_uncertainty_ms'] = timed(lambda: m.sobol_indices(uncertainty=True), a.reps)
    out['shapley_effects_uncertainty_ms'] = timed(lambda: m.shapley_effects(uncertainty=True), a.reps)
    s, sh = m.sobol_indices(order=2), m.shapley_effects()
    sv = s.second.numpy()
    iu = np.triu_indices(d, 1)
    out['second_sum_range'] = [float(sv[:, iu[0], iu[1]].sum(axis=1).min()), float(sv[:, iu[0], iu[1]].sum(axis=1).max())]
    out['shapley_sum_minus_variance'] = float(np.max(np.abs(sh.effects.numpy().sum(axis=1) - sh.variance.numpy()) / sh.variance.numpy()))
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
