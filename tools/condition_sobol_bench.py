"""Timing of the Sobol queries on a conditioned view (ConditionedLCGP.integrated_variance / sobol_indices) at the
headline shape, beside the model's own calls and beside the route without these queries.

At n = 4096, d = 6, p = 64, q = 8 in fp64 (synth.make_config(3)) and m = 32 / 256 / 1024 new runs one process times, by the wall
clock around calls that end in a device-to-host copy ([median, min, max] over --reps calls after one warm-up call):
  - the model's integrated_variance(), sobol_indices(), sobol_indices(uncertainty=True);
  - per m the view's three calls and HotPathEngine.condition_sobol_matrix_sums on the 8 components (per component: E = P P^T
    on the tile kernel, then one pair pass over the (n + m)^2 plane), with the pair-count ratio ((n + m) / n)^2 they are
    expected to cost over the model's calls;
  - per m the route without the view's queries: a HotPathEngine on the n + m points (construction), one evaluation, its
    sobol_matrix_sums (what integrated_variance needs) and its sobol_pairs on the 36 pairs (what sobol_indices needs).
--only view-matrix runs the view's engine pass alone at one m (--ms), for a kernel trace of this tool.
Prints one JSON line.  Nothing is gated: the figures are recorded in profiles/condition_sobol_bench.txt."""
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
    ap.add_argument('--ms', default='32,256,1024')
    ap.add_argument('--only', default=None, choices=('view-matrix',))
    a = ap.parse_args()
    import torch
    from lcgp_amd import LCGP, synth
    from lcgp_amd.engine import HotPathEngine
    x, y, cfg = synth.make_config(3)
    x = np.asarray(x)
    m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0')
    m.loss_and_grad(m._get_flat())
    eng = m._ensure_aux64()
    n, d, q = int(eng.n), int(eng.d), int(m.q)
    th = eng._theta_last.copy()
    scale, nug = m.lLmb0.numpy(), m.lnugGPs.numpy()
    c = scale * (1.0 - nug / (1.0 + nug))
    D = m.diag_D.numpy().reshape(-1).astype(np.float64)
    ell = m.lLmb.numpy()
    box = np.stack([np.zeros(d), np.ones(d)])
    lo, hi = x.min(axis=0), x.max(axis=0)
    rng = np.random.default_rng(1)
    out = dict(n=n, d=d, p=int(m.p), q=q, reps=a.reps)
    if not a.only:
        out['model'] = dict(integrated_variance_ms=timed(lambda: m.integrated_variance(), a.reps),
                            sobol_indices_ms=timed(lambda: m.sobol_indices(), a.reps),
                            sobol_indices_uncertainty_ms=timed(lambda: m.sobol_indices(uncertainty=True), a.reps))
    pairs = np.array([(k, kp) for k in range(q) for kp in range(k, q)], np.int32)
    for mn in [int(v) for v in a.ms.split(',')]:
        xn = lo + (hi - lo) * rng.random((mn, d))
        yn = rng.standard_normal((int(m.p), mn))
        view = m.condition(xn, yn)
        v = c[:, None] * np.ones((1, n + mn))
        r = dict(pair_ratio=((n + mn) / n) ** 2)
        r['condition_sobol_matrix_sums_ms'] = timed(lambda: eng.condition_sobol_matrix_sums(view._state, v, ell, box, np.arange(q)),
                                                    a.reps)
        if a.only:
            out['m=%d' % mn] = r
            continue
        r['integrated_variance_ms'] = timed(lambda: view.integrated_variance(), a.reps)
        r['sobol_indices_ms'] = timed(lambda: view.sobol_indices(), a.reps)
        r['sobol_indices_uncertainty_ms'] = timed(lambda: view.sobol_indices(uncertainty=True), a.reps)
        for name in ('integrated_variance_ms', 'sobol_indices_ms', 'sobol_indices_uncertainty_ms'):
            ratio = r[name][0] / out['model'][name][0]
            r[name.replace('_ms', '_over_model')] = ratio
            r[name.replace('_ms', '_within_1p5_of_pair_ratio')] = bool(ratio <= 1.5 * r['pair_ratio'])
        iv_view, iv_model = view.integrated_variance().numpy(), m.integrated_variance().numpy()
        r['integrated_variance_over_models_range'] = [float((iv_view / iv_model).min()), float((iv_view / iv_model).max())]
        # the route without the view's queries
        xs = m._standardise_x0(xn)[0]
        ys = (yn - m.ymean.numpy()) / m.ystd.numpy()
        xa, Ya = np.vstack([m._x_train(), xs]), np.hstack([m.y.numpy(), ys])
        made = []

        def construct():
            made.clear()
            torch.cuda.empty_cache()
            made.append(HotPathEngine(xa, Ya, None, q_local=q, kernel=m.kernel))
            torch.cuda.synchronize()

        r['augmented_construct_ms'] = timed(construct, a.reps)
        aug = made[0]
        r['augmented_evaluate_ms'] = timed(lambda: aug.evaluate(th), a.reps)
        va = (c * np.sqrt(D))[:, None] * np.ones((1, n + mn))
        r['augmented_sobol_matrix_sums_ms'] = timed(lambda: aug.sobol_matrix_sums(xa, va, ell, box, np.arange(q)), a.reps)
        w = c[:, None] * np.stack([aug.fetch_vector(1, k) for k in range(q)])
        r['augmented_sobol_pairs_ms'] = timed(lambda: aug.sobol_pairs(xa, w, ell, box, pairs), a.reps)
        r['augmented_route_integrated_variance_ms'] = (r['augmented_construct_ms'][0] + r['augmented_evaluate_ms'][0]
                                                       + r['augmented_sobol_matrix_sums_ms'][0])
        r['augmented_route_sobol_indices_uncertainty_ms'] = (r['augmented_route_integrated_variance_ms']
                                                             + r['augmented_sobol_pairs_ms'][0])
        out['m=%d' % mn] = r
        del aug, made, view
        torch.cuda.empty_cache()
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
