"""Timing and accuracy of the exact box ALC (LCGP.integrated_variance_reduction) at the headline shape, beside
the two ways there were to the same decision.

At n = 4096, d = 6, p = 64, q = 8 in fp64 (synth.make_config(3)) and 2000 candidates uniform in the training box one process
times, by the wall clock around calls that end in a device-to-host copy (median, minimum and maximum over --reps calls after one
warm-up call):
  - LCGP.integrated_variance_reduction(x_cand) and HotPathEngine.box_alc_block on the 8 components;
  - LCGP.variance_reduction(x_cand, x_ref) with 4096 uniform reference points in the box: ALC over a Monte Carlo stand-in;
  - LCGP.integrated_variance() and 8 single-run condition(x_c, .).integrated_variance() calls: the only exact route before.
For those 8 candidates it reports |gain - (IV - IV_view)| over the prior term scale_a^2 sum_k W_ka^2 c_k and over the gain (worst
over the outputs): the only accuracy figure at this n.  Prints one JSON line.  Nothing is gated: the figures are recorded in
profiles/box_alc_bench.txt.

    python tools/box_alc_bench.py
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/box_alc_bench.py --only pass      (the per-kernel split)"""
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
    ap.add_argument('--cands', type=int, default=2000)
    ap.add_argument('--only', default=None, choices=('pass',), help='the engine pass alone, for a kernel trace of this tool')
    a = ap.parse_args()
    from lcgp_amd import LCGP, synth
    x, y, cfg = synth.make_config(3)
    m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0')
    m.loss_and_grad(m._get_flat())
    eng = m._ensure_aux64()
    n, d, q, p = int(eng.n), int(eng.d), int(m.q), int(m.p)
    xn = np.asarray(x, np.float64)
    lo, hi = xn.min(axis=0), xn.max(axis=0)
    rng = np.random.default_rng(3)
    xc = lo + (hi - lo) * rng.random((a.cands, d))
    xc_s = m._standardise_x0(xc)[0]
    box_s = np.stack([np.zeros(d), np.ones(d)])
    out = dict(n=n, d=d, p=p, q=q, n_cand=a.cands, reps=a.reps)
    out['box_alc_block_ms'] = timed(lambda: eng.box_alc_block(xc_s, box_s, None, 1).cpu(), a.reps)
    if a.only:
        print(json.dumps(out))
        return 0
    out['integrated_variance_reduction_ms'] = timed(lambda: m.integrated_variance_reduction(xc), a.reps)
    xr = lo + (hi - lo) * rng.random((4096, d))
    out['variance_reduction_4096_ref_ms'] = timed(lambda: m.variance_reduction(xc, x_ref=xr), a.reps)
    out['integrated_variance_ms'] = timed(lambda: m.integrated_variance(), a.reps)
    gain = m.integrated_variance_reduction(xc).numpy()
    iv = m.integrated_variance().numpy()
    W, _, scale, _ = m._output_map()
    scale_k, nug = m.lLmb0.numpy(), m.lnugGPs.numpy()
    prior = scale ** 2 * ((W ** 2).T @ (scale_k * (1.0 - nug / (1.0 + nug))))
    ts, over_prior, over_gain = [], [], []
    for j in range(8):
        t0 = time.perf_counter()
        after = m.condition(xc[j:j + 1], np.zeros((p, 1))).integrated_variance().numpy()
        ts.append(1e3 * (time.perf_counter() - t0))
        err = np.abs(gain[:, j] - (iv - after))
        over_prior.append(float(np.max(err / prior)))
        over_gain.append(float(np.max(err / np.abs(gain[:, j]))))
    out['condition_integrated_variance_ms'] = [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]
    out['gain_error_over_prior'] = over_prior
    out['gain_error_over_gain'] = over_gain
    out['gain_over_prior_range'] = [float((gain / prior[:, None]).min()), float((gain / prior[:, None]).max())]
    out['negative_gains'] = int(np.sum(gain < 0.0))
    alc = m.variance_reduction(xc, x_ref=xr).numpy()
    out['monte_carlo_alc_relative_difference_range'] = [float(np.min(np.abs(alc - gain) / np.abs(gain))),
                                                        float(np.max(np.abs(alc - gain) / np.abs(gain)))]
    out['same_best_candidate_outputs'] = int(np.sum(np.argmax(alc, axis=1) == np.argmax(gain, axis=1)))
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
