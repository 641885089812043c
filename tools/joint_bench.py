"""Timing of the joint posterior covariance (LCGP.predict_latent_cov / predict_jointcov / sample) at the headline shape.

Reports, with device synchronisation around each timed window (median of --reps after a warm-up):
  - lcgp_predict_cov at n = 4096, q = 8, n0 = 2000: the whole call, and the lower tiles of C00 - D U U^T alone
    (= the call minus lcgp_predict at the same n0, which forms the same X and U; rocprofv3 --kernel-trace --stats gives
    the tile_gemm<..., 6, ...> launch on its own);
  - lcgp_potrf_logdet of the cov workspace at n0 = 2048;
  - LCGP.sample(size = 1000) end to end (cov + factorisation + draws + the host projection).
Flop counts are those of the algorithm, from the shapes (n0pad = n0 rounded up to 128):
  lower 64x64 tiles of U U^T: q * t (t + 1) / 2 * 64^2 * npad * 2 with t = n0pad / 64 (2 flops per multiply-add).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lcgp_amd import LCGP, synth  # noqa: E402

FP64_PEAK = 78.6e12


def timed(fn, reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n0', type=int, default=2000)
    ap.add_argument('--n0-factor', type=int, default=2048)
    ap.add_argument('--size', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=10)
    a = ap.parse_args()
    x, y, cfg = synth.make_config(3)
    m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0')
    m.loss_and_grad(m._get_flat())
    eng = m._aux_engine
    rng = np.random.default_rng(0)
    x0s = rng.uniform(0, 1, (a.n0, cfg['d']))
    q, npad = eng.q_local, (eng.n + 127) // 128 * 128
    t = (a.n0 + 127) // 128 * 2
    fl_cov = q * t * (t + 1) / 2 * 64.0 ** 2 * npad * 2
    t_cov = timed(lambda: eng.form_cov(x0s, False, 1e-10), a.reps)
    t_pred = timed(lambda: eng.predict_block(x0s, False), a.reps)
    t_tiles = t_cov - t_pred
    x0f = rng.uniform(0, 1, (a.n0_factor, cfg['d']))
    eng.form_cov(x0f, False, 1e-8)

    def refactor():
        eng.form_cov(x0f, False, 1e-8)
        eng.factor_cov(a.n0_factor)
    t_refac = timed(refactor, a.reps)
    t_form = timed(lambda: eng.form_cov(x0f, False, 1e-8), a.reps)
    t_fac = t_refac - t_form
    fl_fac = q * a.n0_factor ** 3 / 3.0
    x0 = rng.uniform(0, 1, (a.n0, cfg['d'])) * (m.x_max.numpy() - m.x_min.numpy()) + m.x_min.numpy()
    t_samp = timed(lambda: m.sample(x0, size=a.size, seed=1), max(3, a.reps // 3))
    out = dict(n=int(eng.n), q=q, n0=a.n0,
               predict_cov_ms=1e3 * t_cov, predict_ms=1e3 * t_pred,
               cov_tiles_ms=1e3 * t_tiles, cov_tiles_flop=fl_cov, cov_tiles_tflops=fl_cov / t_tiles / 1e12,
               cov_tiles_frac_fp64_peak=fl_cov / t_tiles / FP64_PEAK,
               factor_n0=a.n0_factor, factor_ms=1e3 * t_fac, factor_tflops=fl_fac / t_fac / 1e12,
               sample_size=a.size, sample_ms=1e3 * t_samp)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
