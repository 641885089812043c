"""Timing of the greedy batch design (LCGP.select_batch) at the headline shape (n = 4096, d = 6, p = 64, q = 8; n_ref = n_cand =
--cands, size = --size), float64 and float32, next to the routes that exist without it, in the same process on the same sets.

Per dtype, median of --reps after a warm-up, each window bracketed by device events on the current stream:
  - begin: HotPathEngine.select_begin (U and gvar of both sets, the step-0 state; the window also holds the host-to-device
    copies of the inputs);
  - select: HotPathEngine.select_batch_block, begin and all `size` steps enqueued without a host synchronisation;
    step = (select - begin) / (size - 1): one lcgp_select_score and one lcgp_select_condition;
  - share: the traffic of a step, 2 q (n_ref + n_cand) npad elements, over the step time, as a share of the 6.29 TB/s copy rate;
  - (a) vr: one HotPathEngine.variance_reduction_block over the same sets (reference set given explicitly);
  - (b) parent route per pick: on an engine built on the training set augmented by one row, one evaluation (refactorisation)
    and one variance_reduction_block (the engine's construction and uploads are left out of the window);
  - the public call end to end (wall clock).
Condition, stated in the output: select (size picks) < size x (a).  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lcgp_amd import LCGP, synth  # noqa: E402
from lcgp_amd.engine import HotPathEngine  # noqa: E402
from tools.vr_bench import device_ms, pad, wall_ms  # noqa: E402

COPY_RATE = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cands', type=int, default=2000)
    ap.add_argument('--size', type=int, default=32)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtypes', default='float64,float32')
    a = ap.parse_args()
    x, y, cfg = synth.make_config(3)
    x = np.asarray(x)
    lo, hi = x.min(axis=0), x.max(axis=0)
    rng = np.random.default_rng(1)
    xc = lo + (hi - lo) * rng.random((a.cands, x.shape[1]))
    xr = lo + (hi - lo) * rng.random((a.cands, x.shape[1]))
    out = dict(n=cfg['n'], d=cfg['d'], p=cfg['p'], q=cfg['q'], n_ref=a.cands, n_cand=a.cands, size=a.size)
    w = np.full(a.cands, 1.0 / a.cands)
    for dt in a.dtypes.split(','):
        m = LCGP(y=y, x=x, q=cfg['q'], device='cuda:0', dtype=dt)
        m.loss_and_grad(m._get_flat())
        eng = m._aux_engine
        xc_s, xr_s, xt = m._standardise_x0(xc)[0], m._standardise_x0(xr)[0], m._x_train()
        W, _, scale, _ = m._output_map()
        om = np.mean(W ** 2 * (scale ** 2)[None, :], axis=1)
        esz = 8 if eng.dtype_name == 'float64' else 4
        t_begin = device_ms(lambda: eng.select_begin(xc_s, xr_s, w, None, 1, a.size), a.reps)
        t_sel = device_ms(lambda: eng.select_batch_block(xc_s, xr_s, w, None, 1, a.size, om), a.reps)
        t_vr = device_ms(lambda: eng.variance_reduction_block(xc_s, xr_s, w, None, 1), a.reps)
        t_step = (t_sel - t_begin) / max(a.size - 1, 1)
        traffic = 2.0 * eng.q_local * (2 * a.cands) * pad(eng.n, 128) * esz
        aug = HotPathEngine(np.vstack([xt, xc_s[:1]]), np.zeros((cfg['p'], len(xt) + 1)), None, q_local=eng.q_local,
                            kernel=m.kernel, dtype=dt)
        th = eng._theta_last.copy()
        aug.evaluate(th)

        def parent():
            aug.upload_theta(th)
            aug.enqueue()
            aug.variance_reduction_block(xc_s, xr_s, w, None, 1)

        t_parent = device_ms(parent, a.reps)
        res = dict(engine=eng.dtype_name, begin_ms=t_begin, select_ms=t_sel, step_ms=t_step, step_bytes=traffic,
                   share_of_copy_rate=traffic / (t_step * 1e-3) / COPY_RATE, vr_ms=t_vr, parent_route_per_pick_ms=t_parent,
                   parent_route_total_ms=a.size * t_parent, size_x_vr_ms=a.size * t_vr,
                   condition_select_below_size_x_vr=bool(t_sel < a.size * t_vr),
                   wall_ms=wall_ms(lambda: m.select_batch(xc, a.size, x_ref=xr), a.reps))
        out[dt] = res
        del m, eng, aug
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
