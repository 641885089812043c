"""Times LCGP.loss_hessian against the 2 P evaluations of loss_and_grad that central differences of the gradient need, at the
headline shape (n = 4096, d = 6, p = 64, q = 8, float64), in one process on one GPU.

    python tools/hess_time.py [--n 4096] [--d 6] [--p 64] [--q 8] [--reps 5] [--out profiles/hess_time.txt]

HIP events around the whole call (host assembly included: it is part of what a user waits for); one warm-up of each side, the
median of `reps` repeats; the clock the chip held in the A^-1 launch of the last evaluation (lcgp_lauum_clock) is printed
beside the two numbers, as bench.py reports it."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402


def timed(fn, reps):
    fn()                                                    # warm-up: first-touch of the scratch, plan, code objects
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--d', type=int, default=6)
    ap.add_argument('--p', type=int, default=64)
    ap.add_argument('--q', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    x, y = synth.make_full(3, a.n, a.d, a.p, a.q)
    m = LCGP(y=y, x=x, q=a.q, device='cuda:0')
    u = synth.param_points(3, m._get_flat())[1]
    P = u.size
    m.loss_and_grad(u)

    def hess():
        m._invalidate()                                     # the factorisation is part of the cost: nothing is reused
        return m.loss_hessian(u)

    def differences():
        for i in range(P):
            e = np.zeros(P)
            e[i] = 1e-5 * max(1.0, abs(u[i]))
            m.loss_and_grad(u + e)
            m.loss_and_grad(u - e)

    t_h, all_h = timed(hess, a.reps)
    t_d, all_d = timed(differences, max(1, a.reps // 2))
    eng = m._get_engine()
    clk = torch.zeros(2, dtype=torch.int64, device='cuda:0')
    eng.lib.lcgp_lauum_clock(eng._stream(), eng.dtype, eng.n, eng.d, eng.p, eng.q_local, eng._p(eng.workspace), eng._p(clk))
    c = clk.cpu().numpy()
    mhz = 100.0 * c[0] / c[1] if c[1] else float('nan')
    lines = ["shape n=%d d=%d p=%d q=%d float64, P=%d parameters, device %s" % (a.n, a.d, a.p, a.q, P, torch.cuda.get_device_name(0)),
             "loss_hessian (factorisation included): median %.1f ms of %s" % (t_h, ["%.1f" % v for v in all_h]),
             "2 P = %d loss_and_grad evaluations: median %.1f ms of %s" % (2 * P, t_d, ["%.1f" % v for v in all_d]),
             "ratio %.2f, clock in the last A^-1 launch %.0f MHz" % (t_d / t_h, mhz)]
    print("\n".join(lines))
    if a.out:
        with open(a.out, 'w') as f:
            f.write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
