"""Timing of the calibration target (LCGP.calibration, lcgp_calib_rows) at the headline shape (n = 4096, d = 6, p = 64, q = 8,
fp64) and at one q = 16 model of the same data shape, for n0 = 64 and n0 = 2000 rows of theta.

Three things, alternated in ONE process (each window: --inner calls between two device synchronisations; median of --reps
windows after a warm-up of every shape), per call:
  1. HotPathEngine.predict_grad_block alone: what a caller paid before this entry existed, the yardstick;
  2. CalibrationTarget.loglik_grad end to end (the same device pass, the row kernel, the copies to the host);
  3. the row kernel alone (ONE launch, lcgp_calib_rows on the device blocks) against the same rows written with batched torch
     operations on the device (torch.linalg.cholesky, solve_triangular, einsum: the formulation below lives in this tool
     only, the library has none).  Their outputs are compared first.
The row kernel has to be no slower than the torch formulation at every shape (margin 0): the tool says PASS / FAIL per shape and
exits 1 on a FAIL.  The overhead of (2) over (1) is recorded, not gated.  Prints text; profiles/calib_bench.txt is its output."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def torch_rows(blk, jac, M, b, c0, lognorm, inv_range):
    """the row formulas of include/lcgp_hip.h with batched torch operations on the device: (ll, dll, s, v)"""
    import torch
    g, h = blk[0].T, blk[1].T.clamp_min(0.0).sqrt()                        # (n0, q)
    mg = g @ M
    w = b - mg
    K = torch.eye(M.shape[0], dtype=M.dtype, device=M.device) + h[:, :, None] * M * h[:, None, :]
    L = torch.linalg.cholesky(K)
    u = torch.linalg.solve_triangular(L, (h * w)[:, :, None], upper=False)[..., 0]
    logs = L.diagonal(dim1=1, dim2=2).log().sum(1)
    ll = -0.5 * (c0 - 2.0 * (g @ b) + (g * mg).sum(1) - (u * u).sum(1) + 2.0 * logs + lognorm)
    a = h * torch.linalg.solve_triangular(L.transpose(1, 2), u[:, :, None], upper=True)[..., 0]
    s = w - a @ M
    R = torch.linalg.solve_triangular(L, h[:, :, None] * M, upper=False)
    v = 0.5 * s * s - 0.5 * (M.diagonal() - (R * R).sum(1))
    dll = inv_range * (torch.einsum('ik,kil->il', s, jac[0]) + torch.einsum('ik,kil->il', v, jac[1]))
    return ll, dll, s.T, v.T


def window(fn, inner):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=20)
    a = ap.parse_args()
    import torch
    from lcgp_amd import LCGP, synth
    from lcgp_amd.engine import calib_rows_device
    _, _, cfg = synth.make_config(3)
    print('# calib_bench: n = %d, d = %d, p = %d, fp64; per call, median of %d windows of %d calls, alternated in one process'
          % (cfg['n'], cfg['d'], cfg['p'], a.reps, a.inner))
    failed = False
    for q in (cfg['q'], 16):
        x, y = synth.make_full(3, cfg['n'], cfg['d'], cfg['p'], q)
        m = LCGP(y=y, x=x, q=q, device='cuda:0')
        m.loss_and_grad(m._get_flat())
        eng = m._aux_engine
        rng = np.random.default_rng(0)
        sd = y.std(axis=1)
        tgt = m.calibration(y[:, 100] + 0.1 * sd * rng.standard_normal(cfg['p']), (0.1 * sd) ** 2)
        for n0 in (64, 2000):
            theta = rng.uniform(0, 1, (n0, cfg['d']))
            x0s = m._x0_2d(theta, 'theta')
            blk, jac = eng.predict_grad_block(x0s)
            M, b, inv_range = tgt._device_consts(blk.device)
            fns = {
                'predict_grad_block': lambda: eng.predict_grad_block(x0s),
                'loglik_grad': lambda: tgt.loglik_grad(theta),
                'row_kernel': lambda: calib_rows_device(blk, jac, M, b, tgt.c0, tgt.lognorm, inv_range, True),
                'torch_rows': lambda: torch_rows(blk, jac, M, b, tgt.c0, tgt.lognorm, inv_range),
            }
            got = [t for t in fns['row_kernel']()]
            want = fns['torch_rows']()
            got = (got[0], got[1], got[2][0], got[2][1])
            diff = [float((g - w_).abs().max() / w_.abs().max()) for g, w_ in zip(got, want)]
            for fn in fns.values():                                   # warm-up of every shape
                window(fn, 3)
            ts = {k: [] for k in fns}
            for _ in range(a.reps):
                for k, fn in fns.items():
                    ts[k].append(window(fn, a.inner if k in ('row_kernel', 'torch_rows') else max(2, a.inner // 5)))
            med = {k: float(np.median(v)) for k, v in ts.items()}
            spread = {k: (float(np.min(v)), float(np.max(v))) for k, v in ts.items()}
            ratio = med['torch_rows'] / med['row_kernel']
            ok = med['row_kernel'] <= med['torch_rows']
            failed |= not ok
            print('q = %2d  n0 = %4d' % (q, n0))
            for k in fns:
                print('    %-20s %10.1f us   (min %.1f, max %.1f)' % (k, 1e6 * med[k], 1e6 * spread[k][0], 1e6 * spread[k][1]))
            print('    loglik_grad over predict_grad_block: +%.1f us (x%.3f)   [recorded, not gated]'
                  % (1e6 * (med['loglik_grad'] - med['predict_grad_block']), med['loglik_grad'] / med['predict_grad_block']))
            print('    torch_rows / row_kernel = %.2f   %s   (largest relative difference ll %.1e, dll %.1e, s %.1e, v %.1e)'
                  % (ratio, 'PASS' if ok else 'FAIL', *diff))
        del m, eng, tgt
        torch.cuda.empty_cache()
    sys.exit(1 if failed else 0)


if __name__ == '__main__':
    main()
