"""Worker of tests/test_gpu_box_alc.py::test_two_ranks_equal_one_rank_bitwise: one rank of a 2-rank gloo job in which both ranks
drive the same GPU (component k -> rank k mod 2).  Every rank also builds the same model on a one-rank group of its own, which
holds all components, and compares integrated_variance_reduction bit for bit."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402


def main():
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
    for mode, q, kernel, maker in (("full", 3, "matern32", lambda: synth.make_full(91, 150, 3, 4, 3)),
                                   ("rep", 4, "se", lambda: synth.make_rep(92, 70, 3, 2, 4, 4))):
        x, y = maker()
        m2 = LCGP(y=y, x=x, q=q, submethod=mode, kernel=kernel, device="cuda:0")
        m1 = LCGP(y=y, x=x, q=q, submethod=mode, kernel=kernel, device="cuda:0", process_group=solo)
        m1.phi = m2.phi.clone()                 # rank 0's basis, as the two-rank model holds it
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        o = orc.OracleLCGP(y=y, x=x, q=q, submethod=mode)
        u = synth.param_points(91, o.get_unconstrained())[1]
        m1._set_flat(u)
        m2._set_flat(u)
        xn = np.asarray(x)
        d = xn.shape[1]
        lo, hi = xn.min(axis=0), xn.max(axis=0)
        xc = lo - 0.05 * (hi - lo) + 1.1 * (hi - lo) * np.random.default_rng(5).random((70, d))
        r = 1
        if mode == "rep":
            xc[3], r = m2.x_unique.numpy()[7], 2
        box = np.stack([lo + 0.2 * (hi - lo), lo + 0.85 * (hi - lo)])
        for latent in (False, True):
            a = m1.integrated_variance_reduction(xc, box=box, replicates=r, latent=latent).numpy()
            b = m2.integrated_variance_reduction(xc, box=box, replicates=r, latent=latent).numpy()
            assert a.shape == ((q if latent else 4), 70)
            assert np.array_equal(a, b), (rank, mode, latent, np.max(np.abs(a - b)))
            assert np.all(np.isfinite(a)) and np.all(a > 0)
        assert len(m2._local_ks) == len(range(rank, q, world)) and len(m1._local_ks) == q
    # q < world: rank 1 holds no component and still takes part in the gather
    x, y = synth.make_full(93, 100, 2, 3, 1)
    m = LCGP(y=y, x=x, q=1, device="cuda:0")
    g = m.integrated_variance_reduction(np.asarray(x)[:5] + 0.01).numpy()
    assert g.shape == (3, 5) and np.all(np.isfinite(g)) and np.all(g > 0)
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
