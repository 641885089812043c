"""Worker of tests/test_gpu_variance_reduction_grad.py::test_two_ranks_reproduce_one_rank_bitwise: one rank of a 2-rank gloo job
in which both ranks drive the same GPU (component k -> rank k mod 2).  Every rank also builds the same model on a one-rank
group of its own, which holds all components, and compares value and gradient of the variance reduction bit for bit."""
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
    for mode, q, maker in (("full", 3, lambda: synth.make_full(81, 300, 2, 4, 3)),
                           ("rep", 4, lambda: synth.make_rep(82, 90, 3, 2, 4, 4))):
        x, y = maker()
        m2 = LCGP(y=y, x=x, q=q, submethod=mode, device="cuda:0")
        m1 = LCGP(y=y, x=x, q=q, submethod=mode, device="cuda:0", process_group=solo)
        m1.phi = m2.phi.clone()
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        u = synth.param_points(81, orc.OracleLCGP(y=y, x=x, q=q, submethod=mode).get_unconstrained())[1]
        m1._set_flat(u)
        m2._set_flat(u)
        xn = np.asarray(x)
        xc = xn.min(axis=0) + (xn.max(axis=0) - xn.min(axis=0)) * np.random.default_rng(5).random((150, xn.shape[1]))
        r = 2 if mode == 'rep' else 1
        for ref in (None, xn[:77]):
            for latent in (True, False):
                a = m2.variance_reduction_grad(xc, x_ref=ref, replicates=r, latent=latent)
                b = m1.variance_reduction_grad(xc, x_ref=ref, replicates=r, latent=latent)
                assert np.array_equal(a[0].numpy(), b[0].numpy()), (rank, mode, latent)
                assert np.array_equal(a[1].numpy(), b[1].numpy()), (rank, mode, latent)
        assert a[1].shape == (int(m1.p), len(xc), xn.shape[1])
        assert len(m2._local_ks) == len(range(rank, q, world)) and len(m1._local_ks) == q
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(83, 100, 2, 3, 1)
    m = LCGP(y=y, x=x, q=1, device="cuda:0")
    assert m.variance_reduction_grad(np.asarray(x)[:20] + 0.01)[1].shape == (3, 20, 2)
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
