"""Worker of tests/test_gpu_matern52.py::test_two_ranks_reproduce_one_rank: one rank of a 2-rank gloo job in which both ranks
drive the same GPU (component k -> rank k mod 2), with the Matern-5/2 kernel.  Every rank also builds the same model on a
one-rank group of its own, which holds all components, and compares: objective, gradient and the joint output covariance
(sums over the ranks) to reduction-order rounding, every other post-fit query bit for bit, as the workers of the existing
two-rank tests do."""
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
        m2 = LCGP(y=y, x=x, q=q, submethod=mode, device="cuda:0", kernel="matern52")
        m1 = LCGP(y=y, x=x, q=q, submethod=mode, device="cuda:0", kernel="matern52", process_group=solo)
        m1.phi = m2.phi.clone()
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        u = synth.param_points(81, orc.OracleLCGP(y=y, x=x, q=q, submethod=mode).get_unconstrained())[1]
        v2, g2 = m2.loss_and_grad(u)
        v1, g1 = m1.loss_and_grad(u)
        assert abs(v1 - v2) <= 1e-12 * abs(v1), (rank, mode, v1, v2)
        assert np.max(np.abs(g1 - g2)) <= 1e-10 * np.max(np.abs(g1)), (rank, mode)
        m1._set_flat(u)
        m2._set_flat(u)
        xn = np.asarray(x)
        xc = xn.min(axis=0) + (xn.max(axis=0) - xn.min(axis=0)) * np.random.default_rng(5).random((60, xn.shape[1]))
        r = 2 if mode == 'rep' else 1
        for a, b in zip(m2.predict(xc), m1.predict(xc)):
            assert torch.equal(a, b), (rank, mode, 'predict')
        for a, b in zip(m2.predict_grad(xc), m1.predict_grad(xc)):
            assert torch.equal(a, b), (rank, mode, 'predict_grad')
        j2, j1 = m2.predict_jointcov(xc).numpy(), m1.predict_jointcov(xc).numpy()      # (summed over the ranks: 1e-13, as
        assert np.max(np.abs(j1 - j2)) <= 1e-13 * np.max(np.abs(j1)), (rank, mode, 'predict_jointcov')    # tests/_joint_gpu_worker.py)
        assert torch.equal(m2.sample(xc, size=3, seed=4), m1.sample(xc, size=3, seed=4)), (rank, mode, 'sample')
        for a, b in zip(m2.predict_loo(), m1.predict_loo()):
            assert torch.equal(a, b), (rank, mode, 'predict_loo')
        a = m2.variance_reduction(xc, x_ref=xn[:77], replicates=r)
        b = m1.variance_reduction(xc, x_ref=xn[:77], replicates=r)
        assert torch.equal(a, b), (rank, mode, 'variance_reduction')
        for a, b in zip(m2.select_batch(xc, 4, replicates=r), m1.select_batch(xc, 4, replicates=r)):
            assert torch.equal(a, b), (rank, mode, 'select_batch')
        assert len(m2._local_ks) == len(range(rank, q, world)) and len(m1._local_ks) == q
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
