"""Worker of tests/test_gpu_grad_cov.py::test_two_ranks_equal_one_rank_bitwise: one rank of a 2-rank gloo job in which both
ranks drive the same GPU (component k -> rank k mod 2).  Every rank also builds the same model on a one-rank group of its
own, which holds all components, and compares predict_grad_cov (outputs and latent) and active_subspace bit for bit."""
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
    for mode, q, maker in (("full", 3, lambda: synth.make_full(91, 300, 2, 4, 3)),
                           ("rep", 4, lambda: synth.make_rep(92, 70, 3, 2, 4, 4))):
        x, y = maker()
        m2 = LCGP(y=y, x=x, q=q, submethod=mode, device="cuda:0")
        m1 = LCGP(y=y, x=x, q=q, submethod=mode, device="cuda:0", process_group=solo)
        m1.phi = m2.phi.clone()                 # rank 0's basis, as the two-rank model holds it
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        o = orc.OracleLCGP(y=y, x=x, q=q, submethod=mode)
        u = synth.param_points(91, o.get_unconstrained())[1]
        m1._set_flat(u)
        m2._set_flat(u)
        x0 = np.random.default_rng(5).uniform(0, 1, (150, 2))
        w = np.random.default_rng(6).uniform(0, 1, 150)
        for latent in (False, True):
            a, b = m1.predict_grad_cov(x0, latent=latent).numpy(), m2.predict_grad_cov(x0, latent=latent).numpy()
            assert a.shape == ((q if latent else 4), 150, 2, 2)
            assert np.array_equal(a, b), (rank, mode, latent, np.max(np.abs(a - b)))
        assert np.array_equal(m1.dghat.numpy(), m2.dghat.numpy())
        r1, r2 = m1.active_subspace(x0, weights=w), m2.active_subspace(x0, weights=w)
        for name in ("matrix", "mean_part", "cov_part", "activity", "eigenvalues", "eigenvectors"):
            assert np.array_equal(getattr(r1, name).numpy(), getattr(r2, name).numpy()), (rank, mode, name)
        assert len(m2._local_ks) == len(range(rank, q, world)) and len(m1._local_ks) == q
    # q < world: rank 1 holds no component and still takes part in the gather
    x, y = synth.make_full(93, 100, 2, 3, 1)
    m = LCGP(y=y, x=x, q=1, device="cuda:0")
    x0 = np.random.default_rng(7).uniform(0, 1, (20, 2))
    g = m.predict_grad_cov(x0).numpy()
    assert g.shape == (3, 20, 2, 2) and np.all(np.isfinite(g))
    assert np.all(np.isfinite(m.active_subspace(x0).matrix.numpy()))
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
