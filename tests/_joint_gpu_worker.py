"""Worker of tests/test_gpu_joint.py::test_two_ranks_draw_and_cover_what_one_rank_does: one rank of a 2-rank gloo job in
which both ranks drive the same GPU (component k -> rank k mod 2).  Every rank also builds the same model on a one-rank
group of its own, which holds all components, and compares: the draws bitwise (the normals of component k are seeded by
its GLOBAL index), the joint covariance to 1e-13 relative."""
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
    for mode, q, maker in (("full", 3, lambda: synth.make_full(61, 300, 2, 4, 3)),
                           ("rep", 4, lambda: synth.make_rep(62, 70, 3, 2, 4, 4))):
        x, y = maker()
        m2 = LCGP(y=y, x=x, q=q, submethod=mode, device="cuda:0")
        m1 = LCGP(y=y, x=x, q=q, submethod=mode, device="cuda:0", process_group=solo)
        m1.phi = m2.phi.clone()                 # rank 0's basis, as the two-rank model holds it
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        o = orc.OracleLCGP(y=y, x=x, q=q, submethod=mode)
        u = synth.param_points(61, o.get_unconstrained())[1]
        m1._set_flat(u)
        m2._set_flat(u)
        x0 = np.random.default_rng(5).uniform(0, 1, (150, 2))
        s2 = m2.sample(x0, size=9, seed=77).numpy()
        s1 = m1.sample(x0, size=9, seed=77).numpy()
        assert len(m2._local_ks) == len(range(rank, q, world)) and len(m1._local_ks) == q
        assert np.array_equal(s1, s2), (rank, mode, np.max(np.abs(s1 - s2)))
        j2 = m2.predict_jointcov(x0).numpy()
        j1 = m1.predict_jointcov(x0).numpy()
        assert np.max(np.abs(j1 - j2)) <= 1e-13 * np.max(np.abs(j1)), (rank, mode, np.max(np.abs(j1 - j2)))
        l2 = m2.predict_latent_cov(x0).numpy()
        l1 = m1.predict_latent_cov(x0).numpy()
        assert l2.shape == (q, 150, 150)
        assert np.max(np.abs(l1 - l2)) <= 1e-13 * np.max(np.abs(l1)), (rank, mode)
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(63, 100, 2, 3, 1)
    m = LCGP(y=y, x=x, q=1, device="cuda:0")
    x0 = np.random.default_rng(6).uniform(0, 1, (20, 2))
    s = m.sample(x0, size=4, seed=5).numpy()
    assert s.shape == (4, 3, 20) and np.all(np.isfinite(s))
    assert m.predict_jointcov(x0).shape == (3, 20, 20)
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
