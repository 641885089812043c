"""Worker of tests/test_marginal_host.py::test_two_ranks_gather_what_one_rank_computes: one rank of a world_size-2 gloo job
(CPU).  The closed form is answered by the numpy stand-in of tests/test_marginal_host.py; what is under test is the sharding of
the components and the single reduction that gathers the (q_local, 2, n0) blocks."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402
from tests.test_marginal_host import patch_engine  # noqa: E402


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
    for mode, q, maker in (("full", 3, lambda: synth.make_full(21, 40, 2, 4, 3)),
                           ("rep", 4, lambda: synth.make_rep(22, 15, 3, 2, 4, 4))):
        x, y = maker()
        m2 = patch_engine(LCGP(y=y, x=x, q=q, submethod=mode))
        m1 = patch_engine(LCGP(y=y, x=x, q=q, submethod=mode, process_group=solo))
        m1.phi = m2.phi.clone()
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        u = synth.param_points(21, orc.OracleLCGP(y=y, x=x, q=q, submethod=mode).get_unconstrained())[1]
        m1._set_flat(u)
        m2._set_flat(u)
        xn = np.asarray(x)
        x0 = xn.min(axis=0) + (xn.max(axis=0) - xn.min(axis=0)) * np.random.default_rng(3).random((7, xn.shape[1]))
        mask = np.random.default_rng(4).random((7, xn.shape[1])) < 0.5
        for latent in (False, True):
            a, b = m2.predict_marginal(x0, mask, latent=latent), m1.predict_marginal(x0, mask, latent=latent)
            assert a[0].shape == ((q if latent else 4), 7)
            assert np.array_equal(a[0].numpy(), b[0].numpy()) and np.array_equal(a[1].numpy(), b[1].numpy()), (rank, mode, latent)
        e2, e1 = m2.main_effects(grid=4), m1.main_effects(grid=4)
        for name in ("grid", "mean", "var", "overall", "overall_var", "effect"):
            assert np.array_equal(getattr(e2, name).numpy(), getattr(e1, name).numpy()), (rank, mode, name)
        assert len(m2._local_ks) < q and len(m1._local_ks) == q
    # q < world: rank 1 holds no component and still takes part in the gather
    x, y = synth.make_full(23, 30, 2, 3, 1)
    m = patch_engine(LCGP(y=y, x=x, q=1))
    assert m.main_effects(grid=3).mean.shape == (3, 2, 3)
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
