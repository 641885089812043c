"""Worker of tests/test_sobol_host.py::test_two_ranks_equal_one_rank_bitwise: one rank of a world_size-2 gloo job (CPU).  The
pair sums are answered by the numpy stand-in of tests/test_sobol_host.py; what is under test is the gather of the weight
vectors, the dealing of the pairs over the ranks that hold an engine and the single reduction that completes the array."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402
from tests.test_sobol_host import patch_engine  # noqa: E402

FIELDS = ("first", "total", "variance", "mean", "first_variance", "closed_variance")


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
    for mode, q, kernel, maker in (("full", 3, "matern52", lambda: synth.make_full(21, 40, 2, 4, 3)),
                                   ("rep", 4, "matern32", lambda: synth.make_rep(22, 15, 3, 2, 4, 4))):
        x, y = maker()
        m2 = patch_engine(LCGP(y=y, x=x, q=q, submethod=mode, kernel=kernel))
        m1 = patch_engine(LCGP(y=y, x=x, q=q, submethod=mode, kernel=kernel, process_group=solo))
        m1.phi = m2.phi.clone()
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        u = synth.param_points(21, orc.OracleLCGP(y=y, x=x, q=q, submethod=mode).get_unconstrained())[1]
        m1._set_flat(u)
        m2._set_flat(u)
        xn = np.asarray(x)
        lo, hi = xn.min(axis=0), xn.max(axis=0)
        for box in (None, np.stack([lo + 0.2 * (hi - lo), lo + 0.9 * (hi - lo)])):
            for latent in (False, True):
                a, b = m2.sobol_indices(box=box, latent=latent), m1.sobol_indices(box=box, latent=latent)
                assert a.first.shape == ((q if latent else 4), 2)
                for name in FIELDS:
                    assert np.array_equal(getattr(a, name).numpy(), getattr(b, name).numpy()), (rank, mode, latent, name)
                assert np.all(np.isfinite(a.first.numpy())) and np.all(a.variance.numpy() > 0)
        assert len(m2._local_ks) < q and len(m1._local_ks) == q
    # q < world: rank 1 holds no component, computes no pair and still takes part in the gather and the reduction
    x, y = synth.make_full(23, 30, 2, 3, 1)
    m = patch_engine(LCGP(y=y, x=x, q=1))
    s = m.sobol_indices()
    assert s.first.shape == (3, 2) and np.all(np.isfinite(s.first.numpy()))
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
