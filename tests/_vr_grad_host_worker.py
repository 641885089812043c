"""Worker of tests/test_variance_reduction_grad_host.py::test_two_ranks_gather_what_one_rank_computes: one rank of a world_size-2
gloo job (CPU).  The closed form is answered by the numpy stand-in of tests/vr_grad_ref.py; what is under test is the sharding
of the components and the single reduction that gathers the (q_local, n_cand + n_cand d) blocks."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402
from tests.test_variance_reduction_host import patch_vr  # noqa: E402
from tests.vr_grad_ref import VrGradOracleEngine  # noqa: E402


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
    for mode, q, maker in (("full", 3, lambda: synth.make_full(21, 40, 2, 4, 3)),
                           ("rep", 4, lambda: synth.make_rep(22, 15, 3, 2, 4, 4))):
        x, y = maker()
        m2 = patch_vr(LCGP(y=y, x=x, q=q, submethod=mode), VrGradOracleEngine)
        m1 = patch_vr(LCGP(y=y, x=x, q=q, submethod=mode, process_group=solo), VrGradOracleEngine)
        m1.phi = m2.phi.clone()
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        u = synth.param_points(21, orc.OracleLCGP(y=y, x=x, q=q, submethod=mode).get_unconstrained())[1]
        m1._set_flat(u)
        m2._set_flat(u)
        xn = np.asarray(x)
        xc = xn.min(axis=0) + (xn.max(axis=0) - xn.min(axis=0)) * np.random.default_rng(3).random((7, xn.shape[1]))
        r = 2 if mode == 'rep' else 1
        for latent in (False, True):
            a = m2.variance_reduction_grad(xc, x_ref=xn[:9], replicates=r, latent=latent)
            b = m1.variance_reduction_grad(xc, x_ref=xn[:9], replicates=r, latent=latent)
            assert np.array_equal(a[0].numpy(), b[0].numpy()), (rank, mode, latent)
            assert np.array_equal(a[1].numpy(), b[1].numpy()), (rank, mode, latent)
        assert a[0].shape == (q, len(xc)) and a[1].shape == (q, len(xc), xn.shape[1])
        assert len(m2._local_ks) < q and len(m1._local_ks) == q
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(23, 30, 2, 3, 1)
    m = patch_vr(LCGP(y=y, x=x, q=1), VrGradOracleEngine)
    assert m.variance_reduction_grad(np.asarray(x)[:5] + 0.01)[1].shape == (3, 5, 2)
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
