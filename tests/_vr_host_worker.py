"""Worker of tests/test_variance_reduction_host.py::test_two_ranks_gather_what_one_rank_computes: one rank of a world_size-2 gloo
job (CPU).  The closed form is answered by the numpy stand-in of test_variance_reduction_host; what is under test is the
sharding of the components, the single reduction that gathers the (q_local, n_cand) blocks, and the agreement of the ranks
on a memory refusal."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402
from tests.test_variance_reduction_host import VrOracleEngine, patch_vr  # noqa: E402


class _RefusesOnComponent1(VrOracleEngine):
    def variance_reduction_block(self, x_cand_s, x_ref_s, w, match, r):
        if 1 in self.comp_ids:
            raise ValueError('the variance reduction needs more device memory than is free')
        return super().variance_reduction_block(x_cand_s, x_ref_s, w, match, r)


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
    for mode, q, maker in (("full", 3, lambda: synth.make_full(21, 40, 2, 4, 3)),
                           ("rep", 4, lambda: synth.make_rep(22, 15, 3, 2, 4, 4))):
        x, y = maker()
        m2 = patch_vr(LCGP(y=y, x=x, q=q, submethod=mode))
        m1 = patch_vr(LCGP(y=y, x=x, q=q, submethod=mode, process_group=solo))
        m1.phi = m2.phi.clone()
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        u = synth.param_points(21, orc.OracleLCGP(y=y, x=x, q=q, submethod=mode).get_unconstrained())[1]
        m1._set_flat(u)
        m2._set_flat(u)
        xn = np.asarray(x)
        xc = xn.min(axis=0) + (xn.max(axis=0) - xn.min(axis=0)) * np.random.default_rng(3).random((7, xn.shape[1]))
        if mode == 'rep':
            xc = np.vstack([xc, m1.x_unique.numpy()[:2]])
        r = 2 if mode == 'rep' else 1
        for latent in (False, True):
            a = m2.variance_reduction(xc, x_ref=xn[:9], replicates=r, latent=latent).numpy()
            b = m1.variance_reduction(xc, x_ref=xn[:9], replicates=r, latent=latent).numpy()
            assert np.array_equal(a, b), (rank, mode, latent)
        assert a.shape == (q, len(xc))
        assert len(m2._local_ks) < q and len(m1._local_ks) == q
        # a refusal on one rank's component is raised on EVERY rank
        patch_vr(m2, _RefusesOnComponent1)
        m2._engine = None
        m2._u_last = None
        try:
            m2.variance_reduction(xc)
        except ValueError as e:
            assert 'device memory' in str(e) or 'another rank' in str(e), str(e)
        else:
            raise AssertionError('no ValueError on rank %d' % rank)
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(23, 30, 2, 3, 1)
    m = patch_vr(LCGP(y=y, x=x, q=1))
    assert m.variance_reduction(np.asarray(x)[:5] + 0.01).shape == (3, 5)
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
