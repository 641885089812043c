"""Worker of tests/test_cv_host.py::test_two_ranks_gather_what_one_rank_computes: one rank of a world_size-2 gloo job (CPU).
The closed form is answered by the numpy stand-in of test_cv_host; what is under test is the sharding of the components, the
single reduction that gathers predictions and fold covariances, and the agreement of the ranks on a failure."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402
from tests.test_cv_host import CvOracleEngine, patch_cv  # noqa: E402


class _FailsOnComponent1(CvOracleEngine):
    def cv_block(self, fold_ptr, fold_idx, return_cov=False):
        if 1 in self.comp_ids:
            err = np.linalg.LinAlgError('fold')
            err.info = np.array([2 if k == 1 else 0 for k in self.comp_ids])
            raise err
        return super().cv_block(fold_ptr, fold_idx, return_cov)


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
    for mode, q, maker in (("full", 3, lambda: synth.make_full(21, 40, 2, 4, 3)),
                           ("rep", 4, lambda: synth.make_rep(22, 15, 3, 2, 4, 4))):
        x, y = maker()
        m2 = patch_cv(LCGP(y=y, x=x, q=q, submethod=mode))
        m1 = patch_cv(LCGP(y=y, x=x, q=q, submethod=mode, process_group=solo))
        m1.phi = m2.phi.clone()
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        u = synth.param_points(21, orc.OracleLCGP(y=y, x=x, q=q, submethod=mode).get_unconstrained())[1]
        m1._set_flat(u)
        m2._set_flat(u)
        for a, b in zip(m2.predict_loo(), m1.predict_loo()):
            assert np.array_equal(a.numpy(), b.numpy()), (rank, mode)
        r2 = m2.predict_cv(3, seed=4, return_latent_cov=True)
        r1 = m1.predict_cv(3, seed=4, return_latent_cov=True)
        assert len(m2._local_ks) < q and len(m1._local_ks) == q
        for a, b in zip(r2[:3], r1[:3]):
            assert np.array_equal(a.numpy(), b.numpy()), (rank, mode)
        for a, b in zip(r2[3], r1[3]):
            assert a.shape[0] == q and np.array_equal(a.numpy(), b.numpy()), (rank, mode)
        # a failure on one rank's component is raised on EVERY rank
        patch_cv(m2, _FailsOnComponent1)
        m2._engine = None
        m2._u_last = None
        try:
            m2.predict_cv(3)
        except np.linalg.LinAlgError as e:
            assert '[1]' in str(e), str(e)
        else:
            raise AssertionError('no LinAlgError on rank %d' % rank)
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(23, 30, 2, 3, 1)
    m = patch_cv(LCGP(y=y, x=x, q=1))
    assert m.predict_loo()[0].shape == (3, 30)
    assert m.predict_cv(5, return_latent_cov=True)[3][0].shape == (1, 6, 6)
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
