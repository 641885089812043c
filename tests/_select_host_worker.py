"""Worker of tests/test_select_batch_host.py::test_two_ranks_pick_what_one_rank_picks: one rank of a world_size-2 gloo job (CPU).
The conditioning is answered by the dense numpy stand-in of test_select_batch_host; what is under test is the sharding of the
components, the per-step gather of the score terms, the broadcast pick and the agreement of the ranks on a memory refusal."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402
from tests.test_select_batch_host import SelectOracleEngine, patch_select  # noqa: E402


class _RefusesOnComponent1(SelectOracleEngine):
    def select_begin(self, *a):
        if 1 in self.comp_ids:
            raise ValueError('the batch selection needs more device memory than is free')
        return super().select_begin(*a)


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
    for mode, q, maker in (("full", 3, lambda: synth.make_full(21, 40, 2, 4, 3)),
                           ("rep", 4, lambda: synth.make_rep(22, 15, 3, 2, 4, 4))):
        x, y = maker()
        m2 = patch_select(LCGP(y=y, x=x, q=q, submethod=mode))
        m1 = patch_select(LCGP(y=y, x=x, q=q, submethod=mode, process_group=solo))
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
        a = [t.numpy() for t in m2.select_batch(xc, 4, x_ref=xn[:9], replicates=r, return_scores=True)]
        b = [t.numpy() for t in m1.select_batch(xc, 4, x_ref=xn[:9], replicates=r, return_scores=True)]
        for u2, u1 in zip(a, b):
            assert np.array_equal(u2, u1), (rank, mode)
        assert len(set(a[0].tolist())) == 4
        assert len(m2._local_ks) < q and len(m1._local_ks) == q
        # a refusal on one rank's component is raised on EVERY rank
        patch_select(m2, _RefusesOnComponent1)
        try:
            m2.select_batch(xc, 2)
        except ValueError as e:
            assert 'device memory' in str(e) or 'another rank' in str(e), str(e)
        else:
            raise AssertionError('no ValueError on rank %d' % rank)
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(23, 30, 2, 3, 1)
    m = patch_select(LCGP(y=y, x=x, q=1))
    idx, gain = m.select_batch(np.asarray(x)[:5] + 0.01, 3)
    assert idx.shape == (3,) and gain.shape == (3,)
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
