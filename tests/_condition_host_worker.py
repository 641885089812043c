"""Worker of tests/test_condition_host.py::test_two_ranks_gather_what_one_rank_computes: one rank of a world_size-2 gloo job
(CPU).  The closed form is answered by the numpy stand-in of test_condition_host; what is under test is the sharding of the
components (each rank holds the state of its own), the single reduction that gathers the view's (q_local, 2, n0) blocks, a
rank without components taking part in the collectives, and the agreement of the ranks on a failure of one of them."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402
from tests.test_condition_host import CondOracleEngine, patch_cond  # noqa: E402


class _FailsOnComponent1(CondOracleEngine):
    def condition_begin(self, xn_s, t, r=None):
        if 1 in self.comp_ids:
            err = np.linalg.LinAlgError('S_k')
            err.info = np.array([5 if k == 1 else 0 for k in self.comp_ids])
            raise err
        return super().condition_begin(xn_s, t, r)


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
    rng = np.random.default_rng(3)
    for mode, q, maker in (("full", 3, lambda: synth.make_full(21, 40, 2, 4, 3)),
                           ("rep", 4, lambda: synth.make_rep(22, 15, 3, 2, 4, 4))):
        x, y = maker()
        m2 = patch_cond(LCGP(y=y, x=x, q=q, submethod=mode))
        m1 = patch_cond(LCGP(y=y, x=x, q=q, submethod=mode, process_group=solo))
        m1.phi = m2.phi.clone()
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        u = synth.param_points(21, orc.OracleLCGP(y=y, x=x, q=q, submethod=mode).get_unconstrained())[1]
        m1._set_flat(u)
        m2._set_flat(u)
        xn = rng.uniform(0, 1, (5, 2))
        if mode == 'rep':
            xn = np.vstack([xn, xn[:2]])
        yn = rng.standard_normal((4, len(xn)))
        x0 = rng.uniform(0, 1, (7, 2))
        v2, v1 = m2.condition(xn, yn), m1.condition(xn, yn)
        assert len(m2._local_ks) < q and len(m1._local_ks) == q and len(v2._state['state']) == len(m2._local_ks)
        for latent in (False, True):
            for a, b in zip(v2.predict(x0, latent=latent), v1.predict(x0, latent=latent)):
                assert np.array_equal(a.numpy(), b.numpy()), (rank, mode, latent)
        assert v2.predict(x0, latent=True)[0].shape == (q, 7)
        # a failure on one rank's component is raised on EVERY rank, naming the component
        patch_cond(m2, _FailsOnComponent1)
        try:
            m2.condition(xn, yn)
        except np.linalg.LinAlgError as e:
            assert '[1]' in str(e) and '[5]' in str(e), str(e)
        else:
            raise AssertionError('no LinAlgError on rank %d' % rank)
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(23, 30, 2, 3, 1)
    m = patch_cond(LCGP(y=y, x=x, q=1))
    view = m.condition(np.asarray(x)[:5] + 0.01, np.asarray(y)[:, :5])
    assert tuple(view.predict(np.asarray(x)[:6] + 0.02)[0].shape) == (3, 6)
    assert (m._engine is None) == (rank == 1) and (view._state is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
