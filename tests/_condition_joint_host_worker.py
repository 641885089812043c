"""Worker of tests/test_condition_joint_host.py::test_two_ranks_draw_what_one_rank_draws: one rank of a world_size-2 gloo job
(CPU).  The closed form is answered by the numpy stand-in of test_condition_joint_host; what is under test is that the joint
covariance, its output projection and the draws of a conditioned view do not depend on how the components are spread over the
ranks (seeding by GLOBAL component, one reduction per query), that a rank without components takes part in the collectives, and
that the ranks agree on a failure of one of them."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402
from tests.test_condition_host import patch_cond  # noqa: E402
from tests.test_condition_joint_host import JointCondOracleEngine  # noqa: E402


class _FailsOnComponent1(JointCondOracleEngine):
    def condition_sample_latent(self, state, x0s, S, seeds, jitter=1e-10):
        if 1 in self.comp_ids:
            err = np.linalg.LinAlgError('Sigma_k')
            err.info = np.array([5 if k == 1 else 0 for k in self.comp_ids])
            raise err
        return super().condition_sample_latent(state, x0s, S, seeds, jitter)


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
    rng = np.random.default_rng(3)
    for mode, q, maker in (("full", 3, lambda: synth.make_full(21, 40, 2, 4, 3)),
                           ("rep", 4, lambda: synth.make_rep(22, 15, 3, 2, 4, 4))):
        x, y = maker()
        m2 = patch_cond(LCGP(y=y, x=x, q=q, submethod=mode), JointCondOracleEngine)
        m1 = patch_cond(LCGP(y=y, x=x, q=q, submethod=mode, process_group=solo), JointCondOracleEngine)
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
        assert len(m2._local_ks) < q and len(m1._local_ks) == q
        assert np.array_equal(v2.predict_latent_cov(x0).numpy(), v1.predict_latent_cov(x0).numpy()), (rank, mode)
        assert tuple(v2.predict_latent_cov(x0).shape) == (q, 7, 7)
        # (the projection sums the ranks' shares: the order of that sum is the one thing that differs)
        a, b = v2.predict_jointcov(x0, outputs=[3, 1]).numpy(), v1.predict_jointcov(x0, outputs=[3, 1]).numpy()
        np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-15 * np.max(np.abs(b)))
        for kw in (dict(seed=5), dict(seed=5, include_noise=False, jitter=1e-8)):
            assert np.array_equal(v2.sample(x0, size=3, **kw).numpy(), v1.sample(x0, size=3, **kw).numpy()), (rank, mode, kw)
        # seed=None: rank 0's fresh seed on every rank
        s = v2.sample(x0, size=2).numpy()
        both = [None, None]
        dist.all_gather_object(both, s.tobytes())
        assert both[0] == both[1]
        # a failure on one rank's component is raised on EVERY rank, naming the component
        vf = patch_cond(m2, _FailsOnComponent1).condition(xn, yn)
        try:
            vf.sample(x0, size=2, seed=1)
        except np.linalg.LinAlgError as e:
            assert '[1]' in str(e) and '[5]' in str(e), str(e)
        else:
            raise AssertionError('no LinAlgError on rank %d' % rank)
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(23, 30, 2, 3, 1)
    m = patch_cond(LCGP(y=y, x=x, q=1), JointCondOracleEngine)
    view = m.condition(np.asarray(x)[:5] + 0.01, np.asarray(y)[:, :5])
    x0 = np.asarray(x)[:6] + 0.02
    assert tuple(view.predict_latent_cov(x0).shape) == (1, 6, 6)
    assert tuple(view.predict_jointcov(x0).shape) == (3, 6, 6)
    assert tuple(view.sample(x0, size=2, seed=0).shape) == (2, 3, 6)
    assert (m._engine is None) == (rank == 1) and (view._state is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
