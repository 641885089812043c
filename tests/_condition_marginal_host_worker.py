"""Worker of tests/test_condition_marginal_host.py::test_two_ranks_gather_what_one_rank_computes: one rank of a world_size-2
gloo job (CPU).  The closed forms are answered by the numpy stand-in of tests/condition_marginal_ref.py; what is under test is
the single reduction that gathers the (q_local, 2 or 3, n0) blocks of predict_marginal(cov_with=...) on the model and on a
view, main_effects(effect_var=True) on both, and a rank without components taking part in the collectives."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402
from tests.condition_marginal_ref import MargCondOracleEngine  # noqa: E402
from tests.test_condition_host import patch_cond  # noqa: E402


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
    rng = np.random.default_rng(4)
    for mode, q, maker in (("full", 3, lambda: synth.make_full(21, 40, 2, 4, 3)),
                           ("rep", 4, lambda: synth.make_rep(22, 15, 3, 2, 4, 4))):
        x, y = maker()
        m2 = patch_cond(LCGP(y=y, x=x, q=q, submethod=mode, kernel='se'), MargCondOracleEngine)
        m1 = patch_cond(LCGP(y=y, x=x, q=q, submethod=mode, kernel='se', process_group=solo), MargCondOracleEngine)
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
        mask = rng.uniform(0, 1, (7, 2)) < 0.5
        row = (np.array([np.nan, 0.4]), [0])
        v2, v1 = m2.condition(xn, yn), m1.condition(xn, yn)
        assert len(m2._local_ks) < q and len(m1._local_ks) == q
        for a2, a1 in ((m2, m1), (v2, v1)):
            for latent in (False, True):
                r2, r1 = a2.predict_marginal(x0, mask, latent=latent, cov_with=row), a1.predict_marginal(x0, mask, latent=latent,
                                                                                                         cov_with=row)
                assert len(r2) == len(r1) == 3 and tuple(r2[2].shape) == ((q if latent else 4), 7)
                for a, b in zip(r2, r1):
                    assert np.array_equal(a.numpy(), b.numpy()), (rank, mode, latent)
            e2, e1 = a2.main_effects(grid=3, effect_var=True), a1.main_effects(grid=3, effect_var=True)
            for name in ('grid', 'mean', 'var', 'overall', 'overall_var', 'effect', 'effect_var'):
                assert np.array_equal(getattr(e2, name).numpy(), getattr(e1, name).numpy()), (rank, mode, name)
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(23, 30, 2, 3, 1)
    m = patch_cond(LCGP(y=y, x=x, q=1), MargCondOracleEngine)
    view = m.condition(np.asarray(x)[:5] + 0.01, np.asarray(y)[:, :5])
    res = view.predict_marginal(np.asarray(x)[:6], [1], cov_with=(np.asarray(x)[0], [0, 1]))
    assert len(res) == 3 and tuple(res[2].shape) == (3, 6)
    assert tuple(view.main_effects(grid=2, effect_var=True).effect_var.shape) == (3, 2, 2)
    assert (m._engine is None) == (rank == 1) and (view._state is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
