"""Worker of tests/test_condition_sobol_host.py::test_two_ranks_equal_one_rank_bitwise: one rank of a world_size-2 gloo job
(CPU).  The closed forms are answered by the numpy stand-in of tests/condition_sobol_ref.py; what is under test is the gather of
the q augmented weight vectors, the round-robin deal of the pairs, the reduction of the matrix-weighted rows of the owners, and
a rank without components taking part in every collective, for sobol_indices(uncertainty=True) and integrated_variance() on a
view."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402
from tests.condition_sobol_ref import ViewSobolOracleEngine  # noqa: E402
from tests.test_condition_host import patch_cond  # noqa: E402

FIELDS = ("first", "total", "variance", "mean", "first_variance", "closed_variance", "expected_variance",
          "expected_first_variance", "expected_closed_variance", "first_expected", "total_expected", "integrated_variance")


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
    rng = np.random.default_rng(4)
    for mode, q, maker in (("full", 3, lambda: synth.make_full(21, 24, 2, 4, 3)),
                           ("rep", 4, lambda: synth.make_rep(22, 12, 3, 2, 4, 4))):
        x, y = maker()
        m2 = patch_cond(LCGP(y=y, x=x, q=q, submethod=mode, kernel='se'), ViewSobolOracleEngine)
        m1 = patch_cond(LCGP(y=y, x=x, q=q, submethod=mode, kernel='se', process_group=solo), ViewSobolOracleEngine)
        m1.phi = m2.phi.clone()
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        u = synth.param_points(21, orc.OracleLCGP(y=y, x=x, q=q, submethod=mode).get_unconstrained())[1]
        m1._set_flat(u)
        m2._set_flat(u)
        xn = rng.uniform(0, 1, (4, 2))
        if mode == 'rep':
            xn = np.vstack([xn, xn[:2]])
        yn = rng.standard_normal((4, len(xn)))
        box = np.array([[0.2, 0.1], [0.8, 0.9]])
        v2, v1 = m2.condition(xn, yn), m1.condition(xn, yn)
        assert len(m2._local_ks) < q and len(m1._local_ks) == q
        for latent in (False, True):
            a, b = v1.sobol_indices(box=box, latent=latent, uncertainty=True), v2.sobol_indices(box=box, latent=latent,
                                                                                                 uncertainty=True)
            assert tuple(a.first_expected.shape) == ((q if latent else 4), 2)
            for name in FIELDS:
                s, t = getattr(a, name).numpy(), getattr(b, name).numpy()
                assert np.array_equal(s, t), (rank, mode, latent, name, np.max(np.abs(s - t)))
            i1, i2 = v1.integrated_variance(box=box, latent=latent).numpy(), v2.integrated_variance(box=box, latent=latent).numpy()
            assert np.array_equal(i1, i2) and np.array_equal(i1, a.integrated_variance.numpy()), (rank, mode, latent)
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(23, 20, 2, 3, 1)
    m = patch_cond(LCGP(y=y, x=x, q=1), ViewSobolOracleEngine)
    view = m.condition(np.asarray(x)[:3] + 0.01, np.asarray(y)[:, :3])
    s = view.sobol_indices(uncertainty=True)
    assert tuple(s.first_expected.shape) == (3, 2) and np.all(np.isfinite(s.first_expected.numpy()))
    assert np.all(view.integrated_variance().numpy() > 0)
    assert (m._engine is None) == (rank == 1) and (view._state is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
