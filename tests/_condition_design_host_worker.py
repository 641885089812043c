"""Worker of tests/test_condition_design_host.py::test_two_ranks_gather_what_one_rank_computes: one rank of a world_size-2 gloo
job (CPU).  The closed form is answered by the numpy stand-in of test_condition_design_host; what is under test is the sharding
of the components, the reduction that gathers the view's (q_local, n_cand) blocks, the per-step gather and rank 0's broadcast
argmax of select_batch (the helper the base method uses), and a rank without components taking part in the collectives."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402
from tests.test_condition_design_host import DesignOracleEngine  # noqa: E402
from tests.test_condition_host import patch_cond  # noqa: E402


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
    rng = np.random.default_rng(3)
    for mode, q, maker in (("full", 3, lambda: synth.make_full(21, 40, 2, 4, 3)),
                           ("rep", 4, lambda: synth.make_rep(22, 15, 3, 2, 4, 4))):
        x, y = maker()
        m2 = patch_cond(LCGP(y=y, x=x, q=q, submethod=mode), DesignOracleEngine)
        m1 = patch_cond(LCGP(y=y, x=x, q=q, submethod=mode, process_group=solo), DesignOracleEngine)
        m1.phi = m2.phi.clone()
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        u = synth.param_points(21, orc.OracleLCGP(y=y, x=x, q=q, submethod=mode).get_unconstrained())[1]
        m1._set_flat(u)
        m2._set_flat(u)
        xn = rng.uniform(0, 1, (5, 2))
        if mode == 'rep':
            xn = np.vstack([xn, xn[:2]])
        yn = rng.standard_normal((4, len(xn)))
        xc, xr = rng.uniform(0, 1, (8, 2)), rng.uniform(0, 1, (6, 2))
        if mode == 'rep':
            xc[2] = m2.x_unique.numpy()[3]
        r = 2 if mode == 'rep' else 1
        v2, v1 = m2.condition(xn, yn), m1.condition(xn, yn)
        assert len(m2._local_ks) < q and len(m1._local_ks) == q
        for latent in (False, True):
            a = v2.variance_reduction(xc, x_ref=xr, replicates=r, latent=latent)
            b = v1.variance_reduction(xc, x_ref=xr, replicates=r, latent=latent)
            assert np.array_equal(a.numpy(), b.numpy()), (rank, mode, latent)
        assert v2.variance_reduction(xc, latent=True).shape == (q, 8)
        for a, b in zip(v2.select_batch(xc, 4, x_ref=xr, replicates=r, return_scores=True),
                        v1.select_batch(xc, 4, x_ref=xr, replicates=r, return_scores=True)):
            assert np.array_equal(a.numpy(), b.numpy()), (rank, mode)
        # the base model's select_batch goes through the same helper and still agrees
        for a, b in zip(m2.select_batch(xc, 3, x_ref=xr, replicates=r), m1.select_batch(xc, 3, x_ref=xr, replicates=r)):
            assert np.array_equal(a.numpy(), b.numpy()), (rank, mode)
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(23, 30, 2, 3, 1)
    m = patch_cond(LCGP(y=y, x=x, q=1), DesignOracleEngine)
    view = m.condition(np.asarray(x)[:5] + 0.01, np.asarray(y)[:, :5])
    xc = np.asarray(x)[:6] + 0.02
    assert tuple(view.variance_reduction(xc).shape) == (3, 6)
    idx, gain = view.select_batch(xc, 3)
    assert idx.shape == (3,) and len(set(idx.tolist())) == 3
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
