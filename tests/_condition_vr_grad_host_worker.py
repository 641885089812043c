"""Worker of tests/test_condition_vr_grad_host.py::test_two_ranks_gather_what_one_rank_computes: one rank of a world_size-2 gloo
job (CPU).  The closed form is answered by the numpy stand-in of test_condition_vr_grad_host; what is under test is the sharding
of the components, the one reduction that gathers the view's (q_local, n_cand + n_cand d) blocks, and a rank without components
taking part in the collectives."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402
from tests.test_condition_host import patch_cond  # noqa: E402
from tests.test_condition_vr_grad_host import VrGradViewOracleEngine  # noqa: E402


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
    rng = np.random.default_rng(3)
    for mode, q, maker in (("full", 3, lambda: synth.make_full(21, 40, 2, 4, 3)),
                           ("rep", 4, lambda: synth.make_rep(22, 15, 3, 2, 4, 4))):
        x, y = maker()
        m2 = patch_cond(LCGP(y=y, x=x, q=q, submethod=mode), VrGradViewOracleEngine)
        m1 = patch_cond(LCGP(y=y, x=x, q=q, submethod=mode, process_group=solo), VrGradViewOracleEngine)
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
            xc[5] = xn[1]
        r = 2 if mode == 'rep' else 1
        v2, v1 = m2.condition(xn, yn), m1.condition(xn, yn)
        assert len(m2._local_ks) < q and len(m1._local_ks) == q
        for latent in (False, True):
            for ref in (xr, None):
                a = v2.variance_reduction_grad(xc, x_ref=ref, replicates=r, latent=latent)
                b = v1.variance_reduction_grad(xc, x_ref=ref, replicates=r, latent=latent)
                for s, t in zip(a, b):
                    assert np.array_equal(s.numpy(), t.numpy()), (rank, mode, latent)
        assert v2.variance_reduction_grad(xc, latent=True)[1].shape == (q, 8, 2)
        t2 = torch.tensor(xc, requires_grad=True)
        t1 = torch.tensor(xc, requires_grad=True)
        (g2,) = torch.autograd.grad(v2.variance_reduction_differentiable(t2, x_ref=xr, replicates=r).sum(), t2)
        (g1,) = torch.autograd.grad(v1.variance_reduction_differentiable(t1, x_ref=xr, replicates=r).sum(), t1)
        assert np.array_equal(g2.numpy(), g1.numpy()), (rank, mode)
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(23, 30, 2, 3, 1)
    m = patch_cond(LCGP(y=y, x=x, q=1), VrGradViewOracleEngine)
    view = m.condition(np.asarray(x)[:5] + 0.01, np.asarray(y)[:, :5])
    xc = np.asarray(x)[:6] + 0.02
    gain, dgain = view.variance_reduction_grad(xc)
    assert tuple(gain.shape) == (3, 6) and tuple(dgain.shape) == (3, 6, 2)
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
