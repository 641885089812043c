"""Worker of tests/test_condition_hess_host.py::test_two_ranks_gather_what_one_rank_computes: one rank of a world_size-2 gloo
job (CPU).  The closed form is answered by the numpy stand-in of test_condition_hess_host; what is under test is the single
reduction that gathers the view's blocks, Jacobians, Hessians and gradient covariances, and a rank without components taking
part in the collectives."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402
from tests.test_condition_hess_host import CondHessOracleEngine  # noqa: E402
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
        m2 = patch_cond(LCGP(y=y, x=x, q=q, submethod=mode, device='cpu'), CondHessOracleEngine)
        m1 = patch_cond(LCGP(y=y, x=x, q=q, submethod=mode, process_group=solo, device='cpu'), CondHessOracleEngine)
        m1.phi = m2.phi.clone()
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        u = synth.param_points(21, orc.OracleLCGP(y=y, x=x, q=q, submethod=mode).get_unconstrained())[1]
        for m in (m1, m2):
            m._set_flat(u)
        xn = rng.uniform(0, 1, (5, 2))
        if mode == 'rep':
            xn = np.vstack([xn, xn[:2]])
        yn = rng.standard_normal((4, len(xn)))
        x0 = rng.uniform(0, 1, (7, 2))
        v2, v1 = m2.condition(xn, yn), m1.condition(xn, yn)
        assert len(m2._local_ks) < q and len(m1._local_ks) == q
        for a, b in zip(v2.predict_hess(x0), v1.predict_hess(x0)):
            assert a.shape == (4, 7, 2, 2) and np.array_equal(a.numpy(), b.numpy()), (rank, mode)
        for a, b in zip(v2._latent_predict_hess(x0), v1._latent_predict_hess(x0)):
            assert np.array_equal(a, b), (rank, mode)
        for latent in (False, True):
            a, b = v2.predict_grad_cov(x0, latent=latent), v1.predict_grad_cov(x0, latent=latent)
            assert a.shape == ((q if latent else 4), 7, 2, 2) and np.array_equal(a.numpy(), b.numpy()), (rank, mode, latent)
        a, b = v2.active_subspace(x0), v1.active_subspace(x0)
        for name in ('matrix', 'mean_part', 'cov_part', 'activity', 'eigenvalues', 'eigenvectors'):
            assert np.array_equal(getattr(a, name).numpy(), getattr(b, name).numpy()), (rank, mode, name)
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(23, 30, 2, 3, 1)
    m = patch_cond(LCGP(y=y, x=x, q=1, device='cpu'), CondHessOracleEngine)
    view = m.condition(np.asarray(x)[:5] + 0.01, np.asarray(y)[:, :5])
    x0 = np.asarray(x)[:6] + 0.02
    assert tuple(view.predict_hess(x0)[0].shape) == (3, 6, 2, 2)
    assert tuple(view.predict_grad_cov(x0).shape) == (3, 6, 2, 2)
    assert tuple(view.active_subspace(x0).matrix.shape) == (3, 2, 2)
    assert (m._engine is None) == (rank == 1) and (view._state is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
