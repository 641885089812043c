"""Worker of tests/test_gpu_condition_hess.py::test_two_ranks_reproduce_one_rank_bitwise: one rank of a 2-rank gloo job in
which both ranks drive the same GPU (component k -> rank k mod 2).  Every rank also builds the same model on a one-rank group
of its own, which holds all components, and compares the views' Hessians, gradient covariances and active subspaces bit for
bit (m = 70: the single schedule of S)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402


def main():
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
    rng = np.random.default_rng(5)
    for mode, q, maker in (("full", 3, lambda: synth.make_full(81, 333, 2, 4, 3)),
                           ("rep", 4, lambda: synth.make_rep(82, 111, 3, 2, 4, 4))):
        x, y = maker()
        m2 = LCGP(y=y, x=x, q=q, submethod=mode, device="cuda:0")
        m1 = LCGP(y=y, x=x, q=q, submethod=mode, device="cuda:0", process_group=solo)
        m1.phi = m2.phi.clone()
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        u = synth.param_points(81, orc.OracleLCGP(y=y, x=x, q=q, submethod=mode).get_unconstrained())[1]
        m1._set_flat(u)
        m2._set_flat(u)
        xn = rng.uniform(0.0, 1.0, (70, 2))
        if mode == 'rep':
            xn = np.vstack([xn, xn[:20], xn[:5]])
        yn = rng.standard_normal((4, len(xn)))
        x0 = rng.uniform(0.0, 1.0, (130, 2))
        v2, v1 = m2.condition(xn, yn), m1.condition(xn, yn)
        for a, b in zip(v2.predict_hess(x0), v1.predict_hess(x0)):
            assert a.shape == (4, 130, 2, 2) and np.array_equal(a.numpy(), b.numpy()), (rank, mode)
        for latent in (True, False):
            a, b = v2.predict_grad_cov(x0, latent=latent), v1.predict_grad_cov(x0, latent=latent)
            assert np.array_equal(a.numpy(), b.numpy()), (rank, mode, latent)
        a, b = v2.active_subspace(x0), v1.active_subspace(x0)
        for name in ('matrix', 'mean_part', 'cov_part', 'activity', 'eigenvalues', 'eigenvectors'):
            assert np.array_equal(getattr(a, name).numpy(), getattr(b, name).numpy()), (rank, mode, name)
        assert len(m2._local_ks) == len(range(rank, q, world)) and len(m1._local_ks) == q
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(83, 100, 2, 3, 1)
    m = LCGP(y=y, x=x, q=1, device="cuda:0")
    view = m.condition(np.asarray(x)[:20] + 0.01, np.asarray(y)[:, :20])
    x0 = np.asarray(x)[:7] + 0.02
    assert tuple(view.predict_hess(x0)[0].shape) == (3, 7, 2, 2)
    assert tuple(view.predict_grad_cov(x0).shape) == (3, 7, 2, 2)
    assert tuple(view.active_subspace(x0).matrix.shape) == (3, 2, 2)
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
