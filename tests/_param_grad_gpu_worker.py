"""Worker of tests/test_gpu_param_grad.py::test_two_ranks_reproduce_one_rank_bitwise: one rank of a 2-rank gloo job in which both
ranks drive the same GPU (component k -> rank k mod 2).  Every rank also builds the same model on a one-rank group of its own,
which holds all three components, and compares predict_param_grad and predict_laplace bit for bit: each component is computed
by one rank, whatever else that rank holds, and the host map runs on the gathered block."""
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
    for mode, maker in (("full", lambda: synth.make_full(7, 200, 2, 4, 3)), ("rep", lambda: synth.make_rep(7, 66, 3, 2, 4, 3))):
        x, y = maker()
        m2 = LCGP(y=y, x=x, q=3, submethod=mode, device="cuda:0")
        m1 = LCGP(y=y, x=x, q=3, submethod=mode, device="cuda:0", process_group=solo)
        m1.phi = m2.phi.clone()
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        u = synth.param_points(7, orc.OracleLCGP(y=y, x=x, q=3, submethod=mode).get_unconstrained())[1]
        m1._set_flat(u)
        m2._set_flat(u)
        x0 = x[:1] + (x[5:70] - x[:1]) * 0.37
        for kw in (dict(space="constrained"), dict(), dict(latent=True)):
            for a, b in zip(m2.predict_param_grad(x0, **kw), m1.predict_param_grad(x0, **kw)):
                assert np.array_equal(a.numpy(), b.numpy()), (rank, mode, kw)
        cov = 1e-3 * np.eye(len(u))
        for a, b in zip(m2.predict_laplace(x0, cov=cov), m1.predict_laplace(x0, cov=cov)):
            assert np.array_equal(a.numpy(), b.numpy()), (rank, mode)
        assert len(m2._local_ks) == len(range(rank, 3, world)) and len(m1._local_ks) == 3
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(83, 100, 2, 3, 1)
    m = LCGP(y=y, x=x, q=1, device="cuda:0")
    assert tuple(m.predict_param_grad(x[:9] * 0.9)[0].shape) == (3, 9, 2 + 2 + 3)
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
