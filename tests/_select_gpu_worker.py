"""Worker of tests/test_gpu_select_batch.py::test_two_ranks_reproduce_one_rank_bitwise: one rank of a 2-rank gloo job in which
both ranks drive the same GPU (component k -> rank k mod 2).  Every rank also builds the same model on a one-rank group of its
own, which holds all components, and compares picks, gains and every score row bit for bit."""
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
    for mode, q, maker in (("full", 3, lambda: synth.make_full(81, 300, 2, 4, 3)),
                           ("rep", 4, lambda: synth.make_rep(82, 90, 3, 2, 4, 4))):
        x, y = maker()
        m2 = LCGP(y=y, x=x, q=q, submethod=mode, device="cuda:0")
        m1 = LCGP(y=y, x=x, q=q, submethod=mode, device="cuda:0", process_group=solo)
        m1.phi = m2.phi.clone()
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        u = synth.param_points(81, orc.OracleLCGP(y=y, x=x, q=q, submethod=mode).get_unconstrained())[1]
        m1._set_flat(u)
        m2._set_flat(u)
        xn = np.asarray(x)
        xc = xn.min(axis=0) + (xn.max(axis=0) - xn.min(axis=0)) * np.random.default_rng(5).random((150, xn.shape[1]))
        if mode == 'rep':
            xc = np.vstack([xc, m1.x_unique.numpy()[:10]])
        r = 2 if mode == 'rep' else 1
        for ref in (None, xn[:77]):
            a = [t.numpy() for t in m2.select_batch(xc, 8, x_ref=ref, replicates=r, return_scores=True)]
            b = [t.numpy() for t in m1.select_batch(xc, 8, x_ref=ref, replicates=r, return_scores=True)]
            for u2, u1 in zip(a, b):
                assert np.array_equal(u2, u1), (rank, mode)
            assert len(set(a[0].tolist())) == 8
        assert len(m2._local_ks) == len(range(rank, q, world)) and len(m1._local_ks) == q
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(83, 100, 2, 3, 1)
    m = LCGP(y=y, x=x, q=1, device="cuda:0")
    idx, gain = m.select_batch(np.asarray(x)[:20] + 0.01, 5)
    assert idx.shape == (5,) and gain.shape == (5,)
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
