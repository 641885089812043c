"""Worker of tests/test_gpu_condition_vr_grad.py::test_two_ranks_reproduce_one_rank_bitwise: one rank of a 2-rank gloo job in
which both ranks drive the same GPU (component k -> rank k mod 2).  Every rank also builds the same model on a one-rank group
of its own, which holds all components, and compares the views' ALC gradients bit for bit."""
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
        xc, xr = rng.uniform(0.0, 1.0, (130, 2)), rng.uniform(0.0, 1.0, (130, 2))
        if mode == 'rep':
            xc[[3, 40]] = m2.x_unique.numpy()[[5, 60]]
            xc[7] = xn[2]
        r = 2 if mode == 'rep' else 1
        v2, v1 = m2.condition(xn, yn), m1.condition(xn, yn)
        for latent in (True, False):
            for ref in (xr, None):
                a = v2.variance_reduction_grad(xc, x_ref=ref, replicates=r, latent=latent)
                b = v1.variance_reduction_grad(xc, x_ref=ref, replicates=r, latent=latent)
                for s, t in zip(a, b):
                    assert np.array_equal(s.numpy(), t.numpy()), (rank, mode, latent)
        assert len(m2._local_ks) == len(range(rank, q, world)) and len(m1._local_ks) == q
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(83, 100, 2, 3, 1)
    m = LCGP(y=y, x=x, q=1, device="cuda:0")
    view = m.condition(np.asarray(x)[:20] + 0.01, np.asarray(y)[:, :20])
    xc = np.asarray(x)[:7] + 0.02
    gain, dgain = view.variance_reduction_grad(xc)
    assert tuple(gain.shape) == (3, 7) and tuple(dgain.shape) == (3, 7, 2)
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
