"""Worker of tests/test_gpu_condition_sobol.py::test_two_ranks_equal_one_rank_bitwise: one rank of a 2-rank gloo job in which
both ranks drive the same GPU (component k -> rank k mod 2, so each rank reads the A^-1 and the view state of the components it
owns).  Every rank also builds the same model on a one-rank group of its own, which holds all components, conditions both on the
same new runs and compares sobol_indices(uncertainty=True) and integrated_variance() of the two views bit for bit."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402

FIELDS = ("first", "total", "variance", "mean", "first_variance", "closed_variance", "expected_variance",
          "expected_first_variance", "expected_closed_variance", "first_expected", "total_expected", "integrated_variance")


def main():
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
    rng = np.random.default_rng(7)
    for mode, q, kernel, maker in (("full", 3, "matern32", lambda: synth.make_full(91, 150, 3, 4, 3)),
                                   ("rep", 4, "se", lambda: synth.make_rep(92, 70, 3, 2, 4, 4))):
        x, y = maker()
        m2 = LCGP(y=y, x=x, q=q, submethod=mode, kernel=kernel, device="cuda:0")
        m1 = LCGP(y=y, x=x, q=q, submethod=mode, kernel=kernel, device="cuda:0", process_group=solo)
        m1.phi = m2.phi.clone()                 # rank 0's basis, as the two-rank model holds it
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        o = orc.OracleLCGP(y=y, x=x, q=q, submethod=mode)
        u = synth.param_points(91, o.get_unconstrained())[1]
        m1._set_flat(u)
        m2._set_flat(u)
        d = np.asarray(x).shape[1]
        xn = rng.uniform(0, 1, (40, d))
        if mode == "rep":
            xn = np.vstack([xn, xn[:9]])
        yn = rng.standard_normal((4, len(xn)))
        box = np.stack([np.full(d, 0.2), np.full(d, 0.85)])
        v1, v2 = m1.condition(xn, yn), m2.condition(xn, yn)
        for latent in (False, True):
            a = v1.sobol_indices(box=box, latent=latent, uncertainty=True)
            b = v2.sobol_indices(box=box, latent=latent, uncertainty=True)
            assert a.first_expected.shape == ((q if latent else 4), d)
            for name in FIELDS:
                s, t = getattr(a, name).numpy(), getattr(b, name).numpy()
                assert np.array_equal(s, t), (rank, mode, latent, name, np.max(np.abs(s - t)))
            assert np.all(np.isfinite(a.first_expected.numpy())) and np.all(a.integrated_variance.numpy() > 0)
            iv1, iv2 = v1.integrated_variance(box=box, latent=latent).numpy(), v2.integrated_variance(box=box, latent=latent).numpy()
            assert np.array_equal(iv1, iv2) and np.array_equal(iv1, a.integrated_variance.numpy()), (rank, mode, latent)
        assert len(m2._local_ks) == len(range(rank, q, world)) and len(m1._local_ks) == q
    # q < world: rank 1 holds no component, computes nothing and still takes part in the collectives
    x, y = synth.make_full(93, 100, 2, 3, 1)
    m = LCGP(y=y, x=x, q=1, device="cuda:0")
    view = m.condition(np.asarray(x)[:5] + 0.01, np.asarray(y)[:, :5])
    s = view.sobol_indices(uncertainty=True)
    assert s.first_expected.shape == (3, 2) and np.all(np.isfinite(s.first_expected.numpy()))
    assert np.all(view.integrated_variance().numpy() > 0)
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
