"""Worker of tests/test_gpu_sobol_subsets.py::test_two_ranks_equal_one_rank_bitwise: one rank of a 2-rank gloo job in which both
ranks drive the same GPU (component k -> rank k mod 2, pair r -> rank r mod 2).  Every rank also builds the same model on a
one-rank group of its own, which holds all components and computes every pair, and compares sobol_subsets, sobol_indices(order=2)
and shapley_effects bit for bit, on the model and on a conditioned view."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402

SUBSETS = ("closed_variance", "closed", "variance", "mean", "expected_closed_variance", "closed_expected", "expected_variance")
SHAPLEY = ("effects", "shares", "variance", "effects_expected", "shares_expected", "expected_variance")
SECOND = ("first", "total", "variance", "second", "second_variance", "expected_second_variance", "second_expected")


def same(a, b, names, what):
    for name in names:
        s, t = getattr(a, name).numpy(), getattr(b, name).numpy()
        assert np.array_equal(s, t, equal_nan=True), (what, name, np.nanmax(np.abs(s - t)))


def main():
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
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
        box = np.stack([np.full(d, 0.2), np.full(d, 0.85)])
        subsets = [(0, 1), (), (d - 1,), tuple(range(d - 1, -1, -1))]
        rng = np.random.default_rng(5)
        xn = 0.1 + 0.8 * rng.random((6, d))
        yn = rng.standard_normal((4, 6))
        for who, a, b in (("model", m1, m2), ("view", m1.condition(xn, yn), m2.condition(xn, yn))):
            for latent in (False, True):
                what = (rank, mode, who, latent)
                sa, sb = (t.sobol_subsets(subsets, box=box, latent=latent, uncertainty=True) for t in (a, b))
                assert sa.closed_variance.shape == ((q if latent else 4), 4)
                same(sa, sb, SUBSETS, what)
                same(a.shapley_effects(box=box, latent=latent, uncertainty=True),
                     b.shapley_effects(box=box, latent=latent, uncertainty=True), SHAPLEY, what)
                same(a.sobol_indices(box=box, latent=latent, uncertainty=True, order=2),
                     b.sobol_indices(box=box, latent=latent, uncertainty=True, order=2), SECOND, what)
                assert np.all(sa.variance.numpy() > 0) and np.all(sa.closed_variance.numpy()[:, 1] == 0.0)
        assert len(m2._local_ks) == len(range(rank, q, world)) and len(m1._local_ks) == q
    # q < world: rank 1 holds no component, computes no pair and still takes part in the gather and the reductions
    x, y = synth.make_full(93, 100, 2, 3, 1)
    m = LCGP(y=y, x=x, q=1, device="cuda:0")
    s = m.shapley_effects(uncertainty=True)
    assert s.effects.shape == (3, 2) and np.all(np.isfinite(s.effects.numpy())) and np.all(s.variance.numpy() > 0)
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
