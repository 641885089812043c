"""Worker of tests/test_gpu_condition_marginal.py::test_two_ranks_equal_one_rank_bitwise: one rank of a 2-rank gloo job in which
both ranks drive the same GPU (component k -> rank k mod 2).  Every rank also builds the same model on a one-rank group of its
own, which holds all components, and compares predict_marginal(cov_with=...) on the model and on a view (outputs and latent)
and main_effects(effect_var=True) bit for bit."""
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
    rng = np.random.default_rng(7)
    for mode, q, kernel, maker in (("full", 3, "matern32", lambda: synth.make_full(91, 300, 2, 4, 3)),
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
        xn = rng.uniform(0, 1, (40, 2))
        yn = rng.standard_normal((4, 40))
        x0 = np.random.default_rng(5).uniform(0, 1, (150, 2))
        mask = np.random.default_rng(6).uniform(0, 1, (150, 2)) < 0.5
        box = np.array([[0.2, 0.1], [0.7, 0.9]])
        row = (np.array([np.nan, 0.35]), [0])
        v1, v2 = m1.condition(xn, yn), m2.condition(xn, yn)
        for a1, a2 in ((m1, m2), (v1, v2)):
            for latent in (False, True):
                a = a1.predict_marginal(x0, mask, box=box, latent=latent, cov_with=row)
                b = a2.predict_marginal(x0, mask, box=box, latent=latent, cov_with=row)
                assert len(a) == 3 and a[2].shape == ((q if latent else 4), 150)
                for s, t in zip(a, b):
                    assert np.array_equal(s.numpy(), t.numpy()), (rank, mode, latent, np.max(np.abs(s.numpy() - t.numpy())))
            e1, e2 = a1.main_effects(grid=7, effect_var=True), a2.main_effects(grid=7, effect_var=True)
            for name in ("grid", "mean", "var", "overall", "overall_var", "effect", "effect_var"):
                assert np.array_equal(getattr(e1, name).numpy(), getattr(e2, name).numpy()), (rank, mode, name)
        assert len(m2._local_ks) == len(range(rank, q, world)) and len(m1._local_ks) == q
    # q < world: rank 1 holds no component and still takes part in the gather
    x, y = synth.make_full(93, 100, 2, 3, 1)
    m = LCGP(y=y, x=x, q=1, device="cuda:0")
    view = m.condition(np.asarray(x)[:5] + 0.01, np.asarray(y)[:, :5])
    me = view.main_effects(grid=5, effect_var=True)
    assert me.effect_var.shape == (3, 2, 5) and np.all(np.isfinite(me.effect_var.numpy())) and np.all(me.var.numpy() > 0)
    assert (m._engine is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
