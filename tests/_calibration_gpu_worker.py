"""Worker of tests/test_gpu_calibration.py::test_two_ranks_equal_one_rank_bitwise: one rank of a 2-rank gloo job in which
both ranks drive the same GPU (component k -> rank k mod 2).  Every rank also builds the same model on a one-rank group of
its own, which holds all components, and compares the calibration target's log likelihood, gradient and latent
sensitivities bit for bit (the two-rank model gathers the latent blocks and runs the row kernel on the gathered block)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from tests import calib_ref as ref  # noqa: E402


def main():
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
    for name in ('full-matern32-q3', 'rep-matern32-q17'):
        m2, x, y = ref.model_case(name)
        m1, _, _ = ref.model_case(name, group=solo)
        m1.phi = m2.phi.clone()                 # rank 0's basis, as the two-rank model holds it
        m1.g, m1.diag_D = m2.g.clone(), m2.diag_D.clone()
        theta, y_obs, obs_var = ref.case_observation(name, x, y, 'dense')
        t1, t2 = m1.calibration(y_obs, obs_var), m2.calibration(y_obs, obs_var)
        assert np.array_equal(t1.M, t2.M) and np.array_equal(t1.b, t2.b)
        q = ref.MODEL_CASES[name]['q']
        r1, r2 = t1.loglik_grad(theta, latent=True), t2.loglik_grad(theta, latent=True)
        assert len(m2._local_ks) == len(range(rank, q, world)) and len(m1._local_ks) == q
        for a, b in zip(r1, r2):
            assert np.array_equal(a.numpy(), b.numpy()), (rank, name, np.max(np.abs(a.numpy() - b.numpy())))
        assert np.array_equal(t2.loglik(theta).numpy(), r1[0].numpy())
        assert r2[1].shape == (17, 3) and r2[2].shape == (q, 17)
    # q < world: rank 1 holds no component, has no engine and still runs the row kernel on the gathered block
    x, y = synth.make_full(95, 100, 2, 3, 1)
    m = LCGP(y=y, x=x, q=1, device="cuda:0")
    tgt = m.calibration(y[:, 3], 0.01)
    ll, dll = tgt.loglik_grad(np.random.default_rng(6).uniform(0.1, 0.9, (20, 2)))
    assert ll.shape == (20,) and dll.shape == (20, 2) and torch.all(torch.isfinite(dll))
    assert (m._engine is None) == (rank == 1)
    both = [None, None]
    dist.all_gather_object(both, ll.numpy().tobytes() + dll.numpy().tobytes())
    assert both[0] == both[1]
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
