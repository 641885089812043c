"""Worker of tests/test_gpu_calibration_hess.py::test_two_ranks_equal_one_rank_bitwise: one rank of a 2-rank gloo job in which
both ranks drive the same GPU (component k -> rank k mod 2).  Every rank also builds the same model on a one-rank group of its
own, which holds all components, and compares loglik_hess's log likelihood, gradient, Hessian, latent sensitivities and B bit
for bit, for the model's target and for a view's (the two-rank model gathers the latent blocks, Jacobians and packed Hessians
and runs the row kernels on the gathered block)."""
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
        q = ref.MODEL_CASES[name]['q']
        rng = np.random.default_rng(8)
        xn = x.min(0) + (x.max(0) - x.min(0)) * rng.uniform(0.1, 0.9, (4, 3))
        if ref.MODEL_CASES[name]['mode'] == 'rep':
            xn = np.vstack([xn, xn[:2]])
        yn = y[:, :len(xn)] + 0.1
        for t1, t2 in ((m1.calibration(y_obs, obs_var), m2.calibration(y_obs, obs_var)),
                       (m1.condition(xn, yn).calibration(y_obs, obs_var), m2.condition(xn, yn).calibration(y_obs, obs_var))):
            assert np.array_equal(t1.M, t2.M) and np.array_equal(t1.b, t2.b)
            r1, r2 = t1.loglik_hess(theta, latent=True), t2.loglik_hess(theta, latent=True)
            assert len(m2._local_ks) == len(range(rank, q, world)) and len(m1._local_ks) == q
            for a, b in zip(r1, r2):
                assert np.array_equal(a.numpy(), b.numpy()), (rank, name, np.max(np.abs(a.numpy() - b.numpy())))
            for a, b in zip(r2[:2], t2.loglik_grad(theta)):
                assert np.array_equal(a.numpy(), b.numpy())
            assert r2[2].shape == (17, 3, 3) and r2[5].shape == (17, q, q)
    # q < world: rank 1 holds no component, has no engine and still runs the row kernels on the gathered block
    x, y = synth.make_full(95, 100, 2, 3, 1)
    m = LCGP(y=y, x=x, q=1, device="cuda:0")
    tgt = m.calibration(y[:, 3], 0.01)
    ll, dll, d2ll = tgt.loglik_hess(np.random.default_rng(6).uniform(0.1, 0.9, (20, 2)))
    assert d2ll.shape == (20, 2, 2) and torch.all(torch.isfinite(d2ll))
    assert (m._engine is None) == (rank == 1)
    both = [None, None]
    dist.all_gather_object(both, ll.numpy().tobytes() + dll.numpy().tobytes() + d2ll.numpy().tobytes())
    assert both[0] == both[1]
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
