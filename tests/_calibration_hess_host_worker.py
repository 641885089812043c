"""Worker of tests/test_calibration_hess_host.py::test_two_ranks_gather_what_one_rank_computes: one rank of a world_size-2 gloo
job (CPU).  The latents are answered by the numpy stand-in of test_condition_hess_host and the rows by calib_hess_ref; what is
under test is the single reduction that gathers blocks, Jacobians and packed Hessians of all components for the calibration
target's second-order mode, of the model and of a view, and a rank without components taking part in the collectives."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcgp_amd import LCGP, synth  # noqa: E402
from oracle import lcgp_oracle as orc  # noqa: E402
from tests import calib_hess_ref as href  # noqa: E402
from tests import calib_ref as ref  # noqa: E402
from tests.test_condition_hess_host import CondHessOracleEngine  # noqa: E402
from tests.test_condition_host import patch_cond  # noqa: E402
from tests.test_predict_hess_host import HessOracleEngine  # noqa: E402


class Engine(CondHessOracleEngine):
    """the view's stand-in, answering the base model's second-order block too"""
    _all = HessOracleEngine._all
    predict_hess_block = HessOracleEngine.predict_hess_block


def _cpu(args):
    return [t.cpu() if isinstance(t, torch.Tensor) else t for t in args]


def _stubs(m):
    m._calib_rows_device = lambda *a: ref.rows_as_host_stub(*_cpu(a))
    m._calib_hess_rows_device = lambda *a: href.rows2_as_host_stub(*_cpu(a))
    return m


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    solo = [dist.new_group([r]) for r in range(world)][rank]
    rng = np.random.default_rng(3)
    for mode, q, maker in (("full", 3, lambda: synth.make_full(21, 40, 2, 4, 3)),
                           ("rep", 4, lambda: synth.make_rep(22, 15, 3, 2, 4, 4))):
        x, y = maker()
        m2 = _stubs(patch_cond(LCGP(y=y, x=x, q=q, submethod=mode, kernel='se', device='cpu'), Engine))
        m1 = _stubs(patch_cond(LCGP(y=y, x=x, q=q, submethod=mode, kernel='se', process_group=solo, device='cpu'), Engine))
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
        y_obs = np.asarray(y)[:, 3] + 0.05
        # the model's target, then a view's
        for t2, t1 in ((m2.calibration(y_obs, 0.2), m1.calibration(y_obs, 0.2)),
                       (m2.condition(xn, yn).calibration(y_obs, 0.2), m1.condition(xn, yn).calibration(y_obs, 0.2))):
            res2, res1 = t2.loglik_hess(x0, latent=True), t1.loglik_hess(x0, latent=True)
            assert len(res2) == 6 and res2[2].shape == (7, 2, 2) and res2[5].shape == (7, q, q)
            for a, b in zip(res2, res1):
                assert np.array_equal(a.numpy(), b.numpy()), (rank, mode)
            for a, b in zip(res2[:2], t2.loglik_grad(x0)):
                assert np.array_equal(a.numpy(), b.numpy()), (rank, mode)
        assert len(m2._local_ks) < q and len(m1._local_ks) == q
    # q < world: rank 1 holds no component and still takes part in every collective
    x, y = synth.make_full(23, 30, 2, 3, 1)
    m = _stubs(patch_cond(LCGP(y=y, x=x, q=1, kernel='se', device='cpu'), Engine))
    x0 = np.asarray(x)[:6] + 0.02
    assert tuple(m.calibration(np.asarray(y)[:, 1], 0.1).loglik_hess(x0)[2].shape) == (6, 2, 2)
    view = m.condition(np.asarray(x)[:5] + 0.01, np.asarray(y)[:, :5])
    assert tuple(view.calibration(np.asarray(y)[:, 1], 0.1).loglik_hess(x0)[2].shape) == (6, 2, 2)
    assert (m._engine is None) == (rank == 1) and (view._state is None) == (rank == 1)
    dist.barrier()
    dist.destroy_process_group()
    print("RANK %d OK" % rank)


if __name__ == "__main__":
    main()
