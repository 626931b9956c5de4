"""FloatVecEnv's initial-state randomisation on the 48-joint tree
(big_tree_cases.tree48): the joint-velocity draws reach the 12th Philox block
(dofs 44..47, block 0x4000034B) and the dofs beyond 32, the start rows are 109
words wide, and a host-commanded twin reset from the reset rows stays bit-equal
over a step."""

import numpy as np
import pytest

import big_tree_cases as C
import float_init_ref as R
from float_env_harness import FREE, _dev, _reset_twin, _twin

pytestmark = pytest.mark.gpu

NAME, N = "tree48", 48


def test_high_dofs_and_twin_parity(require_gpu, oracle):
    from mwstep import FloatVecEnv
    n_worlds, seed, jv = 4, 14, 0.6
    base, links = C.env_home(oracle, NAME)
    ranges = dict(pos=((0, 0), (0, 0), (0.02, 0.05)), rpy=((-0.05, 0.05), (-0.05, 0.05), (-1.0, 1.0)),
                  ang=((-0.3, 0.3), (-0.3, 0.3), (-0.3, 0.3)))
    env = FloatVecEnv(C.urdf(NAME), n_worlds, action_mode="torque", home_base=base, contact_links=links, pgs_iters=50,
                      pid_gains=None, seed=seed, joint_noise=0.05, init_pos_range=ranges["pos"],
                      init_rpy_range=ranges["rpy"], init_ang_vel_range=ranges["ang"], init_joint_vel=jv, **FREE)
    env._pgs_iters = 50
    assert env.sim.dofs == N and env.init_state.shape == (n_worlds, 13 + 2 * N)
    assert env.init_draws.shape == (n_worlds, 13 + N)
    obs = env.reset().cpu().numpy()
    state, draws = env.init_state.cpu().numpy(), env.init_draws.cpu().numpy()
    tol = R.draw_tols(N, joint_vel=jv, **ranges)
    worst = {}
    for w in range(n_worlds):
        ref = R.draws_ref(oracle, seed, w, 0, N, joint_vel=jv, **ranges)
        err = np.abs(draws[w].astype(np.float64) - ref)
        assert (err[tol == 0] == 0).all()
        for name, dofs in (("dofs 44..47", range(44, 48)), ("dofs 32..35", range(32, 36)), ("every dof", range(N))):
            idx = [13 + d for d in dofs]
            worst[name] = max(worst.get(name, 0.0), float((err[idx] / tol[idx]).max()))
        worst["base"] = max(worst.get("base", 0.0), float((err[:12][tol[:12] > 0] / tol[:12][tol[:12] > 0]).max()))
    print("tree48 init draws (error / bound): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values())
    assert (draws[:, 13 + 44:] != 0).all() and len(np.unique(draws[:, 13 + 32:])) > 0.9 * n_worlds * 16
    np.testing.assert_array_equal(state[:, 13 + N:].view(np.uint32), draws[:, 13:].view(np.uint32))
    np.testing.assert_array_equal(obs[:, :13 + 2 * N].view(np.uint32), state.view(np.uint32))
    # one twin-parity step after the reset
    twin = _twin(env, C.urdf(NAME))
    _reset_twin(twin, obs)
    twin.run(paused=True)
    np.testing.assert_array_equal(env.sim.get_state(), twin.get_state())
    a = np.random.default_rng(2).uniform(-20, 20, (n_worlds, N)).astype(np.float32)
    env.step(_dev(env, a))
    twin.set("force_target", a.astype(np.float64))
    twin.run()
    np.testing.assert_array_equal(env.sim.get_state(), twin.get_state())
    env.close()
    twin.close()
