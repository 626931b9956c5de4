"""Joint randomisation of the floating-base env (mw_floatenv_joints: per-world
damping, friction and effort limit of the joints drawn on the device into the
simulator's per-world records).

The yardstick of the parity tests is the one of test_gpu_float_inertia_env.py:
a host-commanded twin Simulator given what the env reports -- here also
env.joint_dynamics[w] through Simulator.set_joint_dynamics at every reset --
must end with a bit-identical mw_get_state record.  The draws are restated on
the host from the oracle's Philox4x32-10 within the fused / unfused rounding
bound of U(lo, hi), 4 * 2^-23 * (hi - lo) (test_gpu_float_rand.py), and the
three words from the reported draws bit for bit by the host build of the
kernel's word function (tests/host_float_joints/harness.cpp)."""

import ctypes

import numpy as np
import pytest

from float_env_harness import (FREE, JOINTS, LOCO, PUSH, STAND, _captured_step_graph, _check_draws, _make, _nominal,
                               _parity, _twin)
from float_joints_ref import build_harness

pytestmark = pytest.mark.gpu

INERTIA = dict(mass_scale_range=(0.8, 1.25), payload_range=(0.0, 5.0), payload_box=(0.1, 0.08, 0.05))
ICUB_LEGS = [f"{s}_{j}" for s in ("l", "r")
             for j in ("hip_pitch", "hip_roll", "hip_yaw", "knee", "ankle_pitch", "ankle_roll")]


@pytest.fixture(scope="module")
def fj(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("fj"))


@pytest.mark.parametrize("W", [1, 63, 65, 130])
def test_tile_edges_quadruped(require_gpu, oracle, fj, W):
    """The 64-world tile of the env kernels and its edges; joints 2 and 5 are
    outside the mask.  Episode 0 at reset(), episode 1 after three steps."""
    import torch
    seed, H = 23, 3
    dofs = [0, 1, 3, 4, 6, 7]
    env = _make("quadruped", W, action_mode="torque", pid_gains=None, seed=seed, max_episode_steps=H,
                joint_rand_dofs=dofs, **FREE, **JOINTS)
    nominal = _nominal(env.sim)
    np.testing.assert_array_equal(nominal, np.tile(np.float32([0.0, 0.0, 60.0]), (8, 1)))
    np.testing.assert_array_equal(env.joint_dynamics.cpu().numpy(), np.tile(nominal, (W, 1, 1)))
    env.reset()
    worlds = sorted({0, W // 2, W - 1, min(W - 1, 63), min(W - 1, 64)})
    worst = [_check_draws(env, oracle, fj, seed, 0, dofs, nominal, worlds)]
    first = env.joint_dynamics.cpu().numpy().copy()
    zero = torch.zeros((W, 8), dtype=torch.float32, device=env.device)
    for k in range(H):
        _, _, d, info = env.step(zero)
        assert bool(d.all()) == (k == H - 1)
        assert info["joint_dynamics"] is env.joint_dynamics and info["joint_draws"] is env.joint_draws
    worst.append(_check_draws(env, oracle, fj, seed, 1, dofs, nominal, worlds))
    second = env.joint_dynamics.cpu().numpy()
    assert all(not np.array_equal(first[w, dofs], second[w, dofs]) for w in range(W))
    if W > 1:
        assert len(np.unique(second[:, dofs, 1])) > 0.9 * W * len(dofs)       # differ across worlds and joints
    print(f"quadruped x{W}: worst draw error / bound {max(worst):.3f}")
    assert env.sim.constraint_overflow() == 0
    env.close()


@pytest.mark.parametrize("masked", [None, ICUB_LEGS], ids=["all", "legs"])
def test_tile_edges_icub(require_gpu, oracle, fj, masked):
    """32 joints over the four waves: every joint drawn, and the twelve leg joints only."""
    W, seed = 5, 24
    env = _make("icub", W, seed=seed, max_episode_steps=50, joint_rand_dofs=masked, **FREE, **JOINTS)
    dofs = None if masked is None else [env.sim.joint_names.index(j) for j in masked]
    sel = list(range(32)) if dofs is None else dofs
    nominal = _nominal(env.sim)
    env.reset()
    worst = _check_draws(env, oracle, fj, seed, 0, dofs, nominal, range(W))
    words = env.joint_dynamics.cpu().numpy()
    assert (words[:, sel, 2] < nominal[sel, 2]).all() and (words[:, sel, 0] > 0).any()
    print(f"icub x{W}: worst draw error / bound {worst:.3f}")
    env.close()


def test_sharding(require_gpu):
    kw = dict(action_mode="torque", pid_gains=None, seed=21, max_episode_steps=4, **FREE, **JOINTS)
    env = _make("quadruped", 70, **kw)
    part = _make("quadruped", 35, world_offset=35, **kw)
    import torch
    env.reset()
    part.reset()
    for k in range(5):
        np.testing.assert_array_equal(part.joint_dynamics.cpu().numpy(), env.joint_dynamics.cpu().numpy()[35:])
        np.testing.assert_array_equal(part.joint_draws.cpu().numpy(), env.joint_draws.cpu().numpy()[35:])
        env.step(torch.zeros((70, 8), dtype=torch.float32, device=env.device))
        part.step(torch.zeros((35, 8), dtype=torch.float32, device=part.device))
    env.close()
    part.close()


def test_twin_parity_torque_quadruped(require_gpu):
    """W = 70: two tiles of the env kernels, the second partial; episodes of 7
    steps, so the draws of every world's resets interleave with the run."""
    W, steps, H = 70, 35, 7
    kw = dict(action_mode="torque", home_base=(0, 0, 0.47, 1, 0, 0, 0), pid_gains=None, seed=11, joint_noise=0.05,
              max_episode_steps=H, action_scale=0.5, friction_range=(0.3, 1.2), **FREE, **PUSH, **LOCO, **INERTIA,
              **JOINTS)
    env = _make("quadruped", W, **kw)
    assert env.joint_dynamics.shape == (W, 8, 3) and env.joint_draws.shape == (W, 8, 3)
    twin = _twin(env, "quadruped")
    rng = np.random.default_rng(3)
    acts = rng.uniform(-40, 40, (steps + 1, W, 8)).astype(np.float32)       # 0.5 a reaches past most effort limits
    seen = _parity(env, twin, lambda k: acts[k], steps, H,
                   lambda t, a: t.set("force_target", (np.float32(0.5) * a).astype(np.float64)),
                   carry=("inertial", "joint_dynamics"))["joint_dynamics"]
    eff = np.stack([s[:, :, 2] for s in seen])
    print(f"quadruped: {len(seen)} episodes, effort limit {eff.min():.2f} .. {eff.max():.2f} N m")
    assert len(np.unique(eff)) > 0.9 * eff.size                                # differ across worlds and episodes
    env.close()
    twin.close()


def test_twin_parity_position_icub(require_gpu):
    """The <32> instance, the leg joints in the mask (the row budget)."""
    from mwstep.models import icub_pid_gains
    W, steps, H = 5, 40, 20
    kw = dict(max_episode_steps=H, seed=12, action_scale=0.25, friction_range=(0.5, 1.2), joint_noise=0.02,
              joint_rand_dofs=ICUB_LEGS, **FREE, **PUSH, **LOCO, **INERTIA, **JOINTS)
    env = _make("icub", W, **kw)
    assert env.joint_dynamics.shape == (W, 32, 3)
    gains = [[p, 0.0, d, -80.0, 80.0, 0.0, 0.0, -1.0] for p, d in icub_pid_gains(env.sim.joint_names)]
    twin = _twin(env, "icub", gains)
    rng = np.random.default_rng(5)
    acts = rng.uniform(-0.4, 0.4, (steps + 1, W, 32)).astype(np.float32)
    seen = _parity(env, twin, lambda k: acts[k], steps, H,
                   lambda t, a: t.set("position_target", env.sim.get("position_target")),
                   carry=("inertial", "joint_dynamics"))["joint_dynamics"]
    assert len(seen) == 3 and not np.array_equal(seen[0], seen[1])
    env.close()
    twin.close()


def test_all_features_off_is_the_plain_env(require_gpu):
    """mw_floatenv_joints with every range (0, 0): the env as made, bit-equal to
    an env without the call over 60 steps with resets."""
    import torch
    W, steps, H = 70, 60, 7
    kw = dict(action_mode="torque", home_base=(0, 0, 0.47, 1, 0, 0, 0), pid_gains=None, seed=9, joint_noise=0.05,
              max_episode_steps=H, **FREE)
    env = _make("quadruped", W, joint_damping_range=(0.0, 0.0), joint_friction_range=(0.0, 0.0),
                effort_scale_range=(0.0, 0.0), **kw)
    plain = _make("quadruped", W, **kw)
    assert env.joint_dynamics is None and env.joint_draws is None and plain.joint_dynamics is None
    np.testing.assert_array_equal(env.reset().cpu().numpy(), plain.reset().cpu().numpy())
    rng = np.random.default_rng(13)
    n_done = 0
    for k in range(1, steps + 1):
        a = torch.from_numpy(rng.uniform(-5, 5, (W, 8)).astype(np.float32)).to(env.device)
        o, r, d, info = env.step(a)
        po, pr, pd, _ = plain.step(a)
        assert set(info) == {"terminal_obs"}
        n_done += int(d.sum())
        if k % 10 == 0 or k == steps:
            np.testing.assert_array_equal(env.sim.get_state(), plain.sim.get_state(), err_msg=f"state after step {k}")
            for x, y in ((o, po), (r, pr), (d, pd)):
                np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
    assert n_done == W * (steps // H)
    # the simulator's records are its own: the setter works
    env.sim.set_joint_dynamics(0, env.sim.joint_dynamics(0))
    env.close()
    plain.close()


def test_graph_capture_with_joints(require_gpu):
    """One captured step with the draws on: 20 replays with resets inside are 20 eager steps."""
    import torch
    W, K = 70, 20
    kw = dict(joint_noise=0.05, seed=4, max_episode_steps=6, friction_range=(0.3, 1.2), **FREE, **PUSH, **INERTIA,
              **JOINTS)
    rng = np.random.default_rng(8)
    acts = (np.float32(STAND) + rng.uniform(-0.2, 0.2, (K + 1, W, 8))).astype(np.float32)
    plain = _make("quadruped", W, **kw)
    plain.reset()
    plain.step(torch.from_numpy(acts[0]).to(plain.device))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        env = _make("quadruped", W, **kw)
        env.reset()
        a = torch.from_numpy(acts[0]).to(env.device)
        env.step(a)                                  # warm-up
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            env.step(a)
        n_done = 0
        for k in range(K):
            a.copy_(torch.from_numpy(acts[k + 1]).to(env.device))
            graph.replay()
            side.synchronize()
            plain.step(torch.from_numpy(acts[k + 1]).to(plain.device))
            np.testing.assert_array_equal(env.sim.get_state(), plain.sim.get_state(), err_msg=f"replay {k + 1}")
            np.testing.assert_array_equal(env.obs.cpu().numpy(), plain.obs.cpu().numpy())
            np.testing.assert_array_equal(env.joint_dynamics.cpu().numpy(), plain.joint_dynamics.cpu().numpy())
            n_done += int(env.done.sum())
        types, _ = _captured_step_graph(env, a)
        side.synchronize()
    assert types == [0, 0, 0], types                 # the step stays three kernel nodes
    assert n_done == 3 * W                           # steps 6, 12, 18 of 21 end an episode
    env.close()
    plain.close()


def test_ownership(require_gpu):
    """While the env lives the simulator's setters are refused and its getter
    reads the drawn words; after the destroy the getter returns the last
    episode's words and the setter works again."""
    import torch
    from mwstep import native as N
    W, H = 9, 4
    env = _make("quadruped", W, action_mode="torque", pid_gains=None, seed=5, max_episode_steps=H, **FREE, **JOINTS)
    sim = env.sim
    env.reset()
    zero = torch.zeros((W, 8), dtype=torch.float32, device=env.device)
    for _ in range(H + 1):
        env.step(zero)
    last = env.joint_dynamics.cpu().numpy()
    with pytest.raises(RuntimeError, match="a floating-base env with joint randomisation owns"):
        sim.set_joint_dynamics(0, last[:, 0])
    with pytest.raises(RuntimeError, match="a floating-base env with joint randomisation owns"):
        sim.set_link_params(0, sim.link_params(0))
    for d in range(8):
        np.testing.assert_array_equal(sim.joint_dynamics(d), last[:, d])
    cfg = N.MwFloatJointConfig(0.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0)
    assert N.lib().mw_floatenv_joints(env._h, ctypes.byref(cfg), None, None) == N.MW_ESTATE
    assert "before the first mw_vecenv_reset" in N.last_error()
    h, env._h = env._h, None
    N.lib().mw_vecenv_destroy(h)
    for d in range(8):
        np.testing.assert_array_equal(sim.joint_dynamics(d), last[:, d])   # the last episode's words
    words = last[[3, 4], 2].copy()
    words[:, 1] = np.float32(0.25)
    sim.set_joint_dynamics(2, words, worlds=[3, 4])
    np.testing.assert_array_equal(sim.joint_dynamics(2, [2, 3, 4]), np.vstack([last[2:3, 2], words]))
    sim.run()
    env.close()
