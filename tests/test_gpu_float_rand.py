"""Domain randomisation of the floating-base env (mw_floatenv_randomize: pushes
on the base and per-world ground friction sampled on the device) and the
per-world ground friction of the simulator (mw_set_ground_friction).

The yardstick is the one of test_gpu_float_env.py: a host-commanded twin
Simulator on the same GPU, given the wrenches (Simulator.apply_world_wrench),
friction coefficients (Simulator.set_ground_friction) and resets the env
reports, must end with a bit-identical mw_get_state record.  The draws are
restated on the host from the oracle's Philox4x32-10 (oracle.philox_raw) with
the uniform mapping of test_gpu_float_env._reset_ref; the device may fuse
lo + (hi - lo) t into one fma, and each of the fused and unfused float32 forms
is within 1.5 ulp at the magnitude |hi - lo|, hence the bound
4 * 2^-23 * (hi - lo) between the two."""

import ctypes

import numpy as np
import pytest

from float_env_harness import EPISODE_BLOCK, FREE, PUSH, STAND, _make, _philox, _reset_twin, _twin, _unif32

pytestmark = pytest.mark.gpu

PUSH_BLOCK = 0x80000000


def _phase(oracle, seed, world, episode, interval):
    return int(_philox(oracle, seed, world, episode, EPISODE_BLOCK)[0]) % interval


def _u(word, lo, hi):
    return float(_unif32(np.array([word], np.uint32), lo, hi)[0])


def _push_ref(oracle, seed, world, episode, t, interval, steps, force, torque):
    """The wrench of step t (steps already taken) of the episode, or None where no push is active."""
    s = t + _phase(oracle, seed, world, episode, interval)
    if s % interval >= steps:
        return None
    r = _philox(oracle, seed, world, episode, PUSH_BLOCK | (s // interval))
    return np.array([_u(r[0], -force, force), _u(r[1], -force, force), 0, 0, 0, _u(r[2], -torque, torque)])


def _friction_ref(oracle, seed, world, episode, lo, hi):
    return _u(_philox(oracle, seed, world, episode, EPISODE_BLOCK)[1], lo, hi)


def _push_parity(env, twin, plain, actions_of, steps, target):
    """env (pushes on) and twin in lockstep, the twin given the env's reported
    wrench of every step for all worlds (zero rows too: both sides take the
    wrench path); plain: an env without pushes under the same actions.
    Returns the [steps, W] mask of pushed steps."""
    import torch
    obs = env.reset().cpu().numpy()
    np.testing.assert_array_equal(plain.reset().cpu().numpy(), obs)
    _reset_twin(twin, obs)
    twin.run(paused=True)
    np.testing.assert_array_equal(env.sim.get_state(), twin.get_state())
    duration = env.sim.steps_per_run * env.sim.step_size
    pushed = np.zeros((steps, env.n_worlds), bool)
    for k in range(steps):
        a = actions_of(k)
        a_dev = torch.from_numpy(a).to(env.device)
        _, _, d, info = env.step(a_dev)
        plain.step(a_dev)
        push = info["push"].cpu().numpy()
        assert info["push"] is env.push and push.shape == (env.n_worlds, 6)
        np.testing.assert_array_equal(push[:, 2:5], 0.0)
        pushed[k] = (push != 0).any(axis=1)
        twin.apply_world_wrench(-1, push.astype(np.float64), duration)
        twin.set(target, a.astype(np.float64))
        twin.run()
        if k % 10 == 9 or k == steps - 1:
            np.testing.assert_array_equal(env.sim.get_state(), twin.get_state(),
                                          err_msg=f"state records differ after step {k + 1}")
            assert not d.cpu().numpy().any()
    assert not np.array_equal(env.sim.get_state(), plain.sim.get_state())   # the pushes moved the robots
    return pushed


def _first_push(pushed):
    """Per world: the first pushed step that follows an unpushed one or opens the episode."""
    start = pushed & ~np.vstack([np.zeros((1, pushed.shape[1]), bool), pushed[:-1]])
    assert start.any(axis=0).all()
    return start.argmax(axis=0)


def test_push_parity_torque_quadruped(require_gpu):
    """W = 70: two tiles, the second partial; the wrench array has 9 nodes."""
    W, seed, steps = 70, 11, 100
    kw = dict(action_mode="torque", home_base=(0, 0, 0.47, 1, 0, 0, 0), max_episode_steps=0, pid_gains=None,
              seed=seed, **FREE)
    env = _make("quadruped", W, **kw, **PUSH)
    plain = _make("quadruped", W, **kw)
    twin = _twin(env, "quadruped")
    acts = np.random.default_rng(3).uniform(-5, 5, (steps, W, 8)).astype(np.float32)
    pushed = _push_parity(env, twin, plain, lambda k: acts[k], steps, "force_target")
    first = _first_push(pushed)
    print(f"quadruped: {int(pushed.sum())} pushed world-steps of {pushed.size}, "
          f"{len(set(first.tolist()))} distinct phases")
    # 2 of every 7 steps of every world, whatever its phase
    assert abs(int(pushed.sum()) - steps * W * 2 // 7) <= 2 * W
    assert len(set(first.tolist())) >= 5
    for x in (env, plain, twin):
        x.close()


def test_push_parity_position_icub(require_gpu, oracle):
    """The <32> instance of the wave kernel: 33 wrench nodes, node 0 written.
    The seed is the first whose five worlds start at five different phases
    (by the oracle's Philox, not by the device's answer)."""
    W, steps, interval = 5, 60, PUSH["push_interval"]
    seed = next(s for s in range(1, 10000)
                if len({max(_phase(oracle, s, w, 0, interval), PUSH["push_steps"] - 1) for w in range(W)}) == W)
    from mwstep.models import icub_pid_gains
    kw = dict(max_episode_steps=0, seed=seed, **FREE)
    env = _make("icub", W, **kw, **PUSH)
    plain = _make("icub", W, **kw)
    gains = [[p, 0.0, d, -80.0, 80.0, 0.0, 0.0, -1.0] for p, d in icub_pid_gains(env.sim.joint_names)]
    twin = _twin(env, "icub", gains)
    rng = np.random.default_rng(5)
    acts = (env.home_q + rng.uniform(-0.1, 0.1, (steps, W, 32))).astype(np.float32)
    pushed = _push_parity(env, twin, plain, lambda k: acts[k], steps, "position_target")
    first = _first_push(pushed)
    print(f"iCub (seed {seed}): {int(pushed.sum())} pushed world-steps of {pushed.size}, first pushes {first.tolist()}")
    assert pushed.any() and len(set(first.tolist())) >= 5
    # a push is under way at t = 0 where phase < push_steps, else the first starts at t = interval - phase
    for w in range(W):
        ph = _phase(oracle, seed, w, 0, interval)
        assert first[w] == (0 if ph < PUSH["push_steps"] else interval - ph)
    for x in (env, plain, twin):
        x.close()


def test_draw_restatement(require_gpu, oracle):
    import torch
    W, seed, H, steps = 70, 21, 20, 65
    lo, hi = 0.3, 1.2
    F, T = PUSH["push_force"], PUSH["push_torque"]
    kw = dict(action_mode="torque", pid_gains=None, seed=seed, max_episode_steps=H, friction_range=(lo, hi),
              **FREE, **PUSH)
    env = _make("quadruped", W, **kw)
    part = _make("quadruped", 35, world_offset=35, **kw)
    env.reset()
    part.reset()
    tol_f, tol_t, tol_mu = (4 * 2.0 ** -23 * span for span in (2 * F, 2 * T, hi - lo))
    worlds = list(range(0, W, 7))
    zero, zero_part = (torch.zeros((n, 8), dtype=torch.float32, device=env.device) for n in (W, 35))

    def check_friction(episode):
        mu = env.friction.cpu().numpy()
        np.testing.assert_array_equal(part.friction.cpu().numpy(), mu[35:])
        np.testing.assert_array_equal(env.sim.ground_friction(), mu.astype(np.float64))
        assert mu.min() >= lo - tol_mu and mu.max() <= hi + tol_mu and len(set(mu.tolist())) > W // 2
        return max(abs(float(mu[w]) - _friction_ref(oracle, seed, w, episode, lo, hi)) for w in worlds)

    worst = {"force": 0.0, "torque": 0.0, "mu": check_friction(0)}
    n_pushed = 0
    for i in range(steps):
        episode, t = divmod(i, H)
        _, _, d, info = env.step(zero)
        part.step(zero_part)
        assert bool(d.all()) == (t == H - 1) and bool(d.any()) == (t == H - 1)
        push = env.push.cpu().numpy()
        np.testing.assert_array_equal(part.push.cpu().numpy(), push[35:])
        for w in worlds:
            ref = _push_ref(oracle, seed, w, episode, t, PUSH["push_interval"], PUSH["push_steps"], F, T)
            if ref is None:
                np.testing.assert_array_equal(push[w], 0.0, err_msg=f"world {w} step {i}")
                continue
            n_pushed += 1
            np.testing.assert_array_equal(push[w, 2:5], 0.0)
            worst["force"] = max(worst["force"], float(np.abs(push[w, :2] - ref[:2]).max()))
            worst["torque"] = max(worst["torque"], abs(float(push[w, 5]) - ref[5]))
        # the post launch has already drawn the friction of the episode a done step starts
        worst["mu"] = max(worst["mu"], check_friction((i + 1) // H))
        assert info["friction"] is env.friction
    print(f"draw restatement, {len(worlds)} worlds x {steps} steps ({n_pushed} pushed): "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + f"; bounds {tol_f:.2e} {tol_t:.2e} {tol_mu:.2e}")
    assert n_pushed >= len(worlds) * steps // 7
    assert worst["force"] <= tol_f and worst["torque"] <= tol_t and worst["mu"] <= tol_mu
    env.close()
    part.close()


def test_zero_push_is_no_push(require_gpu):
    """A zero wrench only adds +-0 to the bias accumulators of the run kernel."""
    import torch
    W, steps = 70, 50
    kw = dict(action_mode="torque", home_base=(0, 0, 0.47, 1, 0, 0, 0), max_episode_steps=0, pid_gains=None, **FREE)
    env = _make("quadruped", W, push_interval=7, push_steps=2, push_force=0.0, push_torque=0.0, **kw)
    plain = _make("quadruped", W, **kw)
    assert plain.push is None and plain.friction is None
    np.testing.assert_array_equal(env.reset().cpu().numpy(), plain.reset().cpu().numpy())
    rng = np.random.default_rng(13)
    for k in range(steps):
        a = torch.from_numpy(rng.uniform(-5, 5, (W, 8)).astype(np.float32)).to(env.device)
        _, _, _, info = env.step(a)
        _, _, _, plain_info = plain.step(a)
        assert set(plain_info) == {"terminal_obs"} and set(info) == {"terminal_obs", "push"}
        if k % 10 == 9:
            np.testing.assert_array_equal(env.push.cpu().numpy(), 0.0)
            np.testing.assert_array_equal(env.sim.get_state(), plain.sim.get_state(),
                                          err_msg=f"state records differ after step {k + 1}")
    env.close()
    plain.close()


def _sliding_quadruped(n_worlds):
    from mwstep import get_model_file
    from mwstep import native as N
    from mwstep.sim import Simulator
    sim = Simulator(get_model_file("quadruped"), n_worlds=n_worlds, pose=(0, 0, 0.45, 1, 0, 0, 0))
    sim.enable_contacts(True)
    sim.set_control_mode(N.MODE_FORCE)
    return sim


def _slide(sim, steps):
    """Standing pose, base velocity 1 m/s along x (the feet slide), zero torque."""
    W = sim.n_worlds
    sim.set("reset_q", np.tile(np.float64(STAND), (W, 1)))
    sim.reset_base_velocity([1.0, 0, 0, 0, 0, 0])
    sim.run(paused=True)
    for _ in range(steps):
        sim.run()
    return sim.get_state()


def test_per_world_friction_reaches_the_kernel(require_gpu):
    mus = [0.2, 0.5, 0.8, 1.1]
    many = _sliding_quadruped(4)
    assert many.float_kernel() == 2
    many.set_ground_plane(True, 1.0)
    np.testing.assert_array_equal(many.ground_friction(), 1.0)
    many.set_ground_friction(mus)
    as_f32 = np.float32(mus).astype(np.float64)
    np.testing.assert_array_equal(many.ground_friction(), as_f32)
    np.testing.assert_array_equal(many.ground_friction(1, 2), as_f32[1:3])
    rec = _slide(many, 150)
    x = many.base_pose()[:, 0]
    for w, mu in enumerate(mus):
        one = _sliding_quadruped(1)
        one.set_ground_plane(True, mu)
        np.testing.assert_array_equal(one.ground_friction(), as_f32[w:w + 1])
        np.testing.assert_array_equal(rec[w], _slide(one, 150)[0], err_msg=f"world {w}, mu {mu}")
        one.close()
    print(f"base x after 150 steps at mu {mus}: {x.tolist()}")
    assert len(set(x.tolist())) == 4
    assert many.contacts(0).shape[0] > 0                         # the feet are on the ground
    # one world of the range, then the old setter: every world again
    many.set_ground_friction(0.05, w0=2, nw=1)
    np.testing.assert_array_equal(many.ground_friction(), np.float32([0.2, 0.5, 0.05, 1.1]).astype(np.float64))
    many.set_ground_plane(True, 0.7)
    np.testing.assert_array_equal(many.ground_friction(), np.float64(np.float32(0.7)))
    with pytest.raises(RuntimeError, match="friction coefficient must be >= 0"):
        many.set_ground_friction([0.1, -0.1], w0=0, nw=2)
    with pytest.raises(RuntimeError, match="world range out of bounds"):
        many.set_ground_friction([0.1, 0.1], w0=3, nw=2)
    np.testing.assert_array_equal(many.ground_friction(), np.float64(np.float32(0.7)))
    many.close()
    # a fixed-base chain is not on the world-per-wavefront kernel
    from mwstep import get_model_file
    from mwstep.sim import Simulator
    cart = Simulator(get_model_file("cartpole"), n_worlds=2)
    with pytest.raises(RuntimeError, match="needs the world-per-wavefront kernel"):
        cart.set_ground_friction([0.5, 0.5])
    cart.close()


def test_friction_in_the_env(require_gpu):
    import torch
    W, H, steps = 70, 15, 40
    env = _make("quadruped", W, action_mode="torque", home_base=(0, 0, 0.47, 1, 0, 0, 0), pid_gains=None, seed=5,
                max_episode_steps=H, friction_range=(0.3, 1.2), joint_noise=0.05, **FREE)
    assert env.push is None
    twin = _twin(env, "quadruped")
    obs = env.reset().cpu().numpy()
    mu = env.friction.cpu().numpy()
    assert 0.3 <= mu.min() and mu.max() <= 1.2 and len(set(mu.tolist())) > W // 2
    twin.set_ground_friction(mu.astype(np.float64))
    _reset_twin(twin, obs)
    twin.run(paused=True)
    np.testing.assert_array_equal(env.sim.get_state(), twin.get_state())
    rng = np.random.default_rng(17)
    n_done = 0
    for k in range(1, steps + 1):
        a = rng.uniform(-5, 5, (W, 8)).astype(np.float32)
        o, _, d, info = env.step(torch.from_numpy(a).to(env.device))
        twin.set("force_target", a.astype(np.float64))
        twin.run()
        np.testing.assert_array_equal(env.sim.get_state(), twin.get_state(), err_msg=f"state after step {k}")
        d = d.cpu().numpy().astype(bool)
        assert d.all() == (k % H == 0) and d.any() == (k % H == 0)
        new = info["friction"].cpu().numpy()
        np.testing.assert_array_equal(new != mu, d, err_msg=f"friction changes at step {k}")
        np.testing.assert_array_equal(env.sim.ground_friction(), new.astype(np.float64))
        if d.any():
            n_done += 1
            assert 0.3 <= new.min() and new.max() <= 1.2
            mu = new
            twin.set_ground_friction(mu.astype(np.float64))
            _reset_twin(twin, o.cpu().numpy(), np.flatnonzero(d))
    assert n_done == steps // H
    env.close()
    twin.close()


def test_graph_capture_with_randomisation(require_gpu):
    """One captured step with pushes and friction on: ten replays are ten eager steps."""
    import torch
    W, K = 70, 10
    kw = dict(joint_noise=0.05, seed=4, max_episode_steps=4, friction_range=(0.3, 1.2), **FREE, **PUSH)
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
        n_pushed = n_done = 0
        for k in range(K):
            a.copy_(torch.from_numpy(acts[k + 1]).to(env.device))
            graph.replay()
            side.synchronize()
            plain.step(torch.from_numpy(acts[k + 1]).to(plain.device))
            np.testing.assert_array_equal(env.sim.get_state(), plain.sim.get_state(), err_msg=f"replay {k + 1}")
            np.testing.assert_array_equal(env.push.cpu().numpy(), plain.push.cpu().numpy())
            np.testing.assert_array_equal(env.friction.cpu().numpy(), plain.friction.cpu().numpy())
            np.testing.assert_array_equal(env.obs.cpu().numpy(), plain.obs.cpu().numpy())
            n_pushed += int((env.push != 0).any(dim=1).sum())
            n_done += int(env.done.sum())
    assert n_pushed > 0 and n_done == 2 * W          # steps 4 and 8 of 11 end an episode
    env.close()
    plain.close()


def test_errors(require_gpu):
    from mwstep import native as N
    from mwstep.vecenv import VecEnv
    L = N.lib()
    with pytest.raises(RuntimeError, match=r"push_steps must be in \[1, push_interval\]"):
        _make("quadruped", 4, push_interval=3, push_steps=4)
    with pytest.raises(RuntimeError, match="0 <= friction_lo <= friction_hi"):
        _make("quadruped", 4, friction_range=(0.9, 0.5))
    env = _make("quadruped", 4)
    bad = [N.MwFloatRandConfig(3, 4, 1.0, 1.0, 0.0, 0.0), N.MwFloatRandConfig(3, 0, 1.0, 1.0, 0.0, 0.0),
           N.MwFloatRandConfig(-1, 1, 1.0, 1.0, 0.0, 0.0), N.MwFloatRandConfig(3, 1, -1.0, 1.0, 0.0, 0.0),
           N.MwFloatRandConfig(3, 1, 1.0, float("nan"), 0.0, 0.0), N.MwFloatRandConfig(0, 1, 0.0, 0.0, 0.9, 0.5),
           N.MwFloatRandConfig(0, 1, 0.0, 0.0, -0.1, 0.5)]
    for cfg in bad:
        assert L.mw_floatenv_randomize(env._h, ctypes.byref(cfg), None, None) == N.MW_EINVAL
    # the refused calls left the env without randomisation: the host setters of its simulator work
    env.sim.apply_world_wrench(-1, np.zeros(6), 1e-3)
    env.sim.set_ground_friction(0.9)
    good = N.MwFloatRandConfig(7, 2, 30.0, 5.0, 0.3, 1.2)
    env.reset()
    assert L.mw_floatenv_randomize(env._h, ctypes.byref(good), None, None) == N.MW_ESTATE
    assert "before the first mw_vecenv_reset" in N.last_error()
    env.close()
    cart = VecEnv("CartPoleDiscreteBalancing", n_worlds=4)
    assert L.mw_floatenv_randomize(cart._h, ctypes.byref(good), None, None) == N.MW_ESTATE
    assert "mw_floatenv_create" in N.last_error()
    cart.close()
    # null output buffers are allowed; the env owns the wrench buffer and the friction array
    env = _make("quadruped", 4)
    assert L.mw_floatenv_randomize(env._h, ctypes.byref(good), None, None) == N.MW_OK
    sim = env.sim
    env.reset()
    with pytest.raises(RuntimeError, match="a floating-base env with pushes owns"):
        sim.apply_world_wrench(-1, np.zeros(6), 1e-3)
    with pytest.raises(RuntimeError, match="a floating-base env with friction randomisation owns"):
        sim.set_ground_friction(0.5)
    with pytest.raises(RuntimeError, match="a floating-base env with friction randomisation owns"):
        sim.set_ground_plane(True, 0.5)
    mu = sim.ground_friction()
    assert 0.3 <= mu.min() and mu.max() <= 1.2 and len(set(mu.tolist())) == 4
    # ... and both work again once the env is gone; the coefficients stay
    h, env._h = env._h, None
    L.mw_vecenv_destroy(h)
    np.testing.assert_array_equal(sim.ground_friction(), mu)
    sim.apply_world_wrench(-1, [1.0, 0, 0, 0, 0, 0], 1e-3)
    sim.set_ground_friction(0.5, w0=1, nw=1)
    assert sim.ground_friction()[1] == 0.5 and sim.ground_friction()[0] == mu[0]
    sim.run()
    env.close()
