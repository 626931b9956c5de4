"""The velocity-command locomotion task of the floating-base env
(mw_floatenv_locomotion, FloatVecEnv(task="locomotion"); the LOCO_EVERY_TERM instances of
csrc/float_env_kernel.hip around the unchanged wave run).

Physics: the yardstick of test_gpu_float_env.py -- a host-commanded twin
Simulator given the scaled actions, pushes, frictions and resets the env
reports ends with a bit-identical mw_get_state record, and the first 13 + 2 n +
n_links words of every row pass _check_obs at its bounds.  New words: the
body-frame velocities are the base words of the state record bit for bit, the
last-action words the action, projected gravity within 2e-6 of fp64 from the
row's quaternion.  Reward: a numpy fp64 restatement that carries the previous
action and the air counters itself, driven by the rows the env returned
(terminal_obs for finished worlds), at 2^-23 (n + 8) sum_i |term_i| -- the
terms are a sum of at most n + 8 float32 roundings, expf's error is relative
to a value of at most its weight.  Commands: restated from the oracle's
Philox4x32-10 with float_env_harness._unif32, at 4 * 2^-23 (hi - lo) as in
test_gpu_float_rand.py (the device may fuse lo + (hi - lo) t); the zero test
compares an exact float32 and must agree exactly."""

import ctypes

import numpy as np
import pytest

from float_env_harness import (FREE, LOCO_EVERY_TERM, RANGES, STAND, _captured_step_graph, _check_obs, _link_forces,
                               _make, _philox, _reset_twin, _RewardRef, _twin, _unif32)

pytestmark = pytest.mark.gpu

CMD_BLOCK = 0xC0000000


def _check_body_velocity(rows, sl, rec, n):
    """The body-frame words are the base twist of the state record (v, then w)."""
    base = rec[:, 7 * n:7 * n + 13]
    np.testing.assert_array_equal(rows[:, sl["body_velocity"]][:, :3].astype(np.float32), base[:, 10:13])
    np.testing.assert_array_equal(rows[:, sl["body_velocity"]][:, 3:].astype(np.float32), base[:, 7:10])


def test_physics_untouched_quadruped(require_gpu):
    """W = 70: two tiles, the second partial; torque mode, action_scale 0.5 (one exact float32 multiply),
    episodes of 7 steps so that resets interleave, pushes and friction randomisation on."""
    import torch
    W, steps, H = 70, 60, 7
    kw = dict(action_mode="torque", home_base=(0, 0, 0.47, 1, 0, 0, 0), pid_gains=None, seed=11, joint_noise=0.05,
              max_episode_steps=H, action_scale=0.5, push_interval=7, push_steps=2, push_force=30.0, push_torque=5.0,
              friction_range=(0.3, 1.2), **FREE, **LOCO_EVERY_TERM)
    env = _make("quadruped", W, **kw)
    n, L = 8, 4
    assert (env.obs_dim, env.action_dim) == (25 + 3 * n + L, n) == (53, 8)
    assert [env.obs_slices[k] for k in ("base", "joints", "contacts", "gravity", "body_velocity", "command",
                                        "last_action")] == [slice(0, 13), slice(13, 29), slice(29, 33), slice(33, 36),
                                                            slice(36, 42), slice(42, 45), slice(45, 53)]
    twin = _twin(env, "quadruped")
    obs = env.reset().cpu().numpy()
    mu = env.friction.cpu().numpy()
    twin.set_ground_friction(mu.astype(np.float64))
    _reset_twin(twin, obs)
    twin.run(paused=True)
    np.testing.assert_array_equal(env.sim.get_state(), twin.get_state())
    ref = _RewardRef(env, kw)
    ref.start(obs)
    duration = env.sim.steps_per_run * env.sim.step_size
    rng = np.random.default_rng(3)
    worst_v = worst_f = 0.0
    n_done = 0
    for k in range(1, steps + 1):
        a = rng.uniform(-5, 5, (W, n)).astype(np.float32)
        o, r, d, info = env.step(torch.from_numpy(a).to(env.device))
        o, r, d = o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy().astype(bool)
        twin.apply_world_wrench(-1, info["push"].cpu().numpy().astype(np.float64), duration)
        twin.set("force_target", (np.float32(0.5) * a).astype(np.float64))
        twin.run()
        assert d.all() == (k % H == 0) and d.any() == (k % H == 0)
        rows = ref.step(a, o, info["terminal_obs"].cpu().numpy(), d, r)
        rec = env.sim.get_state()
        _check_body_velocity(rows, env.obs_slices, rec, n)
        if k % 10 == 0:
            np.testing.assert_array_equal(rec, twin.get_state(), err_msg=f"state records differ after step {k}")
            ev, ef = _check_obs(rows[:, :13 + 2 * n + L].astype(np.float32), twin, env.contact_links)
            worst_v, worst_f = max(worst_v, ev), max(worst_f, ef)
        if d.any():
            n_done += 1
            twin.set_ground_friction(info["friction"].cpu().numpy().astype(np.float64))
            _reset_twin(twin, o, np.flatnonzero(d))
    print(f"quadruped locomotion parity: velocity words {worst_v:.2e}, contact words {worst_f:.2e}, "
          f"reward error / bound {ref.worst:.3f}, {ref.touchdowns} touchdowns, {n_done} resets of all worlds")
    assert n_done == steps // H
    assert worst_v <= 2e-6 and worst_f <= 1e-5
    assert ref.worst <= 1.0
    env.close()
    twin.close()


def test_physics_untouched_icub(require_gpu):
    """The <32> instance of the wave kernel, rows of 123 words > 64 lanes; position mode, action_scale 0.25:
    the target the env wrote is home + 0.25 a within one float32 ulp, and drives the twin."""
    import torch
    from mwstep.models import icub_pid_gains
    W, steps, n, L = 5, 60, 32, 2
    kw = dict(max_episode_steps=0, action_scale=0.25, **FREE, **LOCO_EVERY_TERM)
    env = _make("icub", W, **kw)
    assert (env.obs_dim, env.action_dim) == (25 + 3 * n + L, n) == (123, 32)
    gains = [[p, 0.0, d, -80.0, 80.0, 0.0, 0.0, -1.0] for p, d in icub_pid_gains(env.sim.joint_names)]
    twin = _twin(env, "icub", gains)
    obs = env.reset().cpu().numpy()
    _reset_twin(twin, obs)
    twin.run(paused=True)
    np.testing.assert_array_equal(env.sim.get_state(), twin.get_state())
    ref = _RewardRef(env, kw)
    ref.start(obs)
    rng = np.random.default_rng(5)
    home = env.home_q.astype(np.float64)
    worst_v = worst_f = worst_ulp = 0.0
    for k in range(1, steps + 1):
        a = rng.uniform(-0.4, 0.4, (W, n)).astype(np.float32)
        o, r, d, info = env.step(torch.from_numpy(a).to(env.device))
        o, r, d = o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy().astype(bool)
        target = env.sim.get("position_target")
        exact = home + 0.25 * a.astype(np.float64)
        ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
        worst_ulp = max(worst_ulp, float((np.abs(target - exact) / ulp).max()))
        twin.set("position_target", target)
        twin.run()
        assert not d.any()
        rows = ref.step(a, o, info["terminal_obs"].cpu().numpy(), d, r)
        rec = env.sim.get_state()
        _check_body_velocity(rows, env.obs_slices, rec, n)
        np.testing.assert_array_equal(rec, twin.get_state(), err_msg=f"state records differ after step {k}")
        if k % 10 == 0:
            ev, ef = _check_obs(o[:, :13 + 2 * n + L], twin, env.contact_links)
            worst_v, worst_f = max(worst_v, ev), max(worst_f, ef)
    print(f"iCub locomotion parity: velocity words {worst_v:.2e}, contact words {worst_f:.2e}, "
          f"targets within {worst_ulp:.2f} ulp, reward error / bound {ref.worst:.3f}")
    assert worst_ulp <= 1.0
    assert worst_v <= 2e-6 and worst_f <= 1e-5
    assert ref.worst <= 1.0
    assert (o[:, 13 + 2 * n:13 + 2 * n + L] != 0).any()
    env.close()
    twin.close()


def test_air_time_touchdowns(require_gpu):
    """The quadruped dropped from z = 0.6 under zero torque and commands of v_x in [0.5, 1]: every foot
    lands after a flight.  The touchdowns are counted on the twin alone first, then paid by the env."""
    import torch
    W, steps, n = 16, 40, 8
    kw = dict(action_mode="torque", home_base=(0, 0, 0.6, 1, 0, 0, 0), pid_gains=None, seed=13, joint_noise=0.05,
              max_episode_steps=0, steps_per_run=10, **FREE, **LOCO_EVERY_TERM)
    kw.update(command_ranges=((0.5, 1.0), (0.0, 0.0), (0.0, 0.0)), cmd_zero_prob=0.0, air_time_target=0.05)
    zero = np.zeros((W, n), np.float32)
    env = _make("quadruped", W, **kw)
    obs = env.reset().cpu().numpy()
    twin = _twin(env, "quadruped")
    _reset_twin(twin, obs)
    twin.run(paused=True)
    # the scout: the twin alone, contact per link from its own getters
    air, scouted = np.zeros((W, 4), np.int64), 0
    for _ in range(steps):
        twin.set("force_target", zero.astype(np.float64))
        twin.run()
        contact = np.array([_link_forces(twin, env.contact_links, w) for w in range(W)]) > 1.0
        scouted += int((contact & (air > 0)).sum())
        air = np.where(contact, 0, air + 1)
    assert scouted >= 10, scouted
    ref = _RewardRef(env, kw)
    ref.start(obs)
    assert (np.hypot(ref.cmd[:, 0], ref.cmd[:, 1]) > 0.1).all() and (ref.cmd[:, 0] >= 0.5).all()
    a_dev = torch.from_numpy(zero).to(env.device)
    paid = 0
    for k in range(1, steps + 1):
        o, r, d, info = env.step(a_dev)
        o, r, d = o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy().astype(bool)
        assert not d.any()
        before = ref.touchdowns
        ref.step(zero, o, info["terminal_obs"].cpu().numpy(), d, r)
        paid += ref.touchdowns - before
    np.testing.assert_array_equal(env.sim.get_state(), twin.get_state())
    print(f"air time: {scouted} touchdowns scouted on the twin, {ref.touchdowns} paid by the env, "
          f"reward error / bound {ref.worst:.3f}")
    assert ref.touchdowns >= 10 and ref.touchdowns == scouted
    assert ref.worst <= 1.0
    env.close()
    twin.close()


def _command_ref(oracle, seed, world, episode, k, zero_prob, ranges=RANGES):
    """(is zero, the three words) of command k of the episode."""
    r = _philox(oracle, seed, world, episode, CMD_BLOCK | k)
    u = np.float32(np.float32(int(r[3]) >> 8) * np.float32(1.0 / 16777216.0))
    if u < np.float32(zero_prob):
        return True, np.zeros(3, np.float32)
    return False, np.array([_unif32(np.array([r[i]], np.uint32), lo, hi)[0] for i, (lo, hi) in enumerate(ranges)],
                           np.float32)


def test_command_schedule(require_gpu, oracle):
    import torch
    W, steps, H, interval, zero_prob = 70, 40, 12, 5, 0.25
    # the rows the test reads: after s steps (episode, k), and the terminal rows of every finished episode
    read = [(s // H, (s % H) // interval) for s in range(steps + 1)] + [(e, H // interval) for e in range(steps // H)]

    def qualifies(seed):
        memo = {}

        def ref(w, e, k):
            if (w, e, k) not in memo:
                memo[w, e, k] = _command_ref(oracle, seed, w, e, k, zero_prob)
            return memo[w, e, k]
        share = np.mean([ref(w, e, k)[0] for w in range(W) for e, k in read])
        own = {tuple(ref(0, e, k)[1].tolist()) for e, k in read if not ref(0, e, k)[0]}
        return 0.15 < share < 0.35 and len(own) >= 5
    seed = next(s for s in range(1, 1000) if qualifies(s))
    kw = dict(action_mode="torque", pid_gains=None, seed=seed, max_episode_steps=H, **FREE, **LOCO_EVERY_TERM)
    kw.update(cmd_interval=interval, cmd_zero_prob=zero_prob)
    env = _make("quadruped", W, **kw)
    part = _make("quadruped", 35, world_offset=35, **kw)
    sl = env.obs_slices["command"]
    tol = np.array([4 * 2.0 ** -23 * (hi - lo) for lo, hi in RANGES])
    zero, zero_part = (torch.zeros((m, 8), dtype=torch.float32, device=env.device) for m in (W, 35))
    worst, n_zero, n_rows = 0.0, 0, 0

    def check(rows, episode, k, what):
        nonlocal worst, n_zero, n_rows
        for w in range(W):
            is_zero, c = _command_ref(oracle, seed, w, episode, k, zero_prob)
            n_rows += 1
            if is_zero:
                n_zero += 1
                np.testing.assert_array_equal(rows[w], 0.0, err_msg=f"{what}: world {w}")
            else:
                err = np.abs(rows[w].astype(np.float64) - c.astype(np.float64)) / tol
                worst = max(worst, float(err.max()))

    obs = env.reset()
    assert env.command.shape == (W, 3)
    np.testing.assert_array_equal(obs.cpu().numpy()[:, sl], env.command.cpu().numpy())
    np.testing.assert_array_equal(part.reset().cpu().numpy()[:, sl], env.command.cpu().numpy()[35:])
    last = env.command.cpu().numpy().copy()
    check(last, 0, 0, "reset")
    for s in range(1, steps + 1):
        o, _, d, info = env.step(zero)
        part.step(zero_part)
        assert info["command"] is env.command
        cmd = env.command.cpu().numpy()
        np.testing.assert_array_equal(o.cpu().numpy()[:, sl], cmd)
        np.testing.assert_array_equal(part.command.cpu().numpy(), cmd[35:])
        np.testing.assert_array_equal(part.obs.cpu().numpy()[:, sl], cmd[35:])
        episode, t = divmod(s, H)
        assert bool(d.all()) == (t == 0) and bool(d.any()) == (t == 0)
        check(cmd, episode, t // interval, f"after step {s}")
        if t == 0:
            # the finished episode's last row: the command it would have had at step count H
            check(info["terminal_obs"].cpu().numpy()[:, sl], episode - 1, H // interval, f"terminal rows of step {s}")
        elif t % interval:
            np.testing.assert_array_equal(cmd, last, err_msg=f"commands moved inside an interval (step {s})")
        last = cmd.copy()
    share = n_zero / n_rows
    print(f"command schedule (seed {seed}): {n_rows} rows, zero share {share:.3f}, worst error / bound {worst:.3f}")
    assert worst <= 1.0 and 0.15 < share < 0.35
    env.close()
    part.close()


def test_default_off(require_gpu):
    import torch
    W, n, L = 70, 8, 4
    kw = dict(joint_noise=0.05, seed=4, max_episode_steps=8, w_action=0.01, w_pose=0.1, **FREE)
    env = _make("quadruped", W, task="forward", **kw)
    old = _make("quadruped", W, **kw)
    assert env.obs_dim == old.obs_dim == 13 + 2 * n + L and env.command is None
    assert set(env.obs_slices) == {"base", "joints", "contacts"}
    np.testing.assert_array_equal(env.reset().cpu().numpy(), old.reset().cpu().numpy())
    rng = np.random.default_rng(6)
    for k in range(30):
        a = torch.from_numpy((np.float32(STAND) + rng.uniform(-0.2, 0.2, (W, n))).astype(np.float32)).to(env.device)
        o, r, d, info = env.step(a)
        oo, ro, do, _ = old.step(a)
        assert set(info) == {"terminal_obs"}
        for got, want in ((o, oo), (r, ro), (d, do)):
            np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy(), err_msg=f"step {k + 1}")
        np.testing.assert_array_equal(env.sim.get_state(), old.sim.get_state())
    env.close()
    old.close()
    with pytest.raises(ValueError, match='need task="locomotion"'):
        _make("quadruped", 4, action_scale=0.5)
    with pytest.raises(ValueError, match="unknown task"):
        _make("quadruped", 4, task="hop")


def test_graph_capture(require_gpu):
    """One captured locomotion step replayed 20 times is 20 eager steps, resets included: a linear chain
    of three kernel nodes."""
    import torch
    W, K = 70, 20
    kw = dict(joint_noise=0.05, seed=4, max_episode_steps=6, **FREE, **LOCO_EVERY_TERM)
    rng = np.random.default_rng(8)
    acts = rng.uniform(-0.8, 0.8, (K + 1, W, 8)).astype(np.float32)      # around the stand: action_scale 0.25
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
            torch.cuda.synchronize()                 # plain runs on the default stream, the copies below on `side`
            for name in ("obs", "reward", "done", "terminal_obs", "command"):
                np.testing.assert_array_equal(getattr(env, name).cpu().numpy(), getattr(plain, name).cpu().numpy(),
                                              err_msg=f"{name} after replay {k + 1}")
            np.testing.assert_array_equal(env.sim.get_state(), plain.sim.get_state(), err_msg=f"replay {k + 1}")
            n_done += int(env.done.sum())
        types, edges = _captured_step_graph(env, a)
        side.synchronize()
    assert n_done == 3 * W                            # steps 6, 12 and 18 of 21 end an episode
    assert types == [0, 0, 0], types                 # hipGraphNodeTypeKernel
    succ = dict(edges)
    assert len(edges) == 2 and len(succ) == 2 and len(set(succ.values())) == 2
    head = ({0, 1, 2} - set(succ.values())).pop()
    assert len({head, succ[head], succ[succ[head]]}) == 3
    env.close()
    plain.close()


def test_errors(require_gpu):
    import torch
    from mwstep import native as N
    from mwstep.vecenv import VecEnv
    L = N.lib()

    def cfg(**kw):
        c = N.MwFloatLocoConfig()
        for i, (lo, hi) in enumerate(RANGES):
            c.cmd_lo[i], c.cmd_hi[i] = lo, hi
        c.track_sigma = 0.25
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    env = _make("quadruped", 4)
    flipped = cfg()
    flipped.cmd_hi[1] = -1.0
    bad = [flipped, cfg(cmd_interval=-1), cfg(cmd_zero_prob=-0.1), cfg(cmd_zero_prob=1.5), cfg(track_sigma=0.0),
           cfg(track_sigma=-1.0), cfg(w_lin_z=float("nan")), cfg(air_time_target=float("inf")),
           cfg(cmd_min=float("nan"))]
    for c in bad:
        assert L.mw_floatenv_locomotion(env._h, ctypes.byref(c), None) == N.MW_EINVAL
    assert L.mw_floatenv_locomotion(env._h, None, None) == N.MW_EINVAL
    bare = _make("quadruped", 4, contact_links=())
    assert L.mw_floatenv_locomotion(bare._h, ctypes.byref(cfg(w_air_time=1.0)), None) == N.MW_EINVAL
    assert "needs contact links" in N.last_error()
    bare.close()
    # the refused calls left the env as it was: the plain width, and it steps
    no = ctypes.c_int32()
    assert L.mw_vecenv_obs_dim(env._h, ctypes.byref(no)) == N.MW_OK and no.value == 33
    env.reset()
    assert L.mw_floatenv_locomotion(env._h, ctypes.byref(cfg()), None) == N.MW_ESTATE
    assert "before the first mw_vecenv_reset" in N.last_error()
    a = torch.from_numpy(np.tile(np.float32(STAND), (4, 1))).to(env.device)
    o, r, d, _ = env.step(a)
    assert o.shape == (4, 33) and np.isfinite(o.cpu().numpy()).all() and not d.any().item()
    env.close()
    cart = VecEnv("CartPoleDiscreteBalancing", n_worlds=4)
    assert L.mw_floatenv_locomotion(cart._h, ctypes.byref(cfg()), None) == N.MW_ESTATE
    assert "mw_floatenv_create" in N.last_error()
    cart.close()
    # the Python layer reports the library's message; a null command buffer is allowed
    with pytest.raises(RuntimeError, match="track_sigma must be > 0"):
        _make("quadruped", 4, task="locomotion", track_sigma=0.0)
    env = _make("quadruped", 4)
    assert L.mw_floatenv_locomotion(env._h, ctypes.byref(cfg()), None) == N.MW_OK
    assert L.mw_vecenv_obs_dim(env._h, ctypes.byref(no)) == N.MW_OK and no.value == 53
    env.close()
