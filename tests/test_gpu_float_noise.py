"""Observation noise and action latency of the floating-base env
(mw_floatenv_noise, FloatVecEnv(obs_noise=, action_delay_range=); the post
kernel's write-out and the DELAY instances of the action kernel in
csrc/float_env_kernel.hip, around the unchanged wave run).

Noise: every row of obs and terminal_obs minus its clean row is amp[k] u, u =
-1 + (x >> 8) 2^-23 restated from the oracle's Philox4x32-10 with the counter
(global world, episode, k >> 2, 1 + t) and the counters env.counters() reports,
at 2^-23 (|clean| + amp): the device forms clean + amp u in one fused
multiply-add, the restatement in fp64.  Words of amplitude zero, the command
and the last action are bit-equal to the clean words.  The clean rows, reward,
done and the simulator's state are bit-equal to an env without noise.

Latency: the yardstick of test_gpu_float_env.py -- a host-commanded twin
Simulator given the delayed commands the test computes itself (the neutral
command while t < d) ends every step with a bit-identical mw_get_state record;
the delays equal the restated draw, word 2 of the episode block.  The reward's
action terms and the last-action words follow the action just given
(float_env_harness._RewardRef, at its bound)."""

import ctypes

import numpy as np
import pytest

from float_env_harness import (FREE, LOCO_EVERY_TERM, STAND, _captured_step_graph, _check_rows, _delay_ref, _make,
                               _reset_twin, _RewardRef, _twin)

pytestmark = pytest.mark.gpu

H = 7                                                 # steps per episode: resets interleave with the steps
NOISE = dict(base_position=0.01, base_orientation=0.0, base_angular_velocity=0.05, joint_positions=0.02,
             joint_velocities=0.5, contacts=2.0, gravity=0.05, body_angular_velocity=0.1)


@pytest.mark.parametrize("kind, W, steps, spread, offset", [("quadruped", 70, 16, 0.8, 1000), ("icub", 3, 9, 0.4, 5)])
def test_noise_is_the_stated_draw(require_gpu, oracle, kind, W, steps, spread, offset):
    """Quadruped: two tiles, the second partial, rows of 53 words (the last Philox block partial).
    iCub: rows of 123 words > 64 lanes, so the word loop wraps."""
    import torch
    seed = 21
    kw = dict(joint_noise=0.05, seed=seed, max_episode_steps=H, world_offset=offset, obs_noise=NOISE, **FREE, **LOCO_EVERY_TERM)
    env = _make(kind, W, **kw)
    n, NO = env.action_dim, env.obs_dim
    assert NO == {"quadruped": 53, "icub": 123}[kind]
    amp = env.obs_noise.cpu().numpy()
    assert amp.shape == (NO,) and amp.dtype == np.float32
    for name, value in NOISE.items():
        np.testing.assert_array_equal(amp[env.noise_slices[name]], np.float32(value))
    for name in ("command", "last_action"):
        np.testing.assert_array_equal(amp[env.obs_slices[name]], 0.0)
    assert 0 < (amp != 0).sum() < NO
    everyone = np.arange(W)
    obs = env.reset().cpu().numpy()
    ep, st = (c.cpu().numpy() for c in env.counters())
    assert not ep.any() and not st.any()
    worst = _check_rows(oracle, seed, offset, amp, obs, env.clean_obs.cpu().numpy(), everyone, ep, st)
    rng = np.random.default_rng(4)
    n_done = n_moved = 0
    for k in range(1, steps + 1):
        a = rng.uniform(-spread, spread, (W, n)).astype(np.float32)
        o, r, d, info = env.step(torch.from_numpy(a).to(env.device))
        assert info["clean_obs"] is env.clean_obs and info["clean_terminal_obs"] is env.clean_terminal_obs
        o, d, clean = o.cpu().numpy(), d.cpu().numpy().astype(bool), env.clean_obs.cpu().numpy()
        last = st + 1                                  # the step count the episode would end with
        ep_before = ep
        ep, st = (c.cpu().numpy() for c in env.counters())
        worst = max(worst, _check_rows(oracle, seed, offset, amp, o, clean, everyone, ep, st))
        n_moved += int((o != clean).sum())
        assert bool(d.all()) == (k % H == 0) and bool(d.any()) == (k % H == 0)
        if d.any():
            done = np.flatnonzero(d)
            n_done += len(done)
            np.testing.assert_array_equal(ep[done], ep_before[done] + 1)
            np.testing.assert_array_equal(st[done], 0)
            worst = max(worst, _check_rows(oracle, seed, offset, amp, info["terminal_obs"].cpu().numpy(),
                                           info["clean_terminal_obs"].cpu().numpy(), done, ep_before, last))
    print(f"{kind} observation noise: worst error / bound {worst:.3f}, {n_moved} words moved, {n_done} terminal rows")
    assert worst <= 1.0
    assert n_done == W * (steps // H) > 0
    assert n_moved > 0.5 * steps * W * (amp != 0).sum()
    env.close()


def test_clean_path_is_untouched(require_gpu):
    import torch
    W, steps = 70, 16
    kw = dict(joint_noise=0.05, seed=22, max_episode_steps=H, **FREE, **LOCO_EVERY_TERM)
    env = _make("quadruped", W, obs_noise=NOISE, **kw)
    plain = _make("quadruped", W, **kw)
    assert plain.obs_noise is None and plain.clean_obs is None and plain.action_delay is None
    assert set(plain._info) == {"terminal_obs", "command"}
    env.reset()
    np.testing.assert_array_equal(env.clean_obs.cpu().numpy(), plain.reset().cpu().numpy())
    rng = np.random.default_rng(5)
    for k in range(1, steps + 1):
        a = torch.from_numpy(rng.uniform(-0.8, 0.8, (W, 8)).astype(np.float32)).to(env.device)
        o, r, d, info = env.step(a)
        op, rp, dp, infop = plain.step(a)
        d = d.cpu().numpy().astype(bool)
        for got, want, name in ((env.clean_obs, op, "clean_obs"), (r, rp, "reward"), (env.done, dp, "done"),
                                (env.command, plain.command, "command")):
            np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy(), err_msg=f"{name} after step {k}")
        np.testing.assert_array_equal(info["clean_terminal_obs"].cpu().numpy()[d],
                                      infop["terminal_obs"].cpu().numpy()[d], err_msg=f"terminal rows of step {k}")
        np.testing.assert_array_equal(env.sim.get_state(), plain.sim.get_state(), err_msg=f"state after step {k}")
        assert (o.cpu().numpy() != op.cpu().numpy()).any()
        assert bool(d.all()) == (k % H == 0)
    env.close()
    plain.close()


def test_shards_agree(require_gpu):
    import torch
    W, steps = 70, 16
    kw = dict(joint_noise=0.05, seed=23, max_episode_steps=H, obs_noise=NOISE, action_delay_range=(0, 3),
              **FREE, **LOCO_EVERY_TERM)
    env = _make("quadruped", W, **kw)
    parts = [_make("quadruped", 35, world_offset=o, **kw) for o in (0, 35)]
    obs = env.reset().cpu().numpy()
    for i, p in enumerate(parts):
        np.testing.assert_array_equal(p.reset().cpu().numpy(), obs[35 * i:35 * i + 35])
    rng = np.random.default_rng(6)
    delays = set()
    for k in range(1, steps + 1):
        a = rng.uniform(-0.8, 0.8, (W, 8)).astype(np.float32)
        env.step(torch.from_numpy(a).to(env.device))
        delays |= set(env.action_delay.cpu().numpy().tolist())
        for i, p in enumerate(parts):
            sl = slice(35 * i, 35 * i + 35)
            p.step(torch.from_numpy(a[sl].copy()).to(p.device))
            for name in ("obs", "terminal_obs", "reward", "done", "action_delay", "clean_obs"):
                np.testing.assert_array_equal(getattr(p, name).cpu().numpy(), getattr(env, name).cpu().numpy()[sl],
                                              err_msg=f"{name} of shard {i} after step {k}")
    assert delays == {0, 1, 2, 3}
    assert (env.obs.cpu().numpy() != env.clean_obs.cpu().numpy()).any()
    env.close()
    for p in parts:
        p.close()


def test_delay_torque_twin(require_gpu, oracle):
    """Quadruped, torque mode, action_scale 0.5 (one exact float32 multiply), delays 0..3: the twin receives
    0.5 a_{t-d}, zeros while t < d."""
    import torch
    W, steps, n, lo, hi = 70, 24, 8, 0, 3
    # a seed whose episodes 0..3 each show all four delays, the partial second tile more than one of them in
    # every episode (restated on the CPU)
    def qualifies(s):
        return all({_delay_ref(oracle, s, w, e, lo, hi) for w in range(W)} == {0, 1, 2, 3} and
                   len({_delay_ref(oracle, s, w, e, lo, hi) for w in range(64, W)}) > 1
                   for e in range(steps // H + 1))
    seed = next(s for s in range(1, 1000) if qualifies(s))
    kw = dict(action_mode="torque", home_base=(0, 0, 0.47, 1, 0, 0, 0), pid_gains=None, seed=seed, joint_noise=0.05,
              max_episode_steps=H, action_scale=0.5, action_delay_range=(lo, hi), **FREE, **LOCO_EVERY_TERM)
    env = _make("quadruped", W, **kw)
    twin = _twin(env, "quadruped")
    obs = env.reset().cpu().numpy()
    assert env.action_delay.dtype == torch.int32 and env.clean_obs is None
    _reset_twin(twin, obs)
    twin.run(paused=True)
    np.testing.assert_array_equal(env.sim.get_state(), twin.get_state())
    ref = _RewardRef(env, kw)
    ref.start(obs)
    episode, t = np.zeros(W, np.int64), np.zeros(W, np.int64)
    delay = env.action_delay.cpu().numpy().copy()
    np.testing.assert_array_equal(delay, [_delay_ref(oracle, seed, w, 0, lo, hi) for w in range(W)])
    history = np.zeros((H, W, n), np.float32)            # the episode's actions by step
    rng = np.random.default_rng(7)
    seen, n_neutral = set(), 0
    for k in range(1, steps + 1):
        a = rng.uniform(-5, 5, (W, n)).astype(np.float32)
        history[t, np.arange(W)] = a
        neutral = t < delay
        applied = np.where(neutral[:, None], np.float32(0), history[np.maximum(t - delay, 0), np.arange(W)])
        n_neutral += int(neutral.sum())
        seen |= set(delay.tolist())
        o, r, d, info = env.step(torch.from_numpy(a).to(env.device))
        assert info["action_delay"] is env.action_delay
        o, r, d = o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy().astype(bool)
        twin.set("force_target", (np.float32(0.5) * applied).astype(np.float64))
        twin.run()
        np.testing.assert_array_equal(env.sim.get_state(), twin.get_state(), err_msg=f"state records after step {k}")
        # sum a^2, the action rate and the last-action words: the action just given
        ref.step(a, o, info["terminal_obs"].cpu().numpy(), d, r)
        t += 1
        assert bool(d.all()) == (k % H == 0) and bool(d.any()) == (k % H == 0)
        if d.any():
            done = np.flatnonzero(d)
            _reset_twin(twin, o, done)
            episode[done] += 1
            t[done] = 0
            delay = env.action_delay.cpu().numpy().copy()
            np.testing.assert_array_equal(delay, [_delay_ref(oracle, seed, w, int(episode[w]), lo, hi)
                                                  for w in range(W)])
    print(f"delay, torque mode (seed {seed}): delays seen {sorted(seen)}, {n_neutral} neutral world-steps, "
          f"reward error / bound {ref.worst:.3f}")
    assert seen == {0, 1, 2, 3} and n_neutral > 0
    assert ref.worst <= 1.0
    env.close()
    twin.close()


def test_delay_position_icub(require_gpu):
    """iCub, position mode, a fixed delay of 2, action_scale 0.25: the targets are home_q for the first two
    steps of every episode and fmaf(0.25, a_{t-2}, home_q) afterwards, and drive the twin."""
    import torch
    from mwstep.models import icub_pid_gains
    W, steps, n = 3, 17, 32
    kw = dict(max_episode_steps=H, action_scale=0.25, joint_noise=0.02, seed=24, action_delay_range=(2, 2),
              **FREE, **LOCO_EVERY_TERM)
    env = _make("icub", W, **kw)
    gains = [[p, 0.0, d, -80.0, 80.0, 0.0, 0.0, -1.0] for p, d in icub_pid_gains(env.sim.joint_names)]
    twin = _twin(env, "icub", gains)
    obs = env.reset().cpu().numpy()
    np.testing.assert_array_equal(env.action_delay.cpu().numpy(), 2)
    _reset_twin(twin, obs)
    twin.run(paused=True)
    np.testing.assert_array_equal(env.sim.get_state(), twin.get_state())
    home = env.home_q.astype(np.float64)
    rng = np.random.default_rng(8)
    history, n_home = [], 0
    for k in range(1, steps + 1):
        a = rng.uniform(-0.4, 0.4, (W, n)).astype(np.float32)
        history.append(a)
        t = (k - 1) % H                                # steps taken in the episode before this one
        o, r, d, info = env.step(torch.from_numpy(a).to(env.device))
        target = env.sim.get("position_target")
        if t < 2:
            np.testing.assert_array_equal(target, np.tile(home, (W, 1)), err_msg=f"step {k}: t = {t} < d")
            n_home += 1
        else:
            # 0.25 a is exact and the fp64 sum of two float32 is too: one rounding, as the device's fmaf
            want = (home + 0.25 * history[-3].astype(np.float64)).astype(np.float32).astype(np.float64)
            np.testing.assert_array_equal(target, want, err_msg=f"step {k}: t = {t}")
        o, d = o.cpu().numpy(), d.cpu().numpy().astype(bool)
        np.testing.assert_array_equal(o[~d][:, env.obs_slices["last_action"]], a[~d])   # the action just given
        twin.set("position_target", target)
        twin.run()
        np.testing.assert_array_equal(env.sim.get_state(), twin.get_state(), err_msg=f"state records after step {k}")
        assert bool(d.all()) == (k % H == 0)
        if d.any():
            _reset_twin(twin, o, np.flatnonzero(d))
    assert n_home == 2 * (steps // H + 1)
    env.close()
    twin.close()


def test_zero_delay_is_the_env_without_it(require_gpu):
    import torch
    W = 70
    kw = dict(joint_noise=0.05, seed=25, max_episode_steps=H, w_action=0.01, w_pose=0.1, **FREE)
    env = _make("quadruped", W, action_delay_range=(0, 0), **kw)
    plain = _make("quadruped", W, **kw)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), plain.reset().cpu().numpy())
    rng = np.random.default_rng(9)
    for k in range(1, 13):
        a = torch.from_numpy((np.float32(STAND) + rng.uniform(-0.2, 0.2, (W, 8))).astype(np.float32)).to(env.device)
        o, r, d, info = env.step(a)
        op, rp, dp, _ = plain.step(a)
        for got, want in ((o, op), (r, rp), (d, dp), (info["terminal_obs"], plain.terminal_obs)):
            np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy(), err_msg=f"step {k}")
        np.testing.assert_array_equal(env.sim.get_state(), plain.sim.get_state(), err_msg=f"state after step {k}")
    np.testing.assert_array_equal(env.action_delay.cpu().numpy(), 0)
    env.close()
    plain.close()


def test_graph_capture(require_gpu):
    """One captured step with both features on, replayed five times, is five eager steps (a reset among them):
    still a linear chain of three kernel nodes."""
    import torch
    W, K = 70, 5
    kw = dict(joint_noise=0.05, seed=26, max_episode_steps=3, obs_noise=NOISE, action_delay_range=(0, 3),
              **FREE, **LOCO_EVERY_TERM)
    rng = np.random.default_rng(10)
    acts = rng.uniform(-0.8, 0.8, (K + 1, W, 8)).astype(np.float32)
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
            for name in ("obs", "reward", "done", "terminal_obs", "clean_obs", "clean_terminal_obs", "action_delay"):
                np.testing.assert_array_equal(getattr(env, name).cpu().numpy(), getattr(plain, name).cpu().numpy(),
                                              err_msg=f"{name} after replay {k + 1}")
            np.testing.assert_array_equal(env.sim.get_state(), plain.sim.get_state(), err_msg=f"replay {k + 1}")
            n_done += int(env.done.sum())
        types, edges = _captured_step_graph(env, a)
        side.synchronize()
    assert n_done == 2 * W                            # steps 3 and 6 of 6 end an episode
    assert (env.obs.cpu().numpy() != env.clean_obs.cpu().numpy()).any()
    assert types == [0, 0, 0], types                 # hipGraphNodeTypeKernel
    succ = dict(edges)
    assert len(edges) == 2 and len(succ) == 2 and len(set(succ.values())) == 2
    env.close()
    plain.close()


def test_errors(require_gpu):
    import torch
    from mwstep import native as N
    from mwstep.vecenv import VecEnv
    L = N.lib()
    fp = ctypes.POINTER(ctypes.c_float)

    def call(env, lo=0, hi=0, amp=None):
        c = N.MwFloatNoiseConfig(lo, hi)
        v = None if amp is None else np.ascontiguousarray(amp, np.float32)
        return L.mw_floatenv_noise(env._h, ctypes.byref(c), None if v is None else v.ctypes.data_as(fp),
                                   None, None, None)

    env = _make("quadruped", 4, task="locomotion")
    NO, sl = env.obs_dim, env.obs_slices
    zeros = np.zeros(NO, np.float32)

    def with_word(k, value):
        v = zeros.copy()
        v[k] = value
        return v
    for amp in (with_word(0, -0.1), with_word(5, float("nan")), with_word(NO - 12, float("inf"))):
        assert call(env, amp=amp) == N.MW_EINVAL
        assert "finite and >= 0" in N.last_error()
    for k in (sl["command"].start, sl["command"].stop - 1, sl["last_action"].start, NO - 1):
        assert call(env, amp=with_word(k, 0.1)) == N.MW_EINVAL
        assert "take no noise" in N.last_error()
    for lo, hi in ((-1, 2), (3, 2), (0, 9), (9, 9)):
        assert call(env, lo, hi) == N.MW_EINVAL
        assert "delay_lo <= delay_hi <= 8" in N.last_error()
    assert L.mw_floatenv_noise(env._h, None, None, None, None, None) == N.MW_EINVAL
    # the refused calls left the env as it was: a word just before the command takes noise, and the env steps
    assert call(env, 0, 8, with_word(sl["command"].start - 1, 0.1)) == N.MW_OK
    assert call(env) == N.MW_OK                       # everything off again
    env.reset()
    assert call(env, 0, 2) == N.MW_ESTATE
    assert "before the first mw_vecenv_reset" in N.last_error()
    a = torch.zeros((4, 8), dtype=torch.float32, device=env.device)
    o, r, d, info = env.step(a)
    assert np.isfinite(o.cpu().numpy()).all() and not d.any().item() and "clean_obs" not in info
    env.close()
    # the locomotion task changes the width of the rows: it comes first
    env = _make("quadruped", 4)
    assert call(env, 0, 2) == N.MW_OK
    lc = N.MwFloatLocoConfig()
    lc.track_sigma = 0.25
    assert L.mw_floatenv_locomotion(env._h, ctypes.byref(lc), None) == N.MW_ESTATE
    assert "before mw_floatenv_noise" in N.last_error()
    assert call(env, amp=np.zeros(env.obs_dim, np.float32)) == N.MW_OK      # the forward rows: every word may be noisy
    assert L.mw_floatenv_locomotion(env._h, ctypes.byref(lc), None) == N.MW_ESTATE
    env.close()
    cart = VecEnv("CartPoleDiscreteBalancing", n_worlds=4)
    assert call(cart, 0, 2) == N.MW_ESTATE
    assert "mw_floatenv_create" in N.last_error()
    cart.close()
    # the Python layer
    for bad in ({"command": 0.1}, {"last_action": 0.1}, {"imu": 0.1}):
        with pytest.raises(ValueError, match="obs_noise"):
            _make("quadruped", 4, task="locomotion", obs_noise=bad)
    with pytest.raises(ValueError, match="unknown group 'gravity'"):
        _make("quadruped", 4, obs_noise={"gravity": 0.1})                    # a locomotion word, forward task
    with pytest.raises(ValueError, match="obs_dim"):
        _make("quadruped", 4, obs_noise=[0.1] * 5)
    with pytest.raises(RuntimeError, match="take no noise"):
        _make("quadruped", 4, task="locomotion", obs_noise=[0.1] * 53)
    with pytest.raises(RuntimeError, match="delay_lo <= delay_hi <= 8"):
        _make("quadruped", 4, action_delay_range=(0, 9))
    with pytest.raises(ValueError, match="whole numbers"):
        _make("quadruped", 4, action_delay_range=(0, 1.5))
