"""The device-resident batched env of floating-base robots (mwstep.FloatVecEnv,
mw_floatenv_create; csrc/float_env_kernel.hip around the unchanged wave run).

The yardstick is the project's own host-commanded path on the same GPU: the
wave kernel is unchanged and receives the same float32 inputs, so a twin
Simulator of the same model (same solver options, PID gains, ground plane),
commanded through sim.set("force_target" | "position_target") + sim.run() and
reset through the host setters with the values the env reported, must end in
a bit-identical state record (mw_get_state: q, qd, qdd, PID state, base, the
warm-start impulses) -- the two-sim array_equal pattern of test_gpu_health.py.
Observation words that the host getters return as float64 of the same float32
are compared bit for bit; the world velocity (rotated on the host in fp64) and
the per-link contact force sums (another summation order) within
2e-6 max(1, |x|) and 1e-5 max(1, |f|)."""

import ctypes
import math

import numpy as np
import pytest

from float_env_harness import QUAD_GAINS, STAND, _captured_step_graph, _check_obs, _make, _reset_twin, _twin, _unif32

pytestmark = pytest.mark.gpu


def _reset_ref(oracle, sim, home, noise, seed, world, episode):
    """Restatement of the kernel's reset draw: home + U(-noise, noise) from
    Philox4x32-10 keyed by the seed, counter (global world, episode, dof // 4,
    0), clipped into the position limits."""
    from mwstep import native as N
    n = sim.dofs
    q = np.zeros(n, np.float32)
    for b in range((n + 3) // 4):
        r = oracle.philox_raw([world, episode, b, 0], [seed & 0xFFFFFFFF, seed >> 32])
        for k in range(4):
            d = 4 * b + k
            if d < n:
                x = np.float32(home[d]) + _unif32(np.array([r[k]], np.uint32), -noise, noise)[0]
                lo = np.float32(max(sim.joint_param(d, N.PARAM_POSITION_LIMIT_MIN), -3e38))
                hi = np.float32(min(sim.joint_param(d, N.PARAM_POSITION_LIMIT_MAX), 3e38))
                q[d] = np.clip(x, lo, hi)
    return q


def _run_parity(env, twin, actions_of, steps, links, target, pid_words=False):
    """Step env and twin together; the records stay bit-equal."""
    import torch
    obs = env.reset().cpu().numpy()
    _reset_twin(twin, obs)
    twin.run(paused=True)
    np.testing.assert_array_equal(env.sim.get_state(), twin.get_state())
    worst_v = worst_f = 0.0
    for k in range(steps):
        a = actions_of(k)
        o, r, d, _ = env.step(torch.from_numpy(a).to(env.device))
        twin.set(target, a.astype(np.float64))
        twin.run()
        if k % 10 == 9 or k == steps - 1:
            rec, ref = env.sim.get_state(), twin.get_state()
            np.testing.assert_array_equal(rec, ref, err_msg=f"state records differ after step {k + 1}")
            assert not d.cpu().numpy().any()
            ev, ef = _check_obs(o.cpu().numpy(), twin, links)
            worst_v, worst_f = max(worst_v, ev), max(worst_f, ef)
    if pid_words:
        n = twin.dofs
        rec, ref = env.sim.get_state(), twin.get_state()
        np.testing.assert_array_equal(rec[:, 3 * n:6 * n], ref[:, 3 * n:6 * n])   # pid_e, pid_i, pid_u
        assert np.abs(ref[:, 3 * n:6 * n]).max() > 0
    return o.cpu().numpy(), worst_v, worst_f


def test_twin_parity_torque_quadruped(require_gpu):
    """W = 70: two tiles, the second partial; n = 8, obs_dim = 33."""
    W = 70
    env = _make("quadruped", W, action_mode="torque", home_base=(0, 0, 0.47, 1, 0, 0, 0), z_min=-10.0,
                max_tilt=math.pi, max_episode_steps=0, pid_gains=None)
    assert (env.obs_dim, env.action_dim) == (33, 8)
    twin = _twin(env, "quadruped")
    rng = np.random.default_rng(3)
    obs, ev, ef = _run_parity(env, twin, lambda k: rng.uniform(-5, 5, (W, 8)).astype(np.float32), 150,
                              env.contact_links, "force_target")
    print(f"quadruped torque parity: velocity words {ev:.2e}, contact words {ef:.2e}; "
          f"{int((obs[:, 29:] != 0).any(axis=1).sum())}/{W} worlds with a loaded foot")
    assert ev <= 2e-6 and ef <= 1e-5
    assert (obs[:, 29:] != 0).any()   # the contact path is exercised
    env.close()
    twin.close()


def test_twin_parity_position_icub(require_gpu):
    """The <32> instance of the wave kernel, obs_dim = 79 > 64."""
    from mwstep.models import icub_pid_gains
    W = 5
    env = _make("icub", W, z_min=-10.0, max_tilt=math.pi, max_episode_steps=0)
    assert (env.obs_dim, env.action_dim) == (79, 32)
    gains = [[p, 0.0, d, -80.0, 80.0, 0.0, 0.0, -1.0] for p, d in icub_pid_gains(env.sim.joint_names)]
    twin = _twin(env, "icub", gains)
    rng = np.random.default_rng(5)
    home = env.home_q
    obs, ev, ef = _run_parity(env, twin, lambda k: (home + rng.uniform(-0.1, 0.1, (W, 32))).astype(np.float32), 120,
                              env.contact_links, "position_target", pid_words=True)
    print(f"iCub position parity: velocity words {ev:.2e}, contact words {ef:.2e}")
    assert ev <= 2e-6 and ef <= 1e-5
    assert (obs[:, 77:] != 0).any()
    env.close()
    twin.close()


def test_reset_sampling(require_gpu, oracle):
    W, seed, noise = 70, 7, 0.05
    kw = dict(action_mode="torque", joint_noise=noise, seed=seed, pid_gains=None)
    env = _make("quadruped", W, **kw)
    obs = env.reset().cpu().numpy()
    for w in range(0, W, 7):
        ref = _reset_ref(oracle, env.sim, env.home_q, noise, seed, w, 0)
        assert np.abs(obs[w, 13:21] - ref).max() <= 1e-6
    assert np.abs(obs[:, 13:21] - env.home_q).max() > 0.01      # the noise is there
    np.testing.assert_array_equal(obs[:, 21:29], 0.0)             # qd
    np.testing.assert_array_equal(obs[:, :7], np.tile(env.home_base, (W, 1)))
    np.testing.assert_array_equal(obs[:, 7:13], 0.0)
    np.testing.assert_array_equal(obs[:, 29:], 0.0)               # contact words
    # the simulator shows the reset at once
    np.testing.assert_array_equal(env.sim.get("q").astype(np.float32), obs[:, 13:21])
    np.testing.assert_array_equal(env.sim.base_pose()[:, :3].astype(np.float32), obs[:, :3])
    # a shard's streams do not depend on where it starts
    part = _make("quadruped", 35, world_offset=35, **kw)
    np.testing.assert_array_equal(part.reset().cpu().numpy(), obs[35:])
    part.close()
    env.close()


def test_termination_and_auto_reset(require_gpu, oracle):
    import torch
    W, seed, noise, H = 70, 9, 0.05, 200
    # crouched and dropped from just above touch-down: under no torque the legs
    # fold, the trunk lands after about 110 steps and then settles slowly, each
    # world at its own pace (from the standing posture the worlds sink almost
    # alike and would all cross any height at the same step)
    kw = dict(action_mode="torque", home_q=[1.2, -2.4] * 4, home_base=(0, 0, 0.22, 1, 0, 0, 0),
              joint_noise=noise, seed=seed, max_tilt=math.pi, max_episode_steps=0, pid_gains=None)
    zero = np.zeros((W, 8), np.float32)
    # the twin alone, from the env's episode-0 reset: every world's base height per step
    scout = _make("quadruped", W, z_min=-10.0, **kw)
    obs0 = scout.reset().cpu().numpy()
    twin = _twin(scout, "quadruped")
    scout.close()
    _reset_twin(twin, obs0)
    twin.run(paused=True)
    z = np.zeros((H + 1, W), np.float32)
    z[0] = twin.base_pose()[:, 2]
    for k in range(H):
        twin.set("force_target", zero.astype(np.float64))
        twin.run()
        z[k + 1] = twin.base_pose()[:, 2]
    # z_min strictly between two consecutive heights of world 0 while it sinks
    def crossing(k):
        zm = np.float32(0.5 * (float(z[k, 0]) + float(z[k + 1, 0])))
        return zm, np.array([int(np.argmax(z[:, w] < zm)) for w in range(W)])   # step whose result is below

    # ... the pair at which the worlds' expected done steps differ most
    ks = [k for k in range(100, H) if z[k + 1, 0] < z[k, 0] and crossing(k)[1].min() >= 1]
    k0 = max(ks, key=lambda k: len(set(crossing(k)[1].tolist())))
    z_min, first = crossing(k0)
    assert z[k0 + 1, 0] < z_min < z[k0, 0]
    assert (z < z_min).any(axis=0).all() and first[0] == k0 + 1 and first.min() >= 1
    print(f"z_min {z_min:.6f} after step {k0}: worlds end at {len(set(first.tolist()))} different steps, "
          f"{first.min()}..{first.max()}")
    assert len(set(first.tolist())) >= 10
    # env and twin in lockstep: the twin is reset with what the env reports
    env = _make("quadruped", W, z_min=float(z_min), **kw)
    obs = env.reset().cpu().numpy()
    np.testing.assert_array_equal(obs, obs0)
    _reset_twin(twin, obs)
    twin.run(paused=True)
    episode, steps = np.zeros(W, np.int64), np.zeros(W, np.int64)
    seen_first = np.zeros(W, np.int64)
    total = int(first.max()) + 50
    a_dev = torch.from_numpy(zero).to(env.device)
    for k in range(1, total + 1):
        o, r, d, info = env.step(a_dev)
        twin.set("force_target", zero.astype(np.float64))
        twin.run()
        o, d = o.cpu().numpy(), d.cpu().numpy().astype(bool)
        expect = twin.base_pose()[:, 2].astype(np.float32) < z_min
        np.testing.assert_array_equal(d, expect, err_msg=f"done at step {k}")
        np.testing.assert_array_equal(env.sim.get_state(), twin.get_state(), err_msg=f"state after step {k}")
        steps += 1
        hit = np.flatnonzero(d)
        if len(hit):
            seen_first[hit] = np.where(seen_first[hit] == 0, k, seen_first[hit])
            term = info["terminal_obs"].cpu().numpy()
            ev, ef = _check_obs(term, twin, env.contact_links, hit)
            assert ev <= 2e-6 and ef <= 1e-5
            # no alive bonus where terminated: w_forward v_x alone (the other weights are 0)
            np.testing.assert_array_equal(r.cpu().numpy()[hit], term[hit, 7])
            episode[hit] += 1
            steps[hit] = 0
            for w in hit[:8]:
                ref = _reset_ref(oracle, env.sim, env.home_q, noise, seed, int(w), int(episode[w]))
                assert np.abs(o[w, 13:21] - ref).max() <= 1e-6
            np.testing.assert_array_equal(o[hit, :7], np.tile(env.home_base, (len(hit), 1)))
            np.testing.assert_array_equal(o[hit, 7:13], 0.0)
            np.testing.assert_array_equal(o[hit, 21:], 0.0)
            _reset_twin(twin, o, hit)
        ep, st = env.counters()
        np.testing.assert_array_equal(ep.cpu().numpy(), episode)
        np.testing.assert_array_equal(st.cpu().numpy(), steps)
    np.testing.assert_array_equal(seen_first, first)
    env.close()
    twin.close()


def test_time_limit(require_gpu):
    import torch
    W = 70
    env = _make("quadruped", W, action_mode="torque", z_min=-10.0, max_tilt=math.pi, max_episode_steps=40,
                pid_gains=None)
    env.reset()
    a = torch.zeros((W, 8), dtype=torch.float32, device=env.device)
    for k in range(1, 86):
        _, _, d, _ = env.step(a)
        assert bool(d.all()) == (k % 40 == 0) and bool(d.any()) == (k % 40 == 0), k
    ep, st = env.counters()
    assert (ep.cpu().numpy() == 2).all() and (st.cpu().numpy() == 5).all()
    env.close()


def test_tilt_termination(require_gpu):
    import torch
    W = 70
    rolled = (0.0, 0.0, 0.6, math.cos(0.6), math.sin(0.6), 0.0, 0.0)     # 1.2 rad about x
    env = _make("quadruped", W, home_base=rolled, z_min=-10.0, max_tilt=1.0, max_episode_steps=0)
    env.reset()
    a = torch.from_numpy(np.tile(np.float32(STAND), (W, 1))).to(env.device)
    _, _, d, _ = env.step(a)
    assert bool(d.all())
    env.close()
    env = _make("quadruped", W, z_min=-10.0, max_tilt=1.0, max_episode_steps=0)
    env.reset()
    for _ in range(20):
        _, r, d, _ = env.step(a)
        assert not bool(d.any())
    assert (r.cpu().numpy() > 0.5).all()    # the alive bonus, hardly any velocity
    env.close()


def test_divergence_resets_the_world(require_gpu):
    import torch
    W, bad = 8, 3
    env = _make("icub", W, action_mode="torque", z_min=-10.0, max_tilt=math.pi, max_episode_steps=0,
                pid_gains=None)
    twin = _twin(env, "icub")
    obs = env.reset().cpu().numpy()
    _reset_twin(twin, obs)
    twin.run(paused=True)
    rng = np.random.default_rng(2)
    others = [w for w in range(W) if w != bad]
    for k in range(1, 26):
        a = rng.uniform(-1, 1, (W, 32)).astype(np.float32)
        at = a.copy()
        if k == 5:
            a[bad, 7] = np.nan
        o, r, d, _ = env.step(torch.from_numpy(a).to(env.device))
        d = d.cpu().numpy().astype(bool)
        if k == 5:
            assert d.tolist() == [w == bad for w in range(W)]
            flags, count = env.sim.diverged()
            assert count == 1 and not flags.any()
        else:
            assert not d.any(), k
        twin.set("force_target", at.astype(np.float64))
        twin.run()
        np.testing.assert_array_equal(env.sim.get_state()[others], twin.get_state()[others])
    assert np.isfinite(env.sim.get_state()[bad]).all()
    flags, count = env.sim.diverged()
    assert count == 1 and not flags.any()
    env.close()
    twin.close()


def test_graph_capture(require_gpu):
    import torch
    W, K = 70, 20
    kw = dict(joint_noise=0.05, seed=4, z_min=-10.0, max_tilt=math.pi, max_episode_steps=0)
    rng = np.random.default_rng(8)
    acts = (np.float32(STAND) + rng.uniform(-0.2, 0.2, (K + 1, W, 8))).astype(np.float32)
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
        for k in range(K):
            a.copy_(torch.from_numpy(acts[k + 1]).to(env.device))
            graph.replay()
        side.synchronize()
        got = env.sim.get_state()
        types, edges = _captured_step_graph(env, a)
        side.synchronize()
    plain = _make("quadruped", W, **kw)
    plain.reset()
    for k in range(K + 1):
        plain.step(torch.from_numpy(acts[k]).to(plain.device))
    np.testing.assert_array_equal(got, plain.sim.get_state())
    # three kernel nodes in one serial chain
    assert types == [0, 0, 0], types                 # hipGraphNodeTypeKernel
    succ = dict(edges)
    assert len(edges) == 2 and len(succ) == 2 and len(set(succ.values())) == 2
    head = ({0, 1, 2} - set(succ.values())).pop()
    assert len({head, succ[head], succ[succ[head]]}) == 3
    env.close()
    plain.close()


def test_errors(require_gpu):
    import torch
    from mwstep import FloatVecEnv
    with pytest.raises(RuntimeError, match="articulated model on a floating base"):
        FloatVecEnv("cartpole", 4)
    with pytest.raises(RuntimeError, match="articulated model on a floating base"):
        FloatVecEnv("cube", 4)
    with pytest.raises(RuntimeError, match="contact link 8 out of range"):
        FloatVecEnv.quadruped(4, contact_links=(0, 8))
    with pytest.raises(ValueError, match="not found"):
        FloatVecEnv.quadruped(4, contact_links=("no_such_link",))
    with pytest.raises(ValueError, match="one value per dof"):
        FloatVecEnv.quadruped(4, home_q=[0.0] * 7)
    env = _make("quadruped", 4)
    # a second env on the same simulator, a null home_q
    from mwstep import native as N
    cfg = N.MwFloatTaskConfig()
    cfg.home_base[3] = 1.0
    h = ctypes.c_void_p()
    assert N.lib().mw_floatenv_create(env.sim.handle, ctypes.byref(cfg), ctypes.byref(h)) == N.MW_ESTATE
    assert "already has a floating-base env" in N.last_error()
    from mwstep.sim import Simulator
    from mwstep import get_model_file
    lone = Simulator(get_model_file("quadruped"), n_worlds=2)
    assert N.lib().mw_floatenv_create(lone.handle, ctypes.byref(cfg), ctypes.byref(h)) == N.MW_EINVAL
    assert "home_q is null" in N.last_error()
    lone.close()
    env.reset()
    good = torch.zeros((4, 8), dtype=torch.float32, device=env.device)
    with pytest.raises(RuntimeError, match="fused rollout is not available"):
        env.rollout(good)
    for bad in (torch.zeros((4, 7), dtype=torch.float32, device=env.device),
                torch.zeros((4, 8), dtype=torch.float64, device=env.device),
                torch.zeros((8, 4), dtype=torch.float32, device=env.device).t(),
                np.zeros((4, 8), np.float32)):
        with pytest.raises(TypeError, match="actions must be"):
            env.step(bad)
    # the env owns the commands and pending resets of its simulator: the host
    # setters of either are refused (MW_ESTATE), not lost; the getters work
    sim = env.sim
    for call in (lambda: sim.set("force_target", np.zeros((4, 8))),
                 lambda: sim.set("position_target", np.zeros((4, 8))),
                 lambda: sim.set("reset_q", np.zeros((4, 8))),
                 lambda: sim.set("reset_qd", np.zeros((4, 8))),
                 lambda: sim.reset_base_pose((0, 0, 1, 1, 0, 0, 0)),
                 lambda: sim.reset_base_velocity(np.zeros(6)),
                 lambda: sim.set_control_mode(N.MODE_FORCE),
                 lambda: sim.set_pid(0, QUAD_GAINS[0]),
                 lambda: sim.set_state(sim.get_state())):
        with pytest.raises(RuntimeError, match="a floating-base env owns this simulator"):
            call()
    before = sim.get_state()
    env.step(good)
    assert sim.get("q").shape == (4, 8) and not np.array_equal(sim.get_state(), before)
    # ... and work again once the env is gone
    h, env._h = env._h, None
    N.lib().mw_vecenv_destroy(h)
    sim.set("reset_q", np.zeros((4, 8)))
    sim.run(paused=True)
    np.testing.assert_array_equal(sim.get("q"), 0.0)
    env.close()
