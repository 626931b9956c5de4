"""FloatVecEnv on a 48-joint tree with 8 contact links (big_tree_cases.tree48:
the seven leaf spheres and the base): the env kernels of float_env_kernel.hip
at n > 32 -- three tiles of action words at (n | 1) = 49, the 13th Philox
block of the link scales, dof_mask bits >= 32, observation rows of 177 words,
and the dynamic LDS of the post kernel at the maximum its launcher computes
(48 dofs, 8 contact links, locomotion and shaping) -- around the 48-body
instances of the wave kernel.

The yardsticks are those of test_gpu_float_env.py, test_gpu_float_inertia_env.py
and test_gpu_float_joints_env.py, through their helpers: a host-commanded twin
Simulator given what the env reports ends every step with a bit-identical
mw_get_state record; the draws are restated from the oracle's Philox; the
shaping terms are the host build's bits.
"""

import numpy as np
import pytest

import big_tree_cases as C
from float_env_harness import (ALL, FREE, JOINTS, PUSH, _captured_step_graph, _check_draws, _check_obs, _check_rows,
                               _delay_ref, _dev, _forces32, _limits, _nominal, _params, _parity, _reset_twin, _twin)
from float_joints_ref import build_harness
from float_shape_ref import ShapeHost

pytestmark = pytest.mark.gpu

NAME, N = "tree48", 48
LOCO = dict(task="locomotion", command_ranges=((-1.0, 1.0), (-0.5, 0.5), (-1.0, 1.0)), cmd_interval=3,
            cmd_zero_prob=0.2, cmd_min=0.1, w_action_rate=0.01)
SCALES, PAYLOADS, BOX = (0.8, 1.25), (0.0, 5.0), (0.1, 0.08, 0.05)
INERTIA = dict(mass_scale_range=SCALES, payload_range=PAYLOADS, payload_box=BOX)
NOISE = dict(base_position=0.01, base_angular_velocity=0.05, joint_positions=0.02, joint_velocities=0.5,
             contacts=2.0, gravity=0.05, body_angular_velocity=0.1)
HIGH_DOFS = list(range(32, N))              # 16 Coulomb rows at most: within the 64 of a world
# the trunk a termination link that a force of 1e6 N never ends an episode by, the leaves penalised
SHAPE = dict(reward_terms=ALL, termination_links=(-1,), termination_force=1e6, penalised_links=tuple(C.leaves(NAME)),
             collision_force_min=0.1, soft_limit=0.3, stumble_ratio=0.2, max_contact_force=5.0)
EVERYTHING = dict(joint_noise=0.05, friction_range=(0.3, 1.2), joint_rand_dofs=HIGH_DOFS, obs_noise=NOISE,
                  action_delay_range=(0, 3), **PUSH, **LOCO, **INERTIA, **JOINTS, **SHAPE)


@pytest.fixture(scope="module")
def home(oracle):
    return C.env_home(oracle, NAME)


@pytest.fixture(scope="module")
def fj(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("fj_big"))


@pytest.fixture(scope="module")
def fs(tmp_path_factory):
    return ShapeHost(tmp_path_factory.mktemp("fs_big"))


def _env(home, n_worlds, action_mode="position", **kw):
    from mwstep import FloatVecEnv
    base, links = home
    args = dict(action_mode=action_mode, home_base=base, contact_links=links, pgs_iters=50,
                pid_gains=[C.ENV_PID] * N if action_mode == "position" else None, **FREE)
    args.update(kw)
    env = FloatVecEnv(C.urdf(NAME), n_worlds, **args)
    env._pgs_iters = 50
    assert env.sim.float_kernel() == 2 and env.sim.dofs == N > 32 and env.action_dim == N
    assert len(env.contact_links) == 8
    return env


def _check_layout(env, loco):
    n_obs = (25 + 3 * N + 8) if loco else (13 + 2 * N + 8)
    assert env.obs_dim == n_obs
    sl = env.obs_slices
    assert sl["base"] == slice(0, 13) and sl["joints"] == slice(13, 13 + 2 * N)
    assert sl["contacts"] == slice(13 + 2 * N, 13 + 2 * N + 8)
    if loco:
        nb = 13 + 2 * N + 8
        assert (sl["gravity"], sl["body_velocity"], sl["command"], sl["last_action"]) == \
            (slice(nb, nb + 3), slice(nb + 3, nb + 9), slice(nb + 9, nb + 12), slice(nb + 12, nb + 12 + N))
        assert sl["last_action"].stop == n_obs == 177


class _CleanRows:
    """The env as _parity drives it, reporting the rows before the observation noise: the twin is reset from
    what the simulator holds, which the noisy rows are not."""

    def __init__(self, env):
        self._env = env

    def __getattr__(self, name):
        return getattr(self._env, name)

    def reset(self):
        self._env.reset()
        return self._env.clean_obs

    def step(self, a):
        _, r, d, info = self._env.step(a)
        return self._env.clean_obs, r, d, info


def _command_of(env, position, scale):
    """What the env sent to its simulator goes to the twin.  Position mode: the simulator's own target words.
    Torque mode: the action of `delay` steps ago times the scale (one exact float32 multiply by 0.5), zero
    during an episode's first `delay` steps -- restated here from env.action_delay as
    test_gpu_float_noise.test_delay_torque_twin restates it."""
    if position:
        return lambda twin, a: twin.set("position_target", env.sim.get("position_target"))
    st = {}

    def send(twin, a):
        W = env.n_worlds
        if not st:
            st.update(t=np.zeros(W, np.int64), history=np.zeros((16, W, N), np.float32))
            st["delay"] = np.zeros(W, np.int64) if env.action_delay is None else None
        done = env.done.cpu().numpy().astype(bool)
        if st["delay"] is None:                    # the first step of the run: no world is done yet
            assert not done.any()
            st["delay"] = env.action_delay.cpu().numpy().astype(np.int64)
        t, delay = st["t"], st["delay"]
        st["history"][t, np.arange(W)] = a
        applied = np.where((t < delay)[:, None], np.float32(0), st["history"][np.maximum(t - delay, 0), np.arange(W)])
        twin.set("force_target", (np.float32(scale) * applied).astype(np.float64))
        t += 1
        t[done] = 0
        if env.action_delay is not None:
            delay[done] = env.action_delay.cpu().numpy()[done]
    return send


def _actions(steps, n_worlds, position, seed):
    rng = np.random.default_rng(seed)
    spread = 0.4 if position else 40.0
    return rng.uniform(-spread, spread, (steps + 1, n_worlds, N)).astype(np.float32)


@pytest.mark.parametrize("mode", ["torque", "position"])
@pytest.mark.parametrize("n_worlds", [1, 65])
def test_twin_parity_plain(require_gpu, home, mode, n_worlds):
    """No randomisation but the reset noise; two episodes of 8 steps and a
    third begun, the twin reset from the rows of every done step."""
    position = mode == "position"
    steps, H = 18, 8
    env = _env(home, n_worlds, mode, joint_noise=0.05, seed=31, max_episode_steps=H)
    _check_layout(env, False)
    twin = _twin(env, C.urdf(NAME), [C.ENV_PID] * N if position else None)
    acts = _actions(steps, n_worlds, position, 3)
    if position:
        acts += env.home_q
    obs = env.reset().cpu().numpy()
    _reset_twin(twin, obs)
    twin.run(paused=True)
    np.testing.assert_array_equal(env.sim.get_state(), twin.get_state())
    worst_v = worst_f = 0.0
    loaded = np.zeros(8, bool)
    for k in range(1, steps + 1):
        o, r, d, _ = env.step(_dev(env, acts[k]))
        twin.set("position_target" if position else "force_target", acts[k].astype(np.float64))
        twin.run()
        np.testing.assert_array_equal(env.sim.get_state(), twin.get_state(), err_msg=f"state after step {k}")
        o, d = o.cpu().numpy(), d.cpu().numpy().astype(bool)
        assert d.all() == (k % H == 0) and d.any() == (k % H == 0)
        assert np.isfinite(o).all() and np.isfinite(r.cpu().numpy()).all()
        if d.any():
            _reset_twin(twin, o, np.flatnonzero(d))
        else:
            ev, ef = _check_obs(o, twin, env.contact_links)
            worst_v, worst_f = max(worst_v, ev), max(worst_f, ef)
            loaded |= (o[:, env.obs_slices["contacts"]] != 0).any(axis=0)
    print(f"tree48 x{n_worlds} {mode}, plain: velocity words {worst_v:.2e}, contact words {worst_f:.2e}; contact "
          f"links that carried load {loaded.astype(int).tolist()}")
    assert worst_v <= 2e-6 and worst_f <= 1e-5
    assert loaded.any() and env.sim.constraint_overflow() == 0
    env.close()
    twin.close()


@pytest.mark.parametrize("mode", ["torque", "position"])
@pytest.mark.parametrize("n_worlds", [1, 65])
def test_twin_parity_with_everything_on(require_gpu, home, mode, n_worlds):
    """Locomotion, shaping (all ten weights, a termination link, seven
    penalised links), observation noise, action delay, pushes, ground friction,
    mass scales with a payload and joint draws on the dofs 32..47: the dynamic
    LDS of the post kernel at the maximum its launcher computes.  The launch
    succeeds, and float_env_harness._parity holds over two episodes."""
    import torch
    position = mode == "position"
    steps, H = 16, 8
    env = _env(home, n_worlds, mode, seed=12, max_episode_steps=H, action_scale=0.25 if position else 0.5, **EVERYTHING)
    _check_layout(env, True)
    assert env.inertial.shape == (n_worlds, N + 1, 10) and env.joint_dynamics.shape == (n_worlds, N, 3)
    assert env.reward_terms.shape == (n_worlds, 10) and env.action_delay.shape == (n_worlds,)
    twin = _twin(env, C.urdf(NAME), [C.ENV_PID] * N if position else None)
    acts = _actions(steps, n_worlds, position, 5)
    seen = _parity(_CleanRows(env), twin, lambda k: acts[k], steps, H, _command_of(env, position, 0.5),
                   carry=("inertial", "joint_dynamics"))["joint_dynamics"]
    torch.cuda.synchronize()
    assert len(seen) == 3 and not np.array_equal(seen[0], seen[1])
    low = [d for d in range(N) if d not in HIGH_DOFS]
    for words in seen:                      # the mask: bits 32..47 and no other
        np.testing.assert_array_equal(words[:, low], np.tile(_nominal(twin)[low], (n_worlds, 1, 1)))
        assert (words[:, HIGH_DOFS, 1] > 0).all()
    obs = env.obs.cpu().numpy()
    assert np.isfinite(obs).all() and np.isfinite(env.reward.cpu().numpy()).all()
    assert np.isfinite(env.reward_terms.cpu().numpy()).all() and (env.reward_terms.cpu().numpy() != 0).any()
    assert (obs != env.clean_obs.cpu().numpy()).any()
    assert env.sim.lcp_unconverged() == 0
    env.close()
    twin.close()


def test_draws_are_the_stated_ones(require_gpu, oracle, home, fj):
    """W = 65, every world of the tile edge, episodes 0 and 1:
      * the 49 link scales (the 13th Philox block holds the last link's alone),
        the payload and its position;
      * the draws of all 48 joints, and the words from them by the host build
        of the kernel's function;
      * the action delay, and the noise of rows of 177 words (45 Philox blocks
        a row, the kernel walks the (row, block) pairs), given as a vector of
        177 amplitudes: every word that can take noise has its own, 0..125, so
        block 31 mixes two noisy words with two that are not.  The words from
        126 on are the command and the last action, which the library refuses
        to make noisy (test_noise_vector_edges): they equal the clean row bit
        for bit.  No row of this env has a noisy word beyond index 125 -- 13 + 2
        n + links + 9 = 126 at n = 48 with 8 links."""
    from float_inertia_ref import draw_ref
    n_worlds, seed, H = 65, 21, 3
    env = _env(home, n_worlds, "torque", seed=seed, max_episode_steps=H, obs_noise=_amplitudes(177, 126),
               action_delay_range=(0, 3), **LOCO, **INERTIA, **JOINTS)
    _check_layout(env, True)
    amp = env.obs_noise.cpu().numpy()
    np.testing.assert_array_equal(amp, _amplitudes(177, 126))
    assert amp[:126].all() and not amp[126:].any()
    nominal = _nominal(env.sim)
    worlds = [0, 31, 63, 64]
    tol_s = 4 * 2.0 ** -23 * (SCALES[1] - SCALES[0])
    tol_m = 4 * 2.0 ** -23 * (PAYLOADS[1] - PAYLOADS[0])
    tol_p = np.array([4 * 2.0 ** -23 * 2 * b for b in BOX])
    zero = _dev(env, np.zeros((n_worlds, N)))
    obs = env.reset().cpu().numpy()
    worst = dict(scale=0.0, payload=0.0, joints=0.0, noise=0.0)
    last_scales = []
    for episode in (0, 1):
        draws = env.inertia_draws.cpu().numpy()
        assert draws.shape == (n_worlds, N + 5)
        s, mp, p = draws[:, :N + 1], draws[:, N + 1], draws[:, N + 2:]
        for w in worlds:
            rs, rm, rp = draw_ref(oracle, seed, w, episode, N, SCALES, PAYLOADS, BOX)
            worst["scale"] = max(worst["scale"], float(np.abs(s[w].astype(np.float64) - rs).max()) / tol_s)
            worst["payload"] = max(worst["payload"], abs(float(mp[w]) - float(rm)) / tol_m,
                                   float((np.abs(p[w].astype(np.float64) - rp) / tol_p).max()))
        last_scales.append(s[:, N].copy())
        # the 49th scale acts: the last link's mass is its nominal one times the draw
        mass = env.inertial.cpu().numpy()[:, N, 0]
        assert len(np.unique(s[:, N])) > 0.9 * n_worlds and len(np.unique(mass)) > 0.9 * n_worlds
        worst["joints"] = max(worst["joints"], _check_draws(env, oracle, fj, seed, episode, None, nominal, worlds))
        delay = env.action_delay.cpu().numpy()
        for w in worlds:
            assert delay[w] == _delay_ref(oracle, seed, w, episode, 0, 3)
        assert len(set(delay.tolist())) > 1
        ep, st = (c.cpu().numpy() for c in env.counters())
        assert (ep == episode).all() and not st.any()
        worst["noise"] = max(worst["noise"], _check_rows(oracle, seed, 0, amp, obs, env.clean_obs.cpu().numpy(),
                                                         worlds, ep, st))
        for k in range(H):
            o, _, d, _ = env.step(zero)
            obs = o.cpu().numpy()
            ep, st = (c.cpu().numpy() for c in env.counters())
            worst["noise"] = max(worst["noise"], _check_rows(oracle, seed, 0, amp, obs, env.clean_obs.cpu().numpy(),
                                                             worlds, ep, st))
        assert d.cpu().numpy().all()
    assert (last_scales[0] != last_scales[1]).all()
    print("tree48 x65 draws (error / bound): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values())
    env.close()


def _amplitudes(n_obs, noisy):
    """n_obs float32 amplitudes, a different one in each word of a Philox block, zero from word `noisy` on"""
    amp = (0.01 * (1 + np.arange(n_obs) % 7)).astype(np.float32)
    amp[noisy:] = 0.0
    return amp


def test_noise_vector_edges(require_gpu, oracle, home):
    """The amplitude vector at its edges.  Locomotion rows (177 words): an
    amplitude on the first command word (126), on word 129 or on the last word
    (176, alone in the last block) is refused.  Forward rows (117 words: every
    word takes noise): the last Philox block, b = 29, holds word 116 alone (NO -
    4 b = 1); every word against the stated draw, terminal rows included, at
    the tile's edge worlds over two episodes."""
    for k in (126, 129, 176):
        amp = _amplitudes(177, 126)
        amp[k] = 0.01
        with pytest.raises(RuntimeError, match=rf"take no noise \(word {k}\)"):
            _env(home, 2, "torque", obs_noise=amp, **LOCO)
    n_worlds, seed, H = 65, 27, 3
    env = _env(home, n_worlds, "torque", seed=seed, max_episode_steps=H, joint_noise=0.05,
               obs_noise=_amplitudes(117, 117))
    _check_layout(env, False)
    amp = env.obs_noise.cpu().numpy()
    assert amp.shape == (117,) and amp.all() and (117 + 3) // 4 == 30 and 117 - 4 * 29 == 1
    worlds = [0, 31, 63, 64]
    zero = _dev(env, np.zeros((n_worlds, N)))
    obs = env.reset().cpu().numpy()
    ep, st = (c.cpu().numpy() for c in env.counters())
    worst = _check_rows(oracle, seed, 0, amp, obs, env.clean_obs.cpu().numpy(), worlds, ep, st)
    moved = 0
    for k in range(1, 2 * H + 1):
        last, ep_before = st + 1, ep
        o, _, d, info = env.step(zero)
        obs, d = o.cpu().numpy(), d.cpu().numpy().astype(bool)
        clean = env.clean_obs.cpu().numpy()
        ep, st = (c.cpu().numpy() for c in env.counters())
        worst = max(worst, _check_rows(oracle, seed, 0, amp, obs, clean, worlds, ep, st))
        moved += int((obs[worlds, 116] != clean[worlds, 116]).sum())
        assert d.all() == (k % H == 0) and d.any() == (k % H == 0)
        if d.any():
            worst = max(worst, _check_rows(oracle, seed, 0, amp, info["terminal_obs"].cpu().numpy(),
                                           info["clean_terminal_obs"].cpu().numpy(), worlds, ep_before, last))
    print(f"tree48 x65, 117 noisy words: worst error / bound {worst:.3f}; word 116 moved in {moved} of "
          f"{2 * H * len(worlds)} rows")
    assert worst <= 1.0 and moved > H * len(worlds)
    env.close()


def test_joint_mask_of_high_dofs_only(require_gpu, oracle, home, fj):
    """dof_mask = bits 32..47: those joints draw, the other 32 keep the nominal
    words bit for bit (asserted by _check_draws) and report the draws 0, 0, 1."""
    n_worlds, seed = 65, 24
    env = _env(home, n_worlds, "torque", seed=seed, max_episode_steps=4, joint_rand_dofs=HIGH_DOFS, **JOINTS)
    nominal = _nominal(env.sim)
    np.testing.assert_array_equal(env.joint_dynamics.cpu().numpy(), np.tile(nominal, (n_worlds, 1, 1)))
    env.reset()
    worst = _check_draws(env, oracle, fj, seed, 0, HIGH_DOFS, nominal, [0, 63, 64])
    words = env.joint_dynamics.cpu().numpy()
    assert (words[:, HIGH_DOFS, 2] < nominal[HIGH_DOFS, 2]).all() and (words[:, HIGH_DOFS, 0] > 0).all()
    print(f"tree48 x65, joints 32..47 drawn: worst draw error / bound {worst:.3f}")
    env.close()


def test_shaping_terms_are_the_host_build(require_gpu, home, fs):
    """All ten terms at n = 48 with 8 contact and 7 penalised links: the four
    waves' partial sums over 48 dofs give the bits of the host build
    (float_shape_ref.ShapeHost) of the same expressions, every world and step."""
    n_worlds, steps = 5, 12
    kw = dict(SHAPE, soft_limit=0.02)      # 0.03 rad / 4 mm about the centre: the reset noise is beyond it
    env = _env(home, n_worlds, "position", seed=6, joint_noise=0.05, max_episode_steps=0, action_scale=0.0,
               **LOCO, **kw)
    sim = env.sim
    lo, hi = _limits(fs, sim, kw["soft_limit"])
    par = _params(fs, env, kw)
    obs = env.reset().cpu().numpy()
    rng = np.random.default_rng(22)
    qd_prev = np.zeros((n_worlds, N), np.float32)
    seen = np.zeros(10, bool)
    for k in range(steps):
        cmd = obs[:, env.obs_slices["command"]]
        a = (env.home_q + rng.uniform(-0.4, 0.4, (n_worlds, N))).astype(np.float32)
        o, _, d, _ = env.step(_dev(env, a))
        obs = o.cpu().numpy()
        assert not d.cpu().numpy().any()
        tau, terms = env.torques.cpu().numpy(), env.reward_terms.cpu().numpy()
        assert (tau[:, 32:] != 0).any()
        q, qd, pose = sim.get("q").astype(np.float32), sim.get("qd").astype(np.float32), sim.base_pose()
        for w in range(n_worlds):
            cf, pf = _forces32(sim, w, env.contact_links), _forces32(sim, w, env.penalised_links)
            standing = fs.standing(cmd[w, 0], cmd[w, 1], LOCO["cmd_min"])
            _, expect = fs.world(par, tau[w], q[w], qd[w], qd_prev[w], lo, hi, env.home_q, cf, pf, pose[w], standing)
            np.testing.assert_array_equal(terms[w], expect, err_msg=f"step {k}, world {w}")
        seen |= (terms < 0).any(axis=0)
        qd_prev = qd
    print(f"tree48 shaping terms: host build bit for bit over {steps} steps; terms that acted "
          f"{seen.astype(int).tolist()}")
    # torque, power, joint_acc, base_height, joint_limits, a leaf pressed
    assert seen[[0, 1, 2, 4, 5, 6]].all(), seen
    env.close()


def test_graph_capture(require_gpu, home):
    """One captured step with everything on: three kernel nodes in a chain;
    10 replays, an episode end among them, are 10 eager steps bit for bit."""
    import torch
    n_worlds, K = 65, 10
    kw = dict(seed=4, max_episode_steps=6, action_scale=0.25, **EVERYTHING)
    acts = _actions(K, n_worlds, True, 8)
    outputs = ("obs", "reward", "done", "reward_terms", "torques", "joint_dynamics", "inertial", "clean_obs")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        env = _env(home, n_worlds, "position", **kw)
        env.reset()
        a = _dev(env, acts[0])
        env.step(a)                                  # warm-up
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            env.step(a)
        for k in range(K):
            a.copy_(_dev(env, acts[k + 1]))
            graph.replay()
        side.synchronize()
        got = {name: getattr(env, name).cpu().numpy().copy() for name in outputs}
        state = env.sim.get_state()
        types, edges = _captured_step_graph(env, a)
        side.synchronize()
    plain = _env(home, n_worlds, "position", **kw)
    plain.reset()
    n_done = 0
    for k in range(K + 1):
        plain.step(_dev(plain, acts[k]))
        n_done += int(plain.done.sum())
    np.testing.assert_array_equal(state, plain.sim.get_state())
    for name in outputs:
        np.testing.assert_array_equal(got[name], getattr(plain, name).cpu().numpy(), err_msg=name)
    assert types == [0, 0, 0] and len(edges) == 2
    assert n_done == n_worlds
    env.close()
    plain.close()


def test_sharding(require_gpu, home):
    """Worlds 30..64 of the whole env are the env made with world_offset = 30, bit for bit."""
    steps = 10
    kw = dict(seed=21, max_episode_steps=4, action_scale=0.5, **EVERYTHING)
    env = _env(home, 65, "torque", **kw)
    part = _env(home, 35, "torque", world_offset=30, **kw)
    acts = _actions(steps, 65, False, 9)
    outputs = ("obs", "reward", "done", "reward_terms", "joint_dynamics", "joint_draws", "inertial", "inertia_draws",
               "friction", "push", "command", "action_delay", "clean_obs")
    env.reset()
    part.reset()
    for k in range(steps + 1):
        for name in outputs:
            np.testing.assert_array_equal(getattr(part, name).cpu().numpy(), getattr(env, name).cpu().numpy()[30:],
                                          err_msg=f"{name} after step {k}")
        np.testing.assert_array_equal(part.sim.get_state(), env.sim.get_state()[30:], err_msg=f"state after step {k}")
        env.step(_dev(env, acts[k]))
        part.step(_dev(part, acts[k, 30:]))
    env.close()
    part.close()
