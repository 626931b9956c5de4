"""Shaping rewards, contact termination and episode statistics of the
floating-base env on the GPU (mwstep.FloatVecEnv reward_terms= /
termination_links= / penalised_links=, mw_floatenv_shaping; the shaping branch
of csrc/float_env_kernel.hip).

The yardsticks: a twin env without the feature (physics, observations and the
old reward keep their bits); the host build of the term arithmetic
(tests/host_float_shape/harness.cpp, itself checked against fp64 by
test_float_shape_host.py) fed with what the simulator's getters report -- the
terms are defined bit for bit, so the device must reproduce them exactly; for
the torques, the action and the PID law written out in numpy; for termination
the getters' contact list; for the statistics the test's own float32 running
sums."""


import math

import numpy as np
import pytest

from float_env_harness import (ALL, FREE, LOCO_EVERY_TERM, STAND, _captured_step_graph, _dev, _forces32, _limits,
                               _make, _params)
from float_shape_ref import TERMS, ShapeHost

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
W = 70                                                # two tiles, the second partial
# a soft limit the standing hips (0.6 of +-1.5) are already beyond, a foot force limit the stance exceeds
SHAPE = dict(reward_terms=ALL, termination_links=("trunk",), termination_force=1.0, penalised_links=("trunk",),
             collision_force_min=0.1, base_height_target=0.4, soft_limit=0.3, stumble_ratio=0.2, max_contact_force=5.0)
P_GAIN, CMD_MAX = 400.0, 100.0
P_ONLY = [[P_GAIN, 0.0, 0.0, -CMD_MAX, CMD_MAX, 0.0, 0.0, -1.0]] * 8


@pytest.fixture(scope="module")
def fs(tmp_path_factory):
    return ShapeHost(tmp_path_factory.mktemp("fs_gpu"))


def _kernel_order_sum(r0, terms):
    r = r0.astype(np.float32).copy()
    for k in range(10):
        r = (r + terms[:, k]).astype(np.float32)
    return r


def test_physics_and_the_old_reward_are_untouched(require_gpu):
    """Position mode, 30 steps of fixed random actions; every weight set, the trunk a termination and a
    penalised link that never touches the ground."""
    kw = dict(seed=5, joint_noise=0.05, max_episode_steps=0, **FREE, **LOCO_EVERY_TERM)
    on, off = _make("quadruped", W, **kw, **SHAPE), _make("quadruped", W, **kw)
    assert on.reward_term_names == TERMS and off.reward_terms is None
    np.testing.assert_array_equal(on.reset().cpu().numpy(), off.reset().cpu().numpy())
    rng = np.random.default_rng(21)
    seen = np.zeros(10, bool)
    for k in range(30):
        a = rng.uniform(-1.5, 1.5, (W, 8)).astype(np.float32)
        o1, r1, d1, _ = on.step(_dev(on, a))
        o0, r0, d0, _ = off.step(_dev(off, a))
        np.testing.assert_array_equal(o1.cpu().numpy(), o0.cpu().numpy(), err_msg=f"obs, step {k}")
        np.testing.assert_array_equal(d1.cpu().numpy(), d0.cpu().numpy())
        assert not d1.cpu().numpy().any()
        np.testing.assert_array_equal(on.sim.get_state(), off.sim.get_state(), err_msg=f"state, step {k}")
        terms = on.reward_terms.cpu().numpy()
        assert (terms <= 0).all()
        seen |= (terms < 0).any(axis=0)
        # reward_on is reward_off with the ten terms added in column order, each addition in float32
        np.testing.assert_array_equal(r1.cpu().numpy(), _kernel_order_sum(r0.cpu().numpy(), terms))
    assert seen[[0, 1, 2, 3, 4, 5, 8, 9]].all(), seen   # every term that can act without a fall did
    np.testing.assert_array_equal(on.reward_terms.cpu().numpy()[:, 6], 0.0)
    on.close()
    off.close()


@pytest.mark.parametrize("case", ["position", "position_effort_scaled", "torque"])
def test_terms_against_an_independent_recomputation(require_gpu, fs, case):
    """Each step the getters' q, qd, base pose and contact forces and env.torques go through the host harness;
    env.reward_terms must be those bits.  env.torques itself is checked against the action and the PID law."""
    position = case != "torque"
    kw = dict(seed=6, joint_noise=0.05, max_episode_steps=0, action_scale=0.0, **FREE, **LOCO_EVERY_TERM)
    if position:
        kw.update(pid_gains=P_ONLY)
    else:
        kw.update(action_mode="torque", pid_gains=None, home_base=(0, 0, 0.47, 1, 0, 0, 0))
    if case == "position_effort_scaled":
        kw.update(effort_scale_range=(0.3, 0.9))
    env = _make("quadruped", W, **kw, **SHAPE)
    sim, n = env.sim, 8
    lo, hi = _limits(fs, sim, SHAPE["soft_limit"])
    par = _params(fs, env, SHAPE)
    obs = env.reset().cpu().numpy()
    if case == "position_effort_scaled":
        effort = env.joint_dynamics.cpu().numpy()[:, :, 2]
        assert 18.0 <= effort.min() < effort.max() <= 54.0 and len(np.unique(effort)) > W
    else:
        effort = np.tile(np.float32([sim.joint_dynamics(d, [0])[0, 2] for d in range(n)]), (W, 1))
        assert (effort == 60.0).all()
    rng = np.random.default_rng(22)
    qd_prev = np.zeros((W, n), np.float32)
    clamped = np.zeros(2, int)
    worst = 0.0
    seen = np.zeros(10, bool)
    for k in range(30):
        cmd = obs[:, env.obs_slices["command"]]
        q_before = sim.get("q").astype(np.float32)
        if position:
            a = (np.float32(STAND) + rng.uniform(-0.4, 0.4, (W, n))).astype(np.float32)
        else:
            a = rng.uniform(-90, 90, (W, n)).astype(np.float32)
        o, r, d, _ = env.step(_dev(env, a))
        obs = o.cpu().numpy()
        assert not d.cpu().numpy().any()
        tau, terms = env.torques.cpu().numpy(), env.reward_terms.cpu().numpy()
        # the torques, from what is not under test
        if position:
            err = (q_before - a).astype(np.float64)            # the PID's error, one float32 rounding
            u = np.clip(-P_GAIN * err, -CMD_MAX, CMD_MAX)
            ref = np.clip(u, -effort.astype(np.float64), effort.astype(np.float64))
            # q - target, p err and the (fused or exact) sum with the zero terms: three operations at most
            bound = 3 * U / (1 - 3 * U) * np.abs(P_GAIN * err)
            worst = max(worst, float((np.abs(tau - ref) / np.maximum(bound, 1e-30)).max()))
            assert (np.abs(tau - ref) <= bound).all()
            clamped += [int((np.abs(-P_GAIN * err) > effort).sum()), int((np.abs(-P_GAIN * err) > CMD_MAX).sum())]
        else:
            np.testing.assert_array_equal(tau, np.clip(a, -effort, effort))
            clamped += [int((np.abs(a) > effort).sum()), 0]
        assert (np.abs(tau) <= effort).all()
        # the terms, through the host build of the same expressions
        q, qd, pose = sim.get("q").astype(np.float32), sim.get("qd").astype(np.float32), sim.base_pose()
        for w in range(W):
            cf, pf = _forces32(sim, w, env.contact_links), _forces32(sim, w, env.penalised_links)
            standing = fs.standing(cmd[w, 0], cmd[w, 1], LOCO_EVERY_TERM["cmd_min"])
            _, expect = fs.world(par, tau[w], q[w], qd[w], qd_prev[w], lo, hi, env.home_q, cf, pf, pose[w], standing)
            np.testing.assert_array_equal(terms[w], expect, err_msg=f"step {k}, world {w}")
        seen |= (terms < 0).any(axis=0)
        qd_prev = qd
    assert clamped[0] > 0, "the effort clamp never acted"
    if position:
        assert clamped[1] > 0, "the PID's own clamp never acted"
        print(f"{case}: worst torque error / bound {worst:.3f}; {clamped[0]} effort and {clamped[1]} command clamps")
    assert seen[[0, 1, 2, 3, 4, 5, 8, 9]].all(), seen
    env.close()


# Legs stretched out level with the trunk (hips at their limit, knees straight), the base pitched by a quarter
# of a radian and dropped from 0.25 m under no torque: the feet of the low end land first and carry the robot
# alone for a while, then the trunk comes down, each world at its own pace -- between physics steps 173 and 193
# on the device, found by stepping a plain env of this posture (no folded-leg posture works: the feet keep the
# trunk off the ground in all of them).  Two physics steps per control step, so that the contacts the env sees
# are those of a run's last physics step.
FALL = dict(action_mode="torque", home_q=[1.5, 0.0] * 4,
            home_base=(0.0, 0.0, 0.25, math.cos(-0.125), 0.0, math.sin(-0.125), 0.0), joint_noise=0.05, seed=9,
            max_episode_steps=0, pid_gains=None, steps_per_run=2, **FREE)


def test_contact_termination(require_gpu):
    """Height and tilt are disabled, so only the trunk's contact can end an episode."""
    kw = FALL
    force = 1.0
    env = _make("quadruped", W, termination_links=("trunk",), termination_force=force, **kw)
    never = _make("quadruped", W, reward_terms={"torque": 1e-5}, termination_links=(), **kw)
    assert env.termination_links == [-1] and never.termination_links == []
    home = env.reset().cpu().numpy()
    never.reset()
    zero = _dev(env, np.zeros((W, 8)))
    first = np.zeros(W, int)
    feet_only = 0
    for k in range(1, 201):
        o, r, d, info = env.step(zero)
        _, _, dn, _ = never.step(zero)
        assert not dn.cpu().numpy().any(), k
        o, r, d = o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy().astype(bool)
        expect = np.zeros(W, bool)
        for w in range(W):
            c, b = env.sim.contacts(w), env.sim.contact_bodies(w)
            norms = np.sqrt((c[b == -1, 6:9] ** 2).sum(axis=1))
            expect[w] = bool((norms > force).any())
            feet_only += int(len(c) > 0 and not (b == -1).any())
        np.testing.assert_array_equal(d, expect, err_msg=f"done at step {k}: a missed or an early termination")
        hit = np.flatnonzero(d)
        term = info["terminal_obs"].cpu().numpy()
        # terminated, not truncated: no alive bonus (w_forward v_x alone); alive worlds keep it
        np.testing.assert_array_equal(r[hit], term[hit, 7])
        alive = np.flatnonzero(~d)
        np.testing.assert_array_equal(r[alive], (np.float32(1.0) + o[alive, 7]).astype(np.float32))
        # the world resets
        np.testing.assert_array_equal(o[hit, :7], home[hit, :7])
        np.testing.assert_array_equal(o[hit, 7:13], 0.0)
        first[hit] = np.where(first[hit] == 0, k, first[hit])
        if (first > 0).all() and k >= first.max() + 5:
            break
    print(f"trunk contact ended the first episodes at steps {first.min()}..{first.max()} "
          f"({len(set(first.tolist()))} different ones); {feet_only} world-steps with the feet alone on the ground")
    assert (first > 0).all(), "the trunk of some world did not reach the ground within 200 steps"
    assert feet_only > 0 and len(set(first.tolist())) > 1
    ep, _ = env.counters()
    assert (ep.cpu().numpy() >= 1).all()
    env.close()
    never.close()


def test_episode_statistics(require_gpu):
    H = 7
    terms_on = {k: v for k, v in ALL.items() if k not in ("collision", "stand_still")}
    env = _make("quadruped", W, seed=8, joint_noise=0.05, max_episode_steps=H, reward_terms=terms_on,
                termination_links=(), soft_limit=0.3, max_contact_force=5.0, stumble_ratio=0.2, **FREE)
    env.reset()
    rng = np.random.default_rng(23)
    ret, length, sums = np.zeros(W, np.float32), np.zeros(W, np.int32), np.zeros((W, 10), np.float32)
    ep = [t.cpu().numpy().copy() for t in (env.episode_return, env.episode_length, env.episode_terms)]
    assert all((e == 0).all() for e in ep)

    def step_and_check(k, expect_done):
        nonlocal ret, length, sums, ep
        a = (np.float32(STAND) + rng.uniform(-0.3, 0.3, (W, 8))).astype(np.float32)
        _, r, d, info = env.step(_dev(env, a))
        r, d = r.cpu().numpy(), d.cpu().numpy().astype(bool)
        terms = info["reward_terms"].cpu().numpy()
        assert d.all() == expect_done and d.any() == expect_done, k
        ret, length, sums = (ret + r).astype(np.float32), length + 1, (sums + terms).astype(np.float32)
        now = [t.cpu().numpy().copy() for t in (info["episode_return"], info["episode_length"], info["episode_terms"])]
        if expect_done:
            assert (now[1] == H).all()
            np.testing.assert_array_equal(now[0], ret)
            np.testing.assert_array_equal(now[2], sums)
            assert (now[2][:, [0, 1, 2, 4]] < 0).all()
            ret, length, sums = np.zeros(W, np.float32), np.zeros(W, np.int32), np.zeros((W, 10), np.float32)
        else:
            for got, kept in zip(now, ep):                    # worlds not done: the finished episode's values stay
                np.testing.assert_array_equal(got, kept)
        ep = now

    for k in range(1, 26):
        step_and_check(k, k % H == 0)
    # four steps into an episode: reset() starts the running sums over and leaves the finished episodes alone
    env.reset()
    for got, kept in zip((env.episode_return, env.episode_length, env.episode_terms), ep):
        np.testing.assert_array_equal(got.cpu().numpy(), kept)
    ret, length, sums = np.zeros(W, np.float32), np.zeros(W, np.int32), np.zeros((W, 10), np.float32)
    for k in range(1, H + 1):
        step_and_check(k, k == H)
    env.close()


def test_contact_step_is_the_episode_length(require_gpu):
    """The statistics of an episode that a contact ended: its length is the contact step."""
    kw = FALL
    env = _make("quadruped", W, termination_links=("trunk",), termination_force=1.0, **kw)
    env.reset()
    zero = _dev(env, np.zeros((W, 8)))
    ret, taken = np.zeros(W, np.float32), np.zeros(W, np.int32)
    finished = np.zeros(W, bool)
    for k in range(1, 201):
        _, r, d, _ = env.step(zero)
        r, d = r.cpu().numpy(), d.cpu().numpy().astype(bool)
        ret, taken = (ret + r).astype(np.float32), taken + 1
        if d.any():
            np.testing.assert_array_equal(env.episode_length.cpu().numpy()[d], taken[d])
            np.testing.assert_array_equal(env.episode_return.cpu().numpy()[d], ret[d])
            finished |= d
            ret[d], taken[d] = 0.0, 0
        if finished.all():
            break
    assert finished.all()
    env.close()


def test_icub(require_gpu, fs):
    """W = 5, 32 dofs, the feet lumped into the ankles' bodies by fixed joints.  The shipped model carries
    collision shapes on the soles alone, so they are the only links the two lists can name: with thresholds
    above the robot's weight a standing step reports no collision and no termination, with low ones both soles
    count; contact_force is recomputed from the soles' forces."""
    Wi = 5
    shape = dict(reward_terms={"torque": 1e-5, "collision": 1.0, "contact_force": 0.01, "joint_limits": 1.0},
                 termination_links=("l_foot", "r_foot"), penalised_links=("l_foot", "r_foot"), max_contact_force=20.0)
    env = _make("icub", Wi, max_episode_steps=0, termination_force=1e5, collision_force_min=1e5, **FREE, **shape)
    low = _make("icub", Wi, max_episode_steps=0, termination_force=1e5, collision_force_min=1.0, **FREE, **shape)
    names = env.sim.link_names
    assert env.termination_links == env.penalised_links == env.contact_links
    assert [names[i] for i in env.penalised_links] == ["l_ankle_2", "r_ankle_2"]      # the bodies the soles are part of
    with pytest.raises(RuntimeError, match="owns no contact slot"):
        _make("icub", Wi, termination_links=("root_link", "chest"))
    lo, hi = _limits(fs, env.sim, 0.9)
    par = _params(fs, env, dict(shape, collision_force_min=1e5, termination_force=1e5))
    for e in (env, low):
        e.reset()
    a = _dev(env, np.tile(env.home_q, (Wi, 1)))
    qd_prev = np.zeros((Wi, 32), np.float32)
    w8 = float(np.float32(0.01))
    loaded = 0
    for k in range(120):                                 # as long as test_twin_parity_position_icub stands
        _, _, d, _ = env.step(a)
        _, _, dl, _ = low.step(a)
        assert not d.cpu().numpy().any() and not dl.cpu().numpy().any()
        terms, tau = env.reward_terms.cpu().numpy(), env.torques.cpu().numpy()
        np.testing.assert_array_equal(terms[:, 6], 0.0)
        q, qd, pose = (env.sim.get("q").astype(np.float32), env.sim.get("qd").astype(np.float32), env.sim.base_pose())
        for w in range(Wi):
            cf = _forces32(env.sim, w, env.contact_links)
            _, expect = fs.world(par, tau[w], q[w], qd[w], qd_prev[w], lo, hi, env.home_q, cf, cf, pose[w])
            np.testing.assert_array_equal(terms[w], expect, err_msg=f"step {k}, world {w}")
            # ... and written out in float64: the soles pressed with more than 1 N, their force beyond the limit
            norms = np.sqrt((cf.astype(np.float64) ** 2).sum(axis=1))
            assert low.reward_terms.cpu().numpy()[w, 6] == -float((norms > 1.0).sum())
            excess = np.maximum(0.0, norms - 20.0).sum()
            assert abs(terms[w, 8] + w8 * excess) <= 8 * U * w8 * (excess + norms.sum())
            loaded += int(excess > 0.0)
        qd_prev = qd
    assert loaded > 0, "no sole ever carried more than max_contact_force"
    env.close()
    low.close()


def test_graph_capture_and_defaults(require_gpu):
    import torch
    K = 20
    kw = dict(joint_noise=0.05, seed=4, max_episode_steps=6, **FREE, **LOCO_EVERY_TERM, **SHAPE)
    rng = np.random.default_rng(8)
    acts = (np.float32(STAND) + rng.uniform(-0.2, 0.2, (K + 1, W, 8))).astype(np.float32)
    outputs = ("obs", "reward", "done", "reward_terms", "torques", "episode_return", "episode_length", "episode_terms")
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
        got = {name: getattr(env, name).cpu().numpy().copy() for name in outputs}
        state = env.sim.get_state()
        types, edges = _captured_step_graph(env, a)
        side.synchronize()
    plain = _make("quadruped", W, **kw)
    plain.reset()
    for k in range(K + 1):
        plain.step(torch.from_numpy(acts[k]).to(plain.device))
    np.testing.assert_array_equal(state, plain.sim.get_state())
    for name in outputs:
        np.testing.assert_array_equal(got[name], getattr(plain, name).cpu().numpy(), err_msg=name)
    assert (got["episode_length"] == 6).all() and (got["episode_return"] != 0).all()
    assert types == [0, 0, 0] and len(edges) == 2    # still three kernel nodes in one chain
    env.close()
    plain.close()
    # without a shaping keyword the env is as it was
    bare = _make("quadruped", 4)
    for name in ("reward_term_names", "reward_terms", "torques", "episode_return", "episode_length", "episode_terms",
                 "termination_links", "penalised_links"):
        assert getattr(bare, name) is None, name
    bare.reset()
    _, _, _, info = bare.step(torch.zeros((4, 8), dtype=torch.float32, device=bare.device))
    assert set(info) == {"terminal_obs"}
    bare.close()
    # the quadruped's default once shaping is in use: it ends on its trunk
    auto = _make("quadruped", 4, reward_terms={"torque": 1e-5})
    assert auto.termination_links == [-1] and auto.penalised_links == []
    assert set(auto._info) == {"terminal_obs", "reward_terms", "torques", "episode_return", "episode_length",
                               "episode_terms"}
    auto.close()


def test_latency_interplay(require_gpu):
    """Torque mode under a fixed delay of two control steps: the torque of step t is the clamped action of
    step t - 2, and zero on the first two steps of an episode."""
    H, delay = 7, 2
    env = _make("quadruped", W, action_mode="torque", pid_gains=None, home_base=(0, 0, 0.47, 1, 0, 0, 0), seed=12,
                max_episode_steps=H, action_delay_range=(delay, delay), reward_terms={"torque": 1e-5, "power": 1e-4},
                termination_links=(), **FREE)
    env.reset()
    rng = np.random.default_rng(24)
    history = []
    for k in range(3 * H):
        a = rng.uniform(-90, 90, (W, 8)).astype(np.float32)
        history.append(a)
        env.step(_dev(env, a))
        t = k % H                                          # steps taken in the episode before this one
        expect = np.zeros((W, 8), np.float32) if t < delay else np.clip(history[k - delay], -60.0, 60.0)
        np.testing.assert_array_equal(env.torques.cpu().numpy(), expect, err_msg=f"step {k}")
        x = (expect.astype(np.float64) ** 2).sum(axis=1)
        got = env.reward_terms.cpu().numpy()[:, 0]
        w0 = float(np.float32(1e-5))
        assert (np.abs(got + w0 * x) <= 8 * U * w0 * x).all()      # 8 dofs: at most six roundings
        assert t < delay or (np.abs(history[k - delay]) > 60.0).any()
    env.close()
