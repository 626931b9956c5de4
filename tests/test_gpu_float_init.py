"""FloatVecEnv's initial-state randomisation and reset-state bank
(mw_floatenv_init_state) on the GPU, against the fp64 restatement of
tests/float_init_ref.py and the yardsticks of the other env tests: the draws
are the stated Philox words, the reported start state is the base row plus the
reported draws, the simulator holds that state at once, a host-commanded twin
reset from the reset rows stays bit-equal across auto-resets, the bank is read
through its pointer at every reset, the locomotion rows, the joint_acc term and
the clean rows see the drawn state, and a step is still three kernel nodes.

Bounds: a uniform draw within 4 2^-23 (hi - lo) of fp64 (_check_draws' bound);
sums of a row word and a reported draw are one float32 rounding, so bit for bit;
the composed quaternion within 2e-6 per composed factor (see
test_float_init_host.py); quaternion-derived words within 2e-6 max(1, |x|)."""

import numpy as np
import pytest

import float_init_ref as R
from float_env_harness import (FREE, JOINTS, LOCO, PUSH, _captured_step_graph, _dev, _f, _make, _reset_twin, _twin)

pytestmark = pytest.mark.gpu

W, NQ = 70, 8                                        # one full tile and a partial one; the quadruped's dofs
NS = 13 + 2 * NQ
POS = ((-0.2, 0.2), (-0.1, 0.1), (0.1, 0.2))         # the base only ever lifted: the feet stay above the ground
RPY = ((-0.2, 0.2), (-0.15, 0.15), (-3.1, 3.1))
LIN = ((-0.5, 0.5), (-0.3, 0.3), (-0.1, 0.1))
ANG = ((-1.0, 1.0), (-0.5, 0.5), (-0.8, 0.8))
JV = 0.7
INIT = dict(init_pos_range=POS, init_rpy_range=RPY, init_lin_vel_range=LIN, init_ang_vel_range=ANG, init_joint_vel=JV)
REF = dict(pos=POS, rpy=RPY, lin=LIN, ang=ANG, joint_vel=JV)
ALL_GROUPS = R.POS | R.RPY | R.LIN | R.ANG
TORQUE = dict(action_mode="torque", pid_gains=None)


def _np(t):
    return t.cpu().numpy()


def _check_reported(oracle, env, seed, episode, worlds, ref_kw, offset=0):
    """env.init_draws of `worlds` against the restatement; returns the worst error / bound."""
    n = env.action_dim
    draws = _np(env.init_draws)
    assert draws.shape == (env.n_worlds, 13 + n)
    tol = R.draw_tols(n, **{k: v for k, v in ref_kw.items() if k in ("pos", "rpy", "lin", "ang", "joint_vel")})
    worst = 0.0
    for w in worlds:
        ref = R.draws_ref(oracle, seed, offset + int(w), int(episode[w]) if np.ndim(episode) else episode, n, **ref_kw)
        err = np.abs(draws[w].astype(np.float64) - ref)
        assert (err[tol == 0] == 0).all(), (w, err[tol == 0])
        worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0)
    return worst


def test_draws_and_state(require_gpu, oracle):
    from test_gpu_float_env import _reset_ref
    seed, noise = 17, 0.05
    kw = dict(joint_noise=noise, seed=seed, **TORQUE, **FREE)
    env = _make("quadruped", W, **kw, **INIT)
    assert env.init_states is None and env.init_state.shape == (W, NS) and env.init_draws.shape == (W, 13 + NQ)
    obs = _np(env.reset())
    state, draws = _np(env.init_state), _np(env.init_draws)
    worst = _check_reported(oracle, env, seed, 0, range(0, W, 7), REF)
    print(f"init draws vs the restatement: worst error / bound {worst:.3f}")
    assert worst <= 1.0
    tol = R.draw_tols(NQ, **REF)
    bounds = [r for group in (POS, RPY, LIN, ANG) for r in group]
    for k, (lo, hi) in enumerate(bounds):
        assert lo - tol[k] <= draws[:, k].min() and draws[:, k].max() <= hi + tol[k], k
    assert -JV - tol[13] <= draws[:, 13:].min() and draws[:, 13:].max() <= JV + tol[13]
    np.testing.assert_array_equal(draws[:, 12], -1.0)                      # no bank: the home row
    assert all(len(np.unique(draws[:, k])) > 0.9 * W for k in list(range(12)) + [13, 13 + NQ - 1])
    # the state: base row plus the reported draws, one rounding each
    home = R.home_row(env.home_base, env.home_q)
    want = np.array([R.base_words32(home, draws[w], ALL_GROUPS) for w in range(W)])
    for sl in (slice(0, 3), slice(7, 13)):
        np.testing.assert_array_equal(state[:, sl].view(np.uint32), want[:, sl].view(np.uint32))
    np.testing.assert_array_equal(state[:, 13 + NQ:].view(np.uint32), draws[:, 13:].view(np.uint32))   # 0 + dv
    worst_q = 0.0
    for w in range(0, W, 7):
        ref = R.orientation_ref(draws[w, 3:6], home[3:7])
        worst_q = max(worst_q, float(np.abs(state[w, 3:7] - ref).max()) / R.quat_tol(draws[w, 3:6], home[3:7]))
    norm = float(np.abs(np.linalg.norm(state[:, 3:7].astype(np.float64), axis=1) - 1).max())
    print(f"init orientation from the reported draws: worst error / bound {worst_q:.3f}, worst |norm - 1| {norm:.2e}")
    assert worst_q <= 1.0 and norm <= R.NORM_TOL
    # the reset row is the observation of that state
    np.testing.assert_array_equal(obs[:, :NS].view(np.uint32), state.view(np.uint32))
    np.testing.assert_array_equal(obs[:, NS:], 0.0)                        # contact words
    # ... and the simulator holds it at once
    np.testing.assert_array_equal(env.sim.get("q").astype(np.float32), state[:, 13:13 + NQ])
    np.testing.assert_array_equal(env.sim.get("qd").astype(np.float32), state[:, 13 + NQ:])
    pose, vel = env.sim.base_pose(), env.sim.base_velocity()
    err_pose = float(np.abs(pose - state[:, :7]).max())
    err_vel = float((np.abs(vel - state[:, 7:13]) / np.maximum(1.0, np.abs(vel))).max())
    print(f"simulator after the reset: base pose {err_pose:.2e}, base velocity {err_vel:.2e}")
    assert err_pose <= 4 * 2.0 ** -23 and err_vel <= 2e-6
    # the joint positions are the draw of the env without the feature: the old blocks are untouched
    plain = _make("quadruped", W, **kw)
    q_plain = _np(plain.reset())[:, 13:13 + NQ]
    assert plain.init_state is None and plain.init_draws is None
    plain.close()
    np.testing.assert_array_equal(state[:, 13:13 + NQ].view(np.uint32), q_plain.view(np.uint32))
    ref_q = np.array([_reset_ref(oracle, env.sim, env.home_q, noise, seed, w, 0) for w in range(0, W, 7)])
    print(f"joint positions against _reset_ref: {int((state[::7, 13:13 + NQ] != ref_q).sum())} of {ref_q.size} words "
          f"differ")
    np.testing.assert_array_equal(state[::7, 13:13 + NQ].view(np.uint32), ref_q.view(np.uint32))
    assert np.abs(state[:, 13:13 + NQ] - env.home_q).max() > 0.01
    # a shard's draws do not depend on where it starts
    part = _make("quadruped", 35, world_offset=35, **kw, **INIT)
    np.testing.assert_array_equal(_np(part.reset()).view(np.uint32), obs[35:].view(np.uint32))
    np.testing.assert_array_equal(_np(part.init_state).view(np.uint32), state[35:].view(np.uint32))
    np.testing.assert_array_equal(_np(part.init_draws).view(np.uint32), draws[35:].view(np.uint32))
    part.close()
    env.close()


@pytest.mark.parametrize("kind", ["quadruped", "icub"])
def test_twin_parity_across_auto_resets(require_gpu, oracle, kind):
    """Torque mode on the quadruped, position mode on the iCub; episodes of 5
    steps, 12 steps: the twin, reset through the host setters from the reset
    rows of the done worlds, ends every step with a bit-equal state record."""
    from mwstep.models import icub_pid_gains
    nw, H, steps, seed = 5, 5, 12, 23
    init = dict(init_pos_range=((0, 0), (0, 0), (0.05, 0.1)), init_rpy_range=((-0.1, 0.1), (-0.1, 0.1), (-3.0, 3.0)),
                init_lin_vel_range=LIN, init_ang_vel_range=ANG, init_joint_vel=0.5)
    ref_kw = dict(pos=init["init_pos_range"], rpy=init["init_rpy_range"], lin=LIN, ang=ANG, joint_vel=0.5)
    if kind == "quadruped":
        env = _make(kind, nw, joint_noise=0.05, seed=seed, max_episode_steps=H, **TORQUE, **FREE, **init)
        twin, target, spread = _twin(env, kind), "force_target", 5.0
    else:
        env = _make(kind, nw, joint_noise=0.02, seed=seed, max_episode_steps=H, **FREE, **init)
        gains = [[p, 0.0, d, -80.0, 80.0, 0.0, 0.0, -1.0] for p, d in icub_pid_gains(env.sim.joint_names)]
        twin, target, spread = _twin(env, kind, gains), "position_target", 0.1
    n = env.action_dim
    rng = np.random.default_rng(4)
    obs = _np(env.reset())
    _reset_twin(twin, obs)
    twin.run(paused=True)
    np.testing.assert_array_equal(env.sim.get_state(), twin.get_state())
    state, draws = _np(env.init_state).copy(), _np(env.init_draws).copy()
    np.testing.assert_array_equal(obs[:, :13 + 2 * n], state)
    episode, worst = np.zeros(nw, np.int64), 0.0
    for k in range(1, steps + 1):
        a = rng.uniform(-spread, spread, (nw, n)).astype(np.float32)
        if kind == "icub":
            a += env.home_q
        o, _, d, info = env.step(_dev(env, a))
        twin.set(target, a.astype(np.float64))
        twin.run()
        np.testing.assert_array_equal(env.sim.get_state(), twin.get_state(), err_msg=f"state after step {k}")
        o, d = _np(o), _np(d).astype(bool)
        assert d.all() == (k % H == 0) and d.any() == (k % H == 0)
        assert info["init_state"] is env.init_state and info["init_draws"] is env.init_draws
        new_state, new_draws = _np(env.init_state), _np(env.init_draws)
        # both change where, and only where, an episode ended
        np.testing.assert_array_equal((new_state != state).any(axis=1), d, err_msg=f"init_state at step {k}")
        np.testing.assert_array_equal((new_draws != draws).any(axis=1), d, err_msg=f"init_draws at step {k}")
        if d.any():
            episode[d] += 1
            state, draws = new_state.copy(), new_draws.copy()
            np.testing.assert_array_equal(o[d][:, :13 + 2 * n], state[d])
            worst = max(worst, _check_reported(oracle, env, seed, episode, np.flatnonzero(d), ref_kw))
            _reset_twin(twin, o, np.flatnonzero(d))
    print(f"{kind}: twin bit-equal over {steps} steps, {int(episode.sum())} auto-resets; draws of the later episodes "
          f"vs the restatement {worst:.3f}")
    assert worst <= 1.0 and (episode == steps // H).all()
    env.close()
    twin.close()


def _bank(home_base, home_q, rows=3):
    """Distinct rows built on the host: quaternions that are not unit-scaled, velocities that are not zero."""
    rng = np.random.default_rng(8)
    n = len(home_q)
    bank = np.zeros((rows, 13 + 2 * n), np.float32)
    for k in range(rows):
        q = np.array([1.0, 0.1 * (k + 1), -0.05 * (k + 1), 0.3 * k])
        # (no word is -0.0: the device code is built without signed zeros, so that one may come back as +0.0)
        bank[k, :3] = [0.1 * (k + 1), -0.2 * (k + 1), home_base[2] + 0.05 * (k + 1)]
        bank[k, 3:7] = q / np.linalg.norm(q) * (0.5, 1.5, 2.0)[k % 3]
        bank[k, 7:13] = rng.uniform(-0.5, 0.5, 6)
        bank[k, 13:13 + n] = home_q + rng.uniform(-0.1, 0.1, n)
        bank[k, 13 + n:] = rng.uniform(-1.0, 1.0, n)
    return bank


def test_bank(require_gpu, oracle):
    import torch
    kw = dict(max_episode_steps=2, **TORQUE, **FREE)
    home_base, home_q = (0.0, 0.0, 0.45, 1.0, 0.0, 0.0, 0.0), np.float32([0.6, -1.2] * 4)
    host = _bank(home_base, home_q)
    K = len(host)
    assert len({row.tobytes() for row in host}) == K
    assert (np.abs(np.linalg.norm(host[:, 3:7], axis=1) - 1) > 0.1).all() and (host[:, 7:13] != 0).all()
    # probability 1, no draws: every world starts from its restated row, verbatim
    seed = 5
    env = _make("quadruped", W, seed=seed, init_states=torch.from_numpy(host).cuda(), **kw)
    obs = _np(env.reset())
    rows = np.array([R.row_ref(oracle, seed, w, 0, K, 1.0) for w in range(W)])
    assert set(rows.tolist()) == set(range(K))
    np.testing.assert_array_equal(_np(env.init_draws)[:, 12], rows.astype(np.float32))
    np.testing.assert_array_equal(_np(env.init_draws)[:, :12], 0.0)
    np.testing.assert_array_equal(_np(env.init_state).view(np.uint32), host[rows].view(np.uint32))
    np.testing.assert_array_equal(obs[:, :NS].view(np.uint32), host[rows].view(np.uint32))
    env.close()
    # probability 0.5: a seed, found on the CPU, under which both kinds of start and all three rows occur
    for seed in range(1, 50):
        rows = [np.array([R.row_ref(oracle, seed, w, e, K, 0.5) for w in range(W)]) for e in (0, 1)]
        counts = [[int((r == k).sum()) for k in range(-1, K)] for r in rows]
        if all(min(c) > 0 for c in counts):
            break
    assert all(min(c) > 0 for c in counts), counts
    print(f"bank at probability 0.5, seed {seed}: home / row 0 / 1 / 2 starts {counts[0]}, next episode {counts[1]}")
    bank = torch.from_numpy(host).cuda()
    env = _make("quadruped", W, seed=seed, init_states=bank, init_state_prob=0.5, **kw)
    assert env.init_states is bank
    home = R.home_row(env.home_base, env.home_q)
    table = np.concatenate([host, home[None]])                              # index -1: the home row
    obs = _np(env.reset())
    np.testing.assert_array_equal(_np(env.init_draws)[:, 12], rows[0].astype(np.float32))
    np.testing.assert_array_equal(_np(env.init_state).view(np.uint32), table[rows[0]].view(np.uint32))
    # a row overwritten between two steps shows in the next reset that selects it
    zero = _dev(env, np.zeros((W, NQ)))
    env.step(zero)
    changed = host.copy()
    changed[1, :3] += np.float32([0.5, 0.25, 0.125])
    changed[1, 13 + NQ:] = 0.25
    bank[1].copy_(torch.from_numpy(changed[1]).cuda())
    _, _, d, _ = env.step(zero)
    assert _np(d).all()
    table = np.concatenate([changed, home[None]])
    np.testing.assert_array_equal(_np(env.init_draws)[:, 12], rows[1].astype(np.float32))
    np.testing.assert_array_equal(_np(env.init_state).view(np.uint32), table[rows[1]].view(np.uint32))
    np.testing.assert_array_equal(_np(env.obs)[:, :NS].view(np.uint32), table[rows[1]].view(np.uint32))
    env.close()


def test_locomotion_rows_see_the_drawn_state(require_gpu):
    env = _make("quadruped", W, seed=3, joint_noise=0.05, **FREE, **LOCO, **INIT)
    obs = _np(env.reset()).astype(np.float64)
    state = _np(env.init_state).astype(np.float64)
    sl = env.obs_slices
    worst = 0.0
    for w in range(W):
        Rm = R.rotation(state[w, 3:7] / np.linalg.norm(state[w, 3:7]))
        want = np.concatenate([-Rm[2], Rm.T @ state[w, 7:10], Rm.T @ state[w, 10:13]])
        got = np.concatenate([obs[w, sl["gravity"]], obs[w, sl["body_velocity"]]])
        worst = max(worst, float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()))
    print(f"locomotion reset rows, gravity and body velocities vs fp64 from the drawn state: {worst:.2e}")
    assert worst <= 2e-6
    assert np.abs(obs[:, sl["body_velocity"]]).max() > 0.1                   # the start is not at rest
    np.testing.assert_array_equal(obs[:, sl["last_action"]], 0.0)
    np.testing.assert_array_equal(_np(env.command), obs[:, sl["command"]].astype(np.float32))
    env.close()


def test_joint_acc_starts_from_the_drawn_velocity(require_gpu):
    """Only joint_acc weighted, init_joint_vel > 0: the term of an episode's
    first step is -w sum ((qd_1 - qd_0) / dt)^2 with qd_0 the drawn velocities;
    a kept velocity of zero would charge the episode for its own start."""
    weight = 2.5e-7
    env = _make("quadruped", W, seed=6, max_episode_steps=3, reward_terms=dict(joint_acc=weight),
                termination_links=(), init_joint_vel=2.0, **TORQUE, **FREE)
    zero = _dev(env, np.zeros((W, NQ)))
    env.reset()
    dt = _f(env.sim.steps_per_run * env.sim.step_size)
    worst = worst_rest = 0.0
    for k in range(1, 5):
        qd0 = _np(env.init_state)[:, 13 + NQ:].astype(np.float64)
        first = k in (1, 4)                                                  # the steps that follow a reset
        _, _, d, _ = env.step(zero)
        assert _np(d).all() == (k == 3)
        if not first:
            continue
        qd1 = env.sim.get("qd").astype(np.float32).astype(np.float64)
        want = -_f(weight) * (((qd1 - qd0) / dt) ** 2).sum(axis=1)
        got = _np(env.reward_terms)[:, 2].astype(np.float64)
        worst = max(worst, float((np.abs(got - want) / np.abs(want)).max()))
        from_rest = -_f(weight) * ((qd1 / dt) ** 2).sum(axis=1)
        worst_rest = max(worst_rest, float((np.abs(got - from_rest) / np.abs(want)).min()))
    print(f"joint_acc of an episode's first step: relative error {worst:.2e} (bound {2.0 ** -23 * (NQ + 4):.2e}); from "
          f"rest it would be off by at least {worst_rest:.2e}")
    assert worst <= 2.0 ** -23 * (NQ + 4)
    env.close()


def test_clean_rows_are_the_start_state(require_gpu):
    noise = dict(base_position=0.01, base_orientation=0.01, joint_velocities=0.5, base_linear_velocity=0.1)
    env = _make("quadruped", W, seed=9, joint_noise=0.05, max_episode_steps=2, obs_noise=noise, **TORQUE, **FREE,
                **INIT)
    zero = _dev(env, np.zeros((W, NQ)))
    obs = _np(env.reset())
    np.testing.assert_array_equal(_np(env.clean_obs)[:, :NS].view(np.uint32), _np(env.init_state).view(np.uint32))
    assert (obs[:, :3] != _np(env.init_state)[:, :3]).any()
    first = _np(env.init_state).copy()
    env.step(zero)
    np.testing.assert_array_equal(_np(env.init_state), first)
    _, _, d, _ = env.step(zero)
    assert _np(d).all() and (_np(env.init_state) != first).any(axis=1).all()
    np.testing.assert_array_equal(_np(env.clean_obs)[:, :NS].view(np.uint32), _np(env.init_state).view(np.uint32))
    env.close()


def test_step_is_still_three_kernel_nodes(require_gpu):
    import torch
    home_q = np.float32([0.6, -1.2] * 4)
    bank = torch.from_numpy(_bank((0.0, 0.0, 0.45, 1.0, 0.0, 0.0, 0.0), home_q, rows=5)).cuda()
    everything = dict(joint_noise=0.05, friction_range=(0.3, 1.2), mass_scale_range=(0.8, 1.25), payload_range=(0.0, 2.0),
                      payload_box=(0.1, 0.08, 0.05), obs_noise=dict(base_position=0.01, joint_velocities=0.5),
                      action_delay_range=(0, 3), reward_terms=dict(torque=2e-5, joint_acc=2.5e-7, orientation=1.0),
                      action_scale=0.25, max_episode_steps=4, init_states=bank, init_state_prob=0.5,
                      **PUSH, **LOCO, **JOINTS, **INIT)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        env = _make("quadruped", W, seed=4, **everything)
        env.reset()
        a = _dev(env, np.zeros((W, NQ)))
        env.step(a)
        side.synchronize()
        types, edges = _captured_step_graph(env, a)
        side.synchronize()
    assert types == [0, 0, 0] and len(edges) == 2
    (a0, b0), (a1, b1) = edges                                               # one chain, whatever the node order
    assert {a0, b0, a1, b1} == {0, 1, 2} and a0 != b0 and a1 != b1 and (b0 == a1 or b1 == a0)
    env.close()
