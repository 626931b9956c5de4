"""Pushes, per-world ground friction, reward and observation words of the
floating-base env against the fp64 oracle (or_float_step_ext), not against a
twin simulator running the same kernel (test_gpu_float_rand.py).

  * one step of the wave kernel with world wrenches on the base and on one
    other link and a friction coefficient per world from 0 to 1.2, on the
    contact states of test_one_step_exact_lcp_random_states, accepted by that
    test's procedure (float_oracle_check.exact_lcp_acceptance); the same with
    the PGS sweeps alone against the oracle's PGS-50;
  * a closed-loop rollout of FloatVecEnv with strong pushes and low friction
    against one FloatWorld per world, replayed from the values the env reports
    (wrench of every step, friction of every episode, reset state);
  * the reward with all four weights and the world-velocity words of the
    observation, recomputed in float64.

Every test first asserts, on the reference alone, that its inputs exercise
what it is about (contacts, saturated friction, a wrench or a coefficient that
moves the state by 10x the bound).
"""

import math

import numpy as np
import pytest

from float_oracle_check import QD_TOL, exact_lcp_acceptance, oracle_step, quat_to_R, random_states

pytestmark = pytest.mark.gpu

MUS = [0.0, 0.05, 0.3, 0.8, 1.2]
# fp32 kernel vs fp64 oracle, one engine step of the same algorithm (test_gpu_float_tree.TOL)
TOL = dict(pose=1e-5, q=1e-5, point=1e-5, vel=2e-3, qd=2e-3, force=5e-3)
ULP = 2.0 ** -23


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _one_step_inputs(oracle, name, W, link):
    """The states of random_states (seed 11), one wrench per world on the base
    (force U(-60, 60) N, torque U(-5, 5) N m per axis: all six components) and
    one on `link` (U(-20, 20) N, U(-2, 2) N m), float32 values."""
    from mwstep import get_model_file
    cm = oracle.load_urdf(get_model_file(name))
    states = random_states(cm, W, np.random.default_rng(11))
    rng = np.random.default_rng(12)
    base_w = _f32(np.column_stack([rng.uniform(-60, 60, (W, 3)), rng.uniform(-5, 5, (W, 3))]))
    link_w = _f32(np.column_stack([rng.uniform(-20, 20, (W, 3)), rng.uniform(-2, 2, (W, 3))]))
    assert (base_w != 0).all() and (link_w != 0).all()
    return cm, states, {-1: base_w, link: link_w}


def _input_conditions(oracle, cm, start, tau, mus, wrenches, with_wrench, pgs_iters, label):
    """Properties of the reference alone (asserted): start = (pose, vel, q, qd)
    [W, ...]; with_wrench: {world: the oracle's FloatWorld after the step with
    the wrenches} of the worlds that have a reference.  Worlds in contact more
    than W // 4; among the contact points on mu > 0 that carry load (f_n > 0;
    an unloaded point, such as most of the iCub's redundant sole corners, has
    no friction for the coefficient to bound) at least a quarter near
    saturation (|f_t| >= 0.7 mu f_n); the wrenches move every world's q-dot or
    base twist by at least 10 QD_TOL."""
    W = len(tau)
    n_contact = n_all = n_pts = n_sat = 0
    moved = []
    for w, ow in with_wrench.items():
        n_contact += len(ow.contacts) > 0
        for (_, f, _, _) in ow.contacts:
            n_all += 1
            if mus[w] > 0 and f[2] > 0:
                n_pts += 1
                n_sat += math.hypot(f[0], f[1]) >= 0.7 * mus[w] * f[2]
        plain = oracle_step(oracle, cm, start[0][w], start[1][w], start[2][w], start[3][w], tau[w], mus[w], pgs_iters)
        moved.append(max(float(np.abs(ow.qd - plain.qd).max()), float(np.abs(ow.V - plain.V).max())))
    print(f"{label}: reference alone: {n_contact}/{W} worlds in contact, {n_sat}/{n_pts} loaded contact points on "
          f"mu > 0 near saturation ({n_all} contact points in all), the wrenches move qd / base twist by "
          f"{min(moved):.2e} .. {max(moved):.2e}")
    assert n_contact > W // 4
    assert 4 * n_sat >= n_pts > 0
    assert min(moved) >= 10 * QD_TOL
    return dict(n_contact=n_contact, n_pts=n_pts, n_sat=n_sat, moved=(min(moved), max(moved)))


def _one_step_sim(name, W, states, wrenches, friction, exact=True):
    """The simulator of the one-step tests after its step: friction = one
    coefficient (set_ground_plane, the scalar instance of the run kernel) or
    one per world (set_ground_friction, the per-world instance).  Returns
    (sim, start, end)."""
    from mwstep import get_model_file
    from mwstep import native as N
    from mwstep.sim import Simulator
    q, qd, pose, vel, tau = states
    sim = Simulator(get_model_file(name), n_worlds=W, pgs_iters=50)
    assert sim.float_kernel() == 2 and sim.lcp_solver() == (True, 48)
    if not exact:
        sim.set_lcp_solver(False)
    if np.ndim(friction) == 0:
        sim.set_ground_plane(True, float(friction))
    else:
        sim.set_ground_plane(True, 0.8)
        sim.set_ground_friction(friction)
    np.testing.assert_array_equal(sim.ground_friction(), np.broadcast_to(_f32(friction), (W,)))
    sim.enable_contacts(True)
    sim.set("reset_q", q)
    sim.set("reset_qd", qd)
    sim.reset_base_pose(pose)
    sim.reset_base_velocity(vel)
    sim.run(paused=True)
    start = (sim.base_pose(), sim.base_velocity(), sim.get("q"), sim.get("qd"))
    sim.set_control_mode(N.MODE_FORCE)
    sim.set("force_target", tau)
    for link, wr in wrenches.items():
        sim.apply_world_wrench(link, wr, sim.step_size)      # one run
    sim.run()
    end = (sim.base_pose(), sim.get("q"), sim.get("qd"), sim.get_state())
    return sim, start, end


# the iCub's W: the smallest from 40 up at which its reference meets the conditions of _input_conditions
@pytest.mark.parametrize("name, W, link, per_world", [("quadruped", 70, 3, True), ("icub", 40, 20, True),
                                                       ("quadruped", 70, 3, False)])
def test_one_step_wrench_and_friction_exact_lcp(require_gpu, oracle, monkeypatch, name, W, link, per_world):
    """One step of the wave kernel's default exact solve under world wrenches
    (base: all six components, which the env's own pushes never produce; one
    more link) and a ground friction per world cycling through 0, 0.05, 0.3,
    0.8, 1.2 -- or the single coefficient 0.05 through the scalar setter, so
    that both instances of the run kernel meet the oracle -- against
    or_float_step_ext's converged LCP, accepted exactly as
    test_one_step_exact_lcp_random_states accepts (q-dot 1e-4, q / pose 1e-5,
    anything else only as a valid fp64 LCP answer, none differing, 85 %
    agreeing outright, no unconverged world on the GPU).  mu = 0 makes the
    stage-2 friction boxes zero-width, 0.05 narrow."""
    monkeypatch.setenv("MWSTEP_WAVE_TREE", "1")
    cm, states, wrenches = _one_step_inputs(oracle, name, W, link)
    mus = np.array([MUS[w % len(MUS)] for w in range(W)]) if per_world else np.full(W, 0.05)
    sim, start, end = _one_step_sim(name, W, states, wrenches, mus if per_world else 0.05)
    label = f"{name} x{W}, wrenches, " + ("mu per world" if per_world else "mu 0.05")
    res = exact_lcp_acceptance(sim, oracle, cm, mus, states[4], start, end,
                               wrench=lambda w: {b: wr[w] for b, wr in wrenches.items()}, label=label)
    sim.close()
    assert len(res["no_ref"]) <= W // 20
    _input_conditions(oracle, cm, start, states[4], mus, wrenches, res["worlds"], oracle.PGS_CONVERGED, label)


def test_one_step_wrench_and_friction_pgs(require_gpu, oracle, monkeypatch):
    """The same quadruped step with the PGS sweeps alone (mw_set_lcp_solver
    PGS, 50 sweeps) against the oracle's PGS-50: the TOL table and the
    ill-conditioning rule of test_one_step_parity_with_contacts -- a world
    over the velocity or force tolerance is accepted only when the oracle
    itself moves as much under a 3e-7 perturbation of its inputs, and at most
    W // 20 worlds are."""
    monkeypatch.setenv("MWSTEP_WAVE_TREE", "1")
    name, W, link, pgs = "quadruped", 70, 3, 50
    cm, states, wrenches = _one_step_inputs(oracle, name, W, link)
    tau = states[4]
    mus = np.array([MUS[w % len(MUS)] for w in range(W)])
    sim, (p0, v0, gq0, gqd0), (p1, gq1, gqd1, _) = _one_step_sim(name, W, states, wrenches, mus, exact=False)
    v1 = sim.base_velocity()
    wrench_of = lambda w: {b: wr[w] for b, wr in wrenches.items()}

    def step(w, eps=0.0, seed=0):
        r = np.random.default_rng(seed)
        jig = (lambda a: a * (1.0 + eps * r.uniform(-1, 1, np.shape(a)))) if eps else None
        return oracle_step(oracle, cm, p0[w], v0[w], gq0[w], gqd0[w], tau[w], mus[w], pgs, wrench_of(w), jig)

    worst = dict.fromkeys(TOL, 0.0)
    ill, worlds = [], {}
    for w in range(W):
        ow = worlds[w] = step(w)
        e = dict(pose=max(float(np.abs(p1[w, :3] - ow.p).max()), float(np.abs(quat_to_R(p1[w, 3:]) - ow.R).max())),
                 q=float(np.abs(gq1[w] - ow.q).max()),
                 vel=float(np.abs(v1[w] - np.concatenate([ow.R @ ow.V[3:], ow.R @ ow.V[:3]])).max()),
                 qd=float(np.abs(gqd1[w] - ow.qd).max()), force=0.0, point=0.0)
        gc, gb = sim.contacts(w), sim.contact_bodies(w)
        assert len(gc) == len(ow.contacts)
        for row, body, (p, f, d, ob) in zip(gc, gb, ow.contacts):
            assert body == ob
            e["point"] = max(e["point"], float(np.abs(row[0:3] - p).max()))
            e["force"] = max(e["force"], float(np.abs(row[6:9] - f).max()) / (1.0 + float(np.abs(f).max())))
        if e["vel"] > TOL["vel"] or e["qd"] > TOL["qd"] or e["force"] > TOL["force"]:
            sens = max(float(np.abs(step(w, 3e-7, k).qd - ow.qd).max()) for k in range(4))
            ill.append((w, e["qd"], sens))
            assert sens >= 0.05 * e["qd"], f"world {w}: GPU-oracle |dqd| {e['qd']:.2e}, oracle sensitivity {sens:.2e}"
            assert e["q"] <= 2e-3 * e["qd"] + TOL["q"] and e["pose"] <= 2e-3 * e["vel"] + TOL["pose"]
            e.update(pose=0.0, q=0.0, vel=0.0, qd=0.0, force=0.0)
        for k in worst:
            worst[k] = max(worst[k], e[k])
    print(f"{name} x{W}, wrenches, mu per world, PGS-{pgs}: one-step " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + f", ill-conditioned: {[(w, f'{a:.1e}', f'{b:.1e}') for w, a, b in ill]}")
    assert sim.constraint_overflow() == 0
    sim.close()
    assert len(ill) <= W // 20
    assert all(worst[k] <= TOL[k] for k in TOL)
    _input_conditions(oracle, cm, (p0, v0, gq0, gqd0), tau, mus, wrenches, worlds, pgs, f"{name} PGS-{pgs}")


QUAD_PID = (400.0, 0.0, 10.0, 60.0)   # p, i, d, |cmd| limit: _stand_sim's gains, FloatVecEnv.quadruped's default


def _replay(oracle, cm, starts, push, target, sample, jig=None, push_scale=1.0, mu_scale=1.0, dt=1e-3):
    """One world of the env in the fp64 oracle: FloatWorld (converged LCP) under
    the JointController PID (pid_update on q - target, reset with the episode).
    starts: {k: (first observation row of the episode that step k opens, its
    friction coefficient)}, k = 0 and the step after every done; push
    [steps, 6] the world wrench on the base during each step; target
    [steps, n].  Returns {k: (q, base position) after k steps} for k in
    sample.  jig perturbs the reset states and the wrenches (the conditioning
    probe); push_scale / mu_scale: the signal checks."""
    n = cm.n
    jig = jig or (lambda a: a)
    p, i, d, lim = QUAD_PID
    gains = oracle.pid_gains(p, i, d, cmdmax=lim, cmdmin=-lim)
    mode = np.full(n, oracle.FORCE, np.int32)
    out, ow, st = {}, None, None
    for k in range(len(push)):
        if k in starts:
            row, mu = starts[k]
            row = np.asarray(row, dtype=np.float64)
            R = quat_to_R(row[3:7])
            ow = oracle.FloatWorld(cm, dt=dt, mu=float(mu) * mu_scale, pgs_iters=oracle.PGS_CONVERGED)
            ow.set_pose(jig(row[:3]), R)
            ow.set_twist(R.T @ row[10:13], R.T @ row[7:10])
            ow.set_joints(jig(row[13:13 + n]), jig(row[13 + n:13 + 2 * n]))
            st = [oracle.OrPidState() for _ in range(n)]
        ow.wrench[0] = jig(np.asarray(push[k], dtype=np.float64)) * push_scale
        q = ow.q
        tau = np.array([oracle.pid_update(gains, st[j], q[j] - float(target[k][j]), dt) for j in range(n)])
        ow.step(mode, tau)
        if k + 1 in sample:
            out[k + 1] = (ow.q, ow.p)
    return out


def _gap(a, b):
    """(largest |dq|, largest base position gap) between two replays / samples."""
    return (max(float(np.abs(a[k][0] - b[k][0]).max()) for k in a),
            max(float(np.abs(a[k][1] - b[k][1]).max()) for k in a))


def test_closed_loop_pushes_and_friction_against_fp64_replay(require_gpu, oracle):
    """FloatVecEnv.quadruped, W = 70 (two tiles, the second partial), position
    mode under _stand_sim's PID gains, 60 steps with a time limit of 30 (every
    world resets once inside the rollout), joint noise, pushes of up to 200 N /
    20 N m on 3 of every 7 steps, ground friction U(0.05, 0.3) per episode and
    joint targets swinging by 0.3 rad (the feet scrub the ground, so the
    coefficient decides how far they slide).  Each world is replayed in a
    FloatWorld of its own from three reported values -- the wrench of every
    step (env.push), the friction of every episode (env.friction), the first
    observation of every episode -- everything else is the oracle's: the
    friction drawn at a reset and the first push of the new episode must act
    from the right step on.  At every tenth step q agrees within 1e-4 and the
    base position within 1e-5 (test_standing_closed_loop_parity's bounds).

    A world outside the bounds is accepted only if its gap is within 10x the
    spread of four replays whose reset states and wrenches are perturbed by
    3e-7 relative (the kernel commits tens of fp32 roundings per step where
    the probe commits one per input), and at most W // 20 worlds may be.
    On the oracle alone: removing the pushes, and raising mu by 10 %, each
    move the compared state of every world by at least 10x its bound.

    Measured (MI355X): worst |dq| 2.4e-06 against 1e-4, worst base position
    gap 1.4e-07 against 1e-5, no world through the conditioning exit (the
    replay spread is 3e-7 in q, 1e-7 in position); the pushes move the
    compared state by 45x .. 707x its bound, the 10 % of friction by
    23x .. 426x (mu 0.057 .. 0.284, 1822 pushed world-steps)."""
    import torch
    from mwstep import FloatVecEnv, get_model_file
    W, H, steps, seed = 70, 30, 60, 31
    sample = set(range(10, steps + 1, 10)) | {steps}
    env = FloatVecEnv.quadruped(W, joint_noise=0.05, seed=seed, max_episode_steps=H, z_min=-10.0, max_tilt=math.pi,
                                friction_range=(0.05, 0.3), push_interval=7, push_steps=3, push_force=200.0,
                                push_torque=20.0)
    assert env.action_mode == "position" and env.sim.float_kernel() == 2
    cm = oracle.load_urdf(get_model_file("quadruped"))
    n = cm.n
    rng = np.random.default_rng(3)
    phase = rng.uniform(0, 2 * np.pi, (W, n))
    target = (env.home_q + 0.3 * np.sin(2 * np.pi * np.arange(steps)[:, None, None] / 30.0 + phase)).astype(np.float32)
    obs = env.reset().cpu().numpy()
    mu = env.friction.cpu().numpy()
    starts = [{0: (obs[w], mu[w])} for w in range(W)]
    mu_seen = [mu.copy()]
    push = np.zeros((steps, W, 6), np.float32)
    got = {}
    for k in range(steps):
        _, _, d, _ = env.step(torch.from_numpy(target[k]).to(env.device))
        push[k] = env.push.cpu().numpy()
        d = d.cpu().numpy().astype(bool)
        assert d.all() == ((k + 1) % H == 0) and d.any() == ((k + 1) % H == 0)
        if k + 1 in sample:      # a done step's reset reaches the simulator with the next run
            got[k + 1] = (env.sim.get("q"), env.sim.base_pose()[:, :3])
        if d.any() and k + 1 < steps:
            o, mu = env.obs.cpu().numpy(), env.friction.cpu().numpy()
            mu_seen.append(mu.copy())
            for w in range(W):
                starts[w][k + 1] = (o[w], mu[w])
    assert env.sim.lcp_unconverged() == 0 and env.sim.constraint_overflow() == 0
    env.close()
    assert len(mu_seen) == 2 and (mu_seen[0] != mu_seen[1]).all()
    pushed = (push != 0).any(axis=2)
    assert pushed[:H].any(axis=0).all() and pushed[H:].any(axis=0).all()     # every world, both episodes

    worst_q = worst_p = 0.0
    excused, spreads = [], []
    push_signal, mu_signal = [], []
    for w in range(W):
        mine = {k: (got[k][0][w], got[k][1][w]) for k in got}
        ref = _replay(oracle, cm, starts[w], push[:, w], target[:, w], sample)
        e_q, e_p = _gap(mine, ref)
        if e_q > 1e-4 or e_p > 1e-5:
            sp = []
            for s in range(4):
                r = np.random.default_rng(s)
                jig = lambda a: a * (1.0 + 3e-7 * r.uniform(-1, 1, np.shape(a)))
                sp.append(_gap(ref, _replay(oracle, cm, starts[w], push[:, w], target[:, w], sample, jig=jig)))
            s_q, s_p = max(x[0] for x in sp), max(x[1] for x in sp)
            spreads.append((w, s_q, s_p))
            assert e_q <= max(1e-4, 10 * s_q) and e_p <= max(1e-5, 10 * s_p), \
                f"world {w}: |dq| {e_q:.2e}, |dp| {e_p:.2e}; replay spread {s_q:.2e}, {s_p:.2e}"
            excused.append((w, f"{e_q:.1e}", f"{e_p:.1e}"))
        else:
            worst_q, worst_p = max(worst_q, e_q), max(worst_p, e_p)
        for scale, signal in ((dict(push_scale=0.0), push_signal), (dict(mu_scale=1.1), mu_signal)):
            g_q, g_p = _gap(ref, _replay(oracle, cm, starts[w], push[:, w], target[:, w], sample, **scale))
            signal.append(max(g_q / 1e-4, g_p / 1e-5))
    print(f"closed loop, pushes + friction, {W} worlds x {steps} steps: worst |dq| {worst_q:.2e}, base position "
          f"{worst_p:.2e}; through the conditioning exit {excused} (spreads {spreads}); on the oracle alone the "
          f"pushes move the compared state by {min(push_signal):.0f}x .. {max(push_signal):.0f}x its bound, "
          f"mu + 10 % by {min(mu_signal):.0f}x .. {max(mu_signal):.0f}x; mu {mu_seen[0].min():.3f} .. "
          f"{mu_seen[0].max():.3f}, {int(pushed.sum())} pushed world-steps")
    assert min(push_signal) >= 10 and min(mu_signal) >= 10
    assert len(excused) <= W // 20
    assert worst_q <= 1e-4 and worst_p <= 1e-5


def _reward_env(kind):
    from mwstep import FloatVecEnv
    if kind == "quadruped":
        # torque mode from the standing pose: the legs fold under random torques, the
        # trunk sinks through z_min after 70-odd steps in some worlds and not in others
        return FloatVecEnv.quadruped(70, action_mode="torque", pid_gains=None, joint_noise=0.05, seed=41,
                                     max_episode_steps=80, z_min=0.4195, max_tilt=math.pi, alive_bonus=1.0,
                                     w_forward=2.0, w_action=0.01, w_pose=0.5)
    # position mode, targets jittering about the posture: the humanoid sags at its own pace in every world
    return FloatVecEnv.icub(5, joint_noise=0.05, seed=41, max_episode_steps=60, z_min=0.560, max_tilt=math.pi,
                            alive_bonus=1.0, w_forward=2.0, w_action=0.1, w_pose=2.0)


@pytest.mark.parametrize("kind", ["quadruped", "icub"])
def test_reward_and_velocity_words_against_fp64(require_gpu, kind):
    """All four reward weights non-zero, random actions, a time limit that
    ends episodes inside the run and a z_min that ends some earlier: the
    quadruped in torque mode (W = 70: two tiles, the second partial; n = 8)
    and the iCub in position mode (W = 5, n = 32, obs_dim 79 > 64).

    Reward: recomputed in float64 for every step and world from the float32
    action row and the observation before the reset (terminal_obs where done,
    else obs): alive [not terminated] + w_f v_x - w_a sum a^2 - w_p sum (q -
    home)^2, terminated = z < z_min, known from that observation alone -- the
    alive bonus is absent exactly where the env terminated and present where
    only the time limit ended the episode.  Bound, derived: (n + 8) 2^-23
    (|alive| + |w_f v_x| + w_a sum a^2 + w_p sum e^2) -- n sequential fp32
    additions of non-negative terms, the roundings of the squares and of the
    subtraction, three more operations, a factor 2 of headroom; fma
    contraction only helps.
    Observation: the world-velocity words recomputed in float64 from the body
    twist and quaternion of the simulator's own record (mw_get_state, whose
    float32 words the other observation words must equal bit for bit), within
    2e-6 max(1, |x|).
    Measured (MI355X): reward error / bound 0.08 (quadruped), 0.02 (iCub);
    velocity words 6.4e-08 and 2.0e-07 against 2e-6; the quadruped ends 57
    episodes by height (2 in the partial tile) and 13 by the time limit (4),
    the iCub 1 and 4; every world has all four terms above 100x the bound on
    at least half its steps."""
    import torch
    env = _reward_env(kind)
    W, n, NO = env.n_worlds, env.action_dim, env.obs_dim
    assert (n, NO) == ((8, 33) if kind == "quadruped" else (32, 79))
    steps, H = 100, (80 if kind == "quadruped" else 60)
    z_min = np.float32(0.4195 if kind == "quadruped" else 0.560)
    alive, w_f, w_a, w_p = (float(np.float32(v)) for v in
                            ((1.0, 2.0, 0.01, 0.5) if kind == "quadruped" else (1.0, 2.0, 0.1, 2.0)))
    home = env.home_q.astype(np.float64)
    rng = np.random.default_rng(7)
    if kind == "quadruped":
        acts = rng.uniform(-5, 5, (steps, W, n)).astype(np.float32)
    else:
        acts = (env.home_q + rng.uniform(-0.1, 0.1, (steps, W, n))).astype(np.float32)
    env.reset()
    in_episode = np.zeros(W, np.int64)
    worst_r = worst_v = 0.0
    n_term, n_limit = np.zeros(W, np.int64), np.zeros(W, np.int64)
    big = np.zeros((steps, W), bool)       # every reward term above 100x the bound
    for k in range(steps):
        o, r, d, info = env.step(torch.from_numpy(acts[k]).to(env.device))
        o, r, d = o.cpu().numpy(), r.cpu().numpy().astype(np.float64), d.cpu().numpy().astype(bool)
        pre = np.where(d[:, None], info["terminal_obs"].cpu().numpy(), o)
        in_episode += 1
        # the record of the simulator is still the finished episode's last state
        rec = env.sim.get_state()
        base = rec[:, 7 * n:7 * n + 13]
        np.testing.assert_array_equal(pre[:, :7], base[:, :7])
        np.testing.assert_array_equal(pre[:, 13:13 + 2 * n], rec[:, :2 * n])
        b = base.astype(np.float64)
        for w in range(W):
            R = quat_to_R(b[w, 3:7])
            v = np.concatenate([R @ b[w, 10:13], R @ b[w, 7:10]])
            worst_v = max(worst_v, float((np.abs(pre[w, 7:13] - v) / np.maximum(1.0, np.abs(v))).max()))
        term = pre[:, 2] < z_min
        np.testing.assert_array_equal(d, term | (in_episode == H), err_msg=f"done at step {k + 1}")
        a2 = (acts[k].astype(np.float64) ** 2).sum(axis=1)
        e2 = ((pre[:, 13:13 + n].astype(np.float64) - home) ** 2).sum(axis=1)
        terms = np.column_stack([np.where(term, 0.0, alive), w_f * pre[:, 7].astype(np.float64), -w_a * a2, -w_p * e2])
        bound = (n + 8) * ULP * np.abs(terms).sum(axis=1)
        worst_r = max(worst_r, float((np.abs(r - terms.sum(axis=1)) / bound).max()))
        above = np.abs(terms) > 100 * bound[:, None]
        above[:, 0] |= term                # no alive term where terminated
        big[k] = above.all(axis=1)
        n_term += d & term
        n_limit += d & ~term
        in_episode[d] = 0
    env.close()
    tile = slice(64 * ((W - 1) // 64), W)      # the partial tile
    strong = int((big.mean(axis=0) >= 0.5).sum())
    print(f"{kind} x{W}, {steps} steps: reward error / bound {worst_r:.2f}, velocity words {worst_v:.2e}; terminated "
          f"{int(n_term.sum())} (partial tile {int(n_term[tile].sum())}), time limit {int(n_limit.sum())} (partial "
          f"tile {int(n_limit[tile].sum())}); {strong}/{W} worlds with every reward term > 100x the bound on at "
          f"least half their steps")
    assert n_term[tile].sum() >= 1 and n_limit[tile].sum() >= 1
    assert 2 * strong >= W
    assert worst_r <= 1.0
    assert worst_v <= 2e-6
