#!/usr/bin/env python3
"""Overhead of the floating-base env's device layer (mwstep.FloatVecEnv).

For the iCub at 512 worlds and the quadruped at 4,096 worlds, in one process:

  env    a captured env.step: action kernel + the run + post kernel
  bare   a captured sim.run_device(1) of an identically configured Simulator
  floor  a captured chain of two one-element kernels (the cost of two more
         graph nodes; torch has no empty kernel, `t.add_(1)` on one float is
         the smallest it launches)

each replayed --replays times per window between HIP events on the stream,
the three graphs alternating over --rounds windows after a warm-up; the
medians are reported.  The two env kernels move about W (obs_dim + n) 4 bytes
(0.3 MB for the iCub case: far below a microsecond of HBM time), so launch
cost is all they should add; the expectation checked here is

  env - bare <= 1.25 x floor.

--randomize adds a fourth graph to the alternation, env_rand: the step of a
second env with pushes and friction randomisation on (mw_floatenv_randomize;
the run then takes the wave kernel's wrench path, and the env kernels move 28
more bytes per world), and reports env_rand - env.

--task locomotion adds env_loco to the alternation: the step of another env
with the velocity-command task on (mw_floatenv_locomotion: the LOCO instances
of both env kernels, 12 + n more observation words and the kept action row
per world), fed zero actions -- the home posture through action_scale, the
same physics as env -- and reports env_loco - env.

--inertia adds two envs with the inertia randomisation on
(mw_floatenv_inertia: the WPAR instances of the run kernel, which read every
world's own body block and base words, and the INERT instance of the post
kernel): env_wpar with mass_scale_range (1, 1), whose per-world records hold
the nominal words -- the same physics as env, so env_wpar - env is the cost of
the mechanism: distinct parameter lines per wave instead of one shared block
-- and env_inertia with real ranges, whose difference from env_wpar is the cost
of the dynamics of robots that differ.  No world resets inside the timed
windows (max_episode_steps 0), so the draw itself runs at reset() only.

--joints adds two envs with the joint randomisation on (mw_floatenv_joints:
the same WPAR instances of the run kernel reading every world's own body block,
and the JOINT instance of the post kernel): env_jnom with effort_scale_range
(1, 1) on one joint, whose records hold the nominal words -- the same physics
as env on the run kernel's per-world instance, so env_jnom - env is the cost of
the mechanism -- and env_joints with real ranges on the leg joints, whose
difference from env_jnom is the cost of the dynamics: the damped model's
second recursion and one friction row per moving masked joint.  No world
resets inside the timed windows, so the draw itself runs at reset() only.

--noise adds env_noise to the alternation: the step of another env with the
observation noise on every sensor group and an action delay of 0..3 steps
(mw_floatenv_noise: the post kernel's noisy write-out, one Philox block per
four words of obs plus the clean rows, and the DELAY instance of the action
kernel with its ring), fed the same home-posture targets -- the delayed and
the neutral command are both the home posture, so the run does the same work
-- and reports env_noise - env.

--shaping adds two envs to the alternation: env_sbase, the velocity-command
task as --task locomotion times it, and env_shape, the same with all ten
shaping terms weighted, a termination and a penalised link list and every
output buffer attached (mw_floatenv_shaping: the shaping branch of the post
kernel), both fed zero actions -- the same physics -- and reports env_shape -
env_sbase beside the bytes the branch moves per world and step, counted from
the kernel: per dof q, qd, the kept qd, the controller output and the effort
word read and the kept qd and the torque written (28 n), the contact mask
again (4), three force words per active contact slot and list that names its
link (12 S), the twelve running sums read and written (96) and the row of
terms (40).

--init adds two envs to the alternation whose episodes last INIT_EPISODE
steps, so that every world resets inside the timed windows: env_ibase, which
resets to the home state as env does, and env_init, the same with the
initial-state randomisation on (mw_floatenv_init_state: all four groups of
draws, the joint-velocity draws and a 256-row bank of perturbed home rows taken
with probability one half, both output buffers attached) -- the branch of the
post kernel's reset block that draws where an episode starts -- and reports
env_init - env_ibase.  The two do not run the same physics after a reset (that
is the feature), so the difference holds the run kernel's share too; the post
launch alone is timed by float_env_trace_probe.py --init.

--tracking adds env_track to the alternation: the step of another env with the
motion-clip tracking task on (mw_floatenv_tracking: the frame clocks, the
reference rows blended out of the clips into an LDS tile, the five errors and
terms, 3 + n more observation words, every output buffer attached) following
two looping clips of TRACK_FRAMES rows that hold the home state, at 2 / 3 frames
per control step and from drawn start frames, fed the home-posture targets --
the same physics as env -- and reports env_track - env beside the clip bytes a
world reads per step.

Not a bench.py leg.  Prints one JSON line per model."""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --randomize: a push of 5 steps every 50, and a new friction coefficient per episode
RANDOMIZE = dict(push_interval=50, push_steps=5, push_force=30.0, push_torque=5.0, friction_range=(0.5, 1.25))
# --task locomotion: commands redrawn every 100 steps, every reward term on
LOCOMOTION = dict(task="locomotion", command_ranges=((-1.0, 1.0), (-0.5, 0.5), (-1.0, 1.0)), cmd_interval=100,
                  cmd_zero_prob=0.1, cmd_min=0.1, w_lin_z=2.0, w_ang_xy=0.05, w_action_rate=0.01, w_air_time=1.0)
# --inertia: every link's mass within -20 % / +25 %, up to 5 kg on the base
INERTIA = dict(mass_scale_range=(0.8, 1.25), payload_range=(0.0, 5.0), payload_box=(0.1, 0.1, 0.05))
# --joints: up to 0.5 N m s/rad and 2 N m on the leg joints, 50 .. 100 % of the effort limit
JOINTS = dict(joint_damping_range=(0.0, 0.5), joint_friction_range=(0.0, 2.0), effort_scale_range=(0.5, 1.0))
JOINT_DOFS = {"quadruped": None,
              "icub": [f"{s}_{j}" for s in ("l", "r")
                       for j in ("hip_pitch", "hip_roll", "hip_yaw", "knee", "ankle_pitch", "ankle_roll")]}
# --noise: encoder- and IMU-sized amplitudes on every sensor group, 0..3 control steps of latency
NOISE = dict(obs_noise=dict(base_position=0.01, base_orientation=0.01, base_linear_velocity=0.1,
                            base_angular_velocity=0.05, joint_positions=0.01, joint_velocities=0.5, contacts=2.0),
             action_delay_range=(0, 3))
# --shaping: all ten terms; links that carry a collision shape (the iCub's soles are its only ones: their
# termination force is out of reach, so that no episode ends inside the timed windows)
SHAPING = dict(reward_terms=dict(torque=2e-5, power=1e-4, joint_acc=2.5e-7, orientation=1.0, base_height=10.0,
                                 joint_limits=5.0, collision=1.0, stumble=0.5, contact_force=0.01, stand_still=0.2),
               collision_force_min=0.1, stumble_ratio=5.0, max_contact_force=50.0)
SHAPING_LINKS = {"quadruped": dict(termination_links=("trunk",), penalised_links=("trunk",), termination_force=1.0),
                 "icub": dict(termination_links=("l_foot", "r_foot"), penalised_links=("l_foot", "r_foot"),
                              termination_force=1e6)}
# --init: every group of draws and the joint velocities, small enough that a 20-step episode stays upright
INIT_EPISODE = 20
INIT = dict(init_pos_range=((-0.2, 0.2), (-0.2, 0.2), (0.0, 0.02)), init_rpy_range=((-0.05, 0.05), (-0.05, 0.05), (-3.1, 3.1)),
            init_lin_vel_range=((-0.2, 0.2), (-0.2, 0.2), (-0.05, 0.05)),
            init_ang_vel_range=((-0.2, 0.2), (-0.2, 0.2), (-0.2, 0.2)), init_joint_vel=0.2, init_state_prob=0.5)
INIT_BANK_ROWS = 256
# --tracking: two looping clips of the home state, a blend between two rows at most steps
TRACK_FRAMES = 64
TRACK = dict(clip_loop=True, rsi_prob=1.0, obs_reference=True)
sys.path.insert(0, os.path.join(ROOT, "gym-ignition_amd", "python"))


def init_bank(torch, env, rows=INIT_BANK_ROWS, seed=0):
    """A bank of `rows` start states on the env's device: the home row with the
    joints within 0.05 rad of the home posture, moving at up to 0.1 rad/s."""
    import numpy as np
    n = env.action_dim
    rng = np.random.default_rng(seed)
    bank = np.zeros((rows, 13 + 2 * n), np.float32)
    bank[:, :7] = env.home_base
    bank[:, 13:13 + n] = env.home_q + rng.uniform(-0.05, 0.05, (rows, n))
    bank[:, 13 + n:] = rng.uniform(-0.1, 0.1, (rows, n))
    return torch.from_numpy(bank).to(env.device)


def home_clips(torch, env, frames=TRACK_FRAMES):
    """Two clips of `frames` rows on the env's device, every row the home row: following them is standing still."""
    import numpy as np
    n = env.action_dim
    row = np.zeros(13 + 2 * n, np.float32)
    row[:7] = env.home_base
    row[13:13 + n] = env.home_q
    return [torch.from_numpy(np.tile(row, (frames, 1))).to(env.device) for _ in range(2)]


def capture(torch, stream, fn, warm):
    with torch.cuda.stream(stream):
        for _ in range(warm):
            fn()
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            fn()
        graph.replay()
        stream.synchronize()
    return graph


def window(torch, stream, graph, replays):
    """Microseconds per replay over one window of `replays` replays."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        for _ in range(replays):
            graph.replay()
        e1.record(stream)
        stream.synchronize()
    return e0.elapsed_time(e1) * 1e3 / replays


def bare_sim(torch, env, model, stream):
    """A Simulator configured as the env's, holding the home posture."""
    import numpy as np
    from mwstep import get_model_file
    from mwstep import native as N
    from mwstep.sim import Simulator
    W, s = env.n_worlds, env.sim
    sim = Simulator(get_model_file(model), n_worlds=W, step_size=s.step_size, steps_per_run=s.steps_per_run,
                    pgs_iters=env.pgs_iters, pose=tuple(env.home_base.tolist()), stream=stream.cuda_stream)
    sim.set_ground_plane(True, 1.0)
    sim.enable_contacts(True)
    for d in range(sim.dofs):
        sim.set_pid(d, s.pid(d))
    sim.set("reset_q", np.tile(env.home_q.astype(np.float64), (W, 1)))
    sim.run(paused=True)
    sim.set_controller_period(s.step_size)
    sim.set_control_mode(N.MODE_POSITION)
    sim.set("position_target", np.tile(env.home_q.astype(np.float64), (W, 1)))
    return sim


def measure(torch, args, model, W):
    import numpy as np
    from mwstep import FloatVecEnv
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        env = getattr(FloatVecEnv, model)(W, max_episode_steps=0, z_min=-10.0)
        env.pgs_iters = 50 if model == "icub" else 20
        env.reset()
        actions = torch.from_numpy(np.tile(env.home_q, (W, 1))).to(env.device)
        sim = bare_sim(torch, env, model, stream)
        one = torch.zeros(1, device=env.device)

    def floor():
        one.add_(1.0)
        one.add_(1.0)

    graphs = {"env": capture(torch, stream, lambda: env.step_raw(actions.data_ptr()), args.warmup),
              "bare": capture(torch, stream, lambda: sim.run_device(1), args.warmup),
              "floor": capture(torch, stream, floor, args.warmup)}
    rand = None
    if args.randomize:
        # a second env with pushes and friction randomisation on, in the same alternation
        with torch.cuda.stream(stream):
            rand = getattr(FloatVecEnv, model)(W, max_episode_steps=0, z_min=-10.0, **RANDOMIZE)
            rand.reset()
        graphs["env_rand"] = capture(torch, stream, lambda: rand.step_raw(actions.data_ptr()), args.warmup)
    loco = None
    if args.task == "locomotion":
        with torch.cuda.stream(stream):
            loco = getattr(FloatVecEnv, model)(W, max_episode_steps=0, z_min=-10.0, **LOCOMOTION)
            loco.reset()
            zeros = torch.zeros((W, loco.action_dim), dtype=torch.float32, device=loco.device)
        graphs["env_loco"] = capture(torch, stream, lambda: loco.step_raw(zeros.data_ptr()), args.warmup)
    wpar = inert = None
    if args.inertia:
        with torch.cuda.stream(stream):
            wpar = getattr(FloatVecEnv, model)(W, max_episode_steps=0, z_min=-10.0, mass_scale_range=(1.0, 1.0))
            wpar.reset()
            inert = getattr(FloatVecEnv, model)(W, max_episode_steps=0, z_min=-10.0, **INERTIA)
            inert.reset()
        graphs["env_wpar"] = capture(torch, stream, lambda: wpar.step_raw(actions.data_ptr()), args.warmup)
        graphs["env_inertia"] = capture(torch, stream, lambda: inert.step_raw(actions.data_ptr()), args.warmup)
    jnom = joints = None
    if args.joints:
        with torch.cuda.stream(stream):
            jnom = getattr(FloatVecEnv, model)(W, max_episode_steps=0, z_min=-10.0, effort_scale_range=(1.0, 1.0),
                                               joint_rand_dofs=[0])
            jnom.reset()
            joints = getattr(FloatVecEnv, model)(W, max_episode_steps=0, z_min=-10.0, joint_rand_dofs=JOINT_DOFS[model],
                                                 **JOINTS)
            joints.reset()
        graphs["env_jnom"] = capture(torch, stream, lambda: jnom.step_raw(actions.data_ptr()), args.warmup)
        graphs["env_joints"] = capture(torch, stream, lambda: joints.step_raw(actions.data_ptr()), args.warmup)
    noisy = None
    if args.noise:
        with torch.cuda.stream(stream):
            noisy = getattr(FloatVecEnv, model)(W, max_episode_steps=0, z_min=-10.0, **NOISE)
            noisy.reset()
        graphs["env_noise"] = capture(torch, stream, lambda: noisy.step_raw(actions.data_ptr()), args.warmup)
    sbase = shaped = None
    if args.shaping:
        with torch.cuda.stream(stream):
            sbase = getattr(FloatVecEnv, model)(W, max_episode_steps=0, z_min=-10.0, **LOCOMOTION)
            sbase.reset()
            shaped = getattr(FloatVecEnv, model)(W, max_episode_steps=0, z_min=-10.0, **LOCOMOTION, **SHAPING,
                                                 **SHAPING_LINKS[model])
            shaped.reset()
            szeros = torch.zeros((W, shaped.action_dim), dtype=torch.float32, device=shaped.device)
        graphs["env_sbase"] = capture(torch, stream, lambda: sbase.step_raw(szeros.data_ptr()), args.warmup)
        graphs["env_shape"] = capture(torch, stream, lambda: shaped.step_raw(szeros.data_ptr()), args.warmup)
    ibase = started = None
    if args.init:
        with torch.cuda.stream(stream):
            ibase = getattr(FloatVecEnv, model)(W, max_episode_steps=INIT_EPISODE, z_min=-10.0)
            ibase.reset()
            started = getattr(FloatVecEnv, model)(W, max_episode_steps=INIT_EPISODE, z_min=-10.0,
                                                  init_states=init_bank(torch, env), **INIT)
            started.reset()
        graphs["env_ibase"] = capture(torch, stream, lambda: ibase.step_raw(actions.data_ptr()), args.warmup)
        graphs["env_init"] = capture(torch, stream, lambda: started.step_raw(actions.data_ptr()), args.warmup)
    tracked = None
    if args.tracking:
        with torch.cuda.stream(stream):
            fps = 2.0 / 3.0 / (env.sim.step_size * env.sim.steps_per_run)
            tracked = getattr(FloatVecEnv, model)(W, max_episode_steps=0, z_min=-10.0, clip_fps=fps,
                                                  motion_clips=home_clips(torch, env), **TRACK)
            tracked.reset()
        graphs["env_track"] = capture(torch, stream, lambda: tracked.step_raw(actions.data_ptr()), args.warmup)
    times = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for k, g in graphs.items():
            times[k].append(window(torch, stream, g, args.replays))
    med = {k: statistics.median(v) for k, v in times.items()}
    done = int(env.counters()[0].sum().item())
    z = env.sim.base_pose()[:, 2]
    excess = med["env"] - med["bare"]
    out = {"model": model, "n_worlds": W, "obs_dim": env.obs_dim, "action_dim": env.action_dim,
           "replays_per_window": args.replays, "rounds": args.rounds,
           "env_step_us": round(med["env"], 3), "bare_run_us": round(med["bare"], 3),
           "two_node_floor_us": round(med["floor"], 3), "excess_us": round(excess, 3),
           "excess_over_floor": round(excess / med["floor"], 3),
           "within_floor_plus_25pct": bool(excess <= 1.25 * med["floor"]),
           "spread_us": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
           "bytes_moved_by_env_kernels": W * (env.obs_dim + env.action_dim) * 4,
           "auto_resets_during_run": done, "base_z_range_after": [round(float(z.min()), 4), round(float(z.max()), 4)]}
    if rand is not None:
        pushed = int((rand.push != 0).any(dim=1).sum().item())
        out.update({"env_rand_step_us": round(med["env_rand"], 3),
                    "rand_minus_env_us": round(med["env_rand"] - med["env"], 3),
                    "randomize": RANDOMIZE, "worlds_pushed_in_last_step": pushed,
                    "friction_range_seen": [round(float(rand.friction.min()), 4), round(float(rand.friction.max()), 4)],
                    "extra_bytes_per_world": 28})
        rand.close()
    if loco is not None:
        zl = loco.sim.base_pose()[:, 2]
        out.update({"env_loco_step_us": round(med["env_loco"], 3),
                    "loco_minus_env_us": round(med["env_loco"] - med["env"], 3),
                    "loco_minus_env_over_floor": round((med["env_loco"] - med["env"]) / med["floor"], 3),
                    "loco_obs_dim": loco.obs_dim,
                    "loco_bytes_moved_by_env_kernels": W * (loco.obs_dim + 3 * loco.action_dim + 3) * 4,
                    "loco_base_z_range_after": [round(float(zl.min()), 4), round(float(zl.max()), 4)]})
        loco.close()
    if inert is not None:
        n = env.action_dim
        stride = 4 * (16 + 8 + 40 * n)
        zi = inert.sim.base_pose()[:, 2]
        same = bool((wpar.sim.get_state() == env.sim.get_state()).all())
        out.update({"env_wpar_step_us": round(med["env_wpar"], 3), "env_inertia_step_us": round(med["env_inertia"], 3),
                    "wpar_minus_env_us": round(med["env_wpar"] - med["env"], 3),
                    "inertia_minus_wpar_us": round(med["env_inertia"] - med["env_wpar"], 3),
                    "inertia": INERTIA, "wpar_state_equals_env_state": same,
                    "link_parameter_bytes_per_world": stride, "friction_bytes_per_world": 4,
                    "inertial_and_draw_output_bytes_per_world": 4 * (10 * (n + 1) + n + 5),
                    "base_mass_range": [round(float(inert.inertial[:, 0, 0].min()), 3),
                                        round(float(inert.inertial[:, 0, 0].max()), 3)],
                    "inertia_base_z_range_after": [round(float(zi.min()), 4), round(float(zi.max()), 4)]})
        wpar.close()
        inert.close()
    if joints is not None:
        n = env.action_dim
        zj = joints.sim.base_pose()[:, 2]
        same = bool((jnom.sim.get_state() == env.sim.get_state()).all())
        words = joints.joint_dynamics.cpu().numpy()
        out.update({"env_jnom_step_us": round(med["env_jnom"], 3), "env_joints_step_us": round(med["env_joints"], 3),
                    "jnom_minus_env_us": round(med["env_jnom"] - med["env"], 3),
                    "joints_minus_jnom_us": round(med["env_joints"] - med["env_jnom"], 3),
                    "joints": JOINTS, "joint_rand_dofs": JOINT_DOFS[model], "jnom_state_equals_env_state": same,
                    "link_parameter_bytes_per_world": 4 * (16 + 8 + 40 * n),
                    "joint_word_and_draw_output_bytes_per_world": 4 * 6 * n,
                    "friction_range_drawn": [round(float(words[:, :, 1].min()), 3), round(float(words[:, :, 1].max()), 3)],
                    "joints_constraint_overflow": int(joints.sim.constraint_overflow()),
                    "joints_base_z_range_after": [round(float(zj.min()), 4), round(float(zj.max()), 4)]})
        jnom.close()
        joints.close()
    if noisy is not None:
        zn = noisy.sim.base_pose()[:, 2]
        moved = int((noisy.obs != noisy.clean_obs).sum().item())
        delays = noisy.action_delay.cpu().numpy()
        ring = W * (NOISE["action_delay_range"][1] + 1) * env.action_dim * 4
        out.update({"env_noise_step_us": round(med["env_noise"], 3),
                    "noise_minus_env_us": round(med["env_noise"] - med["env"], 3),
                    "noise_minus_env_over_floor": round((med["env_noise"] - med["env"]) / med["floor"], 3),
                    "noise_share_of_step": round((med["env_noise"] - med["env"]) / med["env_noise"], 4),
                    "noise": {"obs_noise": NOISE["obs_noise"], "action_delay_range": list(NOISE["action_delay_range"])},
                    "noisy_words_in_last_obs": moved, "delays_drawn": sorted(set(delays.tolist())),
                    "noise_state_equals_env_state": bool((noisy.sim.get_state() == env.sim.get_state()).all()),
                    "clean_row_bytes_per_step": W * env.obs_dim * 4, "ring_bytes": ring,
                    "noise_base_z_range_after": [round(float(zn.min()), 4), round(float(zn.max()), 4)]})
        noisy.close()
    if shaped is not None:
        n = env.action_dim
        lists = [shaped.contact_links, shaped.penalised_links, shaped.termination_links]
        slots = sum(int((shaped.sim.contact_bodies(w)[:, None] == np.asarray(links)[None, :]).sum())
                    for w in range(min(W, 64)) for links in lists) / min(W, 64)
        terms = shaped.reward_terms.cpu().numpy()
        out.update({"env_sbase_step_us": round(med["env_sbase"], 3), "env_shape_step_us": round(med["env_shape"], 3),
                    "shape_minus_sbase_us": round(med["env_shape"] - med["env_sbase"], 3),
                    "shape_share_of_step": round((med["env_shape"] - med["env_sbase"]) / med["env_shape"], 4),
                    "shaping": {**SHAPING, **SHAPING_LINKS[model]},
                    "shape_state_equals_sbase_state": bool((shaped.sim.get_state() == sbase.sim.get_state()).all()),
                    "shape_active_slot_reads_per_world": round(slots, 2),
                    "shape_bytes_per_world_step": round(28 * n + 4 + 12 * slots + 96 + 40, 1),
                    "shape_terms_nonzero_columns": [int(k) for k in np.flatnonzero((terms != 0).any(axis=0))],
                    "shape_episodes_finished": int(shaped.counters()[0].sum().item())})
        sbase.close()
        shaped.close()
    if started is not None:
        n = env.action_dim
        draws = started.init_draws.cpu().numpy()
        zs = started.sim.base_pose()[:, 2]
        out.update({"env_ibase_step_us": round(med["env_ibase"], 3), "env_init_step_us": round(med["env_init"], 3),
                    "init_minus_ibase_us": round(med["env_init"] - med["env_ibase"], 3),
                    "ibase_minus_env_us": round(med["env_ibase"] - med["env"], 3),
                    "init": {k: v for k, v in INIT.items()}, "init_bank_rows": INIT_BANK_ROWS,
                    "init_episode_steps": INIT_EPISODE,
                    "init_episodes_finished": int(started.counters()[0].sum().item()),
                    "ibase_episodes_finished": int(ibase.counters()[0].sum().item()),
                    "init_bank_starts_in_last_episode": int((draws[:, 12] >= 0).sum()),
                    "init_output_bytes_per_world_and_reset": 4 * (13 + 2 * n + 13 + n),
                    "init_bank_bytes_read_per_bank_start": 4 * (13 + 2 * n),
                    "init_base_z_range_after": [round(float(zs.min()), 4), round(float(zs.max()), 4)]})
        ibase.close()
        started.close()
    if tracked is not None:
        n = env.action_dim
        errors = tracked.tracking_errors.cpu().numpy()
        out.update({"env_track_step_us": round(med["env_track"], 3),
                    "track_minus_env_us": round(med["env_track"] - med["env"], 3),
                    "track_share_of_step": round((med["env_track"] - med["env"]) / med["env_track"], 4),
                    "tracking": {**TRACK, "frames": TRACK_FRAMES, "clips": 2, "frames_per_step": list(tracked.clip_fraction)},
                    "track_obs_dim": tracked.obs_dim,
                    "track_state_equals_env_state": bool((tracked.sim.get_state() == env.sim.get_state()).all()),
                    "track_clip_bytes_read_per_world_step": 4 * (2 * (13 + 2 * n) + 2 * n),
                    "track_output_bytes_per_world_step": 4 * (5 + 5 + 3 + n),
                    "track_start_frames_drawn": len(set(tracked.track_frame.cpu().numpy().tolist())),
                    "track_largest_error": float(errors.max())})
        tracked.close()
    env.close()
    sim.close()
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--replays", type=int, default=2000, help="graph replays per timed window (>= 200)")
    p.add_argument("--rounds", type=int, default=5, help="windows per graph, the three graphs alternating")
    p.add_argument("--warmup", type=int, default=50, help="uncaptured calls before each capture")
    p.add_argument("--icub-worlds", type=int, default=512)
    p.add_argument("--quadruped-worlds", type=int, default=4096)
    p.add_argument("--randomize", action="store_true",
                   help="also time an env with pushes and friction randomisation on (env_rand)")
    p.add_argument("--inertia", action="store_true",
                   help="also time envs with per-world link parameters: nominal words (env_wpar) and real ranges "
                        "(env_inertia)")
    p.add_argument("--joints", action="store_true",
                   help="also time envs with per-world joint dynamics: nominal words (env_jnom) and real ranges "
                        "(env_joints)")
    p.add_argument("--noise", action="store_true",
                   help="also time an env with observation noise and action latency on (env_noise)")
    p.add_argument("--shaping", action="store_true",
                   help="also time the locomotion env without (env_sbase) and with (env_shape) the shaping terms, "
                        "contact termination and episode statistics")
    p.add_argument("--init", action="store_true",
                   help="also time envs whose worlds reset inside the windows: to the home state (env_ibase) and with "
                        "the initial-state randomisation and a 256-row bank on (env_init)")
    p.add_argument("--tracking", action="store_true",
                   help="also time an env that follows two looping clips of the home state (env_track)")
    p.add_argument("--task", choices=("forward", "locomotion"), default="forward",
                   help="locomotion: also time an env with the velocity-command task on (env_loco)")
    args = p.parse_args()
    if args.replays < 200:
        p.error("--replays must be >= 200")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_float_env.py needs the GPU: there is no CPU path to time")
    for model, W in (("icub", args.icub_worlds), ("quadruped", args.quadruped_worlds)):
        print(json.dumps(measure(torch, args, model, W)), flush=True)


if __name__ == "__main__":
    main()
