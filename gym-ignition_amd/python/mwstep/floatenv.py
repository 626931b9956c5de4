"""Batched, device-resident environment for floating-base robots with contacts.

``FloatVecEnv`` is the ``VecEnv`` of articulated models on a floating base (the
quadruped, the iCub-class humanoid, any tree of up to 48 bodies that the
world-per-wavefront kernel steps).  One ``step()`` is three launches on the
current stream -- actions to device commands, the simulator's own run, and
observation / reward / done / auto-reset -- with no host copy and no
synchronisation, so a step can be captured into a graph.

Observation, float32 ``[n_worlds, 13 + 2 n + n_contact_links]``: base position
(3), orientation wxyz (4), world linear (3) and angular (3) velocity, joint
positions and velocities, then per contact link the world z force (N) summed
over its contact points.  Auto-reset follows the ``VecEnv`` convention: where
``done`` is set, ``obs`` holds the first observation of the next episode and
``info["terminal_obs"]`` the last one of the finished episode; the simulator
itself takes the reset with the next step's run.

While the env exists it owns the simulator's joint commands and pending
resets: the host setters of ``env.sim`` that write them (``set("force_target"
| "position_target" | "reset_q" | ...)``, ``reset_base_pose``,
``set_control_mode``, ``set_pid``, ``set_state``) raise; the getters work.
With pushes on it also owns the simulator's wrench buffer
(``apply_world_wrench`` raises), with friction randomisation on the per-world
ground friction (``set_ground_friction`` / ``set_ground_plane`` raise,
``ground_friction()`` reads the device copy), with inertia or joint
randomisation on the per-world link parameters (``set_link_params``
and ``set_joint_dynamics`` raise, ``link_params()`` and ``joint_dynamics()``
read the device copy).

``task="locomotion"`` (``mw_floatenv_locomotion``) turns the env into a
velocity-command task, still three launches per step: every world follows a
command (v_x, v_y, yaw rate in the body frame) drawn on the device, the
observation grows by projected gravity (3), body-frame linear (3) and angular
(3) velocity, the command (3) and the last raw action (n) -- ``25 + 3 n +
n_contact_links`` words, ``env.obs_slices`` names them --, actions may be
scaled around the home posture, and the reward gains command-tracking,
vertical / roll-pitch velocity, action-rate and feet-air-time terms.

``obs_noise=`` and ``action_delay_range=`` (``mw_floatenv_noise``) give the
policy side of sim-to-real randomisation inside the same three launches:
per-word uniform noise on ``obs`` and ``terminal_obs`` with the clean rows kept
beside them (``env.clean_obs``), and a per-episode latency of up to 8 control
steps between an action and the command the simulator receives.

``reward_terms=``, ``termination_links=`` and ``penalised_links=``
(``mw_floatenv_shaping``) add, again inside the same three launches, the
regularisers that keep a learned gait physical -- joint torque, mechanical
power, joint acceleration, base orientation and height, joint limits,
collisions of non-foot links, stumbling, excessive foot forces, standing still
-- as ten signed reward columns (``env.reward_terms``), a termination on
contact of chosen links, and per-episode statistics of the finished episodes
(``env.episode_return``, ``env.episode_length``, ``env.episode_terms``).

``init_states=``, ``init_pos_range=``, ``init_rpy_range=``,
``init_lin_vel_range=``, ``init_ang_vel_range=`` and ``init_joint_vel=``
(``mw_floatenv_init_state``) vary where an episode starts, drawn by the launch
that issues the reset: from a row of a bank of recorded states or the home
state, plus offsets on the base pose, the base velocity and the joint
velocities (``env.init_state``, ``env.init_draws``).

``motion_clips=`` (``mw_floatenv_tracking``) makes the env a DeepMimic-style
imitation task, again inside the same three launches: every world follows a
clip of recorded states on an exact frame clock, its episodes start from a
frame of a clip drawn on the device (reference-state initialisation), and the
reward, the termination and the observation compare the state with the clip
(``env.tracking_terms``, ``env.tracking_errors``, ``env.track_clip``,
``env.track_frame``).
"""

from __future__ import annotations

import ctypes
import fractions
import math
import os
import xml.etree.ElementTree as ET
from collections.abc import Mapping
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import native as N
from .models import get_model_file
from .sim import Simulator

ACTION_MODES = {"torque": N.FLOAT_ACTION_TORQUE, "position": N.FLOAT_ACTION_POSITION}
TASKS = ("forward", "locomotion")
MAX_CONTACT_LINKS = 8
# the columns of env.reward_terms, in order (mw_float_shape_config::weights)
# the columns of env.tracking_terms and env.tracking_errors, in order (mw_float_track_config::weights)
TRACKING_TERMS = ("pose", "velocity", "root_pos", "root_rot", "root_vel")
TRACKING_WEIGHTS = dict(pose=0.5, velocity=0.05, root_pos=0.2, root_rot=0.15, root_vel=0.1)
TRACKING_SCALES = dict(pose=2.0, velocity=0.1, root_pos=10.0, root_rot=5.0, root_vel=1.0, ang_scale=0.1)
REWARD_TERMS = ("torque", "power", "joint_acc", "orientation", "base_height", "joint_limits", "collision", "stumble",
                "contact_force", "stand_still")


def _torch():
    import torch  # noqa: WPS433 (plumbing only: device memory + streams)
    return torch


def _ptr(t):
    """The device pointer of a tensor for the C layer; None (a feature that is off) stays None."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _iptr(a: np.ndarray):
    """An int32 list of the C layer; an empty one is passed as NULL."""
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if len(a) else None


def _fixed_parents(model: str) -> Dict[str, str]:
    """child link -> parent link of every fixed joint of a URDF (file or text):
    the model compiler lumps such a child into the body of its parent."""
    try:
        text = open(model).read() if os.path.exists(model) else model
        root = ET.fromstring(text.strip())
    except (OSError, ET.ParseError):
        return {}
    return {j.find("child").get("link"): j.find("parent").get("link")
            for j in root.findall("joint") if j.get("type") == "fixed"}


class FloatVecEnv:
    """``n_worlds`` copies of one floating-base robot stepped together on one GPU."""

    def __init__(self, model: str, n_worlds: int, action_mode: str = "position",
                 home_q: Optional[Sequence[float]] = None,
                 home_base: Sequence[float] = (0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0),
                 pid_gains: Optional[Sequence[Sequence[float]]] = None,
                 contact_links: Sequence = (), z_min: float = 0.0, max_tilt: float = math.pi,
                 alive_bonus: float = 1.0, w_forward: float = 1.0, w_action: float = 0.0,
                 w_pose: float = 0.0, joint_noise: float = 0.0, max_episode_steps: int = 1000,
                 seed: int = 42, world_offset: int = 0, step_size: float = 1e-3, steps_per_run: int = 1,
                 device: int = 0, pgs_iters: int = 20, ground_mu: float = 1.0,
                 push_interval: int = 0, push_steps: int = 1, push_force: float = 0.0, push_torque: float = 0.0,
                 friction_range: Optional[Sequence[float]] = None,
                 mass_scale_range: Optional[Sequence[float]] = None,
                 payload_range: Optional[Sequence[float]] = None,
                 payload_box: Sequence[float] = (0.0, 0.0, 0.0),
                 joint_damping_range: Optional[Sequence[float]] = None,
                 joint_friction_range: Optional[Sequence[float]] = None,
                 effort_scale_range: Optional[Sequence[float]] = None,
                 joint_rand_dofs: Optional[Sequence] = None,
                 task: str = "forward",
                 command_ranges: Sequence[Sequence[float]] = ((0.0, 0.0), (0.0, 0.0), (0.0, 0.0)),
                 cmd_interval: int = 0, cmd_zero_prob: float = 0.0, cmd_min: float = 0.0,
                 action_scale: float = 0.0, w_track_lin: float = 1.0, w_track_yaw: float = 0.5,
                 track_sigma: float = 0.25, w_lin_z: float = 0.0, w_ang_xy: float = 0.0,
                 w_action_rate: float = 0.0, w_air_time: float = 0.0, air_time_target: float = 0.0,
                 contact_force_min: float = 1.0,
                 obs_noise=None, action_delay_range: Optional[Sequence[int]] = None,
                 reward_terms: Optional[Mapping] = None, termination_links: Optional[Sequence] = None,
                 termination_force: float = 1.0, penalised_links: Sequence = (), collision_force_min: float = 0.1,
                 base_height_target: Optional[float] = None, soft_limit: float = 0.9, stumble_ratio: float = 5.0,
                 max_contact_force: float = 100.0,
                 init_states=None, init_state_prob: float = 1.0,
                 init_pos_range: Optional[Sequence[Sequence[float]]] = None,
                 init_rpy_range: Optional[Sequence[Sequence[float]]] = None,
                 init_lin_vel_range: Optional[Sequence[Sequence[float]]] = None,
                 init_ang_vel_range: Optional[Sequence[Sequence[float]]] = None,
                 init_joint_vel: Optional[float] = None,
                 motion_clips=None, clip_loop=False, clip_fps: Optional[float] = None,
                 track_weights: Optional[Mapping] = None, track_scales: Optional[Mapping] = None,
                 track_joint_weights: Optional[Sequence[float]] = None,
                 track_termination: Optional[Mapping] = None, rsi_prob: float = 1.0, obs_reference: bool = True):
        """``model``: a shipped model's name or a URDF / SDF file.  ``home_q``
        (one value per dof) and ``home_base`` (x y z qw qx qy qz) are the reset
        state; ``pid_gains`` per dof ``(p, i, d)`` or the eight values of
        ``Simulator.set_pid`` (position mode); either may be a function of the
        joint names in dof order.  ``contact_links``: link names
        or dof indices (-1 = the base) whose ground reaction enters the
        observation.  ``max_tilt`` (rad): the episode ends when the base's z
        axis leans further from the world's.

        Domain randomisation, sampled on the device (``mw_floatenv_randomize``):
        ``push_interval`` > 0 pushes every world's base for ``push_steps``
        steps out of every ``push_interval``, each episode at its own phase,
        with a world force (fx, fy) ~ U(-``push_force``, ``push_force``) N and a
        torque tz ~ U(-``push_torque``, ``push_torque``) N m; ``friction_range``
        ``(lo, hi)`` draws every world's ground friction anew at each reset.
        ``env.push`` ``[n_worlds, 6]`` holds the wrench the last step applied and
        ``env.friction`` ``[n_worlds]`` the current coefficients; both are also
        in ``info`` (``"push"``, ``"friction"``) when the feature is on.

        Inertia randomisation (``mw_floatenv_inertia``), drawn anew at each
        reset: ``mass_scale_range`` ``(lo, hi)`` scales the mass and the
        rotational inertia of every link, the base included, by its own factor
        U(lo, hi); ``payload_range`` ``(lo, hi)`` kg adds a point mass to the
        base at a position uniform in ±``payload_box`` (m, base frame).
        ``env.inertial`` ``[n_worlds, n + 1, 10]`` (also ``info["inertial"]``)
        holds the words in force for the current episode, base first, in the
        layout of ``Simulator.set_link_params``, and ``env.inertia_draws``
        ``[n_worlds, n + 5]`` (``info["inertia_draws"]``) the draws themselves:
        the ``n + 1`` scales, the payload mass and its position; both ``None``
        with the feature off.

        Joint randomisation (``mw_floatenv_joints``), drawn anew at each reset
        for every joint of ``joint_rand_dofs`` (names or dof indices; ``None``
        = every joint): ``joint_damping_range`` ``(lo, hi)`` N m s/rad and
        ``joint_friction_range`` ``(lo, hi)`` N m are added to the model's
        values, ``effort_scale_range`` ``(lo, hi)`` scales the effort limit (an
        unbounded one stays unbounded).  Joint friction costs one constraint
        row per moving joint out of a world's 64 (``sim.constraint_overflow``
        counts dropped rows): randomise, say, the legs only.  ``env.joint_dynamics``
        ``[n_worlds, n, 3]`` (``info["joint_dynamics"]``) holds damping,
        friction and effort limit in force for the current episode, in the
        layout of ``Simulator.set_joint_dynamics``, and ``env.joint_draws``
        ``[n_worlds, n, 3]`` (``info["joint_draws"]``) the draws themselves
        (0, 0, 1 where nothing is drawn); both ``None`` with the feature off.

        ``task="locomotion"``: ``command_ranges`` holds the ``(lo, hi)`` of
        v_x, v_y (m/s) and the yaw rate (rad/s); a command is drawn every
        ``cmd_interval`` steps (0: once per episode) and is zero with
        probability ``cmd_zero_prob``.  ``action_scale`` > 0 sends ``home_q +
        action_scale * a`` (position mode) or ``action_scale * a`` (torque
        mode) to the simulator.  Reward terms on top of the forward task's
        (set ``w_forward=0`` to drop that one): ``w_track_lin``, ``w_track_yaw``
        (``exp(-error^2 / track_sigma)``), ``w_lin_z``, ``w_ang_xy``,
        ``w_action_rate``, and ``w_air_time`` per touchdown of a contact link
        (force above ``contact_force_min`` N) after ``air_time_target`` s of
        flight, for commands faster than ``cmd_min``.  ``env.command``
        ``[n_worlds, 3]`` (also ``info["command"]``) is the command in force
        for the next step, the same words as ``obs[:, env.obs_slices["command"]]``.
        With ``task="forward"`` ``env.command`` is ``None``; command ranges,
        ``cmd_interval``, ``action_scale`` and ``w_air_time`` are refused there
        and the other locomotion weights have no effect.

        Sensor noise and actuation latency (``mw_floatenv_noise``), both drawn
        on the device inside the same three launches.  ``obs_noise`` maps group
        names to amplitudes -- ``base_position``, ``base_orientation``,
        ``base_linear_velocity``, ``base_angular_velocity``,
        ``joint_positions``, ``joint_velocities``, ``contacts`` and, in the
        locomotion task, ``gravity``, ``body_linear_velocity``,
        ``body_angular_velocity`` (``env.noise_slices`` has their words) -- or
        is a full vector of ``obs_dim`` amplitudes: word ``k`` of ``obs`` and
        ``terminal_obs`` becomes ``clean + amplitude[k] * u``, ``u`` uniform in
        [-1, 1), a pure function of (seed, global world, episode, step, k).
        The command and last-action words take no noise; reward, termination
        and the task's bookkeeping use the clean rows.  ``env.obs_noise``
        ``[obs_dim]`` holds the amplitudes, ``env.clean_obs`` (also
        ``info["clean_obs"]``) the rows before the noise -- what an asymmetric
        critic is given -- and ``info["clean_terminal_obs"]`` those of
        ``terminal_obs``.  ``action_delay_range`` ``(lo, hi)``, at most 8
        control steps: every episode draws a delay ``d`` in it and the
        simulator receives the action of ``d`` steps ago (scaled as usual),
        during an episode's first ``d`` steps the neutral command -- ``home_q``
        in position mode, zero torque otherwise; the reward's action terms and
        the last-action words stay on the action just given.
        ``env.action_delay`` ``[n_worlds]`` int32 (also
        ``info["action_delay"]``) holds the current delays.  Each attribute is
        ``None`` with its feature off.

        Shaping rewards, contact termination and episode statistics
        (``mw_floatenv_shaping``), on when ``reward_terms``,
        ``termination_links`` or ``penalised_links`` is given.  ``reward_terms``
        maps term names to weights >= 0; a step's reward gains ``-weight * x``
        per term, in this order: ``torque`` (sum tau^2), ``power`` (sum |tau
        qd|), ``joint_acc`` (sum of squared finite-difference joint
        accelerations), ``orientation`` (g_x^2 + g_y^2 of the projected
        gravity), ``base_height`` ((z - ``base_height_target``)^2; default: the
        home height), ``joint_limits`` (distance beyond ``soft_limit`` times
        the half-range around the centre of the position limits),
        ``collision`` (number of ``penalised_links`` pressed with more than
        ``collision_force_min`` N), ``stumble`` (contact links whose horizontal
        force exceeds ``stumble_ratio`` times the vertical one),
        ``contact_force`` (force of the contact links above
        ``max_contact_force`` N) and ``stand_still`` (sum |q - home_q| under a
        command slower than ``cmd_min``; needs ``task="locomotion"``).  tau is
        the torque the simulator applied, clamped with the world's own effort
        limit.  ``termination_links``: the episode ends -- terminated, without
        the alive bonus -- when a contact point of one of these links carries
        more than ``termination_force`` N.  Contacts are those of the last
        physics step of a control step: with ``steps_per_run`` > 1 a touch that
        ends earlier within the step is not seen.  Link names resolve as
        ``contact_links`` do; a link without a collision shape is refused,
        since it could never fire.  ``env.reward_term_names`` holds the ten
        names, ``env.reward_terms`` ``[n_worlds, 10]`` the step's signed terms,
        ``env.torques`` ``[n_worlds, n]`` the torque they used, and
        ``env.episode_return`` ``[n_worlds]``, ``env.episode_length``
        ``[n_worlds]`` int32 and ``env.episode_terms`` ``[n_worlds, 10]`` the
        return, length and term sums of the last finished episode of each
        world, valid where that world has been ``done`` (``reset()`` starts the
        running sums over and leaves these three alone).  All are mirrored in ``info``
        under the same names and are ``None`` with the feature off.

        Initial-state randomisation and the reset-state bank
        (``mw_floatenv_init_state``), on when ``init_states`` or any of the
        ``init_*`` ranges is given; every reset then draws where the episode
        starts, inside the same launches, as a pure function of (seed, global
        world, episode).  An episode starts from a base row of ``13 + 2 n``
        words in the layout of ``obs[:, :13 + 2 n]`` -- base position,
        quaternion wxyz, world linear and angular velocity, ``q``, ``qd`` --
        so a recorded observation row is a valid row.  Without a bank it is the
        home row (``home_base``, ``home_q``, at rest).  ``init_states``: a
        contiguous float32 tensor ``[K, 13 + 2 n]`` on the env's device; an
        episode starts from one of its rows with probability
        ``init_state_prob`` (default 1), else from the home row.  The env keeps
        the tensor and reads it at every reset: rows overwritten between two
        steps (on the env's stream) are what the next resets see.  What a row
        holds is the caller's business: a zero quaternion or a non-finite word
        gives a non-finite state, which ends at the next step like any diverged
        world and is reset.  On top of the row, each off unless given:
        ``init_pos_range``, three ``(lo, hi)`` pairs (m) added to the base
        position in the world frame; ``init_rpy_range``, three ``(lo, hi)``
        pairs (rad) for roll, pitch and yaw, world-frame rotations applied
        after the row's own orientation (``qz(yaw) qy(pitch) qx(roll) q_row``,
        normalised; without it the row's quaternion is taken as it is);
        ``init_lin_vel_range`` and ``init_ang_vel_range``, three ``(lo, hi)``
        pairs each, added to the row's world linear (m/s) and angular (rad/s)
        velocity; ``init_joint_vel`` ``v >= 0``: every joint velocity gains
        U(-v, v).  Joint positions are the row's plus ``joint_noise`` as
        before, clipped into the position limits.  The reset observation is
        that of the drawn state (in the locomotion task its gravity and
        body-velocity words too), and the ``joint_acc`` term of an episode's
        first step is taken from the drawn joint velocities.  Nothing checks a
        drawn state against ``z_min``, ``max_tilt`` or the ground: a start
        beyond the first two simply ends at the next step, and a start below
        the ground is yours to avoid through the ranges.  ``env.init_state``
        ``[n_worlds, 13 + 2 n]`` (also ``info["init_state"]``) holds the state
        the current episode started from -- the first words of the clean reset
        row -- and ``env.init_draws`` ``[n_worlds, 13 + n]``
        (``info["init_draws"]``) the draws themselves: position offsets (3),
        roll pitch yaw (3), linear (3) and angular (3) velocity offsets, the
        bank row as a float (-1 for the home row) and the ``n`` joint-velocity
        draws; both change where, and only where, an episode ended, and are
        ``None`` with the feature off.

        Motion-clip tracking (``mw_floatenv_tracking``), on when
        ``motion_clips`` is given: a contiguous float32 tensor ``[F, 13 + 2
        n]`` on the env's device, or a list of such tensors (at most 16), one
        clip each, concatenated once into ``env.motion_clips``; rows in the
        layout of ``obs[:, :13 + 2 n]``, so recorded observation rows make a
        clip, at least 2 per clip.  The env reads the rows at every step.
        ``clip_loop`` (one flag, or one per clip): a looping clip's last row
        is its first pose again; it is followed round and round, the reference
        base x and y gaining the clip's displacement at every wrap.  Its
        heading is assumed periodic: a clip that turns over a period is not
        followed across the wrap (heading drift is out of scope).  A clip that
        does not loop ends the episode as truncated -- ``done`` without a
        termination, the alive bonus kept, like the time limit -- at the first
        step whose reference would lie beyond its last row.  ``clip_fps``: the
        clips' frames per second (default: one frame per control step); the
        frames per control step, ``clip_fps * step_size * steps_per_run``, must
        be a ratio of whole numbers with a denominator of at most 1000 to
        within 1e-9 (``ValueError`` otherwise): the frame clock is integer
        arithmetic and never drifts; between two rows the reference is their
        blend, the orientation by normalised linear interpolation.  Every
        reset draws a clip and, with probability ``rsi_prob``, a start frame
        of it (else frame 0), and starts the episode from that row; the
        ``init_*`` offsets and ``joint_noise`` apply on top of it, and
        ``init_states`` (a bank) is refused.  The reward gains ``weight *
        exp(-scale * error)`` for five errors of the state against the
        reference -- ``pose`` (sum of weighted squared joint position
        errors, ``track_joint_weights`` per dof, default 1), ``velocity`` (the
        same on joint velocities), ``root_pos`` (squared base position error),
        ``root_rot`` (1 - (q . q_ref)^2), ``root_vel`` (squared base linear
        velocity error plus ``ang_scale`` times the angular one) -- with
        ``track_weights`` and ``track_scales`` mapping those names to values
        (``track_scales`` also takes ``ang_scale``); names left out keep the
        defaults of ``TRACKING_WEIGHTS`` / ``TRACKING_SCALES``.
        ``track_termination`` maps ``pose``, ``root_pos``, ``root_rot`` to a
        bound: the episode ends terminated, without the alive bonus, when the
        error exceeds it.  The observation grows by a block behind everything
        else: ``obs_slices["phase"]`` (sin and cos of 2 pi times the fraction
        of the clip gone by), ``obs_slices["clip"]`` (the clip's index as a
        float) and, with ``obs_reference``, ``obs_slices["reference"]``: the
        ``n`` reference joint positions one step ahead, the target of the next
        action.  These words take no noise.  ``env.tracking_terms`` and
        ``env.tracking_errors`` ``[n_worlds, 5]`` hold the step's signed terms
        and errors (``env.tracking_term_names``), ``env.track_clip`` and
        ``env.track_frame`` ``[n_worlds]`` int32 the clip and the start frame
        of every world's current episode; all are mirrored in ``info`` and are
        ``None`` with the feature off.  With shaping on, ``env.episode_return``
        includes the tracking terms.  Out of scope: end-effector or key-body
        position terms (the post launch has no link poses), a residual action
        around the reference, weighted clip sampling."""
        torch = _torch()
        if action_mode not in ACTION_MODES:
            raise ValueError(f"unknown action_mode {action_mode!r}; known: {sorted(ACTION_MODES)}")
        if task not in TASKS:
            raise ValueError(f"unknown task {task!r}; known: {list(TASKS)}")
        if len(command_ranges) != 3 or any(len(r) != 2 for r in command_ranges):
            raise ValueError("command_ranges must hold three (lo, hi) pairs: v_x, v_y, yaw rate")
        if task == "forward" and (action_scale != 0.0 or cmd_interval != 0 or w_air_time != 0.0 or
                                  any(float(v) != 0.0 for r in command_ranges for v in r)):
            raise ValueError('commands, action_scale and the air-time term need task="locomotion"')
        try:
            model_file = get_model_file(model)
        except ValueError:
            model_file = model
        self.action_mode = action_mode
        self.task = task
        self.n_worlds = n_worlds
        self.device = torch.device("cuda", device)
        self._h = None
        with torch.cuda.device(self.device):
            self._stream = torch.cuda.current_stream(self.device)
            self.sim = Simulator(model_file, n_worlds=n_worlds, step_size=step_size,
                                 steps_per_run=steps_per_run, device=device, pgs_iters=pgs_iters,
                                 pose=tuple(home_base), stream=self._stream.cuda_stream)
        sim = self.sim
        n = sim.dofs
        if home_q is None:
            home_q = np.zeros(n)
        if callable(home_q):      # of the joint names, in dof order
            home_q = home_q(sim.joint_names)
        if callable(pid_gains):
            pid_gains = pid_gains(sim.joint_names)
        self.home_q = np.ascontiguousarray(home_q, dtype=np.float32)
        if self.home_q.shape != (n,):
            raise ValueError(f"home_q must hold one value per dof ({n}), got shape {self.home_q.shape}")
        self.home_base = np.ascontiguousarray(home_base, dtype=np.float32)
        if self.home_base.shape != (7,):
            raise ValueError("home_base must be (x, y, z, qw, qx, qy, qz)")
        self.contact_links = self._resolve_links(model_file, contact_links)
        sim.set_ground_plane(True, ground_mu)
        sim.enable_contacts(True)
        if pid_gains is not None:
            if len(pid_gains) != n:
                raise ValueError(f"pid_gains must hold one entry per dof ({n})")
            big = float(np.finfo(np.float64).max)
            for d, g in enumerate(pid_gains):
                g = list(g)
                sim.set_pid(d, g if len(g) == 8 else [g[0], g[1], g[2], -big, big, 0.0, -big, big])
        links = np.ascontiguousarray(self.contact_links, dtype=np.int32)
        cfg = N.MwFloatTaskConfig(
            ACTION_MODES[action_mode], max_episode_steps, world_offset, len(links), seed & 0xFFFFFFFFFFFFFFFF,
            z_min, math.cos(max_tilt), alive_bonus, w_forward, w_action, w_pose, joint_noise, 0.0,
            (ctypes.c_float * 7)(*self.home_base.tolist()), _fptr(self.home_q), _iptr(links))
        h = ctypes.c_void_p()
        N.check(N.lib().mw_floatenv_create(sim.handle, ctypes.byref(cfg), ctypes.byref(h)), "mw_floatenv_create")
        self._h = h
        # the C layer takes the locomotion task first: it sets the width of the rows
        self._setup_locomotion(command_ranges, cmd_interval, cmd_zero_prob, cmd_min, action_scale, w_track_lin,
                               w_track_yaw, track_sigma, w_lin_z, w_ang_xy, w_action_rate, w_air_time,
                               air_time_target, contact_force_min)
        # ... then the tracking task, which appends its block behind the locomotion block
        self._setup_tracking(motion_clips, clip_loop, clip_fps, track_weights, track_scales, track_joint_weights,
                             track_termination, rsi_prob, obs_reference)
        no = ctypes.c_int32()
        N.check(N.lib().mw_vecenv_obs_dim(h, ctypes.byref(no)))
        self.obs_dim = no.value
        self.action_dim = n
        nl = len(links)
        self.obs_slices = {"base": slice(0, 13), "joints": slice(13, 13 + 2 * n),
                           "contacts": slice(13 + 2 * n, 13 + 2 * n + nl)}
        if task == "locomotion":
            nb = 13 + 2 * n + nl
            self.obs_slices.update(gravity=slice(nb, nb + 3), body_velocity=slice(nb + 3, nb + 9),
                                   command=slice(nb + 9, nb + 12), last_action=slice(nb + 12, nb + 12 + n))
        if self.motion_clips is not None:
            nt = 13 + 2 * n + nl + (12 + n if task == "locomotion" else 0)
            self.obs_slices.update(phase=slice(nt, nt + 2), clip=slice(nt + 2, nt + 3))
            if obs_reference:
                self.obs_slices["reference"] = slice(nt + 3, nt + 3 + n)
        # the groups obs_noise names: the sensors behind the words
        self.noise_slices = {"base_position": slice(0, 3), "base_orientation": slice(3, 7),
                             "base_linear_velocity": slice(7, 10), "base_angular_velocity": slice(10, 13),
                             "joint_positions": slice(13, 13 + n), "joint_velocities": slice(13 + n, 13 + 2 * n),
                             "contacts": self.obs_slices["contacts"]}
        if task == "locomotion":
            self.noise_slices.update(gravity=slice(nb, nb + 3), body_linear_velocity=slice(nb + 3, nb + 6),
                                     body_angular_velocity=slice(nb + 6, nb + 9))
        self.obs = self._zeros(n_worlds, self.obs_dim)
        self.reward = self._zeros(n_worlds)
        self.done = self._zeros(n_worlds, dtype=torch.uint8)
        self.terminal_obs = self._zeros(n_worlds, self.obs_dim)
        # what step(), step_raw() and rollout() pass after the actions
        self._out = tuple(_ptr(t) for t in (self.obs, self.reward, self.done, self.terminal_obs))
        self._info = {"terminal_obs": self.terminal_obs}
        if self.command is not None:
            self._info["command"] = self.command
        if self.motion_clips is not None:
            self._info.update(tracking_terms=self.tracking_terms, tracking_errors=self.tracking_errors,
                              track_clip=self.track_clip, track_frame=self.track_frame)
        self._setup_randomize(push_interval, push_steps, push_force, push_torque, friction_range, ground_mu)
        self._setup_inertia(mass_scale_range, payload_range, payload_box)
        self._setup_joints(joint_damping_range, joint_friction_range, effort_scale_range, joint_rand_dofs)
        self._setup_noise(obs_noise, action_delay_range)
        self._setup_shaping(model_file, reward_terms, termination_links, termination_force, penalised_links,
                            collision_force_min, base_height_target, soft_limit, stumble_ratio, max_contact_force)
        self._setup_init_state(init_states, init_state_prob, init_pos_range, init_rpy_range, init_lin_vel_range,
                               init_ang_vel_range, init_joint_vel)

    def _zeros(self, *shape, dtype=None):
        torch = _torch()
        return torch.zeros(shape, dtype=dtype or torch.float32, device=self.device)

    # One method per feature: its argument checks, its tensors, its config
    # struct and its one C call.  A feature that is off leaves its attributes None.

    def _setup_locomotion(self, command_ranges, cmd_interval, cmd_zero_prob, cmd_min, action_scale, w_track_lin,
                          w_track_yaw, track_sigma, w_lin_z, w_ang_xy, w_action_rate, w_air_time, air_time_target,
                          contact_force_min):
        self.command = None
        if self.task != "locomotion":
            return
        self.command = self._zeros(self.n_worlds, 3)
        lc = N.MwFloatLocoConfig(
            (ctypes.c_float * 3)(*[float(r[0]) for r in command_ranges]),
            (ctypes.c_float * 3)(*[float(r[1]) for r in command_ranges]),
            cmd_interval, cmd_zero_prob, cmd_min, action_scale, w_track_lin, w_track_yaw, track_sigma,
            w_lin_z, w_ang_xy, w_action_rate, w_air_time, air_time_target, contact_force_min)
        N.check(N.lib().mw_floatenv_locomotion(self._h, ctypes.byref(lc), _ptr(self.command)),
                "mw_floatenv_locomotion")

    def _setup_tracking(self, motion_clips, clip_loop, clip_fps, track_weights, track_scales, track_joint_weights,
                        track_termination, rsi_prob, obs_reference):
        self.motion_clips = self.clip_table = self.clip_fraction = self.tracking_term_names = None
        self.tracking_terms = self.tracking_errors = self.track_clip = self.track_frame = None
        if motion_clips is None:
            return
        torch = _torch()
        n, words = self.sim.dofs, 13 + 2 * self.sim.dofs
        clips = [motion_clips] if isinstance(motion_clips, torch.Tensor) else list(motion_clips)
        if not 1 <= len(clips) <= N.FLOAT_MAX_CLIPS:
            raise ValueError(f"motion_clips must hold 1 to {N.FLOAT_MAX_CLIPS} clips, got {len(clips)}")
        for c in clips:
            if not isinstance(c, torch.Tensor) or c.device != self.device:
                raise TypeError(f"motion_clips must be torch tensors on {self.device}")
            if c.dtype != torch.float32 or c.dim() != 2 or c.shape[1] != words or not c.is_contiguous():
                raise TypeError(f"every clip must be a contiguous {torch.float32} tensor of shape [F, {words}]")
        loops = [bool(clip_loop)] * len(clips) if isinstance(clip_loop, (bool, int)) else [bool(v) for v in clip_loop]
        if len(loops) != len(clips):
            raise ValueError("clip_loop must be one flag or one per clip")
        # frames per control step as an exact ratio: the device's frame clock is integer arithmetic
        num, den = 1, 1
        if clip_fps is not None:
            per_step = float(clip_fps) * self.sim.step_size * self.sim.steps_per_run
            ratio = fractions.Fraction(per_step).limit_denominator(1000)
            if ratio <= 0 or abs(float(ratio) - per_step) > 1e-9:
                raise ValueError(f"clip_fps {clip_fps} gives {per_step!r} frames per control step, which is no ratio of "
                                 f"whole numbers with a denominator <= 1000 to within 1e-9")
            num, den = ratio.numerator, ratio.denominator
        self.clip_fraction = (num, den)

        def named(given, defaults, what):
            out = dict(defaults)
            for name, value in (given or {}).items():
                if name not in defaults:
                    raise ValueError(f"{what}: unknown name {name!r}; known: {list(defaults)}")
                out[name] = float(value)
            return out
        weights = named(track_weights, TRACKING_WEIGHTS, "track_weights")
        scales = named(track_scales, TRACKING_SCALES, "track_scales")
        bounds = named(track_termination, dict(pose=0.0, root_pos=0.0, root_rot=0.0), "track_termination")
        wj = None
        if track_joint_weights is not None:
            wj = np.ascontiguousarray(track_joint_weights, dtype=np.float32)
            if wj.shape != (n,):
                raise ValueError(f"track_joint_weights must hold one value per dof ({n}), got shape {wj.shape}")
        # one buffer, concatenated once; the env keeps it: the launches read it at every step
        self.motion_clips = clips[0] if len(clips) == 1 else torch.cat(clips).contiguous()
        lengths = [int(c.shape[0]) for c in clips]
        firsts = [sum(lengths[:k]) for k in range(len(clips))]
        self.clip_table = tuple(zip(firsts, lengths, loops))
        self.tracking_term_names = TRACKING_TERMS
        self.tracking_terms = self._zeros(self.n_worlds, N.FLOAT_TRACK_TERMS)
        self.tracking_errors = self._zeros(self.n_worlds, N.FLOAT_TRACK_TERMS)
        self.track_clip = self._zeros(self.n_worlds, dtype=torch.int32)
        self.track_frame = self._zeros(self.n_worlds, dtype=torch.int32)
        pad = [0] * (N.FLOAT_MAX_CLIPS - len(clips))
        i16 = ctypes.c_int32 * N.FLOAT_MAX_CLIPS
        f5 = ctypes.c_float * N.FLOAT_TRACK_TERMS
        tc = N.MwFloatTrackConfig(
            sum(lengths), len(clips), i16(*firsts, *pad), i16(*lengths, *pad), i16(*[int(v) for v in loops], *pad),
            num, den, f5(*[weights[k] for k in TRACKING_TERMS]), f5(*[scales[k] for k in TRACKING_TERMS]),
            scales["ang_scale"], bounds["pose"], bounds["root_pos"], bounds["root_rot"], rsi_prob,
            1 if obs_reference else 0, None if wj is None else _fptr(wj))
        N.check(N.lib().mw_floatenv_tracking(
            self._h, ctypes.byref(tc), _ptr(self.motion_clips), _ptr(self.tracking_terms), _ptr(self.tracking_errors),
            _ptr(self.track_clip), _ptr(self.track_frame)), "mw_floatenv_tracking")

    def _setup_randomize(self, push_interval, push_steps, push_force, push_torque, friction_range, ground_mu):
        self.push = self.friction = None
        if not push_interval and friction_range is None:
            return
        lo, hi = (0.0, 0.0) if friction_range is None else friction_range
        if push_interval:
            self.push = self._info["push"] = self._zeros(self.n_worlds, 6)
        if hi > 0:
            self.friction = self._info["friction"] = self._zeros(self.n_worlds).fill_(float(ground_mu))
        rc = N.MwFloatRandConfig(push_interval, push_steps, push_force, push_torque, lo, hi)
        N.check(N.lib().mw_floatenv_randomize(self._h, ctypes.byref(rc), _ptr(self.push), _ptr(self.friction)),
                "mw_floatenv_randomize")

    def _setup_inertia(self, mass_scale_range, payload_range, payload_box):
        self.inertial = self.inertia_draws = None
        if mass_scale_range is None and payload_range is None:
            return
        sim, n, n_worlds = self.sim, self.action_dim, self.n_worlds
        slo, shi = (0.0, 0.0) if mass_scale_range is None else mass_scale_range
        plo, phi = (0.0, 0.0) if payload_range is None else payload_range
        if len(payload_box) != 3:
            raise ValueError("payload_box must hold three half extents (m)")
        if shi > 0 or phi > 0:
            nominal = np.stack([sim.link_params(k - 1, [0])[0] for k in range(n + 1)])
            self.inertial = self._info["inertial"] = _torch().from_numpy(
                np.ascontiguousarray(np.broadcast_to(nominal, (n_worlds, n + 1, 10)))).to(self.device)
            self.inertia_draws = self._info["inertia_draws"] = self._zeros(n_worlds, n + 5)
            self.inertia_draws[:, :n + 1] = 1.0
        ic = N.MwFloatInertiaConfig(slo, shi, plo, phi, (ctypes.c_float * 3)(*[float(b) for b in payload_box]))
        N.check(N.lib().mw_floatenv_inertia(self._h, ctypes.byref(ic), _ptr(self.inertial), _ptr(self.inertia_draws)),
                "mw_floatenv_inertia")

    def _setup_joints(self, joint_damping_range, joint_friction_range, effort_scale_range, joint_rand_dofs):
        self.joint_dynamics = self.joint_draws = None
        if joint_damping_range is None and joint_friction_range is None and effort_scale_range is None:
            return
        sim, n, n_worlds = self.sim, self.action_dim, self.n_worlds
        dlo, dhi = (0.0, 0.0) if joint_damping_range is None else joint_damping_range
        flo, fhi = (0.0, 0.0) if joint_friction_range is None else joint_friction_range
        elo, ehi = (0.0, 0.0) if effort_scale_range is None else effort_scale_range
        mask = 0
        for d in (() if joint_rand_dofs is None else joint_rand_dofs):
            di = sim.joint_names.index(d) if isinstance(d, str) else int(d)
            if not 0 <= di < n:
                raise ValueError(f"joint_rand_dofs: dof {d!r} out of range [0, {n})")
            mask |= 1 << di
        if joint_rand_dofs is not None and mask == 0:
            raise ValueError("joint_rand_dofs is empty (None = every joint)")
        if dhi > 0 or fhi > 0 or ehi > 0:
            nominal = np.stack([sim.joint_dynamics(d, [0])[0] for d in range(n)])
            self.joint_dynamics = self._info["joint_dynamics"] = _torch().from_numpy(
                np.tile(nominal, (n_worlds, 1, 1))).to(self.device)
            self.joint_draws = self._info["joint_draws"] = self._zeros(n_worlds, n, 3)
            self.joint_draws[:, :, 2] = 1.0
        jc = N.MwFloatJointConfig(dlo, dhi, flo, fhi, elo, ehi, mask)
        N.check(N.lib().mw_floatenv_joints(self._h, ctypes.byref(jc), _ptr(self.joint_dynamics),
                                           _ptr(self.joint_draws)), "mw_floatenv_joints")

    def _setup_noise(self, obs_noise, action_delay_range):
        self.obs_noise = self.clean_obs = self.clean_terminal_obs = self.action_delay = None
        if obs_noise is None and action_delay_range is None:
            return
        torch = _torch()
        amp = None
        if obs_noise is not None:
            amp = self._noise_vector(obs_noise)
            self.obs_noise = torch.from_numpy(amp).to(self.device)
            self.clean_obs = self._info["clean_obs"] = self._zeros(self.n_worlds, self.obs_dim)
            self.clean_terminal_obs = self._info["clean_terminal_obs"] = self._zeros(self.n_worlds, self.obs_dim)
        lo, hi = (0, 0) if action_delay_range is None else action_delay_range
        if int(lo) != lo or int(hi) != hi:
            raise ValueError("action_delay_range must hold two whole numbers of control steps")
        if action_delay_range is not None:
            self.action_delay = self._info["action_delay"] = self._zeros(self.n_worlds, dtype=torch.int32)
        nc = N.MwFloatNoiseConfig(int(lo), int(hi))
        N.check(N.lib().mw_floatenv_noise(
            self._h, ctypes.byref(nc), None if amp is None else _fptr(amp), _ptr(self.clean_obs),
            _ptr(self.clean_terminal_obs), _ptr(self.action_delay)), "mw_floatenv_noise")

    def _setup_shaping(self, model_file, reward_terms, termination_links, termination_force, penalised_links,
                       collision_force_min, base_height_target, soft_limit, stumble_ratio, max_contact_force):
        self.reward_term_names = self.reward_terms = self.torques = None
        self.episode_return = self.episode_length = self.episode_terms = None
        self.termination_links = self.penalised_links = None
        if not (reward_terms or termination_links or penalised_links):
            return
        n_worlds = self.n_worlds
        weights = np.zeros(N.FLOAT_SHAPE_TERMS, np.float32)
        for name, value in (reward_terms or {}).items():
            if name not in REWARD_TERMS:
                raise ValueError(f"reward_terms: unknown term {name!r}; known: {list(REWARD_TERMS)}")
            weights[REWARD_TERMS.index(name)] = value
        self.termination_links = self._resolve_links(model_file, termination_links or (), limit=None)
        self.penalised_links = self._resolve_links(model_file, penalised_links or ())
        term = np.ascontiguousarray(self.termination_links, dtype=np.int32)
        pen = np.ascontiguousarray(self.penalised_links, dtype=np.int32)
        self.reward_term_names = REWARD_TERMS
        self.reward_terms = self._zeros(n_worlds, N.FLOAT_SHAPE_TERMS)
        self.torques = self._zeros(n_worlds, self.action_dim)
        self.episode_return = self._zeros(n_worlds)
        self.episode_length = self._zeros(n_worlds, dtype=_torch().int32)
        self.episode_terms = self._zeros(n_worlds, N.FLOAT_SHAPE_TERMS)
        sc = N.MwFloatShapeConfig(
            (ctypes.c_float * N.FLOAT_SHAPE_TERMS)(*weights.tolist()),
            float(self.home_base[2]) if base_height_target is None else base_height_target, soft_limit,
            collision_force_min, stumble_ratio, max_contact_force, termination_force, len(pen), len(term),
            _iptr(pen), _iptr(term))
        N.check(N.lib().mw_floatenv_shaping(
            self._h, ctypes.byref(sc), _ptr(self.reward_terms), _ptr(self.torques), _ptr(self.episode_return),
            _ptr(self.episode_length), _ptr(self.episode_terms)), "mw_floatenv_shaping")
        self._info.update(reward_terms=self.reward_terms, torques=self.torques,
                          episode_return=self.episode_return, episode_length=self.episode_length,
                          episode_terms=self.episode_terms)

    def _setup_init_state(self, init_states, init_state_prob, init_pos_range, init_rpy_range, init_lin_vel_range,
                          init_ang_vel_range, init_joint_vel):
        self.init_states = self.init_state = self.init_draws = None
        ranges = (init_pos_range, init_rpy_range, init_lin_vel_range, init_ang_vel_range)
        if (init_states is None and init_joint_vel is None and all(r is None for r in ranges) and
                self.motion_clips is None):        # tracking resets through this path: its start states are reported
            return
        torch = _torch()
        n, words = self.action_dim, 13 + 2 * self.action_dim
        bounds = []
        for name, r in zip(("init_pos_range", "init_rpy_range", "init_lin_vel_range", "init_ang_vel_range"), ranges):
            r = ((0.0, 0.0),) * 3 if r is None else r
            if len(r) != 3 or any(len(pair) != 2 for pair in r):
                raise ValueError(f"{name} must hold three (lo, hi) pairs")
            bounds += [(ctypes.c_float * 3)(*[float(pair[0]) for pair in r]),
                       (ctypes.c_float * 3)(*[float(pair[1]) for pair in r])]
        if init_states is not None:
            if not isinstance(init_states, torch.Tensor) or init_states.device != self.device:
                raise TypeError(f"init_states must be a torch tensor on {self.device}")
            if (init_states.dtype != torch.float32 or init_states.dim() != 2 or init_states.shape[0] < 1 or
                    init_states.shape[1] != words or not init_states.is_contiguous()):
                raise TypeError(f"init_states must be a contiguous {torch.float32} tensor of shape [K >= 1, {words}]")
            self.init_states = init_states      # kept: the launches read it at every reset
        self.init_state = self._info["init_state"] = self._zeros(self.n_worlds, words)
        self.init_draws = self._info["init_draws"] = self._zeros(self.n_worlds, 13 + n)
        ic = N.MwFloatInitConfig(*bounds, 0.0 if init_joint_vel is None else init_joint_vel, init_state_prob,
                                 0 if init_states is None else init_states.shape[0])
        N.check(N.lib().mw_floatenv_init_state(self._h, ctypes.byref(ic), _ptr(self.init_states),
                                               _ptr(self.init_state), _ptr(self.init_draws)),
                "mw_floatenv_init_state")

    def _noise_vector(self, obs_noise) -> np.ndarray:
        """obs_noise (group name -> amplitude, or obs_dim values) as the float32 vector the library takes."""
        if isinstance(obs_noise, Mapping):
            amp = np.zeros(self.obs_dim, np.float32)
            for name, value in obs_noise.items():
                if name in ("command", "last_action", "phase", "clip", "reference"):
                    raise ValueError(f"obs_noise: the {name} words take no noise")
                if name not in self.noise_slices:
                    raise ValueError(f"obs_noise: unknown group {name!r}; known: {sorted(self.noise_slices)}")
                amp[self.noise_slices[name]] = value
            return amp
        amp = np.ascontiguousarray(obs_noise, dtype=np.float32)
        if amp.shape != (self.obs_dim,):
            raise ValueError(f"obs_noise must map group names to amplitudes or hold obs_dim ({self.obs_dim}) values, "
                             f"got shape {amp.shape}")
        return amp

    # ------------------------------------------------------------------
    # what quadruped() / icub() add for task="locomotion" unless the caller sets it
    LOCOMOTION_DEFAULTS = dict(action_scale=0.25, track_sigma=0.25, air_time_target=0.3)

    @classmethod
    def icub(cls, n_worlds: int, **kw) -> "FloatVecEnv":
        """The iCub-class humanoid (BASELINE config 5) from the reference
        wrapper's pose and posture, under its posture-hold gains; the soles'
        ground reaction in the observation."""
        from .models import ICUB_POSE, icub_pid_gains, icub_posture

        def gains(names):
            return [[p, 0.0, d, -80.0, 80.0, 0.0, 0.0, -1.0] for p, d in icub_pid_gains(names)]
        args = dict(action_mode="position", home_q=icub_posture, home_base=ICUB_POSE, pid_gains=gains,
                    contact_links=("l_foot", "r_foot"), z_min=0.3, max_tilt=1.0, pgs_iters=50)
        if kw.get("task") == "locomotion":
            args.update(cls.LOCOMOTION_DEFAULTS)
        # no shaping default here: the shipped model has collision shapes on the
        # soles alone, so no other link (root link, chest) can report a contact
        args.update(kw)
        return cls("icub", n_worlds, **args)

    @classmethod
    def quadruped(cls, n_worlds: int, **kw) -> "FloatVecEnv":
        """The 8-dof quadruped standing on its four feet (the shanks' spheres)."""
        args = dict(action_mode="position", home_q=[0.6, -1.2] * 4, home_base=(0.0, 0.0, 0.45, 1.0, 0.0, 0.0, 0.0),
                    pid_gains=[[400.0, 0.0, 10.0, -60.0, 60.0, 0.0, 0.0, -1.0]] * 8,
                    contact_links=("shank_fl", "shank_fr", "shank_hl", "shank_hr"), z_min=0.15, max_tilt=1.0)
        if kw.get("task") == "locomotion":
            args.update(cls.LOCOMOTION_DEFAULTS)
        if kw.get("reward_terms") and "termination_links" not in kw:
            # shaping in use: a quadruped on its trunk has fallen (the thighs of
            # the shipped model carry no collision shape, so none is penalised)
            args.update(termination_links=("trunk",))
        args.update(kw)
        return cls("quadruped", n_worlds, **args)

    # ------------------------------------------------------------------
    def _resolve_links(self, model_file: str, links: Sequence, limit: Optional[int] = MAX_CONTACT_LINKS):
        """Link names / dof indices -> the dof index of the link's body (-1 =
        the base); a link welded to its parent by fixed joints counts as the
        body it is lumped into (the iCub's soles sit on the ankles' bodies)."""
        if limit is not None and len(links) > limit:
            raise ValueError(f"at most {limit} contact links")
        known = {self.sim.base_frame: -1}
        known.update({name: i for i, name in enumerate(self.sim.link_names)})
        fixed = None
        out = []
        for link in links:
            if isinstance(link, str):
                name = link
                while name not in known:
                    if fixed is None:
                        fixed = _fixed_parents(model_file)
                    if name not in fixed:
                        raise ValueError(f"link {link!r} not found in model {self.sim.model_name!r}")
                    name = fixed[name]
                out.append(known[name])
            else:
                out.append(int(link))
        return out

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            N.lib().mw_vecenv_destroy(self._h)
            self._h = None
        if getattr(self, "sim", None) is not None:
            self.sim.close()
            self.sim = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check_actions(self, actions) -> None:
        torch = _torch()
        shape = (self.n_worlds, self.action_dim)
        if not isinstance(actions, torch.Tensor) or actions.device != self.device:
            raise TypeError(f"actions must be a torch tensor on {self.device}")
        if actions.dtype != torch.float32 or tuple(actions.shape) != shape or not actions.is_contiguous():
            raise TypeError(f"actions must be a contiguous {torch.float32} tensor of shape {shape}")

    def reset(self):
        """Reset every world (episode 0); returns obs [n_worlds, obs_dim].  The
        simulator shows the reset state at once (a paused run applies it)."""
        self.sim._cache.clear()
        N.check(N.lib().mw_vecenv_reset(self._h, self._out[0]), "reset")
        return self.obs

    def step(self, actions) -> Tuple[object, object, object, Dict]:
        """Asynchronous on the current stream; returns views of reused buffers."""
        self._check_actions(actions)
        self.sim._cache.clear()
        N.check(N.lib().mw_vecenv_step(self._h, _ptr(actions), *self._out), "step")
        return self.obs, self.reward, self.done, dict(self._info)

    def step_raw(self, actions_ptr: int) -> None:
        """Launch one step with a raw device pointer (bench / graph capture)."""
        N.check(N.lib().mw_vecenv_step(self._h, ctypes.c_void_p(actions_ptr), *self._out), "step")

    def rollout(self, actions):
        """Not available: a floating-base step is three launches, not a fused one."""
        N.check(N.lib().mw_vecenv_rollout(self._h, 1, _ptr(actions), *self._out), "rollout")

    def counters(self):
        """(episode, steps) per world as int32 tensors (copies of the uint32 counters)."""
        torch = _torch()
        ep = torch.empty((self.n_worlds,), dtype=torch.int32, device=self.device)
        st = torch.empty_like(ep)
        N.check(N.lib().mw_vecenv_counters(self._h, ctypes.c_void_p(ep.data_ptr()),
                                           ctypes.c_void_p(st.data_ptr())), "counters")
        return ep, st
