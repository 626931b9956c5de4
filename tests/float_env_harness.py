"""What the GPU tests of the floating-base env (tests/test_gpu_float_env*.py,
_rand, _loco, _noise, _shape, _inertia*, _joints*) share: the env and its
host-commanded twin Simulator, the restatements of the device's draws from the
oracle's Philox4x32-10, the fp64 restatement of the locomotion reward, the
graph-capture helper, the float32 helpers of the shaping tests, and the
lockstep driver of the randomised-parameter parity tests.

A plain module like the *_cases.py / *_ref.py helpers: no tests, no fixtures.
The names keep the leading underscore they had in the test modules they came
from, where `twin`, `nominal` or `limits` are the usual local variables."""

import ctypes
import math
import os

import numpy as np

from float_joints_ref import DAMPING, EFFORT, FRICTION, draw_ref, harness_apply

# the quadruped's stand posture and the gains FloatVecEnv.quadruped defaults to
STAND = [0.6, -1.2] * 4
QUAD_GAINS = [[400.0, 0.0, 10.0, -60.0, 60.0, 0.0, 0.0, -1.0]] * 8
FREE = dict(z_min=-10.0, max_tilt=math.pi)           # no termination by height or tilt
PUSH = dict(push_interval=7, push_steps=2, push_force=30.0, push_torque=5.0)
# the locomotion task as the randomisation tests turn it on
LOCO = dict(task="locomotion", command_ranges=((-1.0, 1.0), (-0.5, 0.5), (-1.0, 1.0)), cmd_interval=3,
            cmd_zero_prob=0.2, w_action_rate=0.01)
# ... and with every reward term on, so that each shows in the restatement (_RewardRef)
RANGES = ((-1.0, 1.0), (-0.5, 0.5), (-1.0, 1.0))
LOCO_EVERY_TERM = dict(task="locomotion", command_ranges=RANGES, cmd_interval=3, cmd_zero_prob=0.2, cmd_min=0.1,
                       w_action=0.01, w_pose=0.1, w_track_lin=1.0, w_track_yaw=0.5, track_sigma=0.25, w_lin_z=2.0,
                       w_ang_xy=0.05, w_action_rate=0.01, w_air_time=1.0, air_time_target=0.01, contact_force_min=1.0)
# the joint randomisation ranges _check_draws restates
DAMP, FRIC, EFF = (0.0, 0.5), (0.0, 2.0), (0.1, 1.0)
JOINTS = dict(joint_damping_range=DAMP, joint_friction_range=FRIC, effort_scale_range=EFF)
# every shaping term on
ALL = dict(torque=2e-5, power=1e-4, joint_acc=2.5e-7, orientation=1.0, base_height=10.0, joint_limits=5.0,
           collision=1.0, stumble=0.5, contact_force=0.01, stand_still=0.2)
EPISODE_BLOCK = 0x40000000


# ---- the env and its twin ----

def _make(kind, W, **kw):
    from mwstep import FloatVecEnv
    env = getattr(FloatVecEnv, kind)(W, **kw)
    env._pgs_iters = kw.get("pgs_iters", 50 if kind == "icub" else 20)
    return env


def _twin(env, model, gains=None):
    """A host-commanded Simulator configured as the env's."""
    from mwstep import get_model_file
    from mwstep import native as N
    from mwstep.sim import Simulator
    s = env.sim
    if not (model.lstrip().startswith("<") or os.path.exists(model)):      # else: a URDF text or file
        model = get_model_file(model)
    twin = Simulator(model, n_worlds=env.n_worlds, step_size=s.step_size,
                     steps_per_run=s.steps_per_run, pgs_iters=env._pgs_iters, pose=tuple(env.home_base.tolist()))
    twin.set_ground_plane(True, 1.0)
    twin.enable_contacts(True)
    for d, g in enumerate(gains or []):
        twin.set_pid(d, g)
    if env.action_mode == "position":
        twin.set_controller_period(s.step_size)
        twin.set_control_mode(N.MODE_POSITION)
    else:
        twin.set_control_mode(N.MODE_FORCE)
    return twin


def _reset_twin(twin, obs, worlds=None):
    """Reset worlds of the twin through the host setters with the values of the env's obs rows."""
    n = twin.dofs
    if worlds is None:
        twin.set("reset_q", obs[:, 13:13 + n].astype(np.float64))
        twin.set("reset_qd", obs[:, 13 + n:13 + 2 * n].astype(np.float64))
        twin.reset_base_pose(obs[:, :7].astype(np.float64))
        twin.reset_base_velocity(obs[:, 7:13].astype(np.float64))
        return
    for w in worlds:
        twin.set("reset_q", obs[w:w + 1, 13:13 + n].astype(np.float64), w0=w, nw=1)
        twin.set("reset_qd", obs[w:w + 1, 13 + n:13 + 2 * n].astype(np.float64), w0=w, nw=1)
        twin.reset_base_pose(obs[w, :7].astype(np.float64), w0=w, nw=1)
        twin.reset_base_velocity(obs[w, 7:13].astype(np.float64), w0=w, nw=1)


def _link_forces(twin, links, w):
    c, b = twin.contacts(w), twin.contact_bodies(w)
    return np.array([c[b == link, 8].sum() for link in links])


def _check_obs(obs, twin, links, worlds=None):
    """obs rows against the twin's getters (after the same step)."""
    n = twin.dofs
    ws = np.arange(twin.n_worlds) if worlds is None else np.asarray(worlds)
    np.testing.assert_array_equal(obs[ws, :7], twin.base_pose()[ws].astype(np.float32))
    np.testing.assert_array_equal(obs[ws, 13:13 + n], twin.get("q")[ws].astype(np.float32))
    np.testing.assert_array_equal(obs[ws, 13 + n:13 + 2 * n], twin.get("qd")[ws].astype(np.float32))
    v = twin.base_velocity()[ws]
    err_v = float((np.abs(obs[ws, 7:13] - v) / np.maximum(1.0, np.abs(v))).max())
    f = np.array([_link_forces(twin, links, w) for w in ws])
    got = obs[ws, 13 + 2 * n:]
    err_f = float((np.abs(got - f) / np.maximum(1.0, np.abs(f))).max()) if len(links) else 0.0
    return err_v, err_f


def _dev(env, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(env.device)


# ---- the simulator alone: a quadruped in contact under torques ----

def _quadruped(W):
    from mwstep import get_model_file
    from mwstep import native as N
    from mwstep.sim import Simulator
    sim = Simulator(get_model_file("quadruped"), n_worlds=W, pose=(0, 0, 0.43, 1, 0, 0, 0))
    assert sim.float_kernel() == 2
    sim.set_ground_plane(True, 1.0)
    sim.enable_contacts(True)
    sim.set_control_mode(N.MODE_FORCE)
    return sim


def _run_quadruped(sim, torques, worlds=None, watch=None):
    """The stand posture 1 cm lower than where it stands on the shanks' spheres
    (z = 0.44), so the feet are in contact from the first step; then one
    run per row of torques [steps, W, 8].  watch: a list that receives, per
    step, how many of worlds 0, W // 2, W - 1 have contact points."""
    W = sim.n_worlds
    sim.set("reset_q", np.tile(np.float64(STAND), (W, 1)))
    sim.run(paused=True)
    for tau in torques:
        sim.set("force_target", tau if worlds is None else tau[worlds])
        sim.run()
        if watch is not None:
            watch.append(sum(len(sim.contacts(w)) > 0 for w in (0, W // 2, W - 1)))
    return sim.get_state()


# ---- the device's draws, restated ----

def _unif32(x, lo, hi):
    t = np.float32((x >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0))
    return np.float32(lo) + (np.float32(hi) - np.float32(lo)) * t


def _philox(oracle, seed, world, episode, block):
    return oracle.philox_raw([world, episode, block, 0], [seed & 0xFFFFFFFF, seed >> 32])


def _key(seed):
    return [seed & 0xFFFFFFFF, seed >> 32]


def _noise_terms(oracle, seed, g, episode, t, amp):
    """amp[k] u of one row in fp64, from the stated draw; words of amplitude zero draw nothing."""
    out = np.zeros(len(amp))
    for b in range((len(amp) + 3) // 4):
        ks = [k for k in range(4 * b, min(4 * b + 4, len(amp))) if amp[k] != 0]
        if ks:
            x = oracle.philox_raw([g, episode, b, 1 + t], _key(seed))
            for k in ks:
                out[k] = float(amp[k]) * (-1.0 + float(int(x[k & 3]) >> 8) * 2.0 ** -23)
    return out


def _check_rows(oracle, seed, offset, amp, noisy, clean, worlds, episode, steps):
    """Rows of `worlds`: noisy - clean is the stated draw; returns the worst error / bound."""
    nz = amp != 0
    worst = 0.0
    for w in worlds:
        c64 = clean[w].astype(np.float64)
        ref = c64 + _noise_terms(oracle, seed, offset + int(w), int(episode[w]), int(steps[w]), amp)
        bound = 2.0 ** -23 * (np.abs(c64) + amp.astype(np.float64))
        err = np.abs(noisy[w].astype(np.float64) - ref)
        assert (err[nz] <= bound[nz]).all(), f"world {w}: worst error / bound {(err[nz] / bound[nz]).max():.3f}"
        worst = max(worst, float((err[nz] / bound[nz]).max()))
        np.testing.assert_array_equal(noisy[w, ~nz].view(np.uint32), clean[w, ~nz].view(np.uint32))
    return worst


def _delay_ref(oracle, seed, g, episode, lo, hi):
    r = oracle.philox_raw([g, episode, EPISODE_BLOCK, 0], _key(seed))
    return lo + int(r[2]) % (hi - lo + 1)


def _nominal(sim):
    return np.stack([sim.joint_dynamics(d, [0])[0] for d in range(sim.dofs)])


def _check_draws(env, oracle, fj, seed, episode, dofs, nominal, worlds, offset=0):
    """env.joint_draws against the restatement, env.joint_dynamics against the
    host build of the kernel's code on those draws; returns the worst draw
    error over its bound."""
    n = env.action_dim
    draws, words = env.joint_draws.cpu().numpy(), env.joint_dynamics.cpu().numpy()
    assert draws.shape == words.shape == (env.n_worlds, n, 3)
    sel = list(range(n)) if dofs is None else list(dofs)
    rest = [d for d in range(n) if d not in sel]
    # masked-out joints: draws 0, 0, 1 and the nominal words
    np.testing.assert_array_equal(draws[:, rest], np.tile(np.float32([0.0, 0.0, 1.0]), (env.n_worlds, len(rest), 1)))
    np.testing.assert_array_equal(words[:, rest], np.tile(nominal[rest], (env.n_worlds, 1, 1)))
    tol = np.array([4 * 2.0 ** -23 * (r[1] - r[0]) for r in (DAMP, FRIC, EFF)])
    for e, r in enumerate((DAMP, FRIC, EFF)):
        assert r[0] - tol[e] <= draws[:, sel, e].min() and draws[:, sel, e].max() <= r[1] + tol[e]
    worst = 0.0
    for w in worlds:
        ref = draw_ref(oracle, seed, offset + w, episode, n, DAMP, FRIC, EFF, dofs)
        worst = max(worst, float((np.abs(draws[w].astype(np.float64) - ref) / tol).max()))
    assert worst <= 1.0, worst
    # the words from the reported draws: the kernel's code on the host, bit for bit
    want = harness_apply(fj, DAMPING | FRICTION | EFFORT, np.tile(nominal, (env.n_worlds, 1, 1)), draws)
    np.testing.assert_array_equal(words, want)
    for d in (sel[0], sel[-1]) + ((rest[0],) if rest else ()):
        np.testing.assert_array_equal(env.sim.joint_dynamics(d), words[:, d])
    return worst


# ---- the locomotion reward, restated ----

def _f(x):
    """The float32 the env holds for a configured value, as fp64."""
    return float(np.float32(x))


class _RewardRef:
    """fp64 restatement of the locomotion reward with its own previous action and air counters."""

    def __init__(self, env, kw):
        self.env, self.kw = env, kw
        self.n, self.sl = env.action_dim, env.obs_slices
        self.prev = np.zeros((env.n_worlds, self.n))
        self.air = np.zeros((env.n_worlds, len(env.contact_links)), np.int64)
        self.cmd = None
        self.touchdowns = 0          # with air_steps > 0 under a command above cmd_min
        self.worst = 0.0             # |reward - restatement| / bound
        self.env_dt = _f(env.sim.steps_per_run * env.sim.step_size)

    def start(self, obs):
        """The reset observation: its command is the one the first step runs under."""
        self.cmd = obs[:, self.sl["command"]].astype(np.float64)
        np.testing.assert_array_equal(obs[:, self.sl["last_action"]], 0.0)
        np.testing.assert_array_equal(obs[:, self.sl["body_velocity"]], 0.0)

    def step(self, a, obs, term_obs, done, reward):
        kw, sl, n = self.kw, self.sl, self.n
        g = lambda name, default=0.0: _f(kw.get(name, default))
        rows = np.where(done[:, None], term_obs, obs).astype(np.float64)
        a64 = a.astype(np.float64)
        z, qx, qy = rows[:, 2], rows[:, 4], rows[:, 5]
        term = (z < g("z_min")) | (1 - 2 * (qx * qx + qy * qy) < _f(math.cos(kw.get("max_tilt", math.pi))))
        v, om = rows[:, sl["body_velocity"]][:, :3], rows[:, sl["body_velocity"]][:, 3:]
        c = self.cmd
        contact = rows[:, sl["contacts"]] > g("contact_force_min")
        touchdown = contact & (self.air > 0)
        pay = np.where(touchdown, self.air * self.env_dt - g("air_time_target"), 0.0).sum(axis=1)
        fast = c[:, 0] ** 2 + c[:, 1] ** 2 > g("cmd_min") ** 2
        self.touchdowns += int((touchdown & fast[:, None]).sum())
        self.air = np.where(contact, 0, self.air + 1)
        sigma = g("track_sigma", 0.25)
        terms = np.stack([
            np.where(term, 0.0, g("alive_bonus", 1.0)),
            g("w_forward", 1.0) * rows[:, 7],
            -g("w_action") * (a64 ** 2).sum(axis=1),
            -g("w_pose") * ((rows[:, 13:13 + n] - self.env.home_q.astype(np.float64)) ** 2).sum(axis=1),
            g("w_track_lin", 1.0) * np.exp(-((c[:, 0] - v[:, 0]) ** 2 + (c[:, 1] - v[:, 1]) ** 2) / sigma),
            g("w_track_yaw", 0.5) * np.exp(-((c[:, 2] - om[:, 2]) ** 2) / sigma),
            -g("w_lin_z") * v[:, 2] ** 2,
            -g("w_ang_xy") * (om[:, 0] ** 2 + om[:, 1] ** 2),
            -g("w_action_rate") * ((a64 - self.prev) ** 2).sum(axis=1),
            np.where(fast, g("w_air_time") * pay, 0.0)], axis=1)
        bound = 2.0 ** -23 * (n + 8) * np.abs(terms).sum(axis=1)
        self.worst = max(self.worst, float((np.abs(reward - terms.sum(axis=1)) / bound).max()))
        # the new words of the rows
        np.testing.assert_array_equal(rows[:, sl["last_action"]], a64)
        np.testing.assert_array_equal(obs[done][:, sl["last_action"]], 0.0)
        w, x, y, zz = rows[:, 3], rows[:, 4], rows[:, 5], rows[:, 6]
        grav = -np.stack([2 * (x * zz - w * y), 2 * (y * zz + w * x), 1 - 2 * (x * x + y * y)], axis=1)
        assert float(np.abs(rows[:, sl["gravity"]] - grav).max()) <= 2e-6
        self.prev = np.where(done[:, None], 0.0, a64)
        self.air[done] = 0
        self.cmd = obs[:, sl["command"]].astype(np.float64)
        return rows


# ---- the shaping terms: float32 inputs of the host build ----

def _forces32(sim, w, links):
    """The summed force vector of every link's contact points, float32, in the getters' (slot) order."""
    c, b = sim.contacts(w), sim.contact_bodies(w)
    out = np.zeros((len(links), 3), np.float32)
    for j, link in enumerate(links):
        f = np.zeros(3, np.float32)
        for row in c[b == link]:
            f = (f + row[6:9].astype(np.float32)).astype(np.float32)
        out[j] = f
    return out


def _limits(fs, sim, soft):
    from mwstep import native as N
    n = sim.dofs
    lower = np.float32([sim.joint_param(d, N.PARAM_POSITION_LIMIT_MIN) for d in range(n)])
    upper = np.float32([sim.joint_param(d, N.PARAM_POSITION_LIMIT_MAX) for d in range(n)])
    return fs.soft_limits(lower, upper, np.float32(soft))


def _params(fs, env, kw):
    g = lambda name, default: np.float32(kw.get(name, default))
    return fs.params(kw.get("reward_terms", {}), g("base_height_target", env.home_base[2]),
                     g("collision_force_min", 0.1), g("stumble_ratio", 5.0), g("max_contact_force", 100.0),
                     g("termination_force", 1.0), np.float32(env.sim.steps_per_run * env.sim.step_size))


# ---- graph capture ----

def _loaded_hip():
    """The HIP runtime this process already uses."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("the HIP runtime is not loaded")


def _captured_step_graph(env, actions):
    """Capture one env.step into a HIP graph (never launched): its node types and edges."""
    import torch
    hip = _loaded_hip()
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream(env.device).cuda_stream)
    graph = vp()
    assert hip.hipStreamBeginCapture(stream, 2) == 0      # relaxed mode
    try:
        env.step_raw(actions.data_ptr())
    finally:
        rc = hip.hipStreamEndCapture(stream, ctypes.byref(graph))
    assert rc == 0 and graph.value
    n = ctypes.c_size_t()
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    nodes = (vp * n.value)()
    assert hip.hipGraphGetNodes(graph, nodes, ctypes.byref(n)) == 0
    types = []
    for node in nodes:
        t = ctypes.c_int()
        assert hip.hipGraphNodeGetType(vp(node), ctypes.byref(t)) == 0
        types.append(t.value)
    m = ctypes.c_size_t()
    assert hip.hipGraphGetEdges(graph, None, None, ctypes.byref(m)) == 0
    src, dst = (vp * m.value)(), (vp * m.value)()
    assert hip.hipGraphGetEdges(graph, src, dst, ctypes.byref(m)) == 0
    edges = [(list(nodes).index(a), list(nodes).index(b)) for a, b in zip(src, dst)]
    hip.hipGraphDestroy(graph)
    return types, edges


# ---- lockstep with per-world records ----

def _carry_records(twin, env, carry, worlds=None):
    """The env's reported per-world words of `carry` into the twin (all worlds, or `worlds`)."""
    if "inertial" in carry:
        inertial = env.inertial.cpu().numpy()
        for link in range(-1, twin.dofs):
            words = inertial[:, link + 1]
            twin.set_link_params(link, words if worlds is None else words[worlds], worlds)
    if "joint_dynamics" in carry:
        joints = env.joint_dynamics.cpu().numpy()
        for d in range(twin.dofs):
            words = joints[:, d]
            twin.set_joint_dynamics(d, words if worlds is None else words[worlds], worlds)


def _parity(env, twin, actions_of, steps, H, command_of, carry):
    """env (pushes, friction randomisation and the locomotion task on, episodes
    of H steps) and twin in lockstep; the twin is given the reported wrench of
    every step and, at every reset, the reported friction, reset state and the
    per-world records `carry` names: "inertial" (env.inertial through
    set_link_params), "joint_dynamics" (env.joint_dynamics through
    set_joint_dynamics) or both.  The state records stay bit-equal; info[name]
    is env.<name>; the words of a record change where, and only where, an
    episode ended; the simulator's getters read the words in force back.
    Returns {name: the words of every episode, first to last}."""
    import torch
    obs = env.reset().cpu().numpy()
    _carry_records(twin, env, carry)
    twin.set_ground_friction(env.friction.cpu().numpy().astype(np.float64))
    _reset_twin(twin, obs)
    twin.run(paused=True)
    np.testing.assert_array_equal(env.sim.get_state(), twin.get_state())
    duration = env.sim.steps_per_run * env.sim.step_size
    words = {name: getattr(env, name).cpu().numpy().copy() for name in carry}
    seen = {name: [words[name]] for name in carry}
    for k in range(1, steps + 1):
        a = actions_of(k)
        o, _, d, info = env.step(torch.from_numpy(a).to(env.device))
        d = d.cpu().numpy().astype(bool)
        twin.apply_world_wrench(-1, info["push"].cpu().numpy().astype(np.float64), duration)
        command_of(twin, a)
        twin.run()
        np.testing.assert_array_equal(env.sim.get_state(), twin.get_state(), err_msg=f"state after step {k}")
        assert d.all() == (k % H == 0) and d.any() == (k % H == 0)
        for name in carry:
            assert info[name] is getattr(env, name)
            new = info[name].cpu().numpy()
            # the words change where, and only where, an episode ended
            np.testing.assert_array_equal((new != words[name]).any(axis=(1, 2)), d,
                                          err_msg=f"{name} changes at step {k}")
            if d.any():
                words[name] = new.copy()
                seen[name].append(words[name])
        if d.any():
            done = np.flatnonzero(d)
            _carry_records(twin, env, carry, done)
            twin.set_ground_friction(info["friction"].cpu().numpy().astype(np.float64))
            _reset_twin(twin, o.cpu().numpy(), done)
        if "inertial" in carry:
            for link in (-1, twin.dofs - 1):
                np.testing.assert_array_equal(env.sim.link_params(link), words["inertial"][:, link + 1])
        if "joint_dynamics" in carry:
            for dof in (0, twin.dofs - 1):
                np.testing.assert_array_equal(env.sim.joint_dynamics(dof), words["joint_dynamics"][:, dof])
    assert all(len(episodes) == 1 + steps // H for episodes in seen.values())
    assert env.sim.constraint_overflow() == twin.constraint_overflow()
    return seen
