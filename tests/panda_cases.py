"""Case builders shared by tests/test_panda_cases.py (CPU, oracle alone),
tests/test_host_dyn.py and tests/test_gpu_panda_variants.py (test helper).

The shipped Panda has limits, no joint damping, no Coulomb friction, and the
config-4 env drives it with the reference's KAT gains and open clamps.  The
variants here reach the code every Panda kernel compiles but no shipped-model
test runs:

  shipped     control
  damped      DAMPING on every joint          -> needs_dual(): DUAL kernels
  frictional  FRICTION on every joint         -> friction rows
  both        DAMPING and FRICTION
  free        the Panda tree with every joint `continuous` (no limit, no
              friction: needs_cons() is false) and DAMPING, so the !CONS
              kernels must keep the implicit damping
  partial     FRICTION on joints 1, 3, 5, 7 and the first finger, DAMPING on
              the others: neighbouring dofs differ in whether they have a
              friction row, so a row mask read from the wrong dof shows

variant() returns (model file or URDF text, {(dof, MW_PARAM_*): value} for
set_joint_param before the first step, the oracle's ChainModel set up the same
way with its limits rounded to float32 as the kernels hold them).

Gains are named tuples (Gain), converted by name to the library's 8-word
layout (mw_set_joint_pid) and to the oracle's set_pid arguments, so a field
swapped in one layer cannot cancel against the same swap in the test."""

import os
from typing import NamedTuple

import numpy as np

from conftest import MODELS

DAMPING = [2.0, 5.0, 1.0, 3.0, 0.5, 0.5, 0.2, 4.0, 4.0]
FRICTION = [0.5, 1.0, 0.3, 0.8, 0.1, 0.2, 0.05, 0.5, 0.5]
VARIANTS = ("shipped", "damped", "frictional", "both", "free", "partial")

# the project's bounds (north star): one teacher-forced step, free-running q, reward
Q_STEP, QD_STEP, Q_FREE, R_REL = 1e-5, 1e-4, 1e-4, 1e-4
INSIDE, BEYOND = 1e-4, 1e-3   # threshold clearance of every start state

KAT = {  # the reference's gains (test_pid_controllers.py:20-30)
    "panda_joint1": (50, 0, 20), "panda_joint2": (10000, 0, 500),
    "panda_joint3": (100, 0, 10), "panda_joint4": (1000, 0, 50),
    "panda_joint5": (100, 0, 10), "panda_joint6": (100, 0, 10),
    "panda_joint7": (10, 0.5, 0.1), "panda_finger_joint1": (100, 0, 50),
    "panda_finger_joint2": (100, 0, 50),
}
JOINTS = list(KAT)
BIG = float(np.finfo(np.float64).max)


class Gain(NamedTuple):
    p: float
    i: float
    d: float
    imin: float = -BIG
    imax: float = BIG
    cmdmin: float = -BIG
    cmdmax: float = BIG
    offset: float = 0.0

    def words(self):
        """mw_set_joint_pid: {p, i, d, cmd_min, cmd_max, cmd_offset, i_min, i_max}."""
        return [self.p, self.i, self.d, self.cmdmin, self.cmdmax, self.offset, self.imin, self.imax]

    def to_oracle(self, ow, dof):
        ow.set_pid(dof, self.p, self.i, self.d, imax=self.imax, imin=self.imin, cmdmax=self.cmdmax,
                   cmdmin=self.cmdmin, offset=self.offset)


def free_urdf() -> str:
    """The shipped Panda with every moving joint `continuous`: same tree, same
    bodies and axes (the fingers turn about their sliding axis), no limit."""
    text = open(os.path.join(MODELS, "panda.urdf")).read()
    return text.replace('type="revolute"', 'type="continuous"').replace('type="prismatic"', 'type="continuous"')


def coefficients(name):
    """(damping, friction) per dof of a variant."""
    even = [1.0 if i % 2 == 0 else 0.0 for i in range(9)]
    if name == "partial":
        return [d * (1.0 - e) for d, e in zip(DAMPING, even)], [f * e for f, e in zip(FRICTION, even)]
    damped, frictional = name in ("damped", "both", "free"), name in ("frictional", "both")
    return [d if damped else 0.0 for d in DAMPING], [f if frictional else 0.0 for f in FRICTION]


def variant(oracle, name):
    from mwstep import native as N
    assert name in VARIANTS, name
    model = free_urdf() if name == "free" else os.path.join(MODELS, "panda.urdf")
    cm = oracle.load_urdf(model)
    assert cm.joint_names == JOINTS
    n = cm.n
    damping, friction = coefficients(name)
    params = {}
    for i in range(n):
        cm.model.lower[i] = float(np.float32(cm.model.lower[i]))
        cm.model.upper[i] = float(np.float32(cm.model.upper[i]))
        if damping[i] != 0.0:
            params[(i, N.PARAM_VISCOUS_FRICTION)] = damping[i]
            cm.model.damping[i] = damping[i]
        if friction[i] != 0.0:
            params[(i, N.PARAM_COULOMB_FRICTION)] = friction[i]
            cm.model.friction[i] = friction[i]
    return model, params, cm


def shipped_limits(oracle):
    """(lower, upper, effort) of the shipped model, limits as float32 values."""
    cm = oracle.load_urdf(os.path.join(MODELS, "panda.urdf"))
    lo = np.array([float(np.float32(cm.model.lower[i])) for i in range(cm.n)])
    hi = np.array([float(np.float32(cm.model.upper[i])) for i in range(cm.n)])
    eff = np.array([cm.model.effort[i] for i in range(cm.n)])
    return lo, hi, eff


# ------------------------------------------------------------ start states --

def step_states(oracle, W, seed, beyond=2e-3):
    """[W, 9] float32 q, qd and targets of the one-step tests: the states of
    test_group_one_step_vs_oracle (a fifth of the joints `beyond` past a limit,
    so limit rows are active) with 30 % of the velocities inside +-2e-3, where
    a friction row can hold the joint.  Joints not beyond a limit are at least
    2e-4 inside it, so no float32 rounding puts one within 1e-4 of a limit."""
    lo, hi, _ = shipped_limits(oracle)
    rng = np.random.default_rng(seed)
    q = rng.uniform(lo + 2e-4, hi - 2e-4, size=(W, 9))
    at = rng.uniform(size=q.shape) < 0.2
    q[at] = np.where(rng.uniform(size=q.shape) < 0.5, lo - beyond, hi + beyond)[at]
    qd = rng.uniform(-0.5, 0.5, size=q.shape)
    slow = rng.uniform(size=q.shape) < 0.3
    qd[slow] = rng.uniform(-2e-3, 2e-3, size=q.shape)[slow]
    tgt = np.clip(q + rng.uniform(-0.05, 0.05, size=q.shape), lo, hi)
    return q.astype(np.float32), qd.astype(np.float32), tgt.astype(np.float32)


def clearance(oracle, q):
    """(smallest distance inside a limit, smallest distance beyond one) over
    the joints of q [.., 9] against the shipped float32 limits."""
    lo, hi, _ = shipped_limits(oracle)
    q = np.asarray(q, dtype=np.float64)
    d = np.minimum(q - lo, hi - q)            # > 0 inside, < 0 beyond
    inside = d[d > 0].min() if (d > 0).any() else np.inf
    beyond = (-d[d <= 0]).min() if (d <= 0).any() else np.inf
    return float(inside), float(beyond)


# ------------------------------------------------------------------- gains --

def kat_gains():
    return [Gain(*KAT[name]) for name in JOINTS]


# A constant force per dof through the controller: p = i = d = 0, offset = tau,
# the command clamp [-0.9, 0.8] effort around it.  On the joints that gravity
# loads lightly (1, 7, the fingers) tau is below the Coulomb friction, so a
# slow joint sticks; elsewhere it slides.
TAU = [0.3, -20.0, 0.2, 12.0, -0.08, 1.5, 0.03, 0.2, -0.3]


def force_gains(oracle):
    _, _, eff = shipped_limits(oracle)
    return [Gain(0.0, 0.0, 0.0, cmdmin=-0.9 * eff[d], cmdmax=0.8 * eff[d], offset=TAU[d]) for d in range(9)]


def clamped_gains(oracle, scale=1.0):
    """The asymmetric clamped set of the rollout: ki = 0.2 kp, integral clamp
    [-0.3, 0.5], command clamp [-0.4, 0.6] effort, offset 0.3, each scaled by
    a per-dof factor so that all eight words differ between dofs and no two
    fields of a dof coincide.  Joint 4 has the reference's empty command range
    (max < min: no clamp), so only the engine's effort clip bounds it."""
    _, _, eff = shipped_limits(oracle)
    out = []
    for d, name in enumerate(JOINTS):
        kp, _, kd = KAT[name]
        f = scale * (1.0 + 0.07 * d)
        g = Gain(kp * scale, 0.2 * kp * scale, kd * scale, imin=-0.3 * f, imax=0.5 * f,
                 cmdmin=-0.4 * eff[d] * f / (1.0 + 0.07 * 8), cmdmax=0.6 * eff[d] * f / (1.0 + 0.07 * 8),
                 offset=0.3 * f)
        if d == 3:
            g = g._replace(cmdmin=0.0, cmdmax=-1.0)
        out.append(g)
    return out


# ------------------------------------------------------------ oracle worlds --

def oracle_world(oracle, cm, q, qd, gains, dt=1e-3, spr=1):
    """A ScenarioWorld in Position mode on every joint, controller period = dt,
    20 sweeps, PID state fresh, targets = q."""
    ow = oracle.ScenarioWorld(cm, dt, spr, 20)
    ow.q, ow.qd = np.asarray(q, dtype=float).copy(), np.asarray(qd, dtype=float).copy()
    ow.period_ns = int(round(dt * 1e9))
    for d in range(cm.n):
        gains[d].to_oracle(ow, d)
        ow.set_mode(d, oracle.POSITION)
    return ow


def oracle_one_step(oracle, cm, q, qd, tgt, gains):
    """One PID step of every world from a fresh controller: (q, qd) [W, 9]."""
    W = len(q)
    oq, oqd = np.zeros((W, cm.n)), np.zeros((W, cm.n))
    for w in range(W):
        ow = oracle_world(oracle, cm, q[w], qd[w], gains)
        ow.ptgt[:] = tgt[w]
        ow.run()
        oq[w], oqd[w] = ow.q, ow.qd
    return oq, oqd


def force_step_rows(oracle, cm, q, qd):
    """The engine step of the constant-force case with the oracle's row report:
    (q, qd, limit_row, friction_row), each [W, 9]."""
    W, n = len(q), cm.n
    oq, oqd = np.zeros((W, n)), np.zeros((W, n))
    lim, fric = np.zeros((W, n), np.int32), np.zeros((W, n), np.int32)
    for w in range(W):
        oq[w], oqd[w], lim[w], fric[w] = oracle.step_rows(
            cm, 1e-3, q[w].astype(float), qd[w].astype(float), [oracle.FORCE] * n, TAU, 20)
    return oq, oqd, lim, fric


# ----------------------------------------------------------------- rollout --

ROLL_W, ROLL_H, ROLL_TLIM, ROLL_SEED = 16, 300, 150, 3


def reset_state(oracle, cm, seed, world, episode):
    """The env kernels' reset (pid_task_reset): home pose + U(-0.05, 0.05) from
    Philox4x32-10 keyed by the seed, counter (world, episode, block, 0)."""
    from test_gpu_panda import _panda_reset_ref
    return _panda_reset_ref(oracle, cm, seed, world, episode)


def rollout_start(oracle):
    """[16, 9] float32 start poses of the rollout: the reset pose of episode 0,
    joint 2 mirrored in every other world (gravity loads joints 2 and 4 in
    either direction, so the integral clamp binds on both sides) and joint 4
    0.18 rad below its upper limit, where the 0.3 rad sinusoid drives it into
    the limit."""
    _, _, cm = variant(oracle, "shipped")
    q0 = np.stack([reset_state(oracle, cm, ROLL_SEED, w, 0) for w in range(ROLL_W)])
    q0[1::2, 1] = -q0[1::2, 1]
    q0[:, 3] = np.float32(-0.0698 - 0.18) - np.float32(0.01) * np.arange(ROLL_W, dtype=np.float32)
    # the reset clips the fingers onto their limits in many worlds: episode 0
    # starts them inside (the episode after the TimeLimit reset starts where
    # the kernels' own reset puts them, on the float32 limits both sides hold)
    q0[:, 7] = 0.012 + 0.001 * np.arange(ROLL_W)
    q0[:, 8] = 0.030 - 0.001 * np.arange(ROLL_W)
    return q0.astype(np.float32)


def rollout_targets(base, k, dt_run=1e-3):
    """Targets [W, 9] float32 of env step k of an episode that started at
    `base`: the KAT sinusoids on joints 1 and 6 (test_panda_vecenv_vs_oracle),
    1 Hz, 0.3 rad on joint 4, a phase per world."""
    W = len(base)
    t = k * dt_run
    phase = np.linspace(0, np.pi, W)
    tgt = base.astype(np.float64).copy()
    tgt[:, 0] += 0.9 * 2.8973 * np.sin(2 * np.pi * 0.33 * t + phase)
    tgt[:, 5] += 0.9 * 1.885 * np.sin(2 * np.pi * 0.33 * t + phase)
    tgt[:, 3] += 0.3 * np.sin(2 * np.pi * 1.0 * t + 0.25 * phase)
    return tgt.astype(np.float32)


_rollouts = {}


def oracle_rollout(oracle, name, spr, gains=None, regain=None, H=ROLL_H, start=None):
    """The free-running oracle trajectory of the rollout case, computed once
    per (variant, steps_per_run) and shared: per env step k the targets, the
    observation after the step (before the TimeLimit reset at step 150
    replaces it: the terminal observation), the reward and the PID state.
    `regain` = (step, gains): the gains are replaced before that step (a new
    PID: its state resets, Joint.cpp:479-525)."""
    key = (name, spr, H, regain is not None, gains is not None, start is not None)
    if key in _rollouts:
        return _rollouts[key]
    _, _, cm = variant(oracle, name)
    gains = gains or clamped_gains(oracle)
    dt = 1e-3 / spr
    q0 = rollout_start(oracle) if start is None else start
    W = len(q0)
    ows = [oracle_world(oracle, cm, q0[w], np.zeros(9), gains, dt, spr) for w in range(W)]
    base = q0.copy()
    out = dict(q0=q0, tgt=np.zeros((H, W, 9), np.float32), obs=np.zeros((H, W, 18)), reward=np.zeros((H, W)),
               ierr=np.zeros((H, W, 9)), cmd=np.zeros((H, W, 9)), reset=np.zeros((H, W, 9), np.float32),
               done=np.zeros(H, bool))
    k_ep = 0
    for k in range(H):
        if regain is not None and k == regain[0]:
            for ow in ows:
                for d in range(9):
                    regain[1][d].to_oracle(ow, d)
            gains = regain[1]
        tgt = rollout_targets(base, k_ep)
        out["tgt"][k] = tgt
        for w, ow in enumerate(ows):
            ow.ptgt[:] = tgt[w]
            ow.run()
            out["obs"][k, w] = np.concatenate([ow.q, ow.qd])
            out["reward"][k, w] = -float(np.sum((ow.q - tgt[w].astype(np.float64)) ** 2))
            out["ierr"][k, w] = [ow.state[d].ierr for d in range(9)]
            out["cmd"][k, w] = [ow.state[d].cmd for d in range(9)]
        k_ep += 1
        if (k + 1) % ROLL_TLIM == 0:
            out["done"][k] = True
            ep = (k + 1) // ROLL_TLIM
            for w in range(W):
                qr = reset_state(oracle, cm, ROLL_SEED, w, ep)
                out["reset"][k, w] = qr
                prev = ows[w]
                ows[w] = oracle_world(oracle, cm, qr, np.zeros(9), gains, dt, spr)
                ows[w].iterations = prev.iterations
                ows[w].prev_ns = 0
            base = out["reset"][k].copy()
            # the kernels' reset clips most fingers onto a limit (home 0.02 +-
            # 0.05 in a 0.04 range).  Held there by its target, a finger would
            # sit within rounding of the limit, where fp32 and fp64 disagree
            # on whether the row is active (a threshold case, not an error of
            # either); a mid-range target pulls it clear within a few steps.
            base[:, 7:] = 0.02
            k_ep = 0
    out["gains"] = gains
    _rollouts[key] = out
    return out


# ------------------------------------------------------------ wave sharing --

def wave_sharing_worlds(oracle, k=4, seed=31):
    """(quiet, loaded): k worlds each as rows [q | qd | target] ([k, 27]
    float32).  Quiet worlds have every joint in the middle 60 % of its range
    (no limit row on the shipped model); loaded worlds have three to five
    joints 2 mrad beyond a limit."""
    lo, hi, _ = shipped_limits(oracle)
    rng = np.random.default_rng(seed)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    quiet = mid + rng.uniform(-0.6, 0.6, size=(k, 9)) * half
    loaded = mid + rng.uniform(-0.6, 0.6, size=(k, 9)) * half
    for w in range(k):
        dofs = rng.choice(9, size=3 + w % 3, replace=False)
        loaded[w, dofs] = np.where(rng.uniform(size=len(dofs)) < 0.5, lo[dofs] - 2e-3, hi[dofs] + 2e-3)
    return quiet.astype(np.float32), loaded.astype(np.float32)


def wave_sharing_rows(oracle, k=4, seed=31):
    """The same worlds with their velocities and targets: (quiet, loaded), each [k, 27]."""
    lo, hi, _ = shipped_limits(oracle)
    q0, q1 = wave_sharing_worlds(oracle, k, seed)
    rng = np.random.default_rng(seed + 1)
    out = []
    for q in (q0, q1):
        qd = rng.uniform(-0.5, 0.5, size=q.shape)
        tgt = np.clip(q.astype(np.float64) + rng.uniform(-0.05, 0.05, size=q.shape), lo, hi)
        out.append(np.concatenate([q, qd, tgt], axis=1).astype(np.float32))
    return out
