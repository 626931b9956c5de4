"""Floating trees of 33..48 joints: the models and start states of the tests
of the wave kernel's 48-body instances (test_gpu_big_tree.py,
test_gpu_float_env_big.py) and of their CPU proof (test_big_tree_cases.py).
numpy and the fp64 oracle only, no GPU.

A tree is a list of limbs hanging from the base, each a trunk followed by
branches hanging from the trunk's end, numbered in DFS order, and built by
test_gpu_float_tree.tree_urdf (random axes, frames and masses, a prismatic
joint every fifth body, a sphere on every leaf):

  tree33   33 joints, one past the 32-body instance; a three-way branch point
  tree40   40 joints, four limbs of 5 + (3, 2)
  tree48   48 joints (kMaxBodies), depth exactly 12 (kWaveMaxDepth)

and the variants `d` (joint damping: the dual recursion), `f` (Coulomb
friction on every second joint: one LCP row per moving joint), `u`
(continuous joints only, no friction: no constraint row can come from a
joint, the CONS = false instances) and `w` (the same tree welded to the
world).

The start states are float_oracle_check.random_states with the seed of the
one-step tests; the `u` variant, whose joints have no range to draw from,
starts from its limited sibling's states.
"""

import functools

import numpy as np

from float_oracle_check import QD_TOL, RES_TOL, oracle_step, random_states  # noqa: F401 (re-exported)
from test_gpu_float_tree import tree_urdf

W, MU, SEED, STATE_SEED = 256, 0.8, 7, 11

LIMBS = {
    "tree33": [(5, (3, 2, 2)), (5, (3, 2)), (6, (3, 2))],
    "tree40": [(5, (3, 2))] * 4,
    "tree48": [(8, (4,)), (5, (4, 3)), (5, (4, 3)), (5, (4, 3))],
}
VARIANTS = {"": {}, "d": dict(damping=2.0), "f": dict(friction=0.3, friction_every=2), "u": dict(unlimited=True),
            "w": dict(welded=True)}

# what the GPU tests run
PGS_MODELS = ["tree33", "tree40", "tree48", "tree48d"]
EXACT_MODELS = ["tree33", "tree40", "tree48", "tree48d", "tree48f", "tree48u"]
WELDED = "tree48w"
FLOATING = sorted(set(PGS_MODELS + EXACT_MODELS))


def parents_of(limbs):
    """DFS-ordered parent list of limbs [(trunk length, (branch lengths))]."""
    parents = []
    for trunk, branches in limbs:
        first = len(parents)
        parents += [-1] + list(range(first, first + trunk - 1))
        end = len(parents) - 1
        for b in branches:
            first = len(parents)
            parents += [end] + list(range(first, first + b - 1))
    return parents


def depth_of(parents):
    d = []
    for pa in parents:
        d.append(1 if pa < 0 else d[pa] + 1)
    return max(d)


def split(name):
    base = name[:6]
    return base, name[6:]


def parents(name):
    return parents_of(LIMBS[split(name)[0]])


def urdf(name):
    base, var = split(name)
    return tree_urdf(parents=parents_of(LIMBS[base]), seed=SEED, **VARIANTS[var])


@functools.lru_cache(maxsize=None)
def states(name, n_worlds=W):
    """(q, qd, pose, vel, tau) of `name`, float32-rounded; every variant of a
    tree starts from the same numbers."""
    import pyoracle
    base, _ = split(name)
    cm = pyoracle.load_urdf(urdf(base))
    out = random_states(cm, n_worlds, np.random.default_rng(STATE_SEED))
    for a in out:
        a.setflags(write=False)
    return out


def oracle_world(oracle, cm, name, w, pgs_iters, tau=None, qd=None, world=None, wrench=None):
    """One oracle step of world `w` from its start state (`world`: another
    world's state; tau / qd: replacements)."""
    q, qd0, pose, vel, tau0 = states(name)
    k = w if world is None else world
    return oracle_step(oracle, cm, pose[k], vel[k], q[k], qd0[k] if qd is None else qd,
                       tau0[k] if tau is None else tau, MU, pgs_iters, wrench)


def survey(oracle, name, n_worlds=W):
    """The converged oracle over every world: dict of per-world arrays
    n_contacts, high (a contact on a body >= 32), rows (LCP rows), res (the
    solve's residual) and qd [W, n]."""
    cm = oracle.load_urdf(urdf(name))
    nc, high, rows, res, qd = [], [], [], [], []
    for w in range(n_worlds):
        ow = oracle_world(oracle, cm, name, w, oracle.PGS_CONVERGED)
        prob = oracle.lcp_last()
        nc.append(len(ow.contacts))
        high.append(any(c[3] >= 32 for c in ow.contacts))
        rows.append(0 if prob is None else len(prob["b"]))
        res.append(oracle.pgs_stats()[1] if prob is not None else 0.0)
        qd.append(ow.qd)
    return dict(cm=cm, n_contacts=np.array(nc), high=np.array(high), rows=np.array(rows), res=np.array(res),
                qd=np.array(qd))


def row_buckets(rows):
    """worlds per row width of the exact solve (wave_lcp.hpp): <= 16, 17..32, 33..64, beyond"""
    rows = np.asarray(rows)
    return (int(((rows > 0) & (rows <= 16)).sum()), int(((rows > 16) & (rows <= 32)).sum()),
            int(((rows > 32) & (rows <= 64)).sum()), int((rows > 64).sum()))


def unconverged(res):
    return int((~((res >= 0.0) & (res <= RES_TOL))).sum())


SENSITIVE_BY = 10 * QD_TOL

# -- the closed loop: tree48 in free fall (no ground: the motion is smooth) under the JointController PID on
# all 48 joints, from a random posture at rest to targets up to 0.3 rad / 0.04 m away
# q bound; p, i, d, |cmd| limit, |i term| limit
CL_WORLDS, CL_BOUND, CL_PID, CL_SEED = 8, 1e-4, (60.0, 12.0, 1.5, 50.0, 5.0), 17
# the longest horizon <= 200 steps at which the oracle's own trajectory moves by less than CL_BOUND / 10 when
# its inputs are perturbed by 3e-7 relative (test_big_tree_cases.test_closed_loop_horizon)
CL_STEPS = 200


def closed_loop_inputs(oracle, name="tree48"):
    """(cm inserted at z = 1 m, posture [CL_WORLDS, n], target [CL_WORLDS, n]), float32 values"""
    cm = oracle.load_urdf(urdf(name), pose_xyz=(0.0, 0.0, 1.0))
    rng = np.random.default_rng(CL_SEED)
    lo, hi = np.array(cm.model.lower[:cm.n]), np.array(cm.model.upper[:cm.n])
    post = rng.uniform(0.5 * lo, 0.5 * hi, (CL_WORLDS, cm.n))
    tgt = post + rng.uniform(-0.2, 0.2, (CL_WORLDS, cm.n)) * hi
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    return cm, f32(post), f32(tgt)


def closed_loop_reference(oracle, cm, post, tgt, steps, eps=0.0, seed=0):
    """q [steps + 1, n] of one world under the oracle's pid_update loop;
    eps: the relative perturbation of posture and target."""
    r = np.random.default_rng(seed)
    jig = (lambda a: a * (1.0 + eps * r.uniform(-1, 1, np.shape(a)))) if eps else (lambda a: a)
    p, i, d, lim, ilim = CL_PID
    n = cm.n
    gains = oracle.pid_gains(p, i, d, imax=ilim, imin=-ilim, cmdmax=lim, cmdmin=-lim)
    st = [oracle.OrPidState() for _ in range(n)]
    ow = oracle.FloatWorld(cm, ground=False, pgs_iters=oracle.PGS_CONVERGED)
    post, tgt = jig(post), jig(tgt)
    ow.set_joints(post, np.zeros(n))
    mode = np.full(n, oracle.FORCE, np.int32)
    out = [ow.q]
    for _ in range(steps):
        q = ow.q
        tau = np.array([oracle.pid_update(gains, st[j], q[j] - tgt[j], 1e-3) for j in range(n)])
        ow.step(mode, tau)
        out.append(ow.q)
    return np.array(out), ow


# -- per-world parameters, wrenches and the warm-started landing (test_gpu_big_tree.py)
PAYLOAD_MAX = 5.0                                 # kg on the base (test_gpu_float_inertia_oracle.py's iCub case)
JOINT_DOFS = (5, 30, 32, 33, 38, 41, 44, 47)      # per-world damping / friction / effort: one more LCP row each
_SURVEYS = {}


def leaves(name):
    pa = parents(name)
    return [i for i in range(len(pa)) if i not in pa]


def survey_contacts(oracle, name, high=False):
    """bool [W]: the worlds in contact (high: on a body >= 32) in the converged oracle"""
    if name not in _SURVEYS:
        _SURVEYS[name] = survey(oracle, name)
    return _SURVEYS[name]["high"] if high else _SURVEYS[name]["n_contacts"] > 0


def friction_signal(oracle, name, mus):
    """Worlds whose converged oracle step with their own coefficient differs
    from the step at MU by more than SENSITIVE_BY."""
    cm = oracle.load_urdf(urdf(name))
    q, qd, pose, vel, tau = states(name)
    n = 0
    for w in range(W):
        if mus[w] != MU:
            a = oracle_step(oracle, cm, pose[w], vel[w], q[w], qd[w], tau[w], mus[w], oracle.PGS_CONVERGED)
            b = oracle_step(oracle, cm, pose[w], vel[w], q[w], qd[w], tau[w], MU, oracle.PGS_CONVERGED)
            n += float(np.abs(a.qd - b.qd).max()) > SENSITIVE_BY
    return n


def joint_words(nominal, name, dofs):
    """[W, n, 3] float32 damping / friction / effort words: float_joints_ref's
    draw on `dofs`; on the unlimited tree friction alone, U(0.5, 2) N m."""
    from float_joints_ref import per_world_words
    if split(name)[1] != "u":
        return per_world_words(nominal, W, list(dofs))
    words = np.tile(nominal, (W, 1, 1))
    words[:, list(dofs), 1] = np.random.default_rng(63).uniform(0.5, 2.0, (W, len(dofs)))
    return words.astype(np.float32)


def wrenches():
    """{link: [W, 6]} world wrenches (force, torque), float32 values: the base
    (U(-60, 60) N, U(-5, 5) N m), link 32 (body 33) and the last link
    (U(-20, 20) N, U(-2, 2) N m)."""
    rng = np.random.default_rng(12)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    out = {-1: f32(np.column_stack([rng.uniform(-60, 60, (W, 3)), rng.uniform(-5, 5, (W, 3))]))}
    for link in (32, 47):
        out[link] = f32(np.column_stack([rng.uniform(-20, 20, (W, 3)), rng.uniform(-2, 2, (W, 3))]))
    return out


WARM_STEPS, WARM_PD, WARM_DROP = 80, (60.0, 1.5), 0.005


def touch_height(oracle, cm, q):
    """The base height (level, to the millimetre from above) at which the
    model in posture q first touches the ground."""
    idle = np.full(cm.n, oracle.FORCE, np.int32), np.zeros(cm.n)

    def touches(mm):
        ow = oracle.FloatWorld(cm, pgs_iters=1)
        ow.set_pose([0, 0, 1e-3 * mm], np.eye(3))
        ow.set_joints(q, np.zeros(cm.n))
        return ow.step(*idle) > 0

    coarse = next(mm for mm in range(1500, 0, -25) if touches(mm))
    return 1e-3 * next(mm for mm in range(coarse + 25, 0, -1) if touches(mm))


def warm_inputs(oracle, name="tree48f", n_worlds=4):
    """(cm, posture [n_worlds, n], base height [n_worlds]): the closed loop's
    postures, the base WARM_DROP above touch_height."""
    cm = oracle.load_urdf(urdf(name))
    _, post, _ = closed_loop_inputs(oracle, name)
    post = post[:n_worlds]
    z = np.array([touch_height(oracle, cm, post[w]) + WARM_DROP for w in range(n_worlds)])
    return cm, post, z.astype(np.float32).astype(np.float64)


# -- the env (test_gpu_float_env_big.py): tree48 at rest in its zero posture, the lowest sphere 2 mm in the ground
ENV_PID = [60.0, 0.0, 1.5, -50.0, 50.0, 0.0, 0.0, -1.0]


def env_home(oracle, name="tree48"):
    """(home_base, contact links: the seven leaves and the base, 8 = the env's most)"""
    cm = oracle.load_urdf(urdf(name))
    z = touch_height(oracle, cm, np.zeros(cm.n)) - 0.002
    return (0.0, 0.0, float(np.float32(z)), 1.0, 0.0, 0.0, 0.0), leaves(name) + [-1]
