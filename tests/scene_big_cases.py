"""Scenes at the edges of the scene kernel's large-contact path (scene_kernel.hip
sc_step: use_big = the scene has a workspace and nc_all > 32 points or
3 nc_all + tj > 64 rows), shared by tests/test_scene_big_cases.py (fp64 oracle
alone, CPU) and tests/test_gpu_scene_big_edges.py (the kernel against it).

A builder takes an rng and returns a Case: the models, and per world the base
poses, velocities, joint states and presence, rounded to float32 so that the
kernel starts from the same numbers.  A Case answers base_pose / base_velocity
/ get like a Scene, so test_gpu_scene._oracle_from_gpu builds the oracle world
(and its perturbed twins) from it directly.

Geometry: 0.2 m cubes in a row along x, axis-aligned (with near-parallel faces
the box-box SAT's reference face is a near-tie that fp32 and fp64 may break
differently), every penetration between 1e-4 and 3e-4 m and every gap 1e-4 m
or more, so both precisions detect the same points (lcp_validity.GRAZE is
1e-6 m).  A row of n touching cubes has 4 n ground corners and 4 (n - 1) face
points.
"""

import numpy as np

from scene_models import cube_urdf
from test_float_tree_oracle import chain_urdf

MU = 0.8
EDGE = 0.2
LIMB_LIMIT = 1.0
LIMB_XYZ = (0.0, 1.0, 1.2)   # the welded chain hangs in the air, 0.8 m beside the row


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def limb_urdf(n=6, friction_last=0.0):
    """A serial chain of n limited revolute joints (+-LIMB_LIMIT rad, axes
    alternating y / x) welded to the world at LIMB_XYZ; no collision shapes.
    friction_last: Coulomb friction of the last joint (one more joint row
    whenever that joint moves)."""
    x, y, z = LIMB_XYZ
    parts = [f'<robot name="limb"><link name="world"/><joint name="weld" type="fixed"><parent link="world"/>'
             f'<child link="base"/><origin xyz="{x} {y} {z}"/></joint><link name="base"><inertial><mass value="2"/>'
             f'<inertia ixx="0.02" iyy="0.02" izz="0.02" ixy="0" ixz="0" iyz="0"/></inertial></link>']
    parent = "base"
    for i in range(n):
        axis = "0 1 0" if i % 2 == 0 else "1 0 0"
        fr = friction_last if i == n - 1 else 0.0
        parts.append(f'<joint name="j{i}" type="revolute"><parent link="{parent}"/><child link="l{i}"/>'
                     f'<origin xyz="0.02 0 -0.12"/><axis xyz="{axis}"/>'
                     f'<limit lower="{-LIMB_LIMIT}" upper="{LIMB_LIMIT}" effort="50" velocity="30"/>'
                     f'<dynamics damping="0" friction="{fr}"/></joint>'
                     f'<link name="l{i}"><inertial><origin xyz="0 0.01 -0.06"/><mass value="{0.6 - 0.05 * i}"/>'
                     f'<inertia ixx="0.003" iyy="0.0035" izz="0.001" ixy="0.0001" ixz="0" iyz="0"/></inertial></link>')
        parent = f"l{i}"
    return "".join(parts) + "</robot>"


class Case:
    """models: (urdf text, insertion xyz, name); the per-world start state in
    pose [m] (W, 7: xyz, wxyz), vel [m] (W, 6: world linear, angular), q / qd
    [m] (W, dofs) -- None where the model has no such state -- and present
    (W, models)."""

    def __init__(self, name, models, W):
        self.name, self.W = name, W
        self.texts = [t for t, _, _ in models]
        self.base = [tuple(b) for _, b, _ in models]
        self.names = [n for _, _, n in models]
        K = len(models)
        self.pose, self.vel, self.q, self.qd = [None] * K, [None] * K, [None] * K, [None] * K
        self.present = np.ones((W, K), bool)
        self.expect = {}     # world -> (points, rows) of the first step
        self.mu = np.full(W, MU)   # friction coefficient of every world (all its contacts)

    # ---- the start state with a Scene's getters (_oracle_from_gpu)
    def base_pose(self, m, w, nw):
        return self.pose[m][w:w + nw]

    def base_velocity(self, m, w, nw):
        return self.vel[m][w:w + nw]

    def get(self, f, m, w, nw):
        return (self.q if f == "q" else self.qd)[m][w:w + nw]

    def models_of(self, w):
        """indices of the models present in world w (an absent model is always
        the last one, so the indices of the others do not move)"""
        ms = [m for m in range(len(self.texts)) if self.present[w, m]]
        assert ms == list(range(len(ms)))
        return ms

    def compile(self, oracle):
        return [oracle.load_urdf(t, pose_xyz=b) for t, b in zip(self.texts, self.base)]


def path(nc, rows):
    """the path sc_step takes for nc points and `rows` rows in all: True = large"""
    return nc > 32 or rows > 64


def _cube_models(n, extra=()):
    return [(cube_urdf(), (EDGE * k, 0.0, EDGE / 2), f"c{k}") for k in range(n)] + list(extra)


def _speeds(W):
    """The velocity scale of every world.  The points of these rows are
    redundant (four corners under a cube, four points on a face), so the
    normal impulses are fixed by DART's CFM alone and the friction boxes follow
    them: where a contact slides, the velocities after the step move by 1e-3
    under an fp32-size (1e-6) perturbation of the Delassus matrix; where
    everything sticks (|v| below mu g dt = 7.8e-3 m/s) they do not move.  One
    world in eight slides (the cap on worlds accepted as other solutions of the
    LCP), the others stick."""
    return np.where(np.arange(W) % 8 == 7, 0.05, 0.005)


def _row(case, n, rng, apart=()):
    """cubes 0 .. n-1 of `case` in a row: the faces of k - 1 and k overlapping
    by 1e-4 .. 3e-4 (k in `apart`: 5e-4 .. 7e-4 clear of each other), corners
    1e-4 .. 3e-4 below the ground, random velocities of scale _speeds (linear;
    ten times that angular); returns the tops' heights (W, n)"""
    W = case.W
    vel = _speeds(W)[:, None]
    x = np.zeros(W)
    tops = np.zeros((W, n))
    for k in range(n):
        if k:
            x = x + EDGE + (rng.uniform(5e-4, 7e-4, W) if k in apart else -rng.uniform(1e-4, 3e-4, W))
        z = EDGE / 2 - rng.uniform(1e-4, 3e-4, W)
        pose = np.column_stack([x, rng.uniform(-1e-3, 1e-3, W), z, np.ones(W), np.zeros((W, 3))])
        case.pose[k] = f32(pose)
        case.vel[k] = f32(np.column_stack([vel * rng.uniform(-1, 1, (W, 3)), 10 * vel * rng.uniform(-1, 1, (W, 3))]))
        tops[:, k] = case.pose[k][:, 2] + EDGE / 2
    return tops


def rows_only(rng, W=16):
    """a. four cubes in a row: 16 + 12 = 28 points, 84 rows, nv 24 (MAXNV 32):
    the large path by its row count alone"""
    c = Case("a rows-only, MAXNV 32", _cube_models(4), W)
    _row(c, 4, rng)
    c.expect = {w: (28, 84) for w in range(W)}
    return c


def points_32(rng, W=16):
    """b. five cubes in a row: 20 + 16 = 36 points, 108 rows, nv 30 (MAXNV 32)"""
    c = Case("b points, MAXNV 32", _cube_models(5), W)
    _row(c, 5, rng)
    c.expect = {w: (36, 108) for w in range(W)}
    return c


def boundary_64(rng, K, friction=False, W=8):
    """c. three cubes in a row (20 points, 60 rows) and the welded six-joint
    limb with K joints 1e-3 rad beyond a limit (K limit rows; with `friction`
    the last joint's Coulomb row as well): 64 rows stay compact, 65 go large;
    nv 24 (MAXNV 32).  The state does not depend on K beyond those joints."""
    n = 6
    limb = (limb_urdf(n, 0.2 if friction else 0.0), (0.0, 0.0, 0.0), "limb")
    c = Case(f"c boundary K={K}{' +friction' if friction else ''}", _cube_models(3, [limb]), W)
    _row(c, 3, rng)
    q = rng.uniform(-0.6, 0.6, (W, n))
    side = np.where(rng.uniform(size=(W, n)) < 0.5, -1.0, 1.0)
    q[:, :K] = (side * (LIMB_LIMIT + 1e-3))[:, :K]
    c.q[3], c.qd[3] = f32(q), f32(rng.uniform(-0.5, 0.5, (W, n)))
    rows = 60 + K + (1 if friction else 0)
    c.expect = {w: (20, rows) for w in range(W)}
    return c


def deep_joint_rows(rng, W=16):
    """d. five cubes in a row and the floating three-link chain
    (test_float_tree_oracle.chain_urdf) with its base box lying across cubes 3
    and 4, its first joint 1e-3 rad beyond the upper limit and the links
    folded up into the air.  Cubes 3 and 4 stand clear of their neighbours:
    overlapping faces push two cubes apart, and a box lying on both then has
    to slide on one of them, which makes every such world ill-conditioned.
    20 ground + 8 face + 8 box = 36 points, 108 + 1 rows, nv 39 (MAXNV 64)"""
    chain = (chain_urdf(3), (0.0, 0.0, 0.5), "chain")
    c = Case("d joint rows deep in the large path", _cube_models(5, [chain]), W)
    tops = _row(c, 5, rng, apart=(3, 4))
    xb = 0.5 * (c.pose[3][:, 0] + c.pose[4][:, 0]) + rng.uniform(-0.01, 0.01, W)
    zb = np.minimum(tops[:, 3], tops[:, 4]) - rng.uniform(1e-4, 2e-4, W) + 0.05
    c.pose[5] = f32(np.column_stack([xb, rng.uniform(-0.02, 0.02, W), zb, np.ones(W), np.zeros((W, 3))]))
    vel = _speeds(W)[:, None]
    c.vel[5] = f32(np.column_stack([vel * rng.uniform(-1, 1, (W, 3)), 10 * vel * rng.uniform(-1, 1, (W, 3))]))
    q = np.column_stack([np.full(W, 2.0 + 1e-3), rng.uniform(-0.3, 0.3, (W, 2))])
    c.q[5], c.qd[5] = f32(q), f32(10 * vel * rng.uniform(-1, 1, (W, 3)))
    c.expect = {w: (36, 109) for w in range(W)}
    return c


def mixed_batch(rng, W=12):
    """e. the models of (b); worlds w % 3 == 0 without the fifth cube (28
    points, 84 rows: large by rows), w % 3 == 1 with the cubes 0.3 m apart (20
    ground points, 60 rows: compact), the rest as (b) (36 points: large)"""
    c = Case("e mixed batch", _cube_models(5), W)
    _row(c, 5, rng)
    spread = np.arange(W) % 3 == 1
    for k in range(5):
        c.pose[k][spread, 0] = f32(0.3 * k)
    c.present[np.arange(W) % 3 == 0, 4] = False
    c.expect = {w: ((28, 84), (20, 60), (36, 108))[w % 3] for w in range(W)}
    return c


def transitions(rng, W=4):
    """f. five cubes 1.5 mm above the ground (angular velocity 0; each yawed
    by 2 mrad against its neighbour, see below), cube k moving along x at
    0.3 (k - 2) m/s.  Even worlds: 5.8 mm apart and closing, without friction
    -- no contact, then ground corners only (compact), then the faces meet:
    36 points (large).  Odd worlds: friction 0.8 (the landing's friction
    impulse takes mu times the 0.17 m/s of the fall out of the motion; the
    rest carries on), faces overlapping by 5.8 mm and separating -- 16 face
    points carrying nothing (compact), the landing with the faces still
    overlapping: 36 points (large), then the faces part: 20 ground points
    (compact).  The closing worlds are frictionless because their faces meet
    while the cubes slide on the ground: with friction such an impact is
    ill-conditioned (the velocities move by 1e-3 .. 1e-2 under a 1e-6
    relative perturbation of the Delassus matrix, at mu = 0.02 still by
    1e-3), and with W = 4 no world may be accepted as another solution of the
    LCP."""
    c = Case("f path transitions", _cube_models(5), W)
    closing = np.arange(W) % 2 == 0
    c.mu = np.where(closing, 0.0, MU)
    step = np.where(closing, EDGE + 5.8e-3, EDGE - 5.8e-3) + rng.uniform(-2e-5, 2e-5, W)
    z = EDGE / 2 + 1.5e-3 + rng.uniform(0.0, 1e-4, W)
    for k in range(5):
        # Over many steps the cubes pick up rotations at the rounding level, and
        # between parallel cubes of one size the SAT's choice of the reference
        # face (A's or B's: the penetrations differ by T . (a_x - b_x)) then
        # hangs on them -- fp32 and fp64 may choose differently, an equally
        # valid manifold.  A yaw of 2 mrad and a sideways step of -2 mm per
        # cube make that difference 4e-6 m or more, the same for both.
        yaw = 2e-3 * k
        pose = np.column_stack([step * k, -2e-3 * k + rng.uniform(-1e-4, 1e-4, W), z + rng.uniform(0, 2e-5, W),
                                np.full(W, np.cos(yaw / 2)), np.zeros((W, 2)), np.full(W, np.sin(yaw / 2))])
        c.pose[k] = f32(pose)
        vx = np.where(closing, -0.3, 0.3) * (k - 2)
        c.vel[k] = f32(np.column_stack([vx, np.zeros((W, 5))]))
    return c


# ------------------------------------------------------------ oracle side
def oracle_world(oracle, cms, src, w, case, eps=0.0, seed=0):
    """the fp64 exact-mode world of world w from src's state (a Case or a
    Scene), holding the models present there"""
    from test_gpu_scene import _oracle_from_gpu
    return _oracle_from_gpu(oracle, [cms[m] for m in case.models_of(w)], src, w, -1, float(case.mu[w]), eps, seed)


def counts(oracle, ow):
    """(points, rows, problem) of the step the oracle world just took (a step
    without rows leaves lcp_last at an older problem; none of these cases has
    joint rows without contacts)"""
    nc = len(ow.contacts)
    p = oracle.lcp_last() if nc else None
    return nc, (len(p["b"]) if nc else 0), p


def cube_gaps(poses, Rs):
    """signed clearances of a row of cubes (positive: apart): every corner
    above the ground, and between neighbours k, k + 1 the least distance of a
    corner of k + 1 beyond the +x face of k (exact for the near-parallel faces
    of these cases)"""
    h = EDGE / 2
    corners = np.array([[sx, sy, sz] for sx in (-h, h) for sy in (-h, h) for sz in (-h, h)])
    ground, pair = [], []
    for k, (p, R) in enumerate(zip(poses, Rs)):
        cw = p + corners @ np.asarray(R).T
        ground.extend(cw[:, 2])
        if k:
            pa, Ra = poses[k - 1], np.asarray(Rs[k - 1])
            pair.append(float(((cw - pa) @ Ra)[:, 0].min() - h))
    return np.array(ground), np.array(pair)


# The cases of both test files, with their seeds (fixed so that at most W / 8
# worlds of a case are ill-conditioned: tests/test_scene_big_cases.py) and the
# path every world must take.
ONE_STEP = {
    "a": (lambda: rows_only(np.random.default_rng(101)), lambda w: True),
    "b": (lambda: points_32(np.random.default_rng(102)), lambda w: True),
    "c-K4": (lambda: boundary_64(np.random.default_rng(103), 4), lambda w: False),
    "c-K5": (lambda: boundary_64(np.random.default_rng(103), 5), lambda w: True),
    "c-K3-friction": (lambda: boundary_64(np.random.default_rng(103), 3, True), lambda w: False),
    "c-K4-friction": (lambda: boundary_64(np.random.default_rng(103), 4, True), lambda w: True),
    "d": (lambda: deep_joint_rows(np.random.default_rng(104)), lambda w: True),
    "e": (lambda: mixed_batch(np.random.default_rng(105)), lambda w: w % 3 != 1),
}
TRANSITIONS = lambda: transitions(np.random.default_rng(111))   # noqa: E731
TRANSITION_STEPS = 40
