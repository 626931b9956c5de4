"""fp64 restatement of the floating-base env's initial-state draw
(mw_floatenv_init_state; gym-ignition_amd/csrc/float_task.hpp, ft_init_*) from
the oracle's Philox4x32-10: the row choice, the offsets, the composed
quaternion and the velocities.  A plain module like the other *_ref.py helpers:
no tests, no fixtures; the CPU tests (test_float_init_host.py) and the GPU tests
(test_gpu_float_init*.py) both use it."""

import numpy as np

ROW_BLOCK, POS_BLOCK, RPY_BLOCK, LIN_BLOCK, ANG_BLOCK, QD_BLOCK = (0x40000300, 0x40000301, 0x40000302, 0x40000303,
                                                                   0x40000304, 0x40000340)
POS, RPY, LIN, ANG = 1, 2, 4, 8            # InitGroup bits
BASE_DRAWS = 13                            # dpos, rpy, dlin, dang, the bank row; then n joint-velocity draws
QUAT_FACTOR_TOL = 2e-6                     # per composed factor of the orientation (the project's quaternion bound)
NORM_TOL = 4 * 2.0 ** -23
ZERO3 = ((0.0, 0.0),) * 3


def key(seed):
    return [seed & 0xFFFFFFFF, seed >> 32]


def u01(x):
    """(x >> 8) 2^-24, exact in float32 and fp64."""
    return float(int(x) >> 8) * 2.0 ** -24


def unif(x, lo, hi):
    """lo + (hi - lo) (x >> 8) 2^-24 in fp64 on the float32 bounds the env holds."""
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    return lo + (hi - lo) * u01(x)


def draw_tol(lo, hi):
    """The bound of a float32 uniform draw against unif(): the one _check_draws uses."""
    return 4 * 2.0 ** -23 * (float(hi) - float(lo))


def row_of(r_a, r_b, n_states, prob):
    """The bank row of an episode from words 0 and 1 of its row block; -1 the home row."""
    if n_states <= 0 or not u01(r_b) < float(np.float32(prob)):
        return -1
    return int(r_a) % n_states


def row_ref(oracle, seed, g, episode, n_states, prob):
    if n_states <= 0:
        return -1
    r = oracle.philox_raw([g, episode, ROW_BLOCK, 0], key(seed))
    return row_of(r[0], r[1], n_states, prob)


def draws_ref(oracle, seed, g, episode, n, pos=None, rpy=None, lin=None, ang=None, joint_vel=0.0, n_states=0,
              prob=1.0):
    """The 13 + n words of env.init_draws of (seed, global world g, episode) in
    fp64; a group that is off (None) draws nothing and reports zeros."""
    out = np.zeros(BASE_DRAWS + n)
    for k, (block, ranges) in enumerate(((POS_BLOCK, pos), (RPY_BLOCK, rpy), (LIN_BLOCK, lin), (ANG_BLOCK, ang))):
        if ranges is not None:
            r = oracle.philox_raw([g, episode, block, 0], key(seed))
            out[3 * k:3 * k + 3] = [unif(r[e], *ranges[e]) for e in range(3)]
    out[12] = row_ref(oracle, seed, g, episode, n_states, prob)
    if joint_vel > 0:
        for b in range((n + 3) // 4):
            r = oracle.philox_raw([g, episode, QD_BLOCK | b, 0], key(seed))
            for e in range(4):
                if 4 * b + e < n:
                    out[BASE_DRAWS + 4 * b + e] = unif(r[e], -joint_vel, joint_vel)
    return out


def draw_tols(n, pos=None, rpy=None, lin=None, ang=None, joint_vel=0.0):
    """Per word of init_draws, the bound against draws_ref (the row word is exact)."""
    out = np.zeros(BASE_DRAWS + n)
    for k, ranges in enumerate((pos, rpy, lin, ang)):
        if ranges is not None:
            out[3 * k:3 * k + 3] = [draw_tol(*ranges[e]) for e in range(3)]
    out[BASE_DRAWS:] = draw_tol(-joint_vel, joint_vel)
    return out


def quat_mul(a, b):
    """Hamilton product, wxyz."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def orientation_ref(rpy, q_row):
    """qz(yaw) qy(pitch) qx(roll) q_row, normalised, fp64."""
    roll, pitch, yaw = (float(a) for a in rpy)
    qx = np.array([np.cos(roll / 2), np.sin(roll / 2), 0.0, 0.0])
    qy = np.array([np.cos(pitch / 2), 0.0, np.sin(pitch / 2), 0.0])
    qz = np.array([np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)])
    q = quat_mul(qz, quat_mul(qy, quat_mul(qx, np.asarray(q_row, np.float64))))
    return q / np.linalg.norm(q)


def quat_tol(rpy, q_row):
    """QUAT_FACTOR_TOL per composed factor: each nonzero angle, and a row that is not the identity."""
    factors = sum(1 for a in rpy if a != 0) + (0 if tuple(np.asarray(q_row).tolist()) == (1.0, 0.0, 0.0, 0.0) else 1)
    return QUAT_FACTOR_TOL * max(1, factors)


def rotation(q):
    """Body -> world rotation of the unit quaternion q (wxyz), fp64."""
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def home_row(home_base, home_q):
    """The base row of an env without a bank: home_base, zeros, home_q, zeros."""
    n = len(home_q)
    row = np.zeros(13 + 2 * n, np.float32)
    row[:7] = home_base
    row[13:13 + n] = home_q
    return row


def base_words32(row, draws, groups):
    """Position and velocity words of the start state from a float32 base row
    and the reported float32 draws: one float32 sum each, bit for bit; a group
    that is off keeps the row's words."""
    row, draws = np.asarray(row, np.float32), np.asarray(draws, np.float32)
    out = row[:13].copy()
    if groups & POS:
        out[0:3] = row[0:3] + draws[0:3]
    if groups & LIN:
        out[7:10] = row[7:10] + draws[6:9]
    if groups & ANG:
        out[10:13] = row[10:13] + draws[9:12]
    return out
