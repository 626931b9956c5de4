"""fp64 restatement of the floating-base env's motion-clip tracking task
(mw_floatenv_tracking; gym-ignition_amd/csrc/float_task.hpp, ft_track_*): the
clip and start-frame draw from the oracle's Philox4x32-10, the integer frame
clock, the blended reference row, the five errors and terms, the words of the
observation -- and the bounds float32 is held to against it.  A plain module
like the other *_ref.py helpers: no tests, no fixtures; the CPU tests
(test_float_track_host.py) and the GPU tests (test_gpu_float_track*.py) use it.

Bounds, u = 2^-24 the unit roundoff of float32:
  lerp     p0 + a (p1 - p0) with a, the difference and the fused step rounded
           once each: u (2 |p1 - p0| + max(|p0|, |p1|)).
  nlerp    four such words of unit quaternions (at most 5 u each), divided by a
           norm of at least sqrt(1/2) that carries the same error and seven
           roundings of its own: 21 u < 2e-6, the project's bound for
           quaternion-derived words (QUAT_TOL).
  sums     m items of at most 3 roundings each and m roundings of the running
           sum: (m + 4) u times the sum, whose items are all >= 0.
  root_rot a dot product of unit quaternions (4 u), squared and subtracted from
           one: 9 u, absolute.
  terms    weight expf(-scale e): the product in the exponent (0.37 u at worst
           after expf), expf itself (2 u) and the last product (u): 4 u weight,
           plus weight scale times whatever error e carries.
  phase    three roundings on the way to 2 pi phi <= 2 pi and sinf / cosf (2 u):
           (3 * 2 pi + 2) u < 2e-6 (PHASE_TOL)."""

from fractions import Fraction

import numpy as np

TRACK_BLOCK = 0x40000400
TERMS = ("pose", "velocity", "root_pos", "root_rot", "root_vel")
U = 2.0 ** -24
QUAT_TOL = 2e-6
PHASE_TOL = 2e-6


def key(seed):
    return [seed & 0xFFFFFFFF, seed >> 32]


def u01(x):
    return float(int(x) >> 8) * 2.0 ** -24


def clip_of(r0, n_clips):
    return int(r0) % n_clips


def start_of(r1, r2, length, prob):
    return int(r1) % (length - 1) if u01(r2) < float(np.float32(prob)) else 0


def draw_ref(oracle, seed, g, episode, table, prob):
    """(clip, start frame) of (seed, global world g, episode); table: (first, length, loop) per clip."""
    r = oracle.philox_raw([g, episode, TRACK_BLOCK, 0], key(seed))
    c = clip_of(r[0], len(table))
    return c, start_of(r[1], r[2], table[c][1], prob)


def clock(f0, t, num, den, length, loop):
    """(i, i1, a, wraps, ended) with Python integers; a an exact Fraction."""
    x = f0 * den + t * num
    fi, rem = divmod(x, den)
    last = length - 1
    a, wraps, ended = Fraction(rem, den), 0, False
    if loop:
        wraps, fi = divmod(fi, last)
    elif fi + (1 if rem else 0) > last:
        ended, fi, a, rem = True, last, Fraction(0), 0
    return fi, fi + (1 if rem else 0), a, wraps, ended


def nlerp(q0, q1, a):
    q0, q1 = np.asarray(q0, np.float64), np.asarray(q1, np.float64)
    if float(q0 @ q1) < 0:
        q1 = -q1
    q = q0 + float(a) * (q1 - q0)
    return q / np.linalg.norm(q)


def reference_row(clips, entry, ck):
    """The reference row (13 + 2 n words, fp64) of a clip (first, length, loop) at the clock ck."""
    first, length, _ = entry
    i, i1, a, wraps, _ = ck
    p0, p1 = clips[first + i].astype(np.float64), clips[first + i1].astype(np.float64)
    row = p0 + float(a) * (p1 - p0)
    row[3:7] = nlerp(p0[3:7], p1[3:7], a)
    if wraps:
        row[:2] += wraps * (clips[first + length - 1, :2].astype(np.float64) - clips[first, :2].astype(np.float64))
    return row


def reference_tol(clips, entry, ck):
    """Per word, the bound of the device's float32 reference row against reference_row."""
    first, length, _ = entry
    i, i1, _, wraps, _ = ck
    p0, p1 = np.abs(clips[first + i].astype(np.float64)), np.abs(clips[first + i1].astype(np.float64))
    d = np.abs(clips[first + i1].astype(np.float64) - clips[first + i].astype(np.float64))
    tol = U * (2 * d + np.maximum(p0, p1))
    tol[3:7] = QUAT_TOL
    if wraps:
        disp = np.abs(clips[first + length - 1, :2].astype(np.float64) - clips[first, :2].astype(np.float64))
        tol[:2] += U * (2 * wraps * disp + p0[:2] + p1[:2])
    return tol


def errors(row, ref, wj, n, ang_scale):
    """The five errors in fp64 of a state row against a reference row."""
    row, ref, wj = np.asarray(row, np.float64), np.asarray(ref, np.float64), np.asarray(wj, np.float64)
    dq, dv = row[13:13 + n] - ref[13:13 + n], row[13 + n:13 + 2 * n] - ref[13 + n:13 + 2 * n]
    dot = float(row[3:7] @ ref[3:7])
    return np.array([float((wj * dq * dq).sum()), float((wj * dv * dv).sum()), float(((row[:3] - ref[:3]) ** 2).sum()),
                     1.0 - dot * dot,
                     float(((row[7:10] - ref[7:10]) ** 2).sum()) + float(ang_scale) * float(((row[10:13] - ref[10:13]) ** 2).sum())])


def errors_tol(e, n):
    """float32 against errors() on the same inputs."""
    e = np.abs(np.asarray(e, np.float64))
    return np.array([(n + 4) * U * e[0], (n + 4) * U * e[1], 7 * U * e[2], 9 * U, 8 * U * e[4]])


def errors_input_tol(row, ref, ref_tol, wj, n, ang_scale):
    """What an error of ref_tol per word of the reference adds to each error: d(x^2) <= 2 |x| t + t^2."""
    row, ref, t = np.asarray(row, np.float64), np.asarray(ref, np.float64), np.asarray(ref_tol, np.float64)
    wj = np.asarray(wj, np.float64)
    d = np.abs(row - ref)
    sq = 2 * d * t + t * t
    q = slice(13, 13 + n)
    v = slice(13 + n, 13 + 2 * n)
    return np.array([float((wj * sq[q]).sum()), float((wj * sq[v]).sum()), float(sq[:3].sum()),
                     2 * float(np.abs(row[3:7]).sum()) * QUAT_TOL,
                     float(sq[7:10].sum()) + float(ang_scale) * float(sq[10:13].sum())])


def terms(weights, scales, e):
    w, s = np.asarray(weights, np.float64), np.asarray(scales, np.float64)
    return np.where(w != 0, w * np.exp(-s * np.asarray(e, np.float64)), 0.0)


def terms_tol(weights, scales, e_tol):
    w, s = np.asarray(weights, np.float64), np.asarray(scales, np.float64)
    return w * (4 * U + s * np.asarray(e_tol, np.float64))


def phase_words(i, a, length):
    phi = (np.asarray(i, np.float64) + np.asarray(a, np.float64)) / (length - 1)
    return np.sin(2 * np.pi * phi), np.cos(2 * np.pi * phi)
