"""The arithmetic of the floating-base env's locomotion task
(gym-ignition_amd/csrc/float_task.hpp: projected gravity, the reward with its
tracking / smoothness / air-time terms, the command schedule, the air-time
counter) compiled for the host (g++, float32, test-only harness
tests/host_float_loco/harness.cpp) against numpy fp64 on 1,000 random states
-- the code the env kernels run per world, checked without a GPU.

Projected gravity within 2e-6 (products of unit-quaternion components).  The
reward within 2^-23 (n + 8) sum_i |term_i|: the terms are sums of at most
n + 8 float32 roundings, and expf's error is relative to a value of at most
the term's weight.  The command index, its Philox block and the zero test are
integers or an exact float32 comparison and must agree exactly, as must the
air-time counter and the steps a touchdown pays for, over a random 200-step
contact sequence per link.  Forces and command speeds are drawn at least 1e-5
away from contact_force_min and cmd_min."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "gym-ignition_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "host_float_loco", "harness.cpp")
COUNT, NDOF, LINKS, STEPS = 1000, 8, 4, 200
MARGIN = 1e-5
# cmd_lo[3], cmd_hi[3], cmd_zero_prob, cmd_min, w_track_lin, w_track_yaw, track_sigma, w_lin_z, w_ang_xy,
# w_action_rate, w_air_time, air_time_target, contact_force_min, env_dt, alive_bonus, w_forward, w_action, w_pose
PAR = np.array([-1.0, -0.5, -1.5, 1.5, 0.5, 1.5, 0.25, 0.2, 1.0, 0.5, 0.25, 2.0, 0.05, 0.01, 1.5, 0.3, 1.0, 0.02,
                1.0, 0.5, 0.01, 0.1], dtype=np.float32)
(ZERO_PROB, CMD_MIN, W_LIN, W_YAW, SIGMA, W_Z, W_XY, W_RATE, W_AIR, AIR_TARGET, F_MIN, ENV_DT, ALIVE, W_FORWARD,
 W_ACTION, W_POSE) = (float(x) for x in PAR[6:])


@pytest.fixture(scope="module")
def fl(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fl") / "libfl.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, HARNESS, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.fl_cmd_block.restype = ctypes.c_uint
    L.fl_cmd_index.restype = ctypes.c_uint
    L.fl_cmd_block.argtypes = [ctypes.c_uint]
    L.fl_cmd_index.argtypes = [ctypes.c_uint, ctypes.c_uint]
    L.fl_commands.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4
    L.fl_eval.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 11
    L.fl_air.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 5
    return L


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def _away(rng, draw, threshold_distance):
    """Redraw the entries of draw() that threshold_distance() puts closer than MARGIN."""
    x = draw(None)
    for _ in range(100):
        close = threshold_distance(x) < MARGIN
        if not close.any():
            return x
        x[close] = draw(int(close.sum()))
    raise AssertionError("could not draw away from the threshold")


def test_gravity_and_reward_match_fp64(fl):
    rng = np.random.default_rng(21)
    quat = rng.normal(size=(COUNT, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    base = np.concatenate([rng.uniform(-2, 2, (COUNT, 2)), rng.uniform(0, 1, (COUNT, 1)), quat,
                           rng.uniform(-3, 3, (COUNT, 6))], axis=1).astype(np.float32)
    q = rng.uniform(-3, 3, (COUNT, NDOF)).astype(np.float32)
    a = rng.uniform(-2, 2, (COUNT, NDOF)).astype(np.float32)
    a_prev = rng.uniform(-2, 2, (COUNT, NDOF)).astype(np.float32)
    a_prev[::5] = 0.0                                         # an episode's first step
    home = rng.uniform(-1, 1, NDOF).astype(np.float32)
    term = (rng.uniform(size=COUNT) < 0.2).astype(np.uint8)

    def draw_cmd(k):
        c = rng.uniform(-1.5, 1.5, (COUNT if k is None else k, 3)).astype(np.float32)
        c[rng.uniform(size=len(c)) < 0.3, :2] *= np.float32(0.1)   # both sides of cmd_min
        return c
    cmd = _away(rng, draw_cmd, lambda c: np.abs(np.hypot(c[:, 0].astype(np.float64), c[:, 1]) - CMD_MIN))
    cmd[::7] = 0.0                                            # the zero command
    # touchdown payments of up to LINKS links: (steps flown) env_dt - target each
    flown = rng.integers(0, 40, (COUNT, LINKS)) * (rng.uniform(size=(COUNT, LINKS)) < 0.3)
    pay64 = np.where(flown > 0, flown * ENV_DT - AIR_TARGET, 0.0).sum(axis=1)
    pay = pay64.astype(np.float32)
    gravity = np.zeros((COUNT, 3), np.float32)
    reward = np.zeros(COUNT, np.float32)
    assert fl.fl_eval(COUNT, NDOF, _p(PAR), _p(base), _p(q), _p(a), _p(a_prev), _p(home), _p(cmd), _p(pay),
                      _p(term), _p(gravity), _p(reward)) == 0

    b = base.astype(np.float64)
    w, x, y, z = b[:, 3], b[:, 4], b[:, 5], b[:, 6]
    ref_g = -np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)
    vx_world = ((1 - 2 * (y * y + z * z)) * b[:, 10] + 2 * (x * y - w * z) * b[:, 11] + 2 * (x * z + w * y) * b[:, 12])
    c64, a64, p64 = cmd.astype(np.float64), a.astype(np.float64), a_prev.astype(np.float64)
    v, om = b[:, 10:13], b[:, 7:10]
    fast = c64[:, 0] ** 2 + c64[:, 1] ** 2 > CMD_MIN ** 2
    terms = np.stack([
        np.where(term != 0, 0.0, ALIVE),
        W_FORWARD * vx_world,
        -W_ACTION * (a64 ** 2).sum(axis=1),
        -W_POSE * ((q.astype(np.float64) - home.astype(np.float64)) ** 2).sum(axis=1),
        W_LIN * np.exp(-((c64[:, 0] - v[:, 0]) ** 2 + (c64[:, 1] - v[:, 1]) ** 2) / SIGMA),
        W_YAW * np.exp(-((c64[:, 2] - om[:, 2]) ** 2) / SIGMA),
        -W_Z * v[:, 2] ** 2,
        -W_XY * (om[:, 0] ** 2 + om[:, 1] ** 2),
        -W_RATE * ((a64 - p64) ** 2).sum(axis=1),
        np.where(fast, W_AIR * pay.astype(np.float64), 0.0)], axis=1)
    ref_r = terms.sum(axis=1)
    bound = 2.0 ** -23 * (NDOF + 8) * np.abs(terms).sum(axis=1)
    err_g = float(np.abs(gravity - ref_g).max())
    ratio = float((np.abs(reward - ref_r) / bound).max())
    print(f"float_task.hpp locomotion vs fp64, {COUNT} states: gravity {err_g:.2e}, reward error / bound {ratio:.3f}; "
          f"{int(fast.sum())} fast commands, {int((pay != 0).sum())} states with a payment")
    assert 0.2 * COUNT < fast.sum() < 0.9 * COUNT and (pay != 0).sum() > 0.3 * COUNT
    assert err_g <= 2e-6
    assert ratio <= 1.0


def test_command_schedule_is_exact(fl):
    rng = np.random.default_rng(22)
    for interval in (0, 1, 5, 7, 1000):
        for t in list(range(0, 40)) + [999, 1000, 1001, 2 ** 31 + 3]:
            k = t // interval if interval else 0
            assert fl.fl_cmd_index(t, interval) == k
    for k in (0, 1, 5, 2 ** 30 - 1):
        assert fl.fl_cmd_block(k) == (0xC0000000 | k)
    # no block of the reset draw (< 12), the episode block or a push block
    assert fl.fl_cmd_block(0) not in (0x40000000, 0x80000000) and fl.fl_cmd_block(0) >> 30 == 3
    words = rng.integers(0, 2 ** 32, (COUNT, 4), dtype=np.uint64).astype(np.uint32)
    # draws on both sides of the zero test, including its edge: u < p with p = 0.25 exactly
    words[0, 3] = np.uint32(0x40000000)          # u = 0.25: not below
    words[1, 3] = np.uint32(0x3FFFFF00)          # the float below 0.25
    words[2, 3] = np.uint32(0x400000FF)          # still 0.25 after the shift
    cmd = np.zeros((COUNT, 3), np.float32)
    zero = np.zeros(COUNT, np.uint8)
    fl.fl_commands(COUNT, _p(PAR), _p(words), _p(cmd), _p(zero))
    u = (words[:, 3] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    ref_zero = u < ZERO_PROB
    np.testing.assert_array_equal(zero.astype(bool), ref_zero)
    assert list(zero[:3]) == [0, 1, 0] and 0.15 * COUNT < ref_zero.sum() < 0.35 * COUNT
    np.testing.assert_array_equal(cmd[ref_zero], 0.0)
    lo, hi = PAR[:3].astype(np.float64), PAR[3:6].astype(np.float64)
    ref = lo + (hi - lo) * ((words[:, :3] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24)
    err = np.abs(cmd[~ref_zero] - ref[~ref_zero]) / (hi - lo)
    assert float(err.max()) <= 4 * 2.0 ** -23


def test_air_time_counter_is_exact(fl):
    rng = np.random.default_rng(23)
    touchdowns = 0
    for link in range(LINKS * 8):
        # contact episodes of random length; forces at least MARGIN away from the threshold
        on = np.repeat(rng.uniform(size=STEPS) < 0.5, rng.integers(1, 9, STEPS))[:STEPS]
        fz = _away(rng, lambda k: rng.uniform(0.0, 2.0 * F_MIN, STEPS if k is None else k).astype(np.float32),
                   lambda f: np.abs(f.astype(np.float64) - F_MIN))
        fz = np.where(on, np.maximum(fz, np.float32(F_MIN + 0.5)), np.minimum(fz, np.float32(F_MIN - 0.5)))
        fz = fz.astype(np.float32)
        if link == 0:
            fz[:] = F_MIN                         # exactly at the threshold: not in contact
        counter = np.zeros(STEPS, np.uint32)
        flown = np.zeros(STEPS, np.uint32)
        pay = np.zeros(STEPS, np.float32)
        fl.fl_air(STEPS, _p(PAR), _p(fz), _p(counter), _p(flown), _p(pay))
        air, ref_counter, ref_flown = 0, [], []
        for t in range(STEPS):
            if float(fz[t]) > F_MIN:
                ref_flown.append(air)
                air = 0
            else:
                ref_flown.append(0)
                air += 1
            ref_counter.append(air)
        np.testing.assert_array_equal(counter, ref_counter)
        np.testing.assert_array_equal(flown, ref_flown)
        ref_pay = np.where(np.array(ref_flown) > 0, np.array(ref_flown) * ENV_DT - AIR_TARGET, 0.0)
        # one product and one difference in float32
        assert float(np.abs(pay - ref_pay).max()) <= 2.0 ** -23 * (max(ref_flown) * ENV_DT + AIR_TARGET)
        np.testing.assert_array_equal(pay[np.array(ref_flown) == 0], 0.0)
        touchdowns += int((np.array(ref_flown) > 0).sum())
    assert touchdowns >= 10 * LINKS
