"""The task arithmetic of the floating-base env (gym-ignition_amd/csrc/
float_task.hpp: world velocity from the stored body twist, tilt, reward,
termination predicate) compiled for the host (g++, float32, test-only harness
tests/host_float_task/harness.cpp) against numpy fp64 on 1,000 random states
-- the code the post kernel runs per world, checked without a GPU.

Tolerance 2e-6 max(1, |reference|) (about 16 float32 ulps: the quantities are
sums of at most 3 + 2 n products with no cancellation beyond a 3x3 rotation).
Termination must agree exactly; every state is drawn at least 1e-5 away from
the height and tilt thresholds."""

import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "gym-ignition_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "host_float_task", "harness.cpp")
COUNT, NDOF = 1000, 8
Z_MIN, COS_TILT = 0.3, math.cos(1.0)
ALIVE, W_FORWARD, W_ACTION, W_POSE = 1.0, 1.0, 0.01, 0.1
MARGIN = 1e-5


@pytest.fixture(scope="module")
def ft(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ft") / "libft.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, HARNESS, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.ft_eval.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 10
    return L


def _rotation(q):
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)


def _bounded(rng, count, bound):
    """Vectors of norm <= bound, uniform in direction."""
    v = rng.normal(size=(count, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0, bound, (count, 1))


def _states(rng, count):
    quat = rng.normal(size=(count, 4))
    # half of the states nearly upright, so that both outcomes of the tilt test occur often
    quat[::2, 1:3] *= 0.2
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    base = np.concatenate([rng.uniform(-2, 2, (count, 2)), rng.uniform(0.0, 1.0, (count, 1)), quat,
                           _bounded(rng, count, 10.0), _bounded(rng, count, 10.0)], axis=1).astype(np.float32)
    return base


def _draw(rng):
    """COUNT states, each at least MARGIN away from both thresholds (in fp64 of the fp32 inputs)."""
    base = _states(rng, COUNT)
    for _ in range(100):
        b = base.astype(np.float64)
        rzz = 1 - 2 * (b[:, 4] ** 2 + b[:, 5] ** 2)
        close = (np.abs(b[:, 2] - Z_MIN) < MARGIN) | (np.abs(rzz - COS_TILT) < MARGIN)
        if not close.any():
            break
        base[close] = _states(rng, int(close.sum()))
    return base


def test_task_arithmetic_matches_fp64(ft):
    rng = np.random.default_rng(11)
    base = _draw(rng)
    q = rng.uniform(-3, 3, (COUNT, NDOF)).astype(np.float32)
    a = rng.uniform(-5, 5, (COUNT, NDOF)).astype(np.float32)
    home = rng.uniform(-1, 1, NDOF).astype(np.float32)
    div = (rng.uniform(size=COUNT) < 0.05).astype(np.uint8)
    weights = np.array([Z_MIN, COS_TILT, ALIVE, W_FORWARD, W_ACTION, W_POSE], dtype=np.float32)
    vel = np.zeros((COUNT, 6), np.float32)
    tilt = np.zeros(COUNT, np.float32)
    reward = np.zeros(COUNT, np.float32)
    term = np.zeros(COUNT, np.uint8)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert ft.ft_eval(COUNT, NDOF, p(base), p(q), p(a), p(home), p(div), p(weights), p(vel), p(tilt), p(reward),
                      p(term)) == 0

    b = base.astype(np.float64)
    w64 = weights.astype(np.float64)
    R = _rotation(b[:, 3:7])
    ref_vel = np.concatenate([np.einsum("kij,kj->ki", R, b[:, 10:13]), np.einsum("kij,kj->ki", R, b[:, 7:10])], axis=1)
    ref_tilt = 1 - 2 * (b[:, 4] ** 2 + b[:, 5] ** 2)
    # every state qualifies for the exact comparison of the predicate
    far = (np.abs(b[:, 2] - w64[0]) >= MARGIN) & (np.abs(ref_tilt - w64[1]) >= MARGIN)
    assert int(far.sum()) == COUNT
    ref_term = (b[:, 2] < w64[0]) | (ref_tilt < w64[1]) | (div != 0)
    ref_reward = (np.where(ref_term, 0.0, w64[2]) + w64[3] * ref_vel[:, 0]
                  - w64[4] * (a.astype(np.float64) ** 2).sum(axis=1)
                  - w64[5] * ((q.astype(np.float64) - home.astype(np.float64)) ** 2).sum(axis=1))

    def worst(got, ref):
        return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())

    figures = {"velocity": worst(vel, ref_vel), "tilt": worst(tilt, ref_tilt), "reward": worst(reward, ref_reward)}
    print(f"float_task.hpp vs fp64, {COUNT} states: " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items())
          + f"; terminated {int(ref_term.sum())}/{COUNT}")
    assert 0.2 * COUNT < ref_term.sum() < 0.9 * COUNT    # both outcomes are exercised
    np.testing.assert_array_equal(term.astype(bool), ref_term)
    for name, v in figures.items():
        assert v <= 2e-6, (name, v)


def test_task_block_holds_every_dof(ft):
    """FloatTaskF carries the home posture of the largest model (48 bodies) and
    the contact slot masks of 8 links."""
    assert ft.ft_sizeof_task() >= 4 * (48 + 8 + 7)
    z = np.zeros(4, np.float32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert ft.ft_eval(0, 49, p(z), p(z), p(z), p(z), p(z), p(z), p(z), p(z), p(z), p(z)) == 1
