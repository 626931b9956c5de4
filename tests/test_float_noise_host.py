"""The arithmetic of the floating-base env's observation noise and action
latency (gym-ignition_amd/csrc/float_task.hpp: ft_noise_unit, ft_noisy,
ft_delay_draw, ft_delay_neutral, ft_delay_slot) compiled for the host (g++,
float32, test-only harness tests/host_float_noise/harness.cpp) -- the code the
env kernels run per word and per world, checked without a GPU.

The noise unit is exact: -1 + (x >> 8) 2^-23, a multiple of 2^-23 in [-1, 1),
compared bit for bit with fp64.  The noisy word is within 2^-23 (|clean| + amp)
of fp64: two roundings at most, one where the operation is fused.  The delay
draw is an integer and must stay in its range and reach every value of it.
The ring is checked against a brute-force model that keeps, per slot, the
action an episode wrote there: for every R in 1..9, every d < R and t in 0..40
the applied slot holds a_{t-d}, t < d selects the neutral command, and no slot
is read before the episode wrote it."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "gym-ignition_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "host_float_noise", "harness.cpp")
COUNT = 4000


@pytest.fixture(scope="module")
def fn(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fn") / "libfn.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, HARNESS, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.fn_noise_unit.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 2
    L.fn_noisy.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4
    L.fn_delay_draw.restype = ctypes.c_uint
    L.fn_delay_draw.argtypes = [ctypes.c_uint] * 3
    L.fn_ring.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_uint] + [ctypes.c_void_p] * 3
    return L


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def _units(fn, x):
    u = np.zeros(len(x), np.float32)
    fn.fn_noise_unit(len(x), _p(x), _p(u))
    return u


def test_noise_unit_is_exact(fn):
    rng = np.random.default_rng(31)
    x = rng.integers(0, 2 ** 32, COUNT, dtype=np.uint64).astype(np.uint32)
    x[:8] = [0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0x800000FF, 0xFFFFFF00, 0xFFFFFFFF]
    u = _units(fn, x)
    ref = -1.0 + (x >> np.uint32(8)).astype(np.float64) * 2.0 ** -23
    np.testing.assert_array_equal(u.astype(np.float64), ref)
    assert u.min() == -1.0 and u.max() == np.float32(1.0 - 2.0 ** -23)      # x = 0 and x = 0xFFFFFFFF
    assert (u >= -1.0).all() and (u < 1.0).all()
    np.testing.assert_array_equal(u.astype(np.float64) * 2.0 ** 23 % 1.0, 0.0)
    assert list(u[:3]) == [-1.0, -1.0, np.float32(-1.0 + 2.0 ** -23)] and u[4] == 0.0


def test_noisy_word_matches_fp64(fn):
    rng = np.random.default_rng(32)
    clean = (rng.uniform(-1, 1, COUNT) * 10.0 ** rng.uniform(-4, 3, COUNT)).astype(np.float32)
    amp = (10.0 ** rng.uniform(-4, 1, COUNT)).astype(np.float32)
    clean[::11] = 0.0
    amp[::13] = 0.0
    u = _units(fn, rng.integers(0, 2 ** 32, COUNT, dtype=np.uint64).astype(np.uint32))
    out = np.zeros(COUNT, np.float32)
    fn.fn_noisy(COUNT, _p(clean), _p(amp), _p(u), _p(out))
    c64, a64 = clean.astype(np.float64), amp.astype(np.float64)
    ref = c64 + a64 * u.astype(np.float64)
    bound = 2.0 ** -23 * (np.abs(c64) + a64)
    err = np.abs(out - ref)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"ft_noisy vs fp64, {COUNT} words: worst error / bound {ratio:.3f}")
    assert (err <= bound).all()
    # a zero amplitude leaves the value alone (the kernel skips such a word: its bits stay too)
    np.testing.assert_array_equal(out[amp == 0], clean[amp == 0])
    assert (out != clean).sum() > 0.8 * COUNT


def test_delay_draw_stays_in_range_and_reaches_every_value(fn):
    rng = np.random.default_rng(33)
    words = [0, 1, 2 ** 31, 2 ** 32 - 1] + rng.integers(0, 2 ** 32, 500, dtype=np.uint64).tolist()
    hi_max = fn.fn_max_delay()
    assert hi_max == 8
    for lo in range(hi_max + 1):
        for hi in range(lo, hi_max + 1):
            got = [fn.fn_delay_draw(int(r), lo, hi) for r in words]
            assert got == [lo + int(r) % (hi - lo + 1) for r in words]
            assert set(got) == set(range(lo, hi + 1)), (lo, hi)


def test_ring_against_a_brute_force_model(fn):
    steps = 41                                        # t in 0..40
    reads = 0
    for R in range(1, 10):
        for d in range(R):
            stored, applied = np.zeros(steps, np.int32), np.zeros(steps, np.int32)
            neutral = np.zeros(steps, np.uint8)
            fn.fn_ring(steps, d, R, _p(stored), _p(applied), _p(neutral))
            ring = {}                                 # slot -> the step whose action this episode wrote there
            for t in range(steps):
                assert 0 <= stored[t] < R
                ring[int(stored[t])] = t
                assert bool(neutral[t]) == (t < d), (R, d, t)
                if t < d:
                    assert applied[t] == -1           # nothing is read
                    continue
                assert int(applied[t]) in ring, f"R {R} d {d} t {t}: slot {applied[t]} read before it was written"
                assert ring[int(applied[t])] == t - d, (R, d, t)
                reads += 1
    assert reads == sum(steps - d for R in range(1, 10) for d in range(R))
