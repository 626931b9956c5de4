"""The push schedule of the floating-base env's randomisation
(gym-ignition_amd/csrc/float_task.hpp: ft_push_phase / ft_push_active /
ft_push_block) compiled for the host (g++, test-only harness
tests/host_float_rand/harness.cpp) against a Python restatement of the rule in
include/mwstep.h: with t the steps already taken in the episode,
k = (t + phase) // interval, o = (t + phase) % interval, the step is pushed iff
o < push_steps, and push k draws from Philox block 0x80000000 | k.  Integers:
everything must be exactly equal."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "gym-ignition_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "host_float_rand", "harness.cpp")
INTERVALS = (1, 2, 7, 50)


@pytest.fixture(scope="module")
def fr(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fr") / "libfr.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, HARNESS, "-o", out], check=True)
    L = ctypes.CDLL(out)
    u = ctypes.c_uint32
    L.fr_episode_block.restype = u
    L.fr_phase.restype = u
    L.fr_phase.argtypes = [u, u]
    L.fr_schedule.restype = None
    L.fr_schedule.argtypes = [u, u, u, u, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return L


def _schedule(fr, count, phase, interval, push_steps):
    active = np.zeros(count, np.uint8)
    k = np.zeros(count, np.uint32)
    block = np.zeros(count, np.uint32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    fr.fr_schedule(count, phase, interval, push_steps, p(active), p(k), p(block))
    return active, k, block


@pytest.mark.parametrize("interval", INTERVALS)
def test_schedule_matches_the_restatement(fr, interval):
    count = 3 * interval
    for push_steps in sorted({1, interval}):
        for phase in range(interval):
            active, k, block = _schedule(fr, count, phase, interval, push_steps)
            t = np.arange(count, dtype=np.int64)
            ref_k = (t + phase) // interval
            ref_active = ((t + phase) % interval) < push_steps
            np.testing.assert_array_equal(k, ref_k, err_msg=f"k: {interval} {push_steps} {phase}")
            np.testing.assert_array_equal(active.astype(bool), ref_active,
                                          err_msg=f"active: {interval} {push_steps} {phase}")
            np.testing.assert_array_equal(block, 0x80000000 | ref_k)
            # every window of `interval` steps holds exactly push_steps pushed ones
            for s in range(count - interval + 1):
                assert int(active[s:s + interval].sum()) == push_steps
            if push_steps == interval:
                assert active.all()


def test_phase_and_blocks(fr):
    """phase = r[0] % interval (0 when pushes are off), and the randomisation
    blocks lie beyond every block a reset draw can use ((n + 3) // 4 <= 12)."""
    rng = np.random.default_rng(5)
    words = [0, 1, 6, 7, 49, 50, 2**31, 2**32 - 1] + rng.integers(0, 2**32, 200).tolist()
    for interval in INTERVALS:
        for r0 in words:
            assert fr.fr_phase(r0, interval) == r0 % interval
    assert fr.fr_phase(12345, 0) == 0
    assert fr.fr_episode_block() == 0x40000000
    _, k, block = _schedule(fr, 200, 6, 7, 2)
    assert block.min() >= 0x80000000 and len(set(block.tolist())) == len(set(k.tolist()))
    assert fr.fr_episode_block() > 12 and fr.fr_episode_block() not in set(block.tolist())
