"""Shared by the tests of the per-world link parameters and the inertia
randomisation (test helper): the host build of the kernel's inertial-word
arithmetic with its derived error bound (tests/host_float_inertia/harness.cpp),
the same operation sequence in numpy fp64, the fp64 parallel-axis shift from the
kernel's origin words back to an inertia about the centre of mass, and the
host restatement of the env's draws from the oracle's Philox4x32-10."""

import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "gym-ignition_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "host_float_inertia", "harness.cpp")
SCALE_BLOCK, PAYLOAD_BLOCK = 0x40000100, 0x40000180
SCALE, PAYLOAD = 1, 2


def build_harness(directory):
    out = os.path.join(str(directory), "libfi.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-DMW_HOST_TEST", "-I", CSRC,
                    HARNESS, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.fi_apply.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6
    L.fi_scale_block.restype = ctypes.c_uint
    L.fi_scale_block.argtypes = [ctypes.c_int]
    L.fi_payload_block.restype = ctypes.c_uint
    return L


def harness_apply(L, flags, w0, s, mp, p):
    """(float32 words [k, 10], derived bound [k, 10]) of the kernel's code on float32 inputs."""
    w0, s, mp, p = (np.ascontiguousarray(a, dtype=np.float32) for a in (w0, s, mp, p))
    k = len(w0)
    assert w0.shape == (k, 10) and s.shape == (k,) and mp.shape == (k,) and p.shape == (k, 3)
    out, bound = np.zeros((k, 10), np.float32), np.zeros((k, 10))
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    L.fi_apply(k, flags, ptr(w0), ptr(s), ptr(mp), ptr(p), ptr(out), ptr(bound))
    return out, bound


def apply_ref(flags, w0, s, mp, p):
    """The stated sequence in fp64 on the same float32 inputs: mass and origin
    inertia scaled, the centre of mass kept; then the point mass mp at p:
    m' = m + mp, com' = (m com + mp p) / m', Io' = Io + mp (|p|^2 1 - p p^T)."""
    w = np.array(w0, dtype=np.float64)
    s, mp, p = (np.asarray(a, dtype=np.float64) for a in (s, mp, p))
    if flags & SCALE:
        w[:, 0] *= s
        w[:, 4:] *= s[:, None]
    if flags & PAYLOAD:
        m = w[:, 0].copy()
        w[:, 0] = m + mp
        w[:, 1:4] = (m[:, None] * w[:, 1:4] + mp[:, None] * p) / w[:, 0:1]
        p2 = (p * p).sum(1)
        w[:, 4:7] += mp[:, None] * (p2[:, None] - p * p)
        w[:, 7] -= mp * p[:, 0] * p[:, 1]
        w[:, 8] -= mp * p[:, 0] * p[:, 2]
        w[:, 9] -= mp * p[:, 1] * p[:, 2]
    return w


def inertia_about_com(words):
    """[..., 10] origin words -> (mass, com [..., 3], Ic [..., 3, 3]) in fp64."""
    w = np.asarray(words, dtype=np.float64)
    m, c = w[..., 0], w[..., 1:4]
    Io = np.empty(w.shape[:-1] + (3, 3))
    for (r, q), k in {(0, 0): 4, (1, 1): 5, (2, 2): 6, (0, 1): 7, (0, 2): 8, (1, 2): 9}.items():
        Io[..., r, q] = Io[..., q, r] = w[..., k]
    c2 = (c * c).sum(-1)
    shift = c2[..., None, None] * np.eye(3) - c[..., :, None] * c[..., None, :]
    return m, c, Io - m[..., None, None] * shift


def _unif32(word, lo, hi):
    t = np.float32(np.float32(int(word) >> 8) * np.float32(1.0 / 16777216.0))
    return np.float32(np.float32(lo) + (np.float32(hi) - np.float32(lo)) * t)


def draw_ref(oracle, seed, world, episode, n, scale_range, payload_range, box):
    """The env's draw of (global world, episode): scales [n + 1] (base first)
    from word k % 4 of block 0x40000100 | k / 4, payload mass and position
    from block 0x40000180; the unfused float32 form of U(lo, hi)."""
    key = [seed & 0xFFFFFFFF, seed >> 32]
    s = np.ones(n + 1, np.float32)
    if scale_range is not None:
        for k in range(n + 1):
            r = oracle.philox_raw([world, episode, SCALE_BLOCK | (k // 4), 0], key)
            s[k] = _unif32(r[k % 4], *scale_range)
    mp, p = np.float32(0), np.zeros(3, np.float32)
    if payload_range is not None:
        r = oracle.philox_raw([world, episode, PAYLOAD_BLOCK, 0], key)
        mp = _unif32(r[0], *payload_range)
        p = np.float32([_unif32(r[1 + k], -box[k], box[k]) for k in range(3)])
    return s, mp, p
