"""The host build of the floating-base env's shaping arithmetic
(tests/host_float_shape/harness.cpp over gym-ignition_amd/csrc/float_task.hpp)
behind numpy: shared by tests/test_float_shape_host.py, which checks it against
fp64, and tests/test_gpu_float_shape.py, which checks the device against it."""

import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "gym-ignition_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "host_float_shape", "harness.cpp")
TERMS = ("torque", "power", "joint_acc", "orientation", "base_height", "joint_limits", "collision", "stumble",
         "contact_force", "stand_still")
FLT_MAX = np.float32(3.402823466e+38)


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def _f(x):
    return np.ascontiguousarray(x, dtype=np.float32)


class ShapeHost:
    """The harness, built once into `directory`."""

    def __init__(self, directory):
        out = os.path.join(str(directory), "libfs.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, HARNESS, "-o", out], check=True)
        L = self.L = ctypes.CDLL(out)
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.fs_soft_limits.argtypes = [ci, vp, vp, cf, vp, vp]
        L.fs_tau.argtypes = [ci, vp, vp, vp]
        L.fs_world.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, vp, ci, vp, vp, ci, ci, vp, vp]
        L.fs_reward.restype = cf
        L.fs_reward.argtypes = [cf, vp]
        L.fs_force_norm.restype = cf
        L.fs_force_norm.argtypes = [cf, cf, cf]
        L.fs_standing.argtypes = [cf, cf, cf]
        L.fs_terminated.argtypes = [vp, ci, vp]
        L.fs_stats.argtypes = [ci] + [vp] * 11

    @staticmethod
    def params(weights, base_height_target=0.0, collision_force_min=0.0, stumble_ratio=0.0, max_contact_force=0.0,
               termination_force=0.0, env_dt=1e-3):
        """The parameter words of fs_world / fs_terminated; weights: a name -> weight mapping or ten values."""
        w = np.zeros(10, np.float32)
        if isinstance(weights, dict):
            for name, value in weights.items():
                w[TERMS.index(name)] = value
        else:
            w[:] = weights
        return np.concatenate([w, _f([base_height_target, collision_force_min, stumble_ratio, max_contact_force,
                                      termination_force, env_dt])])

    def soft_limits(self, lower, upper, soft):
        lower, upper = _f(lower), _f(upper)
        lo, hi = np.zeros_like(lower), np.zeros_like(upper)
        self.L.fs_soft_limits(len(lower), _p(lower), _p(upper), soft, _p(lo), _p(hi))
        return lo, hi

    def tau(self, u, effort):
        u, effort = _f(u).ravel(), _f(effort).ravel()
        out = np.zeros_like(u)
        self.L.fs_tau(len(u), _p(u), _p(effort), _p(out))
        return out

    def world(self, par, tau, q, qd, qd_prev, lo, hi, home, contact_f, pen_f, pose, standing=False, diverged=False):
        """(x [10], term [10]) of one world."""
        tau, q, qd, qd_prev, lo, hi, home = (_f(a) for a in (tau, q, qd, qd_prev, lo, hi, home))
        contact_f, pen_f, pose, par = _f(contact_f).reshape(-1, 3), _f(pen_f).reshape(-1, 3), _f(pose), _f(par)
        x, term = np.zeros(10, np.float32), np.zeros(10, np.float32)
        self.L.fs_world(_p(par), len(q), _p(tau), _p(q), _p(qd), _p(qd_prev), _p(lo), _p(hi), _p(home),
                        len(contact_f), _p(contact_f), len(pen_f), _p(pen_f), _p(pose), int(standing), int(diverged),
                        _p(x), _p(term))
        return x, term

    def reward(self, r_existing, term):
        term = _f(term)
        return np.float32(self.L.fs_reward(float(r_existing), _p(term)))

    def force_norm(self, f):
        return np.float32(self.L.fs_force_norm(float(f[0]), float(f[1]), float(f[2])))

    def standing(self, cx, cy, cmd_min):
        return bool(self.L.fs_standing(float(cx), float(cy), float(cmd_min)))

    def terminated(self, par, forces):
        forces, par = _f(forces).reshape(-1, 3), _f(par)
        return bool(self.L.fs_terminated(_p(par), len(forces), _p(forces)))

    def stats(self, reward, term, diverged, done):
        reward, term = _f(reward), _f(term).reshape(-1, 10)
        T = len(reward)
        diverged, done = (np.ascontiguousarray(a, dtype=np.uint8) for a in (diverged, done))
        out = dict(acc_return=np.zeros(T, np.float32), acc_length=np.zeros(T, np.int32),
                   acc_terms=np.zeros((T, 10), np.float32), finished=np.zeros(T, np.uint8),
                   ep_return=np.zeros(T, np.float32), ep_length=np.zeros(T, np.int32),
                   ep_terms=np.zeros((T, 10), np.float32))
        self.L.fs_stats(T, _p(reward), _p(term), _p(diverged), _p(done), *[_p(out[k]) for k in (
            "acc_return", "acc_length", "acc_terms", "finished", "ep_return", "ep_length", "ep_terms")])
        return out
