"""The library's host layer built without a GPU, for the tests that pin what the
host decides -- validation, the mirrors, the shared setters, ownership, call
order: sim.cpp, world_params.cpp, vecenv.cpp, floatenv.cpp, scene.cpp, model.cpp
and mesh.cpp over tests/sanitize/hip_standin.cpp, the stand-in for the HIP
runtime that the sanitizer lifecycle driver uses (plain g++, no sanitizer).
Device memory is host memory and the kernel launchers do nothing."""

import ctypes
import os
import subprocess

from conftest import ROOT

HOST_SOURCES = ("sim.cpp", "world_params.cpp", "vecenv.cpp", "floatenv.cpp", "scene.cpp", "model.cpp", "mesh.cpp")


def build_host(N, directory):
    """Compile the host layer into `directory` and load it with the signatures of mwstep.native."""
    csrc = os.path.join(ROOT, "gym-ignition_amd", "csrc")
    out = os.path.join(str(directory), "libmwhost.so")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    srcs = [os.path.join(csrc, f) for f in HOST_SOURCES]
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-w", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "sanitize", "hip_standin.cpp"), *srcs, "-o", out], check=True)
    L = ctypes.CDLL(out)
    for name, res, args in N.SIGNATURES:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def host_sim(N, L, model, W, steps_per_run=1):
    """An initialised simulator of a shipped model (or model text) at W worlds."""
    import numpy as np
    from mwstep import get_model_file
    sim = ctypes.c_void_p()
    mc = N.MwConfig(1e-3, 1.0, steps_per_run, W, 0, 20)
    assert L.mw_create(ctypes.byref(mc), ctypes.byref(sim)) == N.MW_OK
    pose = np.float64([0, 0, 0.45, 1, 0, 0, 0])
    try:
        model = get_model_file(model)
    except ValueError:
        pass
    assert L.mw_load_model(sim, model.encode(), N.dptr(pose), b"") == N.MW_OK, L.mw_last_error()
    assert L.mw_initialize(sim) == N.MW_OK, L.mw_last_error()
    return sim


def fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
