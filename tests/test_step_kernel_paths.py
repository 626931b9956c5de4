"""Instructions along the common path of the headline step kernel (CPU only).

scripts/step_kernel_isa.py walks the disassembly of vecenv_step_kernel<2,0,
false,true,false,cartpole,false,64,true,...> from its entry to s_endpgm, once
per role (`path_instructions`; the branch decisions are in the script's _walk):
wave 0 with a lane inside W, no limit row active and no lane done, and the
helper wave that draws the reset state.  A count, no timing.

Reference: the same script on a build of the commit before the single-substep
instantiation, the 32-bit offsets and the |o| <= hi done test:

    role     instructions   taken branches
    wave 0       216              7
    helper       155              1

That build's headline kernel ran the runtime `substeps` loop once, addressed
every load and store with 64-bit vector adds, and compared each observation
twice.  The counts of this build when the test was written, recorded and not
asserted: wave 0 166 instructions and 5 taken branches, helper 141 and 1.
"""

import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("step_kernel_isa", os.path.join(ROOT, "scripts", "step_kernel_isa.py"))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)

PARENT = {"wave0": {"instructions": 216, "taken_branches": 7},
          "helper": {"instructions": 155, "taken_branches": 1}}


def test_headline_kernel_paths_shorter_than_parent():
    if isa.llvm_tools() is None:
        pytest.skip("the ROCm LLVM tools (llvm-readelf, llvm-objdump) are not installed")
    from mwstep import native
    paths = isa.path_instructions(native.LIB_PATH)
    assert paths, f"no headline helper-wave step kernel found in {native.LIB_PATH}"
    print(paths)
    assert "error" not in paths, paths
    for role in ("wave0", "helper"):
        assert paths[role]["instructions"] < PARENT[role]["instructions"], role
        assert paths[role]["taken_branches"] <= PARENT[role]["taken_branches"], role
    # the walked wave-0 path is the one that stores: reward, done, obs, q, qd (2 dofs each), steps
    assert paths["wave0"]["stores"] == 8 and paths["helper"]["stores"] == 0


def test_headline_is_the_single_substep_instantiation():
    if isa.llvm_tools() is None:
        pytest.skip("the ROCm LLVM tools (llvm-readelf, llvm-objdump) are not installed")
    from mwstep import native
    res = isa.analyse(native.LIB_PATH)
    assert res and res["kernel"].split("EEv")[0].endswith("Li64ELb1ELb1E"), res and res["kernel"]
