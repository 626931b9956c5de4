"""Structure of the headline step kernel's code in the built library (CPU only).

scripts/step_kernel_isa.py disassembles vecenv_step_kernel<2,0,false,true,
false,cartpole,false> and counts.  The conditions follow from the design
(DESIGN 3.1), they are not measurements:

  * its kernargs are a few flat arguments and one compact block: <= 192 bytes;
  * when the build preloads kernargs, at least the five leading pointers
    (10 dwords) arrive in SGPRs;
  * then no scalar-memory wait stands before the first state load ...
  * ... and every remaining kernarg is fetched in one batch before the first
    wait on vector memory: no s_load between the physics and the stores.
"""

import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("step_kernel_isa", os.path.join(ROOT, "scripts", "step_kernel_isa.py"))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)


def test_headline_kernel_structure():
    if isa.llvm_tools() is None:
        pytest.skip("the ROCm LLVM tools (llvm-readelf, llvm-objdump) are not installed")
    from mwstep import native
    res = isa.analyse(native.LIB_PATH)
    assert res, f"no headline step kernel found in {native.LIB_PATH}"
    print(res)
    assert res["kernarg_size"] <= 192
    preload = res["kernarg_preload_dwords"]
    if preload:
        assert preload >= 10
    assert res["lgkm_waits_before_first_global_load"] == 0
    assert res["s_load_after_first_vmcnt_wait"] == 0
