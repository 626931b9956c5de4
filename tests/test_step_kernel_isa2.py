"""Stores and LDS of the headline step kernel's code in the built library (CPU only).

scripts/step_kernel_isa.py disassembles vecenv_step_kernel<2,0,false,true,
false,cartpole,false,64,...>.  Conditions of the design, not
measurements:

  * no store waits for an earlier store: no `s_waitcnt vmcnt` can execute
    after a `global_store` (the use that keeps the action load with the state
    loads stands ahead of the first store);
  * the seven loads still issue together, before the first vector-memory wait;
  * the headline kernel is the helper-wave variant: it has LDS (the reset
    state handed from the helper wave to the physics wave), 2 * N * 64 floats.
"""

import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("step_kernel_isa", os.path.join(ROOT, "scripts", "step_kernel_isa.py"))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)

HELPER_WAVE_KEPT = True   # the helper wave paid and was kept


def test_headline_kernel_stores_and_lds():
    if isa.llvm_tools() is None:
        pytest.skip("the ROCm LLVM tools (llvm-readelf, llvm-objdump) are not installed")
    from mwstep import native
    res = isa.analyse(native.LIB_PATH)
    assert res, f"no headline step kernel found in {native.LIB_PATH}"
    print(res)
    assert res["vmcnt_waits_after_first_store"] == 0
    assert res["global_loads_before_first_vmcnt_wait"] == res["global_loads"] == 7
    assert (res["lds_bytes"] > 0) == HELPER_WAVE_KEPT
    if HELPER_WAVE_KEPT:
        assert res["lds_bytes"] == 2 * 2 * 64 * 4
