"""Bit-identity of the batched env's step kernels with the recorded build.

tests/golden/step_bits.json holds sha256 digests of obs, reward, done,
terminal_obs, q, qd, steps and episode (and the sampled physics of the
randomised variant) written by tests/golden/make_step_bits.py on the GPU from
the build that preceded the step kernel's flat, preloaded argument list.  The
kernels' arithmetic has not changed since, so the digests must be EQUAL: how
the arguments reach the kernel, the workgroup-size template and the order of
its loads may not move one bit of any result.

Cases (make_step_bits.py): the four tasks, CartPole discrete with randomised
physics, with world_offset=1000, with two substeps per step, and as a fused
50-step rollout; 1, 65 (a partial second wave) and 16449 worlds (256-thread
workgroups, partial last one); each on the constant-folded and on the generic
kernel.  120 closed-loop steps with max_episode_steps=40.

The randomised kernels have 36 more cases, recorded later from a build that
reproduced the digests above: randomised physics on the other three tasks, and
CartPole discrete with randomised physics as a fused rollout, with
world_offset=1000 and with two substeps.  A digest shows a change; that the
values are right is tests/test_gpu_randomized_matrix.py's business.
"""

import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_step_bits", os.path.join(_GOLDEN, "make_step_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.fixture(scope="module")
def recorded():
    with open(bits.FIXTURE) as f:
        doc = json.load(f)
    assert (doc["steps"], doc["max_episode_steps"], doc["rollout_steps"]) == (
        bits.STEPS, bits.MAX_EPISODE_STEPS, bits.ROLLOUT_STEPS)
    assert sorted(doc["digests"]) == sorted(c[0] for c in bits.CASES)
    return doc["digests"]


@pytest.mark.parametrize("case", bits.CASES, ids=[c[0] for c in bits.CASES])
def test_step_bits(require_gpu, recorded, monkeypatch, case):
    if case[5]:
        monkeypatch.setenv("MWSTEP_DISABLE_BAKED", "1")
    else:
        monkeypatch.delenv("MWSTEP_DISABLE_BAKED", raising=False)
    got = bits.run_case(case)
    want = recorded[case[0]]
    differing = sorted(k for k in want if got.get(k) != want[k])
    assert not differing and sorted(got) == sorted(want), f"{case[0]}: digests differ for {differing}"
