"""The word function of the joint randomisation (gym-ignition_amd/csrc/
float_task.hpp: ft_joint_words) compiled for the host (g++, float32,
tests/host_float_joints/harness.cpp) against numpy fp64 on 1,000 random
(nominal, draw) triples -- the code the post kernel runs per joint, checked
without a GPU.

Each word is one rounded float32 operation on float32 inputs, so it must lie
within one rounding of the exact result: |got - exact| <= 2^-24 |exact|, and
be exactly the float32 nearest to it.  An unbounded effort limit (FLT_MAX) is
kept, not scaled.  The Philox block of every joint 0..47 is distinct from every
block already in use."""

import numpy as np
import pytest

from float_joints_ref import DAMPING, EFFORT, FLT_MAX, FRICTION, JOINT_BLOCK, build_harness, harness_apply

COUNT = 1000
U = 2.0 ** -24


@pytest.fixture(scope="module")
def fj(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("fj"))


def test_words_are_within_one_rounding_of_fp64(fj):
    rng = np.random.default_rng(37)
    nom = np.column_stack([rng.uniform(0.0, 2.0, COUNT), rng.uniform(0.0, 5.0, COUNT),
                           rng.uniform(1.0, 200.0, COUNT)]).astype(np.float32)
    nom[::7, 0] = 0.0      # the shipped robots have no <dynamics>: zero damping
    nom[::5, 1] = 0.0      # ... and zero friction
    draw = np.column_stack([rng.uniform(0.0, 0.5, COUNT), rng.uniform(0.0, 2.0, COUNT),
                            rng.uniform(0.1, 1.0, COUNT)]).astype(np.float32)
    got = harness_apply(fj, DAMPING | FRICTION | EFFORT, nom, draw)
    n64, d64 = nom.astype(np.float64), draw.astype(np.float64)
    exact = np.column_stack([n64[:, 0] + d64[:, 0], n64[:, 1] + d64[:, 1], d64[:, 2] * n64[:, 2]])
    err = np.abs(got.astype(np.float64) - exact)
    for e, label in enumerate(("damping", "friction", "effort")):
        print(f"{label}: worst |error| / (2^-24 |exact|) {float((err[:, e] / (U * np.abs(exact[:, e]))).max()):.3f}")
    assert (err <= U * np.abs(exact)).all(), np.argwhere(err > U * np.abs(exact))[:5]
    np.testing.assert_array_equal(got, exact.astype(np.float32))        # the correctly rounded result
    assert got.dtype == np.float32 and (got[:, :2] >= 0).all() and (got[:, 2] > 0).all()
    # a feature that is off keeps the nominal word, whatever the draw holds
    for flags in (DAMPING, FRICTION, EFFORT, DAMPING | EFFORT):
        part = harness_apply(fj, flags, nom, draw)
        for e in range(3):
            np.testing.assert_array_equal(part[:, e], got[:, e] if flags >> e & 1 else nom[:, e])
    # the neutral draws change no bit
    neutral = np.tile(np.float32([0.0, 0.0, 1.0]), (COUNT, 1))
    np.testing.assert_array_equal(harness_apply(fj, 7, nom, neutral), nom)


def test_unbounded_effort_is_kept(fj):
    nom = np.float32([[0.0, 0.0, FLT_MAX], [0.1, 0.2, FLT_MAX], [0.0, 0.0, 60.0]])
    draw = np.float32([[0.1, 0.5, 0.25], [0.0, 0.0, 1.0], [0.1, 0.5, 0.25]])
    got = harness_apply(fj, 7, nom, draw)
    assert got[0, 2] == FLT_MAX and got[1, 2] == FLT_MAX and got[2, 2] == np.float32(15.0)
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got[:, :2], nom[:, :2] + draw[:, :2])


def test_blocks_collide_with_no_other_draw(fj):
    """Block 0x40000200 | d, words 0..2, for every joint 0..47 against the reset
    blocks 0..11, the episode block 0x40000000, the scale blocks 0x40000100 |
    k / 4, the payload block 0x40000180 and the push (0x80000000) and command
    (0xC0000000) families."""
    mine = [fj.fj_joint_block(d) for d in range(48)]
    assert mine == [JOINT_BLOCK | d for d in range(48)] and len(set(mine)) == 48
    assert [fj.fj_word(e) for e in range(3)] == [26, 27, 30]           # BodyF damping, friction, effort
    others = set(range(12)) | {fj.fj_episode_block(), fj.fj_payload_block()}
    others |= {fj.fj_scale_block(k) for k in range(49)}
    others |= {fj.fj_push_block(k) for k in (0, 1, 1000, 0x3FFFFFFF)} | {fj.fj_cmd_block(k) for k in (0, 1, 1000)}
    assert fj.fj_episode_block() == 0x40000000 and fj.fj_payload_block() == 0x40000180
    assert not others & set(mine)
    for b in mine:
        assert b >= 12 and b & 0xC0000000 == 0x40000000 and 0x40000200 <= b < 0x40000230
        assert b & 0xFFFFFF00 != 0x40000100                             # not in the scale / payload page
