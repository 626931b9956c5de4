// world_params.hpp -- layout of the wave kernel's per-world parameter records
// (RunArgs::wpar; mw_sim::d_wpar / h_wpar).  Plain C++: the kernels, the host
// module that owns the records (world_params.cpp) and the host harnesses under
// tests/ all index a record through these values.
//
// One record of wpar_stride_words(n) float words per world, wave-uniform like
// the per-world friction (RunArgs::mu):
//   [0, kWparInertialWords)  the base's inertial words, as FloatF's first ten:
//                            mass, com[3], Io[6] about the origin (padded to
//                            kWparBaseWords)
//   [kWparBaseWords, ..)     the world's body block, stored compactly: the
//                            ChainF header (kWparHeadWords) and n BodyF, not
//                            the 48-body struct; the kernel reads it as a ChainF
// The inertial words (mw_set_link_params) and a joint's damping, friction and
// effort (mw_set_joint_dynamics) differ between worlds; everything else in the
// body block (joint frames, position limits) is a copy of the shared ChainF,
// and every setter that rewrites the shared block (mw_set_joint_param,
// mw_set_gravity: upload_params) rewrites all copies, keeping each world's own
// words.  FloatF (ground, shapes, gravity, topology tables) is not duplicated
// and keeps one owner.  With wpar set the kernel runs its WPAR instances, which
// imply the per-world friction read: mu is then non-null as well.
//
// Device code addresses a record as float words at these constant offsets (no
// BodyF* member stores); the host uses the same offsets or copies whole BodyF.
#pragma once

#include <cstddef>
#include <cstdint>

#include "chain_params.hpp"

namespace mw {

// The base block is the one chosen layout: FloatF's leading mass, com[3],
// Io[6] (world_params.cpp, which copies them, asserts that FloatF starts with
// them), padded to sixteen words.  Everything else follows the types.
constexpr int kWparInertialWords = 10;
constexpr int kWparBaseWords = 16;
constexpr int kWparHeadWords = static_cast<int>(offsetof(ChainF, b) / sizeof(float));
constexpr int kWparBodyWords = static_cast<int>(sizeof(BodyF) / sizeof(float));
constexpr int kWparBody0 = kWparBaseWords + kWparHeadWords;  // words of a record before its first BodyF
// words of a BodyF: its ten inertial words (mass, com[3], Io[6]) start at
// kBodyInertial; the three joint dynamics words of mw_set_joint_dynamics
constexpr int kBodyInertial = static_cast<int>(offsetof(BodyF, mass) / sizeof(float));
constexpr int kBodyDamping = static_cast<int>(offsetof(BodyF, damping) / sizeof(float));
constexpr int kBodyFriction = static_cast<int>(offsetof(BodyF, friction) / sizeof(float));
constexpr int kBodyEffort = static_cast<int>(offsetof(BodyF, effort) / sizeof(float));
constexpr int kBodyJointWord[3] = {kBodyDamping, kBodyFriction, kBodyEffort};
// the names tests/host_float_joints/harness.cpp exports the three words under
constexpr int kFtBodyDamping = kBodyDamping, kFtBodyFriction = kBodyFriction, kFtBodyEffort = kBodyEffort;
static_assert(kBodyDamping == kBodyInertial + kWparInertialWords, "a body's inertial words end where its damping starts");

// words of a record of n bodies; of the ChainF header and n bodies alone
constexpr int chain_words(int n) { return kWparHeadWords + kWparBodyWords * n; }
constexpr int wpar_stride_words(int n) { return kWparBaseWords + chain_words(n); }
// word offset of body d inside a record, and of the ten inertial words of
// link k (-1 = the base)
constexpr int wpar_body_word(int d) { return kWparBody0 + kWparBodyWords * d; }
constexpr int wpar_inertial_word(int k) { return k < 0 ? 0 : wpar_body_word(k) + kBodyInertial; }

}  // namespace mw
