// Host build of the joint randomisation's arithmetic (csrc/float_task.hpp:
// ft_joint_words, ft_joint_block), test only: the float32 code the post kernel
// runs per joint, with g++ (-DMW_HOST_TEST -ffp-contract=off).
//
// Each of the three words is one rounded operation on float32 inputs --
// damping = fl(damping0 + a), friction = fl(friction0 + f), effort =
// fl(s effort0) -- so each lies within one float32 rounding, u |exact| with
// u = 2^-24, of the exact result; an unbounded effort limit (FLT_MAX) is kept.
#include "float_task.hpp"

// nom [count][3], draw [count][3]: float32 inputs; flags bit 0: damping, bit 1:
// friction, bit 2: effort (a feature that is off keeps the nominal word, as in
// the kernel).  out [count][3]: the float32 words.
extern "C" void fj_apply(int count, int flags, const float* nom, const float* draw, float* out) {
    for (int i = 0; i < count; ++i) {
        const float n[3] = {nom[3 * i], nom[3 * i + 1], nom[3 * i + 2]};
        const float a[3] = {draw[3 * i], draw[3 * i + 1], draw[3 * i + 2]};
        float w[3];
        mw::dev::ft_joint_words(n, a, w);
        for (int e = 0; e < 3; ++e) out[3 * i + e] = (flags >> e) & 1 ? w[e] : n[e];
    }
}

extern "C" unsigned fj_joint_block(int d) { return mw::dev::ft_joint_block(d); }
extern "C" unsigned fj_scale_block(int k) { return mw::dev::ft_scale_block(k); }
extern "C" unsigned fj_payload_block() { return mw::kFtPayloadBlock; }
extern "C" unsigned fj_episode_block() { return mw::kFtEpisodeBlock; }
extern "C" unsigned fj_push_block(unsigned k) { return mw::dev::ft_push_block(k); }
extern "C" unsigned fj_cmd_block(unsigned k) { return mw::dev::ft_cmd_block(k); }
extern "C" int fj_word(int e) { return e == 0 ? mw::kFtBodyDamping : e == 1 ? mw::kFtBodyFriction : mw::kFtBodyEffort; }
