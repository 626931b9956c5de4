// Test-only reader of an env handle of the host build (tests/host_build.py):
// what an accepted mw_floatenv_tracking left in the env's FloatTaskF, and the
// bytes of the whole struct, so tests/test_float_track_abi.py can see that a
// refused call changed nothing.  The host build's device memory is host memory,
// so the clip table and the joint weights can be read through their pointers.
// Built into a library of its own against the same headers.  Not part of the
// product.
#include <cstring>

#include "vecenv_state.hpp"

extern "C" int ftk_task_bytes(const mw_vecenv* e, unsigned char* out, int cap) {
    if (!e || !e->fenv) return -1;
    const int bytes = static_cast<int>(sizeof(mw::FloatTaskF));
    if (out && cap >= bytes) std::memcpy(out, &e->fenv->ftask, sizeof(mw::FloatTaskF));
    return bytes;
}

// i = on, n_clips, frame_num, frame_den, obs_reference, nb, n_obs, init.on, init.n_states;
// f = rsi_prob, ang_scale, weight[5], scale[5], max_pose, max_root_pos, max_root_rot;
// table [n_clips][4] and wj [n] where on; p = clips, terms_out, errors_out, clip_out, frame_out
extern "C" int ftk_track_fields(const mw_vecenv* e, int* i, float* f, int* table, float* wj, int n, const void** p) {
    if (!e || !e->fenv) return -1;
    const mw::FloatTaskF& T = e->fenv->ftask;
    const mw::FloatTrackF& K = T.track;
    i[0] = static_cast<int>(K.on);
    i[1] = K.n_clips;
    i[2] = K.frame_num;
    i[3] = K.frame_den;
    i[4] = K.obs_reference;
    i[5] = K.nb;
    i[6] = T.n_obs;
    i[7] = static_cast<int>(T.init.on);
    i[8] = T.init.n_states;
    f[0] = K.rsi_prob;
    f[1] = K.ang_scale;
    for (int k = 0; k < mw::kTrackTerms; ++k) {
        f[2 + k] = K.weight[k];
        f[7 + k] = K.scale[k];
    }
    f[12] = K.max_pose;
    f[13] = K.max_root_pos;
    f[14] = K.max_root_rot;
    if (K.on) {
        for (int k = 0; k < K.n_clips * mw::kTrackTableWords; ++k) table[k] = K.table[k];
        for (int d = 0; d < n; ++d) wj[d] = K.wj[d];
    }
    p[0] = K.clips;
    p[1] = K.terms_out;
    p[2] = K.errors_out;
    p[3] = K.clip_out;
    p[4] = K.frame_out;
    return static_cast<int>(sizeof(mw::FloatTrackF));
}
