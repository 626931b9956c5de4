// Test-only host build of the arithmetic of the motion-clip tracking task
// (gym-ignition_amd/csrc/float_task.hpp: ft_track_clip, ft_track_start,
// ft_track_clock, ft_track_phase, ft_track_phase_words, ft_track_lerp,
// ft_track_wrapped, ft_track_nlerp, ft_track_errors, ft_track_terms,
// ft_track_reward, ft_track_failed): what the post kernel runs per world, on the
// CPU in float32, so tests/test_float_track_host.py can compare it with the fp64
// restatement of tests/float_track_ref.py without a GPU, and the GPU tests can
// ask for the same bits.  Not part of the product.
#define MW_HOST_TEST 1
#include "float_task.hpp"

using namespace mw;

extern "C" unsigned ftk_block() { return kFtTrackBlock; }
extern "C" int ftk_max_clips() { return kMaxClips; }
extern "C" int ftk_terms_count() { return kTrackTerms; }

extern "C" void ftk_clip(int count, const unsigned* r0, int n_clips, int* out) {
    for (int i = 0; i < count; ++i) out[i] = dev::ft_track_clip(r0[i], n_clips);
}
extern "C" void ftk_start(int count, const unsigned* r1, const unsigned* r2, int length, float prob, int* out) {
    for (int i = 0; i < count; ++i) out[i] = dev::ft_track_start(r1[i], r2[i], length, prob);
}

// f0 [count], t [count] -> ints [count][4] (i, i1, wraps, ended), a [count]
extern "C" void ftk_clock(int count, const int* f0, const unsigned* t, int num, int den, int length, int loop, int* ints,
                          float* a) {
    for (int k = 0; k < count; ++k) {
        const dev::TrackClock c = dev::ft_track_clock(f0[k], t[k], num, den, length, loop != 0);
        ints[4 * k] = c.i;
        ints[4 * k + 1] = c.i1;
        ints[4 * k + 2] = static_cast<int>(c.wraps);
        ints[4 * k + 3] = c.ended ? 1 : 0;
        a[k] = c.a;
    }
}

// i [count], a [count] -> out [count][3]: phi, sin, cos
extern "C" void ftk_phase(int count, const int* i, const float* a, int length, float* out) {
    for (int k = 0; k < count; ++k) {
        const float phi = dev::ft_track_phase(i[k], a[k], length);
        out[3 * k] = phi;
        dev::ft_track_phase_words(phi, out[3 * k + 1], out[3 * k + 2]);
    }
}

extern "C" void ftk_lerp(int count, const float* p0, const float* p1, const float* a, float* out) {
    for (int k = 0; k < count; ++k) out[k] = dev::ft_track_lerp(p0[k], p1[k], a[k]);
}
extern "C" void ftk_wrapped(int count, const float* word, const unsigned* wraps, const float* last, const float* first,
                            float* out) {
    for (int k = 0; k < count; ++k) out[k] = dev::ft_track_wrapped(word[k], wraps[k], last[k], first[k]);
}

// q0, q1 [count][4], a [count] -> q [count][4]
extern "C" void ftk_nlerp(int count, const float* q0, const float* q1, const float* a, float* q) {
    for (int k = 0; k < count; ++k) {
        const float x[4] = {q0[4 * k], q0[4 * k + 1], q0[4 * k + 2], q0[4 * k + 3]};
        const float y[4] = {q1[4 * k], q1[4 * k + 1], q1[4 * k + 2], q1[4 * k + 3]};
        float o[4];
        dev::ft_track_nlerp(x, y, a[k], o);
        for (int e = 0; e < 4; ++e) q[4 * k + e] = o[e];
    }
}

// rows, refs [count][13 + 2 n], qr [count][4], wj [n] -> e [count][5]
extern "C" void ftk_errors(int count, int n, const float* rows, const float* refs, const float* qr, const float* wj,
                           float ang_scale, float* e) {
    const int NS = 13 + 2 * n;
    for (int k = 0; k < count; ++k) {
        const float q[4] = {qr[4 * k], qr[4 * k + 1], qr[4 * k + 2], qr[4 * k + 3]};
        float o[kTrackTerms];
        dev::ft_track_errors(rows + k * NS, refs + k * NS, q, wj, n, ang_scale, o);
        for (int j = 0; j < kTrackTerms; ++j) e[kTrackTerms * k + j] = o[j];
    }
}

// weights, scales, bounds (max_pose, max_root_pos, max_root_rot); e [count][5],
// diverged [count], r_existing [count] -> term [count][5], reward [count], failed [count]
extern "C" void ftk_terms(int count, const float* weights, const float* scales, const float* bounds, const float* e,
                          const unsigned char* diverged, const float* r_existing, float* term, float* reward,
                          unsigned char* failed) {
    FloatTrackF K{};
    K.on = 1u;
    for (int j = 0; j < kTrackTerms; ++j) {
        K.weight[j] = weights[j];
        K.scale[j] = scales[j];
    }
    K.max_pose = bounds[0];
    K.max_root_pos = bounds[1];
    K.max_root_rot = bounds[2];
    for (int k = 0; k < count; ++k) {
        float x[kTrackTerms], o[kTrackTerms];
        for (int j = 0; j < kTrackTerms; ++j) x[j] = e[kTrackTerms * k + j];
        dev::ft_track_terms(K, x, diverged[k] != 0, o);
        for (int j = 0; j < kTrackTerms; ++j) term[kTrackTerms * k + j] = o[j];
        reward[k] = dev::ft_track_reward(r_existing[k], o);
        failed[k] = dev::ft_track_failed(K, x) ? 1 : 0;
    }
}
