// world_params.cpp -- owner of a simulator's per-world wave-kernel parameters
// and their C ABI: the ground friction array (mw_sim::d_mu / h_mu) and the link
// parameter records (d_wpar / h_wpar / wpar_stride; layout: world_params.hpp).
#include "world_params.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "errors.hpp"
#include "sim_state.hpp"

using mw::fail;

// The per-world friction array, every world at the current coefficient (the
// float32 FloatF::mu holds): allocate, fill, then publish.
int alloc_ground_friction(mw_sim* s) {
    if (s->d_mu) return MW_OK;
    const size_t W = static_cast<size_t>(s->W);
    mw::dev_ptr<float[]> d;
    MW_HIP(mw::dev_alloc(d, W * sizeof(float)));
    s->h_mu.assign(W, static_cast<float>(s->ground_mu));
    MW_HIP(hipMemcpyAsync(d.get(), s->h_mu.data(), W * sizeof(float), hipMemcpyHostToDevice, s->stream));
    MW_HIP(hipStreamSynchronize(s->stream));  // h_mu is pageable and rewritten by the setters
    s->d_mu = std::move(d);
    return MW_OK;
}

// device -> host mirror of the friction array (an env's kernels wrote it)
int pull_ground_friction(mw_sim* s) {
    if (!s->d_mu) return MW_OK;
    MW_HIP(hipMemcpyAsync(s->h_mu.data(), s->d_mu.get(), static_cast<size_t>(s->W) * sizeof(float),
                          hipMemcpyDeviceToHost, s->stream));
    MW_HIP(hipStreamSynchronize(s->stream));
    return MW_OK;
}

// host mirror -> device, worlds [w0, w0 + nw)
static int upload_ground_friction(mw_sim* s, int32_t w0, int32_t nw) {
    if (nw <= 0) return MW_OK;
    MW_HIP(hipSetDevice(s->cfg.device));
    MW_HIP(hipMemcpyAsync(s->d_mu.get() + w0, s->h_mu.data() + w0, static_cast<size_t>(nw) * sizeof(float),
                          hipMemcpyHostToDevice, s->stream));
    MW_HIP(hipStreamSynchronize(s->stream));  // the pageable mirror may be rewritten at once
    return MW_OK;
}

// every world takes mu (mw_set_ground_plane); nothing to do before the array exists
int fill_ground_friction(mw_sim* s, double mu) {
    if (!s->d_mu) return MW_OK;
    std::fill(s->h_mu.begin(), s->h_mu.end(), static_cast<float>(mu));
    return upload_ground_friction(s, 0, s->W);
}

// Host setters of the per-world ground friction while an env randomises it
// fail, as those of the commands and pending resets do (check_not_env_owned) ...
int check_not_env_friction(const mw_sim* s, const char* what) {
    if (s && s->env_friction)
        return fail(MW_ESTATE, std::string(what) + ": a floating-base env with friction randomisation owns this "
                                                   "simulator's per-world ground friction (it lives on the "
                                                   "device); destroy the env first");
    return MW_OK;
}

// ... and those of the link parameter records while an env randomises inertias
// or joints; the message names the feature of the caller's own words
// (`joint_words`) where the env has both on.
static int check_not_env_wpar(const mw_sim* s, const char* what, bool joint_words) {
    if (!s->env_wpar()) return MW_OK;
    const bool joint = joint_words ? s->env_joints : !s->env_inertia;
    return fail(MW_ESTATE, std::string(what) + ": a floating-base env with " + (joint ? "joint" : "inertia") +
                               " randomisation owns this simulator's per-world link parameters (they live on "
                               "the device); destroy the env first");
}

static_assert(offsetof(mw::FloatF, Io) == 4 * sizeof(float) &&
                  offsetof(mw::FloatF, g) == mw::kWparInertialWords * sizeof(float),
              "FloatF starts with the base's ten inertial words");

// One world's record from the shared blocks: the base's ten inertial words,
// the ChainF header, n BodyF.
static void fill_link_record(const mw_sim* s, float* rec) {
    std::memset(rec, 0, mw::kWparBaseWords * sizeof(float));
    std::memcpy(rec, &s->h_float.mass, mw::kWparInertialWords * sizeof(float));
    std::memcpy(rec + mw::kWparBaseWords, &s->h_params, mw::chain_words(s->n) * sizeof(float));
}

// a world's record in the host mirror
static float* record(mw_sim* s, int32_t w) { return s->h_wpar.data() + static_cast<size_t>(w) * s->wpar_stride; }

// The per-world link parameters, every world at the model's nominal words:
// allocate and fill, then publish (a failed call leaves the simulator as it
// was).  The friction array comes with them: the kernel's per-world-parameter
// instances imply the per-world friction read.
int alloc_link_params(mw_sim* s) {
    if (s->d_wpar) return MW_OK;
    const int stride = mw::wpar_stride_words(s->n);
    const size_t W = static_cast<size_t>(s->W), words = W * stride;
    mw::dev_ptr<float[]> d;
    MW_HIP(mw::dev_alloc(d, words * sizeof(float)));
    std::vector<float> h(words);
    fill_link_record(s, h.data());
    for (size_t w = 1; w < W; ++w) std::memcpy(h.data() + w * stride, h.data(), stride * sizeof(float));
    MW_HIP(hipMemcpyAsync(d.get(), h.data(), words * sizeof(float), hipMemcpyHostToDevice, s->stream));
    MW_HIP(hipStreamSynchronize(s->stream));  // the mirror is pageable and rewritten by the setter
    if (int rc = alloc_ground_friction(s)) return rc;
    s->h_wpar = std::move(h);
    s->wpar_stride = stride;
    s->d_wpar = std::move(d);
    return MW_OK;
}

// device -> host mirror of the link parameter records (an env's kernels wrote them)
int pull_link_params(mw_sim* s) {
    if (!s->d_wpar) return MW_OK;
    MW_HIP(hipMemcpyAsync(s->h_wpar.data(), s->d_wpar.get(), s->h_wpar.size() * sizeof(float), hipMemcpyDeviceToHost,
                          s->stream));
    MW_HIP(hipStreamSynchronize(s->stream));
    return MW_OK;
}

// host mirror -> device, worlds [w0, w0 + nw)
static int upload_link_params(mw_sim* s, int32_t w0, int32_t nw) {
    if (nw <= 0) return MW_OK;
    const size_t stride = static_cast<size_t>(s->wpar_stride);
    MW_HIP(hipMemcpyAsync(s->d_wpar.get() + w0 * stride, s->h_wpar.data() + w0 * stride, nw * stride * sizeof(float),
                          hipMemcpyHostToDevice, s->stream));
    MW_HIP(hipStreamSynchronize(s->stream));  // the pageable mirror may be rewritten at once
    return MW_OK;
}

// The shared parameter blocks were rebuilt (upload_params): every world's
// record takes the new shared words and keeps its own -- the inertial words
// and the three joint dynamics words (damping, friction, effort).  A joint
// word that was never set per world is a copy of the shared one, so keeping it
// is taking the shared value; the one word a shared setter changed
// (mw_set_joint_param) is overwritten in every record: set_dof, set_word.
int refresh_link_params(mw_sim* s, int set_dof, int set_word) {
    if (!s->d_wpar) return MW_OK;
    if (s->env_wpar())
        if (int rc = pull_link_params(s)) return rc;
    std::vector<float> shared(s->wpar_stride), next;
    fill_link_record(s, shared.data());
    for (int32_t w = 0; w < s->W; ++w) {
        float* rec = record(s, w);
        next = shared;
        for (int l = -1; l < s->n; ++l)
            std::memcpy(&next[mw::wpar_inertial_word(l)], rec + mw::wpar_inertial_word(l),
                        mw::kWparInertialWords * sizeof(float));
        for (int d = 0; d < s->n; ++d)
            for (int word : mw::kBodyJointWord)
                if (!(d == set_dof && word == set_word))
                    next[mw::wpar_body_word(d) + word] = rec[mw::wpar_body_word(d) + word];
        std::memcpy(rec, next.data(), next.size() * sizeof(float));
    }
    return upload_link_params(s, 0, s->W);
}

// wpar_friction / wpar_damping, the instance choices that follow per-world joint words
int set_joint_dynamics_flags(mw_sim* s, bool friction, bool damping) {
    s->wpar_friction = friction;
    const bool changed = damping != s->wpar_damping;
    s->wpar_damping = damping;
    // FloatF::dual may follow: rebuild and upload the shared blocks (the records follow, words kept)
    return changed ? upload_params(s) : MW_OK;
}

extern "C" {

// Per-world friction coefficients of the ground plane (wave kernel): the
// float32 values the run kernel reads from mw_sim::d_mu, from the next run on.
int mw_set_ground_friction(mw_sim* s, int32_t w0, int32_t nw, const double* mu) {
    if (!s || !s->loaded) return fail(MW_ESTATE, "no model loaded");
    if (!s->initialized) return fail(MW_ESTATE, "the simulator is not initialized");
    if (!mu && nw > 0) return fail(MW_EINVAL, "null argument");
    if (w0 < 0 || nw < 0 || w0 + nw > s->W) return fail(MW_EINVAL, "world range out of bounds");
    if (!s->wave)
        return fail(MW_ESTATE, "per-world ground friction on mw_sim needs the world-per-wavefront kernel (articulated "
                               "floating bases, generic fixed-base trees); other models take one coefficient for "
                               "all worlds (mw_set_ground_plane) or per-world friction through a scene "
                               "(mw_scene_set_world_friction)");
    if (int own = check_not_env_friction(s, "mw_set_ground_friction")) return own;
    for (int32_t k = 0; k < nw; ++k)
        if (!(mu[k] >= 0.0)) return fail(MW_EINVAL, "the friction coefficient must be >= 0");
    MW_HIP(hipSetDevice(s->cfg.device));
    if (int rc = alloc_ground_friction(s)) return rc;
    for (int32_t k = 0; k < nw; ++k) s->h_mu[w0 + k] = static_cast<float>(mu[k]);
    return upload_ground_friction(s, w0, nw);
}

int mw_ground_friction(mw_sim* s, int32_t w0, int32_t nw, double* mu) {
    if (!s || !s->loaded) return fail(MW_ESTATE, "no model loaded");
    if (!s->initialized) return fail(MW_ESTATE, "the simulator is not initialized");
    if (!mu && nw > 0) return fail(MW_EINVAL, "null argument");
    if (w0 < 0 || nw < 0 || w0 + nw > s->W) return fail(MW_EINVAL, "world range out of bounds");
    if (s->env_friction) {  // the env's kernels write the array
        MW_HIP(hipSetDevice(s->cfg.device));
        if (int rc = pull_ground_friction(s)) return rc;
    }
    for (int32_t k = 0; k < nw; ++k) mu[k] = s->d_mu ? s->h_mu[w0 + k] : static_cast<float>(s->ground_mu);
    return MW_OK;
}

// Per-world inertial words of one link (wave kernel): the float32 words the
// run kernel reads from mw_sim::d_wpar, from the next run on.
static int check_link_params(const mw_sim* s, int32_t w0, int32_t nw, int32_t link, const void* params) {
    if (!s || !s->loaded) return fail(MW_ESTATE, "no model loaded");
    if (!s->initialized) return fail(MW_ESTATE, "the simulator is not initialized");
    if (!s->wave)
        return fail(MW_ESTATE, "per-world link parameters need the world-per-wavefront kernel (articulated floating "
                               "bases, mw_float_kernel == 2; generic fixed-base trees)");
    if (!params && nw > 0) return fail(MW_EINVAL, "null argument");
    if (w0 < 0 || nw < 0 || w0 + nw > s->W) return fail(MW_EINVAL, "world range out of bounds");
    if (link < -1 || link >= s->n)
        return fail(MW_EINVAL, "link " + std::to_string(link) + " out of range [-1, " + std::to_string(s->n) + ")");
    return MW_OK;
}

int mw_set_link_params(mw_sim* s, int32_t w0, int32_t nw, int32_t link, const float* params) {
    constexpr int kI = mw::kWparInertialWords;
    if (int rc = check_link_params(s, w0, nw, link, params)) return rc;
    if (int own = check_not_env_wpar(s, "mw_set_link_params", false)) return own;
    for (int32_t k = 0; k < nw; ++k) {
        const float* p = params + kI * static_cast<size_t>(k);
        for (int e = 0; e < kI; ++e)
            if (!std::isfinite(p[e])) return fail(MW_EINVAL, "the link parameters must be finite");
        if (!(p[0] > 0.f)) return fail(MW_EINVAL, "the link mass must be > 0");
    }
    MW_HIP(hipSetDevice(s->cfg.device));
    if (int rc = alloc_link_params(s)) return rc;
    for (int32_t k = 0; k < nw; ++k)
        std::memcpy(record(s, w0 + k) + mw::wpar_inertial_word(link), params + kI * static_cast<size_t>(k),
                    kI * sizeof(float));
    return upload_link_params(s, w0, nw);
}

int mw_link_params(mw_sim* s, int32_t w0, int32_t nw, int32_t link, float* params) {
    constexpr int kI = mw::kWparInertialWords;
    if (int rc = check_link_params(s, w0, nw, link, params)) return rc;
    if (s->env_wpar()) {  // the env's kernels write the records
        MW_HIP(hipSetDevice(s->cfg.device));
        if (int rc = pull_link_params(s)) return rc;
    }
    const float* nominal = link < 0 ? &s->h_float.mass : &s->h_params.b[link].mass;
    for (int32_t k = 0; k < nw; ++k)
        std::memcpy(params + kI * static_cast<size_t>(k),
                    s->d_wpar ? record(s, w0 + k) + mw::wpar_inertial_word(link) : nominal, kI * sizeof(float));
    return MW_OK;
}

// Per-world joint dynamics of one dof (wave kernel): damping, friction and
// effort (kBodyJointWord) of the dof's BodyF in the same records.
static int check_joint_dynamics(const mw_sim* s, int32_t w0, int32_t nw, int32_t dof, const void* params) {
    if (int rc = check_link_params(s, w0, nw, 0, params)) return rc;
    if (dof < 0 || dof >= s->n)
        return fail(MW_EINVAL, "dof " + std::to_string(dof) + " out of range [0, " + std::to_string(s->n) + ")");
    return MW_OK;
}

int mw_set_joint_dynamics(mw_sim* s, int32_t w0, int32_t nw, int32_t dof, const float* params) {
    if (int rc = check_joint_dynamics(s, w0, nw, dof, params)) return rc;
    if (int own = check_not_env_wpar(s, "mw_set_joint_dynamics", true)) return own;
    bool friction = false, damping = false;
    for (int32_t k = 0; k < nw; ++k) {
        const float* p = params + 3 * static_cast<size_t>(k);
        for (int e = 0; e < 3; ++e)
            if (!std::isfinite(p[e])) return fail(MW_EINVAL, "the joint dynamics words must be finite");
        if (!(p[0] >= 0.f)) return fail(MW_EINVAL, "the joint damping must be >= 0");
        if (!(p[1] >= 0.f)) return fail(MW_EINVAL, "the joint friction must be >= 0");
        if (!(p[2] > 0.f)) return fail(MW_EINVAL, "the joint effort limit must be > 0 (FLT_MAX: unbounded)");
        damping = damping || p[0] != 0.f;
        friction = friction || p[1] != 0.f;
    }
    MW_HIP(hipSetDevice(s->cfg.device));
    if (int rc = alloc_link_params(s)) return rc;
    for (int32_t k = 0; k < nw; ++k) {
        float* b = record(s, w0 + k) + mw::wpar_body_word(dof);
        for (int e = 0; e < 3; ++e) b[mw::kBodyJointWord[e]] = params[3 * static_cast<size_t>(k) + e];
    }
    if (int rc = upload_link_params(s, w0, nw)) return rc;
    return set_joint_dynamics_flags(s, s->wpar_friction || friction, s->wpar_damping || damping);
}

int mw_joint_dynamics(mw_sim* s, int32_t w0, int32_t nw, int32_t dof, float* params) {
    if (int rc = check_joint_dynamics(s, w0, nw, dof, params)) return rc;
    if (s->env_wpar()) {  // the env's kernels write the records
        MW_HIP(hipSetDevice(s->cfg.device));
        if (int rc = pull_link_params(s)) return rc;
    }
    const mw::BodyF& b0 = s->h_params.b[dof];
    const float nominal[3] = {b0.damping, b0.friction, b0.effort};
    for (int32_t k = 0; k < nw; ++k)
        for (int e = 0; e < 3; ++e)
            params[3 * static_cast<size_t>(k) + e] =
                s->d_wpar ? record(s, w0 + k)[mw::wpar_body_word(dof) + mw::kBodyJointWord[e]] : nominal[e];
    return MW_OK;
}

}  // extern "C"
