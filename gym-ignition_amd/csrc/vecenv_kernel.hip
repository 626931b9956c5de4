// vecenv_kernel.hip -- the device-side gym env of the lane-per-world models.
//
//  vecenv_step    : one gym step of every world with the Task logic of
//                   python/gym_ignition_environments/tasks/*.py fused in
//                   (obs, reward, done, TimeLimit, auto-reset).
//  vecenv_reset   : initial reset of every world (Philox4x32-10).
//
// A translation unit of its own because the Makefile builds it with
// -amdgpu-kernarg-preload-count: the step kernel's leading arguments (state
// pointers, action pointer, W, dt, substeps, pgs_iters) arrive in SGPRs, so its first
// global loads wait on no kernarg round trip.  The step kernel
// therefore takes flat arguments and one compact by-value block (VecArgs)
// instead of the TaskF / SimDev / VecDev structs.
#include <cstdlib>
#include <type_traits>

#include "baked_models.hpp"
#include "chain_dyn.hpp"
#include "kernels.hpp"
#include "rng.hpp"

namespace mw {
namespace dev {

// The shipped models' parameter blocks as device constants (kernels.hip has
// the Panda's): a kernel instantiated with BAKED != 0 reads the model from
// here and the compiler folds its zeros and ones.
__constant__ constexpr baked::CartpoleBlock kCartpoleDev = {{MW_BAKED_CARTPOLE_INIT}};
__constant__ constexpr baked::PendulumBlock kPendulumDev = {{MW_BAKED_PENDULUM_INIT}};

template <int BAKED>
__device__ __forceinline__ const ChainF* model_params(const ChainF* P) {
    if constexpr (BAKED == baked::kCartpoleId) return reinterpret_cast<const ChainF*>(&kCartpoleDev);
    else if constexpr (BAKED == baked::kPendulumId) return reinterpret_cast<const ChainF*>(&kPendulumDev);
    else return P;
}

// ------------------------------------------------------ kernel arguments ----
// What the step kernel needs after the physics, as one kernarg block that it
// reads in a single early batch.  The task functions below take it (or the
// host's TaskF, in the reset kernel) as their task description T.
struct VecTail {
    float* obs;
    float* reward;
    uint8_t* done;
    float* term_obs;
    int32_t T_steps;
    int32_t max_steps;
    int32_t reward_cart_at_center;
    uint32_t seed_lo, seed_hi;
    uint32_t world_offset;
    float force_mag;
    float x_factor;
    float hi[4];
};
// the randomised tasks' additions (TaskF / VecDev fields of the same names)
struct VecTailRand : VecTail {
    int32_t randomize;
    float mass_lo, mass_hi;
    float g_mean, g_std;
    float gdir[3];
    float* rmass;
    float* rgz;
};
// the generic (not constant-folded) kernels also carry the model block
template <bool RAND, bool GENERIC>
struct VecArgs : std::conditional_t<RAND, VecTailRand, VecTail> {};
template <bool RAND>
struct VecArgs<RAND, true> : std::conditional_t<RAND, VecTailRand, VecTail> {
    const ChainF* P;
};
static_assert(sizeof(VecArgs<true, true>) <= 136, "the step kernel's kernargs stay within 192 bytes");

// Makes the compiler fetch every word of a kernarg block where this is
// called, and hold it in SGPRs, instead of sinking the scalar loads to the
// fields' first uses (after the physics, in front of the stores).
template <class A>
__device__ __forceinline__ void fetch_now(const A& a) {
    static_assert(sizeof(A) % 4 == 0);
    uint32_t v[sizeof(A) / 4];
    __builtin_memcpy(v, &a, sizeof(A));
#pragma unroll
    for (unsigned k = 0; k < sizeof(A) / 4; ++k) asm volatile("" ::"s"(v[k]));
}

constexpr float kPi = 3.14159265358979323846f;

// ----------------------------------------------------------- tasks ------
// kinds: 0 CartPoleDiscreteBalancing, 1 CartPoleContinuousBalancing,
//        2 CartPoleContinuousSwingup, 3 PendulumSwingUp
// FOLD (the helper wave's draw): rng.hpp's unif_folded, the same bits.
template <int N, int KIND, bool FOLD = false, class TT>
__device__ __forceinline__ void task_reset(const TT& T, uint32_t w, uint32_t episode,
                                           float (&q)[N], float (&qd)[N]) {
    uint32_t r[4];
    philox(T.seed_lo, T.seed_hi, w, episode, r);
    const auto unif = [](uint32_t x, float lo, float hi) {
        if constexpr (FOLD) return unif_folded(x, lo, hi);
        else return dev::unif(x, lo, hi);
    };
    if constexpr (KIND == 0 || KIND == 1) {
        // x, dx, q, dq = U(-0.05, 0.05)   cartpole_discrete_balancing.py:137
        q[0] = unif(r[0], -0.05f, 0.05f); qd[0] = unif(r[1], -0.05f, 0.05f);
        q[1] = unif(r[2], -0.05f, 0.05f); qd[1] = unif(r[3], -0.05f, 0.05f);
    } else if constexpr (KIND == 2) {
        // q = pi - deg2rad(U(-60, 60)); x, dx, dq = U(-0.05, 0.05)  cartpole_continuous_swingup.py:145-146
        q[1] = kPi - unif(r[0], -60.f, 60.f) * (kPi / 180.f);
        q[0] = unif(r[1], -0.05f, 0.05f); qd[0] = unif(r[2], -0.05f, 0.05f);
        qd[1] = unif(r[3], -0.05f, 0.05f);
    } else {
        // cos, sin, dq = observation_space.sample(); q = atan2(sin, cos)  pendulum_swingup.py:117-127
        const float c = unif(r[0], -1.f, 1.f), s = unif(r[1], -1.f, 1.f);
        q[0] = atan2f(s, c);
        qd[0] = unif(r[2], -10.f, 10.f);
    }
}

template <int N, int KIND>
__device__ __forceinline__ void task_obs(const float (&q)[N], const float (&qd)[N], float (&o)[4]) {
    if constexpr (KIND == 3) {
        float s, c;
        sincosf(q[0], &s, &c);
        o[0] = c; o[1] = s; o[2] = qd[0]; o[3] = 0.f;
    } else {
        o[0] = q[0]; o[1] = qd[0]; o[2] = q[1]; o[3] = qd[1];   // [x, dx, q, dq]
    }
}

// ABS (the HELP kernels): |o| <= hi in place of -hi <= o <= hi, half the
// compares.  The same boolean for every finite o and either sign of hi
// (hi < 0: both say "outside"); the kernels are built finite-math-only.
template <int KIND, bool ABS = false, class TT>
__device__ __forceinline__ bool task_done(const TT& T, const float (&o)[4]) {
    constexpr int no = (KIND == 3) ? 3 : 4;
    // every comparison evaluated, combined bitwise: the same boolean as the
    // short-circuit form without its nested exec-mask branches
    bool inside = true;
#pragma unroll
    for (int k = 0; k < no; ++k) {
        if constexpr (ABS) inside = inside & (fabsf(o[k]) <= T.hi[k]);
        else inside = inside & (o[k] >= -T.hi[k]) & (o[k] <= T.hi[k]);
    }
    return !inside;
}

template <int N, int KIND, class TT>
__device__ __forceinline__ float task_reward(const TT& T, const float (&q)[N], const float (&qd)[N],
                                             const float (&o)[4], bool done) {
    // no FMA contraction: the reward is bit-identical in the per-step and the
    // fused-rollout kernels (contraction would otherwise depend on context)
#pragma clang fp contract(off)
    if constexpr (KIND == 0 || KIND == 1) {
        float r = done ? 0.f : 1.f;
        if (T.reward_cart_at_center)
            r = r - 0.10f * fabsf(o[0]) - 0.10f * fabsf(o[1]) -
                10.0f * (o[0] >= T.x_factor * 2.4f ? 1.f : 0.f);
        return r;
    } else if constexpr (KIND == 2) {
        return (cosf(q[1]) + 1.f) * 0.5f - 0.1f * qd[0] * qd[0] -
               10.0f * (q[0] >= T.x_factor * 2.4f ? 1.f : 0.f);
    } else {
        // the force target read after the run is the zero-filled JointForceCmd
        // (Physics.cpp:2250-2254), so the 0.001 tau^2 term of
        // pendulum_swingup.py:86-88 is identically zero
        const float cost = (done ? 100.f : 0.f) + q[0] * q[0] + 0.1f * qd[0] * qd[0];
        return -cost;
    }
}

// Per-world physics sample of (world, episode): masses from Philox blocks
// 1.., gravity from block 8 by Box-Muller (SDFRandomizer.sample,
// randomizers/model/sdf.py:264-315: force_positive clips the SAMPLE at 0, so
// an additive mass change is max(U(lo, hi), 0); cartpole.py:51-56 gravity).
template <int N, class TT>
__device__ __forceinline__ Dyn<N> sample_dyn(const ChainF* __restrict__ P, const TT& T, uint32_t w,
                                             uint32_t episode, float& gz_out) {
    Dyn<N> D = nominal_dyn<N>(P);
    gz_out = 0.f;
    if (T.randomize & kRandMass) {
#pragma unroll
        for (int b = 0; b < (N + 3) / 4; ++b) {
            uint32_t r[4];
            philox(T.seed_lo, T.seed_hi, w, episode, r, 1u + static_cast<uint32_t>(b));
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * b + k < N) D.m[4 * b + k] += fmaxf(unif(r[k], T.mass_lo, T.mass_hi), 0.f);
        }
    }
    if (T.randomize & kRandGravity) {
        uint32_t r[4];
        philox(T.seed_lo, T.seed_hi, w, episode, r, 8u);
        const float u1 = static_cast<float>((r[0] >> 8) + 1u) * (1.f / 16777216.f);  // (0, 1]
        const float u2 = static_cast<float>(r[1] >> 8) * (1.f / 16777216.f);
        const float z = sqrtf(-2.f * logf(u1)) * cosf(2.f * kPi * u2);
        const float gz = T.g_mean + T.g_std * z;
        D.g = {gz * T.gdir[0], gz * T.gdir[1], gz * T.gdir[2]};
        gz_out = gz;
    }
    return D;
}

// V: whatever holds the rmass / rgz arrays (VecDev, or the step kernel's block)
template <int N, class TT, class VV>
__device__ __forceinline__ Dyn<N> load_dyn(const ChainF* __restrict__ P, const TT& T, const VV& V, int W, int w) {
    Dyn<N> D = nominal_dyn<N>(P);
    if (T.randomize & kRandMass) {
#pragma unroll
        for (int d = 0; d < N; ++d) D.m[d] = V.rmass[d * W + w];
    }
    if (T.randomize & kRandGravity) {
        const float gz = V.rgz[w];
        D.g = {gz * T.gdir[0], gz * T.gdir[1], gz * T.gdir[2]};
    }
    return D;
}

template <int N, class TT, class VV>
__device__ __forceinline__ void store_dyn(const TT& T, const VV& V, int W, int w, const Dyn<N>& D, float gz) {
    if (T.randomize & kRandMass) {
#pragma unroll
        for (int d = 0; d < N; ++d) V.rmass[d * W + w] = D.m[d];
    }
    if (T.randomize & kRandGravity) V.rgz[w] = gz;
}

// Element i of a uniform array.  OFF32 (the HELP kernels, W <= 16384 worlds):
// one unsigned 32-bit byte offset added to the uniform pointer, which the
// compiler emits as the scalar-base form `global_load_dword v, v_off, s[b:b+1]`
// with no 64-bit vector address arithmetic.  A row d > 0 goes into i (d * W
// + w), never into the pointer.  Otherwise the plain index, as written.
template <bool OFF32, class E, class I>
__device__ __forceinline__ E* elem(E* base, I i) {
    if constexpr (OFF32) {
        using Byte = std::conditional_t<std::is_const_v<E>, const char, char>;
        return reinterpret_cast<E*>(reinterpret_cast<Byte*>(base) +
                                    static_cast<uint32_t>(i) * static_cast<uint32_t>(sizeof(E)));
    } else {
        return base + i;
    }
}

// The world index as a value of the basic block that calls this.  The
// compiler otherwise reuses the 64-bit addresses of the loads at the top for
// the stores of another block, and builds them with vector 64-bit adds; an
// offset computed in the store's own block folds into the scalar-base form.
// Emits no instruction.
__device__ __forceinline__ int own_block(int w) {
    asm volatile("" : "+v"(w));
    return w;
}

template <int N, bool OFF32 = false>
__device__ __forceinline__ void store_state(float* __restrict__ sq, float* __restrict__ sqd, int W, int w,
                                            const float (&q)[N], const float (&qd)[N]) {
#pragma unroll
    for (int d = 0; d < N; ++d) {
        *elem<OFF32>(sq, d * W + w) = q[d];
        *elem<OFF32>(sqd, d * W + w) = qd[d];
    }
}

template <int NO>
__device__ __forceinline__ void store_obs(float* __restrict__ dst, const float (&o)[4]) {
    if constexpr (NO == 4) {
        *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int k = 0; k < NO; ++k) dst[k] = o[k];
    }
}

// ---------------------------------------------------------- kernels -----

template <int N, int KIND>
__global__ void __launch_bounds__(256) vecenv_reset_kernel(const ChainF* __restrict__ P, TaskF T, SimDev S,
                                                           VecDev V, float* __restrict__ obs, int W) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= W) return;
    float q[N], qd[N], o[4];
    if (T.randomize) {
        const uint32_t gw = T.world_offset + static_cast<uint32_t>(w);
        float gz;
        const Dyn<N> D = sample_dyn<N>(P, T, gw, 0u, gz);
        store_dyn<N>(T, V, W, w, D, gz);
    }
    task_reset<N, KIND>(T, T.world_offset + static_cast<uint32_t>(w), 0u, q, qd);
    task_obs<N, KIND>(q, qd, o);
    constexpr int NO = (KIND == 3) ? 3 : 4;
    store_obs<NO>(obs + static_cast<size_t>(w) * NO, o);
    store_state<N>(S.q, S.qd, W, w, q, qd);
    V.episode[w] = 0u;
    V.steps[w] = 0u;
}

// ROLLOUT: loop over A.T_steps with [t, w] layouts; otherwise a single step.
// B: the worlds of one workgroup.  The 14 leading argument dwords are
// preloaded into SGPRs; A is fetched while the state loads are in flight.
//
// HELP: the workgroup has 2 * B threads (B == 64, two waves).  Wave 0 is the
// kernel of worlds blockIdx.x * B + lane.  Wave 1, the helper, draws the same
// worlds' next reset state (it depends on seed, world and episode only, not
// on the physics) while wave 0 runs the physics, and leaves it in LDS; the
// two meet at one workgroup barrier after wave 0 knows `done` and before its
// first store, and a done lane reads its reset state from LDS instead of
// running Philox behind the physics.  Every thread reaches the barrier: there
// is no early return, lanes past W work on world W - 1 and store nothing.
// The HELP kernels address every array by a 32-bit byte offset (elem above);
// they run at W <= kHelpMaxWorlds.
//
// ONE (HELP kernels only): the engine substep as straight-line code for
// substeps == 1, chosen by the launcher; `substeps` is then not read.  The
// same arithmetic as one trip of the loop, without the loop's phi copies,
// counter and force select, and with the limit rows' setup inside their branch.
constexpr int kHelpMaxWorlds = 64 * 256;
template <int N, int KIND, bool DUAL, bool CONS, bool ROLLOUT, int BAKED, bool RAND, int B, bool HELP = false,
          bool ONE = false>
__global__ void __launch_bounds__(256) vecenv_step_kernel(float* __restrict__ sq, float* __restrict__ sqd,
                                                          uint32_t* __restrict__ ep, uint32_t* __restrict__ st,
                                                          const void* __restrict__ actions, int W, float dt,
                                                          int substeps, int pgs_iters,
                                                          VecArgs<RAND, BAKED == 0> A) {
    static_assert(!HELP || (B == 64 && !ROLLOUT && !RAND), "the helper wave serves the closed-loop 64-world blocks");
    static_assert(!ONE || HELP, "the single-substep form exists for the helper-wave kernels");
    // the largest byte offset of a HELP kernel: a float4 row of obs / term_obs
    static_assert(static_cast<uint64_t>(kHelpMaxWorlds) * (N > 4 ? N : 4) * sizeof(float) < (1ull << 32),
                  "32-bit byte offsets cover every array of the HELP kernels");
    __shared__ float reset_lds[HELP ? 2 * N * B : 1];   // [component][lane]
    const int lane = HELP ? static_cast<int>(threadIdx.x) & (B - 1) : static_cast<int>(threadIdx.x);
    int w = blockIdx.x * B + lane;
    bool live = true;
    if constexpr (HELP) {
        live = w < W;
        w = live ? w : W - 1;
    } else {
        if (w >= W) return;
    }
    constexpr int NO = (KIND == 3) ? 3 : 4;
    using ActT = std::conditional_t<KIND == 0, int32_t, float>;
    float q[N], qd[N];
#pragma unroll
    for (int d = 0; d < N; ++d) {
        q[d] = *elem<HELP>(sq, d * W + w);
        qd[d] = *elem<HELP>(sqd, d * W + w);
    }
    const uint32_t episode0 = *elem<HELP>(ep, w);
    uint32_t episode = episode0;
    uint32_t steps = *elem<HELP>(st, w);
    ActT a0 = ActT(0);
    if constexpr (!ROLLOUT) a0 = *elem<HELP>(static_cast<const ActT*>(actions), w);
    fetch_now(A);
    float* __restrict__ obs = A.obs;
    float* __restrict__ reward = A.reward;
    uint8_t* __restrict__ done_out = A.done;
    float* __restrict__ term_obs = A.term_obs;
    const ChainF* __restrict__ P;
    if constexpr (BAKED == 0) P = A.P;
    else P = model_params<BAKED>(nullptr);
    uint8_t act[N];
    float vc[N];
#pragma unroll
    for (int d = 0; d < N; ++d) { act[d] = kActForce; vc[d] = 0.f; }
    Dyn<N> D;
    if constexpr (RAND) D = load_dyn<N>(P, A, A, W, w);
    if constexpr (HELP) {
        // the role is wave-uniform and chosen after the shared prologue
        // (addresses, loads, A): the loads above still issue from the first
        // instructions with no scalar wait in front of them
        if (__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x)) >= B) {
            float rq[N], rqd[N];
            task_reset<N, KIND, true>(A, A.world_offset + static_cast<uint32_t>(w), episode0 + 1u, rq, rqd);
#pragma unroll
            for (int d = 0; d < N; ++d) {
                reset_lds[d * B + lane] = rq[d];
                reset_lds[(N + d) * B + lane] = rqd[d];
            }
            __syncthreads();
            // a use of the state loads on this side too: they stay in the
            // shared prologue, ahead of the wait for A, instead of sinking
            // into wave 0's branch.  Behind the barrier they landed long ago.
#pragma unroll
            for (int d = 0; d < N; ++d) asm volatile("" ::"v"(q[d]), "v"(qd[d]));
            asm volatile("" ::"v"(steps), "v"(a0));
            return;
        }
    }
    int ws = w;   // HELP: the world index of the final stores' block (own_block)
    const int nsteps = ROLLOUT ? A.T_steps : 1;
    for (int t = 0; t < nsteps; ++t) {
        const size_t idx = static_cast<size_t>(t) * W + w;
        ActT a = a0;
        if constexpr (ROLLOUT) a = static_cast<const ActT*>(actions)[idx];
        float force;
        if constexpr (KIND == 0) {
            force = (a == 1) ? A.force_mag : -A.force_mag;   // cartpole_discrete_balancing.py:70
        } else {
            force = a;
        }
        // the driven joint ("linear" / "pivot") is dof 0; other joints are Idle
        const float e = P->b[0].effort;
        force = fminf(fmaxf(force, -e), e);
        float tau[N], qdd[N];
        if constexpr (ONE) {
#pragma unroll
            for (int d = 0; d < N; ++d) tau[d] = 0.f;
            tau[0] = force;
            substep<N, DUAL, CONS>(P, q, qd, tau, act, vc, dt, pgs_iters, qdd);
        } else {
            for (int s = 0; s < substeps; ++s) {
#pragma unroll
                for (int d = 0; d < N; ++d) tau[d] = 0.f;
                tau[0] = (s == 0) ? force : 0.f;
                if constexpr (RAND) substep_dyn<N, DUAL, CONS>(P, q, qd, tau, act, vc, dt, pgs_iters, qdd, D);
                else substep<N, DUAL, CONS>(P, q, qd, tau, act, vc, dt, pgs_iters, qdd);
            }
        }
        // an unconditional use of the action: its load stays with the state
        // loads above instead of sinking under the `substeps > 0` branch,
        // behind the wait for A.  It stands ahead of the first store: after
        // the stores it would make them wait for each other (the use needs a
        // vmcnt wait, and by then the counter holds stores only).
        if constexpr (!ROLLOUT) asm volatile("" ::"v"(a0));
        float o[4];
        task_obs<N, KIND>(q, qd, o);
        const bool tdone = task_done<KIND, HELP>(A, o);
        const float rew = task_reward<N, KIND>(A, q, qd, o, tdone);
        if constexpr (!HELP) reward[idx] = rew;
        steps += 1u;
        const bool d_ = tdone || (A.max_steps > 0 && steps >= static_cast<uint32_t>(A.max_steps));
        if constexpr (HELP) {
            // the helper's reset state is in LDS behind this barrier; no
            // store has been issued yet, so the barrier waits on LDS only
            __syncthreads();
            if (!live) return;
            *elem<HELP>(reward, idx) = rew;
        }
        if constexpr (HELP) *elem<true>(done_out, idx) = d_ ? 1 : 0;
        else done_out[idx] = d_ ? 1 : 0;
        if (d_) {
            if constexpr (HELP) store_obs<NO>(elem<true>(term_obs, own_block(w) * NO), o);
            else store_obs<NO>(term_obs + idx * NO, o);
            episode += 1u;
            steps = 0u;
            if constexpr (RAND) {
                // GazeboEnvRandomizer.reset: new physics and model sample per episode
                float gz;
                D = sample_dyn<N>(P, A, A.world_offset + static_cast<uint32_t>(w), episode, gz);
                store_dyn<N>(A, A, W, w, D, gz);
            }
            if constexpr (HELP) {
#pragma unroll
                for (int d = 0; d < N; ++d) {
                    q[d] = reset_lds[d * B + lane];
                    qd[d] = reset_lds[(N + d) * B + lane];
                }
            } else {
                task_reset<N, KIND>(A, A.world_offset + static_cast<uint32_t>(w), episode, q, qd);
            }
            task_obs<N, KIND>(q, qd, o);
        }
        if constexpr (HELP) {
            ws = own_block(w);
            store_obs<NO>(elem<true>(obs, ws * NO), o);
        } else {
            store_obs<NO>(obs + idx * NO, o);
        }
    }
    store_state<N, HELP>(sq, sqd, W, ws, q, qd);
    if constexpr (HELP) {
        // the unconditional stores in one block; the rare one behind them
        *elem<true>(st, ws) = steps;
        if (episode != episode0) *elem<true>(ep, own_block(ws)) = episode;   // changes only on auto-reset
    } else {
        if (episode != episode0) ep[w] = episode;  // changes only on auto-reset
        st[w] = steps;
    }
}

}  // namespace dev

// ------------------------------------------------------- launchers ------
namespace {

dim3 grid_for(int W, int block) { return dim3(static_cast<unsigned>((W + block - 1) / block)); }

// 64-thread blocks spread a small world count over as many CUs as possible
// (each wave runs a long dependent chain); 256 once there is work for all.
int block_for(int W) { return (W <= dev::kHelpMaxWorlds) ? 64 : 256; }

// MWSTEP_FORCE_SUBSTEP_LOOP=1 keeps the loop instantiation at substeps == 1
// (the A/B and the bit-equality test of the single-substep kernels).
bool substep_loop_forced() {
    const char* v = std::getenv("MWSTEP_FORCE_SUBSTEP_LOOP");
    return v && *v && *v != '0';
}

struct StepCall {
    const ChainF* P;
    const TaskF& T;
    const SimDev& S;
    const VecDev& V;
    const void* a;
    float *o, *r;
    uint8_t* d;
    float* to;
    int W;
    float dt;
    int substeps, pgs, Ts;
    hipStream_t st;
};

template <bool RAND, bool GENERIC>
dev::VecArgs<RAND, GENERIC> step_args(const StepCall& c) {
    dev::VecArgs<RAND, GENERIC> A;
    const TaskF& T = c.T;
    A.obs = c.o; A.reward = c.r; A.done = c.d; A.term_obs = c.to;
    A.T_steps = c.Ts;
    A.max_steps = T.max_steps;
    A.reward_cart_at_center = T.reward_cart_at_center;
    A.seed_lo = T.seed_lo; A.seed_hi = T.seed_hi;
    A.world_offset = T.world_offset;
    A.force_mag = T.force_mag;
    A.x_factor = T.x_factor;
    for (int k = 0; k < 4; ++k) A.hi[k] = T.hi[k];
    if constexpr (RAND) {
        A.randomize = T.randomize;
        A.mass_lo = T.mass_lo; A.mass_hi = T.mass_hi;
        A.g_mean = T.g_mean; A.g_std = T.g_std;
        for (int k = 0; k < 3; ++k) A.gdir[k] = T.gdir[k];
        A.rmass = c.V.rmass; A.rgz = c.V.rgz;
    }
    if constexpr (GENERIC) A.P = c.P;
    return A;
}

template <int N, int KIND, bool DUAL, bool CONS, bool ROLLOUT, int BAKED, bool RAND>
hipError_t vec_launch(const StepCall& c) {
    const auto A = step_args<RAND, BAKED == 0>(c);
    const int W = c.W;
    // the closed-loop 64-world blocks run with a helper wave (the kernel's
    // HELP); the rollout, the randomised physics (its sample_dyn stays
    // inline) and the 256-thread path, where doubled waves would cost
    // throughput, keep the inline reset
    constexpr bool HELP = !ROLLOUT && !RAND;
    if (HELP && block_for(W) == 64 && c.substeps == 1 && !substep_loop_forced())
        // one substep: the straight-line instantiation (the kernel's ONE)
        hipLaunchKernelGGL((dev::vecenv_step_kernel<N, KIND, DUAL, CONS, ROLLOUT, BAKED, RAND, 64, HELP, HELP>),
                           grid_for(W, 64), dim3(128), 0, c.st, c.S.q, c.S.qd, c.V.episode, c.V.steps, c.a, W, c.dt,
                           c.substeps, c.pgs, A);
    else if (block_for(W) == 64)
        hipLaunchKernelGGL((dev::vecenv_step_kernel<N, KIND, DUAL, CONS, ROLLOUT, BAKED, RAND, 64, HELP>),
                           grid_for(W, 64), dim3(HELP ? 128 : 64), 0, c.st, c.S.q, c.S.qd, c.V.episode, c.V.steps, c.a,
                           W, c.dt, c.substeps, c.pgs, A);
    else
        hipLaunchKernelGGL((dev::vecenv_step_kernel<N, KIND, DUAL, CONS, ROLLOUT, BAKED, RAND, 256>), grid_for(W, 256),
                           dim3(256), 0, c.st, c.S.q, c.S.qd, c.V.episode, c.V.steps, c.a, W, c.dt, c.substeps, c.pgs,
                           A);
    return hipGetLastError();
}

template <int N, int KIND, bool ROLLOUT, bool RAND>
hipError_t vec_nk(bool cons, bool dual, int baked, const StepCall& c) {
    // constant-folded instantiations for the shipped models (their flags fix cons/dual)
    if constexpr (N == 2 && KIND <= 2) {
        if (baked == baked::kCartpoleId && cons && !dual)
            return vec_launch<N, KIND, false, true, ROLLOUT, baked::kCartpoleId, RAND>(c);
    }
    if constexpr (N == 1 && KIND == 3) {
        if (baked == baked::kPendulumId && !cons)
            return vec_launch<N, KIND, false, false, ROLLOUT, baked::kPendulumId, RAND>(c);
    }
    if (!cons) return vec_launch<N, KIND, false, false, ROLLOUT, 0, RAND>(c);
    if (!dual) return vec_launch<N, KIND, false, true, ROLLOUT, 0, RAND>(c);
    return vec_launch<N, KIND, true, true, ROLLOUT, 0, RAND>(c);
}

}  // namespace

hipError_t launch_vecenv_reset(const ChainF* P, int n, const TaskF& T, const SimDev& S,
                               const VecDev& V, float* obs, int W, hipStream_t st) {
    if (T.kind == 4) return launch_vecenv_pid_reset(P, n, T, S, V, obs, W, st);
    const int B = block_for(W);
    if (T.kind == 3 && n == 1)
        hipLaunchKernelGGL((dev::vecenv_reset_kernel<1, 3>), grid_for(W, B), dim3(B), 0, st, P, T, S, V, obs, W);
    else if (T.kind == 0 && n == 2)
        hipLaunchKernelGGL((dev::vecenv_reset_kernel<2, 0>), grid_for(W, B), dim3(B), 0, st, P, T, S, V, obs, W);
    else if (T.kind == 1 && n == 2)
        hipLaunchKernelGGL((dev::vecenv_reset_kernel<2, 1>), grid_for(W, B), dim3(B), 0, st, P, T, S, V, obs, W);
    else if (T.kind == 2 && n == 2)
        hipLaunchKernelGGL((dev::vecenv_reset_kernel<2, 2>), grid_for(W, B), dim3(B), 0, st, P, T, S, V, obs, W);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_vecenv_step(const ChainF* P, int n, bool cons, bool dual, int baked, const TaskF& T,
                              const SimDev& S, const VecDev& V, const void* actions, float* obs,
                              float* reward, uint8_t* done, float* term_obs, int W, float dt,
                              int substeps, int pgs_iters, int T_steps, hipStream_t st) {
    const StepCall c{P, T, S, V, actions, obs, reward, done, term_obs, W, dt, substeps, pgs_iters,
                     T_steps > 0 ? T_steps : 1, st};
#define MW_VEC_R(NN, KK, RR) \
    return (T_steps > 0) ? vec_nk<NN, KK, true, RR>(cons, dual, baked, c) : vec_nk<NN, KK, false, RR>(cons, dual, baked, c)
#define MW_VEC(NN, KK)              \
    if (T.randomize) MW_VEC_R(NN, KK, true); \
    MW_VEC_R(NN, KK, false)
    if (T.kind == 3 && n == 1) { MW_VEC(1, 3); }
    if (T.kind == 0 && n == 2) { MW_VEC(2, 0); }
    if (T.kind == 1 && n == 2) { MW_VEC(2, 1); }
    if (T.kind == 2 && n == 2) { MW_VEC(2, 2); }
#undef MW_VEC
#undef MW_VEC_R
    return hipErrorInvalidValue;
}

}  // namespace mw
