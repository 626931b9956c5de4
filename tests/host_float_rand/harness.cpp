// Test-only host build of the push schedule of the floating-base env's
// randomisation (gym-ignition_amd/csrc/float_task.hpp: ft_push_phase,
// ft_push_active, ft_push_block): the integer arithmetic the post kernel runs
// per world, on the CPU, so tests/test_float_rand_host.py can compare it with
// a Python restatement without a GPU.  Not part of the product.
#define MW_HOST_TEST 1
#include "float_task.hpp"

using namespace mw;

extern "C" unsigned fr_episode_block() { return kFtEpisodeBlock; }
extern "C" unsigned fr_phase(unsigned r0, unsigned interval) { return dev::ft_push_phase(r0, interval); }

// steps t = 0 .. count - 1 of an episode with this phase: active[t] (0 / 1),
// k[t] (the push the step belongs to) and block[t] (its Philox block)
extern "C" void fr_schedule(unsigned count, unsigned phase, unsigned interval, unsigned push_steps,
                            unsigned char* active, unsigned* k, unsigned* block) {
    for (unsigned t = 0; t < count; ++t) {
        uint32_t kk = 0;
        active[t] = dev::ft_push_active(t, phase, interval, push_steps, kk) ? 1 : 0;
        k[t] = kk;
        block[t] = dev::ft_push_block(kk);
    }
}
