// Test-only host build of the arithmetic of the observation noise and the
// action latency (gym-ignition_amd/csrc/float_task.hpp: ft_noise_unit,
// ft_noisy, ft_delay_draw, ft_delay_neutral, ft_delay_slot): what the env
// kernels run per word and per world, on the CPU in float32, so
// tests/test_float_noise_host.py can compare it with numpy fp64 and a
// brute-force ring without a GPU.  Not part of the product.
#define MW_HOST_TEST 1
#include "float_task.hpp"

using namespace mw;

extern "C" int fn_max_delay() { return kMaxActionDelay; }

extern "C" void fn_noise_unit(int count, const unsigned* x, float* u) {
    for (int i = 0; i < count; ++i) u[i] = dev::ft_noise_unit(x[i]);
}

extern "C" void fn_noisy(int count, const float* clean, const float* amp, const float* u, float* out) {
    for (int i = 0; i < count; ++i) out[i] = dev::ft_noisy(clean[i], amp[i], u[i]);
}

extern "C" unsigned fn_delay_draw(unsigned r2, unsigned lo, unsigned hi) { return dev::ft_delay_draw(r2, lo, hi); }

// steps 0 .. steps - 1 of one episode with delay d on a ring of R rows: the slot
// every step stores its action in, whether it applies the neutral command, and
// the slot it applies otherwise (-1 where neutral: the kernel reads none)
extern "C" void fn_ring(int steps, unsigned d, unsigned R, int* stored, int* applied, unsigned char* neutral) {
    for (int t = 0; t < steps; ++t) {
        const uint32_t ut = static_cast<uint32_t>(t);
        stored[t] = static_cast<int>(dev::ft_delay_slot(ut, 0u, R));
        neutral[t] = dev::ft_delay_neutral(ut, d) ? 1 : 0;
        applied[t] = neutral[t] ? -1 : static_cast<int>(dev::ft_delay_slot(ut, d, R));
    }
}
