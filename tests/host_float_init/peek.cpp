// Test-only reader of an env handle of the host build (tests/host_build.py):
// the FloatTaskF a floating-base env holds, so tests/test_float_init_abi.py can
// see that a refused configure call left it as it was and where an accepted
// mw_floatenv_init_state lands.  Built into a library of its own against the
// same headers; it only reads through the handle.  Not part of the product.
#include <cstring>

#include "vecenv_state.hpp"

// the bytes of the env's FloatTaskF into out (where cap allows); returns their count, -1 without a floating-base env
extern "C" int fi_task_bytes(const mw_vecenv* e, unsigned char* out, int cap) {
    if (!e || !e->fenv) return -1;
    const int bytes = static_cast<int>(sizeof(mw::FloatTaskF));
    if (out && cap >= bytes) std::memcpy(out, &e->fenv->ftask, sizeof(mw::FloatTaskF));
    return bytes;
}

// FloatTaskF::init: u = on, groups, n_states; f = the eight bound triples in
// the struct's order (pos lo hi, rpy lo hi, lin lo hi, ang lo hi), joint_vel,
// state_prob; p = states, state_out, draws_out
extern "C" int fi_init_fields(const mw_vecenv* e, unsigned* u, float* f, const void** p) {
    if (!e || !e->fenv) return -1;
    const mw::FloatInitF& I = e->fenv->ftask.init;
    u[0] = I.on;
    u[1] = I.groups;
    u[2] = static_cast<unsigned>(I.n_states);
    const float* triples[8] = {I.pos_lo, I.pos_hi, I.rpy_lo, I.rpy_hi, I.lin_lo, I.lin_hi, I.ang_lo, I.ang_hi};
    for (int t = 0; t < 8; ++t)
        for (int k = 0; k < 3; ++k) f[3 * t + k] = triples[t][k];
    f[24] = I.joint_vel;
    f[25] = I.state_prob;
    p[0] = I.states;
    p[1] = I.state_out;
    p[2] = I.draws_out;
    return static_cast<int>(sizeof(mw::FloatInitF));
}
