// errors.hpp -- the thread-local last error behind mw_last_error() (sim.cpp)
// and the result helpers of the host layer (sim.cpp, world_params.cpp, vecenv.cpp,
// floatenv.cpp, scene.cpp).
#pragma once

#include <cstring>
#include <string>

#include "mwstep.h"

namespace mw {
void set_last_error(const std::string& msg);

inline int fail(int code, const std::string& msg) {
    set_last_error(msg);
    return code;
}

// a string result of the C ABI into the caller's buffer
inline int copy_str(const std::string& v, char* buf, int32_t len) {
    if (!buf || len <= 0) return fail(MW_EINVAL, "invalid output buffer");
    if (static_cast<int32_t>(v.size()) + 1 > len) return fail(MW_EINVAL, "output buffer too small");
    std::memcpy(buf, v.c_str(), v.size() + 1);
    return MW_OK;
}
}  // namespace mw

#define MW_HIP(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return mw::fail(MW_EHIP, std::string(#call " failed: ") + hipGetErrorString(e_)); \
    } while (0)
