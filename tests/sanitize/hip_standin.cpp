// hip_standin.cpp -- a host stand-in for the HIP runtime and the kernel
// launchers, for the lifecycle harness (lifecycle_driver.cpp).  The runtime
// entry points the host layer calls work on plain heap memory, so the
// sanitizers see every buffer, copy and free; launches do nothing (the scene's
// writes a contact record).  It counts
// the live objects (buffers, streams, events) and can make one chosen creating
// call fail, which is how the harness checks what each handle owns.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "float_task.hpp"
#include "kernels.hpp"
#include "scene_params.hpp"

namespace {
long g_live = 0;
long g_countdown = -1;  // creating calls left before the one that fails; < 0: none fails
bool g_fired = false;

// one creating call: true if it is the one to fail
bool refuse() {
    if (g_countdown < 0) return false;
    if (g_countdown-- > 0) return false;
    g_fired = true;
    return true;
}

hipError_t create(void** out, size_t bytes) {
    *out = nullptr;
    if (refuse()) return hipErrorOutOfMemory;
    *out = std::calloc(1, bytes ? bytes : 1);
    if (!*out) return hipErrorOutOfMemory;
    ++g_live;
    return hipSuccess;
}

hipError_t release(void* p) {
    if (p) --g_live;
    std::free(p);
    return hipSuccess;
}
}  // namespace

// the harness's controls
extern "C" long standin_live() { return g_live; }
extern "C" void standin_fail_at(long k) {
    g_countdown = k;
    g_fired = false;
}
extern "C" int standin_fired() { return g_fired ? 1 : 0; }

extern "C" {

hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "out of memory (injected)"; }

hipError_t hipMalloc(void** p, size_t n) { return create(p, n); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) { return create(p, n); }
hipError_t hipFree(void* p) { return release(p); }
hipError_t hipHostFree(void* p) { return release(p); }
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned int) {
    *d = h;
    return hipSuccess;
}

hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) {
    if (n) std::memmove(d, s, n);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) {
    if (n) std::memmove(d, s, n);
    return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void* d, size_t dpitch, const void* s, size_t spitch, size_t width, size_t height,
                            hipMemcpyKind, hipStream_t) {
    for (size_t r = 0; r < height && width; ++r)
        std::memmove(static_cast<char*>(d) + r * dpitch, static_cast<const char*>(s) + r * spitch, width);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) {
    if (n) std::memset(d, v, n);
    return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t* st, unsigned int) {
    return create(reinterpret_cast<void**>(st), 1);
}
hipError_t hipStreamDestroy(hipStream_t st) { return release(st); }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus* c) {
    *c = hipStreamCaptureStatusNone;
    return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned) { return create(reinterpret_cast<void**>(ev), 1); }
hipError_t hipEventDestroy(hipEvent_t ev) { return release(ev); }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }

}  // extern "C"

namespace mw {

// serial chains and the 9-dof Panda tree, as the library's; nothing else
int kernel_topology(const int* parents, int n) {
    bool chain = n >= 1 && n <= 9;
    for (int i = 0; i < n; ++i) chain = chain && parents[i] == i - 1;
    return chain ? 0 : (n == 9 ? 1 : -1);
}
// no lane kernel for floating trees: they all take the world-per-wavefront path
int float_workspace_words(int, int) { return -1; }

hipError_t launch_scenario_run(const ChainF*, int, int, bool, bool, int, const SimDev&, const PidSet&, int,
                               const RunArgs&, hipStream_t) { return hipSuccess; }
hipError_t launch_free_run(const FreeF*, const FreeDev&, int, const RunArgs&, int, int, hipStream_t) {
    return hipSuccess;
}
hipError_t launch_float_run(const ChainF*, int, int, bool, const FloatF*, const SimDev&, const FreeDev&,
                            const PidSet&, float*, int, const RunArgs&, int, hipStream_t) { return hipSuccess; }
hipError_t launch_wave_run(const ChainF*, int, int, bool, const FloatF*, const SimDev&, const FreeDev&, const PidF*,
                           int, const RunArgs&, int, int*, hipStream_t) { return hipSuccess; }
hipError_t launch_vecenv_reset(const ChainF*, int, const TaskF&, const SimDev&, const VecDev&, float*, int,
                               hipStream_t) { return hipSuccess; }
hipError_t launch_vecenv_pid_reset(const ChainF*, int, const TaskF&, const SimDev&, const VecDev&, float*, int,
                                   hipStream_t) { return hipSuccess; }
hipError_t launch_vecenv_pid_step(const ChainF*, int, int, bool, bool, int, const TaskF&, const SimDev&,
                                  const VecDev&, const PidSet&, const float*, float*, float*, uint8_t*, float*, int,
                                  float, int, int, hipStream_t) { return hipSuccess; }
hipError_t launch_vecenv_pid_group(const ChainF*, int, bool, bool, const TaskF&, const SimDev&, const VecDev&,
                                   const GLaneTask*, const float*, float*, float*, uint8_t*, float*, int, float, int,
                                   int, hipStream_t) { return hipSuccess; }
hipError_t launch_float_env_action(const FloatTaskF&, const float*, float*, float*, uint8_t*, unsigned long long*, int,
                                   int, hipStream_t) { return hipSuccess; }
hipError_t launch_float_env_post(const ChainF*, const FloatTaskF&, const SimDev&, const FreeDev&, const VecDev&,
                                 const float*, float*, float*, uint8_t*, float*, int, int, int, hipStream_t) {
    return hipSuccess;
}
hipError_t launch_vecenv_step(const ChainF*, int, bool, bool, int, const TaskF&, const SimDev&, const VecDev&,
                              const void*, float*, float*, uint8_t*, float*, int, float, int, int, int, hipStream_t) {
    return hipSuccess;
}
// The one launch that leaves something behind: a step's contact output, so
// that the host's readback (mw_scene_get_contacts) has records to index --
// every ground slot of every world touches, node c % n_nodes against the
// ground, the values numbered.  A paused launch writes nothing, as the kernel.
hipError_t launch_scene_run(const SceneF* P, int, const SceneDev& D, const PidF*, const SceneGates&, int W,
                            const SceneArgs& a, hipStream_t) {
    if (a.paused || !D.contact || !D.ncontact || P->n_nodes <= 0) return hipSuccess;
    const int slots = P->ground ? P->n_slots : 0;
    const int nc = slots < D.contact_cap ? slots : D.contact_cap;
    for (int w = 0; w < W; ++w) {
        D.ncontact[w] = nc;
        for (int c = 0; c < nc; ++c) {
            float* o = D.contact + static_cast<size_t>(c) * 12 * W + w;
            for (int f = 0; f < 10; ++f) o[static_cast<size_t>(f) * W] = static_cast<float>(100 * w + c + 0.125f * f);
            const int32_t na = c % P->n_nodes, nb = -1;
            std::memcpy(o + static_cast<size_t>(10) * W, &na, sizeof na);
            std::memcpy(o + static_cast<size_t>(11) * W, &nb, sizeof nb);
        }
    }
    return hipSuccess;
}

}  // namespace mw
