// device_mem.hpp -- move-only owners of the host layer's HIP resources (host
// only).  The handles (mw_sim, mw_scene, mw_vecenv) own through these; the
// structs handed to kernels (SimDev, SceneDev, ...) hold raw views into them.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <type_traits>
#include <utility>

namespace mw {

struct DevFree { void operator()(void* p) const { (void)hipFree(p); } };
struct PinFree { void operator()(void* p) const { (void)hipHostFree(p); } };
struct EventDestroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct StreamDestroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };

// T is void, an object type, or U[] where the buffer is indexed
template <typename T> using dev_ptr = std::unique_ptr<T, DevFree>;
template <typename T> using pin_ptr = std::unique_ptr<T, PinFree>;
using event_ptr = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;
// a stream the handle created; a caller's stream (mw_set_stream) is a raw view
using stream_ptr = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDestroy>;

// On success the owner takes the new resource and releases the one it held; on
// failure it keeps what it held.
template <typename T>
hipError_t dev_alloc(dev_ptr<T>& out, size_t bytes) {
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) out.reset(static_cast<typename dev_ptr<T>::pointer>(p));
    return e;
}
// ... and the new buffer is zeroed on `stream` first
template <typename T>
hipError_t dev_alloc_zeroed(dev_ptr<T>& out, size_t bytes, hipStream_t stream) {
    dev_ptr<T> p;
    hipError_t e = dev_alloc(p, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(p.get(), 0, bytes, stream);
    if (e == hipSuccess) out = std::move(p);
    return e;
}
template <typename T>
hipError_t pin_alloc(pin_ptr<T>& out, size_t bytes, unsigned flags = hipHostMallocDefault) {
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes, flags);
    if (e == hipSuccess) out.reset(static_cast<typename pin_ptr<T>::pointer>(p));
    return e;
}
inline hipError_t event_create(event_ptr& out, unsigned flags) {
    hipEvent_t ev = nullptr;
    const hipError_t e = hipEventCreateWithFlags(&ev, flags);
    if (e == hipSuccess) out.reset(ev);
    return e;
}
inline hipError_t stream_create(stream_ptr& out, unsigned flags) {
    hipStream_t st = nullptr;
    const hipError_t e = hipStreamCreateWithFlags(&st, flags);
    if (e == hipSuccess) out.reset(st);
    return e;
}

}  // namespace mw
