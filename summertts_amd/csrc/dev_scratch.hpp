// dev_scratch.hpp -- the device side of a stand-alone C API entry (capi_apply.hip, capi_debug.hip): one stream and one allocation per
// tensor, released on every return path.  `ok` latches the first failure; every call after it is a no-op that returns null.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace sts {

struct DevScratch {
    std::vector<void*> ptrs; hipStream_t st = nullptr; bool ok = true;
    static constexpr const char* kNoBuffers = "hipMalloc failed";       // the conv entries' text for !ok before the launch
    DevScratch() { ok = hipStreamCreate(&st) == hipSuccess; }
    ~DevScratch() { if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); } for (void* p : ptrs) (void)hipFree(p); }
    DevScratch(const DevScratch&) = delete;
    DevScratch& operator=(const DevScratch&) = delete;

    static size_t room(size_t bytes) { return bytes ? (bytes + 255) & ~(size_t)255 : 256; }     // what a buffer of `bytes` bytes takes
    void* raw(size_t bytes) {                                           // contents: whatever the allocator returns
        void* d = nullptr;
        if (ok && hipMalloc(&d, room(bytes)) == hipSuccess) { ptrs.push_back(d); return d; }
        ok = false; return nullptr;
    }
    void* filled(size_t bytes, int byte) {
        void* d = raw(bytes);
        ok = ok && hipMemsetAsync(d, byte, room(bytes), st) == hipSuccess;
        return d;
    }
    void put(void* dev, const void* host, size_t bytes) { if (bytes) ok = ok && hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, st) == hipSuccess; }
    void* up_bytes(const void* host, size_t bytes) {                    // null stays null
        if (!host) return nullptr;
        void* d = raw(bytes);
        put(d, host, bytes);
        return d;
    }
    template <class T> const T* up(const T* host, size_t count) { return (const T*)up_bytes(host, count * sizeof(T)); }
    // zero-filled, then the first host_bytes bytes from host (overflow words, a bias, weights followed by their slack)
    void* zeros(size_t bytes, const void* host = nullptr, size_t host_bytes = 0) {
        void* d = filled(bytes, 0);
        if (host) put(d, host, host_bytes);
        return d;
    }
    float* out(size_t count) { return (float*)filled(count * 4, 0xFF); }               // starts out as the sentinel 0xFFFFFFFF (a NaN)
    int16_t* out16(size_t count) {                                                     // starts out as the sentinel 0x7FFF
        int16_t* d = (int16_t*)raw(count * 2);
        ok = ok && hipMemsetD16Async((hipDeviceptr_t)d, 0x7FFF, room(count * 2) / 2, st) == hipSuccess;
        return d;
    }
    // queued copy back; a null destination or source is skipped
    void down(void* host_dst, const void* dev_src, size_t bytes) {
        if (host_dst && dev_src && bytes) ok = ok && hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, st) == hipSuccess;
    }
    bool finish() { return ok = ok && hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess; }
};

}  // namespace sts
