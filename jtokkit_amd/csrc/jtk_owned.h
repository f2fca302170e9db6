// jtk_owned.h -- what the host library (jtk_abi.cpp, jtk_comm.cpp) owns on a device, each freed by its destructor: device
// buffers, pinned host buffers, streams, events.  Host C++ only.  Owners are members of the heap objects that a jtk_*_destroy
// deletes, or locals of one call; none is global.  None can be copied; a move leaves the source empty.  An empty owner's
// destructor makes no HIP call: an encoding that never reached a device is deleted on a machine that has none.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <string>
#include <utility>

#include "../../include/jtokkit_amd.h"

int jtk_fail_msg(int code, const std::string& msg);          // jtk_abi.cpp: sets jtk_last_error()

#pragma GCC visibility push(hidden)                          // (not part of the library's exported symbols)

// Device memory.  ensure(): scratch that grows with the largest job it has seen (the old memory goes first, nothing is kept);
// alloc(): exactly `bytes` in place of what it held, for what is sized once.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); } return *this; }
    ~DevBuf() { reset(); }
    void reset() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    hipError_t alloc(size_t bytes) {
        reset();
        const hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes; else p = nullptr;
        return e;
    }
    int ensure(size_t bytes) { return bytes <= cap ? JTK_OK : grow(bytes); }       // (the hit is one compare at the call site)
    int grow(size_t bytes) {
        const hipError_t e = alloc(bytes + bytes / 8 + 256);
        return e == hipSuccess ? JTK_OK : jtk_fail_msg(JTK_ERR_OUT_OF_MEMORY, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
};

// Pinned host memory of T; cap is in bytes.  ensure() keeps the first keep_bytes of the old contents and frees the old memory
// last: a grow that fails keeps what it had.
template <class T> struct Pinned {
    T* p = nullptr;
    size_t cap = 0;
    Pinned() = default;
    Pinned(Pinned&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    Pinned& operator=(Pinned&& o) noexcept { if (this != &o) { reset(); p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); } return *this; }
    ~Pinned() { reset(); }
    void reset() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    hipError_t alloc(size_t bytes) {
        reset();
        const hipError_t e = hipHostMalloc((void**)&p, bytes, hipHostMallocDefault);
        if (e == hipSuccess) cap = bytes; else p = nullptr;
        return e;
    }
    int ensure(size_t bytes, size_t keep_bytes = 0) { return bytes <= cap ? JTK_OK : grow(bytes, keep_bytes); }
    int grow(size_t bytes, size_t keep_bytes) {
        Pinned grown;
        const hipError_t e = grown.alloc(bytes + bytes / 4 + 4096);
        if (e != hipSuccess) return jtk_fail_msg(JTK_ERR_OUT_OF_MEMORY, std::string("hipHostMalloc: ") + hipGetErrorString(e));
        if (p && keep_bytes) memcpy(grown.p, p, keep_bytes);
        *this = std::move(grown);
        return JTK_OK;
    }
};

// A stream, an event: create() makes the handle on first use and does nothing after that.
struct Stream {
    hipStream_t h = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Stream& operator=(Stream&& o) noexcept { if (this != &o) { reset(); h = std::exchange(o.h, nullptr); } return *this; }
    ~Stream() { reset(); }
    void reset() { if (h) (void)hipStreamDestroy(h); h = nullptr; }
    hipError_t create() { return h ? hipSuccess : hipStreamCreateWithFlags(&h, hipStreamNonBlocking); }
    operator hipStream_t() const { return h; }
};
struct Event {
    hipEvent_t h = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Event& operator=(Event&& o) noexcept { if (this != &o) { reset(); h = std::exchange(o.h, nullptr); } return *this; }
    ~Event() { reset(); }
    void reset() { if (h) (void)hipEventDestroy(h); h = nullptr; }
    hipError_t create() { return h ? hipSuccess : hipEventCreateWithFlags(&h, hipEventDisableTiming); }   // to order streams
    hipError_t create_timed() { return h ? hipSuccess : hipEventCreate(&h); }                              // for hipEventElapsedTime
    operator hipEvent_t() const { return h; }
};
#pragma GCC visibility pop
