// owned_main.cpp -- the owning types of jtokkit_amd/csrc/jtk_owned.h (device buffer, pinned buffer, stream, event) on the CPU,
// under AddressSanitizer and UBSan.  The HIP calls the header makes are stubbed out here: allocations and handles come from
// malloc (so the sanitizer sees a double free, a leak, a read of freed memory), every stub call is counted, live handles are
// counted per kind, and the n-th creating call can be told to fail.  Built by tests/test_abi_and_host.py as
//   g++ -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include tests/cpp/owned_main.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../jtokkit_amd/csrc/jtk_owned.h"

namespace {

enum { DEV, PIN, STREAM, EVENT, KINDS };
int g_calls = 0;                 // every stub call
int g_creates = 0, g_fail_at = 0;   // creating calls so far; the one (counted from 1) that fails, 0: none
int g_live[KINDS] = {0, 0, 0, 0};
int g_frees = 0;
size_t g_last_size = 0;
std::string g_msg;

// a creating call: hipErrorOutOfMemory when it is the one to fail, else a malloc block (filled with 0xEE) as the handle
hipError_t create(int kind, void** out, size_t bytes) {
    g_calls++;
    if (++g_creates == g_fail_at) return hipErrorOutOfMemory;
    *out = malloc(bytes ? bytes : 1);
    memset(*out, 0xEE, bytes ? bytes : 1);
    g_live[kind]++;
    g_last_size = bytes;
    return hipSuccess;
}
hipError_t destroy(int kind, void* p) {
    g_calls++;
    g_frees++;
    g_live[kind]--;
    free(p);
    return hipSuccess;
}
bool none_live() { return !g_live[DEV] && !g_live[PIN] && !g_live[STREAM] && !g_live[EVENT]; }

#define CHECK(cond)                                                                                \
    do {                                                                                           \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); exit(1); }                        \
    } while (0)

// one of each owner, as a batch holds them; make(): every creating path once, the two regrows included
struct All {
    DevBuf d;
    Pinned<int64_t> h;
    Stream s;
    Event e, t;
};
int make(All& a) {
    int rc;
    if ((rc = a.d.ensure(100)) || (rc = a.h.ensure(100))) return rc;
    if (a.s.create() != hipSuccess || a.e.create() != hipSuccess || a.t.create_timed() != hipSuccess) return JTK_ERR_HIP;
    if (a.s.create() != hipSuccess || a.e.create() != hipSuccess || a.t.create_timed() != hipSuccess) return JTK_ERR_HIP;   // (no-ops)
    if ((rc = a.d.ensure(1000)) || (rc = a.h.ensure(10000, 8))) return rc;
    DevBuf exact;
    if (exact.alloc(24) != hipSuccess) return JTK_ERR_OUT_OF_MEMORY;
    a.d = std::move(exact);
    return JTK_OK;
}

}  // namespace

int jtk_fail_msg(int code, const std::string& msg) { g_msg = msg; return code; }

extern "C" {
hipError_t hipMalloc(void** p, size_t n) { return create(DEV, p, n); }
hipError_t hipFree(void* p) { return destroy(DEV, p); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) { return create(PIN, p, n); }
hipError_t hipHostFree(void* p) { return destroy(PIN, p); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { return create(STREAM, (void**)s, 1); }
hipError_t hipStreamDestroy(hipStream_t s) { return destroy(STREAM, s); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return create(EVENT, (void**)e, 1); }
hipError_t hipEventCreate(hipEvent_t* e) { return create(EVENT, (void**)e, 1); }
hipError_t hipEventDestroy(hipEvent_t e) { return destroy(EVENT, e); }
const char* hipGetErrorString(hipError_t) { return "stub error"; }
}

int main() {
    // growth: bytes + bytes / 8 + 256 on the device, bytes + bytes / 4 + 4096 pinned; an exact allocation is exact
    const size_t sizes[4] = {1, 255, 256, 4097}, dev_want[4] = {257, 542, 544, 4865}, pin_want[4] = {4097, 4414, 4416, 9217};
    for (int i = 0; i < 4; i++) {
        DevBuf d;
        CHECK(d.ensure(sizes[i]) == JTK_OK && d.cap == dev_want[i] && g_last_size == dev_want[i] && d.p);
        Pinned<uint8_t> h;
        CHECK(h.ensure(sizes[i]) == JTK_OK && h.cap == pin_want[i] && g_last_size == pin_want[i] && h.p);
        // the hit path: not one stub call, the same memory
        const int calls = g_calls;
        void* const dp = d.p;
        uint8_t* const hp = h.p;
        CHECK(d.ensure(dev_want[i]) == JTK_OK && d.ensure(1) == JTK_OK && d.ensure(0) == JTK_OK && d.p == dp && d.cap == dev_want[i]);
        CHECK(h.ensure(pin_want[i]) == JTK_OK && h.ensure(1, 1) == JTK_OK && h.p == hp && h.cap == pin_want[i]);
        CHECK(g_calls == calls);
        CHECK(d.alloc(sizes[i]) == hipSuccess && d.cap == sizes[i] && g_last_size == sizes[i] && g_live[DEV] == 1);
        CHECK(h.alloc(sizes[i]) == hipSuccess && h.cap == sizes[i] && g_last_size == sizes[i] && g_live[PIN] == 1);
    }
    CHECK(none_live());

    {   // a pinned grow keeps exactly keep_bytes (fresh stub memory is 0xEE), and frees the old allocation once
        Pinned<uint8_t> h;
        CHECK(h.ensure(100) == JTK_OK);
        for (int i = 0; i < 100; i++) h.p[i] = (uint8_t)i;
        const int frees = g_frees;
        CHECK(h.ensure(10000, 40) == JTK_OK && h.cap == 16596 && g_frees == frees + 1 && g_live[PIN] == 1);
        for (int i = 0; i < 40; i++) CHECK(h.p[i] == i);
        for (int i = 40; i < 100; i++) CHECK(h.p[i] == 0xEE);
    }
    {   // a device grow frees first and keeps nothing
        DevBuf d;
        CHECK(d.ensure(10) == JTK_OK);
        const int frees = g_frees;
        CHECK(d.ensure(1000) == JTK_OK && d.cap == 1381 && g_frees == frees + 1 && g_live[DEV] == 1);
    }
    CHECK(none_live());

    {   // move-assign: the target's old allocation is freed once, the source is left empty; a vector of events may grow
        DevBuf a, b;
        CHECK(a.alloc(16) == hipSuccess && b.alloc(32) == hipSuccess);
        void* const pb = b.p;
        const int frees = g_frees;
        a = std::move(b);
        CHECK(g_frees == frees + 1 && a.p == pb && a.cap == 32 && !b.p && !b.cap && g_live[DEV] == 1);
        DevBuf c(std::move(a));
        CHECK(g_frees == frees + 1 && c.p == pb && !a.p && g_live[DEV] == 1);
        Stream s, s2;
        CHECK(s.create() == hipSuccess && s2.create() == hipSuccess);
        s = std::move(s2);
        CHECK(g_live[STREAM] == 1 && !s2.h && (hipStream_t)s == s.h);
        std::vector<Event> ev;
        for (int i = 0; i < 9; i++) { Event e; CHECK(e.create_timed() == hipSuccess); ev.push_back(std::move(e)); }
        CHECK(g_live[EVENT] == 9 && (hipEvent_t)ev[8] == ev[8].h && ev[0].h);
    }
    CHECK(none_live());

    {   // a failed grow: the device buffer is left empty (its old memory went first), the pinned one keeps what it had;
        // both work again afterwards
        DevBuf d;
        Pinned<uint8_t> h;
        CHECK(d.ensure(10) == JTK_OK && h.ensure(10) == JTK_OK);
        memset(h.p, 7, 10);
        uint8_t* const hp = h.p;
        const size_t hcap = h.cap;
        g_fail_at = g_creates + 1;
        CHECK(d.ensure(1000) == JTK_ERR_OUT_OF_MEMORY && !d.p && !d.cap && g_live[DEV] == 0 && g_msg == "hipMalloc: stub error");
        g_fail_at = g_creates + 1;
        CHECK(h.ensure(100000, 10) == JTK_ERR_OUT_OF_MEMORY && h.p == hp && h.cap == hcap && g_live[PIN] == 1 && g_msg == "hipHostMalloc: stub error");
        for (int i = 0; i < 10; i++) CHECK(h.p[i] == 7);
        g_fail_at = 0;
        CHECK(d.ensure(1000) == JTK_OK && d.cap == 1381 && h.ensure(100000, 10) == JTK_OK && h.p[9] == 7 && g_live[DEV] == 1 && g_live[PIN] == 1);
        Stream s;
        Event e;
        g_fail_at = g_creates + 1;
        CHECK(s.create() != hipSuccess && !s.h);
        g_fail_at = g_creates + 1;
        CHECK(e.create() != hipSuccess && !e.h);
        g_fail_at = 0;
    }
    CHECK(none_live());

    {   // an empty owner (never used, or moved from) is destroyed without a stub call
        const int calls = g_calls;
        {
            DevBuf d, d2(std::move(d));
            Pinned<int32_t> h;
            Stream s;
            Event e;
            std::vector<Event> none(4);
            All all;
        }
        CHECK(g_calls == calls);
    }

    // one of each in a struct: whichever creating call fails, the error comes back and nothing outlives the struct
    int total;
    {
        const int before = g_creates;
        All a;
        CHECK(make(a) == JTK_OK && a.d.cap == 24 && g_live[DEV] == 1 && g_live[PIN] == 1 && g_live[STREAM] == 1 && g_live[EVENT] == 2);
        total = g_creates - before;
    }
    CHECK(none_live() && total == 8);
    for (int k = 1; k <= total; k++) {
        {
            All a;
            g_fail_at = g_creates + k;
            CHECK(make(a) != JTK_OK);
            g_fail_at = 0;
        }
        CHECK(none_live());
    }
    printf("owned ok: %d stub calls\n", g_calls);
    return 0;
}
