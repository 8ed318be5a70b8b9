// hip_host.hpp — host-side scaffolding shared by the listing handles (lookup.hip, subjects.hip):
// checked HIP calls and launches, a device array that only grows, and the C ABI's error guard.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>

#include "ketogpu_internal.hpp"

namespace ketogpu {

#define HIP_CHECK(x)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (x);                                                                           \
        if (_e != hipSuccess)                                                                          \
            throw Error(KETOGPU_EDEVICE, std::string(#x) + ": " + hipGetErrorString(_e));              \
    } while (0)

// every launch is checked: a failed launch must fail its call, not a later one
#define KLAUNCH(...)                                 \
    do {                                             \
        hipLaunchKernelGGL(__VA_ARGS__);             \
        HIP_CHECK(hipGetLastError());                \
    } while (0)

// a device array that only grows
template <class T>
struct DBuf {
    T *p = nullptr;
    size_t cap = 0;
    void need(size_t n) {
        if (n <= cap && p) return;
        if (p) (void)hipFree(p);
        p = nullptr, cap = 0;
        void *q = nullptr;
        n = std::max<size_t>(n, 1);
        hipError_t e = hipMalloc(&q, n * sizeof(T));
        if (e != hipSuccess) throw Error(KETOGPU_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
        p = (T *)q, cap = n;
    }
    void drop() {
        if (p) (void)hipFree(p);
        p = nullptr, cap = 0;
    }
};

template <class F>
int guarded(F &&f) {
    try {
        f();
        return KETOGPU_OK;
    } catch (const Error &e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc &) {
        set_last_error("out of host memory");
        return KETOGPU_ENOMEM;
    }
}

}  // namespace ketogpu
