// host_util.h — the host-side plumbing the satellite modules (stage1, flow_cnn, body_model, eval_metrics) share: the error slot,
// the split-bf16 packing helpers, an owner of device allocations, a device guard and the argument checks of a context.  Host code
// only; no kernel reads it.  Everything is static: each .hip file is its own translation unit and so keeps its own error slot.
// (egoego_hip.hip, the denoiser, does not include this: it keeps its own allocator and does not restore the caller's device.)
#pragma once

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/egoego_hip.h"

static thread_local std::string last_err;  // what the module's egoego_<mod>_last_error() returns
static inline int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    last_err = buf;
    return code;
}
#define HIP_TRY(expr)                                                                                                  \
    do {                                                                                                               \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess)                                                                                          \
            return fail(EGOEGO_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);       \
    } while (0)

static inline hipStream_t as_stream(void* s) { return (hipStream_t)s; }

static inline uint16_t bf16_bits(float v) {  // round to nearest even
    uint32_t u;
    memcpy(&u, &v, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static inline float bf16_val(uint16_t b) {
    uint32_t u = (uint32_t)b << 16;
    float v;
    memcpy(&v, &u, 4);
    return v;
}
// v = hi + lo + O(2^-16 |v|): the two bf16 planes a split-bf16 MFMA reads
static inline void split_store(std::vector<uint16_t>& hi, std::vector<uint16_t>& lo, size_t idx, float v) {
    const uint16_t h = bf16_bits(v);
    hi[idx] = h;
    lo[idx] = bf16_bits(v - bf16_val(h));
}

// n values of a caller's device array -> h.  `name` set: "model pointer <name> is NULL"; unset: "a weight pointer is NULL".
template <typename T>
static int fetch(const T* d, size_t n, std::vector<T>& h, const char* name = nullptr) {
    if (!d) return name ? fail(EGOEGO_E_INVALID, "model pointer %s is NULL", name) : fail(EGOEGO_E_INVALID, "a weight pointer is NULL");
    h.resize(n);
    HIP_TRY(hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}

// The device allocations of one context (on the current device: callers hold a DeviceGuard).
struct DevMem {
    std::vector<void*> ptrs;

    int alloc(size_t bytes, void** p) {
        HIP_TRY(hipMalloc(p, bytes));
        ptrs.push_back(*p);
        return 0;
    }
    template <typename T>
    int upload(const std::vector<T>& h, const T** out) {
        void* p;
        if (int rc = alloc(h.size() * sizeof(T), &p)) return rc;
        HIP_TRY(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
        *out = (const T*)p;
        return 0;
    }
    int copy_dev(const float* d, size_t n, float** out) {  // a copy of a caller's device array
        if (!d) return fail(EGOEGO_E_INVALID, "a weight pointer is NULL");
        void* p;
        if (int rc = alloc(n * sizeof(float), &p)) return rc;
        HIP_TRY(hipMemcpy(p, d, n * sizeof(float), hipMemcpyDeviceToDevice));
        *out = (float*)p;
        return 0;
    }
    void free_all() {
        for (void* p : ptrs) (void)hipFree(p);
        ptrs.clear();
    }
};

// Makes `device` current; the destructor makes the caller's device current again, on every way out of the scope.
struct DeviceGuard {
    int prev = 0;
    bool entered = false;

    DeviceGuard() = default;
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
    int enter(int device) {
        HIP_TRY(hipGetDevice(&prev));
        HIP_TRY(hipSetDevice(device));
        entered = true;
        return 0;
    }
    ~DeviceGuard() {
        if (entered) (void)hipSetDevice(prev);
    }
};

static inline int check_workspace(const void* ws, size_t have, size_t need) {
    if (!ws || ((uintptr_t)ws & 255) || have < need)
        return fail(EGOEGO_E_WORKSPACE, "workspace: %zu bytes at %p, need %zu (256-byte aligned)", have, ws, need);
    return 0;
}

static inline int check_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(EGOEGO_E_INVALID, "device %d not available", device);
    return 0;
}

// The body of egoego_<mod>_ctx_destroy: a context has `device` and a DevMem `mem`.
template <typename Ctx>
static void destroy_ctx(Ctx* c) {
    if (!c) return;
    DeviceGuard g;
    (void)g.enter(c->device);
    c->mem.free_all();
    delete c;
}
