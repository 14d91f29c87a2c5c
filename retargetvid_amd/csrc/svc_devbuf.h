// svc_devbuf.h — DevBuf, the one owner of a block of device memory, and ResampleTab, which holds two.
// Needs only the HIP runtime API's declarations (no device code), so tests/native/devbuf_harness.cpp builds it on the host
// over counting stubs of hipMalloc / hipFree.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

#include <vector>

#include "../../include/svc.h"

void svc_set_error(const char *fmt, ...);

// Move-only: whoever holds the DevBuf holds the block, and the block is freed when that DevBuf goes (or grows: ensure).
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p; bytes = o.bytes;
            o.p = nullptr; o.bytes = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    int ensure(size_t need) {
        if (need <= bytes) return SVC_OK;
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
        hipError_t e = hipMalloc(&p, need);
        if (e != hipSuccess) { svc_set_error("hipMalloc(%zu) failed: %s", need, hipGetErrorString(e)); return SVC_E_NOMEM; }
        bytes = need;
        return SVC_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

// Fixed-point resampling tables for one (in, out) size pair, device resident.
struct ResampleTab {
    int ksize = 0;
    DevBuf bounds;    // int32[out][2]  (first, count)
    DevBuf coeff;     // int32[out][ksize]
    int max_span = 0; // max over blocks of rows spanned (host-computed helper)
    std::vector<int> bounds_host;
    std::vector<int> coeff_host;      // until the first upload (a table is built and checked on the host before any device work)
};
