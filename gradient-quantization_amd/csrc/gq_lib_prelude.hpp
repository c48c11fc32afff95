// What every small library beside libgq_hsq.so (libgq_topk / sign / maurey / pvq / rq.so: one .hip file each) starts with.
// Everything here has internal linkage, so each library keeps an error text and a *_last_error of its own; a file brings
// the names into its namespace with using-declarations (`using gql::fail;`).  libgq_hsq.so has gq_common.hpp instead.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "gq_hsq.h"

namespace gql {

// the text of the last failure (gq_*_last_error); one buffer for the process: the checks fail before any launch, and a
// caller that drives the library from several threads at once reads the text of whichever failure came last
static char err_buf[512];

static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf, sizeof(err_buf), fmt, ap);
    va_end(ap);
    return code;
}

// the { seed, step } pair of a stepped launch (libgq_drive.so, libgq_eden.so: SIGNS, STEPPED of their headers)
static inline int check_rotation(const uint64_t *rotation, const char *what) {
    if (!rotation || (reinterpret_cast<uintptr_t>(rotation) & 7) != 0)
        return fail(GQ_ERR_INVALID_ARG, "%s: rotation must be the 8-byte aligned address of a device { seed, step } pair", what);
    return GQ_OK;
}

#define GQL_CHECK_LAUNCH(what)                                                                       \
    do {                                                                                             \
        hipError_t e__ = hipGetLastError();                                                          \
        if (e__ != hipSuccess) return gql::fail(GQ_ERR_HIP, "%s: %s", what, hipGetErrorString(e__)); \
    } while (0)

// compute units of the current device, asked once (256 where the runtime does not say)
static int cu_count() {
    static int cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
            n = 256;
        return n;
    }();
    return cus;
}

// the identity-compressed tensors into the wire, a workgroup of THREADS lanes per tensor in turn (dense_table: int64
// [ndense, 3] = source pointer, byte offset in the wire, elements)
template <int THREADS>
__device__ __forceinline__ void copy_dense(const int64_t *__restrict__ dense_table, int ndense, uint8_t *__restrict__ wire) {
    for (int t = blockIdx.x; t < ndense; t += gridDim.x) {
        const float *src = reinterpret_cast<const float *>(dense_table[3 * t]);
        float *dst = reinterpret_cast<float *>(wire + dense_table[3 * t + 1]);
        const int64_t n = dense_table[3 * t + 2];
        for (int64_t i = threadIdx.x; i < n; i += THREADS) dst[i] = src[i];
    }
}

__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace gql
