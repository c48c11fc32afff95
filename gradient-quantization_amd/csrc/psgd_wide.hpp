// The rank 16 / 32 launches of libgq_psgd.so (csrc/psgd_wide.hip), as csrc/psgd.hip's entry points reach them.  The descriptor
// has passed check_batch; `what` names the launch that failed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gq_psgd.h"

hipError_t gq_psgd_wide_compress(const gq_psgd_batch *b, uint8_t *wire, bool ef, float ef_scale, float *out, hipStream_t st,
                                 const char **what);
hipError_t gq_psgd_wide_decode(const gq_psgd_batch *b, const uint8_t *gathered, int64_t stride, int R, float *out, hipStream_t st);
