// The host side of pw_encode_run (pvq_walk.hpp) for the libraries that launch it: libgq_pvq.so and libgq_rq.so.
#pragma once
#include "gq_lib_prelude.hpp"
#include "pvq_walk.hpp"

namespace gq {

// the shapes the run walker is built for: d in {8, 16, 32}, K = 32 ... 256 in whole blocks of 32, byte codes
inline bool pw_run_serves(int d, int K, int code_bytes) {
    return (d == 8 || d == 16 || d == 32) && K >= 32 && K <= 256 && (K & 31) == 0 && code_bytes == 1;
}

// What the sampler needs of (random_mode, seed, r_flat); `what` names the entry point in the error text.  The kernel reads
// the { seed, step } words of GQ_RANDOM_DEVICE_COUNTER with one 64-bit load each: a null or misaligned address is refused here.
static int pw_check_draws(int random_mode, uint64_t seed, const float *r_flat, const char *what) {
    if (random_mode != GQ_RANDOM_GIVEN && random_mode != GQ_RANDOM_DEVICE && random_mode != GQ_RANDOM_DEVICE_KEYED &&
        random_mode != GQ_RANDOM_DEVICE_COUNTER)
        return gql::fail(GQ_ERR_INVALID_ARG, "%s: random_mode must be GIVEN, DEVICE, DEVICE_KEYED or DEVICE_COUNTER (the sampler needs draws)", what);
    if (random_mode == GQ_RANDOM_GIVEN && !r_flat) return gql::fail(GQ_ERR_INVALID_ARG, "%s: r_flat is null", what);
    if (random_mode == GQ_RANDOM_DEVICE_COUNTER && (!seed || (seed & 7)))
        return gql::fail(GQ_ERR_INVALID_ARG, "%s: DEVICE_COUNTER needs the 8-byte aligned address of the { seed, step } words", what);
    return GQ_OK;
}

// One launch of Kernel(const Args), a kernel whose body is pw_encode_run<D> over a.run: at most one resident wave of
// workgroups, so that none queues behind another, and every wave's run of consecutive tiles filled in.
template <int D, auto Kernel, class Args>
static int pw_launch_run(const Args &a, hipStream_t st, const char *what) {
    constexpr size_t lds_bytes = PwShape<D>::LDS_BYTES;
    static const int bpc = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)hipGetLastError();
        return resident_blocks_per_cu(Kernel, ENC_THREADS, lds_bytes);
    }();
    int64_t blocks = (a.run.ntiles + ENC_WAVES - 1) / ENC_WAVES;
    const int64_t cap = (int64_t)gql::cu_count() * bpc;
    if (blocks > cap) blocks = cap;
    Args b = a;
    const int64_t waves = blocks * ENC_WAVES;
    b.run.tiles_per_wave = (int)(a.run.ntiles / waves);
    b.run.waves_with_one_more = (int)(a.run.ntiles - (int64_t)b.run.tiles_per_wave * waves);
    hipLaunchKernelGGL(Kernel, dim3((unsigned)blocks), dim3(ENC_THREADS), lds_bytes, st, b);
    GQL_CHECK_LAUNCH(what);
    return GQ_OK;
}

}  // namespace gq
