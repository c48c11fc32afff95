// The count sketch's hash and its window lists on the host (include/gq_sketch.h: HASH, SUM ORDER).  No device code: sketch.hip
// exports build_lists as gq_sketch_build_lists, and tools/sketch_lists_check.cpp runs it under the host sanitizers.
#pragma once
#include <stdint.h>

#include <vector>

namespace gqk_host {

constexpr uint64_t G = 0x9E3779B97F4A7C15ull, M = 0xD6E8FEB86659FD93ull;

inline uint64_t fin(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

inline uint64_t row_key(uint64_t seed, int j) { return fin(seed + (uint64_t)(j + 1) * G); }
inline uint32_t row_mul(uint64_t key) { return ((uint32_t)(key >> 20) & 0xfffu) | 1u; }

// the inverse of an odd a mod 4096 (Newton: every step doubles the correct low bits, three of them to start with)
inline uint32_t inverse12(uint32_t a) {
    uint32_t x = a;
    for (int s = 0; s < 3; ++s) x = x * (2u - a * x);
    return x & 0xfffu;
}

inline uint64_t item_hash(uint64_t key, int64_t a) { return fin(key + (uint64_t)(a + 1) * G); }
inline int64_t window_of(uint64_t h, int64_t nwin) { return (int64_t)(((h >> 32) * (uint64_t)nwin) >> 32); }

// 0, or a negative number naming the argument that is out of range
inline int build_lists(uint64_t seed, int rows, int64_t items, int64_t nwin, uint32_t *list, int64_t *starts) {
    if (rows != 1 && rows != 3 && rows != 5) return -1;
    if (items < 1 || items > (1ll << 19)) return -2;
    if (nwin < 1 || nwin > items) return -3;
    if (!list || !starts) return -4;
    std::vector<int64_t> fill((size_t)nwin);
    std::vector<uint32_t> win((size_t)items), off((size_t)items);
    for (int j = 0; j < rows; ++j) {
        const uint64_t key = row_key(seed, j);
        int64_t *st = starts + (int64_t)j * nwin;
        for (int64_t v = 0; v < nwin; ++v) fill[(size_t)v] = 0;
        for (int64_t a = 0; a < items; ++a) {
            const uint64_t h = item_hash(key, a);
            win[(size_t)a] = (uint32_t)window_of(h, nwin);
            off[(size_t)a] = (uint32_t)(h & 0xfffu);
            fill[win[(size_t)a]] += 1;
        }
        int64_t at = (int64_t)j * items;
        for (int64_t v = 0; v < nwin; ++v) {
            st[v] = at;
            at += fill[(size_t)v];
            fill[(size_t)v] = st[v];      // (from here on: the window's next free entry)
        }
        for (int64_t a = 0; a < items; ++a) list[fill[win[(size_t)a]]++] = (uint32_t)a + (off[(size_t)a] << 19);
    }
    starts[(int64_t)rows * nwin] = (int64_t)rows * items;
    return 0;
}

}  // namespace gqk_host
