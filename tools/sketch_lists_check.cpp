// The host code that builds the count sketch's window lists (csrc/sketch_host.hpp), on its own, for the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Igradient-quantization_amd/csrc \
//       tools/sketch_lists_check.cpp -o /tmp/sketch_lists_check && /tmp/sketch_lists_check
// Every layout a tensor can have at small sizes, the largest item count, and the refused arguments; every list is checked to be a
// partition of the items into ascending runs inside exactly-sized buffers (the sanitizer watches their ends).
#include <stdio.h>

#include <vector>

#include "sketch_host.hpp"

static int check(uint64_t seed, int rows, int64_t items, int64_t nwin) {
    std::vector<uint32_t> list((size_t)(rows * items));
    std::vector<int64_t> starts((size_t)(rows * nwin + 1));
    if (gqk_host::build_lists(seed, rows, items, nwin, list.data(), starts.data()) != 0) return 1;
    for (int j = 0; j < rows; ++j) {
        const uint64_t key = gqk_host::row_key(seed, j);
        if (((gqk_host::row_mul(key) * gqk_host::inverse12(gqk_host::row_mul(key))) & 0xfffu) != 1u) return 2;
        std::vector<int> seen((size_t)items);
        for (int64_t v = 0; v < nwin; ++v)
            for (int64_t e = starts[(size_t)(j * nwin + v)]; e < starts[(size_t)(j * nwin + v + 1)]; ++e) {
                const int64_t a = list[(size_t)e] & 0x7ffffu;
                const uint64_t h = gqk_host::item_hash(key, a);
                if (a >= items || seen[(size_t)a]++ || gqk_host::window_of(h, nwin) != v || (list[(size_t)e] >> 19) != (h & 0xfffu)) return 3;
                if (e > starts[(size_t)(j * nwin + v)] && (list[(size_t)(e - 1)] & 0x7ffffu) >= a) return 4;
            }
        for (int64_t a = 0; a < items; ++a)
            if (seen[(size_t)a] != 1) return 5;
    }
    return starts[(size_t)(rows * nwin)] == rows * items ? 0 : 6;
}

int main() {
    const int rows[3] = {1, 3, 5};
    for (int r : rows) {
        for (int64_t items = 1; items <= 200; items += 7)
            for (int64_t nwin = 1; nwin <= items; nwin += 1 + items / 5) {
                const int rc = check(0x1234 + items, r, items, nwin);
                if (rc) return printf("rows %d items %lld nwin %lld: %d\n", r, (long long)items, (long long)nwin, rc), 1;
            }
        if (check(~0ull, r, 1ll << 19, 5462)) return printf("rows %d: the largest tensor\n", r), 1;
    }
    uint32_t l[8];
    int64_t s[8];
    if (gqk_host::build_lists(0, 2, 4, 1, l, s) != -1 || gqk_host::build_lists(0, 1, 0, 1, l, s) != -2 ||
        gqk_host::build_lists(0, 1, (1ll << 19) + 1, 1, l, s) != -2 || gqk_host::build_lists(0, 1, 4, 5, l, s) != -3 ||
        gqk_host::build_lists(0, 1, 4, 1, nullptr, s) != -4)
        return printf("a bad argument went through\n"), 1;
    printf("sketch lists: ok\n");
    return 0;
}
