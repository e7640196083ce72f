// Stand-alone check of the host arithmetic of the levelled max-min ordering (pynngp_amd/csrc/order_maxmin.h):
// the key, the level radii, the table sizing and the cell bound, meant to be built with
// -fsanitize=address,undefined.  Prints "ok", eight keys (seed 0 and 5, rows 0..3) and level 7's r2 and h for
// R = 3.7 in 2-D, which tests/test_order_host.py compares with the numpy restatement.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "order_maxmin.h"

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                             \
        }                                                         \
    } while (0)

int main() {
    using namespace nngp;
    CHECK(maxmin_mix32(0u) == 0u && maxmin_mix32(1u) == 0x514e28b7u && maxmin_mix32(0xdeadbeefu) == 0x0de5c6a9u);
    CHECK((uint32_t)maxmin_key(0xffffffffu, 0xffffffffu) == 0xffffffffu);  // the sum wraps mod 2^32
    CHECK(maxmin_key(7u, 0u) >> 32 == maxmin_mix32(7u));

    // table sizing: a power of two, >= 2 x entries, >= 64, for every count up to 2^31
    const uint64_t counts[] = {0, 1, 31, 32, 33, 1000, 65536, 65537, 10000000, (1ull << 31) - 1};
    for (uint64_t c : counts) {
        const uint64_t cap = maxmin_table_capacity(c);
        CHECK(cap >= 64 && cap >= 2 * c && (cap & (cap - 1)) == 0 && (cap == 64 || cap < 4 * c));
    }

    // level radii: halving, r2 = r r, h = r c_d; false once r2 leaves the normal range, and for R = 0, inf, NaN
    MaxminLevel lv, prev;
    for (int dim = 1; dim <= 3; ++dim) {
        CHECK(maxmin_level(3.7, dim, 1, &prev));
        for (int l = 2; l <= kMaxminLevels; ++l) {
            CHECK(maxmin_level(3.7, dim, l, &lv));
            CHECK(lv.r2 * 4.0 == prev.r2 && lv.h * 2.0 == prev.h && lv.h * lv.h * dim < lv.r2);
            prev = lv;
        }
        CHECK(!maxmin_level(0.0, dim, 1, &lv));
        CHECK(!maxmin_level(1e-150, dim, 19, &lv) && maxmin_level(1e-140, dim, 19, &lv));
        CHECK(!maxmin_level(INFINITY, dim, 3, &lv) && !maxmin_level(NAN, dim, 3, &lv));
    }

    // cell bound: never below the cells a box holds, saturating, and below 2^21 per axis through level 19
    const double lo[3] = {-1.0, 0.0, 2.0}, hi[3] = {1.0, 0.5, 2.0};
    CHECK(maxmin_cell_bound(lo, hi, 3, 0.25, 1000) == 9 * 3 * 1);
    CHECK(maxmin_cell_bound(lo, hi, 3, 1e-9, 1000) == 1000);
    CHECK(maxmin_cell_bound(lo, hi, 1, 0.5, 1000) == 5);
    for (int dim = 1; dim <= 3; ++dim) {
        // the widest box for a start radius R = 1 is 2 R per axis
        CHECK(maxmin_level(1.0, dim, kMaxminLevels, &lv));
        const double per_axis = 2.0 / lv.h;
        CHECK(dim == 1 ? per_axis <= 2097152.0 : per_axis < 2097152.0 - 2.0);
    }

    // the stats block is what include/nngp.h says it is
    std::vector<int32_t> block(kMaxminStatsLen, 0);
    MaxminStats* st = reinterpret_cast<MaxminStats*>(block.data());
    st->selected[kMaxminLevels] = 5;
    CHECK(block[kMaxminStatsLen - 1] == 5);

    std::printf("ok");
    for (uint32_t seed : {0u, 5u})
        for (uint32_t i = 0; i < 4; ++i) std::printf(" %llx", (unsigned long long)maxmin_key(i, seed));
    CHECK(maxmin_level(3.7, 2, 7, &lv));
    std::printf(" %a %a\n", lv.r2, lv.h);
    return 0;
}
