// Stand-alone driver of the factor solves' level builder (pynngp_amd/csrc/factor_levels.h) for the sanitizer
// build of tests/test_factor_levels_host.py: exact-size heap buffers, so any read or write past an array is an
// AddressSanitizer report.  Checks the schedule's defining properties on a few DAG shapes and prints "ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../pynngp_amd/csrc/factor_levels.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}

static int fail(const char* what, int64_t n, int m, int trans) {
    fprintf(stderr, "FAIL %s (n=%lld m=%d trans=%d)\n", what, (long long)n, m, trans);
    return 1;
}

// kind 0: random earlier rows with some -1 and some out-of-rule slots (>= the row); 1: the chain i - 1, i - 2, ..;
// 2: all -1; 3: leaves (rows >= n / 3 point below n / 3)
static int check(int64_t n, int m, int kind) {
    std::vector<int32_t> nbr((size_t)(n * m));
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < m; ++k) {
            int32_t j = -1;
            if (kind == 0) {
                const uint32_t r = rnd() % 8;
                if (r == 0) j = -1;
                else if (r == 1) j = (int32_t)(i + rnd() % 3);  // not below the row: ignored
                else if (i > 0) j = (int32_t)(rnd() % (uint32_t)i);
            } else if (kind == 1) {
                j = i - 1 - k >= 0 ? (int32_t)(i - 1 - k) : -1;
            } else if (kind == 3) {
                const int64_t ns = n / 3 > 0 ? n / 3 : 1;
                const int64_t top = i < ns ? i : ns;
                j = top > 0 ? (int32_t)(rnd() % (uint32_t)top) : -1;
            }
            nbr[(size_t)(i * m + k)] = j;
        }
    for (int trans = 0; trans < 2; ++trans) {
        // exact sizes: n, n, n + 1 (malloc, so that n = 0 still gives distinct zero-size blocks)
        int32_t* level = (int32_t*)malloc(sizeof(int32_t) * (size_t)n);
        int32_t* rows = (int32_t*)malloc(sizeof(int32_t) * (size_t)n);
        int32_t* off = (int32_t*)malloc(sizeof(int32_t) * (size_t)(n + 1));
        const int64_t L = nngp::factor_levels_build(nbr.data(), n, m, trans, level, rows, off);
        int bad = 0;
        if (off[0] != 0 || off[L] != n || (n == 0) != (L == 0)) bad = fail("offsets", n, m, trans);
        std::vector<int32_t> want((size_t)n, 0);  // the level each row must have
        if (!trans) {
            for (int64_t i = 0; i < n; ++i)
                for (int k = 0; k < m; ++k) {
                    const int32_t j = nbr[(size_t)(i * m + k)];
                    if (j >= 0 && j < i && want[j] + 1 > want[i]) want[i] = want[j] + 1;
                }
        } else {
            for (int64_t i = n - 1; i >= 0; --i)
                for (int k = 0; k < m; ++k) {
                    const int32_t j = nbr[(size_t)(i * m + k)];
                    if (j >= 0 && j < i && want[i] + 1 > want[j]) want[j] = want[i] + 1;
                }
        }
        for (int64_t i = 0; i < n && !bad; ++i)
            if (level[i] != want[i]) bad = fail("level", n, m, trans);
        for (int64_t l = 0; l < L && !bad; ++l) {
            if (off[l + 1] <= off[l]) bad = fail("empty level", n, m, trans);
            for (int64_t r = off[l]; r < off[l + 1] && !bad; ++r) {
                if (rows[r] < 0 || rows[r] >= n || level[rows[r]] != l) bad = fail("rows' level", n, m, trans);
                if (r > off[l] && rows[r] <= rows[r - 1]) bad = fail("rows' order", n, m, trans);
            }
        }
        if (kind == 1 && n > 0 && L != n) bad = fail("chain depth", n, m, trans);
        if (kind == 2 && n > 0 && L != 1) bad = fail("flat depth", n, m, trans);
        free(level);
        free(rows);
        free(off);
        if (bad) return 1;
    }
    return 0;
}

int main() {
    const int64_t ns[] = {0, 1, 2, 7, 64, 257, 1000};
    const int ms[] = {1, 3, 15, 63};
    int n_cases = 0;
    for (int64_t n : ns)
        for (int m : ms)
            for (int kind = 0; kind < 4; ++kind) {
                if (check(n, m, kind)) return 1;
                ++n_cases;
            }
    printf("ok %d cases\n", n_cases);
    return 0;
}
