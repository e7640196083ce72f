// Level schedule of the NNGP factor's triangular solves (factor_solve.hip).  Host code only, no HIP: the C ABI
// (nngp_factor_levels) and a stand-alone sanitizer driver both include it.
//
// The DAG: row i depends on its valid neighbours, a slot being valid when 0 <= nbr[i, k] < i (anything else is
// treated as -1, as the precision operator does).
//   forward     level(i) = 0 without a valid neighbour, else 1 + max level(nbr[i, k]):   one pass in index order
//   transposed  level(j) = 0 when no row lists j, else 1 + max level(i) over the rows i listing j:  one pass in
//               reverse index order (every row listing j has a larger index, so its level is final when it is read)
// rows: the rows sorted by (level, index) -- a counting sort filled in index order; level_off: n_levels + 1
// offsets into it.  The schedule depends on the neighbour sets alone, not on theta.
#pragma once
#include <stdint.h>

namespace nngp {

// level, rows: n entries; level_off: n + 1 entries (a chain has n levels).  Returns the number of levels (0 for
// n = 0, where level_off[0] = 0 is still written).  Requires 0 <= n <= INT32_MAX, m >= 1, trans in {0, 1}.
inline int64_t factor_levels_build(const int32_t* nbr, int64_t n, int m, int trans, int32_t* level, int32_t* rows,
                                   int32_t* level_off) {
    level_off[0] = 0;
    if (n == 0) return 0;
    int32_t top = 0;
    if (trans == 0) {
        for (int64_t i = 0; i < n; ++i) {
            int32_t lv = 0;
            const int32_t* nb = nbr + i * m;
            for (int k = 0; k < m; ++k) {
                const int32_t j = nb[k];
                if (j >= 0 && (int64_t)j < i && level[j] + 1 > lv) lv = level[j] + 1;
            }
            level[i] = lv;
            if (lv > top) top = lv;
        }
    } else {
        for (int64_t i = 0; i < n; ++i) level[i] = 0;
        for (int64_t i = n - 1; i >= 0; --i) {
            const int32_t lv = level[i];
            if (lv > top) top = lv;
            const int32_t* nb = nbr + i * m;
            for (int k = 0; k < m; ++k) {
                const int32_t j = nb[k];
                if (j >= 0 && (int64_t)j < i && lv + 1 > level[j]) level[j] = lv + 1;
            }
        }
    }
    const int64_t n_levels = (int64_t)top + 1;
    for (int64_t l = 0; l <= n_levels; ++l) level_off[l] = 0;
    for (int64_t i = 0; i < n; ++i) ++level_off[level[i] + 1];
    for (int64_t l = 0; l < n_levels; ++l) level_off[l + 1] += level_off[l];
    // fill in index order through a moving cursor kept in level_off itself, then shift the offsets back
    for (int64_t i = 0; i < n; ++i) rows[level_off[level[i]]++] = (int32_t)i;
    for (int64_t l = n_levels; l > 0; --l) level_off[l] = level_off[l - 1];
    level_off[0] = 0;
    return n_levels;
}

}  // namespace nngp
