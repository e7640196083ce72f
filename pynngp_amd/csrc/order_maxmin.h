// Levelled max-min (nested-net) point ordering, nngp_order_maxmin: the parts of it that are plain host
// arithmetic -- the key, the per-level radius / cell side, the hash-table sizing -- and the launch interface of
// order_maxmin.hip.  Everything above the launch interface compiles without HIP (tests/host/order_check.cpp).
//
// The order.  dist2 is the squared distance summed in axis order with every operation rounded on
// its own.  key(i) = mix32(i + seed * 0x9e3779b9) << 32 | i, the smaller key wins.  p1 is the point nearest the
// centre of the bounding box (ties: the smallest index), R = sqrt(max dist2(x_i, p1)).  Level l = 1 .. 19 has
// r = R 2^-l and cells of side h = r c_d (c_1, c_2, c_3 = 0.5, 0.7, 0.57: two points of one cell are closer than
// r, points closer than r are at most 2 cells apart per axis).  With A the points selected so far and U the
// unselected points at dist2 >= r^2 from all of A, rounds run until U is empty: the smallest key of U in every
// non-empty cell is that cell's winner; the winners are visited in ascending key order and one is accepted when
// its dist2 to every winner accepted in this round is >= r^2; the accepted join A and every point of U closer
// than r to one of them leaves U.  The order is p1, then the points of level 1, 2, .. 19, then whatever is left
// (level 20, the tail), each level sorted by key.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace nngp {

constexpr int kMaxminLevels = 19;  // the last refining level
constexpr int kMaxminTail = 20;    // level of the points no level selected
constexpr int kMaxminStatsLen = 64;  // int32 counters left at the head of the workspace (include/nngp.h)

inline uint32_t maxmin_mix32(uint32_t h) {  // the murmur3 finaliser
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

inline uint32_t maxmin_hash(uint32_t i, uint32_t seed) { return maxmin_mix32(i + seed * 0x9e3779b9u); }

inline uint64_t maxmin_key(uint32_t i, uint32_t seed) { return ((uint64_t)maxmin_hash(i, seed) << 32) | i; }

inline double maxmin_cell_factor(int dim) { return dim == 1 ? 0.5 : (dim == 2 ? 0.7 : 0.57); }

struct MaxminLevel {
    double r2;  // squared radius of the level
    double h;   // cell side
};

// radius and cell side of level l for the start radius R; false once r^2 is no longer a normal number (the
// remaining points then go to the tail: R = 0, or a point set whose extent squares below DBL_MIN)
inline bool maxmin_level(double R, int dim, int l, MaxminLevel* out) {
    const double r = ldexp(R, -l);
    out->r2 = r * r;
    out->h = r * maxmin_cell_factor(dim);
    return out->r2 >= 2.2250738585072014e-308 && isfinite(out->r2);
}

// slots of an open-addressing table for `entries` keys: a power of two, at least twice the entries and at least 64
inline uint64_t maxmin_table_capacity(uint64_t entries) {
    uint64_t cap = 64;
    while (cap < 2 * entries) cap <<= 1;
    return cap;
}

// cells of side h that the bounding box [lo, hi] can hold, saturating at `limit` (a bound on the non-empty cells
// of a level, hence on the winners of a round, that is far below the point count on the early levels)
inline uint64_t maxmin_cell_bound(const double* lo, const double* hi, int dim, double h, uint64_t limit) {
    double cells = 1.0;
    for (int k = 0; k < dim; ++k) cells *= floor((hi[k] - lo[k]) / h) + 1.0;
    return cells < (double)limit ? (uint64_t)cells : limit;
}

struct MaxminStats {  // what the call did, for the benchmark: kMaxminStatsLen int32 in all
    int32_t launches;     // kernel launches, fills and sorts enqueued
    int32_t host_reads;   // device-to-host count reads (each one a stream synchronise)
    int32_t levels;       // levels run (the last l entered)
    int32_t n_tail;       // points left to the tail
    int32_t rounds[kMaxminLevels + 1];       // rounds of level l (index 0 unused)
    int32_t luby[kMaxminLevels + 1];         // accept / retire iterations of level l, all rounds
    int32_t selected[kMaxminLevels + 1];     // points level l selected (index 0: p1)
};
static_assert(sizeof(MaxminStats) == kMaxminStatsLen * sizeof(int32_t), "MaxminStats layout");

enum MaxminStatus { kMaxminOk = 0, kMaxminHipError = 1, kMaxminTableOverflow = 2, kMaxminNotFinite = 3 };

#ifdef __HIPCC__
size_t order_maxmin_workspace_bytes(int64_t n, int dim);
// perm_out int64 (n,), level_out int32 (n,) (by position); synchronises `s` (one count read per round).  On a
// HIP failure *err holds the error.
MaxminStatus order_maxmin_launch(const double* coords, int64_t n, int dim, uint32_t seed, int64_t* perm_out,
                                 int32_t* level_out, void* workspace, hipStream_t s, hipError_t* err);
#endif

}  // namespace nngp
