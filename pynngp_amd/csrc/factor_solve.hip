// Triangular solves with the NNGP factor: (I - B) x = b and (I - B)^T x = b.
//
// The recurrences
//   forward     x_i = b_i + sum_{k = 0 .. m-1} B[i,k] x[nbr[i,k]]                 (slots that are -1 or >= i: skipped)
//   transposed  x_j = b_j + sum_{e in [off_j, off_j+1)} Brev[e] x[rev_j[e]]       (entries whose child is <= j: skipped)
// are sequential in index order, but their dependency DAG is shallow for spatial input.  The host builds a level
// schedule once per neighbour set (factor_levels.h): the rows of one level depend on earlier levels only, so a
// level is one parallel step.  Two kernels run it, stream-ordered, no atomics, no graph:
//   wide level     (more than fuse_width rows)   one launch over the level's rows
//   narrow run     (consecutive levels of <= fuse_width rows each)   ONE launch of ONE workgroup that walks the
//                  levels with a workgroup barrier between them: the chain of the first m + 1 rows, the long tail
//                  of coordinate-sorted input and a 1-D series cost one launch, not one per level.
//
// A row belongs to an aligned group of kLanes lanes.  The lanes load a chunk of kLanes indices, coefficients and
// gathered x values in parallel (the latency is the gathers'), each index and coefficient once for all columns;
// then every lane of the group folds the chunk IN SLOT ORDER, one fused multiply-add per slot, fetching slot k's
// operands from lane k.  The sum is therefore the sequential one, b_i first, then slot 0, 1, ..., in every column:
// a row's bits depend on its operands alone, not on the kernel that ran it, the level it sits in, fuse_width or
// nrhs.  An invalid slot folds fma(0, 0, acc).
//
// Visibility in the narrow-run kernel.  A value stored in level l by one wave is loaded in level l + 1 by another
// wave of the same workgroup.  __syncthreads() is a workgroup-scope release, the barrier, and a workgroup-scope
// acquire.  That is enough on gfx950 because a workgroup runs on one compute unit (the kernels are not built in
// threadgroup-split mode), whose waves share one vector L1 that serves their requests in order and is
// write-through: a store that precedes the barrier in its wave is seen by every load that another wave of the
// workgroup issues after the barrier, and nothing has to be written back or invalidated -- no agent-scope fence,
// no spinning, no flags.  What it requires of the code: x is read through vector loads of a pointer the compiler
// must treat as written (not const __restrict__, which would allow the scalar cache that this ordering does not
// cover).  Across launches the stream orders everything.
#include "factor.h"

#include <math.h>

#include "../../include/nngp.h"
#include "nngp_internal.h"
#include "philox.h"

namespace nngp {

namespace {

constexpr int kLanes = 16;                            // lanes per row
constexpr int kWideBlock = 256;
constexpr int kWideRows = kWideBlock / kLanes;        // rows per block of the wide kernel
constexpr int kNarrowBlock = 1024;
constexpr int kNarrowGroups = kNarrowBlock / kLanes;  // rows per pass of the narrow-run workgroup
static_assert(NNGP_LATENT_MAX_RHS == 8, "solve_trans dispatches the padded column counts 1, 2, 4, 8");
static_assert(kFactorMaxFuse == NNGP_FACTOR_MAX_FUSE_WIDTH, "header and kernel disagree on the row capacity");

struct Geom {
    const int32_t* nbr;
    const double* B;
    const int32_t* off;
    const int32_t* rev_j;
    const double* Brev;
    int64_t n;
    int m;
};

// One row by its lane group (lane l of kLanes).  KP: the padded column count (1, 2, 4, 8); a padding slot
// re-reads column nrhs - 1 and is never stored, as in latent.hip.  x is deliberately neither const nor
// __restrict__ (see the head of the file); b may alias it: row i alone reads b_i and writes x_i, and the store
// depends on the load.
template <int KP, bool TRANS>
__device__ __forceinline__ void factor_row(const Geom& g, int64_t i, int l, int nrhs, const double* b, double* x) {
    int cc[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) cc[c] = KP == 1 ? 0 : (c < nrhs ? c : nrhs - 1);
    double acc[KP];
    {
        const double* bi = b + i * nrhs;
#pragma unroll
        for (int c = 0; c < KP; ++c) acc[c] = bi[cc[c]];
    }
    int64_t s0, s1;  // the row's slots or reverse entries
    if (TRANS) {
        s0 = g.off[i];
        s1 = g.off[i + 1];
    } else {
        s0 = i * g.m;
        s1 = s0 + g.m;
    }
    const int32_t* idx = TRANS ? g.rev_j : g.nbr;
    const double* coefs = TRANS ? g.Brev : g.B;
    for (int64_t base = s0; base < s1; base += kLanes) {
        const int64_t s = base + l;
        double coef = 0.0, xv[KP];
#pragma unroll
        for (int c = 0; c < KP; ++c) xv[c] = 0.0;
        if (s < s1) {
            const int64_t j = idx[s];
            const bool valid = TRANS ? (j > i && j < g.n) : (j >= 0 && j < i);
            if (valid) {
                coef = coefs[s];
                const double* xj = x + j * nrhs;
#pragma unroll
                for (int c = 0; c < KP; ++c) xv[c] = xj[cc[c]];
            }
        }
        const int cnt = (int)(s1 - base < kLanes ? s1 - base : kLanes);  // uniform over the group
        for (int k = 0; k < cnt; ++k) {
            const double bk = __shfl(coef, k, kLanes);
#pragma unroll
            for (int c = 0; c < KP; ++c) acc[c] = fma(bk, __shfl(xv[c], k, kLanes), acc[c]);
        }
    }
    if (l == 0) {
        double* xi = x + i * nrhs;
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if (c < nrhs) xi[c] = acc[c];
    }
}

// one level: rows[r0 .. r1)
template <int KP, bool TRANS>
__global__ __launch_bounds__(kWideBlock) void factor_wide_kernel(Geom g, const int32_t* __restrict__ rows, int64_t r0,
                                                                 int64_t r1, int nrhs, const double* b, double* x) {
    if (KP == 1) nrhs = 1;
    const int grp = threadIdx.x / kLanes, l = threadIdx.x % kLanes;
    const int64_t r = r0 + (int64_t)blockIdx.x * kWideRows + grp;
    if (r >= r1) return;  // the whole lane group leaves
    const int64_t i = rows[r];
    if ((uint64_t)i >= (uint64_t)g.n) return;
    factor_row<KP, TRANS>(g, i, l, nrhs, b, x);
}

// the levels [l0, l1), each of at most kFactorMaxFuse rows, by one workgroup
template <int KP, bool TRANS>
__global__ __launch_bounds__(kNarrowBlock) void factor_narrow_kernel(Geom g, const int32_t* __restrict__ rows,
                                                                     const int32_t* __restrict__ level_off,
                                                                     int64_t l0, int64_t l1, int nrhs, const double* b,
                                                                     double* x) {
    if (KP == 1) nrhs = 1;
    const int grp = threadIdx.x / kLanes, l = threadIdx.x % kLanes;
    for (int64_t lv = l0; lv < l1; ++lv) {
        const int64_t r0 = level_off[lv], r1 = level_off[lv + 1];
        for (int64_t r = r0 + grp; r < r1; r += kNarrowGroups) {
            const int64_t i = rows[r];
            if ((uint64_t)i < (uint64_t)g.n) factor_row<KP, TRANS>(g, i, l, nrhs, b, x);
        }
        __syncthreads();  // level lv's x is visible to every wave of this workgroup from here on
    }
}

template <int KP, bool TRANS>
hipError_t solve_kp(const Geom& g, const FactorSchedule& sc, int nrhs, int fuse_width, const double* b, double* x,
                    hipStream_t s) {
    const int32_t* lo = sc.level_off_host;
    int64_t lv = 0;
    while (lv < sc.n_levels) {
        const int64_t r0 = lo[lv], r1 = lo[lv + 1];
        if (r1 - r0 > fuse_width) {
            const int64_t blocks = (r1 - r0 + kWideRows - 1) / kWideRows;
            hipLaunchKernelGGL((factor_wide_kernel<KP, TRANS>), dim3((unsigned)blocks), dim3(kWideBlock), 0, s, g,
                               sc.rows, r0, r1, nrhs, b, x);
            ++lv;
        } else {
            int64_t l1 = lv + 1;
            while (l1 < sc.n_levels && lo[l1 + 1] - lo[l1] <= fuse_width) ++l1;
            hipLaunchKernelGGL((factor_narrow_kernel<KP, TRANS>), dim3(1), dim3(kNarrowBlock), 0, s, g, sc.rows,
                               sc.level_off, lv, l1, nrhs, b, x);
            lv = l1;
        }
    }
    return hipGetLastError();
}

template <bool TRANS>
hipError_t solve_trans(const Geom& g, const FactorSchedule& sc, int nrhs, int fuse_width, const double* b, double* x,
                       hipStream_t s) {
    if (nrhs == 1) return solve_kp<1, TRANS>(g, sc, nrhs, fuse_width, b, x, s);
    if (nrhs == 2) return solve_kp<2, TRANS>(g, sc, nrhs, fuse_width, b, x, s);
    if (nrhs <= 4) return solve_kp<4, TRANS>(g, sc, nrhs, fuse_width, b, x, s);
    return solve_kp<8, TRANS>(g, sc, nrhs, fuse_width, b, x, s);
}

// out[i, c] = v[i, c] sc_i, sc_i = sigma2 F_i or its square root; v null: the Philox normal of (seed, i, draw0 + c)
template <bool ROOT>
__global__ __launch_bounds__(256) void factor_scale_kernel(const double* __restrict__ F, double sigma2, int64_t n,
                                                           int nrhs, const double* v, uint64_t seed, uint64_t draw0,
                                                           double* out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double sf = sigma2 * F[i];
        const double sc = ROOT ? sqrt(sf) : sf;
        for (int c = 0; c < nrhs; ++c) {
            const double z = v != nullptr ? v[i * nrhs + c] : philox_normal(seed, (uint64_t)i, draw0 + (uint64_t)c);
            out[i * nrhs + c] = z * sc;
        }
    }
}

}  // namespace

void factor_launch_counts(const FactorSchedule& sc, int fuse_width, int64_t* n_wide, int64_t* n_runs) {
    const int32_t* lo = sc.level_off_host;
    int64_t wide = 0, runs = 0, lv = 0;
    while (lv < sc.n_levels) {
        if (lo[lv + 1] - lo[lv] > fuse_width) {
            ++wide;
            ++lv;
        } else {
            ++runs;
            ++lv;
            while (lv < sc.n_levels && lo[lv + 1] - lo[lv] <= fuse_width) ++lv;
        }
    }
    *n_wide = wide;
    *n_runs = runs;
}

hipError_t factor_solve_launch(const FactorGeom& fg, const FactorSchedule& sc, int nrhs, int trans, int fuse_width,
                               const double* b, double* x, hipStream_t s) {
    if (fg.n == 0 || sc.n_levels == 0) return hipSuccess;
    const Geom g{fg.nbr, fg.B, fg.off, fg.rev_j, fg.Brev, fg.n, fg.m};
    return trans ? solve_trans<true>(g, sc, nrhs, fuse_width, b, x, s)
                 : solve_trans<false>(g, sc, nrhs, fuse_width, b, x, s);
}

hipError_t factor_scale_launch(const double* F, double sigma2, bool root, int64_t n, int nrhs, const double* v,
                               uint64_t seed, uint64_t draw0, double* out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const int64_t want = (n + 255) / 256;
    const unsigned blocks = (unsigned)(want < 65536 ? want : 65536);
    if (root)
        hipLaunchKernelGGL(factor_scale_kernel<true>, dim3(blocks), dim3(256), 0, s, F, sigma2, n, nrhs, v, seed, draw0,
                           out);
    else
        hipLaunchKernelGGL(factor_scale_kernel<false>, dim3(blocks), dim3(256), 0, s, F, sigma2, n, nrhs, v, seed,
                           draw0, out);
    return hipGetLastError();
}

}  // namespace nngp
