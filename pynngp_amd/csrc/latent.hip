// Latent-field posterior at fixed theta: w | y, theta ~ N(A^-1 b, A^-1) with
//   A = (I - B)^T (sigma2 F)^-1 (I - B) + diag(d),   d = h / tau2,   b = h (y - X beta) / tau2
// (B, F the unit-variance factors of nngp_bf_sweep; oracle/nngp_gibbs_oracle.py::dag_posterior).  A is
// never assembled.  The reference keeps the latent state as ws / wt (pyNNGP/nngp.py:42-47) and has no
// estimator for it; this is the deterministic one next to the Gibbs sampler (gibbs.hip), whose reverse
// lists and `prep` buffer (Brev, P, invF) it reuses.
//
// One product with A is two stream-ordered phases, no atomics:
//   row phase     t_i   = (x_i - sum_s B[i,s] x[nbr[i,s]]) invF_i / sigma2       (gather over nbr)
//   column phase  out_i = t_i - sum_{e in [off_i, off_i+1)} Brev[e] t[rev_j[e]] + d_i x_i   (gather over the
//                 reverse list, in its stored order)
// Every sum has a fixed order that depends on (m, the list's length) only: a row's slots and a short
// list's entries are dealt lane-strided over an aligned lane group and folded by a fixed xor butterfly; a
// list longer than kLongList is summed by the whole 256-thread block (thread-strided, the fixed wave
// butterfly, then the four wave sums in order).  Which block or tile a location lands in changes nothing,
// so the result is bit-identical run to run and independent of the grid.
//
// The CG keeps alpha and beta on the device.  Its dots go through per-block records folded in a fixed
// order by every block that needs the scalar (the same bits in each), so a solve is bit-reproducible.
//
// One kernel family serves every call.  Vectors are (n, nrhs) row-major, 1 <= nrhs <= kMaxRhs, a single
// right-hand side being nrhs = 1: an index or coefficient is loaded once for all columns and a gather
// fetches nrhs contiguous doubles.  The kernels are templates on KP, the padded column count (1, 2, 4, 8:
// the smallest that holds nrhs): register arrays are indexed by compile-time constants only; a padding
// column c >= nrhs re-reads column nrhs - 1 (a valid address, no branch around the load) and is never stored.
// A column's bits depend neither on KP nor on the other columns: the lane groups, tiles, grids, thread ->
// location and tile -> block mappings are the same for every KP, no arithmetic crosses columns, and each
// column's expression sequence is one text (every multiply-add is an explicit fma or cannot fuse).
//
// A reference set (S != T): nodes 0 .. n_s - 1 are reference points, n_s .. n - 1 leaves whose parents are all
// reference points.  A leaf is conditionally independent of everything else given S and is integrated out, which
// leaves the posterior of w_S alone, with L the stacked [(I - B_S); -B_L] and s the row scale (f_r = invF_r /
// sigma2 on a reference row, g_r = f_r d_r / (f_r + d_r) on a leaf row):
//   A_S = L^T diag(s) L + diag(d_S),   b_S = d_S v_S + B_L^T (g v_L)
// This is the same two-phase operator written over the n-node structure: the REF instantiations of the row and
// column kernels take the row scale from the vector s, give a leaf row no self term (its x is implicitly 0) and
// run the column phase over the first n_s nodes only, whose reverse lists hold both kinds of children.  The
// S = T instantiations (REF = false) are the text they were.
//
// The host side has one launch per operation, in the reference-set form (latent.h).  S = T is the system without
// leaves, n_s = n: each launch then leaves g.s null, which selects the REF = false instantiations and the plain
// workspace layout, so nothing is computed or read for leaves that do not exist.
#include "latent.h"

#include <math.h>

#include "../../include/nngp.h"
#include "nngp_internal.h"

namespace nngp {

namespace {

constexpr int kBlock = 256;
constexpr int kColLanes = 16;                    // lanes per location in the column phase
constexpr int kColRows = kBlock / kColLanes;     // locations per tile
constexpr int kLongList = 32 * kColLanes;        // a lane group's budget; longer lists go to the block
constexpr int kMaxTileBlocks = 2048;             // persistent grid of the operator phases (= p.q records)
constexpr int kMaxVecBlocks = 1024;              // grid of the CG's vector kernels (= records per dot)
constexpr int kMaxRhs = NNGP_LATENT_MAX_RHS;

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// sum over an aligned group of G lanes, every lane getting the bits of the descending xor butterfly
template <int G>
__device__ __forceinline__ double lane_group_sum(double v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// fixed-order sum over the 256-thread block, the same bits in every thread; all threads call it
__device__ __forceinline__ double block_sum(double v, double* sh4) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh4[0] + sh4[1]) + sh4[2]) + sh4[3];
}

// fold of n_rec per-block records: thread-strided partial sums, then block_sum.  Every block that folds the
// same records gets the same bits.
__device__ __forceinline__ double fold_records(const double* __restrict__ rec, int n_rec, double* sh4) {
    double a = 0.0;
    for (int k = threadIdx.x; k < n_rec; k += kBlock) a += rec[k];
    return block_sum(a, sh4);
}

// the contiguous run of tiles a block of a persistent grid owns (XCD-contiguous: neighbours meet in one L2)
__device__ __forceinline__ void tile_range(int64_t n_tiles, int64_t* lo, int64_t* hi) {
    const int64_t nb = gridDim.x, lb = xcd_logical_block(blockIdx.x, nb);
    *lo = lb * n_tiles / nb;
    *hi = (lb + 1) * n_tiles / nb;
}

// The column count as a KP instantiation sees it: the launch's nrhs, except that KP = 1 serves nrhs = 1 only
// and knows it at compile time.  There the row stride is the constant 1 and the padding clamp and the store
// guards fold away, which keeps the one-column kernels at the cost of kernels written for one vector.
template <int KP>
__device__ __forceinline__ int columns(int nrhs) {
    return KP == 1 ? 1 : nrhs;
}

// the column that register slot c reads: its own, or column nrhs - 1 for a padding slot
__device__ __forceinline__ int column_of(int c, int nrhs) { return c < nrhs ? c : nrhs - 1; }

// CG state words (doubles) of one column; kMaxRhs such blocks end the workspace, followed by the two "every
// column is finished" words for the even and the odd iterations (the operator launches' stop word)
enum { kRz0 = 0, kRz1 = 1, kRr = 2, kBb = 3, kTol2 = 4, kAlpha = 5, kBeta = 6, kIter = 7, kStatus = 8, kFlag0 = 9,
       kFlag1 = 10, kBrk = 11, kStateWords = 32 };
enum { kAll0 = kMaxRhs * kStateWords, kAll1 = kAll0 + 1 };

// ---------------------------------------------------------------- row phase
// G lanes per location (G = 4, 8 or 16 by m alone); lane l takes slots l, l + G, ...: the nbr and B rows are
// read coalesced.  stop: null, or a device word that makes the launch a no-op when non-zero (a finished CG).
// REF: x has n_s rows, t all n; `invF` is the row scale s itself (inv_s2 unused); a slot naming a node >= n_s
// counts as -1; a leaf row i >= n_s has no self term: t_i = -s_i sum_s B[i,s] x[nbr[i,s]].
template <int G, int KP, bool REF>
__global__ __launch_bounds__(kBlock) void latent_row_kernel(const int32_t* __restrict__ nbr,
                                                            const double* __restrict__ B,
                                                            const double* __restrict__ invF,
                                                            const double* __restrict__ x, double* __restrict__ t,
                                                            int64_t n, int m, int nrhs, double inv_s2,
                                                            const double* __restrict__ stop, int64_t n_s) {
    if (stop != nullptr && *stop != 0.0) return;
    const int64_t nx = REF ? n_s : n;  // rows of x
    nrhs = columns<KP>(nrhs);
    constexpr int kRows = kBlock / G;
    const int g = threadIdx.x / G, l = threadIdx.x % G;
    int cc[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) cc[c] = column_of(c, nrhs);
    int64_t lo, hi;
    tile_range((n + kRows - 1) / kRows, &lo, &hi);
    for (int64_t tile = lo; tile < hi; ++tile) {
        const int64_t i = tile * kRows + g;
        double acc[KP];
#pragma unroll
        for (int c = 0; c < KP; ++c) acc[c] = 0.0;
        if (i < n) {
            const int32_t* nb = nbr + i * m;
            const double* bb = B + i * m;
            for (int s = l; s < m; s += G) {
                const int32_t j = nb[s];
                if (j >= 0 && (int64_t)j < nx) {  // a slot without a point: exactly 0 in every column
                    const double b = bb[s];
                    const double* xj = x + (int64_t)j * nrhs;
#pragma unroll
                    for (int c = 0; c < KP; ++c) acc[c] = fma(b, xj[cc[c]], acc[c]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < KP; ++c) acc[c] = lane_group_sum<G>(acc[c]);
        if (i < n && l == 0) {
            const double sc = REF ? invF[i] : invF[i] * inv_s2;
            const bool self = !REF || i < nx;
            const double* xi = x + (self ? i : 0) * nrhs;
            double* ti = t + i * nrhs;
#pragma unroll
            for (int c = 0; c < KP; ++c)
                if (c < nrhs) ti[c] = ((self ? xi[c] : 0.0) - acc[c]) * sc;
        }
    }
}

// The row phase's gather with two weights and no scale: for every node row i (reference rows and leaves alike)
//   p[i, c] = sum_s B[i,s] x[nbr[i,s], c],   q[i, c] = sum_s dB[i,s] x[nbr[i,s], c]
// with x on the n_s reference nodes.  An index is read once for both weights and all columns; lanes, slots and
// the butterfly are latent_row_kernel's, so each sum has that kernel's order and a column's bits depend on
// neither KP nor the other columns.  A slot that is -1 or names a node >= n_s: exactly 0.
template <int G, int KP>
__global__ __launch_bounds__(kBlock) void latent_row_dot2_kernel(const int32_t* __restrict__ nbr,
                                                                 const double* __restrict__ B,
                                                                 const double* __restrict__ dB,
                                                                 const double* __restrict__ x, double* __restrict__ p,
                                                                 double* __restrict__ q, int64_t n, int64_t n_s, int m,
                                                                 int nrhs) {
    nrhs = columns<KP>(nrhs);
    constexpr int kRows = kBlock / G;
    const int g = threadIdx.x / G, l = threadIdx.x % G;
    int cc[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) cc[c] = column_of(c, nrhs);
    int64_t lo, hi;
    tile_range((n + kRows - 1) / kRows, &lo, &hi);
    for (int64_t tile = lo; tile < hi; ++tile) {
        const int64_t i = tile * kRows + g;
        double ap[KP], aq[KP];
#pragma unroll
        for (int c = 0; c < KP; ++c) ap[c] = aq[c] = 0.0;
        if (i < n) {
            const int32_t* nb = nbr + i * m;
            const double* bb = B + i * m;
            const double* db = dB + i * m;
            for (int s = l; s < m; s += G) {
                const int32_t j = nb[s];
                if (j >= 0 && (int64_t)j < n_s) {
                    const double b = bb[s], d = db[s];
                    const double* xj = x + (int64_t)j * nrhs;
#pragma unroll
                    for (int c = 0; c < KP; ++c) {
                        const double xv = xj[cc[c]];
                        ap[c] = fma(b, xv, ap[c]);
                        aq[c] = fma(d, xv, aq[c]);
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            ap[c] = lane_group_sum<G>(ap[c]);
            aq[c] = lane_group_sum<G>(aq[c]);
        }
        if (i < n && l == 0) {
#pragma unroll
            for (int c = 0; c < KP; ++c)
                if (c < nrhs) {
                    p[i * nrhs + c] = ap[c];
                    q[i * nrhs + c] = aq[c];
                }
        }
    }
}

// u[i, c] = z1[i, c] sqrt(invF_i / sigma2): the column phase's input for the square-root operator
__global__ __launch_bounds__(kBlock) void latent_scale_kernel(const double* __restrict__ invF,
                                                              const double* __restrict__ z1, double* __restrict__ u,
                                                              int64_t n, int nrhs, double inv_s2) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const double sc = sqrt(invF[i] * inv_s2);
        for (int c = 0; c < nrhs; ++c) u[i * nrhs + c] = z1[i * nrhs + c] * sc;
    }
}

// The row scale of a reference-set system: s_i = invF_i / sigma2 on a reference row, g_i = f_i d_i / (f_i + d_i)
// on a leaf row (exactly 0 where d_i = 0 or d is null: a leaf without data drops out)
__global__ __launch_bounds__(kBlock) void latent_ref_s_kernel(const double* __restrict__ invF,
                                                              const double* __restrict__ d, double* __restrict__ s,
                                                              int64_t n, int64_t n_s, double inv_s2) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const double f = invF[i] * inv_s2;
        double v = f;
        if (i >= n_s) {
            const double di = d != nullptr ? d[i] : 0.0;
            v = di == 0.0 ? 0.0 : f * di / (f + di);
        }
        s[i] = v;
    }
}

// The column phase's input over all n nodes for the two maps that start from a given vector z (n, nrhs):
//   FOLD   u = 0 on a reference row, -s z on a leaf row:        the column phase gives d_S z_S + B_L^T (g z_L)
//   !FOLD  u = sqrt(s) z on a reference row, -sqrt(s) z on a leaf row:  ... (I - B_S)^T f^1/2 z_S + B_L^T g^1/2 z_L
template <bool FOLD>
__global__ __launch_bounds__(kBlock) void latent_ref_scale_kernel(const double* __restrict__ s,
                                                                  const double* __restrict__ z,
                                                                  double* __restrict__ u, int64_t n, int64_t n_s,
                                                                  int nrhs) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const bool leaf = i >= n_s;
        const double a = FOLD ? s[i] : sqrt(s[i]);
        const double sc = leaf ? -a : (FOLD ? 0.0 : a);
        for (int c = 0; c < nrhs; ++c) u[i * nrhs + c] = z[i * nrhs + c] * sc;
    }
}

// ---------------------------------------------------------------- column phase
// out_i = t_i - sum_e Brev[e] t[rev_j[e]] + dd_i x_i, dd = d (kColSqrt: sqrt(d)); d null: no diagonal term.
// rec: null, or column c's record of sum_i x_i out_i (the CG's p.q) at rec[c * kMaxTileBlocks + blockIdx.x].
// REF: the nodes are the first n of the n_t that t covers (S = T: n_t is not read).
// kColDiag (one column, t = the row scale s): out_i = (s_i + sum_e Brev[e]^2 s[rev_j[e]]) + d_i, the diagonal of
// A_S, its sum in this phase's order.
enum { kColApply = 0, kColSqrt = 1, kColDiag = 2 };

template <int MODE, int KP, bool REF>
__global__ __launch_bounds__(kBlock) void latent_col_kernel(const int32_t* __restrict__ off,
                                                            const int32_t* __restrict__ rev_j,
                                                            const double* __restrict__ Brev,
                                                            const double* __restrict__ t,
                                                            const double* __restrict__ d,
                                                            const double* __restrict__ x, double* __restrict__ out,
                                                            int64_t n, int nrhs, double* __restrict__ rec,
                                                            const double* __restrict__ stop, int64_t n_t) {
    __shared__ int32_t sh_e0[kColRows], sh_e1[kColRows];
    __shared__ double sh4[4];
    constexpr bool SQRT = MODE == kColSqrt;
    if (stop != nullptr && *stop != 0.0) return;
    nrhs = columns<KP>(nrhs);
    const int64_t nt = REF ? n_t : n;  // rows of t
    const int g = threadIdx.x / kColLanes, l = threadIdx.x % kColLanes;
    int cc[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) cc[c] = column_of(c, nrhs);
    int64_t lo, hi;
    tile_range((n + kColRows - 1) / kColRows, &lo, &hi);
    double dot[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) dot[c] = 0.0;
    for (int64_t tile = lo; tile < hi; ++tile) {
        const int64_t i = tile * kColRows + g;
        const bool live = i < n;
        const int32_t e0 = live ? off[i] : 0, e1 = live ? off[i + 1] : 0;
        const bool is_long = e1 - e0 > kLongList;
        double acc[KP];
#pragma unroll
        for (int c = 0; c < KP; ++c) acc[c] = 0.0;
        if (!is_long) {
            for (int32_t e = e0 + l; e < e1; e += kColLanes) {
                const int32_t j = rev_j[e];
                if ((uint32_t)j < (uint64_t)nt) {
                    const double b = MODE == kColDiag ? Brev[e] * Brev[e] : Brev[e];
                    const double* tj = t + (int64_t)j * nrhs;
#pragma unroll
                    for (int c = 0; c < KP; ++c) acc[c] = fma(b, tj[cc[c]], acc[c]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < KP; ++c) acc[c] = lane_group_sum<kColLanes>(acc[c]);
        if (__syncthreads_or(is_long)) {  // block-uniform; rare (hubs)
            if (l == 0) {
                sh_e0[g] = e0;
                sh_e1[g] = is_long ? e1 : e0;
            }
            __syncthreads();
            for (int k = 0; k < kColRows; ++k) {
                const int32_t a0 = sh_e0[k], a1 = sh_e1[k];
                if (a1 <= a0) continue;  // block-uniform
                double s[KP];
#pragma unroll
                for (int c = 0; c < KP; ++c) s[c] = 0.0;
                for (int32_t e = a0 + (int32_t)threadIdx.x; e < a1; e += kBlock) {
                    const int32_t j = rev_j[e];
                    if ((uint32_t)j < (uint64_t)nt) {
                        const double b = MODE == kColDiag ? Brev[e] * Brev[e] : Brev[e];
                        const double* tj = t + (int64_t)j * nrhs;
#pragma unroll
                        for (int c = 0; c < KP; ++c) s[c] = fma(b, tj[cc[c]], s[c]);
                    }
                }
#pragma unroll
                for (int c = 0; c < KP; ++c) {
                    const double sc = block_sum(s[c], sh4);
                    if (g == k) acc[c] = sc;
                }
            }
            __syncthreads();
        }
        if (live && l == 0) {
            const bool want_x = (d != nullptr || rec != nullptr) && x != nullptr;
            double dd = 0.0;
            if (d != nullptr) dd = SQRT ? sqrt(d[i]) : d[i];
#pragma unroll
            for (int c = 0; c < KP; ++c) {
                if (MODE == kColDiag) {
                    out[i] = (t[i] + acc[c]) + dd;
                    continue;
                }
                double o = t[i * nrhs + cc[c]] - acc[c];
                const double xi = want_x ? x[i * nrhs + cc[c]] : 0.0;
                if (d != nullptr) o = fma(dd, xi, o);
                if (c < nrhs) out[i * nrhs + c] = o;
                dot[c] = fma(xi, o, dot[c]);
            }
        }
    }
    if (rec != nullptr) {
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            const double v = block_sum(dot[c], sh4);
            if (threadIdx.x == 0 && c < nrhs) rec[c * kMaxTileBlocks + blockIdx.x] = v;
        }
    }
}

// ---------------------------------------------------------------- the diagonal
// diag(A)_i = d_i + (invF_i + P_i) / sigma2, the Jacobi preconditioner's and nngp_precision_diag's.  One fused
// multiply-add, written out: it is what the compiler contracted the plain expression to, and every kernel that
// needs the diagonal must get these bits whatever its surroundings.
__device__ __forceinline__ double latent_diag(const double* __restrict__ d, const double* __restrict__ invF,
                                              const double* __restrict__ P, double inv_s2, int64_t i) {
    return fma(invF[i] + P[i], inv_s2, d != nullptr ? d[i] : 0.0);
}

// out_i = diag(A)_i
__global__ __launch_bounds__(kBlock) void latent_diag_kernel(int64_t n, const double* __restrict__ d,
                                                             const double* __restrict__ invF,
                                                             const double* __restrict__ P, double inv_s2,
                                                             double* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        out[i] = latent_diag(d, invF, P, inv_s2, i);
}

// ---------------------------------------------------------------- CG vector kernels
// nrhs recurrences in lock step.  Column c owns the state block st + c * kStateWords and the record rows
// rec + c * 3 * kMaxVecBlocks and pq_rec + c * kMaxTileBlocks.  A finished column (converged or broken down) is
// frozen: from then on none of its x, r, z, p or state is written.  M^-1 does not depend on the column.
//
// start: M^-1 = 1 / (d + (invF + P) / sigma2), r = b - A x0 (q holds A x0), z = M^-1 r, p = z; records of
// r.z, r.r and b.b.  REF: `P` is the diagonal of A_S itself (latent_col_kernel<kColDiag>), d and invF unread.
template <int KP, bool REF>
__global__ __launch_bounds__(kBlock) void latent_cg_init_kernel(
    int64_t n, int nrhs, const double* __restrict__ b, const double* __restrict__ q, const double* __restrict__ d,
    const double* __restrict__ invF, const double* __restrict__ P, double inv_s2, double* __restrict__ r,
    double* __restrict__ z, double* __restrict__ p, double* __restrict__ Minv, double* __restrict__ rec) {
    __shared__ double sh4[4];
    nrhs = columns<KP>(nrhs);
    int cc[KP];
    double rz[KP], rr[KP], bb[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        cc[c] = column_of(c, nrhs);
        rz[c] = rr[c] = bb[c] = 0.0;
    }
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const double mi = 1.0 / (REF ? P[i] : latent_diag(d, invF, P, inv_s2, i));
        Minv[i] = mi;
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            const int64_t e = i * nrhs + cc[c];
            const double bi = b[e], ri = bi - q[e], zi = mi * ri;
            if (c < nrhs) {
                r[e] = ri;
                z[e] = zi;
                p[e] = zi;
            }
            rz[c] = fma(ri, zi, rz[c]);
            rr[c] = fma(ri, ri, rr[c]);
            bb[c] = fma(bi, bi, bb[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        const double a0 = block_sum(rz[c], sh4), a1 = block_sum(rr[c], sh4), a2 = block_sum(bb[c], sh4);
        if (threadIdx.x == 0 && c < nrhs) {
            double* rc = rec + (size_t)c * 3 * kMaxVecBlocks;
            rc[blockIdx.x] = a0;
            rc[kMaxVecBlocks + blockIdx.x] = a1;
            rc[2 * kMaxVecBlocks + blockIdx.x] = a2;
        }
    }
}

// one block: fold each column's start records into its state
__global__ __launch_bounds__(kBlock) void latent_cg_start_kernel(const double* __restrict__ rec, int n_rec, int nrhs,
                                                                 double rtol, double* __restrict__ st) {
    __shared__ double sh4[4];
    double all = 1.0;
    for (int c = 0; c < nrhs; ++c) {
        const double* rc = rec + (size_t)c * 3 * kMaxVecBlocks;
        const double rz = fold_records(rc, n_rec, sh4);
        const double rr = fold_records(rc + kMaxVecBlocks, n_rec, sh4);
        const double bb = fold_records(rc + 2 * kMaxVecBlocks, n_rec, sh4);
        const double tol2 = rtol * rtol * bb;
        const double done = rr <= tol2 ? 1.0 : 0.0;
        if (done == 0.0) all = 0.0;
        if (threadIdx.x == 0) {
            double* sc = st + c * kStateWords;
            sc[kRz0] = rz;
            sc[kRz1] = 0.0;
            sc[kRr] = rr;
            sc[kBb] = bb;
            sc[kTol2] = tol2;
            sc[kAlpha] = sc[kBeta] = 0.0;
            sc[kIter] = 0.0;
            sc[kStatus] = done;
            sc[kFlag0] = done;
            sc[kFlag1] = 0.0;
            sc[kBrk] = 0.0;
        }
    }
    if (threadIdx.x == 0) {
        st[kAll0] = all;
        st[kAll1] = 0.0;
    }
}

// iteration k, after q = A p and the p.q records: per column alpha = r.z / p.q (a breakdown -- p.q not above 0
// or not finite -- is flagged in that column and nothing of it moves), x += alpha p, r -= alpha q, z = M^-1 r;
// records of r.z and r.r
template <int KP>
__global__ __launch_bounds__(kBlock) void latent_cg_update_kernel(
    int64_t n, int nrhs, int64_t k, const double* __restrict__ pq_rec, int n_pq, const double* __restrict__ p,
    const double* __restrict__ q, const double* __restrict__ Minv, double* __restrict__ x, double* __restrict__ r,
    double* __restrict__ z, double* __restrict__ rec, double* __restrict__ st) {
    __shared__ double sh4[4];
    const int cur = (int)(k & 1);
    nrhs = columns<KP>(nrhs);
    int cc[KP];
    bool act[KP];
    double alpha[KP], rz[KP], rr[KP];
    bool any = false;
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        cc[c] = column_of(c, nrhs);
        act[c] = false;
        alpha[c] = rz[c] = rr[c] = 0.0;
        if (c < nrhs) {  // block-uniform, as is everything read from the state
            double* sc = st + c * kStateWords;
            if (sc[kFlag0 + cur] == 0.0) {
                const double pq = fold_records(pq_rec + (size_t)c * kMaxTileBlocks, n_pq, sh4);
                if (!(pq > 0.0) || pq > 1.7976931348623157e308) {  // not above 0, NaN or +inf: this column only
                    if (blockIdx.x == 0 && threadIdx.x == 0) sc[kBrk] = 1.0;
                } else {
                    alpha[c] = sc[kRz0 + cur] / pq;
                    act[c] = any = true;
                }
            }
        }
    }
    if (!any) return;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const double mi = Minv[i];
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            const int64_t e = i * nrhs + cc[c];
            const double xe = fma(alpha[c], p[e], x[e]);
            const double ri = fma(-alpha[c], q[e], r[e]);
            const double zi = mi * ri;
            if (act[c]) {
                x[e] = xe;
                r[e] = ri;
                z[e] = zi;
            }
            rz[c] = fma(ri, zi, rz[c]);
            rr[c] = fma(ri, ri, rr[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        const double a0 = block_sum(rz[c], sh4), a1 = block_sum(rr[c], sh4);
        if (threadIdx.x == 0 && act[c]) {
            double* rc = rec + (size_t)c * 3 * kMaxVecBlocks;
            rc[blockIdx.x] = a0;
            rc[kMaxVecBlocks + blockIdx.x] = a1;
            if (blockIdx.x == 0) st[c * kStateWords + kAlpha] = alpha[c];
        }
    }
}

// iteration k, last launch: per column beta = r.z' / r.z, p = z + beta p; block 0 moves the states on (the
// scalars of iteration k + 1 live in the other slot, so no block reads a word this launch writes).
// trace: null, or (nrhs, trace_len, 2): the lead thread records (alpha_k, beta_k) of every column that completed
// iteration k at trace[c][k] -- the Lanczos tridiagonal of M^-1/2 A M^-1/2 (latent.h).  A frozen column and one that
// broke down in this iteration write nothing; nothing else of the launch depends on trace.
template <int KP>
__global__ __launch_bounds__(kBlock) void latent_cg_direction_kernel(int64_t n, int nrhs, int64_t k,
                                                                     const double* __restrict__ rec, int n_rec,
                                                                     const double* __restrict__ z,
                                                                     double* __restrict__ p, double* __restrict__ st,
                                                                     double* __restrict__ trace, int64_t trace_len) {
    __shared__ double sh4[4];
    nrhs = columns<KP>(nrhs);
    const int cur = (int)(k & 1), nxt = cur ^ 1;
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    int cc[KP];
    bool act[KP];
    double beta[KP];
    bool any = false, all_done = true;
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        cc[c] = column_of(c, nrhs);
        act[c] = false;
        beta[c] = 0.0;
        if (c < nrhs) {  // block-uniform
            double* sc = st + c * kStateWords;
            const double flag = sc[kFlag0 + cur];
            if (flag != 0.0) {
                if (lead) sc[kFlag0 + nxt] = flag;
            } else if (sc[kBrk] != 0.0) {
                if (lead) sc[kFlag0 + nxt] = sc[kStatus] = -1.0;
            } else {
                const double* rc = rec + (size_t)c * 3 * kMaxVecBlocks;
                const double rz = fold_records(rc, n_rec, sh4);
                const double rr = fold_records(rc + kMaxVecBlocks, n_rec, sh4);
                beta[c] = rz / sc[kRz0 + cur];
                act[c] = any = true;
                const bool done = rr <= sc[kTol2];
                if (!done) all_done = false;
                if (lead) {
                    sc[kRz0 + nxt] = rz;
                    sc[kRr] = rr;
                    sc[kBeta] = beta[c];
                    sc[kIter] = (double)(k + 1);
                    sc[kFlag0 + nxt] = sc[kStatus] = done ? 1.0 : 0.0;
                    if (trace != nullptr && k < trace_len) {
                        double* tr = trace + ((size_t)c * (size_t)trace_len + (size_t)k) * 2;
                        tr[0] = sc[kAlpha];  // the update launch of this iteration left it there
                        tr[1] = beta[c];
                    }
                }
            }
        }
    }
    if (lead) st[kAll0 + nxt] = all_done ? 1.0 : 0.0;
    if (!any) return;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            const int64_t e = i * nrhs + cc[c];
            const double pe = fma(beta[c], p[e], z[e]);
            if (act[c]) p[e] = pe;
        }
    }
}

// ---------------------------------------------------------------- the leaves given w_S
// Leaf j = n_s + r, r in [0, n_l): w_j | w_S, y ~ N((f_j a_j + d_j v_j) / (f_j + d_j), 1 / (f_j + d_j)), a_j =
// sum_s B[j,s] x[nbr[j,s]] in the row phase's lane groups and order, f_j = invF_j / sigma2.
//   out[r, c] = (f_j a_j + d_j v[r, c]) / (f_j + d_j)  [+ z[r, c] / sqrt(f_j + d_j)]
// v, z: (n_l, nrhs) or null (v null: 0).  d null: no data on any leaf, out = a_j as it stands (kriging of the
// nrhs fields x) [+ z / sqrt(f_j)].
template <int G, int KP>
__global__ __launch_bounds__(kBlock) void latent_leaf_kernel(const int32_t* __restrict__ nbr,
                                                             const double* __restrict__ B,
                                                             const double* __restrict__ invF,
                                                             const double* __restrict__ d,
                                                             const double* __restrict__ x,
                                                             const double* __restrict__ v,
                                                             const double* __restrict__ z, double* __restrict__ out,
                                                             int64_t n, int64_t n_s, int m, int nrhs, double inv_s2) {
    nrhs = columns<KP>(nrhs);
    constexpr int kRows = kBlock / G;
    const int g = threadIdx.x / G, l = threadIdx.x % G;
    const int64_t n_l = n - n_s;
    int cc[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) cc[c] = column_of(c, nrhs);
    int64_t lo, hi;
    tile_range((n_l + kRows - 1) / kRows, &lo, &hi);
    for (int64_t tile = lo; tile < hi; ++tile) {
        const int64_t r = tile * kRows + g, i = n_s + r;
        double acc[KP];
#pragma unroll
        for (int c = 0; c < KP; ++c) acc[c] = 0.0;
        if (r < n_l) {
            const int32_t* nb = nbr + i * m;
            const double* bb = B + i * m;
            for (int s = l; s < m; s += G) {
                const int32_t j = nb[s];
                if (j >= 0 && (int64_t)j < n_s) {
                    const double b = bb[s];
                    const double* xj = x + (int64_t)j * nrhs;
#pragma unroll
                    for (int c = 0; c < KP; ++c) acc[c] = fma(b, xj[cc[c]], acc[c]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < KP; ++c) acc[c] = lane_group_sum<G>(acc[c]);
        if (r < n_l && l == 0) {
            const double f = invF[i] * inv_s2;
            const double di = d != nullptr ? d[i] : 0.0;
            const double prec = f + di;
            const double sd = z != nullptr ? 1.0 / sqrt(prec) : 0.0;
#pragma unroll
            for (int c = 0; c < KP; ++c) {
                const int64_t e = r * nrhs + cc[c];
                double o = acc[c];
                if (d != nullptr) o = fma(f, acc[c], di * (v != nullptr ? v[e] : 0.0)) / prec;
                if (z != nullptr) o = fma(z[e], sd, o);
                if (c < nrhs) out[r * nrhs + c] = o;
            }
        }
    }
}

// ---------------------------------------------------------------- launches
int tile_blocks(int64_t n, int rows_per_tile) {
    const int64_t tiles = (n + rows_per_tile - 1) / rows_per_tile;
    return (int)(tiles < kMaxTileBlocks ? tiles : kMaxTileBlocks);
}

int vec_blocks(int64_t n) {
    const int64_t b = (n + kBlock - 1) / kBlock;
    return (int)(b < kMaxVecBlocks ? b : kMaxVecBlocks);
}

// KP: the padded column count of the instantiation that serves nrhs
#define NNGP_LATENT_KP(nrhs, ...) \
    do {                          \
        if ((nrhs) == 1) {        \
            constexpr int KP = 1; \
            __VA_ARGS__;          \
        } else if ((nrhs) <= 2) { \
            constexpr int KP = 2; \
            __VA_ARGS__;          \
        } else if ((nrhs) <= 4) { \
            constexpr int KP = 4; \
            __VA_ARGS__;          \
        } else {                  \
            constexpr int KP = 8; \
            __VA_ARGS__;          \
        }                         \
    } while (0)

// g.s != null: a reference-set system (the REF instantiations; vectors have g.n_s rows, t has g.n)
template <int KP, bool REF>
void row_launch_kp(const LatentGeom& g, int nrhs, const double* x, double* t, const double* stop, hipStream_t s) {
    const double inv_s2 = 1.0 / g.sigma2;
    const double* scale = REF ? g.s : g.prep.invF;
    // lanes per location from m alone (part of the fixed summation order)
    if (g.m <= 4)
        hipLaunchKernelGGL((latent_row_kernel<4, KP, REF>), dim3(tile_blocks(g.n, kBlock / 4)), dim3(kBlock), 0, s,
                           g.nbr, g.B, scale, x, t, g.n, g.m, nrhs, inv_s2, stop, g.n_s);
    else if (g.m <= 8)
        hipLaunchKernelGGL((latent_row_kernel<8, KP, REF>), dim3(tile_blocks(g.n, kBlock / 8)), dim3(kBlock), 0, s,
                           g.nbr, g.B, scale, x, t, g.n, g.m, nrhs, inv_s2, stop, g.n_s);
    else
        hipLaunchKernelGGL((latent_row_kernel<16, KP, REF>), dim3(tile_blocks(g.n, kBlock / 16)), dim3(kBlock), 0, s,
                           g.nbr, g.B, scale, x, t, g.n, g.m, nrhs, inv_s2, stop, g.n_s);
}

void row_launch(const LatentGeom& g, int nrhs, const double* x, double* t, const double* stop, hipStream_t s) {
    if (g.s != nullptr)
        NNGP_LATENT_KP(nrhs, row_launch_kp<KP, true>(g, nrhs, x, t, stop, s));
    else
        NNGP_LATENT_KP(nrhs, row_launch_kp<KP, false>(g, nrhs, x, t, stop, s));
}

// the vectors' row count: the nodes the column phase and the CG's vector kernels run over
int64_t vec_rows(const LatentGeom& g) { return g.s != nullptr ? g.n_s : g.n; }

template <int MODE>
void col_launch(const LatentGeom& g, int nrhs, const double* t, const double* x, double* out, double* rec,
                const double* stop, hipStream_t s) {
    if (g.s != nullptr)
        NNGP_LATENT_KP(nrhs, hipLaunchKernelGGL((latent_col_kernel<MODE, KP, true>),
                                                dim3(tile_blocks(g.n_s, kColRows)), dim3(kBlock), 0, s, g.off,
                                                g.rev_j, g.prep.Brev, t, g.d, x, out, g.n_s, nrhs, rec, stop, g.n));
    else
        NNGP_LATENT_KP(nrhs, hipLaunchKernelGGL((latent_col_kernel<MODE, KP, false>),
                                                dim3(tile_blocks(g.n, kColRows)), dim3(kBlock), 0, s, g.off, g.rev_j,
                                                g.prep.Brev, t, g.d, x, out, g.n, nrhs, rec, stop, g.n));
}

// reference-set systems: s for (theta, d), and diag(A_S) from it by the column phase
void ref_s_launch(const LatentGeom& g, double* sv, hipStream_t s) {
    hipLaunchKernelGGL(latent_ref_s_kernel, dim3(vec_blocks(g.n)), dim3(kBlock), 0, s, g.prep.invF, g.d, sv, g.n,
                       g.n_s, 1.0 / g.sigma2);
}

void ref_diag_launch(const LatentGeom& g, double* out, hipStream_t s) {
    hipLaunchKernelGGL((latent_col_kernel<kColDiag, 1, true>), dim3(tile_blocks(g.n_s, kColRows)), dim3(kBlock), 0,
                       s, g.off, g.rev_j, g.prep.Brev, g.s, g.d, (const double*)nullptr, out, g.n_s, 1,
                       (double*)nullptr, (const double*)nullptr, g.n);
}

// the CG workspace: six (n, nrhs) slots (M^-1, shared by the columns, uses n doubles of its own), kMaxRhs rows
// of records, kMaxRhs state blocks and the block of the two "all finished" words
struct CgLayout {
    double *t, *r, *z, *p, *q, *Minv, *rec, *pq_rec, *st;
    double *s, *diag;  // reference-set systems only
};

constexpr size_t kCgStateWords = (size_t)(kMaxRhs + 1) * kStateWords;
const size_t kCgTailBytes = align256((size_t)kMaxRhs * 3 * kMaxVecBlocks * 8) +
                            align256((size_t)kMaxRhs * kMaxTileBlocks * 8) + align256(kCgStateWords * 8);

void cg_layout_tail(CgLayout* L, char* w) {
    L->rec = (double*)w;
    w += align256((size_t)kMaxRhs * 3 * kMaxVecBlocks * 8);
    L->pq_rec = (double*)w;
    w += align256((size_t)kMaxRhs * kMaxTileBlocks * 8);
    L->st = (double*)w;
}

CgLayout cg_layout(void* workspace, int64_t n, int nrhs) {
    char* w = (char*)workspace;
    const size_t v = align256((size_t)n * nrhs * 8);
    CgLayout L;
    L.t = (double*)w;
    L.r = (double*)(w + v);
    L.z = (double*)(w + 2 * v);
    L.p = (double*)(w + 3 * v);
    L.q = (double*)(w + 4 * v);
    L.Minv = (double*)(w + 5 * v);
    L.s = L.diag = nullptr;
    cg_layout_tail(&L, w + 6 * v);
    return L;
}

// a reference-set system's: t (n, nrhs); r, z, p, q (n_s, nrhs); M^-1 and diag(A_S) (n_s,); s (n,); the tail
size_t ref_cg_head_bytes(int64_t n, int64_t n_s, int nrhs) {
    return align256((size_t)n * nrhs * 8) + 4 * align256((size_t)n_s * nrhs * 8) + 2 * align256((size_t)n_s * 8) +
           align256((size_t)n * 8);
}

CgLayout ref_cg_layout(void* workspace, int64_t n, int64_t n_s, int nrhs) {
    char* w = (char*)workspace;
    const size_t vt = align256((size_t)n * nrhs * 8), v = align256((size_t)n_s * nrhs * 8),
                 v1 = align256((size_t)n_s * 8);
    CgLayout L;
    L.t = (double*)w;
    w += vt;
    L.r = (double*)w;
    L.z = (double*)(w + v);
    L.p = (double*)(w + 2 * v);
    L.q = (double*)(w + 3 * v);
    w += 4 * v;
    L.Minv = (double*)w;
    L.diag = (double*)(w + v1);
    w += 2 * v1;
    L.s = (double*)w;
    w += align256((size_t)n * 8);
    cg_layout_tail(&L, w);
    return L;
}

// the recurrences on a geometry whose workspace is laid out (and, for a reference-set system, whose s and
// diag(A_S) are in place); vectors have vec_rows(g) rows
hipError_t cg_iterate(const LatentGeom& g, const CgLayout& L, int nrhs, const double* b, double* x, double rtol,
                      int64_t max_iter, int check_every, double* info_host, double* trace, int64_t trace_len,
                      hipStream_t s) {
    const int64_t nr = vec_rows(g);
    const int nv = vec_blocks(nr), nt = tile_blocks(nr, kColRows);
    const double inv_s2 = 1.0 / g.sigma2;
    hipError_t e;
    // r = b - A x0, z = M^-1 r, p = z, per column
    row_launch(g, nrhs, x, L.t, nullptr, s);
    col_launch<kColApply>(g, nrhs, L.t, x, L.q, nullptr, nullptr, s);
    if (g.s != nullptr)
        NNGP_LATENT_KP(nrhs, hipLaunchKernelGGL((latent_cg_init_kernel<KP, true>), dim3(nv), dim3(kBlock), 0, s, nr,
                                                nrhs, b, (const double*)L.q, g.d, g.prep.invF,
                                                (const double*)L.diag, inv_s2, L.r, L.z, L.p, L.Minv, L.rec));
    else
        NNGP_LATENT_KP(nrhs, hipLaunchKernelGGL((latent_cg_init_kernel<KP, false>), dim3(nv), dim3(kBlock), 0, s, nr,
                                                nrhs, b, (const double*)L.q, g.d, g.prep.invF, g.prep.P, inv_s2, L.r,
                                                L.z, L.p, L.Minv, L.rec));
    hipLaunchKernelGGL(latent_cg_start_kernel, dim3(1), dim3(kBlock), 0, s, (const double*)L.rec, nv, nrhs, rtol,
                       L.st);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    double st[kCgStateWords];
    int64_t k = 0;
    for (;;) {
        // one chunk: no host synchronisation inside; once every column is finished the launches are no-ops
        for (int c = 0; c < check_every && k < max_iter; ++c, ++k) {
            const double* stop = L.st + kAll0 + (k & 1);
            row_launch(g, nrhs, L.p, L.t, stop, s);
            col_launch<kColApply>(g, nrhs, L.t, L.p, L.q, L.pq_rec, stop, s);
            NNGP_LATENT_KP(nrhs, hipLaunchKernelGGL(latent_cg_update_kernel<KP>, dim3(nv), dim3(kBlock), 0, s, nr,
                                                    nrhs, k, (const double*)L.pq_rec, nt, (const double*)L.p,
                                                    (const double*)L.q, (const double*)L.Minv, x, L.r, L.z, L.rec,
                                                    L.st));
            NNGP_LATENT_KP(nrhs, hipLaunchKernelGGL(latent_cg_direction_kernel<KP>, dim3(nv), dim3(kBlock), 0, s,
                                                    nr, nrhs, k, (const double*)L.rec, nv, (const double*)L.z, L.p,
                                                    L.st, trace, trace_len));
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(st, L.st, sizeof st, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        if (st[kAll0 + (k & 1)] != 0.0 || k >= max_iter) break;
    }
    for (int c = 0; c < nrhs; ++c) {
        const double* sc = st + c * kStateWords;
        info_host[4 * c + 0] = sc[kIter];
        info_host[4 * c + 1] = sc[kStatus];
        info_host[4 * c + 2] = sc[kRr];
        info_host[4 * c + 3] = sc[kBb];
    }
    return hipSuccess;
}

void cg_info_clear(int nrhs, double* info_host) {
    for (int c = 0; c < nrhs; ++c) {
        info_host[4 * c + 0] = 0.0;
        info_host[4 * c + 1] = 1.0;
        info_host[4 * c + 2] = info_host[4 * c + 3] = 0.0;
    }
}

size_t max_size(size_t a, size_t b) { return a > b ? a : b; }

// t and s of an operator workspace; s is computed and g made a reference-set geometry
double* ref_begin(LatentGeom* g, int nrhs, void* workspace, hipStream_t s) {
    char* w = (char*)workspace;
    double* sv = (double*)(w + align256((size_t)g->n * nrhs * 8));
    ref_s_launch(*g, sv, s);
    g->s = sv;
    return (double*)w;
}

// Without a leaf (g.n_s == g.n) g.s stays null: the REF = false instantiations serve the call on prep's own
// scale, and the workspace is t alone.  These are the launches, and the bits, S = T always had.
bool leafless(const LatentGeom& g) { return g.n_s == g.n; }

double* op_begin(LatentGeom* g, int nrhs, void* workspace, hipStream_t s) {
    return leafless(*g) ? (double*)workspace : ref_begin(g, nrhs, workspace, s);
}

}  // namespace

size_t latent_apply_workspace_bytes(int64_t n, int nrhs) { return align256((size_t)(n > 0 ? n : 1) * nrhs * 8); }

size_t latent_cg_workspace_bytes(int64_t n, int nrhs) {
    return 6 * align256((size_t)n * nrhs * 8) + kCgTailBytes;
}

// with leaves the workspace starts with t (n, nrhs) and s (n,) (the CG's: ref_cg_layout)
size_t latent_ref_apply_workspace_bytes(int64_t n, int64_t n_s, int nrhs) {
    const size_t w = align256((size_t)(n > 0 ? n : 1) * nrhs * 8) + align256((size_t)(n > 0 ? n : 1) * 8);
    return n_s == n ? max_size(w, latent_apply_workspace_bytes(n, nrhs)) : w;
}

size_t latent_ref_cg_workspace_bytes(int64_t n, int64_t n_s, int nrhs) {
    const size_t w = ref_cg_head_bytes(n, n_s, nrhs) + kCgTailBytes;
    return n_s == n ? max_size(w, latent_cg_workspace_bytes(n, nrhs)) : w;
}

hipError_t latent_apply_launch(LatentGeom g, int nrhs, const double* x, double* out, void* workspace, hipStream_t s) {
    if (g.n_s == 0) return hipSuccess;
    double* t = op_begin(&g, nrhs, workspace, s);
    row_launch(g, nrhs, x, t, nullptr, s);
    col_launch<kColApply>(g, nrhs, t, x, out, nullptr, nullptr, s);
    return hipGetLastError();
}

hipError_t latent_sqrt_t_apply_launch(LatentGeom g, int nrhs, const double* z1, const double* z2, double* out,
                                      void* workspace, hipStream_t s) {
    if (g.n_s == 0) return hipSuccess;
    double* u = op_begin(&g, nrhs, workspace, s);
    if (leafless(g))
        hipLaunchKernelGGL(latent_scale_kernel, dim3(vec_blocks(g.n)), dim3(kBlock), 0, s, g.prep.invF, z1, u, g.n,
                           nrhs, 1.0 / g.sigma2);
    else
        hipLaunchKernelGGL(latent_ref_scale_kernel<false>, dim3(vec_blocks(g.n)), dim3(kBlock), 0, s, g.s, z1, u, g.n,
                           g.n_s, nrhs);
    col_launch<kColSqrt>(g, nrhs, u, z2, out, nullptr, nullptr, s);
    return hipGetLastError();
}

hipError_t latent_fold_launch(LatentGeom g, int nrhs, const double* v, double* out, void* workspace, hipStream_t s) {
    if (g.n_s == 0) return hipSuccess;
    double* u = ref_begin(&g, nrhs, workspace, s);
    hipLaunchKernelGGL(latent_ref_scale_kernel<true>, dim3(vec_blocks(g.n)), dim3(kBlock), 0, s, g.s, v, u, g.n,
                       g.n_s, nrhs);
    col_launch<kColApply>(g, nrhs, u, v, out, nullptr, nullptr, s);
    return hipGetLastError();
}

hipError_t latent_diag_launch(LatentGeom g, double* out, void* workspace, hipStream_t s) {
    if (g.n_s == 0) return hipSuccess;
    if (leafless(g)) {
        hipLaunchKernelGGL(latent_diag_kernel, dim3(vec_blocks(g.n)), dim3(kBlock), 0, s, g.n, g.d, g.prep.invF,
                           g.prep.P, 1.0 / g.sigma2, out);
    } else {
        ref_begin(&g, 1, workspace, s);
        ref_diag_launch(g, out, s);
    }
    return hipGetLastError();
}

hipError_t latent_cg_run(LatentGeom g, int nrhs, const double* b, double* x, double rtol, int64_t max_iter,
                         int check_every, double* info_host, void* workspace, hipStream_t s, double* trace,
                         int64_t trace_len) {
    cg_info_clear(nrhs, info_host);
    if (g.n_s == 0) return hipSuccess;
    if (leafless(g))
        return cg_iterate(g, cg_layout(workspace, g.n, nrhs), nrhs, b, x, rtol, max_iter, check_every, info_host,
                          trace, trace_len, s);
    const CgLayout L = ref_cg_layout(workspace, g.n, g.n_s, nrhs);
    ref_s_launch(g, L.s, s);
    g.s = L.s;
    ref_diag_launch(g, L.diag, s);
    return cg_iterate(g, L, nrhs, b, x, rtol, max_iter, check_every, info_host, trace, trace_len, s);
}

hipError_t latent_leaves_launch(const LatentGeom& g, int nrhs, const double* x, const double* v, const double* z,
                                double* out, hipStream_t s) {
    const int64_t n_l = g.n - g.n_s;
    if (n_l == 0) return hipSuccess;
    const double inv_s2 = 1.0 / g.sigma2;
    if (g.m <= 4)
        NNGP_LATENT_KP(nrhs, hipLaunchKernelGGL((latent_leaf_kernel<4, KP>), dim3(tile_blocks(n_l, kBlock / 4)),
                                                dim3(kBlock), 0, s, g.nbr, g.B, g.prep.invF, g.d, x, v, z, out, g.n,
                                                g.n_s, g.m, nrhs, inv_s2));
    else if (g.m <= 8)
        NNGP_LATENT_KP(nrhs, hipLaunchKernelGGL((latent_leaf_kernel<8, KP>), dim3(tile_blocks(n_l, kBlock / 8)),
                                                dim3(kBlock), 0, s, g.nbr, g.B, g.prep.invF, g.d, x, v, z, out, g.n,
                                                g.n_s, g.m, nrhs, inv_s2));
    else
        NNGP_LATENT_KP(nrhs, hipLaunchKernelGGL((latent_leaf_kernel<16, KP>), dim3(tile_blocks(n_l, kBlock / 16)),
                                                dim3(kBlock), 0, s, g.nbr, g.B, g.prep.invF, g.d, x, v, z, out, g.n,
                                                g.n_s, g.m, nrhs, inv_s2));
    return hipGetLastError();
}

hipError_t latent_rows_dot2_launch(const int32_t* nbr, const double* B, const double* dB, int64_t n, int64_t n_s,
                                   int m, int nrhs, const double* x, double* p, double* q, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (m <= 4)
        NNGP_LATENT_KP(nrhs, hipLaunchKernelGGL((latent_row_dot2_kernel<4, KP>), dim3(tile_blocks(n, kBlock / 4)),
                                                dim3(kBlock), 0, s, nbr, B, dB, x, p, q, n, n_s, m, nrhs));
    else if (m <= 8)
        NNGP_LATENT_KP(nrhs, hipLaunchKernelGGL((latent_row_dot2_kernel<8, KP>), dim3(tile_blocks(n, kBlock / 8)),
                                                dim3(kBlock), 0, s, nbr, B, dB, x, p, q, n, n_s, m, nrhs));
    else
        NNGP_LATENT_KP(nrhs, hipLaunchKernelGGL((latent_row_dot2_kernel<16, KP>), dim3(tile_blocks(n, kBlock / 16)),
                                                dim3(kBlock), 0, s, nbr, B, dB, x, p, q, n, n_s, m, nrhs));
    return hipGetLastError();
}

}  // namespace nngp
