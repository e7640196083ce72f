// Exact ordered neighbour sets for ordinates of dimension 4 .. 16, by tiled brute force.
//
// The ordering key is knn.hip's and sklearn's: the fp64 reduced distance rdist = ((0 + t0*t0) + t1*t1) + ... in axis
// order with contraction disabled, exact ties broken by the lower index, rows padded with -1 where fewer than m
// candidates exist.  A uniform grid does not pay in these dimensions (a cell's 3^d - 1 neighbours outnumber the
// points), so every query scans every candidate.
//
//   prior form  query row t is point i = q0 + t and searches coords[0 : i];
//   query form  query row t is query[q0 + t] and searches all n reference points (self included when it is there).
//
// A block owns kKnnNdQueries consecutive queries, one per lane, and streams the candidates through LDS in tiles of
// kKnnNdTile points; every lane reads the same tile entry at the same time (an LDS broadcast) and keeps its k best
// (rdist, j) in knn.hip's register-resident sorted list.  Points and queries are held as DP = 4, 8, 12 or 16
// coordinates, the missing ones 0: a padded term adds +0.0 to a non-negative sum, so the key is unchanged.  In the
// prior form a block stops at the tile that holds its last query, and the blocks are issued heaviest first (the last
// rows do N times the work of the first), so the tail of the grid is made of the light blocks.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "bf_nd.h"

namespace nngp {

__device__ __forceinline__ bool nd_key_less(double da, int32_t ia, double db, int32_t ib) {
    return da < db || (da == db && ia < ib);
}

// knn.hip's sorted list: real entries occupy [KMAX-k, KMAX), the slots below hold (-inf, -1) sentinels that never
// move, so the worst kept entry is always slot KMAX-1 (static register indexing throughout).
template <int KMAX>
struct NdTopK {
    double d[KMAX];
    int32_t j[KMAX];
    __device__ __forceinline__ void init(int k) {
#pragma unroll
        for (int s = 0; s < KMAX; ++s) {
            const bool real = s >= KMAX - k;
            d[s] = real ? INFINITY : -INFINITY;
            j[s] = real ? INT32_MAX : -1;
        }
    }
    __device__ __forceinline__ void push(double dc, int32_t jc) {
        if (!nd_key_less(dc, jc, d[KMAX - 1], j[KMAX - 1])) return;
#pragma unroll
        for (int s = KMAX - 1; s > 0; --s) {
            const bool below = nd_key_less(dc, jc, d[s - 1], j[s - 1]);
            const bool here = !below && nd_key_less(dc, jc, d[s], j[s]);
            const double nd = below ? d[s - 1] : (here ? dc : d[s]);
            const int32_t nj = below ? j[s - 1] : (here ? jc : j[s]);
            d[s] = nd;
            j[s] = nj;
        }
        if (nd_key_less(dc, jc, d[0], j[0])) {
            d[0] = dc;
            j[0] = jc;
        }
    }
};

template <int DP>
__device__ __forceinline__ double nd_rdist(const double (&q)[DP], const double* __restrict__ p) {
#pragma clang fp contract(off)
    double d = 0.0;
#pragma unroll
    for (int k = 0; k < DP; ++k) {
        const double t = q[k] - p[k];
        d = d + t * t;
    }
    return d;
}

template <int KMAX, bool PRIOR, int DP>
__global__ __launch_bounds__(kKnnNdQueries) void knn_nd_kernel(const double* __restrict__ coords, int64_t n, int dim,
                                                               int m, const double* __restrict__ query, int64_t q0,
                                                               int64_t q1, int32_t* __restrict__ nbr) {
    __shared__ double tile[kKnnNdTile * DP];
    // heaviest block first: block 0 takes the last queries
    const int64_t qb = q0 + (int64_t)(gridDim.x - 1 - blockIdx.x) * kKnnNdQueries;
    const int64_t i = qb + threadIdx.x;  // this lane's query
    const bool live = i < q1;
    const int64_t limit = live ? (PRIOR ? i : n) : 0;  // candidates are reference points j < limit
    const int k = (int)(limit < m ? limit : m);
    double q[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) q[c] = (live && c < dim) ? (PRIOR ? coords : query)[i * dim + c] : 0.0;
    NdTopK<KMAX> top;
    top.init(k);
    // candidates of the whole block: the prior form's last live query bounds them
    const int64_t last = (qb + kKnnNdQueries < q1 ? qb + kKnnNdQueries : q1) - 1;
    const int64_t jend = PRIOR ? last : n;
    for (int64_t base = 0; base < jend; base += kKnnNdTile) {
        __syncthreads();  // the previous tile is read
        for (int e = threadIdx.x; e < kKnnNdTile * DP; e += kKnnNdQueries) {
            const int64_t j = base + e / DP;
            const int c = e % DP;
            tile[e] = (j < jend && c < dim) ? coords[j * dim + c] : 0.0;
        }
        __syncthreads();
        const int64_t rest = jend - base;
        const int cnt = (int)(rest < kKnnNdTile ? rest : kKnnNdTile);
        if (base < limit) {
            for (int jj = 0; jj < cnt; ++jj) {
                const int64_t j = base + jj;
                if (j < limit) top.push(nd_rdist<DP>(q, tile + jj * DP), (int32_t)j);
            }
        }
    }
    if (!live) return;
    int32_t* out = nbr + (i - q0) * m;
#pragma unroll
    for (int s = 0; s < KMAX; ++s) {
        const int o = s - (KMAX - k);
        if (o >= 0) out[o] = top.j[s];
    }
    for (int s = k; s < m; ++s) out[s] = -1;
}

template <int KMAX, int DP>
static void knn_nd_go(bool prior, const double* coords, int64_t n, int dim, int m, const double* query, int64_t q0,
                      int64_t q1, int32_t* nbr, hipStream_t s) {
    const dim3 grid((unsigned)((q1 - q0 + kKnnNdQueries - 1) / kKnnNdQueries)), block(kKnnNdQueries);
    if (prior)
        hipLaunchKernelGGL((knn_nd_kernel<KMAX, true, DP>), grid, block, 0, s, coords, n, dim, m, query, q0, q1, nbr);
    else
        hipLaunchKernelGGL((knn_nd_kernel<KMAX, false, DP>), grid, block, 0, s, coords, n, dim, m, query, q0, q1, nbr);
}

template <int DP>
static hipError_t knn_nd_k(bool prior, const double* coords, int64_t n, int dim, int m, const double* query, int64_t q0,
                           int64_t q1, int32_t* nbr, hipStream_t s) {
    if (m <= 8)
        knn_nd_go<8, DP>(prior, coords, n, dim, m, query, q0, q1, nbr, s);
    else if (m <= 16)
        knn_nd_go<16, DP>(prior, coords, n, dim, m, query, q0, q1, nbr, s);
    else if (m <= 32)
        knn_nd_go<32, DP>(prior, coords, n, dim, m, query, q0, q1, nbr, s);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t knn_nd_launch(bool prior, const double* coords, int64_t n, int dim, int m, const double* query, int64_t q0,
                         int64_t q1, int32_t* nbr, hipStream_t s) {
    if (dim < kNdMinDim || dim > kNdMaxDim || m < 1) return hipErrorInvalidValue;
    if (q1 <= q0) return hipSuccess;
    if (dim <= 4) return knn_nd_k<4>(prior, coords, n, dim, m, query, q0, q1, nbr, s);
    if (dim <= 8) return knn_nd_k<8>(prior, coords, n, dim, m, query, q0, q1, nbr, s);
    if (dim <= 12) return knn_nd_k<12>(prior, coords, n, dim, m, query, q0, q1, nbr, s);
    return knn_nd_k<16>(prior, coords, n, dim, m, query, q0, q1, nbr, s);
}

}  // namespace nngp
