// Whitening of several columns by a stored NNGP factor, and the Gram matrix of the whitened columns:
//   U[t, c] = (self[t, c] - sum_s B[t,s] V[nbr[t,s], c]) / sqrt(F[t]),   G[a, b] = sum_t U[t,a] U[t,b]
// for 1 <= ncol <= 16 columns V (n_points, ncol) row-major.  B, F and nbr are read as nngp_bf_sweep /
// nngp_bf_cross / nngp_bf_sweep_blocks wrote them (any kind, any 1 <= m <= NNGP_MAX_M: nothing here is a
// template on m or kind).  With [y, X] as the columns, G holds y'Qy, X'Qy and X'QX of the NNGP precision
// Q = (I - B)^T F^-1 (I - B): GLS, the profile and restricted likelihoods, universal kriging and the conjugate
// NNGP all follow from it on the host (pynngp_amd/regression.py).
//
// Whitening: one lane per (row, column), the KP = 1, 2, 4, 8 or 16 lanes of a row side by side (KP: the smallest
// that holds ncol).  A lane walks the row's m slots in slot order, one fma per slot, so a column's chain is one
// thread's and its bits depend on neither ncol nor the other columns.  The lanes of a row read the same index
// and coefficient (one fetch, broadcast) and gather ncol contiguous doubles of V's row: a 128-byte segment at 16
// columns.  A slot that is negative or >= n_points adds exactly 0 (it is skipped: a NaN coefficient there does
// not reach the sum).  A row whose F is NaN or not positive gets NaN.
//
// Gram: U is re-read in tiles of 1,024 rows, one block per tile, staged through LDS 256 rows at a time (2 KiB
// per column).  Thread p of the block owns pair p = (a, b), a <= b, and sums it over the tile's rows in row
// order on four interleaved chains (row mod 4), one fma per row, folded ((0 + 1) + (2 + 3)) into the tile's
// record: 136 accumulators spread over 136 threads, four registers each.  Rows past n_rows are staged as 0 and
// add exactly 0.  One block then folds the records in tile order, thread p its pair (32 loads in flight, the adds
// in order), and writes both triangles.
// The order of every sum depends on n_rows alone -- not on ncol, on which columns sit beside (a, b), on the
// grid or on timing: no atomics, no flags.  So G[a, b] is the bits of the two-column call on (a, b), a NaN in
// column c stays in row and column c, and every output repeats run to run.
#include "whiten_gram.h"

#include <math.h>

namespace nngp {

namespace {

constexpr int kBlock = 256;

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

template <int KP>
__global__ __launch_bounds__(kBlock) void whiten_kernel(const int32_t* __restrict__ nbr,
                                                        const int32_t* __restrict__ order,
                                                        const double* __restrict__ B, const double* __restrict__ F,
                                                        const double* __restrict__ V, const double* __restrict__ Vq,
                                                        double* __restrict__ U, int64_t n_rows, int m, int64_t i0,
                                                        int64_t n_points, int ncol) {
    constexpr int kRows = kBlock / KP;
    const int64_t t = (int64_t)blockIdx.x * kRows + threadIdx.x / KP;
    const int c = threadIdx.x % KP;
    if (t >= n_rows || c >= ncol) return;
    const int64_t r = order != nullptr ? (int64_t)order[t] : t;
    if (r < 0 || r >= n_rows) return;  // not a row of this sweep: nothing is read or written for it
    const int32_t* nb = nbr + t * m;
    const double* bb = B + r * m;
    double acc = 0.0;
    for (int s = 0; s < m; ++s) {
        const int32_t j = nb[s];
        if (j >= 0 && (int64_t)j < n_points) acc = fma(bb[s], V[(int64_t)j * ncol + c], acc);
    }
    const double self = Vq != nullptr ? Vq[r * ncol + c] : V[(i0 + r) * ncol + c];
    const double f = F[r];
    U[r * ncol + c] = f > 0.0 ? (self - acc) / sqrt(f) : (double)NAN;
}

// pair p of the upper triangle, row by row: (0,0), (0,1), .., (0,ncol-1), (1,1), ..
__device__ __forceinline__ void pair_of(int p, int ncol, int* a, int* b) {
    int row = 0, len = ncol;
    while (p >= len) {
        p -= len;
        ++row;
        --len;
    }
    *a = row;
    *b = row + p;
}

__global__ __launch_bounds__(kBlock) void gram_tile_kernel(const double* __restrict__ U, int64_t n_rows, int ncol,
                                                           double* __restrict__ rec) {
    extern __shared__ double lds[];  // (kGramChunkRows, ncol)
    const int npairs = ncol * (ncol + 1) / 2;
    const int p = threadIdx.x;
    int a = 0, b = 0;
    if (p < npairs) pair_of(p, ncol, &a, &b);
    const int64_t row0 = (int64_t)blockIdx.x * kGramTileRows;
    const int64_t n_val = n_rows * ncol;
    const int chunk_val = kGramChunkRows * ncol;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int ch = 0; ch < kGramTileRows / kGramChunkRows; ++ch) {
        const int64_t base = (row0 + (int64_t)ch * kGramChunkRows) * ncol;
        if (base >= n_val) break;  // block-uniform
        __syncthreads();
        for (int k = threadIdx.x; k < chunk_val; k += kBlock) lds[k] = base + k < n_val ? U[base + k] : 0.0;
        __syncthreads();
        if (p < npairs) {
            const double* ua = lds + a;
            const double* ub = lds + b;
#pragma unroll 2
            for (int r = 0; r < kGramChunkRows; r += 4) {
                a0 = fma(ua[(r + 0) * ncol], ub[(r + 0) * ncol], a0);
                a1 = fma(ua[(r + 1) * ncol], ub[(r + 1) * ncol], a1);
                a2 = fma(ua[(r + 2) * ncol], ub[(r + 2) * ncol], a2);
                a3 = fma(ua[(r + 3) * ncol], ub[(r + 3) * ncol], a3);
            }
        }
    }
    if (p < npairs) rec[(int64_t)blockIdx.x * npairs + p] = (a0 + a1) + (a2 + a3);
}

// one block: thread p folds pair p's records in tile order and writes both triangles
__global__ __launch_bounds__(kBlock) void gram_fold_kernel(const double* __restrict__ rec, int64_t n_tiles, int ncol,
                                                           double* __restrict__ gram) {
    const int npairs = ncol * (ncol + 1) / 2;
    const int p = threadIdx.x;
    if (p >= npairs) return;
    int a, b;
    pair_of(p, ncol, &a, &b);
    // the adds stay in tile order; the loads of kFoldBatch records are issued together, so the chain waits for
    // memory once per batch instead of once per record
    constexpr int kFoldBatch = 32;
    double s = 0.0;
    int64_t k = 0;
    for (; k + kFoldBatch <= n_tiles; k += kFoldBatch) {
        double v[kFoldBatch];
#pragma unroll
        for (int j = 0; j < kFoldBatch; ++j) v[j] = rec[(k + j) * npairs + p];
#pragma unroll
        for (int j = 0; j < kFoldBatch; ++j) s += v[j];
    }
    for (; k < n_tiles; ++k) s += rec[k * npairs + p];
    gram[a * ncol + b] = s;
    gram[b * ncol + a] = s;
}

template <int KP>
void whiten_launch(const WhitenArgs& a, double* U, hipStream_t s) {
    constexpr int kRows = kBlock / KP;
    const int64_t blocks = (a.n_rows + kRows - 1) / kRows;
    hipLaunchKernelGGL((whiten_kernel<KP>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a.nbr, a.order, a.B, a.F, a.V,
                       a.Vq, U, a.n_rows, a.m, a.i0, a.n_points, a.ncol);
}

}  // namespace

int64_t whiten_gram_tiles(int64_t n_rows) { return (n_rows + kGramTileRows - 1) / kGramTileRows; }

size_t whiten_gram_workspace_bytes(int64_t n_rows, int ncol) {
    if (n_rows < 0 || ncol < 1 || ncol > kWhitenMaxCols) return 0;
    const size_t rec = (size_t)whiten_gram_tiles(n_rows) * (size_t)(ncol * (ncol + 1) / 2) * sizeof(double);
    return align256(rec > 0 ? rec : 1);
}

hipError_t whiten_gram_launch(const WhitenArgs& a, double* U, double* gram, void* workspace, hipStream_t s) {
    if (a.n_rows == 0)
        return gram != nullptr ? hipMemsetAsync(gram, 0, sizeof(double) * a.ncol * a.ncol, s) : hipSuccess;
    if (a.ncol == 1) whiten_launch<1>(a, U, s);
    else if (a.ncol == 2) whiten_launch<2>(a, U, s);
    else if (a.ncol <= 4) whiten_launch<4>(a, U, s);
    else if (a.ncol <= 8) whiten_launch<8>(a, U, s);
    else whiten_launch<16>(a, U, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || gram == nullptr) return e;
    const int64_t n_tiles = whiten_gram_tiles(a.n_rows);
    double* rec = (double*)workspace;
    hipLaunchKernelGGL(gram_tile_kernel, dim3((unsigned)n_tiles), dim3(kBlock),
                       (size_t)kGramChunkRows * a.ncol * sizeof(double), s, U, a.n_rows, a.ncol, rec);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gram_fold_kernel, dim3(1), dim3(kBlock), 0, s, rec, n_tiles, a.ncol, gram);
    return hipGetLastError();
}

}  // namespace nngp
