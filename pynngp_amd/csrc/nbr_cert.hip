// Device passes of nngp_nbr_cert_build (nbr_cert.h): the checked-tile bits of a neighbour set and the
// bounding box of its coordinates.  A set-up call, run once per neighbour set.
#include <hip/hip_runtime.h>

#include "bf_pairb.h"
#include "nbr_cert.h"
#include "nngp_internal.h"

namespace nngp {

static_assert(kCertTileRows == kPairbTile && kCertMaxM == kPairbCertMaxM, "nbr_cert.h mirrors bf_pairb.h");

// one block per tile, one thread per row: a tile is checked when any slot of its rows is
__global__ __launch_bounds__(kCertTileRows) void cert_tiles_kernel(const int32_t* __restrict__ nbr, int64_t n_rows,
                                                                   int m, int64_t n_points, int64_t tq, int64_t trem,
                                                                   uint32_t* __restrict__ mask,
                                                                   int32_t* __restrict__ n_checked) {
    const int64_t t = blockIdx.x;
    const int64_t r = t * tq + (t < trem ? t : trem) + threadIdx.x;  // (cert_tile_row0, a host function)
    const bool live = (int64_t)threadIdx.x < tq + (t < trem ? 1 : 0) && r < n_rows;
    bool any = false;
    if (live) {
        const int32_t* row = nbr + r * m;
        for (int s = 0; s < m; ++s) any |= cert_slot_checked(row[s], n_points);
    }
    if (__syncthreads_or(any ? 1 : 0) != 0 && threadIdx.x == 0) {
        atomicOr(&mask[t >> 5], 1u << (t & 31));
        atomicAdd(n_checked, 1);
    }
}

// per-dimension min / max of the coordinates and whether any is not finite: block b's record at rec + 8 b
__global__ __launch_bounds__(256) void cert_span_kernel(const double* __restrict__ coords, int64_t n_points, int dim,
                                                        double* __restrict__ rec) {
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY}, bad = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_points; p += (int64_t)gridDim.x * 256) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c < dim) {
                const double x = coords[p * dim + c];
                if (!isfinite(x)) bad = 1.0;
                mn[c] = fmin(mn[c], x);
                mx[c] = fmax(mx[c], x);
            }
        }
    }
    __shared__ double sh[4][8];
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mn[c] = wave_min(mn[c]);
        mx[c] = -wave_min(-mx[c]);
    }
    bad = -wave_min(-bad);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            sh[w][c] = mn[c];
            sh[w][3 + c] = mx[c];
        }
        sh[w][6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* o = rec + 8 * (int64_t)blockIdx.x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o[c] = fmin(fmin(sh[0][c], sh[1][c]), fmin(sh[2][c], sh[3][c]));
            o[3 + c] = fmax(fmax(sh[0][3 + c], sh[1][3 + c]), fmax(sh[2][3 + c], sh[3][3 + c]));
        }
        o[6] = fmax(fmax(sh[0][6], sh[1][6]), fmax(sh[2][6], sh[3][6]));
        o[7] = 0.0;
    }
}

hipError_t nbr_cert_launch(const double* coords, int64_t n_points, int dim, const int32_t* nbr, int64_t n_rows, int m,
                           void* cert, hipStream_t s) {
    const PairbTiling tl = pairb_tiling(n_rows, m, 0);
    if (tl.tiles != cert_tiles(n_rows)) return hipErrorInvalidValue;
    char* base = (char*)cert;
    hipError_t e = hipMemsetAsync(base, 0, cert_span_off(tl.tiles), s);  // the header and the bits
    if (e != hipSuccess) return e;
    if (tl.tiles > 0) {
        hipLaunchKernelGGL(cert_tiles_kernel, dim3((unsigned)tl.tiles), dim3(kCertTileRows), 0, s, nbr, n_rows, m, n_points,
                           tl.q, tl.rem, (uint32_t*)(base + kCertMaskOff), (int32_t*)base);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(cert_span_kernel, dim3(kCertSpanBlocks), dim3(256), 0, s, coords, n_points, dim,
                       (double*)(base + cert_span_off(tl.tiles)));
    return hipGetLastError();
}

}  // namespace nngp
