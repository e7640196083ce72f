// Multivariate gradient sweep (bf_mv_grad.h): dispatch over the instantiation units and the fixed-order fold of the
// per-location records of nrec = 4 + P doubles.  The records are indexed by location, so the fold does not depend on
// `order`: chunks of kMvGradChunk consecutive locations first (a block each), then the chunk records in one block.
#include "bf_mv_grad.h"

namespace nngp {

// Block c folds locations [c kMvGradChunk, (c + 1) kMvGradChunk): one component of the record at a time, thread t
// adds rows t, t + 256, ..., then a fixed xor-butterfly inside each wave and a fixed fold over the 4 waves.
__global__ __launch_bounds__(256) void bf_mv_grad_chunks(const double* __restrict__ rows, int64_t n_rows, int nrec,
                                                         double* __restrict__ crec) {
    __shared__ double sh[4];
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kMvGradChunk;
    for (int c = 0; c < nrec; ++c) {
        const bool mn = c == 2 || c == 3;
        double a = mn ? INFINITY : 0.0;
        for (int u = 0; u < kMvGradChunk / 256; ++u) {
            const int64_t r = r0 + t + 256 * u;
            if (r < n_rows) {
                const double v = rows[r * nrec + c];
                a = mn ? fmin(a, v) : a + v;
            }
        }
        a = mn ? wave_min(a) : wave_sum(a);
        if ((t & 63) == 0) sh[t >> 6] = a;
        __syncthreads();
        if (t == 0) {
            a = mn ? INFINITY : 0.0;
            for (int w = 0; w < 4; ++w) a = mn ? fmin(a, sh[w]) : a + sh[w];
            crec[(int64_t)blockIdx.x * nrec + c] = a;
        }
        __syncthreads();
    }
}

// bf_nd_finalize's fold over the chunk records: thread t folds records t, t + 1024, ...; a fixed butterfly inside each
// wave and a fixed fold over the 16 waves.  grad takes the P gradient sums.
__global__ __launch_bounds__(1024) void bf_mv_grad_finalize(const double* __restrict__ crec, int64_t n_chunks, int nrec,
                                                            double* __restrict__ partials, double* __restrict__ grad) {
    __shared__ double sh[16];
    const int t = threadIdx.x;
    for (int c = 0; c < nrec; ++c) {
        const bool mn = c == 2 || c == 3;
        double a = mn ? INFINITY : 0.0;
        for (int64_t k = t; k < n_chunks; k += 1024) {
            const double v = crec[(int64_t)nrec * k + c];
            a = mn ? fmin(a, v) : a + v;
        }
        a = mn ? wave_min(a) : wave_sum(a);
        if ((t & 63) == 0) sh[t >> 6] = a;
        __syncthreads();
        if (t == 0) {
            a = mn ? INFINITY : 0.0;
            for (int w = 0; w < 16; ++w) a = mn ? fmin(a, sh[w]) : a + sh[w];
            if (c < 2)
                partials[c] = a;
            else if (c < 4)
                partials[c] = a == INFINITY ? -1.0 : a;
            else
                grad[c - 4] = a;
        }
        __syncthreads();
    }
}

hipError_t bf_mv_grad_launch(const MvGradArgs& a, double* partials, double* grad, hipStream_t s) {
    const int nrec = 4 + mv_grad_len(a.q);
    double* crec = (double*)((char*)a.rows + mv_grad_rows_bytes(a.n_rows, a.q));
    const int64_t nc = mv_grad_chunks(a.n_rows);
    if (a.n_rows > 0) {
        if (!(bf_mv_grad_launch_q2(a, s) || bf_mv_grad_launch_q3(a, s) || bf_mv_grad_launch_q4(a, s)))
            return hipErrorInvalidValue;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(bf_mv_grad_chunks, dim3((unsigned)nc), dim3(256), 0, s, a.rows, a.n_rows, nrec, crec);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(bf_mv_grad_finalize, dim3(1), dim3(1024), 0, s, crec, nc, nrec, partials, grad);
    return hipGetLastError();
}

}  // namespace nngp
