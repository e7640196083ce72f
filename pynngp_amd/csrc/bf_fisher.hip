// Fisher information sweep (bf_fisher.h): dispatch over the instantiation units and the fixed-order fold of the
// per-block records into partials[4], grad[3] and info[6].
#include "bf_fisher.h"

namespace nngp {

// Thread t folds records t, t + 1024, ...; then a fixed xor-butterfly inside each wave and a fixed fold over
// the 16 waves (bf_finalize's order, with the gradient and information sums alongside): two runs give
// identical bits.
__global__ __launch_bounds__(1024) void bf_fisher_finalize(const double* __restrict__ rec, int64_t n_blocks,
                                                           double* __restrict__ partials, double* __restrict__ grad,
                                                           double* __restrict__ info) {
    __shared__ double sh[16][kFisherRec];
    const int t = threadIdx.x;
    double v[kFisherRec];
#pragma unroll
    for (int j = 0; j < kFisherRec; ++j) v[j] = (j == 2 || j == 3) ? INFINITY : 0.0;
    for (int64_t k = t; k < n_blocks; k += 1024) {
        const double* p = rec + kFisherRec * k;
#pragma unroll
        for (int j = 0; j < kFisherRec; ++j) v[j] = (j == 2 || j == 3) ? fmin(v[j], p[j]) : v[j] + p[j];
    }
#pragma unroll
    for (int j = 0; j < kFisherRec; ++j) v[j] = (j == 2 || j == 3) ? wave_min(v[j]) : wave_sum(v[j]);
    if ((t & 63) == 0) {
#pragma unroll
        for (int j = 0; j < kFisherRec; ++j) sh[t >> 6][j] = v[j];
    }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int j = 0; j < kFisherRec; ++j) v[j] = (j == 2 || j == 3) ? INFINITY : 0.0;
        for (int w = 0; w < 16; ++w) {
#pragma unroll
            for (int j = 0; j < kFisherRec; ++j) v[j] = (j == 2 || j == 3) ? fmin(v[j], sh[w][j]) : v[j] + sh[w][j];
        }
        partials[0] = v[0];
        partials[1] = v[1];
        partials[2] = v[2] == INFINITY ? -1.0 : v[2];
        partials[3] = v[3] == INFINITY ? -1.0 : v[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) grad[j] = v[4 + j];
#pragma unroll
        for (int j = 0; j < 6; ++j) info[j] = v[7 + j];
    }
}

hipError_t bf_fisher_launch(const FisherArgs& a, double* partials, double* grad, double* info, hipStream_t s) {
    int64_t nb = 0;
    if (a.n_rows > 0) {
        nb = bf_grad_blocks(a.n_rows, a.m);
        if (!(bf_fisher_launch_a(a, s) || bf_fisher_launch_b(a, s) || bf_fisher_launch_c(a, s) ||
              bf_fisher_launch_d(a, s) || bf_fisher_launch_e(a, s) || bf_fisher_launch_f(a, s) ||
              bf_fisher_launch_g(a, s) || bf_fisher_launch_h(a, s)))
            return hipErrorInvalidValue;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(bf_fisher_finalize, dim3(1), dim3(1024), 0, s, a.rec, nb, partials, grad, info);
    return hipGetLastError();
}

}  // namespace nngp
