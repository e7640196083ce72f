// Gneiting space-time sweeps (bf_gneiting.h): dispatch over the instantiation units and the fixed-order folds of
// the per-block records -- bf_finalize's for the forward sweep, bf_sep_finalize's order with five gradient sums
// for the gradient.
#include "bf_gneiting.h"

namespace nngp {

// Thread t folds records t, t + 1024, ...; then a fixed xor-butterfly inside each wave and a fixed fold over
// the 16 waves: two runs give identical bits.  grad takes (sigma2, c, a, beta, tau2).
__global__ __launch_bounds__(1024) void bf_gneiting_finalize(const double* __restrict__ rec, int64_t n_blocks,
                                                             double* __restrict__ partials,
                                                             double* __restrict__ grad) {
    __shared__ double sh[16][kGnRec];
    const int t = threadIdx.x;
    double a = 0.0, b = 0.0, c = INFINITY, d = INFINITY, g[kGnSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t k = t; k < n_blocks; k += 1024) {
        const double* o = rec + kGnRec * k;
        a += o[0];
        b += o[1];
        c = fmin(c, o[2]);
        d = fmin(d, o[3]);
#pragma unroll
        for (int j = 0; j < kGnSums; ++j) g[j] += o[4 + j];
    }
    a = wave_sum(a);
    b = wave_sum(b);
    c = wave_min(c);
    d = wave_min(d);
#pragma unroll
    for (int k = 0; k < kGnSums; ++k) g[k] = wave_sum(g[k]);
    if ((t & 63) == 0) {
        double* o = sh[t >> 6];
        o[0] = a;
        o[1] = b;
        o[2] = c;
        o[3] = d;
#pragma unroll
        for (int k = 0; k < kGnSums; ++k) o[4 + k] = g[k];
    }
    __syncthreads();
    if (t == 0) {
        a = 0.0, b = 0.0, c = INFINITY, d = INFINITY;
        for (int k = 0; k < kGnSums; ++k) g[k] = 0.0;
        for (int w = 0; w < 16; ++w) {
            a += sh[w][0];
            b += sh[w][1];
            c = fmin(c, sh[w][2]);
            d = fmin(d, sh[w][3]);
            for (int k = 0; k < kGnSums; ++k) g[k] += sh[w][4 + k];
        }
        partials[0] = a;
        partials[1] = b;
        partials[2] = c == INFINITY ? -1.0 : c;
        partials[3] = d == INFINITY ? -1.0 : d;
        for (int k = 0; k < kGnSums; ++k) grad[k] = g[k];
    }
}

hipError_t bf_gneiting_launch(const GneitingArgs& a, double* partials, double* grad, hipStream_t s) {
    const bool g = grad != nullptr;
    int64_t nb = 0;
    if (a.n_rows > 0) {
        nb = bf_grad_blocks(a.n_rows, a.m);
        if (!(bf_gneiting_launch_a(a, g, s) || bf_gneiting_launch_b(a, g, s) || bf_gneiting_launch_c(a, g, s) ||
              bf_gneiting_launch_d(a, g, s) || bf_gneiting_launch_e(a, g, s) || bf_gneiting_launch_f(a, g, s) ||
              bf_gneiting_launch_g(a, g, s) || bf_gneiting_launch_h(a, g, s)))
            return hipErrorInvalidValue;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (!g) return bf_finalize_launch(a.rec, nb, partials, s);
    hipLaunchKernelGGL(bf_gneiting_finalize, dim3(1), dim3(1024), 0, s, a.rec, nb, partials, grad);
    return hipGetLastError();
}

}  // namespace nngp
