// Separable space-time sweeps (bf_sep.h): dispatch over the instantiation units and the fixed-order folds of the
// per-block records -- bf_finalize's for the forward sweep, bf_grad_finalize's order with four gradient sums for
// the gradient (bf_grad_fold_launch writes three).
#include "bf_sep.h"

namespace nngp {

// Thread t folds records t, t + 1024, ...; then a fixed xor-butterfly inside each wave and a fixed fold over
// the 16 waves: two runs give identical bits.  grad takes (sigma2, phi_s, phi_t, tau2).
__global__ __launch_bounds__(1024) void bf_sep_finalize(const double* __restrict__ rec, int64_t n_blocks,
                                                        double* __restrict__ partials, double* __restrict__ grad) {
    __shared__ double sh[16][kSepRec];
    const int t = threadIdx.x;
    double a = 0.0, b = 0.0, c = INFINITY, d = INFINITY, g[kSepSums] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t k = t; k < n_blocks; k += 1024) {
        const double4 lo = *(const double4*)(rec + kSepRec * k);
        const double4 hi = *(const double4*)(rec + kSepRec * k + 4);
        a += lo.x;
        b += lo.y;
        c = fmin(c, lo.z);
        d = fmin(d, lo.w);
        g[0] += hi.x;
        g[1] += hi.y;
        g[2] += hi.z;
        g[3] += hi.w;
    }
    a = wave_sum(a);
    b = wave_sum(b);
    c = wave_min(c);
    d = wave_min(d);
#pragma unroll
    for (int k = 0; k < kSepSums; ++k) g[k] = wave_sum(g[k]);
    if ((t & 63) == 0) {
        double* o = sh[t >> 6];
        o[0] = a;
        o[1] = b;
        o[2] = c;
        o[3] = d;
#pragma unroll
        for (int k = 0; k < kSepSums; ++k) o[4 + k] = g[k];
    }
    __syncthreads();
    if (t == 0) {
        a = 0.0, b = 0.0, c = INFINITY, d = INFINITY;
        for (int k = 0; k < kSepSums; ++k) g[k] = 0.0;
        for (int w = 0; w < 16; ++w) {
            a += sh[w][0];
            b += sh[w][1];
            c = fmin(c, sh[w][2]);
            d = fmin(d, sh[w][3]);
            for (int k = 0; k < kSepSums; ++k) g[k] += sh[w][4 + k];
        }
        partials[0] = a;
        partials[1] = b;
        partials[2] = c == INFINITY ? -1.0 : c;
        partials[3] = d == INFINITY ? -1.0 : d;
        for (int k = 0; k < kSepSums; ++k) grad[k] = g[k];
    }
}

hipError_t bf_sep_launch(const SepArgs& a, double* partials, double* grad, hipStream_t s) {
    const bool g = grad != nullptr;
    int64_t nb = 0;
    if (a.n_rows > 0) {
        nb = bf_grad_blocks(a.n_rows, a.m);
        if (!(bf_sep_launch_a(a, g, s) || bf_sep_launch_b(a, g, s) || bf_sep_launch_c(a, g, s) ||
              bf_sep_launch_d(a, g, s) || bf_sep_launch_e(a, g, s) || bf_sep_launch_f(a, g, s) ||
              bf_sep_launch_g(a, g, s) || bf_sep_launch_h(a, g, s)))
            return hipErrorInvalidValue;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (!g) return bf_finalize_launch(a.rec, nb, partials, s);
    hipLaunchKernelGGL(bf_sep_finalize, dim3(1), dim3(1024), 0, s, a.rec, nb, partials, grad);
    return hipGetLastError();
}

}  // namespace nngp
