// Gradient sweep (bf_grad.h): dispatch over the instantiation units and the fixed-order fold of the
// per-block records into partials[4] and grad[3].
#include "bf_grad.h"

namespace nngp {

// Thread t folds records t, t + 1024, ...; then a fixed xor-butterfly inside each wave and a fixed fold over
// the 16 waves (bf_finalize's order, with the three gradient sums alongside): two runs give identical bits.
__global__ __launch_bounds__(1024) void bf_grad_finalize(const double* __restrict__ rec, int64_t n_blocks,
                                                         double* __restrict__ partials, double* __restrict__ grad) {
    __shared__ double sh[16][kGradRec];
    const int t = threadIdx.x;
    double a = 0.0, b = 0.0, c = INFINITY, d = INFINITY, g0 = 0.0, g1 = 0.0, g2 = 0.0;
    for (int64_t k = t; k < n_blocks; k += 1024) {
        const double4 lo = *(const double4*)(rec + kGradRec * k);
        const double4 hi = *(const double4*)(rec + kGradRec * k + 4);
        a += lo.x;
        b += lo.y;
        c = fmin(c, lo.z);
        d = fmin(d, lo.w);
        g0 += hi.x;
        g1 += hi.y;
        g2 += hi.z;
    }
    a = wave_sum(a);
    b = wave_sum(b);
    c = wave_min(c);
    d = wave_min(d);
    g0 = wave_sum(g0);
    g1 = wave_sum(g1);
    g2 = wave_sum(g2);
    if ((t & 63) == 0) {
        double* o = sh[t >> 6];
        o[0] = a;
        o[1] = b;
        o[2] = c;
        o[3] = d;
        o[4] = g0;
        o[5] = g1;
        o[6] = g2;
    }
    __syncthreads();
    if (t == 0) {
        a = 0.0, b = 0.0, c = INFINITY, d = INFINITY, g0 = 0.0, g1 = 0.0, g2 = 0.0;
        for (int w = 0; w < 16; ++w) {
            a += sh[w][0];
            b += sh[w][1];
            c = fmin(c, sh[w][2]);
            d = fmin(d, sh[w][3]);
            g0 += sh[w][4];
            g1 += sh[w][5];
            g2 += sh[w][6];
        }
        partials[0] = a;
        partials[1] = b;
        partials[2] = c == INFINITY ? -1.0 : c;
        partials[3] = d == INFINITY ? -1.0 : d;
        grad[0] = g0;
        grad[1] = g1;
        grad[2] = g2;
    }
}

hipError_t bf_grad_launch(const GradArgs& a, double* partials, double* grad, hipStream_t s) {
    int64_t nb = 0;
    if (a.n_rows > 0) {
        nb = bf_grad_blocks(a.n_rows, a.m);
        if (!(bf_grad_launch_a(a, s) || bf_grad_launch_b(a, s) || bf_grad_launch_c(a, s) || bf_grad_launch_d(a, s) ||
              bf_grad_launch_e(a, s) || bf_grad_launch_f(a, s) || bf_grad_launch_g(a, s) || bf_grad_launch_h(a, s)))
            return hipErrorInvalidValue;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return bf_grad_fold_launch(a.rec, nb, partials, grad, s);
}

hipError_t bf_grad_fold_launch(const double* rec, int64_t n_blocks, double* partials, double* grad, hipStream_t s) {
    hipLaunchKernelGGL(bf_grad_finalize, dim3(1), dim3(1024), 0, s, rec, n_blocks, partials, grad);
    return hipGetLastError();
}

}  // namespace nngp
