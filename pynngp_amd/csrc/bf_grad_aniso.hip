// Per-axis gradient sweep (bf_grad_aniso.h): dispatch over the instantiation units and the fixed-order fold of
// the per-block records into partials[4] and grad[dim + 2].
#include "bf_grad_aniso.h"

namespace nngp {

// bf_grad_finalize's order (thread t folds records t, t + 1024, ...; a fixed xor-butterfly inside each wave, a
// fixed fold over the 16 waves) with five gradient sums: two runs give identical bits.  grad takes
// (sigma2, phi_1..phi_dim, tau2).
__global__ __launch_bounds__(1024) void bf_grad_aniso_finalize(const double* __restrict__ rec, int64_t n_blocks,
                                                               double* __restrict__ partials,
                                                               double* __restrict__ grad, int dim) {
    __shared__ double sh[16][kGradAnisoRec];
    const int t = threadIdx.x;
    double a = 0.0, b = 0.0, c = INFINITY, d = INFINITY, g[kGradAnisoSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t k = t; k < n_blocks; k += 1024) {
        const double4 lo = *(const double4*)(rec + kGradAnisoRec * k);
        const double4 mi = *(const double4*)(rec + kGradAnisoRec * k + 4);
        const double4 hi = *(const double4*)(rec + kGradAnisoRec * k + 8);
        a += lo.x;
        b += lo.y;
        c = fmin(c, lo.z);
        d = fmin(d, lo.w);
        g[0] += mi.x;
        g[1] += mi.y;
        g[2] += mi.z;
        g[3] += mi.w;
        g[4] += hi.x;
    }
    a = wave_sum(a);
    b = wave_sum(b);
    c = wave_min(c);
    d = wave_min(d);
#pragma unroll
    for (int k = 0; k < kGradAnisoSums; ++k) g[k] = wave_sum(g[k]);
    if ((t & 63) == 0) {
        double* o = sh[t >> 6];
        o[0] = a;
        o[1] = b;
        o[2] = c;
        o[3] = d;
#pragma unroll
        for (int k = 0; k < kGradAnisoSums; ++k) o[4 + k] = g[k];
    }
    __syncthreads();
    if (t == 0) {
        a = 0.0, b = 0.0, c = INFINITY, d = INFINITY;
        for (int k = 0; k < kGradAnisoSums; ++k) g[k] = 0.0;
        for (int w = 0; w < 16; ++w) {
            a += sh[w][0];
            b += sh[w][1];
            c = fmin(c, sh[w][2]);
            d = fmin(d, sh[w][3]);
            for (int k = 0; k < kGradAnisoSums; ++k) g[k] += sh[w][4 + k];
        }
        partials[0] = a;
        partials[1] = b;
        partials[2] = c == INFINITY ? -1.0 : c;
        partials[3] = d == INFINITY ? -1.0 : d;
        grad[0] = g[0];
        grad[1] = g[1];
        if (dim > 1) grad[2] = g[2];
        if (dim > 2) grad[3] = g[3];
        grad[1 + dim] = g[4];
    }
}

hipError_t bf_grad_aniso_launch(const GradAnisoArgs& a, double* partials, double* grad, hipStream_t s) {
    int64_t nb = 0;
    if (a.n_rows > 0) {
        nb = bf_grad_blocks(a.n_rows, a.m);
        if (!(bf_grad_aniso_launch_a(a, s) || bf_grad_aniso_launch_b(a, s) || bf_grad_aniso_launch_c(a, s) ||
              bf_grad_aniso_launch_d(a, s) || bf_grad_aniso_launch_e(a, s) || bf_grad_aniso_launch_f(a, s) ||
              bf_grad_aniso_launch_g(a, s) || bf_grad_aniso_launch_h(a, s)))
            return hipErrorInvalidValue;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(bf_grad_aniso_finalize, dim3(1), dim3(1024), 0, s, a.rec, nb, partials, grad, a.dim);
    return hipGetLastError();
}

}  // namespace nngp
