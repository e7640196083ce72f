// Sweeps for points in 4 .. 16 dimensions (bf_nd.h): dispatch over the instantiation units and the fixed-order
// folds of the per-block records -- bf_finalize's for the forward sweep, and for the gradient a fold of
// nd_rec(dim) = 4 + dim + 2 doubles per block in bf_grad_finalize's order.
#include "bf_nd.h"

namespace nngp {

// One component of the record at a time: thread t folds records t, t + 1024, ...; then a fixed xor-butterfly inside
// each wave and a fixed fold over the 16 waves: two runs give identical bits.  grad takes (sigma2, phi_1..phi_dim,
// tau2).
__global__ __launch_bounds__(1024) void bf_nd_finalize(const double* __restrict__ rec, int64_t n_blocks, int nrec,
                                                       double* __restrict__ partials, double* __restrict__ grad) {
    __shared__ double sh[16];
    const int t = threadIdx.x;
    for (int c = 0; c < nrec; ++c) {
        const bool mn = c == 2 || c == 3;
        double a = mn ? INFINITY : 0.0;
        for (int64_t k = t; k < n_blocks; k += 1024) {
            const double v = rec[(int64_t)nrec * k + c];
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

hipError_t bf_nd_launch(const NdArgs& a, double* partials, double* grad, hipStream_t s) {
    const bool g = grad != nullptr;
    int64_t nb = 0;
    if (a.n_rows > 0) {
        nb = bf_grad_blocks(a.n_rows, a.m);
        if (!(bf_nd_launch_a(a, g, s) || bf_nd_launch_b(a, g, s) || bf_nd_launch_c(a, g, s) ||
              bf_nd_launch_d(a, g, s) || bf_nd_launch_e(a, g, s) || bf_nd_launch_f(a, g, s) ||
              bf_nd_launch_g(a, g, s) || bf_nd_launch_h(a, g, s)))
            return hipErrorInvalidValue;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (!g) return bf_finalize_launch(a.rec, nb, partials, s);
    hipLaunchKernelGGL(bf_nd_finalize, dim3(1), dim3(1024), 0, s, a.rec, nb, nd_rec(a.dim), partials, grad);
    return hipGetLastError();
}

}  // namespace nngp
