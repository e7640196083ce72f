// Nonstationary sweeps (bf_ns.h): the packing kernel of the per-point records, the dispatch over the instantiation
// units and bf_finalize's fixed-order fold of the per-block records.
#include "bf_ns.h"

namespace nngp {

__global__ __launch_bounds__(256) void ns_pack(const double* __restrict__ sigma2, const double* __restrict__ phi,
                                               const double* __restrict__ tau2, int64_t n, double4* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double s = sigma2[i], p = phi[i], t = tau2[i];
    // (the comparisons are false for NaN)
    const bool ok = s > 0.0 && s < INFINITY && p > 0.0 && p < INFINITY && t >= 0.0 && t < INFINITY;
    out[i] = ok ? make_double4(sqrt(s), p, t, 0.0) : make_double4(1.0, 1.0, 1.0, 1.0);
}

hipError_t bf_ns_pack_launch(const double* sigma2, const double* phi, const double* tau2, int64_t n, double4* out,
                             hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ns_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, sigma2, phi, tau2, n, out);
    return hipGetLastError();
}

// Block b adds rows 256 b .. 256 b + 255 of lfq in a fixed order into the two sums of record b, which the sweep
// wrote as 0 (the sweep has at least as many blocks: P >= 1 lanes per row).  The flags of the record stay.
__global__ __launch_bounds__(256) void ns_fold(const double2* __restrict__ lfq, int64_t n_rows,
                                               double* __restrict__ rec) {
    __shared__ double sh[4][2];
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const double2 v = r < n_rows ? lfq[r] : make_double2(0.0, 0.0);
    const double a = wave_sum(v.x), b = wave_sum(v.y);
    if ((threadIdx.x & 63) == 0) {
        sh[threadIdx.x >> 6][0] = a;
        sh[threadIdx.x >> 6][1] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        rec[4 * (int64_t)blockIdx.x] = ((sh[0][0] + sh[1][0]) + sh[2][0]) + sh[3][0];
        rec[4 * (int64_t)blockIdx.x + 1] = ((sh[0][1] + sh[1][1]) + sh[2][1]) + sh[3][1];
    }
}

hipError_t bf_ns_launch(const NsArgs& a, double* partials, hipStream_t s) {
    int64_t nb = 0;
    if (a.n_rows > 0) {
        nb = bf_grad_blocks(a.n_rows, a.m);
        if (!(bf_ns_launch_a(a, s) || bf_ns_launch_b(a, s) || bf_ns_launch_c(a, s) || bf_ns_launch_d(a, s) ||
              bf_ns_launch_e(a, s) || bf_ns_launch_f(a, s) || bf_ns_launch_g(a, s) || bf_ns_launch_h(a, s)))
            return hipErrorInvalidValue;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(ns_fold, dim3((unsigned)((a.n_rows + 255) / 256)), dim3(256), 0, s, a.lfq, a.n_rows, a.rec);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return bf_finalize_launch(a.rec, nb, partials, s);
}

}  // namespace nngp
