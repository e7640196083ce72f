// Polya-Gamma kernels of the binomial / logistic NNGP sampler (pynngp_amd/gibbs_binomial.py): the draws
// omega_i ~ PG(b_i, c_i) (polya_gamma.h: Devroye's exact sampler, the source a CPU program checks), the
// fused per-iteration update and the statistics of the beta / sigma2 draws.
//
// Shape: one lane per location, 256-thread blocks, no LDS; trials are int32.  The sampler is a chain of
// data-dependent rejection loops, so lanes diverge: a wave costs what its largest b (and its unluckiest lane)
// costs.  That is accepted -- the draws of a location must not depend on its neighbours in the wave, so the
// work is not rebalanced across lanes; Bernoulli data (b = 1 everywhere) has no imbalance beyond the
// rejection rounds (acceptance above 0.999).
// A location whose c is not finite, whose trials lie outside [0, NNGP_PG_MAX_TRIALS] or whose sampler hit
// a loop cap gets NaN and reports index + 1 into the status word (0 = clean; the smallest index wins).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "nngp_internal.h"
#include "polya_gamma.h"

namespace nngp {

// status = min over the flagged locations of index + 1, 0 meaning clean: the first flag replaces the 0, every
// later one is a minimum (vector atomics; the path is taken by faulty locations only)
__device__ __forceinline__ void pg_flag(int32_t* status, int64_t i) {
    const int32_t v = (int32_t)(i + 1);
    if (atomicCAS(status, 0, v) != 0) atomicMin(status, v);
}

// FUSED: c_i = xb_i + w_i, and yres_i = kappa_i / omega_i - xb_i (0 where trials_i = 0) is written too
template <bool FUSED>
__global__ __launch_bounds__(256) void polya_gamma_kernel(int64_t n, const int32_t* __restrict__ trials,
                                                          const double* __restrict__ c,
                                                          const double* __restrict__ kappa,
                                                          const double* __restrict__ xb,
                                                          const double* __restrict__ w, uint64_t seed,
                                                          uint64_t sweep, double* __restrict__ omega,
                                                          double* __restrict__ yres, int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t b = trials[i];
    double xi = 0.0, ci;
    if constexpr (FUSED) {
        xi = xb[i];
        ci = xi + w[i];
    } else {
        ci = c[i];
    }
    PgStream s = pg_stream(seed, (uint64_t)i, sweep);
    bool bad = false;
    const double om = pg_draw(b, ci, s, &bad);
    omega[i] = om;
    if constexpr (FUSED) yres[i] = b == 0 ? 0.0 : kappa[i] / om - xi;
    if (bad) pg_flag(status, i);
}

hipError_t polya_gamma_launch(int64_t n, const int32_t* trials, const double* c, const double* kappa,
                              const double* xb, const double* w, uint64_t seed, uint64_t sweep, double* omega,
                              double* yres, int32_t* status, hipStream_t s) {
    hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    if (n == 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (c != nullptr)
        hipLaunchKernelGGL(polya_gamma_kernel<false>, grid, dim3(256), 0, s, n, trials, c, nullptr, nullptr, nullptr,
                           seed, sweep, omega, nullptr, status);
    else
        hipLaunchKernelGGL(polya_gamma_kernel<true>, grid, dim3(256), 0, s, n, trials, nullptr, kappa, xb, w, seed,
                           sweep, omega, yres, status);
    return hipGetLastError();
}

// ---------------------------------------------------------------- statistics of the conjugate steps
// nv = 1 + p (p + 1) / 2 + p values: sum r_i^2 / Ft_i; the upper triangle of X' Omega X row by row;
// X' (kappa - Omega w).  Per-block records and one fold in a fixed order, as gibbs_stats_blocks /
// gibbs_stats_fold (gibbs.hip): bit-reproducible, independent of the grid.
__global__ __launch_bounds__(256) void gibbs_pg_stats_blocks(int64_t n, const double* __restrict__ r,
                                                             const double* __restrict__ Ft,
                                                             const double* __restrict__ omega,
                                                             const double* __restrict__ kappa,
                                                             const double* __restrict__ X, int p,
                                                             const double* __restrict__ w,
                                                             double* __restrict__ rec) {
    __shared__ double sh[256];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int nt = p * (p + 1) / 2, nv = 1 + nt + p;
    const bool live = i < n;
    const double om = live ? omega[i] : 0.0;
    int a = 0, c = 0;  // the (row, column) of the triangle's current entry
    for (int v = 0; v < nv; ++v) {
        double x = 0.0;
        if (live) {
            if (v == 0) {
                x = r[i] * r[i] / Ft[i];
            } else if (v <= nt) {
                x = X[i * p + a] * om * X[i * p + c];
            } else {
                x = X[i * p + (v - 1 - nt)] * (kappa[i] - om * w[i]);
            }
        }
        if (v >= 1 && v <= nt && ++c == p) c = ++a;
        sh[threadIdx.x] = x;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) rec[blockIdx.x * (int64_t)nv + v] = sh[0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void gibbs_pg_stats_fold(const double* __restrict__ rec, int64_t nb, int nv,
                                                            double* __restrict__ out) {
    // fixed order: thread t folds records t, t + 1024, ...; xor-butterfly per wave; 16 waves in order
    __shared__ double sh[16];
    const int t = threadIdx.x;
    for (int v = 0; v < nv; ++v) {
        double a = 0.0;
        for (int64_t b = t; b < nb; b += 1024) a += rec[b * nv + v];
        a = wave_sum(a);
        if ((t & 63) == 0) sh[t >> 6] = a;
        __syncthreads();
        if (t == 0) {
            double x = 0.0;
            for (int k = 0; k < 16; ++k) x += sh[k];
            out[v] = x;
        }
        __syncthreads();
    }
}

size_t gibbs_pg_stats_workspace_bytes(int64_t n, int p) {
    const size_t nv = 1 + (size_t)p * (p + 1) / 2 + p;
    return (((size_t)((n + 255) / 256) * nv * 8) + 255) & ~(size_t)255;
}

hipError_t gibbs_pg_stats_launch(int64_t n, const double* r, const double* Ft, const double* omega,
                                 const double* kappa, const double* X, int p, const double* w, double* out,
                                 void* workspace, hipStream_t s) {
    const int64_t nb = (n + 255) / 256;
    if (nb == 0) return hipErrorInvalidValue;
    const int nv = 1 + p * (p + 1) / 2 + p;
    hipLaunchKernelGGL(gibbs_pg_stats_blocks, dim3((unsigned)nb), dim3(256), 0, s, n, r, Ft, omega, kappa, X, p, w,
                       (double*)workspace);
    hipLaunchKernelGGL(gibbs_pg_stats_fold, dim3(1), dim3(1024), 0, s, (const double*)workspace, nb, nv, out);
    return hipGetLastError();
}

}  // namespace nngp
