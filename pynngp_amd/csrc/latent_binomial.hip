// Binomial / logistic latent posterior by Laplace approximation (pynngp_amd/latent_binomial.py): the per-node
// link step of its Newton iteration and the logistic-normal integral of its predictions.
//
// s_i ~ Binomial(b_i, logistic(eta_i)), eta_i = offset_i + w_i.  One Newton / IRLS step is a Gaussian latent solve
// whose noise precision is the working weight W_i = b_i p_i (1 - p_i) and whose right-hand side is the working
// response times that weight; the solver is the one of latent.hip, this unit only forms its two vectors.
//
// Shape: one lane per node, 256-thread blocks, no LDS beyond the block fold; the kernel is a stream over four
// input and three output vectors (28 B read, 24 B written per node) with one exp and one log1p per node.
// Every quantity comes from e = exp(-|eta|) in (0, 1]:
//   p = 1 / (1 + e) (eta >= 0) or e / (1 + e),   q = 1 - p the other of the two,   W = b e / (1 + e)^2,
//   g = s - b p = s q - (b - s) p,   l = s eta - b log(1 + exp(eta)) = -(eta >= 0 ? b - s : s) |eta| - b log1p(e):
// sums of terms of one sign, so nothing cancels and nothing overflows for any finite eta (e and W underflow to
// exactly 0 beyond |eta| ~ 745).  The expressions are evaluated as written (no fused multiply-add contraction),
// so a host restatement in fp64 differs by the roundings of exp and log1p alone.
// Faults are data: a node whose eta is not finite, or whose trials are negative, gets NaN in d, rhs and g, adds
// nothing to the two statistics and reports index + 1 (the smallest wins) in partials[2] / partials[3].
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "latent_binomial.h"
#include "nngp_internal.h"

namespace nngp {

#pragma clang fp contract(off)

// logistic(t) from e = exp(-|t|); the link kernel's p and nngp_logistic_normal's integrand (and its s = 0 value)
__device__ __forceinline__ double logistic_stable(double t) {
#pragma clang fp contract(off)
    const double e = exp(-fabs(t));
    const double den = 1.0 + e;
    return t >= 0.0 ? 1.0 / den : e / den;
}

constexpr int kBinRec = 4;  // per-block record: sum l, max |g|, first non-finite node, first negative-trials node

__global__ __launch_bounds__(256) void binomial_newton_step_kernel(int64_t n, const int32_t* __restrict__ trials,
                                                                   const double* __restrict__ successes,
                                                                   const double* __restrict__ offset,
                                                                   const double* __restrict__ w,
                                                                   double* __restrict__ d, double* __restrict__ rhs,
                                                                   double* __restrict__ g, double* __restrict__ rec) {
#pragma clang fp contract(off)
    __shared__ double sh[4][kBinRec];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double ll = 0.0, gm = 0.0, bad = INFINITY, neg = INFINITY;
    if (i < n) {
        const int32_t bi = trials[i];
        double di = 0.0, ri = 0.0, gi = 0.0;
        if (bi != 0) {
            const double wi = w[i];
            const double eta = offset[i] + wi;
            if (bi < 0 || !isfinite(eta)) {
                di = ri = gi = NAN;
                if (bi < 0) neg = (double)i;
                else bad = (double)i;
            } else {
                const double b = (double)bi, s = successes[i];
                const double a = fabs(eta);
                const double e = exp(-a);
                const double den = 1.0 + e;
                const double big = 1.0 / den, small = e / den;  // logistic(|eta|), logistic(-|eta|)
                const bool pos = eta >= 0.0;
                const double p = pos ? big : small, q = pos ? small : big;
                di = b * (e / (den * den));
                gi = s * q - (b - s) * p;
                ri = di * wi + gi;
                ll = -((pos ? b - s : s) * a) - b * log1p(e);
                gm = fabs(gi);
            }
        }
        d[i] = di;
        rhs[i] = ri;
        g[i] = gi;
    }
    // the block's record in a fixed order: xor-butterfly per wave, then the four waves in index order
    ll = wave_sum(ll);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gm = fmax(gm, __shfl_xor(gm, o));
    if (__any(bad != INFINITY || neg != INFINITY)) {  // wave-uniform; rare
        bad = wave_min(bad);
        neg = wave_min(neg);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh[wv][0] = ll;
        sh[wv][1] = gm;
        sh[wv][2] = bad;
        sh[wv][3] = neg;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0, c = INFINITY, e = INFINITY;
        for (int k = 0; k < 4; ++k) {
            a += sh[k][0];
            b = fmax(b, sh[k][1]);
            c = fmin(c, sh[k][2]);
            e = fmin(e, sh[k][3]);
        }
        double* o = rec + kBinRec * (int64_t)blockIdx.x;
        o[0] = a;
        o[1] = b;
        o[2] = c;
        o[3] = e;
    }
}

// Thread t folds records t, t + 1024, ... in index order; then the xor-butterfly inside each wave and the 16 waves
// in order (bf_grad_finalize's order): two runs give identical bits.
__global__ __launch_bounds__(1024) void binomial_newton_step_fold(const double* __restrict__ rec, int64_t n_blocks,
                                                                  double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double sh[16][kBinRec];
    const int t = threadIdx.x;
    double a = 0.0, b = 0.0, c = INFINITY, e = INFINITY;
    for (int64_t k = t; k < n_blocks; k += 1024) {
        const double4 r = *(const double4*)(rec + kBinRec * k);
        a += r.x;
        b = fmax(b, r.y);
        c = fmin(c, r.z);
        e = fmin(e, r.w);
    }
    a = wave_sum(a);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b = fmax(b, __shfl_xor(b, o));
    c = wave_min(c);
    e = wave_min(e);
    if ((t & 63) == 0) {
        sh[t >> 6][0] = a;
        sh[t >> 6][1] = b;
        sh[t >> 6][2] = c;
        sh[t >> 6][3] = e;
    }
    __syncthreads();
    if (t == 0) {
        a = 0.0, b = 0.0, c = INFINITY, e = INFINITY;
        for (int k = 0; k < 16; ++k) {
            a += sh[k][0];
            b = fmax(b, sh[k][1]);
            c = fmin(c, sh[k][2]);
            e = fmin(e, sh[k][3]);
        }
        partials[0] = a;
        partials[1] = b;
        partials[2] = c == INFINITY ? 0.0 : c + 1.0;
        partials[3] = e == INFINITY ? 0.0 : e + 1.0;
    }
}

size_t binomial_newton_step_workspace_bytes(int64_t n) {
    return (((size_t)((n + 255) / 256) * kBinRec * sizeof(double)) + 255) & ~(size_t)255;
}

hipError_t binomial_newton_step_launch(int64_t n, const int32_t* trials, const double* successes,
                                       const double* offset, const double* w, double* d, double* rhs, double* g,
                                       double* partials, void* workspace, hipStream_t s) {
    const int64_t nb = (n + 255) / 256;
    if (nb > 0)
        hipLaunchKernelGGL(binomial_newton_step_kernel, dim3((unsigned)nb), dim3(256), 0, s, n, trials, successes,
                           offset, w, d, rhs, g, (double*)workspace);
    hipLaunchKernelGGL(binomial_newton_step_fold, dim3(1), dim3(1024), 0, s, (const double*)workspace, nb, partials);
    return hipGetLastError();
}

// ---------------------------------------------------------------- E[logistic(mu + s Z)], Z ~ N(0, 1)
// Trapezoid rule in z with step h = 1/16 on [-7, 7]: 225 nodes, the two of a pair +-z_k sharing their Gaussian
// weight (113 weights, computed once per block into LDS).  The integrand is analytic in the strip |Im z| < pi / s
// (the logistic's poles), so the rule's error falls like exp(-2 pi^2 / (s h)) = exp(-316 / s); the truncated tails
// hold 2.6e-12.  Against 30-digit quadrature: <= 1e-11 for s <= 13, 2.5e-9 at s = 17, 3.5e-8 at 20, 1.2e-5 at 34
// and 2e-3 at 100 (the limit s -> inf is the rule applied to a step: at most h phi(0) / 2 = 0.0125).  The loop count
// is fixed: no lane waits for another.  s = 0 returns logistic(mu) itself; a NaN or negative s, or a NaN mu, NaN.
constexpr int kLnPairs = 112;
constexpr double kLnStep = 0.0625;

__global__ __launch_bounds__(256) void logistic_normal_kernel(int64_t n, const double* __restrict__ mu,
                                                              const double* __restrict__ sd,
                                                              double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double wt[kLnPairs + 1];
    if (threadIdx.x <= kLnPairs) {
        const double z = kLnStep * (double)threadIdx.x;
        wt[threadIdx.x] = kLnStep * 0.3989422804014327 * exp(-0.5 * z * z);
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double m = mu[i], s = sd[i];
    double r;
    if (s == 0.0) {
        r = logistic_stable(m);
    } else if (!(s > 0.0) || m != m) {
        r = NAN;
    } else {
        r = wt[0] * logistic_stable(m);
        for (int k = 1; k <= kLnPairs; ++k) {
            const double sz = s * (kLnStep * (double)k);
            r += wt[k] * (logistic_stable(m + sz) + logistic_stable(m - sz));
        }
    }
    out[i] = r;
}

hipError_t logistic_normal_launch(int64_t n, const double* mu, const double* sd, double* out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(logistic_normal_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, mu, sd, out);
    return hipGetLastError();
}

}  // namespace nngp
