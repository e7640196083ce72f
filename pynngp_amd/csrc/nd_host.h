// Host side of the 4 .. 16-dimensional path (bf_nd.h, knn_nd.hip): its constants, the size of its workspace and the
// argument checks of its C entry points.  Plain C++ with no HIP in it, so tests/host/nd_check.cpp builds it under
// AddressSanitizer and UBSan on its own.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/nngp.h"

namespace nngp {

constexpr int kNdMinDim = 4;
constexpr int kNdMaxDim = NNGP_ND_MAX_DIM;
constexpr int kNdMaxM = 32;
constexpr int kNdThreads = 256;  // kGradThreads (bf_nd.h asserts it)

// lanes per location: grad_lanes (bf_grad.h; bf_nd.h asserts the two agree for every m)
constexpr int nd_lanes(int m) { return m <= 8 ? 2 : m <= 15 ? 4 : m <= 23 ? 8 : m <= 31 ? 16 : 64; }
inline int64_t nd_blocks(int64_t n_rows, int m) { return (n_rows * nd_lanes(m) + kNdThreads - 1) / kNdThreads; }

// per-block record of the gradient sweep: sum log F, sum r^2/F, first bad-pivot row, first bad-index row, then the
// dim + 2 gradient sums (sigma2, phi_1..phi_dim, tau2).  The forward sweep's four doubles fit inside it.
constexpr int nd_rec(int dim) { return 4 + dim + 2; }
constexpr int kNdRecMax = nd_rec(kNdMaxDim);

inline bool nd_scope(int64_t n_rows, int m, int dim) {
    return n_rows >= 0 && m >= 1 && m <= kNdMaxM && dim >= kNdMinDim && dim <= kNdMaxDim;
}

// one record per block and at least one, 256-byte granules; 0 outside the scope.  n_rows < 2^47 keeps the lane count
// inside int64.
inline size_t nd_workspace_bytes(int64_t n_rows, int m, int dim) {
    if (!nd_scope(n_rows, m, dim) || n_rows > ((int64_t)1 << 47)) return 0;
    const int64_t nb = n_rows > 0 ? nd_blocks(n_rows, m) : 1;
    const size_t bytes = (size_t)nb * (size_t)nd_rec(dim) * sizeof(double);
    return (bytes + 255) & ~(size_t)255;
}

struct NdError {
    int code = NNGP_OK;
    char msg[320] = "";
};

inline int nd_fail(NdError& e, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(e.msg, sizeof e.msg, fmt, ap);
    va_end(ap);
    e.code = code;
    return code;
}

// the checks the three sweep entry points share (scope, theta, pointers, rows, workspace); nothing is dereferenced
// but phi[0 .. dim)
inline int nd_sweep_check(NdError& e, const void* coords, int64_t n_points, int dim, const void* nbr, int64_t n_rows,
                          int m, int64_t i0, int64_t n_locs, int kind, double sigma2, const double* phi, double tau2,
                          const void* partials, const void* workspace, size_t workspace_bytes) {
    if (dim < kNdMinDim || dim > kNdMaxDim)
        return nd_fail(e, NNGP_EUNSUP, "the n-dimensional sweeps serve %d <= dim <= %d (dim=%d; dim <= %d has nngp_bf_sweep)",
                       kNdMinDim, kNdMaxDim, dim, NNGP_MAX_DIM);
    if (m < 1 || m > kNdMaxM) return nd_fail(e, NNGP_EUNSUP, "the n-dimensional sweeps serve 1 <= m <= %d (m=%d)", kNdMaxM, m);
    if (kind == NNGP_COV_SPHERICAL)
        return nd_fail(e, NNGP_EUNSUP, "the spherical correlation is not positive definite above three dimensions "
                                       "(dim=%d): the n-dimensional sweeps refuse it", dim);
    if (kind == NNGP_COV_MATERN)
        return nd_fail(e, NNGP_EUNSUP, "the n-dimensional sweeps serve the exponential, Matern-3/2, Matern-5/2 and "
                                       "Gaussian kinds, not the general-nu matern");
    if (kind < NNGP_COV_EXPONENTIAL || kind > NNGP_COV_MATERN) return nd_fail(e, NNGP_EINVAL, "unknown kind %d", kind);
    if (phi == nullptr) return nd_fail(e, NNGP_EINVAL, "phi must be non-null (dim decays)");
    if (!(sigma2 > 0.0) || !(tau2 >= 0.0) || !isfinite(sigma2) || !isfinite(tau2))
        return nd_fail(e, NNGP_EINVAL, "theta must satisfy sigma2 > 0, phi_k > 0, tau2 >= 0 (finite)");
    for (int k = 0; k < dim; ++k)
        if (!(phi[k] > 0.0) || !isfinite(phi[k]))
            return nd_fail(e, NNGP_EINVAL, "theta must satisfy sigma2 > 0, phi_k > 0, tau2 >= 0 (finite): phi[%d]", k);
    if (coords == nullptr || workspace == nullptr)
        return nd_fail(e, NNGP_EINVAL, "coordinates and workspace must be non-null");
    if (partials == nullptr) return nd_fail(e, NNGP_EINVAL, "partials must be non-null");
    if (n_rows > 0 && nbr == nullptr) return nd_fail(e, NNGP_EINVAL, "nbr must be non-null");
    if (n_points < 1 || n_points > INT32_MAX)
        return nd_fail(e, NNGP_EINVAL, "n_points=%lld outside [1, 2^31)", (long long)n_points);
    if (n_rows < 0 || i0 < 0 || n_locs < 0 || n_rows > n_locs || i0 > n_locs - n_rows)
        return nd_fail(e, NNGP_EINVAL, "rows [%lld, %lld + %lld) outside [0, %lld)", (long long)i0, (long long)i0,
                       (long long)n_rows, (long long)n_locs);
    if (((uintptr_t)workspace & 255) != 0) return nd_fail(e, NNGP_EINVAL, "workspace must be 256-byte aligned");
    const size_t need = nd_workspace_bytes(n_rows, m, dim);
    if (need == 0) return nd_fail(e, NNGP_EINVAL, "n_rows=%lld is too large", (long long)n_rows);
    if (workspace_bytes < need)
        return nd_fail(e, NNGP_EINVAL, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    return NNGP_OK;
}

// the neighbour searches need no scratch memory; the size is one granule so that 0 still means "unsupported"
inline size_t nd_knn_workspace_bytes(int64_t n_points, int dim, int m) {
    if (n_points < 1 || n_points > INT32_MAX || dim < kNdMinDim || dim > kNdMaxDim || m < 0 || m > kNdMaxM) return 0;
    return 256;
}

inline int nd_knn_check(NdError& e, const void* coords, int64_t n_points, int dim, int m, const void* workspace,
                        size_t workspace_bytes) {
    if (dim < kNdMinDim || dim > kNdMaxDim)
        return nd_fail(e, NNGP_EUNSUP, "the n-dimensional neighbour search serves %d <= dim <= %d (dim=%d; dim <= %d has "
                                       "nngp_knn_prior)", kNdMinDim, kNdMaxDim, dim, NNGP_MAX_DIM);
    if (m < 0 || m > kNdMaxM) return nd_fail(e, NNGP_EUNSUP, "m=%d outside [0, %d]", m, kNdMaxM);
    if (coords == nullptr || workspace == nullptr)
        return nd_fail(e, NNGP_EINVAL, "coords and workspace must be non-null");
    if (n_points < 1 || n_points > INT32_MAX)
        return nd_fail(e, NNGP_EINVAL, "n_points=%lld outside [1, 2^31)", (long long)n_points);
    if (((uintptr_t)workspace & 255) != 0) return nd_fail(e, NNGP_EINVAL, "workspace must be 256-byte aligned");
    const size_t need = nd_knn_workspace_bytes(n_points, dim, m);
    if (workspace_bytes < need)
        return nd_fail(e, NNGP_EINVAL, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    return NNGP_OK;
}

}  // namespace nngp
