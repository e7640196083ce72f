// Host side of the multivariate (coregionalised) sweep (bf_mv.h): its constants, the size of its workspace and the
// argument checks of its C entry points.  Plain C++ with no HIP in it, so tests/host/mv_check.cpp builds it under
// AddressSanitizer and UBSan on its own.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/nngp.h"

namespace nngp {

constexpr int kMvMinQ = 2;
constexpr int kMvMaxQ = NNGP_MV_MAX_Q;
constexpr int kMvMaxRows = 64;  // n = (m + 1) q joint rows at most
constexpr int kMvMaxCols = NNGP_MV_MAX_COLS;
constexpr int kMvWaves = 4;  // locations per 256-thread block, one wavefront each

// 16-row tiles of the neighbours' m q rows (the q target rows and the value columns share one more tile row)
constexpr int mv_tiles(int m, int q) { return (m * q + 15) / 16; }
inline int64_t mv_blocks(int64_t n_rows) { return (n_rows + kMvWaves - 1) / kMvWaves; }

inline bool mv_scope(int64_t n_rows, int m, int q) {
    return n_rows >= 0 && q >= kMvMinQ && q <= kMvMaxQ && m >= 1 && (m + 1) * q <= kMvMaxRows;
}

// one 4-double record per block and at least one, 256-byte granules; 0 outside the scope
inline size_t mv_workspace_bytes(int64_t n_rows, int m, int q) {
    if (!mv_scope(n_rows, m, q) || n_rows > ((int64_t)1 << 47)) return 0;
    const int64_t nb = n_rows > 0 ? mv_blocks(n_rows) : 1;
    return ((size_t)nb * 4 * sizeof(double) + 255) & ~(size_t)255;
}

// the gradient sweep (bf_mv_grad.h): P = q (q + 1) / 2 + 2 q parameters (A's lower triangle row-major, phi, tau2); a
// record of 4 + P doubles per location, folded in chunks of kMvGradChunk locations (a record per chunk), each part
// in 256-byte granules and at least one record; 0 outside the scope
constexpr int mv_grad_len(int q) { return q * (q + 1) / 2 + 2 * q; }
constexpr int kMvGradChunk = 1024;
inline int64_t mv_grad_chunks(int64_t n_rows) { return (n_rows + kMvGradChunk - 1) / kMvGradChunk; }
inline size_t mv_grad_rows_bytes(int64_t n_rows, int q) {
    return ((size_t)(n_rows > 0 ? n_rows : 1) * (4 + mv_grad_len(q)) * sizeof(double) + 255) & ~(size_t)255;
}
inline size_t mv_grad_workspace_bytes(int64_t n_rows, int m, int q) {
    if (!mv_scope(n_rows, m, q) || n_rows > ((int64_t)1 << 47)) return 0;
    return mv_grad_rows_bytes(n_rows, q) + mv_grad_rows_bytes(mv_grad_chunks(n_rows), q);
}

struct MvError {
    int code = NNGP_OK;
    char msg[320] = "";
};

inline int mv_fail(MvError& e, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(e.msg, sizeof e.msg, fmt, ap);
    va_end(ap);
    e.code = code;
    return code;
}

// the checks the two entry points share (scope, the LMC parameters, pointers, rows, workspace).  A (q, q) row-major,
// phi (q,) and tau2 (q,) are host arrays and the only memory read.
inline int mv_sweep_check(MvError& e, const void* coords, int64_t n_points, int dim, const void* nbr, int64_t n_rows,
                          int m, int q, int64_t i0, int64_t n_locs, int kind, const double* A, const double* phi,
                          const double* tau2, int c, const void* partials, const void* workspace,
                          size_t workspace_bytes) {
    if (q < kMvMinQ || q > kMvMaxQ)
        return mv_fail(e, NNGP_EUNSUP, "the multivariate sweeps serve %d <= q <= %d outcomes (q=%d)", kMvMinQ, kMvMaxQ, q);
    if (m < 1 || (m + 1) * q > kMvMaxRows)
        return mv_fail(e, NNGP_EUNSUP, "the multivariate sweeps serve m >= 1 and (m + 1) q <= %d joint rows (m=%d, q=%d)",
                       kMvMaxRows, m, q);
    if (kind == NNGP_COV_SPHERICAL || kind == NNGP_COV_MATERN)
        return mv_fail(e, NNGP_EUNSUP, "the multivariate sweeps serve the exponential, Matern-3/2, Matern-5/2 and "
                                       "Gaussian kinds (kind=%d)", kind);
    if (kind < NNGP_COV_EXPONENTIAL || kind > NNGP_COV_MATERN) return mv_fail(e, NNGP_EINVAL, "unknown kind %d", kind);
    if (dim < 1 || dim > NNGP_MAX_DIM) return mv_fail(e, NNGP_EINVAL, "dim=%d outside [1, %d]", dim, NNGP_MAX_DIM);
    if (A == nullptr || phi == nullptr || tau2 == nullptr)
        return mv_fail(e, NNGP_EINVAL, "A, phi and tau2 must be non-null (host arrays)");
    for (int a = 0; a < q; ++a) {
        if (!(A[a * q + a] > 0.0) || !isfinite(A[a * q + a]))
            return mv_fail(e, NNGP_EINVAL, "A must have a positive finite diagonal: A[%d][%d]", a, a);
        for (int b = 0; b < q; ++b) {
            if (b > a && A[a * q + b] != 0.0)
                return mv_fail(e, NNGP_EINVAL, "A must be lower-triangular: A[%d][%d] is not 0", a, b);
            if (!isfinite(A[a * q + b])) return mv_fail(e, NNGP_EINVAL, "A must be finite: A[%d][%d]", a, b);
        }
        if (!(phi[a] > 0.0) || !isfinite(phi[a])) return mv_fail(e, NNGP_EINVAL, "phi must be positive and finite: phi[%d]", a);
        if (!(tau2[a] >= 0.0) || !isfinite(tau2[a]))
            return mv_fail(e, NNGP_EINVAL, "tau2 must be non-negative and finite: tau2[%d]", a);
    }
    if (c < 1 || c > kMvMaxCols) return mv_fail(e, NNGP_EINVAL, "c=%d value columns outside [1, %d]", c, kMvMaxCols);
    if (coords == nullptr || workspace == nullptr)
        return mv_fail(e, NNGP_EINVAL, "coordinates and workspace must be non-null");
    if (partials == nullptr) return mv_fail(e, NNGP_EINVAL, "partials must be non-null");
    if (n_rows > 0 && nbr == nullptr) return mv_fail(e, NNGP_EINVAL, "nbr must be non-null");
    if (n_points < 1 || n_points > INT32_MAX)
        return mv_fail(e, NNGP_EINVAL, "n_points=%lld outside [1, 2^31)", (long long)n_points);
    if (n_rows < 0 || i0 < 0 || n_locs < 0 || n_rows > n_locs || i0 > n_locs - n_rows)
        return mv_fail(e, NNGP_EINVAL, "rows [%lld, %lld + %lld) outside [0, %lld)", (long long)i0, (long long)i0,
                       (long long)n_rows, (long long)n_locs);
    if (((uintptr_t)workspace & 255) != 0) return mv_fail(e, NNGP_EINVAL, "workspace must be 256-byte aligned");
    const size_t need = mv_workspace_bytes(n_rows, m, q);
    if (need == 0) return mv_fail(e, NNGP_EINVAL, "n_rows=%lld is too large", (long long)n_rows);
    if (workspace_bytes < need)
        return mv_fail(e, NNGP_EINVAL, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    return NNGP_OK;
}

// nngp_bf_grad_mv: the sweep's checks (S = T, one value column), the pointers of its own and its larger workspace
inline int mv_grad_check(MvError& e, const void* coords, int64_t n_points, int dim, const void* nbr, int64_t n_rows,
                         int m, int q, int64_t i0, int kind, const double* A, const double* phi, const double* tau2,
                         const void* values, const void* partials, const void* grad, const void* workspace,
                         size_t workspace_bytes) {
    if (mv_sweep_check(e, coords, n_points, dim, nbr, n_rows, m, q, i0, n_points, kind, A, phi, tau2, 1, partials,
                       workspace, workspace_bytes) != NNGP_OK)
        return e.code;
    if (values == nullptr || grad == nullptr) return mv_fail(e, NNGP_EINVAL, "values and grad must be non-null");
    const size_t need = mv_grad_workspace_bytes(n_rows, m, q);
    if (workspace_bytes < need)
        return mv_fail(e, NNGP_EINVAL, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    return NNGP_OK;
}

}  // namespace nngp
