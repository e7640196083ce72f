// Host side of the multivariate sweep with outcomes missing at some sites (bf_mv_obs.h): its constants, scope, the size
// of its workspace and the argument checks of its C entry points.  Plain C++ with no HIP in it, so
// tests/host/mv_obs_check.cpp builds it under AddressSanitizer and UBSan on its own.
#pragma once
#include "mv_host.h"

namespace nngp {

constexpr int kMvObsMaxM = 63;      // one lane per neighbour slot and one for the target
constexpr int kMvObsMaxRows = 64;   // packed (observed) neighbour rows per location at most

// 16-row tiles that LDS and the register arrays are sized for, from the caller's bound on the packed rows
constexpr int mv_obs_tiles(int rows_max) { return (rows_max + 15) / 16; }

inline bool mv_obs_scope(int64_t n_rows, int m, int q) {
    return n_rows >= 0 && q >= kMvMinQ && q <= kMvMaxQ && m >= 1 && m <= kMvObsMaxM;
}

// one 4-double record per location (not per block: a block's four rows are other locations under another `order`,
// and the partials must not depend on it) and at least one, 256-byte granules; 0 outside the scope
inline size_t mv_obs_workspace_bytes(int64_t n_rows, int m, int q) {
    if (!mv_obs_scope(n_rows, m, q) || n_rows > ((int64_t)1 << 47)) return 0;
    return ((size_t)(n_rows > 0 ? n_rows : 1) * 4 * sizeof(double) + 255) & ~(size_t)255;
}

// the checks of nngp_bf_sweep_mv_obs / nngp_bf_cross_mv_obs: this sweep's own scope, then mv_sweep_check for what
// the two sweeps share (it is called with m = 1, which passes its scope test; its workspace is never larger)
inline int mv_obs_check(MvError& e, const void* coords, int64_t n_points, int dim, const void* nbr, int64_t n_rows,
                        int m, int q, int64_t i0, int64_t n_locs, int kind, const double* A, const double* phi,
                        const double* tau2, int c, const void* obs, int rows_max, const void* partials,
                        const void* workspace, size_t workspace_bytes) {
    if (q < kMvMinQ || q > kMvMaxQ)
        return mv_fail(e, NNGP_EUNSUP, "the multivariate sweeps serve %d <= q <= %d outcomes (q=%d)", kMvMinQ, kMvMaxQ, q);
    if (m < 1 || m > kMvObsMaxM)
        return mv_fail(e, NNGP_EUNSUP, "the packed-row multivariate sweep serves 1 <= m <= %d (m=%d)", kMvObsMaxM, m);
    if (rows_max < 1 || rows_max > kMvObsMaxRows)
        return mv_fail(e, NNGP_EUNSUP, "the packed-row multivariate sweep serves 1 <= rows_max <= %d observed "
                                       "neighbour rows per location (rows_max=%d)", kMvObsMaxRows, rows_max);
    if (mv_sweep_check(e, coords, n_points, dim, nbr, n_rows, 1, q, i0, n_locs, kind, A, phi, tau2, c, partials,
                       workspace, workspace_bytes) != NNGP_OK)
        return e.code;
    if (obs == nullptr) return mv_fail(e, NNGP_EINVAL, "obs must be non-null");
    const size_t need = mv_obs_workspace_bytes(n_rows, m, q);
    if (workspace_bytes < need)
        return mv_fail(e, NNGP_EINVAL, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    return NNGP_OK;
}

// the gradient sweep on packed rows (bf_mv_obs_grad.h): bf_mv_grad's records (4 + P doubles per location, then per
// chunk of kMvGradChunk locations) in this sweep's scope; 0 outside it
inline size_t mv_obs_grad_workspace_bytes(int64_t n_rows, int m, int q) {
    if (!mv_obs_scope(n_rows, m, q) || n_rows > ((int64_t)1 << 47)) return 0;
    return mv_grad_rows_bytes(n_rows, q) + mv_grad_rows_bytes(mv_grad_chunks(n_rows), q);
}

// nngp_bf_grad_mv_obs: the packed sweep's checks (S = T, one value column), the pointers of its own and its larger
// workspace
inline int mv_obs_grad_check(MvError& e, const void* coords, int64_t n_points, int dim, const void* nbr, int64_t n_rows,
                             int m, int q, int64_t i0, int kind, const double* A, const double* phi, const double* tau2,
                             const void* obs, int rows_max, const void* values, const void* partials, const void* grad,
                             const void* workspace, size_t workspace_bytes) {
    if (mv_obs_check(e, coords, n_points, dim, nbr, n_rows, m, q, i0, n_points, kind, A, phi, tau2, 1, obs, rows_max,
                     partials, workspace, workspace_bytes) != NNGP_OK)
        return e.code;
    if (values == nullptr || grad == nullptr) return mv_fail(e, NNGP_EINVAL, "values and grad must be non-null");
    const size_t need = mv_obs_grad_workspace_bytes(n_rows, m, q);
    if (workspace_bytes < need)
        return mv_fail(e, NNGP_EINVAL, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    return NNGP_OK;
}

}  // namespace nngp
