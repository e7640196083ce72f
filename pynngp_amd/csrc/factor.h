// Triangular solves with the NNGP factor (factor_solve.hip): (I - B) x = b and (I - B)^T x = b by level
// scheduling, and what is composed from them: the covariance product and prior draws.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace nngp {

// rows a single workgroup of the narrow-run kernel takes per level (NNGP_FACTOR_MAX_FUSE_WIDTH)
constexpr int kFactorMaxFuse = 1024;

struct FactorSchedule {
    const int32_t* rows;            // device (n,): the rows sorted by (level, index)
    const int32_t* level_off;       // device (n_levels + 1,): the narrow-run kernel walks it
    const int32_t* level_off_host;  // the same offsets on the host: they steer the launches
    int64_t n_levels;
};

struct FactorGeom {
    const int32_t* nbr;    // (n, m), -1 padded
    const double* B;       // (n, m)
    const int32_t* off;    // (n + 1,) reverse lists (trans only)
    const int32_t* rev_j;  // child row per reverse entry (trans only)
    const double* Brev;    // B per reverse entry, from the Gibbs prep buffer (trans only)
    int64_t n;
    int m;
};

// the launches a solve makes for this schedule and fuse_width (no GPU work)
void factor_launch_counts(const FactorSchedule& sc, int fuse_width, int64_t* n_wide, int64_t* n_runs);
// x = (I - B)^-1 b (trans = 0) or (I - B)^-T b (trans = 1); b and x (n, nrhs) row-major, may alias
hipError_t factor_solve_launch(const FactorGeom& g, const FactorSchedule& sc, int nrhs, int trans, int fuse_width,
                               const double* b, double* x, hipStream_t s);
// out[i, c] = v[i, c] * (sigma2 F_i) (root = false) or * sqrt(sigma2 F_i) (root = true); v null: the Philox normal
// of (seed, location i, sweep draw0 + c) in v's place.  v and out may alias.
hipError_t factor_scale_launch(const double* F, double sigma2, bool root, int64_t n, int nrhs, const double* v,
                               uint64_t seed, uint64_t draw0, double* out, hipStream_t s);

}  // namespace nngp
