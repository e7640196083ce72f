// The time-lag routine of the nonseparable (Gneiting) space-time covariance (bf_gneiting.h).
//
// With psi = 1 + x, x = (a u)^2 >= 0 (u the time lag), every pair needs
//     1 / psi,    L = ln psi,    s2 = psi^-beta        (0 <= beta <= 1),
// the last one scaling the squared spatial distance before the spatial correlation is evaluated.  No library pow
// or log:
//   * psi = ph + pl exactly (a branch-free two-sum of 1 and x), so nothing of a small x is lost in 1 + x;
//   * ph = 2^k m, m in [1, 2); j = the top 7 mantissa bits, c_j = 1 + j/128; d = m - c_j is exact and
//     r = d (1 / c_j) in [0, 2^-7) carries one rounding of a quantity below 2^-7.  Then
//         log2 psi = (k + hi_j) + (lo_j + log2(e) (log1p(r) + pl / ph)),
//     with {1 / c_j, hi_j, lo_j} from a 128-entry table (3 KB in LDS, gneiting_table.h): hi_j is a multiple of
//     2^-40, so k + hi_j is exact, and the bracket is below 2^-6;
//   * psi < 1 + 2^-7 (k = 0, j = 0, table entry {1, 0, 0}): the same lines are log1p(ph - 1) + pl / ph, and L is
//     taken from them directly instead of through log2 (L keeps its relative accuracy as the lag goes to 0, and
//     x = 0 gives L = 0, 1 / psi = 1 and s2 = 1 exactly).  No branch and no conditional table read: the compiler
//     turned an earlier select between a direct and a table form into three branches per pair;
//   * log1p(r) = r - r^2/2 + .. - r^8/8 on [0, 2^-7] (the next term is below 2^-59 r);
//   * s2 = 2^(-beta log2 psi) by nngp_exp_tab's scheme (the 2^(j/256) table and its degree-4 polynomial) on the
//     two-part argument: -256 beta (yh + yl) is split as k + f with k from yh alone, so the argument's error is
//     that of yl (below 2^-58), not half an ulp of a log2 psi up to 400;
//   * 1 / psi from v_rcp_f64 and a second-order step y (1 + e + e^2), e = 1 - ph y (v_rcp_f64 alone is taken
//     at 2^-24, as v_rsq_f64 measured; e^3 is below 2^-70).
// x is clamped at 2^400, so psi is finite and s2 >= 2^-400: a slot without a point sits at k 1e150 in space
// (far_point), h^2 s2 >= 1e300 2^-400 = 3.9e179 is past d2max for every c > 1e-87, and its covariance is exactly
// 0 whatever the time lag.
//
// Error bounds (tests/host/gneiting_check.cpp, against long double over x in {0, 2^-60 .. 2^40} with the table
// seams and their neighbours, beta in {0, 0.3, 0.5, 1}): each of 1 / psi, L and s2 within 2 ulp (measured 1.50,
// 1.74 and 1.01).
//
// The same source compiles on the host (NNGP_MATH_HOST), v_rcp_f64 emulated at 2^-24 with either sign.
#pragma once
#include "gneiting_table.h"
#include "nngp_math.h"

#define NNGP_GN_TAB_N 128
#define NNGP_GN_XMAX 0x1p400
#define NNGP_LN2 0x1.62e42fefa39efp-1

#ifdef NNGP_MATH_HOST
static const double kGnLogTab[3 * NNGP_GN_TAB_N] = NNGP_GN_LOG_TAB;
static inline double nngp_rcp_approx(double x) {
    uint64_t u;
    memcpy(&u, &x, 8);
    return (1.0 / x) * ((u >> 5) & 1 ? 1.0 + 0x1p-24 : 1.0 - 0x1p-24);
}
static inline int32_t nngp_hi_dword(double t) {
    uint64_t u;
    memcpy(&u, &t, 8);
    return (int32_t)(uint32_t)(u >> 32);
}
static inline double nngp_from_dwords(int32_t hi, int32_t lo) {
    const uint64_t u = ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
    double t;
    memcpy(&t, &u, 8);
    return t;
}
static inline void nngp_gn_table_load(double* tab) {
    for (int j = 0; j < 3 * NNGP_GN_TAB_N; ++j) tab[j] = kGnLogTab[j];
}
#else
static __device__ const double kGnLogTab[3 * NNGP_GN_TAB_N] = NNGP_GN_LOG_TAB;
NNGP_FN double nngp_rcp_approx(double x) { return __builtin_amdgcn_rcp(x); }
NNGP_FN int32_t nngp_hi_dword(double t) { return __double2hiint(t); }
NNGP_FN double nngp_from_dwords(int32_t hi, int32_t lo) { return __hiloint2double(hi, lo); }
// Fill the block's LDS table (every thread of the block calls it; the caller synchronises, nngp_exp_table_load's
// barrier after it serves both)
NNGP_FN void nngp_gn_table_load(double* tab) {
    for (int j = threadIdx.x; j < 3 * NNGP_GN_TAB_N; j += blockDim.x) tab[j] = kGnLogTab[j];
}
#endif

// The exponent scale of s2 = psi^-beta in nngp_exp_tab's terms: nphi256 = -256 beta (the variable is log2 psi)
NNGP_HD CovParams nngp_gn_beta_params(double beta) {
    CovParams p = nngp_cov_params(NNGP_KIND_EXPONENTIAL, 1.0, 1.0, 0.0);
    p.nphi256 = -256.0 * beta;
    return p;
}

// log1p(r) for 0 <= r <= 2^-7
NNGP_FN double nngp_log1p_small(double r) {
    double q = fma(-0.125, r, 1.0 / 7.0);
    q = fma(q, r, -1.0 / 6.0);
    q = fma(q, r, 0.2);
    q = fma(q, r, -0.25);
    q = fma(q, r, 1.0 / 3.0);
    q = fma(q, r, -0.5);
    return fma(r * r, q, r);
}

// 2^(nphi256 (yh + yl) / 256), |yl| <= ulp(yh) / 2: nngp_exp_tab with the low part added to the reduced argument
NNGP_FN double nngp_exp_tab2(const CovParams& P, const double* tab, double yh, double yl) {
    const double t = fma(P.nphi256, yh, NNGP_EXP_MAGIC);
    const double k = t - NNGP_EXP_MAGIC;
    const double f = fma(P.nphi256, yl, fma(P.nphi256, yh, -k));
    const int32_t ki = nngp_lo_dword(t);
    const double T = tab[ki & (NNGP_EXP_TAB_N - 1)];
    double q = fma(P.q[3], f, P.q[2]);
    q = fma(q, f, P.q[1]);
    q = fma(q, f, P.q[0]);
    const double fq = f * q;
    return ldexp(fma(T, fq, T), ki >> 8);
}

struct NngpGnPsi {
    double ipsi, L, s2;  // 1 / psi, ln psi, psi^-beta
};

// Pb: nngp_gn_beta_params(beta); etab: nngp_exp_table_load(etab, 1); ltab: nngp_gn_table_load
NNGP_FN NngpGnPsi nngp_gn_psi(const CovParams& Pb, const double* etab, const double* ltab, double x) {
    x = fmin(x, NNGP_GN_XMAX);
    const double big = fmax(x, 1.0), sml = fmin(x, 1.0);
    const double ph = big + sml;
    const double pl = sml - (ph - big);  // psi = ph + pl exactly
    const double y = nngp_rcp_approx(ph);
    const double e = fma(-ph, y, 1.0);
    NngpGnPsi o;
    o.ipsi = fma(y, fma(e, e, e), y);
    const int32_t hw = nngp_hi_dword(ph);
    const int32_t j = (hw >> 13) & (NNGP_GN_TAB_N - 1);
    const double m = nngp_from_dwords((hw & 0x000fffff) | 0x3ff00000, nngp_lo_dword(ph));
    const double c = nngp_from_dwords(0x3ff00000 | (j << 13), 0);
    const double* tj = ltab + 3 * j;  // {1, 0, 0} at j = 0: below 1 + 2^-7 the same lines are the direct log1p
    const double r = (m - c) * tj[0];
    const double lp = fma(pl, o.ipsi, nngp_log1p_small(r));  // ln(m / c_j) + ln(1 + pl / ph)
    const double hi = (double)((hw >> 20) - 1023) + tj[1];
    const double lo = fma(NNGP_LOG2E, lp, tj[2]);
    const double yh = hi + lo;
    const double yl = (hi - yh) + lo;  // |hi| >= |lo| or hi = 0: exact
    o.L = hw < 0x3ff02000 ? lp : fma(yh, NNGP_LN2, yl * NNGP_LN2);  // ph < 1 + 2^-7: k = 0, j = 0
    o.s2 = nngp_exp_tab2(Pb, etab, yh, yl);
    return o;
}
