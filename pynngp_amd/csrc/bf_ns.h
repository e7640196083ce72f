// Nonstationary covariance: every point carries its own variance sigma2_i > 0, decay phi_i > 0 (range 1 / phi_i)
// and nugget tau2_i >= 0.  The Paciorek-Schervish (2006) form with kernel matrices phi_i^-2 I in d = 1, 2 or 3
// dimensions:
//
//   C(i, j) = sigma_i sigma_j x_ij^(d/2) rho(u_ij) + tau2_i delta_ij
//   x_ij    = 2 phi_i phi_j / (phi_i^2 + phi_j^2)                       (<= 1; 1 when phi_i = phi_j)
//   u_ij^2  = 2 |s_i - s_j|^2 phi_i^2 phi_j^2 / (phi_i^2 + phi_j^2)      = |s_i - s_j|^2 x_ij phi_i phi_j
//
// with rho the correlation of the kind at scaled distance u: nngp_cov_d2<NNGP_KIND_GENERIC> at sigma2 = phi = 1.
// With constant fields the model is bf_noise's at v = 1.  Kinds: exponential, Matern-3/2, Matern-5/2, gaussian.
// Each is a scale mixture of gaussians in u^2, which is what makes the construction positive definite in every
// dimension.  The spherical kind is refused: as a function of u^2 it is not completely monotone (it is no such
// mixture -- it is not even positive definite above three dimensions), so the theorem that validates the
// per-point ranges does not cover it.  The general-nu kind is refused as in bf_noise.
//
// One kernel on bf_noise<M, P, false>'s layout (P = grad_lanes(m) lanes per location, rows dealt cyclically,
// right-looking elimination with the value column carried along, block_partials_store's records folded by
// bf_finalize), one instantiation per m: kind and dimension are run-time arguments and the cross form differs from
// the prior form in its q* pointers alone.  What is its own:
//
//   * the partials do not depend on `order`: each location's (log F, r^2 / F) is stored at its local row, ns_fold
//     (bf_ns.hip) adds them 256 rows per record in row order, and the sweep's own records carry only the flags
//     (minima, which no order changes);
//   * the fields travel as one 32-byte record per point, (sigma_i, phi_i, tau2_i, flag), packed once per call by
//     ns_pack (bf_ns.hip) and gathered with the point's coordinates by one aligned 32-byte load.  The record holds
//     sigma = sqrt(sigma2) and phi itself: the pair needs sigma_i sigma_j and phi_i phi_j, and a record of phi^2
//     would cost a square root per pair in every dimension;
//   * per pair one reciprocal, of phi_i^2 + phi_j^2: x = 2 phi_i phi_j / (.), u^2 = d^2 x phi_i phi_j; x^(d/2) is
//     x (d = 2), sqrt x (d = 1) or x sqrt x (d = 3), no pow.  The square root is taken in every dimension and
//     selected: skipping it for d = 2 behind a branch put a diamond at each of the unrolled pair sites and the
//     allocator then needed 454 registers at m = 15 (one wave per SIMD) where the straight-line form needs 162;
//   * ns_pack checks the fields: a point whose sigma2 or phi is not positive and finite, or whose tau2 is negative
//     or not finite, gets the record (1, 1, 1, 1), and a row that holds it in a slot (its own included) reports
//     itself in partials[3], as a row with an out-of-range neighbour index does;
//   * a slot without a point (-1, out of range) sits at a far point with the record (1, 1, 1, 0): x phi_i phi_j <= 2
//     there, u^2 is past the clamp, rho is exactly 0, the diagonal entry is 2 and B is written as 0.
#pragma once
#include "bf_grad.h"

namespace nngp {

static __device__ double4 kNsFarRec[1] = {{1.0, 1.0, 1.0, 0.0}};

struct NsArgs {
    const double* coords;  // (n_points, dim)
    int64_t n_points;
    const int32_t* nbr;    // (n_rows, m), -1 padded
    const int32_t* order;  // or null
    int64_t n_rows, i0;
    int m, kind, dim;
    const double* values;   // (n_points,) or null
    const double4* prec;    // (n_points,) records of the points the neighbour slots index
    const double* qcoords;  // the locations themselves: coords (S = T) or the query points (cross)
    const double* qvalues;  // values (S = T), query values or null
    const double4* qrec;    // prec (S = T) or the query points' records
    double* B;              // (n_rows, m) or null
    double* F;              // (n_rows,) or null
    double* R;              // (n_rows,) or null
    double* rec;            // 4 doubles per block
    double2* lfq;           // (n_rows,) each location's (log F, r^2 / F), by local row
};

// 1 / x for a positive normal x: v_rcp_f64 and the second-order series in e = 1 - x y (nngp_rsqrt's scheme; e^3 is
// below 2^-66)
__device__ __forceinline__ double ns_rcp(double x) {
    const double y = __builtin_amdgcn_rcp(x);
    const double e = fma(-x, y, 1.0);
    return fma(y, fma(e, e, e), y);
}

// C(a, b) off the diagonal: own point (sa, pa), the column's (sb, pb) with pb2 = pb^2, squared distance d2
__device__ __forceinline__ double ns_cov(const CovParams& Pc, const double* etab, double d2, double sa, double pa,
                                         double sb, double pb, double pb2, int dim) {
    const double g = pa * pb, g2 = g + g;
    const double den = fma(pa, pa, pb2), inv = ns_rcp(den);
    // one residual step on the quotient: x is exactly 1 where pa == pb (den == g2 then), so two coincident points
    // of equal fields are exactly collinear, as in the stationary sweeps
    double x = g2 * inv;
    x = fma(fma(-den, x, g2), inv, x);
    const double rho = nngp_cov_d2<NNGP_KIND_GENERIC>(Pc, etab, d2 * (x * g));
    const double sq = nngp_sqrt(x);
    const double pre = dim == 2 ? x : (dim == 1 ? sq : x * sq);
    return (sa * sb) * (pre * rho);
}

template <int M, int P>
__global__ __launch_bounds__(kGradThreads) void bf_ns(const double* __restrict__ coords, int64_t n_points,
                                                      const int32_t* __restrict__ nbr,
                                                      const int32_t* __restrict__ order, int64_t n_rows, int64_t i0,
                                                      const CovParams Pc, const double* __restrict__ values,
                                                      const double4* __restrict__ prec,
                                                      const double* __restrict__ qcoords,
                                                      const double* __restrict__ qvalues,
                                                      const double4* __restrict__ qrec, double* __restrict__ Bout,
                                                      double* __restrict__ Fout, double* __restrict__ Rout,
                                                      double* __restrict__ rec, double2* __restrict__ lfq,
                                                      int dim) {
    static_assert(M >= 1 && M <= 32, "bf_grad.h's lane groups serve 1 <= m <= 32");
    constexpr int NR = M + 1;            // joint rows 0..M (row M = the location)
    constexpr int S = (NR + P - 1) / P;  // local rows per lane
    constexpr int DA = 3;
    __shared__ double etab[NNGP_EXP_TAB_N];
    nngp_exp_table_load(etab, 1.0);
    const int64_t blk = xcd_logical_block(blockIdx.x, gridDim.x);
    const int64_t tid = blk * blockDim.x + threadIdx.x;
    const int q = (int)(threadIdx.x % P);
    const int64_t r = tid / P;
    const bool live = r < n_rows;
    const int64_t rl = live ? r : n_rows - 1;
    const int64_t rr = order != nullptr ? (int64_t)order[rl] : rl;
    const int64_t i = i0 + rr;

    // ---- own rows a = P*s + q: neighbour slot (a < M), the location (a == M), padding (a > M); the record is
    // gathered with the point (branch-free: resolved addresses, as bf_group)
    int32_t jn[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int a = P * s + q;
        jn[s] = nbr[rl * M + (a < M ? a : M - 1)];
    }
    double o[S][DA], z[S], sg[S], ph[S], dg[S];
    bool oval[S];
    bool bad_index = false;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int a = P * s + q;
        const int32_t j = a < M ? jn[s] : -1;
        const bool in_range = j >= 0 && (int64_t)j < n_points;
        bad_index |= j != -1 && !in_range;
        oval[s] = in_range;
        const bool self = a == M;
        const double* pc = self ? qcoords + i * dim : (in_range ? coords + (int64_t)j * dim : far_point<DA>(a));
        const double* pv = self ? (qvalues != nullptr ? qvalues + i : kZeroValue)
                                : ((values != nullptr && in_range) ? values + j : kZeroValue);
        const double4* pr = self ? qrec + i : (in_range ? prec + j : kNsFarRec);
        load_point_rt(pc, dim, o[s]);
        z[s] = *pv;
        const double4 w = *pr;
        sg[s] = w.x;
        ph[s] = w.y;
        dg[s] = fma(w.x, w.x, w.z);
        bad_index |= w.w != 0.0;
    }

    // ---- joint block rows: R[s][b], b < min(P*s + P, NR); column by column, so one broadcast point is live
    double R[S][NR];
#pragma unroll
    for (int b = 0; b < NR; ++b) {
        double xb[DA];
#pragma unroll
        for (int k = 0; k < DA; ++k) xb[k] = gbcast<P>(o[b / P][k], b % P);
        const double sb = gbcast<P>(sg[b / P], b % P);
        const double pb = gbcast<P>(ph[b / P], b % P);
        const double pb2 = pb * pb;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int a = P * s + q;
            if (b >= P * s + P) continue;  // beyond this local row's width
            if (b < P * s) {
                R[s][b] = ns_cov(Pc, etab, point_d2<DA>(o[s], xb), sg[s], ph[s], sb, pb, pb2, dim);
            } else if (b < P * s + P - 1) {  // diagonal block: lane-dependent
                const double c = ns_cov(Pc, etab, point_d2<DA>(o[s], xb), sg[s], ph[s], sb, pb, pb2, dim);
                R[s][b] = b < a ? c : (b == a ? dg[s] : 0.0);
            } else {
                R[s][b] = b == a ? dg[s] : 0.0;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }

    // ---- right-looking elimination; the owner of row p keeps 1/L[p][p] in R[p/P][p]
    bool bad = false;
#pragma unroll
    for (int p = 0; p < M; ++p) {
        const int qp = p % P, sp = p / P;
        const double piv = gbcast<P>(R[sp][p], qp);
        bad |= !(piv > 0.0);
        const double ip = nngp_rsqrt(piv);
        R[sp][p] = q == qp ? ip : R[sp][p] * ip;
#pragma unroll
        for (int s = sp + 1; s < S; ++s) R[s][p] *= ip;
        z[sp] = q == qp ? z[sp] * ip : z[sp];
        const double zp = gbcast<P>(z[sp], qp);
        double lb[NR];
#pragma unroll
        for (int b = p + 1; b < NR; ++b) lb[b] = gbcast<P>(R[b / P][p], b % P);
#pragma unroll
        for (int s = sp; s < S; ++s) {
#pragma unroll
            for (int b = p + 1; b < NR; ++b) {
                if (b >= P * s + P) continue;
                R[s][b] = fma(-R[s][p], lb[b], R[s][b]);
            }
            if (s == sp) {
                if (P > 1) z[s] = q > qp ? fma(-R[s][p], zp, z[s]) : z[s];
            } else {
                z[s] = fma(-R[s][p], zp, z[s]);
            }
        }
    }
    const double F = gbcast<P>(R[M / P][M], M % P);
    const double res = gbcast<P>(z[M / P], M % P);
    bad |= !(F > 0.0);

    // ---- b = L_N^-T v (v = row M of L); lane q ends with b of its own rows
    double bown[S];
#pragma unroll
    for (int s = 0; s < S; ++s) bown[s] = 0.0;
    if (Bout != nullptr) {
#pragma unroll
        for (int a = M - 1; a >= 0; --a) {
            double pb = 0.0;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (P * s + P - 1 <= a) continue;  // every row of this local row is <= a
                const int ar = P * s + q;
                pb = (ar > a && ar < M) ? fma(R[s][a], bown[s], pb) : pb;
            }
            const double tb = gsum<P>(pb);
            const double va = gbcast<P>(R[M / P][a], M % P);
            const double iva = gbcast<P>(R[a / P][a], a % P);
            const double ba = (va - tb) * iva;
            bown[a / P] = q == a % P ? ba : bown[a / P];
        }
    }
    const bool lead = live && q == 0;
    // the two sums go out per location, indexed by the local row and not by the thread: ns_fold (bf_ns.hip) adds
    // them in row order, so the partials' bits do not depend on `order`; the block record carries the flags
    double badp = INFINITY, badi = INFINITY;
    if (lead) {
        lfq[rr] = make_double2(log(F), res * res / F);
        if (bad) badp = (double)i;
    }
    if (live && bad_index) badi = (double)i;
    if (Bout != nullptr && live) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int a = P * s + q;
            if (a < M) Bout[rr * M + a] = bad ? NAN : (oval[s] ? bown[s] : 0.0);
        }
    }
    if (Fout != nullptr && lead) Fout[rr] = bad ? NAN : F;
    if (Rout != nullptr && lead) Rout[rr] = bad ? NAN : res;
    block_partials_store(0.0, 0.0, badp, badi, rec, blk);
}

template <int M>
static bool launch_ns_if(const NsArgs& a, hipStream_t s) {
    if (a.m != M) return false;
    constexpr int P = grad_lanes(M);
    const CovParams Pc = nngp_cov_params(a.kind, 1.0, 1.0, 0.0);  // rho(u): unit variance and decay
    const dim3 grid((unsigned)bf_grad_blocks(a.n_rows, M)), block(kGradThreads);
    hipLaunchKernelGGL((bf_ns<M, P>), grid, block, 0, s, a.coords, a.n_points, a.nbr, a.order, a.n_rows, a.i0, Pc,
                       a.values, a.prec, a.qcoords, a.qvalues, a.qrec, a.B, a.F, a.R, a.rec, a.lfq, a.dim);
    return true;
}

// the instantiation units (bf_ns_m*.hip); the packing kernel, the dispatch and the fold (bf_ns.hip)
bool bf_ns_launch_a(const NsArgs& a, hipStream_t s);
bool bf_ns_launch_b(const NsArgs& a, hipStream_t s);
bool bf_ns_launch_c(const NsArgs& a, hipStream_t s);
bool bf_ns_launch_d(const NsArgs& a, hipStream_t s);
bool bf_ns_launch_e(const NsArgs& a, hipStream_t s);
bool bf_ns_launch_f(const NsArgs& a, hipStream_t s);
bool bf_ns_launch_g(const NsArgs& a, hipStream_t s);
bool bf_ns_launch_h(const NsArgs& a, hipStream_t s);
// out[i] = (sqrt sigma2_i, phi_i, tau2_i, 0), or (1, 1, 1, 1) for a point whose fields are refused
hipError_t bf_ns_pack_launch(const double* sigma2, const double* phi, const double* tau2, int64_t n, double4* out,
                             hipStream_t s);
hipError_t bf_ns_launch(const NsArgs& a, double* partials, hipStream_t s);

}  // namespace nngp
