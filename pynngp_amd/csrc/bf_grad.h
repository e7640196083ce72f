// Analytic gradient of the NNGP log-likelihood in (sigma2, phi, tau2), one fused sweep.
//
// bf_group.h's layout (P = 2 .. 64 lanes per location, joint-block rows dealt cyclically, DPP broadcasts and
// butterfly sums, right-looking elimination with the value column carried along) with three added
// steps.  For location i with joint block C (nugget on the whole diagonal), c = C[:k, k],
// b = C_N^-1 c, a = C_N^-1 y_N, u = [-b; 1], alpha = [a; 0], F = u^T C u, r = y_i - b^T y_N:
//
//   d l_i / d theta = -1/2 [ (dF / F) (1 - r^2 / F) + 2 r dr / F ]
//   dF = u^T (dC/dtheta) u      (b minimises F: no db term)
//   dr = -alpha^T (dC/dtheta) u
//
//   tau2:    dC = I              dF = 1 + |b|^2                        dr = a.b
//   sigma2:  dC = (C - tau2 I) / sigma2, C u = [0; F]
//                                dF = (F - tau2 (1 + |b|^2)) / sigma2  dr = -tau2 (a.b) / sigma2
//   phi:     D_ab = sigma2 d_ab rho'(phi d_ab), zero diagonal
//                                dF = 2 sum_{a>b} D_ab u_a u_b         dr = -sum_{a>b} D_ab (alpha_a u_b + alpha_b u_a)
//
//   * z[s] after the elimination is L^-1 y_N, so a comes from a second back-substitution that shares
//     the factor reads, pivots and butterflies of the one for b;
//   * u and alpha are broadcast column by column in a second pass over each lane's own strict-lower
//     pairs, which recomputes d^2 from the coordinates the lane still holds: four scalars per lane
//     (the two phi sums, |b|^2, a.b), no derivative block, no stored vector;
//   * slots without a point (-1 padding) or with an out-of-range index are masked: u, alpha and D are
//     exactly 0 there.
//
// One instantiation per m: the kind (0..4) and the dimension (1..3) are runtime arguments, as in
// bf_group<M, NNGP_KIND_GENERIC, P, 0>.  rho'(u) of every kind is e(u) (g0 + g1 u + g2 u^2) with e the
// kind's exponential factor (1 for the spherical kind, u clamped at 1 where the bracket is 0).
#pragma once
#include "bf_group.h"

namespace nngp {

struct GradParams {
    double g[3];   // rho'(u) = e(u) (g[0] + g[1] u + g[2] u^2)
    double tau2;
    double isig2;  // 1 / sigma2
};

inline GradParams grad_params(int kind, double sigma2, double tau2) {
    GradParams g;
    g.g[0] = kind == NNGP_KIND_EXPONENTIAL ? -1.0 : kind == NNGP_KIND_SPHERICAL ? -1.5 : 0.0;
    g.g[1] = kind == NNGP_KIND_MATERN32 ? -1.0 : kind == NNGP_KIND_MATERN52 ? -1.0 / 3.0 : kind == NNGP_KIND_GAUSSIAN ? -2.0 : 0.0;
    g.g[2] = kind == NNGP_KIND_MATERN52 ? -1.0 / 3.0 : kind == NNGP_KIND_SPHERICAL ? 1.5 : 0.0;
    g.tau2 = tau2;
    g.isig2 = 1.0 / sigma2;
    return g;
}

struct GradArgs {
    const double* coords;  // (n_points, dim)
    int64_t n_points;
    const int32_t* nbr;    // (n_rows, m), -1 padded
    const int32_t* order;  // or null
    int64_t n_rows, i0;
    int m, kind, dim;
    double sigma2, phi, tau2;
    const double* values;  // (n_points,)
    double* G;             // (n_rows, 3) or null
    double* rec;           // kGradRec doubles per block
};

// group broadcast / sum for P lanes per location: DPP inside a quad (bf_group.h) up to P = 4, the cross-lane
// permute (no memory traffic) for the 8- and 16-lane groups of the larger m
template <int P>
__device__ __forceinline__ double gbcast(double v, int src) {
    if constexpr (P <= 4) return grp_bcast<P>(v, src);
    else return __shfl(v, src, P);
}
template <int P>
__device__ __forceinline__ double gsum(double v) {
    if constexpr (P <= 4) return grp_sum<P>(v);
    else {
        v = grp_sum<4>(v);
        v = v + __shfl_xor(v, 4);
        if constexpr (P > 8) v = v + __shfl_xor(v, 8);
        if constexpr (P > 16) v = v + __shfl_xor(v, 16);
        if constexpr (P > 32) v = v + __shfl_xor(v, 32);
        return v;
    }
}

// per-block record: sum log F, sum r^2/F, first bad-pivot row, first bad-index row, the three gradient sums, 0
constexpr int kGradRec = 8;
constexpr int kGradThreads = 256;
// lanes per location, chosen per m so that every instantiation stays in registers with the fewest lanes (permutes cost per lane)
// (DESIGN.md 4.3c has the figures): DPP quads up to m = 15, 8 lanes to m = 23, 16 to m = 31 and the whole
// wavefront at m = 32
constexpr int grad_lanes(int m) { return m <= 8 ? 2 : m <= 15 ? 4 : m <= 23 ? 8 : m <= 31 ? 16 : 64; }
inline int64_t bf_grad_blocks(int64_t n_rows, int m) { return (n_rows * grad_lanes(m) + kGradThreads - 1) / kGradThreads; }

// Fixed-order reduction of one block's sums into rec[kGradRec * block ..] (block_partials_store with the
// three gradient sums alongside).  Every thread of the block calls it.
__device__ __forceinline__ void block_grad_store(double lf, double qq, double badp, double badi, const double (&g)[3],
                                                 double* rec, int64_t block) {
    __shared__ double sh[kGradThreads / 64][kGradRec];
    lf = wave_sum(lf);
    qq = wave_sum(qq);
    double gs[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) gs[k] = wave_sum(g[k]);
    if (__any(badp != INFINITY || badi != INFINITY)) {  // wave-uniform; rare
        badp = wave_min(badp);
        badi = wave_min(badi);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh[w][0] = lf;
        sh[w][1] = qq;
        sh[w][2] = badp;
        sh[w][3] = badi;
#pragma unroll
        for (int k = 0; k < 3; ++k) sh[w][4 + k] = gs[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0, c = INFINITY, d = INFINITY, e[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < kGradThreads / 64; ++k) {
            a += sh[k][0];
            b += sh[k][1];
            c = fmin(c, sh[k][2]);
            d = fmin(d, sh[k][3]);
            for (int j = 0; j < 3; ++j) e[j] += sh[k][4 + j];
        }
        double* o = rec + kGradRec * block;
        o[0] = a;
        o[1] = b;
        o[2] = c;
        o[3] = d;
        o[4] = e[0];
        o[5] = e[1];
        o[6] = e[2];
        o[7] = 0.0;
    }
}

template <int M, int P>
__global__ __launch_bounds__(kGradThreads) void bf_grad(const double* __restrict__ coords, int64_t n_points,
                                                        const int32_t* __restrict__ nbr,
                                                        const int32_t* __restrict__ order, int64_t n_rows, int64_t i0,
                                                        const CovParams Pc, const GradParams Gp,
                                                        const double* __restrict__ values, double* __restrict__ Gout,
                                                        double* __restrict__ rec, int dim) {
    static_assert(M >= 1 && M <= 32, "the validity mask holds one bit per neighbour slot");
    constexpr int NR = M + 1;            // joint rows 0..M (row M = the location)
    constexpr int S = (NR + P - 1) / P;  // local rows per lane
    constexpr int DA = 3;
    __shared__ double etab[NNGP_EXP_TAB_N];
    nngp_exp_table_load(etab, Pc.sigma2);
    const int64_t blk = xcd_logical_block(blockIdx.x, gridDim.x);
    const int64_t tid = blk * blockDim.x + threadIdx.x;
    const int q = (int)(threadIdx.x % P);
    const int64_t r = tid / P;
    const bool live = r < n_rows;
    const int64_t rl = live ? r : n_rows - 1;
    const int64_t rr = order != nullptr ? (int64_t)order[rl] : rl;
    const int64_t i = i0 + rr;

    // ---- own rows a = P*s + q: neighbour slot (a < M), the location (a == M), padding (a > M)
    int32_t jn[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int a = P * s + q;
        jn[s] = nbr[rl * M + (a < M ? a : M - 1)];
    }
    double o[S][DA], z[S];
    bool oval[S];
    bool bad_index = false;
    uint32_t vm = 0;  // bit a: neighbour slot a holds a point
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int a = P * s + q;
        const int32_t j = a < M ? jn[s] : -1;
        const bool in_range = j >= 0 && (int64_t)j < n_points;
        bad_index |= j != -1 && !in_range;
        oval[s] = in_range;
        vm |= in_range ? (1u << (a & 31)) : 0u;
        const bool self = a == M;
        const double* pc = self ? coords + i * dim : (in_range ? coords + (int64_t)j * dim : far_point<DA>(a));
        const double* pv = self ? values + i : (in_range ? values + j : kZeroValue);
        load_point_rt(pc, dim, o[s]);
        z[s] = *pv;
    }
    if constexpr (P > 1) vm |= (uint32_t)__builtin_amdgcn_mov_dpp((int)vm, 0xB1, 0xf, 0xf, true);
    if constexpr (P > 2) vm |= (uint32_t)__builtin_amdgcn_mov_dpp((int)vm, 0x4E, 0xf, 0xf, true);
    if constexpr (P > 4) vm |= (uint32_t)__shfl_xor((int)vm, 4);
    if constexpr (P > 8) vm |= (uint32_t)__shfl_xor((int)vm, 8);
    if constexpr (P > 16) vm |= (uint32_t)__shfl_xor((int)vm, 16);
    if constexpr (P > 32) vm |= (uint32_t)__shfl_xor((int)vm, 32);

    // ---- joint block rows: R[s][b], b < min(P*s + P, NR); column by column, so one broadcast point is live
    double R[S][NR];
#pragma unroll
    for (int b = 0; b < NR; ++b) {
        double xb[DA];
#pragma unroll
        for (int k = 0; k < DA; ++k) xb[k] = gbcast<P>(o[b / P][k], b % P);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int a = P * s + q;
            if (b >= P * s + P) continue;  // beyond this local row's width
            if (b < P * s) {
                R[s][b] = nngp_cov_d2<NNGP_KIND_GENERIC>(Pc, etab, point_d2<DA>(o[s], xb));
            } else if (b < P * s + P - 1) {  // diagonal block: lane-dependent
                const double c = nngp_cov_d2<NNGP_KIND_GENERIC>(Pc, etab, point_d2<DA>(o[s], xb));
                R[s][b] = b < a ? c : (b == a ? Pc.diag : 0.0);
            } else {
                R[s][b] = b == a ? Pc.diag : 0.0;
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

    // ---- b = L_N^-T v (v = row M of L) and a = L_N^-T z_N together; lane q ends with b, a of its own rows
    double bown[S], aown[S];
#pragma unroll
    for (int s = 0; s < S; ++s) bown[s] = aown[s] = 0.0;
#pragma unroll
    for (int a = M - 1; a >= 0; --a) {
        double pb = 0.0, pa = 0.0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (P * s + P - 1 <= a) continue;  // every row of this local row is <= a
            const int ar = P * s + q;
            const bool in = ar > a && ar < M;
            pb = in ? fma(R[s][a], bown[s], pb) : pb;
            pa = in ? fma(R[s][a], aown[s], pa) : pa;
        }
        const double tb = gsum<P>(pb);
        const double ta = gsum<P>(pa);
        const double va = gbcast<P>(R[M / P][a], M % P);
        const double za = gbcast<P>(z[a / P], a % P);
        const double iva = gbcast<P>(R[a / P][a], a % P);
        const double ba = (va - tb) * iva;
        const double aa = (za - ta) * iva;
        bown[a / P] = q == a % P ? ba : bown[a / P];
        aown[a / P] = q == a % P ? aa : aown[a / P];
    }

    // ---- u = [-b; 1], alpha = [a; 0], exactly 0 in slots without a point; |b|^2 and a.b
    double uo[S], ao[S];
    bool rowok[S];
    double nbp = 0.0, abp = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int a = P * s + q;
        const bool nb = a < M && oval[s];
        rowok[s] = nb || a == M;
        uo[s] = nb ? -bown[s] : (a == M ? 1.0 : 0.0);
        ao[s] = nb ? aown[s] : 0.0;
        nbp = nb ? fma(bown[s], bown[s], nbp) : nbp;
        abp = nb ? fma(aown[s], bown[s], abp) : abp;
    }

    // ---- second pass over the own strict-lower pairs (a > b): the two phi sums
    double dfp = 0.0, drp = 0.0;
    // (the coordinates pass through an opaque barrier: without it the compiler keeps the build pass's
    // broadcasts alive across the elimination, or evaluates this pass's covariances ahead of it)
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int k = 0; k < DA; ++k) asm volatile("" : "+v"(o[s][k]));
#pragma unroll
    for (int b = 0; b < M; ++b) {
        double xb[DA];
#pragma unroll
        for (int k = 0; k < DA; ++k) xb[k] = gbcast<P>(o[b / P][k], b % P);
        const double ub = gbcast<P>(uo[b / P], b % P);
        const double alb = gbcast<P>(ao[b / P], b % P);
        const bool colok = (vm >> (b & 31)) & 1u;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (P * s + P - 1 <= b) continue;  // every row of this local row is <= b
            const int a = P * s + q;
            const double x = fmin(point_d2<DA>(o[s], xb), Pc.d2max);
            const double d = nngp_sqrt(x);
            const double e = nngp_exp_tab(Pc, etab, Pc.gauss ? x : d);  // sigma2 e(u)
            const double u = fmin(Pc.phi * d, Pc.umax);
            const double dv = d * e * fma(u, fma(u, Gp.g[2], Gp.g[1]), Gp.g[0]);
            const double D = (a > b && rowok[s] && colok) ? dv : 0.0;
            dfp = fma(D * uo[s], ub, dfp);
            drp = fma(D, fma(ao[s], ub, alb * uo[s]), drp);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    const double nb2 = gsum<P>(nbp);
    const double adb = gsum<P>(abp);
    const double dFphi = 2.0 * gsum<P>(dfp);
    const double drphi = -gsum<P>(drp);

    const double iF = 1.0 / F;
    const double w = 1.0 - res * res * iF;  // 1 - r^2 / F
    const double dFt = 1.0 + nb2;
    const double dFs = (F - Gp.tau2 * dFt) * Gp.isig2;
    const double drs = -Gp.tau2 * adb * Gp.isig2;
    double g[3];
    g[0] = -0.5 * iF * fma(dFs, w, 2.0 * res * drs);
    g[1] = -0.5 * iF * fma(dFphi, w, 2.0 * res * drphi);
    g[2] = -0.5 * iF * fma(dFt, w, 2.0 * res * adb);

    const bool lead = live && q == 0;
    if (Gout != nullptr && lead) {
#pragma unroll
        for (int k = 0; k < 3; ++k) Gout[rr * 3 + k] = bad ? NAN : g[k];
    }
    double lf = 0.0, qq = 0.0, badp = INFINITY, badi = INFINITY;
    if (lead) {
        lf = log(F);
        qq = res * res * iF;
        if (bad) badp = (double)i;
    } else {
        g[0] = g[1] = g[2] = 0.0;
    }
    if (live && bad_index) badi = (double)i;
    block_grad_store(lf, qq, badp, badi, g, rec, blk);
}

template <int M>
static bool launch_grad_if(const GradArgs& a, hipStream_t s) {
    if (a.m != M) return false;
    constexpr int P = grad_lanes(M);
    const CovParams Pc = nngp_cov_params(a.kind, a.sigma2, a.phi, a.tau2);
    const GradParams Gp = grad_params(a.kind, a.sigma2, a.tau2);
    hipLaunchKernelGGL((bf_grad<M, P>), dim3((unsigned)bf_grad_blocks(a.n_rows, M)), dim3(kGradThreads), 0, s, a.coords,
                       a.n_points, a.nbr, a.order, a.n_rows, a.i0, Pc, Gp, a.values, a.G, a.rec, a.dim);
    return true;
}

// the instantiation units (bf_grad_m*.hip) and the dispatch + fold (bf_grad.hip)
bool bf_grad_launch_a(const GradArgs& a, hipStream_t s);
bool bf_grad_launch_b(const GradArgs& a, hipStream_t s);
bool bf_grad_launch_c(const GradArgs& a, hipStream_t s);
bool bf_grad_launch_d(const GradArgs& a, hipStream_t s);
bool bf_grad_launch_e(const GradArgs& a, hipStream_t s);
bool bf_grad_launch_f(const GradArgs& a, hipStream_t s);
bool bf_grad_launch_g(const GradArgs& a, hipStream_t s);
bool bf_grad_launch_h(const GradArgs& a, hipStream_t s);
hipError_t bf_grad_launch(const GradArgs& a, double* partials, double* grad, hipStream_t s);
// the fold alone: n_blocks records of kGradRec doubles (block_grad_store) -> partials[4], grad[3]
hipError_t bf_grad_fold_launch(const double* rec, int64_t n_blocks, double* partials, double* grad, hipStream_t s);

}  // namespace nngp
