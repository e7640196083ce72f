// Analytic gradient of the NNGP log-likelihood in (sigma2, phi_1..phi_dim, tau2) for a covariance with one
// decay per axis, u = sqrt(sum_k (phi_k (a_k - b_k))^2): one fused sweep on bf_grad.h's layout.
//
// Same lane groups (grad_lanes(M)), elimination, two back-substitutions and masks as bf_grad<M, P>.  Two
// differences:
//
//   * load: each point is multiplied by phi_k as it is loaded, once per point (far points of empty or
//     out-of-range slots are left where they are), and the covariance runs at phi = 1 on the scaled
//     coordinates: the d2max / umax clamps apply to the scaled distance unchanged;
//   * second pass: with x = d^2 (scaled), dv = d e poly(u) as in bf_grad (u = d) and delta_k the scaled
//     coordinate difference,
//         dC_ab / dphi_k = sigma2 rho'(u) delta_k^2 / (u phi_k) = (dv / x) delta_k^2 / phi_k.
//     w = dv / x = e poly(u) / d comes from the reciprocal square root the square root is built on (one more
//     FMA, no division); it is exactly 0 for a masked pair and where x is the floor (coincident points, where
//     every delta_k^2 is 0 too).  Per pair w u_a u_b and w (alpha_a u_b + alpha_b u_a) are formed once and
//     three pairs of accumulators take delta_k^2 times them; 1 / phi_k is applied once after the group sums.
//
// G is (n_rows, dim + 2) in the order (sigma2, phi_1..phi_dim, tau2).  The block records hold the family's four
// sums and five gradient sums (sigma2, phi_1, phi_2, phi_3, tau2; the unused axes are exactly 0).
#pragma once
#include "bf_grad.h"

namespace nngp {

struct GradAnisoArgs {
    const double* coords;  // (n_points, dim), raw
    int64_t n_points;
    const int32_t* nbr;    // (n_rows, m), -1 padded
    const int32_t* order;  // or null
    int64_t n_rows, i0;
    int m, kind, dim;
    double sigma2, phi[3], tau2;  // phi[k] = 1 for k >= dim
    const double* values;  // (n_points,)
    double* G;             // (n_rows, dim + 2) or null
    double* rec;           // kGradAnisoRec doubles per block
};

struct AnisoPhi {
    double phi[3], iphi[3];  // iphi = 1 / phi
};

// per-block record: sum log F, sum r^2/F, first bad-pivot row, first bad-index row, the five gradient sums
// (sigma2, phi_1, phi_2, phi_3, tau2), 0 x 3
constexpr int kGradAnisoRec = 12;
constexpr int kGradAnisoSums = 5;

// block_grad_store with five gradient sums.  Every thread of the block calls it.
__device__ __forceinline__ void block_grad_aniso_store(double lf, double qq, double badp, double badi,
                                                       const double (&g)[kGradAnisoSums], double* rec, int64_t block) {
    __shared__ double sh[kGradThreads / 64][kGradAnisoRec];
    lf = wave_sum(lf);
    qq = wave_sum(qq);
    double gs[kGradAnisoSums];
#pragma unroll
    for (int k = 0; k < kGradAnisoSums; ++k) gs[k] = wave_sum(g[k]);
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
        for (int k = 0; k < kGradAnisoSums; ++k) sh[w][4 + k] = gs[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0, c = INFINITY, d = INFINITY, e[kGradAnisoSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < kGradThreads / 64; ++k) {
            a += sh[k][0];
            b += sh[k][1];
            c = fmin(c, sh[k][2]);
            d = fmin(d, sh[k][3]);
            for (int j = 0; j < kGradAnisoSums; ++j) e[j] += sh[k][4 + j];
        }
        double* o = rec + kGradAnisoRec * block;
        o[0] = a;
        o[1] = b;
        o[2] = c;
        o[3] = d;
        for (int j = 0; j < kGradAnisoSums; ++j) o[4 + j] = e[j];
        for (int j = 4 + kGradAnisoSums; j < kGradAnisoRec; ++j) o[j] = 0.0;
    }
}

template <int M, int P>
__global__ __launch_bounds__(kGradThreads) void bf_grad_aniso(const double* __restrict__ coords, int64_t n_points,
                                                              const int32_t* __restrict__ nbr,
                                                              const int32_t* __restrict__ order, int64_t n_rows,
                                                              int64_t i0, const CovParams Pc, const GradParams Gp,
                                                              const AnisoPhi Ph, const double* __restrict__ values,
                                                              double* __restrict__ Gout, double* __restrict__ rec,
                                                              int dim) {
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

    // ---- own rows a = P*s + q: neighbour slot (a < M), the location (a == M), padding (a > M); a point that
    // exists is scaled axis by axis as it arrives
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
#pragma unroll
        for (int k = 0; k < DA; ++k) o[s][k] *= (self || in_range) ? Ph.phi[k] : 1.0;
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

    // ---- second pass over the own strict-lower pairs (a > b): the two sums of every axis
    double dfp[DA], drp[DA];
#pragma unroll
    for (int k = 0; k < DA; ++k) dfp[k] = drp[k] = 0.0;
    // (the coordinates pass through an opaque barrier, as in bf_grad: without it the compiler keeps the build
    // pass's broadcasts alive across the elimination, or evaluates this pass's covariances ahead of it)
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
            // point_d2's order, with the squared differences kept
            double t2[DA];
            double x2 = NNGP_D2_FLOOR;
#pragma unroll
            for (int k = DA - 1; k >= 0; --k) {
                const double t = o[s][k] - xb[k];
                t2[k] = t * t;
                x2 = fma(t, t, x2);
            }
            const double x = fmin(x2, Pc.d2max);
            // nngp_sqrt's steps, with 1 / sqrt(x) from the same correction
            const double y = nngp_rsq_approx(x);
            const double sx = x * y;
            const double ex = fma(-sx, y, 1.0);
            const double gx = ex * fma(0.375, ex, 0.5);
            const double d = fma(sx, gx, sx);
            const double id = fma(y, gx, y);
            const double e = nngp_exp_tab(Pc, etab, Pc.gauss ? x : d);  // sigma2 e(u)
            const double u = fmin(d, Pc.umax);
            const double wv = id * e * fma(u, fma(u, Gp.g[2], Gp.g[1]), Gp.g[0]);  // dv / x
            const double w = (a > b && rowok[s] && colok && x > NNGP_D2_FLOOR) ? wv : 0.0;
            const double wf = w * uo[s] * ub;
            const double wr = w * fma(ao[s], ub, alb * uo[s]);
#pragma unroll
            for (int k = 0; k < DA; ++k) {
                dfp[k] = fma(t2[k], wf, dfp[k]);
                drp[k] = fma(t2[k], wr, drp[k]);
            }
        }
        // (the six sums pass through an opaque barrier per column: without it the compiler sinks every column's
        // accumulation below the last column and keeps each pair's factors until then -- 916 B of scratch per
        // lane at m = 15; the scheduling barrier alone orders only what is already placed in its column)
#pragma unroll
        for (int k = 0; k < DA; ++k) asm volatile("" : "+v"(dfp[k]), "+v"(drp[k]));
        __builtin_amdgcn_sched_barrier(0);
    }
    const double nb2 = gsum<P>(nbp);
    const double adb = gsum<P>(abp);

    const double iF = 1.0 / F;
    const double w = 1.0 - res * res * iF;  // 1 - r^2 / F
    const double dFt = 1.0 + nb2;
    const double dFs = (F - Gp.tau2 * dFt) * Gp.isig2;
    const double drs = -Gp.tau2 * adb * Gp.isig2;
    double g[kGradAnisoSums];
    g[0] = -0.5 * iF * fma(dFs, w, 2.0 * res * drs);
#pragma unroll
    for (int k = 0; k < DA; ++k) {
        const double dFphi = 2.0 * gsum<P>(dfp[k]) * Ph.iphi[k];
        const double drphi = -gsum<P>(drp[k]) * Ph.iphi[k];
        g[1 + k] = -0.5 * iF * fma(dFphi, w, 2.0 * res * drphi);
    }
    g[4] = -0.5 * iF * fma(dFt, w, 2.0 * res * adb);

    const bool lead = live && q == 0;
    if (Gout != nullptr && lead) {
        double* go = Gout + rr * (dim + 2);
        go[0] = bad ? NAN : g[0];
#pragma unroll
        for (int k = 0; k < DA; ++k)
            if (k < dim) go[1 + k] = bad ? NAN : g[1 + k];
        go[1 + dim] = bad ? NAN : g[4];
    }
    double lf = 0.0, qq = 0.0, badp = INFINITY, badi = INFINITY;
    if (lead) {
        lf = log(F);
        qq = res * res * iF;
        if (bad) badp = (double)i;
    } else {
#pragma unroll
        for (int k = 0; k < kGradAnisoSums; ++k) g[k] = 0.0;
    }
    if (live && bad_index) badi = (double)i;
    block_grad_aniso_store(lf, qq, badp, badi, g, rec, blk);
}

template <int M>
static bool launch_grad_aniso_if(const GradAnisoArgs& a, hipStream_t s) {
    if (a.m != M) return false;
    constexpr int P = grad_lanes(M);
    const CovParams Pc = nngp_cov_params(a.kind, a.sigma2, 1.0, a.tau2);
    const GradParams Gp = grad_params(a.kind, a.sigma2, a.tau2);
    AnisoPhi Ph;
    for (int k = 0; k < 3; ++k) {
        Ph.phi[k] = k < a.dim ? a.phi[k] : 1.0;
        Ph.iphi[k] = 1.0 / Ph.phi[k];
    }
    hipLaunchKernelGGL((bf_grad_aniso<M, P>), dim3((unsigned)bf_grad_blocks(a.n_rows, M)), dim3(kGradThreads), 0, s,
                       a.coords, a.n_points, a.nbr, a.order, a.n_rows, a.i0, Pc, Gp, Ph, a.values, a.G, a.rec, a.dim);
    return true;
}

// the instantiation units (bf_grad_aniso_m*.hip) and the dispatch + fold (bf_grad_aniso.hip)
bool bf_grad_aniso_launch_a(const GradAnisoArgs& a, hipStream_t s);
bool bf_grad_aniso_launch_b(const GradAnisoArgs& a, hipStream_t s);
bool bf_grad_aniso_launch_c(const GradAnisoArgs& a, hipStream_t s);
bool bf_grad_aniso_launch_d(const GradAnisoArgs& a, hipStream_t s);
bool bf_grad_aniso_launch_e(const GradAnisoArgs& a, hipStream_t s);
bool bf_grad_aniso_launch_f(const GradAnisoArgs& a, hipStream_t s);
bool bf_grad_aniso_launch_g(const GradAnisoArgs& a, hipStream_t s);
bool bf_grad_aniso_launch_h(const GradAnisoArgs& a, hipStream_t s);
hipError_t bf_grad_aniso_launch(const GradAnisoArgs& a, double* partials, double* grad, hipStream_t s);

}  // namespace nngp
