// Analytic gradient of the NNGP log-likelihood in (sigma2, phi, tau2, nu) for the general-smoothness Matern kind,
// one fused sweep: bf_grad.h's kernel (its layout, elimination, the two back-substitutions, the second pass
// over each lane's own strict-lower pairs, its masks) with the covariance and its derivatives from tables.
//
//   * Build pass: C_ab = sigma2 rho(t), t = phi^2 d^2, from the launch's rho table copied to dynamic LDS
//     (nngp_matern_tab, as bf_group<M, NNGP_KIND_MATERN, ...> reads it).
//   * Second pass: the two derivative functions of the correlation (nngp_math.h, nngp_matern_drho),
//       h(u) = u rho'(u)          d C_ab / d phi = sigma2 h / phi
//       n(u) = d rho / d nu       d C_ab / d nu  = sigma2 n
//     from one derivative table with rho's geometry (nngp_matern_tab_d: a bin's h and n coefficients adjacent),
//     read from global memory: rho's table alone takes up to 100 KB of LDS (NNGP_MT_MAX_OCT octaves), three
//     would not fit the 160 KB of a workgroup for every nu the forward sweep accepts, and a bin's 160 bytes
//     stay in L2.  Four running sums (dF and dr for phi and for nu) share the products u_a u_b and
//     alpha_a u_b + alpha_b u_a; sigma2 / phi and sigma2 are applied once per location.
//   * h and n are exactly 0 for coincident points (the end octave, or the below-table series' floor), for padded
//     slots (far points: the last octave) and under the masks rowok, colok, a > b.
//
// Output: g[4] per location in the order (sigma2, phi, tau2, nu); the block record keeps kGradRec columns.
#pragma once
#include "bf_grad.h"

namespace nngp {

struct GradMaternArgs {
    const double* coords;  // (n_points, dim)
    int64_t n_points;
    const int32_t* nbr;    // (n_rows, m), -1 padded
    const int32_t* order;  // or null
    int64_t n_rows, i0;
    int m, dim;
    double sigma2, phi, tau2, nu;
    const double* values;  // (n_points,)
    double* G;             // (n_rows, 4) or null
    double* rec;           // kGradRec doubles per block
    double* tab;           // the rho table, then the derivative table (matern_tables_launch)
    CovParams Pc;          // set by bf_grad_matern_launch
};

// doubles of the launch's tables for noct octaves: rho, then (h, n) per bin
inline size_t grad_matern_table_doubles(int noct) { return (size_t)noct * NNGP_MT_K * NNGP_MT_NC * 3; }

// Fixed-order reduction of one block's sums into rec[kGradRec * block ..]: block_grad_store (bf_grad.h) with the
// fourth gradient sum in the record's last column, which bf_grad leaves 0.  Every thread of the block calls it.
__device__ __forceinline__ void block_grad_matern_store(double lf, double qq, double badp, double badi, const double (&g)[4],
                                                 double* rec, int64_t block) {
    __shared__ double sh[kGradThreads / 64][kGradRec];
    lf = wave_sum(lf);
    qq = wave_sum(qq);
    double gs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) gs[k] = wave_sum(g[k]);
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
        for (int k = 0; k < 4; ++k) sh[w][4 + k] = gs[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0, c = INFINITY, d = INFINITY, e[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < kGradThreads / 64; ++k) {
            a += sh[k][0];
            b += sh[k][1];
            c = fmin(c, sh[k][2]);
            d = fmin(d, sh[k][3]);
            for (int j = 0; j < 4; ++j) e[j] += sh[k][4 + j];
        }
        double* o = rec + kGradRec * block;
        o[0] = a;
        o[1] = b;
        o[2] = c;
        o[3] = d;
        o[4] = e[0];
        o[5] = e[1];
        o[6] = e[2];
        o[7] = e[3];
    }
}

template <int M, int P>
__global__ __launch_bounds__(kGradThreads) void bf_grad_matern(const double* __restrict__ coords, int64_t n_points,
                                                        const int32_t* __restrict__ nbr,
                                                        const int32_t* __restrict__ order, int64_t n_rows, int64_t i0,
                                                        const CovParams Pc, const GradParams Gp,
                                                               const double* __restrict__ mtab,  // rho | (h, n)
                                                        const double* __restrict__ values, double* __restrict__ Gout,
                                                        double* __restrict__ rec, int dim) {
    static_assert(M >= 1 && M <= 32, "the validity mask holds one bit per neighbour slot");
    constexpr int NR = M + 1;            // joint rows 0..M (row M = the location)
    constexpr int S = (NR + P - 1) / P;  // local rows per lane
    constexpr int DA = 3;
    // the rho table in dynamic LDS (bf_group's grp_mtab); the derivative table stays in global memory
    extern __shared__ double4 gm_rtab[];
    {
        const int n4 = Pc.mt_noct * (NNGP_MT_K * NNGP_MT_NC / 4);
        const double4* g = (const double4*)mtab;
        for (int k = (int)threadIdx.x; k < n4; k += blockDim.x) gm_rtab[k] = g[k];
        __syncthreads();
    }
    const double* __restrict__ dtab = mtab + (size_t)Pc.mt_noct * (NNGP_MT_K * NNGP_MT_NC);
    auto cov = [&](double d2) -> double { return Pc.sigma2 * nngp_matern_tab(Pc, (const double*)gm_rtab, d2); };
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
                R[s][b] = cov(point_d2<DA>(o[s], xb));
            } else if (b < P * s + P - 1) {  // diagonal block: lane-dependent
                // (the self entry's value is not used; d2 = 1 keeps it off the below-table branch, as in bf_group)
                const double c = cov(b == a ? 1.0 : point_d2<DA>(o[s], xb));
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

    // ---- second pass over the own strict-lower pairs (a > b): the phi sums and the nu sums, sharing the products
    double dfp = 0.0, drp = 0.0, dfn = 0.0, drn = 0.0;
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
            double hv, nv;
            nngp_matern_tab_d(Pc, dtab, a == b ? 1.0 : point_d2<DA>(o[s], xb), &hv, &nv);
            const bool ok = a > b && rowok[s] && colok;
            const double Dh = ok ? hv : 0.0;  // u rho'(u): d C / d phi = sigma2 Dh / phi
            const double Dn = ok ? nv : 0.0;  // d rho / d nu: d C / d nu = sigma2 Dn
            const double wf = uo[s] * ub;
            const double wr = fma(ao[s], ub, alb * uo[s]);
            dfp = fma(Dh, wf, dfp);
            drp = fma(Dh, wr, drp);
            dfn = fma(Dn, wf, dfn);
            drn = fma(Dn, wr, drn);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    const double nb2 = gsum<P>(nbp);
    const double adb = gsum<P>(abp);
    const double sphi = Pc.sigma2 / Pc.phi;
    const double dFphi = 2.0 * sphi * gsum<P>(dfp);
    const double drphi = -sphi * gsum<P>(drp);
    const double dFnu = 2.0 * Pc.sigma2 * gsum<P>(dfn);
    const double drnu = -Pc.sigma2 * gsum<P>(drn);

    const double iF = 1.0 / F;
    const double w = 1.0 - res * res * iF;  // 1 - r^2 / F
    const double dFt = 1.0 + nb2;
    const double dFs = (F - Gp.tau2 * dFt) * Gp.isig2;
    const double drs = -Gp.tau2 * adb * Gp.isig2;
    double g[4];
    g[0] = -0.5 * iF * fma(dFs, w, 2.0 * res * drs);
    g[1] = -0.5 * iF * fma(dFphi, w, 2.0 * res * drphi);
    g[2] = -0.5 * iF * fma(dFt, w, 2.0 * res * adb);
    g[3] = -0.5 * iF * fma(dFnu, w, 2.0 * res * drnu);

    const bool lead = live && q == 0;
    if (Gout != nullptr && lead) {
#pragma unroll
        for (int k = 0; k < 4; ++k) Gout[rr * 4 + k] = bad ? NAN : g[k];
    }
    double lf = 0.0, qq = 0.0, badp = INFINITY, badi = INFINITY;
    if (lead) {
        lf = log(F);
        qq = res * res * iF;
        if (bad) badp = (double)i;
    } else {
        g[0] = g[1] = g[2] = g[3] = 0.0;
    }
    if (live && bad_index) badi = (double)i;
    block_grad_matern_store(lf, qq, badp, badi, g, rec, blk);
}

template <int M>
static bool launch_grad_matern_if(const GradMaternArgs& a, hipStream_t s) {
    if (a.m != M) return false;
    constexpr int P = grad_lanes(M);
    const GradParams Gp = grad_params(NNGP_KIND_EXPONENTIAL, a.sigma2, a.tau2);  // tau2 and 1 / sigma2; g unused
    hipLaunchKernelGGL((bf_grad_matern<M, P>), dim3((unsigned)bf_grad_blocks(a.n_rows, M)), dim3(kGradThreads),
                       NNGP_MT_BYTES(a.Pc.mt_noct), s, a.coords, a.n_points, a.nbr, a.order, a.n_rows, a.i0, a.Pc, Gp,
                       a.tab, a.values, a.G, a.rec, a.dim);
    return true;
}

// the instantiation units (bf_grad_matern_m*.hip) and the dispatch + fold (bf_grad_matern.hip)
bool bf_grad_matern_launch_a(const GradMaternArgs& a, hipStream_t s);
bool bf_grad_matern_launch_b(const GradMaternArgs& a, hipStream_t s);
bool bf_grad_matern_launch_c(const GradMaternArgs& a, hipStream_t s);
bool bf_grad_matern_launch_d(const GradMaternArgs& a, hipStream_t s);
bool bf_grad_matern_launch_e(const GradMaternArgs& a, hipStream_t s);
bool bf_grad_matern_launch_f(const GradMaternArgs& a, hipStream_t s);
bool bf_grad_matern_launch_g(const GradMaternArgs& a, hipStream_t s);
bool bf_grad_matern_launch_h(const GradMaternArgs& a, hipStream_t s);
hipError_t bf_grad_matern_launch(GradMaternArgs a, double* partials, double* grad, hipStream_t s);

}  // namespace nngp
