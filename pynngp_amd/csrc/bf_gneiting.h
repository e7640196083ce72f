// Nonseparable space-time covariance of Gneiting's (2002) class.  With h = |a_s - b_s|, u = |a_t - b_t| and
// psi = 1 + (a u)^2:
//
//     C(a, b) = sigma2 rho(v) / psi + tau2 delta_ab,      v = c h psi^(-beta/2),      0 <= beta <= 1,
//
// rho the spatial kind (exponential, Matern-3/2, Matern-5/2, gaussian).  beta = 0 is separable (rho(c h) times a
// Cauchy factor in time), beta = 1 fully nonseparable.  The points are (n, dim) with dim = 2 or 3: the last column
// is time, the first dim - 1 columns are space (bf_sep.h's convention and its point form, load_point_sep).
//
// One kernel on bf_grad.h's layout, as bf_sep.h is (P = grad_lanes(m) lanes per location, rows dealt cyclically,
// right-looking elimination with the value column carried along, the same masks, flags and block records),
// instantiated twice per m; the kind and the dimension are run-time arguments:
//
//   GRAD = false  the forward sweep (nngp_bf_sweep_gneiting, nngp_bf_cross_gneiting): B, F, R and bf_group's
//                 4-double block records; the location's coordinates and value come from the q* arrays;
//   GRAD = true   the gradient sweep (nngp_bf_grad_gneiting) in (sigma2, c, a, beta, tau2): bf_grad's second
//                 back-substitution and second pass.  With dv(v) = v rho'(v) (bf_grad.h's e(v) (g0 + g1 v + g2 v^2)
//                 times v) and L = ln psi:
//                   c:     dC_ab = sigma2 dv / (psi c)
//                   a:     dC_ab = -2 sigma2 (psi - 1) / (a psi^2) (rho + (beta / 2) dv)
//                   beta:  dC_ab = -sigma2 dv L / (2 psi)
//                   sigma2, tau2: as bf_grad (the diagonal is sigma2 + tau2 everywhere).
//                 Three pairs of accumulators take the per-pair terms without their scalar factors; sigma2 / c,
//                 -2 sigma2 / a and -sigma2 / 2 are applied once after the group sums.  The c term is exactly 0
//                 where the squared spatial distance is the floor, the a and beta terms where the time lag is 0
//                 (psi = 1 and L = 0 exactly there, gneiting_math.h), and all three where the pair is masked.
//
// Every pair costs the two squared distances, the time-lag routine (nngp_gn_psi: 1 / psi, L, s2 = psi^-beta; the
// 2^(j/256) table and a 3 KB logarithm table in LDS) and ONE run-time-kind covariance evaluation at the scaled
// squared distance h^2 s2 (nngp_cov_d2<NNGP_KIND_GENERIC> at sigma2 = 1; d2max / umax keep their meaning, and the
// gaussian kind works unchanged since the evaluation takes a squared distance).  The scaled distance is floored
// again at NNGP_D2_FLOOR (s2 <= 1 can take it below, where nngp_sqrt is not defined).  A slot without a point sits
// at a far spatial coordinate (far_point, k 1e150): s2 >= 2^-400 (x is clamped), so the scaled squared distance is
// still past d2max and rho, with it the covariance, is exactly 0 for any time lag.
#pragma once
#include "bf_sep.h"
#include "gneiting_math.h"

namespace nngp {

struct GneitingArgs {
    const double* coords;  // (n_points, dim): space in the first dim - 1 columns, time in the last
    int64_t n_points;
    const int32_t* nbr;    // (n_rows, m), -1 padded
    const int32_t* order;  // or null
    int64_t n_rows, i0;
    int m, kind, dim;
    double sigma2, c, a, beta, tau2;
    const double* values;   // (n_points,); null allowed for the forward sweep
    const double* qcoords;  // the locations themselves: coords (S = T) or the query points (cross)
    const double* qvalues;  // values (S = T), query values or null
    double* B;              // forward: (n_rows, m) or null
    double* F;              // forward: (n_rows,) or null
    double* R;              // forward: (n_rows,) or null
    double* G;              // gradient: (n_rows, 5) or null
    double* rec;            // 4 (forward) or kGnRec (gradient) doubles per block
};

struct GneitingParams {
    double g[3];  // rho'(v) = e(v) (g[0] + g[1] v + g[2] v^2) of the spatial kind
    double sigma2, diag, tau2, isig2;
    double a2, hbeta;        // a^2, beta / 2
    double sic, sia, sib;    // sigma2 / c, -2 sigma2 / a, -sigma2 / 2
};

inline GneitingParams gneiting_params(int kind, double sigma2, double c, double a, double beta, double tau2) {
    const GradParams gp = grad_params(kind, sigma2, tau2);
    GneitingParams p;
    for (int k = 0; k < 3; ++k) p.g[k] = gp.g[k];
    p.sigma2 = sigma2;
    p.diag = sigma2 + tau2;
    p.tau2 = tau2;
    p.isig2 = 1.0 / sigma2;
    p.a2 = a * a;
    p.hbeta = 0.5 * beta;
    p.sic = sigma2 / c;
    p.sia = -2.0 * sigma2 / a;
    p.sib = -0.5 * sigma2;
    return p;
}

// per-block record of the gradient sweep: sum log F, sum r^2/F, first bad-pivot row, first bad-index row, the
// five gradient sums (sigma2, c, a, beta, tau2)
constexpr int kGnSums = 5;
constexpr int kGnRec = 4 + kGnSums;

// block_grad_store with five gradient sums.  Every thread of the block calls it.
__device__ __forceinline__ void block_gn_store(double lf, double qq, double badp, double badi,
                                               const double (&g)[kGnSums], double* rec, int64_t block) {
    __shared__ double sh[kGradThreads / 64][kGnRec];
    lf = wave_sum(lf);
    qq = wave_sum(qq);
    double gs[kGnSums];
#pragma unroll
    for (int k = 0; k < kGnSums; ++k) gs[k] = wave_sum(g[k]);
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
        for (int k = 0; k < kGnSums; ++k) sh[w][4 + k] = gs[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0, c = INFINITY, d = INFINITY, e[kGnSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < kGradThreads / 64; ++k) {
            a += sh[k][0];
            b += sh[k][1];
            c = fmin(c, sh[k][2]);
            d = fmin(d, sh[k][3]);
            for (int j = 0; j < kGnSums; ++j) e[j] += sh[k][4 + j];
        }
        double* o = rec + kGnRec * block;
        o[0] = a;
        o[1] = b;
        o[2] = c;
        o[3] = d;
        for (int j = 0; j < kGnSums; ++j) o[4 + j] = e[j];
    }
}

// the squared spatial distance (floored as sep_d2's) and x = (a u)^2, exactly 0 at a zero time lag
__device__ __forceinline__ void gn_d2(const GneitingParams& Gp, const double (&a)[3], const double (&b)[3], double& ds2,
                                      double& x) {
    const double t = a[2] - b[2], y = a[1] - b[1], xs = a[0] - b[0];
    x = Gp.a2 * (t * t);
    ds2 = fma(xs, xs, fma(y, y, NNGP_D2_FLOOR));
}

// rho(v) / psi: the time-lag routine and one run-time-kind evaluation at sigma2 = 1
__device__ __forceinline__ double gn_rho(const CovParams& Pc, const CovParams& Pb, const GneitingParams& Gp,
                                         const double* etab, const double* ltab, const double (&a)[3],
                                         const double (&b)[3]) {
    double ds2, x;
    gn_d2(Gp, a, b, ds2, x);
    const NngpGnPsi ps = nngp_gn_psi(Pb, etab, ltab, x);
    return ps.ipsi * nngp_cov_d2<NNGP_KIND_GENERIC>(Pc, etab, fmax(ds2 * ps.s2, NNGP_D2_FLOOR));
}

template <int M, int P, bool GRAD>
__global__ __launch_bounds__(kGradThreads) void bf_gneiting(
    const double* __restrict__ coords, int64_t n_points, const int32_t* __restrict__ nbr,
    const int32_t* __restrict__ order, int64_t n_rows, int64_t i0, const CovParams Pc, const CovParams Pb,
    const GneitingParams Gp, const double* __restrict__ values, const double* __restrict__ qcoords,
    const double* __restrict__ qvalues, double* __restrict__ Bout, double* __restrict__ Fout,
    double* __restrict__ Rout, double* __restrict__ Gout, double* __restrict__ rec, int dim) {
    static_assert(M >= 1 && M <= 32, "the validity mask holds one bit per neighbour slot");
    constexpr int NR = M + 1;            // joint rows 0..M (row M = the location)
    constexpr int S = (NR + P - 1) / P;  // local rows per lane
    constexpr int DA = 3;
    __shared__ double etab[NNGP_EXP_TAB_N];
    __shared__ double ltab[3 * NNGP_GN_TAB_N];
    nngp_gn_table_load(ltab);
    nngp_exp_table_load(etab, 1.0);  // (its barrier serves both tables)
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
        const double* pc = self ? qcoords + i * dim : (in_range ? coords + (int64_t)j * dim : far_point<DA>(a));
        const double* pv = self ? (qvalues != nullptr ? qvalues + i : kZeroValue)
                                : ((values != nullptr && in_range) ? values + j : kZeroValue);
        load_point_sep(pc, dim, o[s]);
        z[s] = *pv;
    }
    if constexpr (GRAD) {
        if constexpr (P > 1) vm |= (uint32_t)__builtin_amdgcn_mov_dpp((int)vm, 0xB1, 0xf, 0xf, true);
        if constexpr (P > 2) vm |= (uint32_t)__builtin_amdgcn_mov_dpp((int)vm, 0x4E, 0xf, 0xf, true);
        if constexpr (P > 4) vm |= (uint32_t)__shfl_xor((int)vm, 4);
        if constexpr (P > 8) vm |= (uint32_t)__shfl_xor((int)vm, 8);
        if constexpr (P > 16) vm |= (uint32_t)__shfl_xor((int)vm, 16);
        if constexpr (P > 32) vm |= (uint32_t)__shfl_xor((int)vm, 32);
    }

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
                R[s][b] = Gp.sigma2 * gn_rho(Pc, Pb, Gp, etab, ltab, o[s], xb);
            } else if (b < P * s + P - 1) {  // diagonal block: lane-dependent
                const double c = Gp.sigma2 * gn_rho(Pc, Pb, Gp, etab, ltab, o[s], xb);
                R[s][b] = b < a ? c : (b == a ? Gp.diag : 0.0);
            } else {
                R[s][b] = b == a ? Gp.diag : 0.0;
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

    // ---- b = L_N^-T v (v = row M of L) and, for the gradient, a = L_N^-T z_N with it; lane q ends with b, a of
    // its own rows
    double bown[S], aown[S];
#pragma unroll
    for (int s = 0; s < S; ++s) bown[s] = aown[s] = 0.0;
    if (GRAD || Bout != nullptr) {
#pragma unroll
        for (int a = M - 1; a >= 0; --a) {
            double pb = 0.0, pa = 0.0;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (P * s + P - 1 <= a) continue;  // every row of this local row is <= a
                const int ar = P * s + q;
                const bool in = ar > a && ar < M;
                pb = in ? fma(R[s][a], bown[s], pb) : pb;
                if constexpr (GRAD) pa = in ? fma(R[s][a], aown[s], pa) : pa;
            }
            const double tb = gsum<P>(pb);
            const double va = gbcast<P>(R[M / P][a], M % P);
            const double iva = gbcast<P>(R[a / P][a], a % P);
            const double ba = (va - tb) * iva;
            bown[a / P] = q == a % P ? ba : bown[a / P];
            if constexpr (GRAD) {
                const double ta = gsum<P>(pa);
                const double za = gbcast<P>(z[a / P], a % P);
                const double aa = (za - ta) * iva;
                aown[a / P] = q == a % P ? aa : aown[a / P];
            }
        }
    }
    const bool lead = live && q == 0;
    const double iF = 1.0 / F;
    double lf = 0.0, qq = 0.0, badp = INFINITY, badi = INFINITY;
    if (lead) {
        lf = log(F);
        qq = res * res * iF;
        if (bad) badp = (double)i;
    }
    if (live && bad_index) badi = (double)i;

    if constexpr (!GRAD) {
        if (Bout != nullptr && live) {
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const int a = P * s + q;
                if (a < M) Bout[rr * M + a] = bad ? NAN : (oval[s] ? bown[s] : 0.0);
            }
        }
        if (Fout != nullptr && lead) Fout[rr] = bad ? NAN : F;
        if (Rout != nullptr && lead) Rout[rr] = bad ? NAN : res;
        block_partials_store(lf, qq, badp, badi, rec, blk);
    } else {
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

        // ---- second pass over the own strict-lower pairs (a > b): the two sums of c, a and beta, without their
        // scalar factors
        double dfc = 0.0, drc = 0.0, dfa = 0.0, dra = 0.0, dfb = 0.0, drb = 0.0;
        // (the coordinates pass through an opaque barrier, as in bf_grad)
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
                double ds2, x, rho, dv;
                gn_d2(Gp, o[s], xb, ds2, x);
                const NngpGnPsi ps = nngp_gn_psi(Pb, etab, ltab, x);
                sep_rho_dv(Pc, Gp.g, etab, fmax(ds2 * ps.s2, NNGP_D2_FLOOR), rho, dv);
                dv = ds2 > NNGP_D2_FLOOR ? dv : 0.0;  // (sep_rho_dv tests the scaled distance)
                const bool ok = a > b && rowok[s] && colok;
                const double pdv = ps.ipsi * dv;
                const double Dc = ok ? pdv : 0.0;
                const double Da = ok ? fmin(x, NNGP_GN_XMAX) * (ps.ipsi * ps.ipsi) * fma(Gp.hbeta, dv, rho) : 0.0;
                const double Db = ok ? pdv * ps.L : 0.0;
                const double wf = uo[s] * ub;
                const double wr = fma(ao[s], ub, alb * uo[s]);
                dfc = fma(Dc, wf, dfc);
                drc = fma(Dc, wr, drc);
                dfa = fma(Da, wf, dfa);
                dra = fma(Da, wr, dra);
                dfb = fma(Db, wf, dfb);
                drb = fma(Db, wr, drb);
            }
            // (the six sums pass through an opaque barrier per column, as bf_sep's: it keeps the compiler from
            // sinking every column's accumulation below the last column)
            asm volatile("" : "+v"(dfc), "+v"(drc), "+v"(dfa), "+v"(dra), "+v"(dfb), "+v"(drb));
            __builtin_amdgcn_sched_barrier(0);
        }
        const double nb2 = gsum<P>(nbp);
        const double adb = gsum<P>(abp);
        const double dFc = 2.0 * gsum<P>(dfc) * Gp.sic;
        const double drcc = -gsum<P>(drc) * Gp.sic;
        const double dFa = 2.0 * gsum<P>(dfa) * Gp.sia;
        const double draa = -gsum<P>(dra) * Gp.sia;
        const double dFb = 2.0 * gsum<P>(dfb) * Gp.sib;
        const double drbb = -gsum<P>(drb) * Gp.sib;

        const double w = 1.0 - res * res * iF;  // 1 - r^2 / F
        const double dFt = 1.0 + nb2;
        const double dFs = (F - Gp.tau2 * dFt) * Gp.isig2;
        const double drsg = -Gp.tau2 * adb * Gp.isig2;
        double g[kGnSums];
        g[0] = -0.5 * iF * fma(dFs, w, 2.0 * res * drsg);
        g[1] = -0.5 * iF * fma(dFc, w, 2.0 * res * drcc);
        g[2] = -0.5 * iF * fma(dFa, w, 2.0 * res * draa);
        g[3] = -0.5 * iF * fma(dFb, w, 2.0 * res * drbb);
        g[4] = -0.5 * iF * fma(dFt, w, 2.0 * res * adb);
        if (Gout != nullptr && lead) {
#pragma unroll
            for (int k = 0; k < kGnSums; ++k) Gout[rr * kGnSums + k] = bad ? NAN : g[k];
        }
        if (!lead) {
#pragma unroll
            for (int k = 0; k < kGnSums; ++k) g[k] = 0.0;
        }
        block_gn_store(lf, qq, badp, badi, g, rec, blk);
    }
}

template <int M>
static bool launch_gneiting_if(const GneitingArgs& a, bool grad, hipStream_t s) {
    if (a.m != M) return false;
    constexpr int P = grad_lanes(M);
    const CovParams Pc = nngp_cov_params(a.kind, 1.0, a.c, 0.0);
    const CovParams Pb = nngp_gn_beta_params(a.beta);
    const GneitingParams Gp = gneiting_params(a.kind, a.sigma2, a.c, a.a, a.beta, a.tau2);
    const dim3 grid((unsigned)bf_grad_blocks(a.n_rows, M)), block(kGradThreads);
    if (grad)
        hipLaunchKernelGGL((bf_gneiting<M, P, true>), grid, block, 0, s, a.coords, a.n_points, a.nbr, a.order, a.n_rows,
                           a.i0, Pc, Pb, Gp, a.values, a.qcoords, a.qvalues, a.B, a.F, a.R, a.G, a.rec, a.dim);
    else
        hipLaunchKernelGGL((bf_gneiting<M, P, false>), grid, block, 0, s, a.coords, a.n_points, a.nbr, a.order, a.n_rows,
                           a.i0, Pc, Pb, Gp, a.values, a.qcoords, a.qvalues, a.B, a.F, a.R, a.G, a.rec, a.dim);
    return true;
}

// the instantiation units (bf_gneiting_m*.hip) and the dispatch + folds (bf_gneiting.hip)
bool bf_gneiting_launch_a(const GneitingArgs& a, bool grad, hipStream_t s);
bool bf_gneiting_launch_b(const GneitingArgs& a, bool grad, hipStream_t s);
bool bf_gneiting_launch_c(const GneitingArgs& a, bool grad, hipStream_t s);
bool bf_gneiting_launch_d(const GneitingArgs& a, bool grad, hipStream_t s);
bool bf_gneiting_launch_e(const GneitingArgs& a, bool grad, hipStream_t s);
bool bf_gneiting_launch_f(const GneitingArgs& a, bool grad, hipStream_t s);
bool bf_gneiting_launch_g(const GneitingArgs& a, bool grad, hipStream_t s);
bool bf_gneiting_launch_h(const GneitingArgs& a, bool grad, hipStream_t s);
// forward (grad == nullptr: partials[4] by bf_finalize's fold) or gradient (partials[4], grad[5] by
// bf_gneiting_finalize)
hipError_t bf_gneiting_launch(const GneitingArgs& a, double* partials, double* grad, hipStream_t s);

}  // namespace nngp
