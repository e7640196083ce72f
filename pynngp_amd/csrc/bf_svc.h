// Spatially varying coefficients: y(s) = x(s)^T beta + sum_k z_k(s) w_k(s) + eps(s), w_k independent GPs, so
//   C(a, b) = sum_{k < r} z_ak z_bk sigma2_k rho(phi_k d_ab) + tau2 delta_ab,   1 <= r <= 4.
//
// The covariance depends on the per-point covariates z (n_points, r), so it is no function of the two coordinate
// rows alone.  One kernel on bf_grad.h's layout, as bf_noise.h and bf_sep.h are (P = grad_lanes(m) lanes per
// location, rows dealt cyclically, right-looking elimination with the value column carried along, the same masks,
// flags and block records), instantiated twice per m.  The kind (0..4, one for every component), the dimension
// (1..3) and the number of components r are run-time arguments: the component loop is unrolled to four with a
// wave-uniform test per component and per column of the block, so a launch with r components evaluates r
// correlations per pair and no more.
//
//   * a point's r covariates are gathered with its coordinates into the owning lane's registers (resolved
//     addresses, as bf_noise gathers its weight); a slot without a point has z = 0, so its row and column are
//     exactly 0 off the diagonal whatever the far point's distance, and a positive diagonal entry;
//   * a column's broadcast carries the coordinates and the z of the components in use;
//   * per strict-lower pair one squared distance serves every component: r evaluations of
//     nngp_cov_d2<NNGP_KIND_GENERIC> at sigma2 = 1 from one LDS table 2^(j/256), combined as
//     sum_k (z_ak z_bk sigma2_k) rho_k in the order k = 0, 1, ..;
//   * the diagonal is sum_k z_ak^2 sigma2_k + tau2 (the target's tau2 is left out by the cross form without
//     target noise: kriging of the noiseless surface, and with z_query = e_k of the coefficient w_k itself);
//   * coincident points sit at the distance floor, where rho = 1 exactly, whatever their z.
//
//   GRAD = false  the forward sweep (nngp_bf_sweep_svc, nngp_bf_cross_svc): B, F, R and bf_group's 4-double block
//                 records;
//   GRAD = true   the gradient sweep (nngp_bf_grad_svc) in (sigma2_1..r, phi_1..r, tau2): bf_grad's second
//                 back-substitution and second pass.  In bf_grad.h's notation, with dv(u) = u rho'(u):
//                   sigma2_k: dC_ab = z_ak z_bk rho_k(u_k), the diagonal z_ak^2 included
//                   phi_k:    dC_ab = z_ak z_bk sigma2_k dv(u_k) / phi_k; exactly 0 on the diagonal, at the
//                             distance floor and for masked pairs
//                   tau2:     dC = I
//                 Two pairs of accumulators per component take the strict-lower terms (sigma2_k / phi_k is applied
//                 once after the group sums); the diagonal terms of sigma2_k are two own-row sums per component.
//                 Every sigma2_k is accumulated, none derived from the homogeneity of C: sigma2_k = 0 is a legal
//                 argument, and a derived component would divide by it.
#pragma once
#include "bf_sep.h"  // bf_grad.h's layout helpers and sep_rho_dv

namespace nngp {

constexpr int kSvcMaxComp = 4;
static __device__ double kSvcZero[1] = {0.0};

struct SvcArgs {
    const double* coords;  // (n_points, dim)
    int64_t n_points;
    const double* Z;       // (n_points, r) covariates of the points
    const int32_t* nbr;    // (n_rows, m), -1 padded
    const int32_t* order;  // or null
    int64_t n_rows, i0;
    int m, kind, dim, r;
    const double* sigma2;  // host (r,)
    const double* phi;     // host (r,)
    double tau2;
    int target_noise;       // tau2 on the location's own diagonal entry (always for S = T)
    const double* values;   // (n_points,); null allowed for the forward sweep
    const double* qcoords;  // the locations themselves: coords (S = T) or the query points (cross)
    const double* qZ;       // their covariates: Z (S = T) or (n_query, r)
    const double* qvalues;  // values (S = T), query values or null
    double* B;              // forward: (n_rows, m) or null
    double* F;              // forward: (n_rows,) or null
    double* R;              // forward: (n_rows,) or null
    double* G;              // gradient: (n_rows, 2 r + 1) or null
    double* rec;            // 4 (forward) or kSvcRec (gradient) doubles per block
};

struct SvcCov {
    CovParams pc[kSvcMaxComp];  // sigma2 = 1, phi_k; the components past r repeat the first
};

struct SvcParams {
    double g[3];                 // rho'(u) = e(u) (g[0] + g[1] u + g[2] u^2) of the kind
    double sigma2[kSvcMaxComp];  // 0 past r
    double sip[kSvcMaxComp];     // sigma2_k / phi_k
    double tau2;
    double tself;                // tau2, or 0 for a target without noise
    double dfar;                 // the diagonal entry of a slot without a point: positive, otherwise free
    int nc;                      // r
};

inline void svc_params(const SvcArgs& a, SvcCov& C, SvcParams& Sp) {
    const GradParams gp = grad_params(a.kind, 1.0, a.tau2);
    for (int k = 0; k < 3; ++k) Sp.g[k] = gp.g[k];
    double tot = a.tau2;
    for (int k = 0; k < kSvcMaxComp; ++k) {
        const bool in = k < a.r;
        C.pc[k] = nngp_cov_params(a.kind, 1.0, a.phi[in ? k : 0], 0.0);
        Sp.sigma2[k] = in ? a.sigma2[k] : 0.0;
        Sp.sip[k] = in ? a.sigma2[k] / a.phi[k] : 0.0;
        tot += Sp.sigma2[k];
    }
    Sp.tau2 = a.tau2;
    Sp.tself = a.target_noise ? a.tau2 : 0.0;
    Sp.dfar = tot > 0.0 ? tot : 1.0;
    Sp.nc = a.r;
}

// per-block record of the gradient sweep: sum log F, sum r^2/F, first bad-pivot row, first bad-index row, then nine
// gradient sums in fixed slots: sigma2_0..3, phi_0..3, tau2 (the slots past r hold 0)
constexpr int kSvcSums = 2 * kSvcMaxComp + 1;
constexpr int kSvcRec = 4 + kSvcSums;

// block_sep_store with nine gradient sums.  Every thread of the block calls it.
__device__ __forceinline__ void block_svc_store(double lf, double qq, double badp, double badi,
                                                const double (&g)[kSvcSums], double* rec, int64_t block) {
    __shared__ double sh[kGradThreads / 64][kSvcRec];
    lf = wave_sum(lf);
    qq = wave_sum(qq);
    double gs[kSvcSums];
#pragma unroll
    for (int k = 0; k < kSvcSums; ++k) gs[k] = wave_sum(g[k]);
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
        for (int k = 0; k < kSvcSums; ++k) sh[w][4 + k] = gs[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0, c = INFINITY, d = INFINITY, e[kSvcSums];
        for (int j = 0; j < kSvcSums; ++j) e[j] = 0.0;
        for (int k = 0; k < kGradThreads / 64; ++k) {
            a += sh[k][0];
            b += sh[k][1];
            c = fmin(c, sh[k][2]);
            d = fmin(d, sh[k][3]);
            for (int j = 0; j < kSvcSums; ++j) e[j] += sh[k][4 + j];
        }
        double* o = rec + kSvcRec * block;
        o[0] = a;
        o[1] = b;
        o[2] = c;
        o[3] = d;
        for (int j = 0; j < kSvcSums; ++j) o[4 + j] = e[j];
    }
}

template <int M, int P, bool GRAD>
__global__ __launch_bounds__(kGradThreads) void bf_svc(const double* __restrict__ coords, int64_t n_points,
                                                       const double* __restrict__ Zp,
                                                       const int32_t* __restrict__ nbr,
                                                       const int32_t* __restrict__ order, int64_t n_rows, int64_t i0,
                                                       const SvcCov Cv, const SvcParams Sp,
                                                       const double* __restrict__ values,
                                                       const double* __restrict__ qcoords,
                                                       const double* __restrict__ qZ,
                                                       const double* __restrict__ qvalues, double* __restrict__ Bout,
                                                       double* __restrict__ Fout, double* __restrict__ Rout,
                                                       double* __restrict__ Gout, double* __restrict__ rec, int dim) {
    static_assert(M >= 1 && M <= 32, "the validity mask holds one bit per neighbour slot");
    constexpr int NR = M + 1;            // joint rows 0..M (row M = the location)
    constexpr int S = (NR + P - 1) / P;  // local rows per lane
    constexpr int DA = 3;
    constexpr int NC = kSvcMaxComp;
    __shared__ double etab[NNGP_EXP_TAB_N];
    nngp_exp_table_load(etab, 1.0);
    const int nc = Sp.nc;  // wave-uniform
    const int64_t blk = xcd_logical_block(blockIdx.x, gridDim.x);
    const int64_t tid = blk * blockDim.x + threadIdx.x;
    const int q = (int)(threadIdx.x % P);
    const int64_t r = tid / P;
    const bool live = r < n_rows;
    const int64_t rl = live ? r : n_rows - 1;
    const int64_t rr = order != nullptr ? (int64_t)order[rl] : rl;
    const int64_t i = i0 + rr;

    // ---- own rows a = P*s + q: neighbour slot (a < M), the location (a == M), padding (a > M); the covariates are
    // gathered with the point (branch-free: resolved addresses, as bf_noise's weight), 0 in a slot without a point
    int32_t jn[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int a = P * s + q;
        jn[s] = nbr[rl * M + (a < M ? a : M - 1)];
    }
    double o[S][DA], zz[S][NC], z[S], dg[S];
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
        const double* pz = self ? qZ + i * nc : Zp + (in_range ? (int64_t)j : 0) * nc;
        load_point_rt(pc, dim, o[s]);
        z[s] = *pv;
        double d = self ? Sp.tself : Sp.tau2;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            zz[s][k] = *((k < nc && (self || in_range)) ? pz + k : kSvcZero);
            d = fma(zz[s][k] * zz[s][k], Sp.sigma2[k], d);
        }
        dg[s] = (self || in_range) ? d : Sp.dfar;
    }
    if constexpr (GRAD) {
        if constexpr (P > 1) vm |= (uint32_t)__builtin_amdgcn_mov_dpp((int)vm, 0xB1, 0xf, 0xf, true);
        if constexpr (P > 2) vm |= (uint32_t)__builtin_amdgcn_mov_dpp((int)vm, 0x4E, 0xf, 0xf, true);
        if constexpr (P > 4) vm |= (uint32_t)__shfl_xor((int)vm, 4);
        if constexpr (P > 8) vm |= (uint32_t)__shfl_xor((int)vm, 8);
        if constexpr (P > 16) vm |= (uint32_t)__shfl_xor((int)vm, 16);
        if constexpr (P > 32) vm |= (uint32_t)__shfl_xor((int)vm, 32);
    }

    // ---- joint block rows: R[s][b], b < min(P*s + P, NR); column by column, so one broadcast point is live.  Per
    // column: the squared distances of the own rows once, then one pass per component in use
    double R[S][NR];
#pragma unroll
    for (int b = 0; b < NR; ++b) {
        double xb[DA], d2[S];
#pragma unroll
        for (int k = 0; k < DA; ++k) xb[k] = gbcast<P>(o[b / P][k], b % P);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (b >= P * s + P - 1) continue;  // no strict-lower entry of this local row in column b
            d2[s] = point_d2<DA>(o[s], xb);
            R[s][b] = 0.0;
        }
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            if (k < nc) {
                const double zb = gbcast<P>(zz[b / P][k], b % P) * Sp.sigma2[k];
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    if (b >= P * s + P - 1) continue;
                    R[s][b] = fma(zz[s][k] * zb, nngp_cov_d2<NNGP_KIND_GENERIC>(Cv.pc[k], etab, d2[s]), R[s][b]);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int a = P * s + q;
            if (b >= P * s + P) continue;  // beyond this local row's width
            if (b < P * s) {
            } else if (b < P * s + P - 1) {  // diagonal block: lane-dependent
                R[s][b] = b < a ? R[s][b] : (b == a ? dg[s] : 0.0);
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
        // ---- u = [-b; 1], alpha = [a; 0], exactly 0 in slots without a point; |b|^2, a.b and the diagonal terms of
        // every sigma2_k: sum_a z_ak^2 u_a^2 and sum_a z_ak^2 alpha_a u_a over the own rows
        double uo[S], ao[S];
        bool rowok[S];
        double nbp = 0.0, abp = 0.0, dfd[NC], drd[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) dfd[k] = drd[k] = 0.0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int a = P * s + q;
            const bool nb = a < M && oval[s];
            rowok[s] = nb || a == M;
            uo[s] = nb ? -bown[s] : (a == M ? 1.0 : 0.0);
            ao[s] = nb ? aown[s] : 0.0;
            nbp = nb ? fma(bown[s], bown[s], nbp) : nbp;
            abp = nb ? fma(aown[s], bown[s], abp) : abp;
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const double z2 = zz[s][k] * zz[s][k];  // 0 past r and in slots without a point
                dfd[k] = fma(z2 * uo[s], uo[s], dfd[k]);
                drd[k] = fma(z2 * ao[s], uo[s], drd[k]);
            }
        }

        // ---- second pass over the own strict-lower pairs (a > b): per component the sigma2 sums (weights rho) and
        // the phi sums (weights dv), at sigma2 = 1
        double dfs[NC], drs[NC], dfp[NC], drp[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) dfs[k] = drs[k] = dfp[k] = drp[k] = 0.0;
        // (the coordinates pass through an opaque barrier, as in bf_grad)
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int k = 0; k < DA; ++k) asm volatile("" : "+v"(o[s][k]));
#pragma unroll
        for (int b = 0; b < M; ++b) {
            double xb[DA], d2[S], wf[S], wr[S];
#pragma unroll
            for (int k = 0; k < DA; ++k) xb[k] = gbcast<P>(o[b / P][k], b % P);
            const double ub = gbcast<P>(uo[b / P], b % P);
            const double alb = gbcast<P>(ao[b / P], b % P);
            const bool colok = (vm >> (b & 31)) & 1u;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (P * s + P - 1 <= b) continue;  // every row of this local row is <= b
                const int a = P * s + q;
                const bool ok = a > b && rowok[s] && colok;
                d2[s] = point_d2<DA>(o[s], xb);
                wf[s] = ok ? uo[s] * ub : 0.0;
                wr[s] = ok ? fma(ao[s], ub, alb * uo[s]) : 0.0;
            }
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                if (k < nc) {
                    const double zb = gbcast<P>(zz[b / P][k], b % P);
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        if (P * s + P - 1 <= b) continue;
                        double rho, dv;
                        sep_rho_dv(Cv.pc[k], Sp.g, etab, d2[s], rho, dv);
                        const double w = zz[s][k] * zb;
                        const double Ds = w * rho, Dp = w * dv;
                        dfs[k] = fma(Ds, wf[s], dfs[k]);
                        drs[k] = fma(Ds, wr[s], drs[k]);
                        dfp[k] = fma(Dp, wf[s], dfp[k]);
                        drp[k] = fma(Dp, wr[s], drp[k]);
                    }
                }
            }
            // (the sums pass through an opaque barrier per column, as bf_grad_aniso's: it keeps the compiler from
            // sinking every column's accumulation below the last column)
#pragma unroll
            for (int k = 0; k < NC; ++k) asm volatile("" : "+v"(dfs[k]), "+v"(drs[k]), "+v"(dfp[k]), "+v"(drp[k]));
            __builtin_amdgcn_sched_barrier(0);
        }
        const double nb2 = gsum<P>(nbp);
        const double adb = gsum<P>(abp);
        const double w = 1.0 - res * res * iF;  // 1 - r^2 / F
        double g[kSvcSums];
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            g[k] = g[NC + k] = 0.0;
            if (k < nc) {
                const double dFs = fma(2.0, gsum<P>(dfs[k]), gsum<P>(dfd[k]));
                const double drsg = -(gsum<P>(drs[k]) + gsum<P>(drd[k]));
                const double dFp = 2.0 * gsum<P>(dfp[k]) * Sp.sip[k];
                const double drph = -gsum<P>(drp[k]) * Sp.sip[k];
                g[k] = -0.5 * iF * fma(dFs, w, 2.0 * res * drsg);
                g[NC + k] = -0.5 * iF * fma(dFp, w, 2.0 * res * drph);
            }
        }
        g[2 * NC] = -0.5 * iF * fma(1.0 + nb2, w, 2.0 * res * adb);
        if (Gout != nullptr && lead) {
            double* go = Gout + rr * (2 * nc + 1);
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                if (k < nc) {
                    go[k] = bad ? NAN : g[k];
                    go[nc + k] = bad ? NAN : g[NC + k];
                }
            }
            go[2 * nc] = bad ? NAN : g[2 * NC];
        }
        if (!lead) {
#pragma unroll
            for (int k = 0; k < kSvcSums; ++k) g[k] = 0.0;
        }
        block_svc_store(lf, qq, badp, badi, g, rec, blk);
    }
}

template <int M>
static bool launch_svc_if(const SvcArgs& a, bool grad, hipStream_t s) {
    if (a.m != M) return false;
    constexpr int P = grad_lanes(M);
    SvcCov Cv;
    SvcParams Sp;
    svc_params(a, Cv, Sp);
    const dim3 grid((unsigned)bf_grad_blocks(a.n_rows, M)), block(kGradThreads);
    if (grad)
        hipLaunchKernelGGL((bf_svc<M, P, true>), grid, block, 0, s, a.coords, a.n_points, a.Z, a.nbr, a.order, a.n_rows,
                           a.i0, Cv, Sp, a.values, a.qcoords, a.qZ, a.qvalues, a.B, a.F, a.R, a.G, a.rec, a.dim);
    else
        hipLaunchKernelGGL((bf_svc<M, P, false>), grid, block, 0, s, a.coords, a.n_points, a.Z, a.nbr, a.order, a.n_rows,
                           a.i0, Cv, Sp, a.values, a.qcoords, a.qZ, a.qvalues, a.B, a.F, a.R, a.G, a.rec, a.dim);
    return true;
}

// the instantiation units (bf_svc_m*.hip) and the dispatch + folds (bf_svc.hip)
bool bf_svc_launch_a(const SvcArgs& a, bool grad, hipStream_t s);
bool bf_svc_launch_b(const SvcArgs& a, bool grad, hipStream_t s);
bool bf_svc_launch_c(const SvcArgs& a, bool grad, hipStream_t s);
bool bf_svc_launch_d(const SvcArgs& a, bool grad, hipStream_t s);
bool bf_svc_launch_e(const SvcArgs& a, bool grad, hipStream_t s);
bool bf_svc_launch_f(const SvcArgs& a, bool grad, hipStream_t s);
bool bf_svc_launch_g(const SvcArgs& a, bool grad, hipStream_t s);
bool bf_svc_launch_h(const SvcArgs& a, bool grad, hipStream_t s);
// forward (grad == nullptr: partials[4] by bf_finalize's fold) or gradient (partials[4], grad[2 r + 1] by
// bf_svc_finalize)
hipError_t bf_svc_launch(const SvcArgs& a, double* partials, double* grad, hipStream_t s);

}  // namespace nngp
