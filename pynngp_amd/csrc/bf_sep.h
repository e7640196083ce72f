// Separable space-time covariance: C(a, b) = sigma2 rho_s(phi_s |a_s - b_s|) rho_t(phi_t |a_t - b_t|) + tau2 delta_ab.
//
// The points are (n, dim) with dim = 2 or 3: the last column is time, the first dim - 1 columns are space.  One
// kernel on bf_grad.h's layout, as bf_noise.h is (P = grad_lanes(m) lanes per location, rows dealt cyclically,
// right-looking elimination with the value column carried along, the same masks, flags and block records),
// instantiated twice per m; the two kinds (0..4 each) and the dimension are run-time arguments:
//
//   GRAD = false  the forward sweep (nngp_bf_sweep_sep, nngp_bf_cross_sep): B, F, R and bf_group's 4-double block
//                 records; the location's coordinates and value come from the q* arrays (the cross form);
//   GRAD = true   the gradient sweep (nngp_bf_grad_sep) in (sigma2, phi_s, phi_t, tau2): bf_grad's second
//                 back-substitution and second pass.  With dv(u) = u rho'(u) of each factor (bf_grad.h's
//                 e(u) (g0 + g1 u + g2 u^2) times u), in bf_grad.h's notation:
//                   phi_s:   dC_ab = sigma2 dv_s(u_s) rho_t(u_t) / phi_s
//                   phi_t:   dC_ab = sigma2 rho_s(u_s) dv_t(u_t) / phi_t
//                   sigma2, tau2: as bf_grad (the diagonal is sigma2 + tau2 everywhere).
//                 Two pairs of accumulators take the per-pair terms at sigma2 = 1; sigma2 / phi is applied once
//                 after the group sums.  A factor's derivative is exactly 0 where its squared distance is the
//                 floor (coincident in that factor) and where the pair is masked.
//
// Every pair costs two run-time-kind covariance evaluations (nngp_cov_d2<NNGP_KIND_GENERIC> at sigma2 = 1, one
// LDS table 2^(j/256) for both) from two squared distances, each with its own d2max / umax clamps.  A slot
// without a point sits at a far spatial coordinate (far_point), so rho_s and with it the product is exactly 0.
#pragma once
#include "bf_grad.h"

namespace nngp {

struct SepArgs {
    const double* coords;  // (n_points, dim): space in the first dim - 1 columns, time in the last
    int64_t n_points;
    const int32_t* nbr;    // (n_rows, m), -1 padded
    const int32_t* order;  // or null
    int64_t n_rows, i0;
    int m, kind_s, kind_t, dim;
    double sigma2, phi_s, phi_t, tau2;
    const double* values;   // (n_points,); null allowed for the forward sweep
    const double* qcoords;  // the locations themselves: coords (S = T) or the query points (cross)
    const double* qvalues;  // values (S = T), query values or null
    double* B;              // forward: (n_rows, m) or null
    double* F;              // forward: (n_rows,) or null
    double* R;              // forward: (n_rows,) or null
    double* G;              // gradient: (n_rows, 4) or null
    double* rec;            // 4 (forward) or kSepRec (gradient) doubles per block
};

struct SepParams {
    double gs[3], gt[3];  // rho'(u) = e(u) (g[0] + g[1] u + g[2] u^2) of the spatial / temporal factor
    double sigma2, diag, tau2, isig2;
    double sips, sipt;    // sigma2 / phi_s, sigma2 / phi_t
};

inline SepParams sep_params(int kind_s, int kind_t, double sigma2, double phi_s, double phi_t, double tau2) {
    const GradParams a = grad_params(kind_s, sigma2, tau2), b = grad_params(kind_t, sigma2, tau2);
    SepParams p;
    for (int k = 0; k < 3; ++k) {
        p.gs[k] = a.g[k];
        p.gt[k] = b.g[k];
    }
    p.sigma2 = sigma2;
    p.diag = sigma2 + tau2;
    p.tau2 = tau2;
    p.isig2 = 1.0 / sigma2;
    p.sips = sigma2 / phi_s;
    p.sipt = sigma2 / phi_t;
    return p;
}

// per-block record of the gradient sweep: sum log F, sum r^2/F, first bad-pivot row, first bad-index row, the
// four gradient sums (sigma2, phi_s, phi_t, tau2)
constexpr int kSepRec = 8;
constexpr int kSepSums = 4;

// block_grad_store with four gradient sums.  Every thread of the block calls it.
__device__ __forceinline__ void block_sep_store(double lf, double qq, double badp, double badi,
                                                const double (&g)[kSepSums], double* rec, int64_t block) {
    __shared__ double sh[kGradThreads / 64][kSepRec];
    lf = wave_sum(lf);
    qq = wave_sum(qq);
    double gs[kSepSums];
#pragma unroll
    for (int k = 0; k < kSepSums; ++k) gs[k] = wave_sum(g[k]);
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
        for (int k = 0; k < kSepSums; ++k) sh[w][4 + k] = gs[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0, c = INFINITY, d = INFINITY, e[kSepSums] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < kGradThreads / 64; ++k) {
            a += sh[k][0];
            b += sh[k][1];
            c = fmin(c, sh[k][2]);
            d = fmin(d, sh[k][3]);
            for (int j = 0; j < kSepSums; ++j) e[j] += sh[k][4 + j];
        }
        double* o = rec + kSepRec * block;
        o[0] = a;
        o[1] = b;
        o[2] = c;
        o[3] = d;
        for (int j = 0; j < kSepSums; ++j) o[4 + j] = e[j];
    }
}

// a point held as (space 0, space 1 or 0, time): dim = 3 as stored, dim = 2 with the time moved to slot 2.  The
// far points (far, 0, 0) pass through unchanged for either dimension.
__device__ __forceinline__ void load_point_sep(const double* __restrict__ p, int dim, double (&x)[3]) {
    x[0] = p[0];
    x[1] = *(dim == 3 ? p + 1 : kZeroValue);
    x[2] = p[dim - 1];
}

// the two squared distances, each floored as point_d2 floors its own (the last coordinate first)
__device__ __forceinline__ void sep_d2(const double (&a)[3], const double (&b)[3], double& ds2, double& dt2) {
    const double t = a[2] - b[2], y = a[1] - b[1], x = a[0] - b[0];
    dt2 = fma(t, t, NNGP_D2_FLOOR);
    ds2 = fma(x, x, fma(y, y, NNGP_D2_FLOOR));
}

// rho_s rho_t: two run-time-kind evaluations at sigma2 = 1 (tab = 2^(j/256))
__device__ __forceinline__ double sep_rho(const CovParams& Ps, const CovParams& Pt, const double* tab,
                                          const double (&a)[3], const double (&b)[3]) {
    double ds2, dt2;
    sep_d2(a, b, ds2, dt2);
    return nngp_cov_d2<NNGP_KIND_GENERIC>(Ps, tab, ds2) * nngp_cov_d2<NNGP_KIND_GENERIC>(Pt, tab, dt2);
}

// one factor's rho(u) and dv(u) = u rho'(u) at squared distance d2 (nngp_cov_d2's generic branch with the
// derivative's bracket alongside); dv is exactly 0 at the floor
__device__ __forceinline__ void sep_rho_dv(const CovParams& Pc, const double (&g)[3], const double* tab, double d2,
                                           double& rho, double& dv) {
    const double x = fmin(d2, Pc.d2max);
    const double d = nngp_sqrt(x);
    const double e = nngp_exp_tab(Pc, tab, Pc.gauss ? x : d);
    const double u = fmin(Pc.phi * d, Pc.umax);
    rho = fma(u, fma(u, fma(u, Pc.c[2], Pc.c[1]), Pc.c[0]), 1.0) * e;
    const double v = u * e * fma(u, fma(u, g[2], g[1]), g[0]);
    dv = d2 > NNGP_D2_FLOOR ? v : 0.0;
}

template <int M, int P, bool GRAD>
__global__ __launch_bounds__(kGradThreads) void bf_sep(const double* __restrict__ coords, int64_t n_points,
                                                       const int32_t* __restrict__ nbr,
                                                       const int32_t* __restrict__ order, int64_t n_rows, int64_t i0,
                                                       const CovParams Ps, const CovParams Pt, const SepParams Sp,
                                                       const double* __restrict__ values,
                                                       const double* __restrict__ qcoords,
                                                       const double* __restrict__ qvalues, double* __restrict__ Bout,
                                                       double* __restrict__ Fout, double* __restrict__ Rout,
                                                       double* __restrict__ Gout, double* __restrict__ rec, int dim) {
    static_assert(M >= 1 && M <= 32, "the validity mask holds one bit per neighbour slot");
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
                R[s][b] = Sp.sigma2 * sep_rho(Ps, Pt, etab, o[s], xb);
            } else if (b < P * s + P - 1) {  // diagonal block: lane-dependent
                const double c = Sp.sigma2 * sep_rho(Ps, Pt, etab, o[s], xb);
                R[s][b] = b < a ? c : (b == a ? Sp.diag : 0.0);
            } else {
                R[s][b] = b == a ? Sp.diag : 0.0;
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

        // ---- second pass over the own strict-lower pairs (a > b): the two sums of each factor, at sigma2 = 1
        double dfs = 0.0, drs = 0.0, dft = 0.0, drt = 0.0;
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
                double ds2, dt2, rs, rt, vs, vt;
                sep_d2(o[s], xb, ds2, dt2);
                sep_rho_dv(Ps, Sp.gs, etab, ds2, rs, vs);
                sep_rho_dv(Pt, Sp.gt, etab, dt2, rt, vt);
                const bool ok = a > b && rowok[s] && colok;
                const double Ds = ok ? vs * rt : 0.0;
                const double Dt = ok ? rs * vt : 0.0;
                const double wf = uo[s] * ub;
                const double wr = fma(ao[s], ub, alb * uo[s]);
                dfs = fma(Ds, wf, dfs);
                drs = fma(Ds, wr, drs);
                dft = fma(Dt, wf, dft);
                drt = fma(Dt, wr, drt);
            }
            // (the four sums pass through an opaque barrier per column, as bf_grad_aniso's: it keeps the compiler from
            // sinking every column's accumulation below the last column)
            asm volatile("" : "+v"(dfs), "+v"(drs), "+v"(dft), "+v"(drt));
            __builtin_amdgcn_sched_barrier(0);
        }
        const double nb2 = gsum<P>(nbp);
        const double adb = gsum<P>(abp);
        const double dFps = 2.0 * gsum<P>(dfs) * Sp.sips;
        const double drps = -gsum<P>(drs) * Sp.sips;
        const double dFpt = 2.0 * gsum<P>(dft) * Sp.sipt;
        const double drpt = -gsum<P>(drt) * Sp.sipt;

        const double w = 1.0 - res * res * iF;  // 1 - r^2 / F
        const double dFt = 1.0 + nb2;
        const double dFs = (F - Sp.tau2 * dFt) * Sp.isig2;
        const double drsg = -Sp.tau2 * adb * Sp.isig2;
        double g[kSepSums];
        g[0] = -0.5 * iF * fma(dFs, w, 2.0 * res * drsg);
        g[1] = -0.5 * iF * fma(dFps, w, 2.0 * res * drps);
        g[2] = -0.5 * iF * fma(dFpt, w, 2.0 * res * drpt);
        g[3] = -0.5 * iF * fma(dFt, w, 2.0 * res * adb);
        if (Gout != nullptr && lead) {
#pragma unroll
            for (int k = 0; k < kSepSums; ++k) Gout[rr * kSepSums + k] = bad ? NAN : g[k];
        }
        if (!lead) g[0] = g[1] = g[2] = g[3] = 0.0;
        block_sep_store(lf, qq, badp, badi, g, rec, blk);
    }
}

template <int M>
static bool launch_sep_if(const SepArgs& a, bool grad, hipStream_t s) {
    if (a.m != M) return false;
    constexpr int P = grad_lanes(M);
    const CovParams Ps = nngp_cov_params(a.kind_s, 1.0, a.phi_s, 0.0);
    const CovParams Pt = nngp_cov_params(a.kind_t, 1.0, a.phi_t, 0.0);
    const SepParams Sp = sep_params(a.kind_s, a.kind_t, a.sigma2, a.phi_s, a.phi_t, a.tau2);
    const dim3 grid((unsigned)bf_grad_blocks(a.n_rows, M)), block(kGradThreads);
    if (grad)
        hipLaunchKernelGGL((bf_sep<M, P, true>), grid, block, 0, s, a.coords, a.n_points, a.nbr, a.order, a.n_rows, a.i0,
                           Ps, Pt, Sp, a.values, a.qcoords, a.qvalues, a.B, a.F, a.R, a.G, a.rec, a.dim);
    else
        hipLaunchKernelGGL((bf_sep<M, P, false>), grid, block, 0, s, a.coords, a.n_points, a.nbr, a.order, a.n_rows, a.i0,
                           Ps, Pt, Sp, a.values, a.qcoords, a.qvalues, a.B, a.F, a.R, a.G, a.rec, a.dim);
    return true;
}

// the instantiation units (bf_sep_m*.hip) and the dispatch + folds (bf_sep.hip)
bool bf_sep_launch_a(const SepArgs& a, bool grad, hipStream_t s);
bool bf_sep_launch_b(const SepArgs& a, bool grad, hipStream_t s);
bool bf_sep_launch_c(const SepArgs& a, bool grad, hipStream_t s);
bool bf_sep_launch_d(const SepArgs& a, bool grad, hipStream_t s);
bool bf_sep_launch_e(const SepArgs& a, bool grad, hipStream_t s);
bool bf_sep_launch_f(const SepArgs& a, bool grad, hipStream_t s);
bool bf_sep_launch_g(const SepArgs& a, bool grad, hipStream_t s);
bool bf_sep_launch_h(const SepArgs& a, bool grad, hipStream_t s);
// forward (grad == nullptr: partials[4] by bf_finalize's fold) or gradient (partials[4], grad[4] by bf_sep_finalize)
hipError_t bf_sep_launch(const SepArgs& a, double* partials, double* grad, hipStream_t s);

}  // namespace nngp
