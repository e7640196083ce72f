// Per-point noise in the response model: y_i = mu + w(s_i) + e_i, e_i ~ N(0, tau2 v_i), v_i >= 0 given per point.
//
// The joint block of location i is the homoscedastic one (bf_sweep.hip) with the diagonal entry of the point in
// slot a equal to sigma2 + tau2 v_a instead of sigma2 + tau2 -- the location's own entry included -- so the
// weight is gathered with the point's coordinates and nothing else in the factorisation changes.  One kernel on
// bf_grad.h's layout (P = grad_lanes(m) lanes per location, rows dealt cyclically, right-looking elimination
// with the value column carried along), instantiated twice per m, kind (0..4) and dimension (1..3) at run time:
//
//   GRAD = false  the forward sweep (nngp_bf_sweep_noise, nngp_bf_cross_noise): B, F, R and bf_group's block
//                 records; the location's coordinates, value and weight come from the q* arrays (the cross form);
//   GRAD = true   the gradient sweep (nngp_bf_grad_noise): bf_grad's second back-substitution and second pass.
//                 With V = diag(v) on the joint block, in bf_grad.h's notation:
//                   tau2:    dC = V                      dF = v_i + sum_j b_j^2 v_j        dr = sum_j a_j b_j v_j
//                   sigma2:  dC = (C - tau2 V) / sigma2  dF = (F - tau2 dF_tau2) / sigma2  dr = -tau2 dr_tau2 / sigma2
//                   phi:     unchanged (the diagonal of D is zero).
//
// Slots without a point (-1 padding, out-of-range indices) keep the homoscedastic diagonal sigma2 + tau2: they
// are decoupled (far points), so their entry only has to be positive.  At v = 1 the model is bf_sweep's / bf_grad's
// and the results agree with theirs to rounding; they are not bit-identical (the forward sweep is another kernel
// than the pair sweep, and the gradient's rows were measured to differ from bf_grad's in the last bits).
#pragma once
#include "bf_grad.h"

namespace nngp {

static __device__ double kNoiseOne[1] = {1.0};  // the weight of a query point given none (nngp_bf_cross_noise)

struct NoiseArgs {
    const double* coords;  // (n_points, dim)
    int64_t n_points;
    const int32_t* nbr;    // (n_rows, m), -1 padded
    const int32_t* order;  // or null
    int64_t n_rows, i0;
    int m, kind, dim;
    double sigma2, phi, tau2;
    const double* values;   // (n_points,); null allowed for the forward sweep
    const double* noise;    // (n_points,) weights v_j of the neighbours
    const double* qcoords;  // the locations themselves: coords (S = T) or the query points (cross)
    const double* qvalues;  // values (S = T), query values or null
    const double* qnoise;   // noise (S = T), the query points' weights, or null: 1
    double* B;              // forward: (n_rows, m) or null
    double* F;              // forward: (n_rows,) or null
    double* R;              // forward: (n_rows,) or null
    double* G;              // gradient: (n_rows, 3) or null
    double* rec;            // 4 (forward) or kGradRec (gradient) doubles per block
};

template <int M, int P, bool GRAD>
__global__ __launch_bounds__(kGradThreads) void bf_noise(const double* __restrict__ coords, int64_t n_points,
                                                         const int32_t* __restrict__ nbr,
                                                         const int32_t* __restrict__ order, int64_t n_rows, int64_t i0,
                                                         const CovParams Pc, const GradParams Gp,
                                                         const double* __restrict__ values,
                                                         const double* __restrict__ noise,
                                                         const double* __restrict__ qcoords,
                                                         const double* __restrict__ qvalues,
                                                         const double* __restrict__ qnoise, double* __restrict__ Bout,
                                                         double* __restrict__ Fout, double* __restrict__ Rout,
                                                         double* __restrict__ Gout, double* __restrict__ rec, int dim) {
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

    // ---- own rows a = P*s + q: neighbour slot (a < M), the location (a == M), padding (a > M); the weight is
    // gathered with the point (branch-free: resolved addresses, as bf_group)
    int32_t jn[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int a = P * s + q;
        jn[s] = nbr[rl * M + (a < M ? a : M - 1)];
    }
    double o[S][DA], z[S], vw[S], dg[S];
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
        const double* pn = self ? (qnoise != nullptr ? qnoise + i : kNoiseOne) : (in_range ? noise + j : kZeroValue);
        load_point_rt(pc, dim, o[s]);
        z[s] = *pv;
        vw[s] = *pn;
        dg[s] = (self || in_range) ? fma(Gp.tau2, vw[s], Pc.sigma2) : Pc.diag;
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
                R[s][b] = nngp_cov_d2<NNGP_KIND_GENERIC>(Pc, etab, point_d2<DA>(o[s], xb));
            } else if (b < P * s + P - 1) {  // diagonal block: lane-dependent
                const double c = nngp_cov_d2<NNGP_KIND_GENERIC>(Pc, etab, point_d2<DA>(o[s], xb));
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
        // ---- u = [-b; 1], alpha = [a; 0], exactly 0 in slots without a point; sum b^2 v and sum a b v
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
            nbp = nb ? fma(bown[s] * vw[s], bown[s], nbp) : nbp;
            abp = nb ? fma(aown[s] * vw[s], bown[s], abp) : abp;
        }
        const double vself = gbcast<P>(vw[M / P], M % P);

        // ---- second pass over the own strict-lower pairs (a > b): the two phi sums (bf_grad's, unchanged)
        double dfp = 0.0, drp = 0.0;
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

        const double w = 1.0 - res * res * iF;  // 1 - r^2 / F
        const double dFt = vself + nb2;
        const double dFs = (F - Gp.tau2 * dFt) * Gp.isig2;
        const double drs = -Gp.tau2 * adb * Gp.isig2;
        double g[3];
        g[0] = -0.5 * iF * fma(dFs, w, 2.0 * res * drs);
        g[1] = -0.5 * iF * fma(dFphi, w, 2.0 * res * drphi);
        g[2] = -0.5 * iF * fma(dFt, w, 2.0 * res * adb);
        if (Gout != nullptr && lead) {
#pragma unroll
            for (int k = 0; k < 3; ++k) Gout[rr * 3 + k] = bad ? NAN : g[k];
        }
        if (!lead) g[0] = g[1] = g[2] = 0.0;
        block_grad_store(lf, qq, badp, badi, g, rec, blk);
    }
}

template <int M>
static bool launch_noise_if(const NoiseArgs& a, bool grad, hipStream_t s) {
    if (a.m != M) return false;
    constexpr int P = grad_lanes(M);
    const CovParams Pc = nngp_cov_params(a.kind, a.sigma2, a.phi, a.tau2);
    const GradParams Gp = grad_params(a.kind, a.sigma2, a.tau2);
    const dim3 grid((unsigned)bf_grad_blocks(a.n_rows, M)), block(kGradThreads);
    if (grad)
        hipLaunchKernelGGL((bf_noise<M, P, true>), grid, block, 0, s, a.coords, a.n_points, a.nbr, a.order, a.n_rows, a.i0,
                           Pc, Gp, a.values, a.noise, a.qcoords, a.qvalues, a.qnoise, a.B, a.F, a.R, a.G, a.rec, a.dim);
    else
        hipLaunchKernelGGL((bf_noise<M, P, false>), grid, block, 0, s, a.coords, a.n_points, a.nbr, a.order, a.n_rows,
                           a.i0, Pc, Gp, a.values, a.noise, a.qcoords, a.qvalues, a.qnoise, a.B, a.F, a.R, a.G, a.rec,
                           a.dim);
    return true;
}

// the instantiation units (bf_noise_m*.hip) and the dispatch + folds (bf_noise.hip)
bool bf_noise_launch_a(const NoiseArgs& a, bool grad, hipStream_t s);
bool bf_noise_launch_b(const NoiseArgs& a, bool grad, hipStream_t s);
bool bf_noise_launch_c(const NoiseArgs& a, bool grad, hipStream_t s);
bool bf_noise_launch_d(const NoiseArgs& a, bool grad, hipStream_t s);
bool bf_noise_launch_e(const NoiseArgs& a, bool grad, hipStream_t s);
bool bf_noise_launch_f(const NoiseArgs& a, bool grad, hipStream_t s);
bool bf_noise_launch_g(const NoiseArgs& a, bool grad, hipStream_t s);
bool bf_noise_launch_h(const NoiseArgs& a, bool grad, hipStream_t s);
// forward (grad == nullptr: partials[4] by bf_finalize's fold) or gradient (partials[4], grad[3] by bf_grad's)
hipError_t bf_noise_launch(const NoiseArgs& a, double* partials, double* grad, hipStream_t s);

}  // namespace nngp
