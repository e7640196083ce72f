// d/dphi of the NNGP factors, one fused sweep: B, F and their phi-derivatives dB, dF per location.
//
// bf_grad.h's layout (grad_lanes(m) lanes per location, joint-block rows dealt cyclically, DPP up to 4 lanes and
// permutes above, right-looking elimination, back-substitution for b on the finished factor) with the value
// column left out and three added steps.  For location i with joint block C (nugget on the whole diagonal),
// c = C[:k, k], b = C_N^-1 c, u = [-b; 1], F = u^T C u, and D_ab = sigma2 d_ab rho'(phi d_ab) (zero diagonal, the
// D of bf_grad.h):
//
//   dB_i / dphi = C_N^-1 (D_c - D_N b) = C_N^-1 (D u)[:k]
//   dF_i / dphi = u^T D u                      (b minimises F: no db term)
//
//   * one pass over each lane's own strict-lower pairs (a > b) recomputes d^2 from the coordinates the lane still
//     holds and adds D_ab u_b to its own row's sum and D_ab u_a to column b's, which a group sum hands to the
//     owner of row b: every lane ends with (D u)_a of its rows, and dF = sum_a u_a (D u)_a;
//   * w = L_N^-1 g runs right-looking on the factor the lanes still hold (one broadcast per column, as the value
//     column did in the elimination), dB = L_N^-T w is the back-substitution of b over again;
//   * no derivative block is stored: a lane adds one vector of S doubles to what the elimination needs;
//   * slots without a point (-1 padding) or with an out-of-range index are masked: u and D are exactly 0 there,
//     so they add nothing to dF, and B and dB are stored as exactly 0; a bad-pivot row stores NaN in all four.
//
// One instantiation per m: the kind (0..4) and the dimension (1..3) are runtime arguments, as in bf_grad<M, P>.
// Per-block records are bf_group's four (sum log F, sum dF / F, first bad-pivot row, first bad-index row), folded
// by bf_finalize in its fixed order.
#pragma once
#include "bf_grad.h"

namespace nngp {

struct DphiArgs {
    const double* coords;  // (n_points, dim)
    int64_t n_points;
    const int32_t* nbr;    // (n_rows, m), -1 padded
    const int32_t* order;  // or null
    int64_t n_rows, i0;
    int m, kind, dim;
    double sigma2, phi, tau2;
    double *B, *F, *dB, *dF;  // (n_rows, m), (n_rows,), (n_rows, m), (n_rows,)
    double* rec;              // 4 doubles per block
};

template <int M, int P>
__global__ __launch_bounds__(kGradThreads) void bf_dphi(const double* __restrict__ coords, int64_t n_points,
                                                        const int32_t* __restrict__ nbr,
                                                        const int32_t* __restrict__ order, int64_t n_rows, int64_t i0,
                                                        const CovParams Pc, const GradParams Gp,
                                                        double* __restrict__ Bout, double* __restrict__ Fout,
                                                        double* __restrict__ dBout, double* __restrict__ dFout,
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
    double o[S][DA];
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
        load_point_rt(pc, dim, o[s]);
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
        }
    }
    const double F = gbcast<P>(R[M / P][M], M % P);
    bad |= !(F > 0.0);

    // ---- b = L_N^-T v (v = row M of L); lane q ends with b of its own rows
    double bown[S];
#pragma unroll
    for (int s = 0; s < S; ++s) bown[s] = 0.0;
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

    // ---- u = [-b; 1], exactly 0 in slots without a point
    double uo[S], go[S];
    bool rowok[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int a = P * s + q;
        const bool nb = a < M && oval[s];
        rowok[s] = nb || a == M;
        uo[s] = nb ? -bown[s] : (a == M ? 1.0 : 0.0);
        go[s] = 0.0;
    }

    // ---- second pass over the own strict-lower pairs (a > b): go[s] = (D u)_a of the own rows
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
        const bool colok = (vm >> (b & 31)) & 1u;
        double cp = 0.0;  // this lane's part of (D u)_b from the rows below b
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
            go[s] = fma(D, ub, go[s]);
            cp = fma(D, uo[s], cp);
        }
        const double cb = gsum<P>(cp);
        go[b / P] = q == b % P ? go[b / P] + cb : go[b / P];
        __builtin_amdgcn_sched_barrier(0);
    }
    double dfp = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) dfp = fma(uo[s], go[s], dfp);
    const double dF = gsum<P>(dfp);

    // ---- w = L_N^-1 g, right-looking: the owner of row p scales, everyone below subtracts
#pragma unroll
    for (int p = 0; p < M; ++p) {
        const int qp = p % P, sp = p / P;
        go[sp] = q == qp ? go[sp] * R[sp][p] : go[sp];
        const double wp = gbcast<P>(go[sp], qp);
#pragma unroll
        for (int s = sp; s < S; ++s) {
            if (s == sp) {
                if (P > 1) go[s] = q > qp ? fma(-R[s][p], wp, go[s]) : go[s];
            } else {
                go[s] = fma(-R[s][p], wp, go[s]);
            }
        }
    }
    // ---- dB = L_N^-T w
    double down[S];
#pragma unroll
    for (int s = 0; s < S; ++s) down[s] = 0.0;
#pragma unroll
    for (int a = M - 1; a >= 0; --a) {
        double pd = 0.0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (P * s + P - 1 <= a) continue;
            const int ar = P * s + q;
            pd = (ar > a && ar < M) ? fma(R[s][a], down[s], pd) : pd;
        }
        const double td = gsum<P>(pd);
        const double wa = gbcast<P>(go[a / P], a % P);
        const double iva = gbcast<P>(R[a / P][a], a % P);
        const double da = (wa - td) * iva;
        down[a / P] = q == a % P ? da : down[a / P];
    }

    if (live) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int a = P * s + q;
            if (a < M) {
                Bout[rr * M + a] = bad ? NAN : (oval[s] ? bown[s] : 0.0);
                dBout[rr * M + a] = bad ? NAN : (oval[s] ? down[s] : 0.0);
            }
        }
    }
    const bool lead = live && q == 0;
    if (lead) {
        Fout[rr] = bad ? NAN : F;
        dFout[rr] = bad ? NAN : dF;
    }
    double lf = 0.0, qq = 0.0, badp = INFINITY, badi = INFINITY;
    if (lead) {
        lf = log(F);
        qq = dF / F;
        if (bad) badp = (double)i;
    }
    if (live && bad_index) badi = (double)i;
    block_partials_store(lf, qq, badp, badi, rec, blk);
}

template <int M>
static bool launch_dphi_if(const DphiArgs& a, hipStream_t s) {
    if (a.m != M) return false;
    constexpr int P = grad_lanes(M);
    const CovParams Pc = nngp_cov_params(a.kind, a.sigma2, a.phi, a.tau2);
    const GradParams Gp = grad_params(a.kind, a.sigma2, a.tau2);
    hipLaunchKernelGGL((bf_dphi<M, P>), dim3((unsigned)bf_grad_blocks(a.n_rows, M)), dim3(kGradThreads), 0, s, a.coords,
                       a.n_points, a.nbr, a.order, a.n_rows, a.i0, Pc, Gp, a.B, a.F, a.dB, a.dF, a.rec, a.dim);
    return true;
}

// the instantiation units (bf_dphi_m*.hip) and the dispatch + fold (bf_dphi.hip)
bool bf_dphi_launch_a(const DphiArgs& a, hipStream_t s);
bool bf_dphi_launch_b(const DphiArgs& a, hipStream_t s);
bool bf_dphi_launch_c(const DphiArgs& a, hipStream_t s);
bool bf_dphi_launch_d(const DphiArgs& a, hipStream_t s);
bool bf_dphi_launch_e(const DphiArgs& a, hipStream_t s);
bool bf_dphi_launch_f(const DphiArgs& a, hipStream_t s);
bool bf_dphi_launch_g(const DphiArgs& a, hipStream_t s);
bool bf_dphi_launch_h(const DphiArgs& a, hipStream_t s);
hipError_t bf_dphi_launch(const DphiArgs& a, double* partials, hipStream_t s);

}  // namespace nngp
