// Fisher information of the NNGP log-likelihood in (sigma2, phi, tau2), with the log-likelihood's terms and its
// gradient, one fused sweep.
//
// bf_dphi.h's layout (grad_lanes(m) lanes per location, joint-block rows dealt cyclically, DPP up to 4 lanes and
// permutes above, right-looking elimination, back-substitution for b on the finished factor) with bf_grad.h's
// value column carried through the elimination and one added forward solve.  For location i with joint block C
// (nugget on the whole diagonal), C_N = L L^T, c = C[:k, k], b = C_N^-1 c, u = [-b; 1], F = u^T C u,
// D_ab = sigma2 d_ab rho'(phi d_ab) (zero diagonal), z = L^-1 y_N, r = y_i - b^T y_N:
//
//   w = L^-1 (D u)[:k]                (bf_dphi.h's w)
//   t = L^-1 b                        (the added solve; it shares w's factor reads and column loop)
//   dF = ((F - tau2 (1 + |b|^2)) / sigma2, u^T D u, 1 + |b|^2)              in the order (sigma2, phi, tau2)
//   W  = ((tau2 / sigma2) t, w, -t)   the L-whitened db / dtheta
//   I_i[j,k]  = 1/2 dF_j dF_k / F^2 + W_j . W_k / F                        (the row's expected information)
//   d l_i / d theta_j = -1/2 (dF_j / F) (1 - r^2 / F) + r (W_j . z) / F
//
//   * the information needs three dot products over the neighbour rows (w.w, w.t, t.t), the gradient two more
//     (w.z, t.z); |b|^2 and u^T D u are bf_grad's and bf_dphi's;
//   * there is no back-substitution after the forward solves (nothing needs C_N^-1 (D u)), and no B, dB or
//     derivative block is stored;
//   * slots without a point (-1 padding) or with an out-of-range index are masked: u, D, t and every dot product's
//     term are exactly 0 there; a bad-pivot row stores NaN in its row outputs;
//   * without values (a null pointer) the value column is 0 and the gradient outputs are written as exactly 0; the
//     information does not read the values, so it is bit for bit that of the call with values.
//
// One instantiation per m: the kind (0..4) and the dimension (1..3) are runtime arguments, as in bf_dphi<M, P>.
// Per-block records are kFisherRec doubles: bf_group's four (sum log F, sum r^2 / F, first bad-pivot row, first
// bad-index row), the three gradient sums and the six information sums (the upper triangle, row-major:
// ss, sp, st, pp, pt, tt), folded by bf_fisher_finalize in bf_finalize's fixed order.
#pragma once
#include "bf_grad.h"

namespace nngp {

constexpr int kFisherRec = 13;
constexpr int kFisherSums = 11;  // the records that are sums: 0, 1 and 4..12

struct FisherArgs {
    const double* coords;  // (n_points, dim)
    int64_t n_points;
    const int32_t* nbr;    // (n_rows, m), -1 padded
    const int32_t* order;  // or null
    int64_t n_rows, i0;
    int m, kind, dim;
    double sigma2, phi, tau2;
    const double* values;  // (n_points,) or null
    double* I_rows;        // (n_rows, 6) or null
    double* G;             // (n_rows, 3) or null
    double* rec;           // kFisherRec doubles per block
};

// Fixed-order reduction of one block's sums into rec[kFisherRec * block ..] (block_grad_store with the six
// information sums alongside).  v holds the sums in record order without the two flags: log F, r^2 / F, the
// gradient's three, the information's six.  Every thread of the block calls it.
__device__ __forceinline__ void block_fisher_store(const double (&v)[kFisherSums], double badp, double badi, double* rec,
                                                   int64_t block) {
    __shared__ double sh[kGradThreads / 64][kFisherRec];
    double vs[kFisherSums];
#pragma unroll
    for (int k = 0; k < kFisherSums; ++k) vs[k] = wave_sum(v[k]);
    if (__any(badp != INFINITY || badi != INFINITY)) {  // wave-uniform; rare
        badp = wave_min(badp);
        badi = wave_min(badi);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh[w][0] = vs[0];
        sh[w][1] = vs[1];
        sh[w][2] = badp;
        sh[w][3] = badi;
#pragma unroll
        for (int k = 2; k < kFisherSums; ++k) sh[w][2 + k] = vs[k];
    }
    __syncthreads();
    if (threadIdx.x < kFisherRec) {
        const int k = threadIdx.x;
        const bool is_min = k == 2 || k == 3;
        double a = is_min ? INFINITY : 0.0;
        for (int j = 0; j < kGradThreads / 64; ++j) a = is_min ? fmin(a, sh[j][k]) : a + sh[j][k];
        rec[kFisherRec * block + k] = a;
    }
}

template <int M, int P>
__global__ __launch_bounds__(kGradThreads) void bf_fisher(const double* __restrict__ coords, int64_t n_points,
                                                          const int32_t* __restrict__ nbr,
                                                          const int32_t* __restrict__ order, int64_t n_rows, int64_t i0,
                                                          const CovParams Pc, const GradParams Gp,
                                                          const double* __restrict__ values, double* __restrict__ Iout,
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
    const bool has_values = values != nullptr;

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
        const double* pv = !has_values ? kZeroValue : self ? values + i : (in_range ? values + j : kZeroValue);
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

    // ---- right-looking elimination with the value column; the owner of row p keeps 1/L[p][p] in R[p/P][p]
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

    // ---- u = [-b; 1] and the right-hand side of t (b itself), exactly 0 in slots without a point; |b|^2
    double uo[S], go[S], to[S];
    bool rowok[S], nbrow[S];
    double nbp = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int a = P * s + q;
        const bool nb = a < M && oval[s];
        nbrow[s] = nb;
        rowok[s] = nb || a == M;
        uo[s] = nb ? -bown[s] : (a == M ? 1.0 : 0.0);
        to[s] = nb ? bown[s] : 0.0;
        go[s] = 0.0;
        nbp = nb ? fma(bown[s], bown[s], nbp) : nbp;
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

    // ---- w = L_N^-1 g and t = L_N^-1 b together, right-looking: the owner of row p scales, everyone below
    // subtracts (row M's entries ride along and are not read)
#pragma unroll
    for (int p = 0; p < M; ++p) {
        const int qp = p % P, sp = p / P;
        go[sp] = q == qp ? go[sp] * R[sp][p] : go[sp];
        to[sp] = q == qp ? to[sp] * R[sp][p] : to[sp];
        const double wp = gbcast<P>(go[sp], qp);
        const double tp = gbcast<P>(to[sp], qp);
#pragma unroll
        for (int s = sp; s < S; ++s) {
            if (s == sp) {
                if (P > 1) {
                    go[s] = q > qp ? fma(-R[s][p], wp, go[s]) : go[s];
                    to[s] = q > qp ? fma(-R[s][p], tp, to[s]) : to[s];
                }
            } else {
                go[s] = fma(-R[s][p], wp, go[s]);
                to[s] = fma(-R[s][p], tp, to[s]);
            }
        }
    }

    // ---- the dot products over the neighbour rows
    double wwp = 0.0, wtp = 0.0, ttp = 0.0, wzp = 0.0, tzp = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const bool nb = nbrow[s];
        wwp = nb ? fma(go[s], go[s], wwp) : wwp;
        wtp = nb ? fma(go[s], to[s], wtp) : wtp;
        ttp = nb ? fma(to[s], to[s], ttp) : ttp;
        wzp = nb ? fma(go[s], z[s], wzp) : wzp;
        tzp = nb ? fma(to[s], z[s], tzp) : tzp;
    }
    const double dFphi = gsum<P>(dfp);
    const double nb2 = gsum<P>(nbp);
    const double ww = gsum<P>(wwp);
    const double wt = gsum<P>(wtp);
    const double tt = gsum<P>(ttp);
    const double wz = gsum<P>(wzp);
    const double tz = gsum<P>(tzp);

    const double iF = 1.0 / F;
    const double ts = Gp.tau2 * Gp.isig2;
    const double dFt = 1.0 + nb2;
    const double dFs = (F - Gp.tau2 * dFt) * Gp.isig2;
    const double as = dFs * iF, ap = dFphi * iF, at = dFt * iF;
    double v[kFisherSums];
    // information, upper triangle: ss, sp, st, pp, pt, tt
    v[5] = fma(0.5 * as, as, ts * ts * tt * iF);
    v[6] = fma(0.5 * as, ap, ts * wt * iF);
    v[7] = fma(0.5 * as, at, -(ts * tt) * iF);
    v[8] = fma(0.5 * ap, ap, ww * iF);
    v[9] = fma(0.5 * ap, at, -wt * iF);
    v[10] = fma(0.5 * at, at, tt * iF);
    // gradient
    const double wq = 1.0 - res * res * iF;  // 1 - r^2 / F
    const double riF = res * iF;
    v[2] = has_values ? fma(-0.5 * as, wq, riF * (ts * tz)) : 0.0;
    v[3] = has_values ? fma(-0.5 * ap, wq, riF * wz) : 0.0;
    v[4] = has_values ? fma(-0.5 * at, wq, -riF * tz) : 0.0;

    const bool lead = live && q == 0;
    if (lead) {
        if (Iout != nullptr) {
#pragma unroll
            for (int k = 0; k < 6; ++k) Iout[rr * 6 + k] = bad ? NAN : v[5 + k];
        }
        if (Gout != nullptr) {
#pragma unroll
            for (int k = 0; k < 3; ++k) Gout[rr * 3 + k] = (bad && has_values) ? NAN : v[2 + k];
        }
    }
    double badp = INFINITY, badi = INFINITY;
    if (lead) {
        v[0] = log(F);
        v[1] = res * res * iF;
        if (bad) badp = (double)i;
    } else {
#pragma unroll
        for (int k = 0; k < kFisherSums; ++k) v[k] = 0.0;
    }
    if (live && bad_index) badi = (double)i;
    block_fisher_store(v, badp, badi, rec, blk);
}

template <int M>
static bool launch_fisher_if(const FisherArgs& a, hipStream_t s) {
    if (a.m != M) return false;
    constexpr int P = grad_lanes(M);
    const CovParams Pc = nngp_cov_params(a.kind, a.sigma2, a.phi, a.tau2);
    const GradParams Gp = grad_params(a.kind, a.sigma2, a.tau2);
    hipLaunchKernelGGL((bf_fisher<M, P>), dim3((unsigned)bf_grad_blocks(a.n_rows, M)), dim3(kGradThreads), 0, s,
                       a.coords, a.n_points, a.nbr, a.order, a.n_rows, a.i0, Pc, Gp, a.values, a.I_rows, a.G, a.rec,
                       a.dim);
    return true;
}

// the instantiation units (bf_fisher_m*.hip) and the dispatch + fold (bf_fisher.hip)
bool bf_fisher_launch_a(const FisherArgs& a, hipStream_t s);
bool bf_fisher_launch_b(const FisherArgs& a, hipStream_t s);
bool bf_fisher_launch_c(const FisherArgs& a, hipStream_t s);
bool bf_fisher_launch_d(const FisherArgs& a, hipStream_t s);
bool bf_fisher_launch_e(const FisherArgs& a, hipStream_t s);
bool bf_fisher_launch_f(const FisherArgs& a, hipStream_t s);
bool bf_fisher_launch_g(const FisherArgs& a, hipStream_t s);
bool bf_fisher_launch_h(const FisherArgs& a, hipStream_t s);
hipError_t bf_fisher_launch(const FisherArgs& a, double* partials, double* grad, double* info, hipStream_t s);

}  // namespace nngp
