// Points in 4 .. 16 dimensions with one decay per axis (ARD):
//   C(a, b) = sigma2 rho(u) + tau2 delta_ab,  u = sqrt(sum_k (phi_k (a_k - b_k))^2),
// rho exponential, Matern-3/2, Matern-5/2 or Gaussian (the spherical kind is not positive definite above three
// dimensions and is refused by the C ABI).
//
// One kernel on bf_grad.h's layout, as bf_noise.h and bf_sep.h are (P = grad_lanes(m) lanes per location, rows dealt
// cyclically, right-looking elimination with the value column carried along, the same flags and block records),
// instantiated twice per m; kind, dimension and the decays are run-time arguments:
//
//   GRAD = false  the forward sweep (nngp_bf_sweep_nd, nngp_bf_cross_nd): B, F, R and bf_group's 4-double block
//                 records; the location's coordinates and value come from the q* arrays (the cross form);
//   GRAD = true   the gradient sweep (nngp_bf_grad_nd) in (sigma2, phi_1..phi_dim, tau2): bf_grad_aniso's second
//                 back-substitution and second pass, dC_ab/dphi_k = sigma2 rho'(u) delta_k^2 / (u phi_k) with
//                 delta_k the scaled coordinate difference.
//
// A lane cannot hold S x 16 own-row coordinates as bf_sep holds S x 3.  The squared scaled distance is accumulated
// axis by axis into the registers that will hold the joint block: one run-time loop over the axes, one coordinate
// per own row live at a time (gathered as the loop goes; a point's row is contiguous, so the axes after the first
// come from L1/L2), and the covariance is evaluated in place afterwards.  The second pass does the same into the
// registers the eliminated block has left (the per-pair weight w = rho'(u) / u), then loops over the axes once more:
// per axis and column b, A_b = sum_a w_ab delta_k^2 u_a and B_b = sum_a w_ab delta_k^2 alpha_a over the own rows
// a > b, folded as u_b A_b and u_b B_b + alpha_b A_b.  An axis's two sums are reduced over the group, turned into
// the row's d l_i / d phi_k, written to G and reduced over the wave before the next axis starts, so no array is
// indexed by the axis in registers.
//
// Slots without a point (-1 padding, an out-of-range index) are masked, not moved far away: their covariances and
// weights are exactly 0, their diagonal is sigma2 + tau2.
#pragma once
#include "bf_grad.h"
#include "nd_host.h"

namespace nngp {

// nd_host.h restates the layout's two constants without HIP
static_assert(kNdThreads == kGradThreads, "nd_host.h's block size is bf_grad.h's");
constexpr bool nd_lanes_agree() {
    for (int m = 1; m <= kNdMaxM; ++m)
        if (nd_lanes(m) != grad_lanes(m)) return false;
    return true;
}
static_assert(nd_lanes_agree(), "nd_host.h's lanes per location are bf_grad.h's");

struct NdArgs {
    const double* coords;  // (n_points, dim), raw
    int64_t n_points;
    const int32_t* nbr;    // (n_rows, m), -1 padded
    const int32_t* order;  // or null
    int64_t n_rows, i0;
    int m, kind, dim;
    double sigma2, tau2;
    const double* phi;      // host, dim decays
    const double* values;   // (n_points,); null allowed for the forward sweep
    const double* qcoords;  // the locations themselves: coords (S = T) or the query points (cross)
    const double* qvalues;  // values (S = T), query values or null
    double* B;              // forward: (n_rows, m) or null
    double* F;              // forward: (n_rows,) or null
    double* R;              // forward: (n_rows,) or null
    double* G;              // gradient: (n_rows, dim + 2) or null
    double* rec;            // 4 (forward) or nd_rec(dim) (gradient) doubles per block
};

struct NdPhi {
    double phi[kNdMaxDim], iphi[kNdMaxDim];  // iphi = 1 / phi; 1 beyond dim
};

template <int M, int P, bool GRAD>
__global__ __launch_bounds__(kGradThreads) void bf_nd(const double* __restrict__ coords, int64_t n_points,
                                                      const int32_t* __restrict__ nbr,
                                                      const int32_t* __restrict__ order, int64_t n_rows, int64_t i0,
                                                      const CovParams Pc, const GradParams Gp, const NdPhi Ph,
                                                      const double* __restrict__ values,
                                                      const double* __restrict__ qcoords,
                                                      const double* __restrict__ qvalues, double* __restrict__ Bout,
                                                      double* __restrict__ Fout, double* __restrict__ Rout,
                                                      double* __restrict__ Gout, double* __restrict__ rec, int dim) {
    static_assert(M >= 1 && M <= 32, "the validity mask holds one bit per neighbour slot");
    constexpr int NR = M + 1;            // joint rows 0..M (row M = the location)
    constexpr int S = (NR + P - 1) / P;  // local rows per lane
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

    // ---- own rows a = P*s + q: neighbour slot (a < M), the location (a == M), padding (a > M).  A row without a
    // point reads point 0 and is masked.
    const double* pc[S];
    double z[S];
    bool oval[S], rowok[S];
    bool bad_index = false;
    uint32_t vm = 0;  // bit a: neighbour slot a holds a point
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int a = P * s + q;
        const int32_t j = a < M ? nbr[rl * M + a] : -1;
        const bool in_range = j >= 0 && (int64_t)j < n_points;
        bad_index |= j != -1 && !in_range;
        oval[s] = in_range;
        vm |= in_range ? (1u << (a & 31)) : 0u;
        const bool self = a == M;
        rowok[s] = self || in_range;
        pc[s] = self ? qcoords + i * dim : coords + (in_range ? (int64_t)j * dim : 0);
        const double* pv = self ? (qvalues != nullptr ? qvalues + i : kZeroValue)
                                : ((values != nullptr && in_range) ? values + j : kZeroValue);
        z[s] = *pv;
    }
    if constexpr (P > 1) vm |= (uint32_t)__builtin_amdgcn_mov_dpp((int)vm, 0xB1, 0xf, 0xf, true);
    if constexpr (P > 2) vm |= (uint32_t)__builtin_amdgcn_mov_dpp((int)vm, 0x4E, 0xf, 0xf, true);
    if constexpr (P > 4) vm |= (uint32_t)__shfl_xor((int)vm, 4);
    if constexpr (P > 8) vm |= (uint32_t)__shfl_xor((int)vm, 8);
    if constexpr (P > 16) vm |= (uint32_t)__shfl_xor((int)vm, 16);
    if constexpr (P > 32) vm |= (uint32_t)__shfl_xor((int)vm, 32);

    // ---- joint block rows: R[s][b], b < min(P*s + P, NR).  First the squared scaled distances, axis by axis (the
    // last column of a local row's diagonal block is never below the diagonal)
    double R[S][NR];
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int b = 0; b < NR; ++b)
            if (b < P * s + P - 1) R[s][b] = NNGP_D2_FLOOR;
#pragma nounroll
    for (int k = 0; k < dim; ++k) {
        const double ph = Ph.phi[k];
        double ok[S];
#pragma unroll
        for (int s = 0; s < S; ++s) ok[s] = pc[s][k] * ph;
#pragma unroll
        for (int b = 0; b < NR; ++b) {
            if (b >= P * (S - 1) + P - 1) continue;  // no local row reaches below this column
            const double xb = gbcast<P>(ok[b / P], b % P);
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (b >= P * s + P - 1) continue;
                const double t = ok[s] - xb;
                R[s][b] = fma(t, t, R[s][b]);
            }
        }
    }
    // ... then the covariances in place
#pragma unroll
    for (int b = 0; b < NR; ++b) {
        const bool colok = b == M ? true : (((vm >> (b & 31)) & 1u) != 0);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int a = P * s + q;
            if (b >= P * s + P) continue;  // beyond this local row's width
            if (b < P * s) {
                const double c = nngp_cov_d2<NNGP_KIND_GENERIC>(Pc, etab, R[s][b]);
                R[s][b] = (rowok[s] && colok) ? c : 0.0;
            } else if (b < P * s + P - 1) {  // diagonal block: lane-dependent
                const double c = nngp_cov_d2<NNGP_KIND_GENERIC>(Pc, etab, R[s][b]);
                R[s][b] = b < a ? ((rowok[s] && colok) ? c : 0.0) : (b == a ? Pc.diag : 0.0);
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
        __shared__ double sh[kGradThreads / 64][kNdRecMax];
        const int wv_ = threadIdx.x >> 6;
        const bool wlead = (threadIdx.x & 63) == 0;
        // ---- u = [-b; 1], alpha = [a; 0], exactly 0 in slots without a point; |b|^2 and a.b
        double uo[S], ao[S];
        double nbp = 0.0, abp = 0.0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int a = P * s + q;
            const bool nb = a < M && oval[s];
            uo[s] = nb ? -bown[s] : (a == M ? 1.0 : 0.0);
            ao[s] = nb ? aown[s] : 0.0;
            nbp = nb ? fma(bown[s], bown[s], nbp) : nbp;
            abp = nb ? fma(aown[s], bown[s], abp) : abp;
        }
        const double nb2 = gsum<P>(nbp);
        const double adb = gsum<P>(abp);
        const double w = 1.0 - res * res * iF;  // 1 - r^2 / F

        // ---- second pass over the own strict-lower pairs (a > b, b < M): the squared scaled distances again, into
        // the registers the block has left ...
        double W[S][NR];
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int b = 0; b < M; ++b)
                if (b < P * s + P - 1) W[s][b] = NNGP_D2_FLOOR;
        // (the pointers pass through an opaque barrier, as bf_grad's coordinates do: it keeps this pass's gathers
        // and distances behind the elimination)
#pragma unroll
        for (int s = 0; s < S; ++s) asm volatile("" : "+v"(pc[s]));
#pragma nounroll
        for (int k = 0; k < dim; ++k) {
            const double ph = Ph.phi[k];
            double ok[S];
#pragma unroll
            for (int s = 0; s < S; ++s) ok[s] = pc[s][k] * ph;
#pragma unroll
            for (int b = 0; b < M; ++b) {
                if (b >= P * (S - 1) + P - 1) continue;
                const double xb = gbcast<P>(ok[b / P], b % P);
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    if (b >= P * s + P - 1) continue;
                    const double t = ok[s] - xb;
                    W[s][b] = fma(t, t, W[s][b]);
                }
            }
        }
        // ... then the per-pair weight w = rho'(u) sigma2 / u in place (bf_grad_aniso's dv / x): exactly 0 for a
        // masked pair, for a <= b and where the distance is the floor
#pragma unroll
        for (int b = 0; b < M; ++b) {
            const bool colok = ((vm >> (b & 31)) & 1u) != 0;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (b >= P * s + P - 1) continue;
                const int a = P * s + q;
                const double x2 = W[s][b];
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
                const double wv = id * e * fma(u, fma(u, Gp.g[2], Gp.g[1]), Gp.g[0]);
                W[s][b] = (a > b && rowok[s] && colok && x2 > NNGP_D2_FLOOR) ? wv : 0.0;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- ... and the axes once more: the two sums of one axis at a time
#pragma nounroll
        for (int k = 0; k < dim; ++k) {
            const double ph = Ph.phi[k];
            double ok[S];
#pragma unroll
            for (int s = 0; s < S; ++s) ok[s] = pc[s][k] * ph;
            double dfk = 0.0, drk = 0.0;
#pragma unroll
            for (int b = 0; b < M; ++b) {
                if (b >= P * (S - 1) + P - 1) continue;
                const double xb = gbcast<P>(ok[b / P], b % P);
                const double ub = gbcast<P>(uo[b / P], b % P);
                const double alb = gbcast<P>(ao[b / P], b % P);
                double Ab = 0.0, Bb = 0.0;
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    if (b >= P * s + P - 1) continue;
                    const double t = ok[s] - xb;
                    const double c = W[s][b] * (t * t);
                    Ab = fma(c, uo[s], Ab);
                    Bb = fma(c, ao[s], Bb);
                }
                dfk = fma(ub, Ab, dfk);
                drk = fma(ub, Bb, fma(alb, Ab, drk));
            }
            const double dFphi = 2.0 * gsum<P>(dfk) * Ph.iphi[k];
            const double drphi = -gsum<P>(drk) * Ph.iphi[k];
            const double gk = -0.5 * iF * fma(dFphi, w, 2.0 * res * drphi);
            if (Gout != nullptr && lead) Gout[rr * (dim + 2) + 1 + k] = bad ? NAN : gk;
            const double gsk = wave_sum(lead ? gk : 0.0);
            if (wlead) sh[wv_][5 + k] = gsk;
        }

        const double dFt = 1.0 + nb2;
        const double dFs = (F - Gp.tau2 * dFt) * Gp.isig2;
        const double drs = -Gp.tau2 * adb * Gp.isig2;
        double g0 = -0.5 * iF * fma(dFs, w, 2.0 * res * drs);
        double g1 = -0.5 * iF * fma(dFt, w, 2.0 * res * adb);
        if (Gout != nullptr && lead) {
            Gout[rr * (dim + 2)] = bad ? NAN : g0;
            Gout[rr * (dim + 2) + 1 + dim] = bad ? NAN : g1;
        }
        if (!lead) g0 = g1 = 0.0;
        // ---- the block record, folded in fixed order (block_grad_store with dim + 2 gradient sums)
        lf = wave_sum(lf);
        qq = wave_sum(qq);
        g0 = wave_sum(g0);
        g1 = wave_sum(g1);
        if (__any(badp != INFINITY || badi != INFINITY)) {  // wave-uniform; rare
            badp = wave_min(badp);
            badi = wave_min(badi);
        }
        if (wlead) {
            sh[wv_][0] = lf;
            sh[wv_][1] = qq;
            sh[wv_][2] = badp;
            sh[wv_][3] = badi;
            sh[wv_][4] = g0;
            sh[wv_][5 + dim] = g1;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int nrec = nd_rec(dim);
            double* o = rec + (int64_t)nrec * blk;
            for (int c = 0; c < nrec; ++c) {
                const bool mn = c == 2 || c == 3;
                double a = mn ? INFINITY : 0.0;
                for (int k = 0; k < kGradThreads / 64; ++k) a = mn ? fmin(a, sh[k][c]) : a + sh[k][c];
                o[c] = a;
            }
        }
    }
}

template <int M>
static bool launch_nd_if(const NdArgs& a, bool grad, hipStream_t s) {
    if (a.m != M) return false;
    constexpr int P = grad_lanes(M);
    const CovParams Pc = nngp_cov_params(a.kind, a.sigma2, 1.0, a.tau2);
    const GradParams Gp = grad_params(a.kind, a.sigma2, a.tau2);
    NdPhi Ph;
    for (int k = 0; k < kNdMaxDim; ++k) {
        Ph.phi[k] = k < a.dim ? a.phi[k] : 1.0;
        Ph.iphi[k] = 1.0 / Ph.phi[k];
    }
    const dim3 grid((unsigned)bf_grad_blocks(a.n_rows, M)), block(kGradThreads);
    if (grad)
        hipLaunchKernelGGL((bf_nd<M, P, true>), grid, block, 0, s, a.coords, a.n_points, a.nbr, a.order, a.n_rows, a.i0,
                           Pc, Gp, Ph, a.values, a.qcoords, a.qvalues, a.B, a.F, a.R, a.G, a.rec, a.dim);
    else
        hipLaunchKernelGGL((bf_nd<M, P, false>), grid, block, 0, s, a.coords, a.n_points, a.nbr, a.order, a.n_rows, a.i0,
                           Pc, Gp, Ph, a.values, a.qcoords, a.qvalues, a.B, a.F, a.R, a.G, a.rec, a.dim);
    return true;
}

// the instantiation units (bf_nd_m*.hip) and the dispatch + folds (bf_nd.hip)
bool bf_nd_launch_a(const NdArgs& a, bool grad, hipStream_t s);
bool bf_nd_launch_b(const NdArgs& a, bool grad, hipStream_t s);
bool bf_nd_launch_c(const NdArgs& a, bool grad, hipStream_t s);
bool bf_nd_launch_d(const NdArgs& a, bool grad, hipStream_t s);
bool bf_nd_launch_e(const NdArgs& a, bool grad, hipStream_t s);
bool bf_nd_launch_f(const NdArgs& a, bool grad, hipStream_t s);
bool bf_nd_launch_g(const NdArgs& a, bool grad, hipStream_t s);
bool bf_nd_launch_h(const NdArgs& a, bool grad, hipStream_t s);
// forward (grad == nullptr: partials[4] by bf_finalize's fold) or gradient (partials[4], grad[dim + 2])
hipError_t bf_nd_launch(const NdArgs& a, double* partials, double* grad, hipStream_t s);

// ---- knn_nd.hip: exact ordered neighbour sets by tiled brute force, dim 4 .. 16
constexpr int kKnnNdQueries = 256;  // queries per block, one per lane
constexpr int kKnnNdTile = 128;     // candidate points per LDS tile
// prior: query row t is point q0 + t and searches coords[0 : q0 + t]; else query row t is query[q0 + t] and searches
// all n points.  nbr rows are (q1 - q0, m).
hipError_t knn_nd_launch(bool prior, const double* coords, int64_t n, int dim, int m, const double* query, int64_t q0,
                         int64_t q1, int32_t* nbr, hipStream_t s);

}  // namespace nngp
