// Analytic gradient of the multivariate (LMC) NNGP log-likelihood in (A's lower triangle, phi_1..phi_q, tau2_1..tau2_q),
// one fused sweep: bf_mv.h's wavefront per location, tiles and factorisation, then three added steps.
//
// One location, joint block K of n = (m + 1) q rows (neighbours slot-major, the q target rows last), B = C_tN C_NN^-1,
// F = C_tt - B C_Nt = LF LF^T, r = y_t - B y_N, e = LF^-1 r, l_i = -1/2 log det F - 1/2 e^T e - (q / 2) log 2 pi.  With
//   a     = [C_NN^-1 y_N ; 0]                (row q of X after the back-substitution: value column 0 rides there)
//   g     = LF^-T e,   alpha = a + [-B^T g ; g]
//   Z     = LF^-1 [-B, I]                    (q rows)
// d l_i = 1/2 tr(S dK),  S = alpha alpha^T - a a^T - Z^T Z: q + 2 signed outer products of n-vectors, no inverse of the
// block and no second factorisation.  With rho_k = rho(phi_k d) and v_k = u rho'(u) at u = phi_k d over point pairs
// (s, s'), and S_ss' the q x q block of S:
//   d l_i / d A_ck   = sum_{s,s'} rho_k (S_ss' A)[c][k]                  (c >= k)
//   d l_i / d phi_k  = 1/2 sum_{s,s'} v_k A[:,k]^T S_ss' A[:,k] / phi_k
//   d l_i / d tau2_a = 1/2 sum_s S_ss[a][a]                              (all m + 1 points)
//
// Steps after bf_mv's forward part (build, left-looking factorisation on v_mfma_f64_16x16x4_f64, G = X X^T, the q x q
// tail, the back-substitution that leaves B in X rows 0..q-1 and a in row q):
//   1. adjoint vectors: lane l < n owns joint row l: its column of B (or -e_a for a target row), its entry of a; one
//      q-term dot for alpha and one q x q forward substitution for its column of Z.  The q + 2 vectors go to LDS over
//      the dead triangle tiles, the point table (kept in registers since the build) over the dead inverses: no LDS
//      beyond bf_mv's.
//   2. pair pass: the (m + 1)(m + 2) / 2 point pairs dealt over the lanes as in the build; per pair one distance, q
//      evaluations of (rho_k, v_k) (sep_rho_dv, bf_grad.h's brackets), the q x q block of S from the q + 2 vectors,
//      symmetrised (an off-diagonal pair stands for both orders), and straight into the lane's P running sums; no T_k
//      is stored.  A pair with a masked slot adds exactly 0.
//   3. reduction in a fixed order: the lanes' sums go to LDS (over the dead tiles) and P lanes each add the lanes'
//      entries in lane order.  The row's 4 + P numbers (the sweep's log det, quadratic form and two flags, then the
//      gradient terms) go to a record indexed by the LOCATION (not by the row of nbr), and the fold runs over the
//      records in location order (bf_mv_grad.hip): the sums are bit-identical run to run and whatever `order` is.
#pragma once
#include "bf_mv.h"
#include "bf_sep.h"

namespace nngp {

struct MvGradArgs {
    const double* coords;  // (n_points, dim)
    int64_t n_points;
    const int32_t* nbr;    // (n_rows, m), -1 padded
    const int32_t* order;  // or null
    int64_t n_rows, i0;
    int m, q, kind, dim;
    const double *A, *phi, *tau2;  // host: (q, q) row-major, (q,), (q,)
    const double* values;          // (n_points, q)
    double* G;                     // (n_rows, P) or null
    double* rows;                  // the workspace: (n_rows, 4 + P) row records, then the chunk records
};

struct MvGradParams {
    double g[3];             // rho'(u) = e(u) (g[0] + g[1] u + g[2] u^2)
    double hiphi[kMvMaxQ];   // 1 / (2 phi_k)
};

template <int Q, int NT>
__global__ __launch_bounds__(64 * kMvWaves) void bf_mv_grad(const double* __restrict__ coords, int64_t n_points,
                                                            const int32_t* __restrict__ nbr,
                                                            const int32_t* __restrict__ order, int64_t n_rows,
                                                            int64_t i0, int m, int dim, const MvParams P,
                                                            const MvGradParams Gp, const double* __restrict__ values,
                                                            double* __restrict__ Gout, double* __restrict__ rows) {
    constexpr int NTRI = NT * (NT + 1) / 2;
    constexpr int WAVE = (NTRI + 2 * NT) * kMvTe + kMvSmall;  // bf_mv's, to the byte
    constexpr int NTQ = Q * (Q + 1) / 2;
    constexpr int NP = mv_grad_len(Q);
    constexpr int REC = 4 + NP;
    constexpr int VS = 16 * NT + 4;  // stride of an adjoint vector: n <= 16 NT + Q
    // the lanes' sums fit the wavefront's tiles: at NT = 1 (m <= 16 / Q) fewer than 64 lanes own a pair
    constexpr int MAXM = NT == 1 ? 16 / Q : kMvMaxRows / Q - 1;
    constexpr int MAXL = (MAXM + 1) * (MAXM + 2) / 2 < 64 ? (MAXM + 1) * (MAXM + 2) / 2 : 64;
    static_assert(MAXL * NP <= WAVE && (Q + 2) * VS <= NTRI * kMvTe && 4 * 33 <= NT * kMvTe, "LDS reuse");
    __shared__ double etab[NNGP_EXP_TAB_N];
    __shared__ double lds[kMvWaves][WAVE];
    nngp_exp_table_load(etab, 1.0);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* Nt = lds[wv];            // the neighbours' lower triangle, tile (i, j) at mv_tri(i, j)
    double* Xt = Nt + NTRI * kMvTe;  // the target / value tile row
    double* It = Xt + NT * kMvTe;    // inverses of the diagonal tiles
    double* ctt = It + NT * kMvTe;   // C_tt, 4 x 4
    double* vt = ctt + 16;           // target values
    double* pts = It;                // build and pair pass: (m + 1) x {x, y, z, point index}

    const int64_t blk = xcd_logical_block(blockIdx.x, gridDim.x);
    const int64_t r = blk * kMvWaves + wv;
    const bool live = r < n_rows;
    const int64_t rl = live ? r : n_rows - 1;
    const int64_t rr = order != nullptr ? (int64_t)order[rl] : rl;
    const int64_t i = i0 + rr;
    const int mq = m * Q, n = mq + Q;

    // ---- the m + 1 points, one per lane (kept in registers for the pair pass); a slot without a point reads point 0
    // and is masked
    int32_t j = -1;
    if (lane < m) j = nbr[rl * m + lane];
    const bool in_range = j >= 0 && (int64_t)j < n_points;
    const bool bad_index = __any(lane < m && j != -1 && !in_range);
    const uint64_t vmask = __ballot(in_range || lane == m);
    double x[3] = {0.0, 0.0, 0.0};
    if (lane <= m) {
        load_point_rt(coords + (lane == m ? i : (in_range ? (int64_t)j : 0)) * dim, dim, x);
        pts[4 * lane] = x[0];
        pts[4 * lane + 1] = x[1];
        pts[4 * lane + 2] = x[2];
        pts[4 * lane + 3] = in_range ? (double)j : -1.0;
    }
    for (int e = lane; e < NT * kMvTe; e += 64) Xt[e] = 0.0;
    for (int e = lane; e < (16 * NT - mq) * 16 * NT; e += 64) {
        const int rw = mq + e / (16 * NT), cl = e % (16 * NT);
        if (cl <= rw) Nt[mv_tri(rw >> 4, cl >> 4) * kMvTe + (cl & 15) * kMvLd + (rw & 15)] = cl == rw ? P.dmin : 0.0;
    }
    mv_sync();

    // ---- the joint block, as bf_mv builds it (S = T: the nugget on every diagonal)
    const int npairs = (m + 1) * (m + 2) / 2;
    for (int p = lane; p < npairs; p += 64) {
        int a = (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
        while (a * (a + 1) / 2 > p) --a;
        while ((a + 1) * (a + 2) / 2 <= p) ++a;
        const int b = p - a * (a + 1) / 2;
        const double pa[3] = {pts[4 * a], pts[4 * a + 1], pts[4 * a + 2]};
        const double pb[3] = {pts[4 * b], pts[4 * b + 1], pts[4 * b + 2]};
        const bool ok = ((vmask >> a) & 1) != 0 && ((vmask >> b) & 1) != 0;
        const double d2 = point_d2<3>(pa, pb);
        double rho[Q];
#pragma unroll
        for (int k = 0; k < Q; ++k) rho[k] = a == b ? 1.0 : nngp_cov_d2<NNGP_KIND_GENERIC>(P.pc[k], etab, d2);
#pragma unroll
        for (int al = 0; al < Q; ++al) {
#pragma unroll
            for (int be = 0; be < Q; ++be) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k <= (al < be ? al : be); ++k) v = fma(P.A[al][k] * P.A[be][k], rho[k], v);
                if (a == b) {
                    if (be > al) continue;
                    v = al == be ? v + P.tau2[al] : (ok ? v : 0.0);
                    if (a < m) {
                        const int rw = a * Q + al, cl = a * Q + be;
                        Nt[mv_tri(rw >> 4, cl >> 4) * kMvTe + (cl & 15) * kMvLd + (rw & 15)] = v;
                    } else {
                        ctt[4 * al + be] = v;
                    }
                } else {
                    v = ok ? v : 0.0;
                    const int cl = b * Q + be;
                    if (a < m) {
                        const int rw = a * Q + al;
                        Nt[mv_tri(rw >> 4, cl >> 4) * kMvTe + (cl & 15) * kMvLd + (rw & 15)] = v;
                    } else {
                        Xt[(cl >> 4) * kMvTe + (cl & 15) * kMvLd + al] = v;
                    }
                }
            }
        }
    }
    // ---- the value column: the neighbours' into X row Q, the target's own into vt
    if (lane < mq) {
        const int slot = lane / Q, be = lane - slot * Q;
        const double jd = pts[4 * slot + 3];
        Xt[(lane >> 4) * kMvTe + (lane & 15) * kMvLd + Q] = jd >= 0.0 ? values[(int64_t)jd * Q + be] : 0.0;
    }
    if (lane < Q) vt[8 * lane] = values[i * Q + lane];
    mv_sync();

    // ---- factorise, left-looking over the tile columns; X is tile row NT
    bool bad = false;
#pragma nounroll
    for (int k = 0; k < NT; ++k) {
        double* Dk = Nt + mv_tri(k, k) * kMvTe;
        if (k > 0) {
            mv_d4 acc = mv_ld(Dk, lane);
            for (int jj = 0; jj < k; ++jj) {
                const double* L = Nt + mv_tri(k, jj) * kMvTe;
                acc = mv_mma_nt<true>(L, L, acc, lane);
            }
            mv_st(Dk, lane, acc);
            mv_sync();
        }
        bad |= mv_chol_inv(Dk, It + k * kMvTe, lane, P.pivmin);
        mv_d4 pa[NT];
        if (k > 0) {
#pragma unroll
            for (int ii = 0; ii < NT; ++ii) {
                const int t = ii + 1;
                if (t <= k) continue;
                double* Tk = t < NT ? Nt + mv_tri(t, k) * kMvTe : Xt + k * kMvTe;
                pa[ii] = mv_ld(Tk, lane);
                for (int jj = 0; jj < k; ++jj)
                    pa[ii] = mv_mma_nt<true>(t < NT ? Nt + mv_tri(t, jj) * kMvTe : Xt + jj * kMvTe,
                                             Nt + mv_tri(k, jj) * kMvTe, pa[ii], lane);
            }
#pragma unroll
            for (int ii = 0; ii < NT; ++ii) {
                const int t = ii + 1;
                if (t <= k) continue;
                mv_st(t < NT ? Nt + mv_tri(t, k) * kMvTe : Xt + k * kMvTe, lane, pa[ii]);
            }
            mv_sync();
        }
#pragma unroll
        for (int ii = 0; ii < NT; ++ii) {
            const int t = ii + 1;
            if (t <= k) continue;
            const double* Tk = t < NT ? Nt + mv_tri(t, k) * kMvTe : Xt + k * kMvTe;
            pa[ii] = mv_mma_nt<false>(Tk, It + k * kMvTe, mv_d4{0.0, 0.0, 0.0, 0.0}, lane);
        }
#pragma unroll
        for (int ii = 0; ii < NT; ++ii) {
            const int t = ii + 1;
            if (t <= k) continue;
            mv_st(t < NT ? Nt + mv_tri(t, k) * kMvTe : Xt + k * kMvTe, lane, pa[ii]);
        }
        mv_sync();
    }

    // ---- G = X X^T into the first diagonal tile
    double* Gt = Nt;
    {
        mv_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < NT; ++k) acc = mv_mma_nt<false>(Xt + k * kMvTe, Xt + k * kMvTe, acc, lane);
        mv_st(Gt, lane, acc);
        mv_sync();
    }

    // ---- the Q x Q tail, every lane the same: LF = chol(C_tt - W W^T), e = LF^-1 r, g = LF^-T e
    double LF[Q][Q];
    double lf = 0.0;
#pragma unroll
    for (int al = 0; al < Q; ++al) {
#pragma unroll
        for (int be = 0; be <= al; ++be) {
            double s = ctt[4 * al + be] - Gt[be * kMvLd + al];
#pragma unroll
            for (int k = 0; k < be; ++k) s = fma(-LF[al][k], LF[be][k], s);
            if (be < al) {
                LF[al][be] = s / LF[be][be];
            } else {
                bad |= !(s > P.pivmin);
                LF[al][al] = sqrt(s);
                lf += 2.0 * log(LF[al][al]);
            }
        }
    }
    double qq = 0.0, g[Q];
    {
        double e[Q];
#pragma unroll
        for (int al = 0; al < Q; ++al) {
            double s = vt[8 * al] - Gt[Q * kMvLd + al];
#pragma unroll
            for (int k = 0; k < al; ++k) s = fma(-LF[al][k], e[k], s);
            e[al] = s / LF[al][al];
            qq = fma(e[al], e[al], qq);
        }
#pragma unroll
        for (int al = Q - 1; al >= 0; --al) {
            double s = e[al];
#pragma unroll
            for (int k = al + 1; k < Q; ++k) s = fma(-LF[k][al], g[k], s);
            g[al] = s / LF[al][al];
        }
    }

    // ---- [B ; a] = X L_N^-1 by back-substitution over the tiles
#pragma nounroll
    for (int k = NT - 1; k >= 0; --k) {
        double* Xk = Xt + k * kMvTe;
        if (k < NT - 1) {
            mv_d4 acc = mv_ld(Xk, lane);
            for (int jj = k + 1; jj < NT; ++jj)
                acc = mv_mma_nn<true>(Xt + jj * kMvTe, Nt + mv_tri(jj, k) * kMvTe, acc, lane);
            mv_st(Xk, lane, acc);
            mv_sync();
        }
        const mv_d4 acc = mv_mma_nn<false>(Xk, It + k * kMvTe, mv_d4{0.0, 0.0, 0.0, 0.0}, lane);
        mv_st(Xk, lane, acc);
        mv_sync();
    }

    // ---- the adjoint vectors alpha, a, Z (a row of the joint block per lane) over the dead triangle tiles, the
    // point table over the dead inverses
    double* V = Nt;
    if (lane <= m) {
        pts[4 * lane] = x[0];
        pts[4 * lane + 1] = x[1];
        pts[4 * lane + 2] = x[2];
    }
    if (lane < n) {
        double b[Q], av = 0.0;
        if (lane < mq) {
            const double* col = Xt + (lane >> 4) * kMvTe + (lane & 15) * kMvLd;
            const bool valid = ((vmask >> (lane / Q)) & 1) != 0;
#pragma unroll
            for (int al = 0; al < Q; ++al) b[al] = valid ? col[al] : 0.0;
            av = valid ? col[Q] : 0.0;
        } else {
#pragma unroll
            for (int al = 0; al < Q; ++al) b[al] = al == lane - mq ? -1.0 : 0.0;
        }
        double alpha = av;
#pragma unroll
        for (int al = 0; al < Q; ++al) alpha = fma(-b[al], g[al], alpha);
        V[lane] = alpha;
        V[VS + lane] = av;
        double z[Q];
#pragma unroll
        for (int al = 0; al < Q; ++al) {
            double s = b[al];
#pragma unroll
            for (int k = 0; k < al; ++k) s = fma(-LF[al][k], z[k], s);
            z[al] = s / LF[al][al];
            V[(2 + al) * VS + lane] = z[al];  // -Z: the sign leaves Z^T Z alone
        }
    }
    mv_sync();

    // ---- the pair pass: an off-diagonal pair stands for both orders, w (S_ab + S_ab^T)
    double acc[NP];
#pragma unroll
    for (int t = 0; t < NP; ++t) acc[t] = 0.0;
    for (int p = lane; p < npairs; p += 64) {
        int a = (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
        while (a * (a + 1) / 2 > p) --a;
        while ((a + 1) * (a + 2) / 2 <= p) ++a;
        const int b = p - a * (a + 1) / 2;
        const double pa[3] = {pts[4 * a], pts[4 * a + 1], pts[4 * a + 2]};
        const double pb[3] = {pts[4 * b], pts[4 * b + 1], pts[4 * b + 2]};
        const bool ok = ((vmask >> a) & 1) != 0 && ((vmask >> b) & 1) != 0;
        const double d2 = point_d2<3>(pa, pb);
        double rho[Q], dv[Q];
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            sep_rho_dv(P.pc[k], Gp.g, etab, d2, rho[k], dv[k]);
            if (a == b) rho[k] = 1.0, dv[k] = 0.0;
        }
        double S[Q][Q];
#pragma unroll
        for (int al = 0; al < Q; ++al)
#pragma unroll
            for (int be = 0; be < Q; ++be) S[al][be] = 0.0;
#pragma unroll
        for (int v = 0; v < Q + 2; ++v) {
            double va[Q], vb[Q];
#pragma unroll
            for (int al = 0; al < Q; ++al) {
                va[al] = V[v * VS + a * Q + al];
                vb[al] = V[v * VS + b * Q + al];
            }
#pragma unroll
            for (int al = 0; al < Q; ++al)
#pragma unroll
                for (int be = 0; be < Q; ++be) S[al][be] = fma(v == 0 ? va[al] : -va[al], vb[be], S[al][be]);
        }
        const double w = !ok ? 0.0 : (a == b ? 0.5 : 1.0);
        double Y[Q][Q];
#pragma unroll
        for (int al = 0; al < Q; ++al)
#pragma unroll
            for (int be = 0; be <= al; ++be) Y[al][be] = Y[be][al] = w * (S[al][be] + S[be][al]);
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            double qk = 0.0;
#pragma unroll
            for (int c = k; c < Q; ++c) {
                double u = 0.0;
#pragma unroll
                for (int be = k; be < Q; ++be) u = fma(Y[c][be], P.A[be][k], u);
                acc[c * (c + 1) / 2 + k] = fma(rho[k], u, acc[c * (c + 1) / 2 + k]);
                qk = fma(P.A[c][k], u, qk);
            }
            acc[NTQ + k] = fma(dv[k], qk, acc[NTQ + k]);
        }
        if (a == b) {
#pragma unroll
            for (int al = 0; al < Q; ++al) acc[NTQ + Q + al] += Y[al][al];
        }
    }
    mv_sync();

    // ---- the lanes' sums, added in lane order by NP lanes
    double* red = Nt;
    const int nl = npairs < 64 ? npairs : 64;
    if (lane < nl) {
#pragma unroll
        for (int t = 0; t < NP; ++t) red[lane * NP + t] = acc[t];
    }
    mv_sync();
    if (lane < NP) {
        double s = 0.0;
        for (int l = 0; l < nl; ++l) s += red[l * NP + lane];
        double scale = lane < NTQ ? 1.0 : 0.5;
#pragma unroll
        for (int k = 0; k < Q; ++k)
            if (lane == NTQ + k) scale = Gp.hiphi[k];
        s = bad ? NAN : s * scale;
        if (live) {
            rows[rr * REC + 4 + lane] = s;
            if (Gout != nullptr) Gout[rr * NP + lane] = s;
        }
    }
    if (live && lane == 0) {
        double* o = rows + rr * REC;
        o[0] = lf;
        o[1] = qq;
        o[2] = bad ? (double)i : INFINITY;
        o[3] = bad_index ? (double)i : INFINITY;
    }
}

template <int Q, int NT>
static bool launch_mv_grad_if(const MvGradArgs& a, hipStream_t s) {
    if (a.q != Q || mv_tiles(a.m, a.q) != NT) return false;
    const MvParams P = mv_params(a.q, a.kind, a.A, a.phi, a.tau2);
    const GradParams gp = grad_params(a.kind, 1.0, 0.0);
    MvGradParams Gp;
    for (int k = 0; k < 3; ++k) Gp.g[k] = gp.g[k];
    for (int k = 0; k < kMvMaxQ; ++k) Gp.hiphi[k] = k < Q ? 0.5 / a.phi[k] : 0.0;
    hipLaunchKernelGGL((bf_mv_grad<Q, NT>), dim3((unsigned)mv_blocks(a.n_rows)), dim3(64 * kMvWaves), 0, s, a.coords,
                       a.n_points, a.nbr, a.order, a.n_rows, a.i0, a.m, a.dim, P, Gp, a.values, a.G, a.rows);
    return true;
}

// the instantiation units (bf_mv_grad_q*.hip) and the dispatch + fold (bf_mv_grad.hip)
bool bf_mv_grad_launch_q2(const MvGradArgs& a, hipStream_t s);
bool bf_mv_grad_launch_q3(const MvGradArgs& a, hipStream_t s);
bool bf_mv_grad_launch_q4(const MvGradArgs& a, hipStream_t s);
hipError_t bf_mv_grad_launch(const MvGradArgs& a, double* partials, double* grad, hipStream_t s);

}  // namespace nngp
