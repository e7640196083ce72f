// Analytic gradient of the multivariate (LMC) NNGP log-likelihood with outcomes missing at some sites, in (A's lower
// triangle row-major, phi_1..phi_q, tau2_1..tau2_q), one fused sweep, S = T form: bf_mv_obs.h's packed-row forward part
// (c = 1, B always computed), then bf_mv_grad.h's three steps restated on the packed rows.
//
// One location, joint block K over its observed rows only: the n_N packed neighbour rows, then the observed target
// outcomes.  bf_mv_grad.h's identity holds on that block unchanged,
//   d l_i = 1/2 tr(S dK),  S = alpha alpha^T - a a^T - Z^T Z,
//   a = [C_NN^-1 y_N ; 0],  g = LF^-T e,  alpha = a + [-B^T g ; g],  Z = LF^-1 [-B, I],
// because a row that is not observed is in neither K nor S.  The kernel keeps the target unpacked (Q rows of X, Q x Q
// LF with a zero row and column per outcome that is not observed, bf_mv_obs.h), so e, g and the target's column of Z
// are exactly 0 there: the divisions by LF[al][al] = 0 are guarded by the scalar target mask, as the tail's are.
//
// Steps after the forward part (which leaves B in X rows 0..Q-1 and a in row Q, both in packed columns):
//   1. adjoint vectors: lane l < n_N owns packed row l (its column of B, its entry of a); the observed target rows
//      follow at n_N.., packed like a slot's (mv_obs_row(n_N, target mask, al)), written by lanes 0..Q-1 in a second
//      step: n_N + Q reaches 68 rows, more than the wavefront has lanes.  The Q + 2 vectors go over the dead triangle
//      tiles, the point table (coordinates kept in registers since the build) over the dead inverses; pk[] stays: no
//      LDS beyond bf_mv_obs's.
//   2. pair pass over the (m + 1)(m + 2) / 2 point pairs, dealt over the lanes as in the build: a pair with a point
//      that has no observed row is skipped before its distance; otherwise one distance, Q evaluations of (rho_k,
//      u rho'(u)) (sep_rho_dv), the Q x Q block of S from the vectors read through mv_obs_row, an outcome that is not
//      observed contributing a 0 operand (its entries of S vanish, the tau2_a term sums observed rows only), and the
//      lane's P running sums.  No T_k is stored.
//   3. reduction: a fixed xor-butterfly over the 64 lanes per sum, in registers.  bf_mv_grad's LDS region would not
//      do: at NTMAX = 1 a location with many empty neighbour sites still has up to 64 lanes with pairs, and 64 x 18
//      sums exceed the wavefront's LDS slice.  The butterfly relies on no fit and is the same whatever `order` is.
//
// Records as bf_mv_grad.h: 4 + P doubles per location at the location index, folded by bf_mv_grad.hip's kernels in
// location order, so the sums are bit-identical run to run and for any `order`.
//
// By construction: nt = 0 (no observed neighbour row) leaves the target rows alone in the block, the gradient flows
// through C_tt; a target with nothing observed writes a zero record; a location over 16 NTMAX rows keeps the longest
// prefix of slots (the others have mask 0 in pk[] and are skipped like empty sites) and is flagged in partials[3]; a
// failed pivot makes the row's P terms NaN and is flagged in partials[2].
#pragma once
#include "bf_mv_grad.h"
#include "bf_mv_obs.h"

namespace nngp {

struct MvObsGradArgs {
    MvGradArgs g;        // rows: (n_rows, 4 + P) row records, then the chunk records
    const uint8_t* obs;  // (n_points,)
    int rows_max;
};

// one row of the joint block into the Q + 2 vectors at index idx: b its column of [B ; -I] (zeros where the target
// outcome is not observed), av its entry of a
template <int Q>
__device__ __forceinline__ void mv_obs_adjoint(double* V, int VS, int idx, const double (&b)[Q], double av,
                                               const double (&g)[Q], const double (&LF)[Q][Q], int tmask) {
    double alpha = av;
#pragma unroll
    for (int al = 0; al < Q; ++al) alpha = fma(-b[al], g[al], alpha);
    V[idx] = alpha;
    V[VS + idx] = av;
    double z[Q];
#pragma unroll
    for (int al = 0; al < Q; ++al) {
        double s = b[al];
#pragma unroll
        for (int k = 0; k < al; ++k) s = fma(-LF[al][k], z[k], s);
        z[al] = ((tmask >> al) & 1) != 0 ? s / LF[al][al] : 0.0;
        V[(2 + al) * VS + idx] = z[al];  // -Z: the sign leaves Z^T Z alone
    }
}

template <int Q, int NTMAX>
__global__ __launch_bounds__(64 * kMvWaves) void bf_mv_obs_grad(
    const double* __restrict__ coords, int64_t n_points, const int32_t* __restrict__ nbr,
    const int32_t* __restrict__ order, const uint8_t* __restrict__ obs, int64_t n_rows, int64_t i0, int m, int dim,
    const MvParams P, const MvGradParams Gp, const double* __restrict__ values, double* __restrict__ Gout,
    double* __restrict__ rows) {
    constexpr int NTRI = NTMAX * (NTMAX + 1) / 2;
    constexpr int WAVE = (NTRI + 2 * NTMAX) * kMvTe + kMvObsSmall;  // bf_mv_obs's, to the byte
    constexpr int CAP = 16 * NTMAX, FULL = (1 << Q) - 1;
    constexpr int NTQ = Q * (Q + 1) / 2;
    constexpr int NP = mv_grad_len(Q);
    constexpr int REC = 4 + NP;
    constexpr int VS = CAP + 4;  // stride of an adjoint vector: n_N + Q <= 16 NTMAX + Q rows
    static_assert((Q + 2) * VS <= NTRI * kMvTe && 4 * (kMvObsMaxM + 1) <= NTMAX * kMvTe && Q <= 4, "LDS reuse");
    __shared__ double etab[NNGP_EXP_TAB_N];
    __shared__ double lds[kMvWaves][WAVE];
    nngp_exp_table_load(etab, 1.0);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* Nt = lds[wv];              // the neighbours' lower triangle, tile (i, j) at mv_tri(i, j)
    double* Xt = Nt + NTRI * kMvTe;    // the target / value tile row
    double* It = Xt + NTMAX * kMvTe;   // inverses of the diagonal tiles
    double* ctt = It + NTMAX * kMvTe;  // C_tt, 4 x 4
    double* vt = ctt + 16;             // target values
    int* pk = (int*)(vt + 32);         // slot s: off[s] | mask_s << 8; slot m: n_N | the target's mask << 8
    double* pts = It;                  // build and pair pass: (m + 1) x {x, y, z, point index}

    const int64_t blk = xcd_logical_block(blockIdx.x, gridDim.x);
    const int64_t r = blk * kMvWaves + wv;
    if (r >= n_rows) return;  // no block barrier below
    const int64_t rr = order != nullptr ? (int64_t)order[r] : r;
    const int64_t i = i0 + rr;

    // ---- the m + 1 points (kept in registers for the pair pass) and the neighbours' masks, one per lane; the packed
    // offsets by a scan over the lanes
    int32_t j = -1;
    if (lane < m) j = nbr[r * m + lane];
    const bool in_range = j >= 0 && (int64_t)j < n_points;
    int mk = in_range ? (int)obs[j] & FULL : 0;
    const int cnt = __popc(mk);
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    // the slots that fit are a prefix (incl grows with the lane); the others are masked and flagged
    const bool keep = incl <= CAP;
    const bool bad_index = __any(lane < m && ((j != -1 && !in_range) || (!keep && cnt > 0)));
    if (!keep) mk = 0;
    const int kept = __popcll(__ballot(lane < m && keep));
    const int nN = kept > 0 ? __builtin_amdgcn_readlane(incl, kept - 1) : 0;
    const int nt = (nN + 15) >> 4;
    const int tmask = __builtin_amdgcn_readfirstlane((int)obs[i] & FULL);
    double x[3] = {0.0, 0.0, 0.0};
    if (lane <= m) {
        load_point_rt(coords + (lane == m ? i : (in_range ? (int64_t)j : 0)) * dim, dim, x);
        pts[4 * lane] = x[0];
        pts[4 * lane + 1] = x[1];
        pts[4 * lane + 2] = x[2];
        pts[4 * lane + 3] = in_range ? (double)j : -1.0;
        pk[lane] = lane == m ? (nN | tmask << 8) : ((keep ? incl - cnt : 0) | mk << 8);
    }
    // X starts as zeros; the rows of N from n_N to 16 nt are decoupled (diagonal) rows
    for (int e = lane; e < nt * kMvTe; e += 64) Xt[e] = 0.0;
    for (int e = lane; e < (16 * nt - nN) * 16 * nt; e += 64) {
        const int rw = nN + e / (16 * nt), cl = e % (16 * nt);
        if (cl <= rw) Nt[mv_tri(rw >> 4, cl >> 4) * kMvTe + (cl & 15) * kMvLd + (rw & 15)] = cl == rw ? P.dmin : 0.0;
    }
    mv_sync();

    // ---- the joint block, as bf_mv_obs builds it (S = T: the nugget on every diagonal): the entries of a pair's Q x Q
    // block whose two rows are observed, to their packed positions
    const int npairs = (m + 1) * (m + 2) / 2;
    for (int p = lane; p < npairs; p += 64) {
        int a = (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
        while (a * (a + 1) / 2 > p) --a;
        while ((a + 1) * (a + 2) / 2 <= p) ++a;
        const int b = p - a * (a + 1) / 2;
        const int ka = pk[a], kb = pk[b];
        const int oa = ka & 255, ma = ka >> 8, ob = kb & 255, mb = kb >> 8;
        if (a != b ? (ma == 0 || mb == 0) : (a < m && ma == 0)) continue;  // no row here (C_tt is always built)
        const double pa[3] = {pts[4 * a], pts[4 * a + 1], pts[4 * a + 2]};
        const double pb[3] = {pts[4 * b], pts[4 * b + 1], pts[4 * b + 2]};
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
                    if (al == be) v += P.tau2[al];
                    if (a == m) {
                        ctt[4 * al + be] = v;
                    } else if (((ma >> al) & (ma >> be) & 1) != 0) {
                        const int rw = mv_obs_row(oa, ma, al), cl = mv_obs_row(oa, ma, be);
                        Nt[mv_tri(rw >> 4, cl >> 4) * kMvTe + (cl & 15) * kMvLd + (rw & 15)] = v;
                    }
                } else if (((ma >> al) & (mb >> be) & 1) != 0) {
                    const int cl = mv_obs_row(ob, mb, be);
                    if (a < m) {
                        const int rw = mv_obs_row(oa, ma, al);
                        Nt[mv_tri(rw >> 4, cl >> 4) * kMvTe + (cl & 15) * kMvLd + (rw & 15)] = v;
                    } else {
                        Xt[(cl >> 4) * kMvTe + (cl & 15) * kMvLd + al] = v;
                    }
                }
            }
        }
    }
    // ---- the value column: the neighbours' observed entries into X row Q, the target's own into vt
    for (int e = lane; e < m * Q; e += 64) {
        const int slot = e / Q, be = e - slot * Q;
        const int ks = pk[slot];
        if (((ks >> (8 + be)) & 1) == 0) continue;
        const int cl = mv_obs_row(ks & 255, ks >> 8, be);
        Xt[(cl >> 4) * kMvTe + (cl & 15) * kMvLd + Q] = values[(int64_t)pts[4 * slot + 3] * Q + be];
    }
    if (lane < Q) vt[8 * lane] = ((tmask >> lane) & 1) != 0 ? values[i * Q + lane] : 0.0;
    mv_sync();

    // ---- factorise, left-looking over the nt tile columns; X is tile row nt
    bool bad = false;
#pragma nounroll
    for (int k = 0; k < nt; ++k) {
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
        mv_d4 pa[NTMAX];
        if (k > 0) {
#pragma unroll
            for (int ii = 0; ii < NTMAX; ++ii) {
                const int t = ii + 1;
                if (t <= k || t > nt) continue;
                double* Tk = t < nt ? Nt + mv_tri(t, k) * kMvTe : Xt + k * kMvTe;
                pa[ii] = mv_ld(Tk, lane);
                for (int jj = 0; jj < k; ++jj)
                    pa[ii] = mv_mma_nt<true>(t < nt ? Nt + mv_tri(t, jj) * kMvTe : Xt + jj * kMvTe,
                                             Nt + mv_tri(k, jj) * kMvTe, pa[ii], lane);
            }
#pragma unroll
            for (int ii = 0; ii < NTMAX; ++ii) {
                const int t = ii + 1;
                if (t <= k || t > nt) continue;
                mv_st(t < nt ? Nt + mv_tri(t, k) * kMvTe : Xt + k * kMvTe, lane, pa[ii]);
            }
            mv_sync();
        }
#pragma unroll
        for (int ii = 0; ii < NTMAX; ++ii) {
            const int t = ii + 1;
            if (t <= k || t > nt) continue;
            const double* Tk = t < nt ? Nt + mv_tri(t, k) * kMvTe : Xt + k * kMvTe;
            pa[ii] = mv_mma_nt<false>(Tk, It + k * kMvTe, mv_d4{0.0, 0.0, 0.0, 0.0}, lane);
        }
#pragma unroll
        for (int ii = 0; ii < NTMAX; ++ii) {
            const int t = ii + 1;
            if (t <= k || t > nt) continue;
            mv_st(t < nt ? Nt + mv_tri(t, k) * kMvTe : Xt + k * kMvTe, lane, pa[ii]);
        }
        mv_sync();
    }

    // ---- G = X X^T into the first diagonal tile (zeros for nt = 0)
    double* Gt = Nt;
    {
        mv_d4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < nt; ++k) acc = mv_mma_nt<false>(Xt + k * kMvTe, Xt + k * kMvTe, acc, lane);
        mv_st(Gt, lane, acc);
        mv_sync();
    }

    // ---- the Q x Q tail over the observed target outcomes, every lane the same: LF = chol(C_tt - W W^T),
    // e = LF^-1 r, g = LF^-T e; an outcome that is not observed keeps zeros in LF, e and g
    double LF[Q][Q];
    double lf = 0.0;
#pragma unroll
    for (int al = 0; al < Q; ++al) {
        const bool ta = ((tmask >> al) & 1) != 0;
#pragma unroll
        for (int be = 0; be <= al; ++be) {
            double s = ctt[4 * al + be] - Gt[be * kMvLd + al];
#pragma unroll
            for (int k = 0; k < be; ++k) s = fma(-LF[al][k], LF[be][k], s);
            if (be < al) {
                LF[al][be] = ta && ((tmask >> be) & 1) != 0 ? s / LF[be][be] : 0.0;
            } else if (ta) {
                bad |= !(s > P.pivmin);
                LF[al][al] = sqrt(s);
                lf += 2.0 * log(LF[al][al]);
            } else {
                LF[al][al] = 0.0;
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
            e[al] = ((tmask >> al) & 1) != 0 ? s / LF[al][al] : 0.0;
            qq = fma(e[al], e[al], qq);
        }
#pragma unroll
        for (int al = Q - 1; al >= 0; --al) {
            double s = e[al];
#pragma unroll
            for (int k = al + 1; k < Q; ++k) s = fma(-LF[k][al], g[k], s);
            g[al] = ((tmask >> al) & 1) != 0 ? s / LF[al][al] : 0.0;
        }
    }

    // ---- [B ; a] = X L_N^-1 by back-substitution over the nt tiles, left in the packed columns
#pragma nounroll
    for (int k = nt - 1; k >= 0; --k) {
        double* Xk = Xt + k * kMvTe;
        if (k < nt - 1) {
            mv_d4 acc = mv_ld(Xk, lane);
            for (int jj = k + 1; jj < nt; ++jj)
                acc = mv_mma_nn<true>(Xt + jj * kMvTe, Nt + mv_tri(jj, k) * kMvTe, acc, lane);
            mv_st(Xk, lane, acc);
            mv_sync();
        }
        const mv_d4 acc = mv_mma_nn<false>(Xk, It + k * kMvTe, mv_d4{0.0, 0.0, 0.0, 0.0}, lane);
        mv_st(Xk, lane, acc);
        mv_sync();
    }

    // ---- the adjoint vectors alpha, a, Z over the dead triangle tiles: a packed neighbour row per lane, then the
    // observed target rows by lanes 0..Q-1; the point table over the dead inverses
    double* V = Nt;
    mv_sync();  // nt = 0: nothing since the tail's reads of G
    if (lane <= m) {
        pts[4 * lane] = x[0];
        pts[4 * lane + 1] = x[1];
        pts[4 * lane + 2] = x[2];
    }
    if (lane < nN) {
        const double* col = Xt + (lane >> 4) * kMvTe + (lane & 15) * kMvLd;
        double b[Q];
#pragma unroll
        for (int al = 0; al < Q; ++al) b[al] = col[al];
        mv_obs_adjoint<Q>(V, VS, lane, b, col[Q], g, LF, tmask);
    }
    if (lane < Q && ((tmask >> lane) & 1) != 0) {
        double b[Q];
#pragma unroll
        for (int al = 0; al < Q; ++al) b[al] = al == lane ? -1.0 : 0.0;
        mv_obs_adjoint<Q>(V, VS, mv_obs_row(nN, tmask, lane), b, 0.0, g, LF, tmask);
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
        const int ka = pk[a], kb = pk[b];
        const int oa = ka & 255, ma = ka >> 8, ob = kb & 255, mb = kb >> 8;
        if (ma == 0 || mb == 0) continue;  // a point without an observed row
        const double pa[3] = {pts[4 * a], pts[4 * a + 1], pts[4 * a + 2]};
        const double pb[3] = {pts[4 * b], pts[4 * b + 1], pts[4 * b + 2]};
        const double d2 = point_d2<3>(pa, pb);
        double rho[Q], dv[Q];
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            sep_rho_dv(P.pc[k], Gp.g, etab, d2, rho[k], dv[k]);
            if (a == b) rho[k] = 1.0, dv[k] = 0.0;
        }
        int ia[Q], ib[Q];
#pragma unroll
        for (int al = 0; al < Q; ++al) {
            ia[al] = mv_obs_row(oa, ma, al);
            ib[al] = mv_obs_row(ob, mb, al);
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
                va[al] = ((ma >> al) & 1) != 0 ? V[v * VS + ia[al]] : 0.0;
                vb[al] = ((mb >> al) & 1) != 0 ? V[v * VS + ib[al]] : 0.0;
            }
#pragma unroll
            for (int al = 0; al < Q; ++al)
#pragma unroll
                for (int be = 0; be < Q; ++be) S[al][be] = fma(v == 0 ? va[al] : -va[al], vb[be], S[al][be]);
        }
        const double w = a == b ? 0.5 : 1.0;
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

    // ---- the lanes' sums by a fixed butterfly; lane t writes sum t
    double mine = 0.0;
#pragma unroll
    for (int t = 0; t < NP; ++t) {
        const double s = wave_sum(acc[t]);
        if (lane == t) mine = s;
    }
    if (lane < NP) {
        double scale = lane < NTQ ? 1.0 : 0.5;
#pragma unroll
        for (int k = 0; k < Q; ++k)
            if (lane == NTQ + k) scale = Gp.hiphi[k];
        mine = bad ? NAN : mine * scale;
        rows[rr * REC + 4 + lane] = mine;
        if (Gout != nullptr) Gout[rr * NP + lane] = mine;
    }
    if (lane == 0) {
        double* o = rows + rr * REC;
        o[0] = lf;
        o[1] = qq;
        o[2] = bad ? (double)i : INFINITY;
        o[3] = bad_index ? (double)i : INFINITY;
    }
}

template <int Q, int NTMAX>
static bool launch_mv_obs_grad_if(const MvObsGradArgs& o, hipStream_t s) {
    const MvGradArgs& a = o.g;
    if (a.q != Q || mv_obs_tiles(o.rows_max) != NTMAX) return false;
    const MvParams P = mv_params(Q, a.kind, a.A, a.phi, a.tau2);
    const GradParams gp = grad_params(a.kind, 1.0, 0.0);
    MvGradParams Gp;
    for (int k = 0; k < 3; ++k) Gp.g[k] = gp.g[k];
    for (int k = 0; k < kMvMaxQ; ++k) Gp.hiphi[k] = k < Q ? 0.5 / a.phi[k] : 0.0;
    hipLaunchKernelGGL((bf_mv_obs_grad<Q, NTMAX>), dim3((unsigned)mv_blocks(a.n_rows)), dim3(64 * kMvWaves), 0, s,
                       a.coords, a.n_points, a.nbr, a.order, o.obs, a.n_rows, a.i0, a.m, a.dim, P, Gp, a.values, a.G,
                       a.rows);
    return true;
}

// bf_mv_grad.hip's fixed-order folds of the per-location records (chunks of kMvGradChunk locations, then the chunks)
__global__ void bf_mv_grad_chunks(const double* __restrict__ rows, int64_t n_rows, int nrec, double* __restrict__ crec);
__global__ void bf_mv_grad_finalize(const double* __restrict__ crec, int64_t n_chunks, int nrec,
                                    double* __restrict__ partials, double* __restrict__ grad);

// the instantiation units (bf_mv_obs_grad_q*.hip) and the dispatch + fold (bf_mv_obs_grad.hip)
bool bf_mv_obs_grad_launch_q2(const MvObsGradArgs& a, hipStream_t s);
bool bf_mv_obs_grad_launch_q3(const MvObsGradArgs& a, hipStream_t s);
bool bf_mv_obs_grad_launch_q4(const MvObsGradArgs& a, hipStream_t s);
hipError_t bf_mv_obs_grad_launch(const MvObsGradArgs& a, double* partials, double* grad, hipStream_t s);

}  // namespace nngp
