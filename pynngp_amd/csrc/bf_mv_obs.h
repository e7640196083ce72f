// Multivariate NNGP (bf_mv.h's model) with outcomes missing at some sites: obs[p] has bit a set iff outcome a is observed
// at point p, and only observed (point, outcome) rows enter a location's joint block.  One wavefront per location, four
// per block, bf_mv's 16 x 16 tiles (stride 17), MFMA products and diagonal-tile Cholesky; what differs:
//
// Packed rows.  Lane s <= m gathers point s and its mask.  An inclusive scan of the popcounts over the lanes gives
// slot s its first packed row off[s]; row (s, a) sits at off[s] + popcount(mask_s & ((1 << a) - 1)), and
// n_N = off[m] is the number of conditioning rows.  (off, mask) of every slot go to LDS as one int next to the small
// tables: the pair build and the store of B read them by slot.
//
// Tile count per location.  nt = ceil(n_N / 16) is wave-uniform; the factorisation, the panel, G = X X^T and the
// back-substitution run to nt.  NTMAX sizes LDS and the unrolled register arrays only.  Rows n_N .. 16 nt - 1 are
// decoupled diagonal rows carrying dmin.  nt = 0 (no observed neighbour row) skips all of it: F = C_tt.
//
// A location whose slots hold more than 16 NTMAX rows keeps the longest prefix of slots that fits, masks the rest like
// slots without a point and is reported like a bad index (partials[3]): nothing is written outside its LDS region.
//
// Target.  Its rows stay unpacked in X rows 0..Q-1 (value columns in rows Q..), as in bf_mv.  In the S = T form an
// outcome that is not observed at the target has a zero row in X, zeros in its row and column of LF, a zero row of E and
// B, and adds no log term and no quadratic term; the tail's Cholesky runs over the observed outcomes, every lane the
// same.  The cross form computes every target outcome.
//
// Outputs keep bf_mv's shapes: B (n_rows, q, m q) slot-major, scattered from the packed columns on the store and
// exactly 0 where a row is not observed; LF (n_rows, q, q); E (n_rows, q, c).  Entries of `values` under a clear bit
// are never loaded.
//
// Records.  Each location writes its own 4-double record at its *location* index (bf_mv_grad.h's reasoning: a per-block
// record sums four nbr rows that another `order` deals to other blocks), and bf_finalize folds them in its fixed order:
// the partials are bit-identical run to run and whatever `order` is.  No block barrier after the table load.
#pragma once
#include "bf_mv.h"
#include "mv_obs_host.h"

namespace nngp {

constexpr int kMvObsSmall = kMvSmall + 32;  // bf_mv's C_tt and target values, and 64 ints (off | mask << 8) per slot

struct MvObsArgs {
    MvArgs a;            // rec: 4 doubles per location
    const uint8_t* obs;  // (n_points,)
    int rows_max;
};

// first packed row of outcome `al` of a slot with first row `off` and mask `mk`
__device__ __forceinline__ int mv_obs_row(int off, int mk, int al) { return off + __popc(mk & ((1 << al) - 1)); }

template <int Q, int NTMAX>
__global__ __launch_bounds__(64 * kMvWaves) void bf_mv_obs(
    const double* __restrict__ coords, int64_t n_points, const int32_t* __restrict__ nbr,
    const int32_t* __restrict__ order, const uint8_t* __restrict__ obs, int64_t n_rows, int64_t i0, int m, int dim,
    const MvParams P, const double* __restrict__ values, const double* __restrict__ qcoords,
    const double* __restrict__ qvalues, int c, int cross, int target_noise, double* __restrict__ Bout,
    double* __restrict__ LFout, double* __restrict__ Eout, double* __restrict__ rec) {
    constexpr int NTRI = NTMAX * (NTMAX + 1) / 2;
    constexpr int WAVE = (NTRI + 2 * NTMAX) * kMvTe + kMvObsSmall;
    constexpr int CAP = 16 * NTMAX, FULL = (1 << Q) - 1;
    __shared__ double etab[NNGP_EXP_TAB_N];
    __shared__ double lds[kMvWaves][WAVE];
    nngp_exp_table_load(etab, 1.0);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* Nt = lds[wv];              // the neighbours' lower triangle, tile (i, j) at mv_tri(i, j)
    double* Xt = Nt + NTRI * kMvTe;    // the target / value tile row
    double* It = Xt + NTMAX * kMvTe;   // inverses of the diagonal tiles
    double* ctt = It + NTMAX * kMvTe;  // C_tt, 4 x 4
    double* vt = ctt + 16;             // target values, 4 x 8
    int* pk = (int*)(vt + 32);         // slot s: off[s] | mask_s << 8; slot m: n_N | the target's mask << 8
    double* pts = It;                  // build only: (m + 1) x {x, y, z, point index}

    const int64_t blk = xcd_logical_block(blockIdx.x, gridDim.x);
    const int64_t r = blk * kMvWaves + wv;
    if (r >= n_rows) return;  // no block barrier below
    const int64_t rr = order != nullptr ? (int64_t)order[r] : r;
    const int64_t i = i0 + rr;
    const int mq = m * Q;

    // ---- the m + 1 points and the neighbours' masks, one per lane; the packed offsets by a scan over the lanes
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
    const int tmask = __builtin_amdgcn_readfirstlane(cross ? FULL : (int)obs[i] & FULL);
    if (lane <= m) {
        double x[3];
        load_point_rt(lane == m ? qcoords + i * dim : coords + (in_range ? (int64_t)j * dim : 0), dim, x);
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

    // ---- the (m + 1)(m + 2) / 2 point pairs a >= b, dealt over the lanes: one distance, Q correlations, and the
    // entries of the Q x Q block whose two rows are observed, to their packed positions
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
                    const bool noise = a < m || !cross || target_noise;
                    if (al == be && noise) v += P.tau2[al];
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
    // ---- the value columns: the neighbours' observed entries into X rows Q.., the target's own into vt
    if (values != nullptr) {
        for (int e = lane; e < mq * c; e += 64) {
            const int s = e / c, col = e - s * c;
            const int slot = s / Q, be = s - slot * Q;
            const int ks = pk[slot];
            if (((ks >> (8 + be)) & 1) == 0) continue;
            const int cl = mv_obs_row(ks & 255, ks >> 8, be);
            Xt[(cl >> 4) * kMvTe + (cl & 15) * kMvLd + Q + col] = values[((int64_t)pts[4 * slot + 3] * Q + be) * c + col];
        }
    }
    if (lane < Q * c) {
        const int al = lane / c, col = lane - al * c;
        vt[8 * al + col] = qvalues != nullptr && ((tmask >> al) & 1) != 0 ? qvalues[(i * Q + al) * c + col] : 0.0;
    }
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

    // ---- the Q x Q tail over the observed target outcomes, every lane the same: LF = chol(C_tt - W W^T); an outcome
    // that is not observed keeps a zero row and column, which drop out of every sum below
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
    // lane col: E[:, col] = LF^-1 (V_t[:, col] - (W z_N)[:, col]), or the conditional mean itself
    double qq = 0.0;
    if (lane < c) {
        double e[Q];
#pragma unroll
        for (int al = 0; al < Q; ++al) {
            const double mean = Gt[(Q + lane) * kMvLd + al];
            double s = vt[8 * al + lane] - mean;
#pragma unroll
            for (int k = 0; k < al; ++k) s = fma(-LF[al][k], e[k], s);
            e[al] = ((tmask >> al) & 1) != 0 ? s / LF[al][al] : 0.0;
            qq = fma(e[al], e[al], qq);
            if (Eout != nullptr) Eout[(rr * Q + al) * c + lane] = bad ? NAN : (cross ? mean : e[al]);
        }
    }
    if (LFout != nullptr) {
#pragma unroll
        for (int al = 0; al < Q; ++al)
#pragma unroll
            for (int be = 0; be < Q; ++be)
                if (lane == al * Q + be) LFout[(rr * Q + al) * Q + be] = bad ? NAN : (be <= al ? LF[al][be] : 0.0);
    }

    // ---- B = W L_N^-1 by back-substitution over the nt tiles, scattered from the packed columns to slot-major
    if (Bout != nullptr) {
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
        for (int e = lane; e < Q * mq; e += 64) {
            const int al = e / mq, s = e - al * mq;
            const int slot = s / Q, be = s - slot * Q;
            const int ks = pk[slot];
            double v = 0.0;
            if (((ks >> (8 + be)) & (tmask >> al) & 1) != 0) {
                const int cl = mv_obs_row(ks & 255, ks >> 8, be);
                v = Xt[(cl >> 4) * kMvTe + (cl & 15) * kMvLd + al];
            }
            Bout[rr * (int64_t)(Q * mq) + e] = bad ? NAN : v;
        }
    }

    if (lane == 0) {
        double* o = rec + 4 * rr;
        o[0] = lf;
        o[1] = cross ? 0.0 : qq;
        o[2] = bad ? (double)i : INFINITY;
        o[3] = bad_index ? (double)i : INFINITY;
    }
}

template <int Q, int NTMAX>
static bool launch_mv_obs_if(const MvObsArgs& o, hipStream_t s) {
    const MvArgs& a = o.a;
    if (a.q != Q || mv_obs_tiles(o.rows_max) != NTMAX) return false;
    const MvParams P = mv_params(Q, a.kind, a.A, a.phi, a.tau2);
    hipLaunchKernelGGL((bf_mv_obs<Q, NTMAX>), dim3((unsigned)mv_blocks(a.n_rows)), dim3(64 * kMvWaves), 0, s, a.coords,
                       a.n_points, a.nbr, a.order, o.obs, a.n_rows, a.i0, a.m, a.dim, P, a.values, a.qcoords,
                       a.qvalues, a.c, a.cross, a.target_noise, a.B, a.LF, a.E, a.rec);
    return true;
}

// the instantiation units (bf_mv_obs_q*.hip) and the dispatch + fold (bf_mv_obs.hip)
bool bf_mv_obs_launch_q2(const MvObsArgs& a, hipStream_t s);
bool bf_mv_obs_launch_q3(const MvObsArgs& a, hipStream_t s);
bool bf_mv_obs_launch_q4(const MvObsArgs& a, hipStream_t s);
hipError_t bf_mv_obs_launch(const MvObsArgs& a, double* partials, hipStream_t s);

}  // namespace nngp
