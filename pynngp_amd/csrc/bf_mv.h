// Multivariate NNGP under the linear model of coregionalisation: q outcomes (2..4) at every location,
//   Cov(y_a(s), y_b(s')) = sum_k A_ak A_bk rho(phi_k |s - s'|) + tau2_a delta_ab delta_ss',
// A lower-triangular, rho exponential, Matern-3/2, Matern-5/2 or Gaussian.  Conditioning the q target rows on the
// m q neighbour rows needs a joint block of (m + 1) q <= 64 rows: one wavefront per location, the block in LDS as
// 16 x 16 tiles, every rank-16 update on v_mfma_f64_16x16x4_f64.
//
// Tiles.  The neighbours' m q rows (slot-major) take NT = ceil(m q / 16) tile rows; rows beyond m q are decoupled
// diagonal rows.  The q target rows do NOT continue them: they would straddle two tiles (q = 3, m = 10: rows 30..32).  They
// sit in one more tile row X (16 x 16 NT) together with the c value columns, transposed:
//   X rows 0..q-1     C(target, neighbours)
//   X rows q..q+c-1   the neighbours' value columns
// so whitening X by L_N (X <- X L_N^-T, the panel step of the factorisation itself) gives W and z_N^T at once, and
// one more product G = X X^T holds W W^T (rows, columns < q) and W z_N (columns q..): F = C_tt - W W^T, the
// conditional mean W z_N.  The q x q tail (LF = chol F, E = LF^-1 (V_t - W z_N)) is VALU work.
//
// A tile is stored column-major with a column stride of 17 doubles: an MFMA operand read X[l % 16][4 s + l / 16] and
// an accumulator access D[4 r + l / 16][l % 16] are both free of bank conflicts.  The lane map of the instruction
// (tests/test_gpu_mv.py pins it): A[i][k] in lane i + 16 k, B[k][j] in lane j + 16 k, D[4 r + l / 16][l % 16] in
// element r of lane l.
//
// Factorisation, left-looking over tile columns k: a tile's updates from the columns j < k accumulate in registers
// (one chain of MFMAs per tile, the chains of a column independent), so a tile is written once.  The diagonal tile
// goes to registers, a row per lane, for a 16 x 16 Cholesky with cross-lane broadcasts; its inverse is a forward
// substitution with a column per lane.  A panel tile is A_ik L_kk^-T, a product with the stored inverse.  B = W L_N^-1
// (only when wanted) is a back-substitution over the tiles on the same inverses.
//
// Slots without a point (-1 padding, an out-of-range index) are masked: covariance 0 off the diagonal, the slot's
// own q x q block kept diagonal, and the rows of B exactly 0.
#pragma once
#include "mv_host.h"
#include "nngp_internal.h"

namespace nngp {

typedef double mv_d4 __attribute__((ext_vector_type(4)));

constexpr int kMvLd = 17;            // column stride of a tile
constexpr int kMvTe = 16 * kMvLd;    // doubles per tile
constexpr int kMvSmall = 16 + 4 * 8; // C_tt (4 x 4) and the target's values (4 x 8)

struct MvParams {
    CovParams pc[kMvMaxQ];  // component k: sigma2 = 1, phi_k
    double A[kMvMaxQ][kMvMaxQ];
    double tau2[kMvMaxQ];
    // dmin = min_a (sum_k A_ak^2 + tau2_a), the smallest marginal variance: the padding rows carry it, and a pivot
    // that is not above 2^-44 dmin counts as non-positive (the pivot of an exactly singular block is rounding noise
    // of either sign, some 2^-52 of the diagonal; a block this far gone has no correct digits left either way)
    double dmin, pivmin;
};

struct MvArgs {
    const double* coords;  // (n_points, dim)
    int64_t n_points;
    const int32_t* nbr;    // (n_rows, m), -1 padded
    const int32_t* order;  // or null
    int64_t n_rows, i0;
    int m, q, kind, dim;
    const double *A, *phi, *tau2;  // host: (q, q) row-major, (q,), (q,)
    const double* values;          // (n_points, q, c) or null
    const double* qcoords;         // the locations themselves: coords (S = T) or the query points (cross)
    const double* qvalues;         // values (S = T) or null (cross)
    int c;
    int cross;                     // E receives the conditional mean W z_N instead of the whitened residual
    int target_noise;              // tau2 on the target's diagonal (always, for the S = T form)
    double* B;                     // (n_rows, q, m q) or null
    double* LF;                    // (n_rows, q, q) or null
    double* E;                     // (n_rows, q, c) or null
    double* rec;                   // 4 doubles per block
};

// LDS written by some lanes of the wavefront and read by others
__device__ __forceinline__ void mv_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ constexpr int mv_tri(int i, int j) { return i * (i + 1) / 2 + j; }

// a tile in the accumulator's layout
__device__ __forceinline__ mv_d4 mv_ld(const double* t, int lane) {
    const double* p = t + (lane & 15) * kMvLd + (lane >> 4);
    return mv_d4{p[0], p[4], p[8], p[12]};
}
__device__ __forceinline__ void mv_st(double* t, int lane, mv_d4 v) {
    double* p = t + (lane & 15) * kMvLd + (lane >> 4);
    p[0] = v[0];
    p[4] = v[1];
    p[8] = v[2];
    p[12] = v[3];
}

// acc +- X Y^T for two tiles
template <bool NEG>
__device__ __forceinline__ mv_d4 mv_mma_nt(const double* X, const double* Y, mv_d4 acc, int lane) {
    const int off = (lane >> 4) * kMvLd + (lane & 15);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const double a = X[off + 4 * kMvLd * s];
        const double b = Y[off + 4 * kMvLd * s];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(NEG ? -a : a, b, acc, 0, 0, 0);
    }
    return acc;
}
// acc +- X Y
template <bool NEG>
__device__ __forceinline__ mv_d4 mv_mma_nn(const double* X, const double* Y, mv_d4 acc, int lane) {
    const int offa = (lane >> 4) * kMvLd + (lane & 15);
    const int offb = (lane & 15) * kMvLd + (lane >> 4);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const double a = X[offa + 4 * kMvLd * s];
        const double b = Y[offb + 4 * s];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(NEG ? -a : a, b, acc, 0, 0, 0);
    }
    return acc;
}

// Cholesky of the diagonal tile Lt in place (lower factor, zeros above) and its inverse into It; true on a
// pivot that is not above pivmin
__device__ __forceinline__ bool mv_chol_inv(double* Lt, double* It, int lane, double pivmin) {
    const int row = lane & 15;
    double a[16], ip[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) a[j] = Lt[j * kMvLd + row];
    bool bad = false;
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        const double piv = wave_bcast(a[p], p);
        bad |= !(piv > pivmin);
        ip[p] = nngp_rsqrt(piv);
        a[p] *= ip[p];  // lane p: L_pp; the lanes below: L[row][p]
#pragma unroll
        for (int b = p + 1; b < 16; ++b) a[b] = fma(-a[p], wave_bcast(a[p], b), a[b]);
    }
    if (lane < 16) {
#pragma unroll
        for (int j = 0; j < 16; ++j) Lt[j * kMvLd + row] = j <= row ? a[j] : 0.0;
    }
    mv_sync();
    // column `row` of L^-1 by forward substitution; L[i][k] is one address for the whole wavefront
    double x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        double s = i == row ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < i; ++k) s = fma(-Lt[k * kMvLd + i], x[k], s);
        x[i] = s * ip[i];
    }
    if (lane < 16) {
#pragma unroll
        for (int i = 0; i < 16; ++i) It[row * kMvLd + i] = x[i];
    }
    mv_sync();
    return bad;
}

template <int Q, int NT>
__global__ __launch_bounds__(64 * kMvWaves) void bf_mv(const double* __restrict__ coords, int64_t n_points,
                                                       const int32_t* __restrict__ nbr,
                                                       const int32_t* __restrict__ order, int64_t n_rows, int64_t i0,
                                                       int m, int dim, const MvParams P,
                                                       const double* __restrict__ values,
                                                       const double* __restrict__ qcoords,
                                                       const double* __restrict__ qvalues, int c, int cross,
                                                       int target_noise, double* __restrict__ Bout,
                                                       double* __restrict__ LFout, double* __restrict__ Eout,
                                                       double* __restrict__ rec) {
    constexpr int NTRI = NT * (NT + 1) / 2;
    constexpr int WAVE = (NTRI + 2 * NT) * kMvTe + kMvSmall;
    __shared__ double etab[NNGP_EXP_TAB_N];
    __shared__ double lds[kMvWaves][WAVE];
    nngp_exp_table_load(etab, 1.0);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* Nt = lds[wv];            // the neighbours' lower triangle, tile (i, j) at mv_tri(i, j)
    double* Xt = Nt + NTRI * kMvTe;  // the target / value tile row
    double* It = Xt + NT * kMvTe;    // inverses of the diagonal tiles
    double* ctt = It + NT * kMvTe;   // C_tt, 4 x 4
    double* vt = ctt + 16;           // target values, 4 x 8
    double* pts = It;                // build only: (m + 1) x {x, y, z, point index}

    const int64_t blk = xcd_logical_block(blockIdx.x, gridDim.x);
    const int64_t r = blk * kMvWaves + wv;
    const bool live = r < n_rows;
    const int64_t rl = live ? r : n_rows - 1;
    const int64_t rr = order != nullptr ? (int64_t)order[rl] : rl;
    const int64_t i = i0 + rr;
    const int mq = m * Q;

    // ---- the m + 1 points, one per lane; a slot without a point reads point 0 and is masked
    int32_t j = -1;
    if (lane < m) j = nbr[rl * m + lane];
    const bool in_range = j >= 0 && (int64_t)j < n_points;
    const bool bad_index = __any(lane < m && j != -1 && !in_range);
    const uint64_t vmask = __ballot(in_range || lane == m);
    if (lane <= m) {
        double x[3];
        load_point_rt(lane == m ? qcoords + i * dim : coords + (in_range ? (int64_t)j * dim : 0), dim, x);
        pts[4 * lane] = x[0];
        pts[4 * lane + 1] = x[1];
        pts[4 * lane + 2] = x[2];
        pts[4 * lane + 3] = in_range ? (double)j : -1.0;
    }
    // X starts as zeros; the rows of N beyond m q are decoupled (diagonal) rows
    for (int e = lane; e < NT * kMvTe; e += 64) Xt[e] = 0.0;
    for (int e = lane; e < (16 * NT - mq) * 16 * NT; e += 64) {
        const int rw = mq + e / (16 * NT), cl = e % (16 * NT);
        if (cl <= rw) Nt[mv_tri(rw >> 4, cl >> 4) * kMvTe + (cl & 15) * kMvLd + (rw & 15)] = cl == rw ? P.dmin : 0.0;
    }
    mv_sync();

    // ---- the (m + 1)(m + 2) / 2 point pairs a >= b, dealt over the lanes: one distance, Q correlations, a Q x Q block
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
                    const bool noise = a < m || !cross || target_noise;
                    v = al == be ? (noise ? v + P.tau2[al] : v) : (ok ? v : 0.0);
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
    // ---- the value columns: the neighbours' into X rows Q.., the target's own into vt
    if (values != nullptr) {
        for (int e = lane; e < mq * c; e += 64) {
            const int s = e / c, col = e - s * c;
            const int slot = s / Q, be = s - slot * Q;
            const double jd = pts[4 * slot + 3];
            const double v = jd >= 0.0 ? values[((int64_t)jd * Q + be) * c + col] : 0.0;
            Xt[(s >> 4) * kMvTe + (s & 15) * kMvLd + Q + col] = v;
        }
    }
    if (lane < Q * c) {
        const int al = lane / c, col = lane - al * c;
        vt[8 * al + col] = qvalues != nullptr ? qvalues[(i * Q + al) * c + col] : 0.0;
    }
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

    // ---- G = X X^T into the first diagonal tile (L_00 is not read again: the back-substitution uses its inverse)
    double* Gt = Nt;
    {
        mv_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < NT; ++k) acc = mv_mma_nt<false>(Xt + k * kMvTe, Xt + k * kMvTe, acc, lane);
        mv_st(Gt, lane, acc);
        mv_sync();
    }

    // ---- the Q x Q tail, every lane the same: LF = chol(C_tt - W W^T)
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
            e[al] = s / LF[al][al];
            qq = fma(e[al], e[al], qq);
            if (Eout != nullptr && live) Eout[(rr * Q + al) * c + lane] = bad ? NAN : (cross ? mean : e[al]);
        }
    }
    if (LFout != nullptr && live) {
#pragma unroll
        for (int al = 0; al < Q; ++al)
#pragma unroll
            for (int be = 0; be < Q; ++be)
                if (lane == al * Q + be) LFout[(rr * Q + al) * Q + be] = bad ? NAN : (be <= al ? LF[al][be] : 0.0);
    }

    // ---- B = W L_N^-1 by back-substitution over the tiles (all 16 rows of X ride along)
    if (Bout != nullptr) {
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
        if (live) {
            for (int e = lane; e < Q * mq; e += 64) {
                const int al = e / mq, s = e - al * mq;
                const double v = Xt[(s >> 4) * kMvTe + (s & 15) * kMvLd + al];
                const bool valid = ((vmask >> (s / Q)) & 1) != 0;
                Bout[rr * (int64_t)(Q * mq) + e] = bad ? NAN : (valid ? v : 0.0);
            }
        }
    }

    const bool lead = live && lane == 0;
    block_partials_store(lead ? lf : 0.0, lead && !cross ? qq : 0.0, lead && bad ? (double)i : INFINITY,
                         lead && bad_index ? (double)i : INFINITY, rec, blk);
}

// the kernels' parameters from the host arrays A (q, q) row-major, phi (q,), tau2 (q,)
inline MvParams mv_params(int q, int kind, const double* A, const double* phi, const double* tau2) {
    MvParams P;
    P.dmin = INFINITY;
    for (int k = 0; k < q; ++k) {
        double d = tau2[k];
        for (int b = 0; b <= k; ++b) d += A[k * q + b] * A[k * q + b];
        P.dmin = fmin(P.dmin, d);
    }
    P.pivmin = ldexp(P.dmin, -44);
    for (int k = 0; k < kMvMaxQ; ++k) {
        P.pc[k] = nngp_cov_params(kind, 1.0, k < q ? phi[k] : 1.0, 0.0);
        P.tau2[k] = k < q ? tau2[k] : 0.0;
        for (int b = 0; b < kMvMaxQ; ++b) P.A[k][b] = (k < q && b <= k) ? A[k * q + b] : 0.0;
    }
    return P;
}

template <int Q, int NT>
static bool launch_mv_if(const MvArgs& a, hipStream_t s) {
    if (a.q != Q || mv_tiles(a.m, a.q) != NT) return false;
    const MvParams P = mv_params(Q, a.kind, a.A, a.phi, a.tau2);
    hipLaunchKernelGGL((bf_mv<Q, NT>), dim3((unsigned)mv_blocks(a.n_rows)), dim3(64 * kMvWaves), 0, s, a.coords,
                       a.n_points, a.nbr, a.order, a.n_rows, a.i0, a.m, a.dim, P, a.values, a.qcoords, a.qvalues, a.c,
                       a.cross, a.target_noise, a.B, a.LF, a.E, a.rec);
    return true;
}

// the instantiation units (bf_mv_q*.hip) and the dispatch + fold (bf_mv.hip)
bool bf_mv_launch_q2(const MvArgs& a, hipStream_t s);
bool bf_mv_launch_q3(const MvArgs& a, hipStream_t s);
bool bf_mv_launch_q4(const MvArgs& a, hipStream_t s);
hipError_t bf_mv_launch(const MvArgs& a, double* partials, hipStream_t s);

}  // namespace nngp
