// Latent-field posterior at fixed theta (latent.hip): the precision operator on a reference set S, the leaves
// integrated out,
//   A_S = (I - B_S)^T diag(f_S) (I - B_S) + diag(d_S) + B_L^T diag(g) B_L,   f = invF / sigma2,   g = f d / (f + d)
// applied matrix-free from the Gibbs `prep` buffer, and a Jacobi-preconditioned CG on it.  S = T is the system
// without leaves (n_s = n):  A = (I - B)^T (sigma2 F)^-1 (I - B) + diag(d).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace nngp {

// the arrays of a nngp_gibbs_prepare buffer the operator reads (gibbs.hip owns the layout)
struct LatentPrep {
    const double* Brev;  // B_{j,i} per reverse entry
    const double* P;     // sum_e B_{j,i}^2 / F_j per location
    const double* invF;  // 1 / F_i
};
LatentPrep latent_prep_view(const void* prep, int64_t n, int m);

struct LatentGeom {
    const int32_t* nbr;    // (n, m), -1 padded
    const double* B;       // (n, m)
    const int32_t* off;    // (n + 1,) reverse lists (nngp_reverse_neighbors)
    const int32_t* rev_j;  // child row per reverse entry
    LatentPrep prep;
    int64_t n;
    int m;
    double sigma2;
    const double* d;  // (n,) diagonal term, or null
    // Nodes 0 .. n_s - 1 are reference points, the others leaves whose parents are reference points; n_s = n: S = T.
    // s: the row scale (n,) once a launch of a system with leaves has computed it; null on entry, and it stays
    // null without leaves.
    int64_t n_s;
    const double* s;
};

// One launch per operation.  Vectors on S are (n_s, nrhs) row-major, on all nodes (n, nrhs), on the leaves
// (n - n_s, nrhs), 1 <= nrhs <= NNGP_LATENT_MAX_RHS; a single right-hand side is nrhs = 1.  Column c of every
// result depends on column c of the inputs alone, bit for bit, whatever nrhs is and whatever the other columns
// hold.  A system without leaves (n_s = n) runs the REF = false kernels on prep's own scale: no s, no vector read
// per row for it, and the bits S = T always had.
// Workspace sizes: of the S = T entry points (n_s = n), and of the reference-set ones, which for n_s = n are the
// larger of the two layouts.
size_t latent_apply_workspace_bytes(int64_t n, int nrhs);
size_t latent_cg_workspace_bytes(int64_t n, int nrhs);
size_t latent_ref_apply_workspace_bytes(int64_t n, int64_t n_s, int nrhs);
size_t latent_ref_cg_workspace_bytes(int64_t n, int64_t n_s, int nrhs);
// out = A_S x
hipError_t latent_apply_launch(LatentGeom g, int nrhs, const double* x, double* out, void* workspace, hipStream_t s);
// out = (I - B_S)^T f_S^1/2 z1_S + B_L^T g^1/2 z1_L + d_S^1/2 z2 (z1 on all nodes, z2 on S)
hipError_t latent_sqrt_t_apply_launch(LatentGeom g, int nrhs, const double* z1, const double* z2, double* out,
                                      void* workspace, hipStream_t s);
// out = d_S v_S + B_L^T (g v_L) (v on all nodes): the right-hand side of the mean.  Always through the REF kernels
hipError_t latent_fold_launch(LatentGeom g, int nrhs, const double* v, double* out, void* workspace, hipStream_t s);
// out = diag(A_S) (n_s,), the CG's preconditioner before its reciprocal: the sum over a node's children in the
// column phase's order (workspace: the operator's at nrhs = 1); without leaves d_i + (invF_i + P_i) / sigma2 from
// prep alone (d null: 0), and no workspace is read
hipError_t latent_diag_launch(LatentGeom g, double* out, void* workspace, hipStream_t s);
// nrhs Jacobi-PCG recurrences for A_S x = b in lock step from the start in x, each with its own scalars and
// stopping; info_host: (nrhs, 4) rows of iterations, converged (1 / 0 / -1 breakdown), |r|^2, |b|^2.  A finished
// column is frozen; the launches are no-ops once every column is finished.  Synchronises the stream once per
// chunk of check_every iterations.
// trace: null, or device (nrhs, trace_len, 2) with trace_len >= max_iter.  After iteration k of column c completes
// (the column was active and did not break down in it) trace[c][k] = (alpha_k, beta_k), beta_k = r_k+1.z_k+1 /
// r_k.z_k; entries at k >= the column's final iteration count are never written, a frozen column writes nothing.
// One thread writes them from the scalars the direction launch holds; the solve is the same bits with or without.
// They are the Lanczos tridiagonal T of M^-1/2 A M^-1/2 for the start M^-1/2 r_0: T[j,j] = 1 / alpha_j +
// beta_j-1 / alpha_j-1 (the second term absent at j = 0), T[j,j+1] = sqrt(beta_j) / alpha_j.
hipError_t latent_cg_run(LatentGeom g, int nrhs, const double* b, double* x, double rtol, int64_t max_iter,
                         int check_every, double* info_host, void* workspace, hipStream_t s, double* trace = nullptr,
                         int64_t trace_len = 0);
// the leaves given x on S: out = (f a + d v) / (f + d) [+ z / sqrt(f + d)], a = B_L x; v, z null or (n - n_s, nrhs);
// g.d null: out = a [+ z / sqrt(f)]
hipError_t latent_leaves_launch(const LatentGeom& g, int nrhs, const double* x, const double* v, const double* z,
                                double* out, hipStream_t s);
// two weighted gathers over every node row in one pass: p = B x, q = dB x, both (n, nrhs), x (n_s, nrhs); a slot that
// is -1 or names a node >= n_s counts 0.  The summation order is the row phase's.
hipError_t latent_rows_dot2_launch(const int32_t* nbr, const double* B, const double* dB, int64_t n, int64_t n_s,
                                   int m, int nrhs, const double* x, double* p, double* q, hipStream_t s);

}  // namespace nngp
