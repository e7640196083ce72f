/*
 * nngp.h -- C ABI of libnngp_hip.so, the MI355X (gfx950) NNGP hot path.
 *
 * The reference (bwpriest/pyNNGP) exposes this path only as Python methods of
 * class NNGP; there is no FFI in it.  Each entry point below names the reference
 * interface it replaces (file:line under /root/reference).  The Python binding
 * (pynngp_amd/_lib.py, ctypes) and the torch custom ops (pynngp_amd/ops.py) are
 * thin layers over exactly these symbols; INTEGRATION.md shows the binding a
 * pyNNGP maintainer would add.
 *
 * Conventions
 *   - Every pointer argument except the host-side `partials_host` of
 *     nngp_loglik_from_partials is a DEVICE pointer (hipMalloc / torch CUDA
 *     tensor memory); the caller owns every buffer.
 *   - `stream` is a hipStream_t (NULL = default stream).  All work is
 *     stream-ordered; no call synchronises the host, allocates, or frees (the exceptions say so:
 *     the setup calls nngp_pair_plan_build / nngp_nbr_cert_build / nngp_color_moral_graph_dev and
 *     the solvers nngp_latent_cg / nngp_latent_cg_batch synchronise the stream).
 *   - Coordinates are fp64 (n_points, dim) row-major, dim = 1, 2 or 3 (the
 *     reference's KDTree takes ordinates of any dimension, nngp.py:55-61); they
 *     must be finite.  Neighbour sets are int32 (rows, m) row-major, padded with -1
 *     (row i holds min(i, m) indices).
 *   - Return 0 on success or a negative NNGP_E* code (nngp_last_error() gives
 *     the message).  Numerical failures are data, not return codes, because the
 *     work is asynchronous: see `partials` of nngp_bf_sweep.
 */
#ifndef NNGP_H
#define NNGP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNGP_OK 0
#define NNGP_EINVAL (-1)    /* bad argument (shape, range, null pointer, small workspace) */
#define NNGP_ENOTPD (-2)    /* a location's C_N / F was not positive definite (nngp_check_partials) */
#define NNGP_EHIP (-3)      /* a HIP runtime call or kernel launch failed */
#define NNGP_EUNSUP (-4)    /* unsupported configuration (e.g. m > 63) */

/* covariance kinds (the reference's `cov` plug-in, nngp.py:6,12), u = phi d: */
#define NNGP_COV_EXPONENTIAL 0 /* sigma2 exp(-u)                                    */
#define NNGP_COV_MATERN32 1    /* sigma2 (1 + u) exp(-u)                            */
#define NNGP_COV_MATERN52 2    /* sigma2 (1 + u + u^2/3) exp(-u)                    */
#define NNGP_COV_GAUSSIAN 3    /* sigma2 exp(-u^2)                                  */
#define NNGP_COV_SPHERICAL 4   /* sigma2 (1 - 3u/2 + u^3/2) for u < 1, else 0       */
#define NNGP_COV_MATERN 5      /* sigma2 u^nu K_nu(u) / (2^(nu-1) Gamma(nu)), 0 < nu <= 50: spNNGP's
                                  "matern" of any smoothness nu (the `nu` argument of the sweeps;
                                  ignored by the other kinds).  m <= 24 (pair kernel) and 25..32
                                  (four-lane kernel): rho from a per-launch table in t = (phi d)^2,
                                  every nu; for nu < 0.9 whose table would pass 160 octaves, below
                                  t = 2^-64 the small-t expansion 1 - A t^nu.  m > 32: the wavefront
                                  kernel's direct Bessel evaluation. */

/* kernels (NNGP_ALGO_AUTO picks the fastest measured one for m, kind and dim); LANE serves 2-D
 * exponential / Matern-3/2 only, QUAD kinds 0..4 in every dimension, PAIRB and WAVE every kind
 * (PAIRB and QUAD: NNGP_COV_MATERN through its table; PAIRB at 25 <= m <= 32: kinds 0..4).  (3 and 7 were comparison-only kernels of earlier
 * builds; they are rejected as unknown.) */
#define NNGP_ALGO_AUTO 0  /* pairb for 1 <= m <= 32 except quad at 31, wave above (matern: see kind 5) */
#define NNGP_ALGO_LANE 1  /* one lane per location (m <= 16)                                 */
#define NNGP_ALGO_WAVE 2  /* one wavefront per location (m <= 63)                            */
#define NNGP_ALGO_QUAD 4  /* four lanes per location (25 <= m <= 32)                         */
#define NNGP_ALGO_PAIRB 5 /* two lanes per location, 2x2-blocked (1 <= m <= 24)              */

/* the kernel NNGP_ALGO_AUTO (or an explicit code, returned as is) resolves to for (m, kind, dim);
 * for NNGP_COV_MATERN the choice depends on nu: nngp_resolve_algo_nu (nngp_resolve_algo assumes a nu
 * the pair kernel's table covers).  nngp_bf_finalize of a matern sweep needs the resolved code. */
int32_t nngp_resolve_algo(int32_t algo, int32_t m, int32_t kind, int32_t dim);
int32_t nngp_resolve_algo_nu(int32_t algo, int32_t m, int32_t kind, int32_t dim, double nu);

#define NNGP_MAX_M 63
#define NNGP_MAX_DIM 3
#define NNGP_ND_MAX_DIM 16 /* the n-dimensional path (nngp_*_nd): 4 <= dim <= NNGP_ND_MAX_DIM */

/* Library version string, e.g. "pynngp_amd 0.3.0 gfx950". */
const char *nngp_version(void);

/* ABI revision of this header (NNGP_ABI_VERSION), for a caller built against an older one to
 * refuse a library whose signatures moved.  Revision 2 (library 0.2.0) changed, relative to 1
 * (0.1.0): nngp_bf_finalize takes workspace_bytes as its 2nd argument; nngp_gibbs_w_sweep reads
 * (n, 4) member rows (nngp_gibbs_member_rows) and lost its `off` argument; nngp_bf_sweep /
 * nngp_bf_cross take `nu` after tau2; nngp_bf_sweep_blocks serves 1 <= m <= 32.  Revision 3
 * (library 0.3.0) adds the tile pair plans (nngp_pair_plan_*, nngp_bf_sweep_plan), the batched
 * chains' sweeps (nngp_gibbs_w_sweep_chains, _il) and the device colouring (nngp_color_moral_graph_dev);
 * NNGP_ALGO_AUTO / PAIRB / QUAD take the general Matern kind for every nu; nothing earlier moved.
 * Revision 4 (library 0.4.0): the pair plans are per wave (a new plan format, m <= 17) and their info
 * array holds 10 words (NNGP_PLAN_INFO_LEN: + the nbr / order pointers, checked by nngp_bf_sweep_plan).
 * Added within revision 4 (nothing earlier moved): the gradient sweep nngp_bf_grad_workspace_bytes /
 * nngp_bf_grad, its per-axis form nngp_bf_grad_aniso_workspace_bytes / nngp_bf_grad_aniso and its
 * general-nu Matern form nngp_bf_grad_matern_workspace_bytes / nngp_bf_grad_matern with nngp_matern_eval_d; the
 * latent-field posterior nngp_precision_workspace_bytes / nngp_precision_apply /
 * nngp_precision_sqrt_t_apply / nngp_latent_cg_workspace_bytes / nngp_latent_cg; their forms for several
 * right-hand sides nngp_precision_batch_workspace_bytes / nngp_precision_apply_batch /
 * nngp_precision_sqrt_t_apply_batch / nngp_latent_cg_batch_workspace_bytes / nngp_latent_cg_batch, and
 * nngp_precision_diag. */
#define NNGP_ABI_VERSION 4
int32_t nngp_abi_version(void);

/* Message for the last error returned on the calling thread. */
const char *nngp_last_error(void);

/* ---------------------------------------------------------------------------
 * Neighbour sets.
 * Replaces NNGP._make_s_neighbor_sets, pyNNGP/nngp.py:49-62 (a sklearn KDTree
 * rebuilt on s[0:i] for every i; ordering key sklearn euclidean_rdist64,
 * sklearn/metrics/_dist_metrics.pxd:26-40).
 * For every query row i in [q0, q1): the k = min(m, i) nearest points among
 * coords[0:i], ascending fp64 rdist = (0 + t0*t0) + t1*t1 (no FMA), exact
 * ties by lower index, written to nbr[(i - q0) * m + s], s < k; -1 beyond.  rdist
 * sums t_k^2 over the dim coordinates in axis order, unfused, as sklearn does.
 * Requires n_points <= INT32_MAX, 1 <= dim <= 3, 0 <= m <= 64,
 * 0 <= q0 <= q1 <= n_points, and finite coordinates (NaN / inf give unspecified
 * sets; the Python layer rejects them).
 * ------------------------------------------------------------------------- */
size_t nngp_knn_workspace_bytes(int64_t n_points, int32_t dim, int32_t m);
int nngp_knn_prior(const double *coords, int64_t n_points, int32_t dim, int32_t m, int64_t q0, int64_t q1,
                   int32_t *nbr, void *workspace, size_t workspace_bytes, void *stream);

/* Same neighbour sets for an arbitrary list of locations: query row t is point rows[t]
 * (its min(m, rows[t]) nearest among coords[0:rows[t]]), written to nbr[t * m + s].
 * Used to build a shard's sets when the shard is a range of a spatial storage order
 * (pynngp_amd.sweep.ShardedLogLik, layout "storage").  Workspace as nngp_knn_prior. */
int nngp_knn_prior_rows(const double *coords, int64_t n_points, int32_t dim, int32_t m, const int32_t *rows,
                        int64_t n_rows, int32_t *nbr, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Unrestricted k-nearest neighbours of query points among a reference set.
 * Replaces the sklearn searches behind NNGP._init_ws (pyNNGP/nngp.py:45-47,
 * KNeighborsRegressor(n_neighbors=5).fit(t, y).predict(s)) and
 * NNGP._make_t_neighbor_sets (nngp.py:64-71, KDTree(s).query(t, m)).
 * nbr[q * k + s] = index into ref of the s-th nearest point to query[q]
 * ((rdist, index) order, self included when a query point is in ref), -1 for
 * s >= n_ref.  ref and query are (n, dim).  Workspace: nngp_knn_workspace_bytes(n_ref, dim, k).
 * ------------------------------------------------------------------------- */
int nngp_knn_query(const double *ref, int64_t n_ref, int32_t dim, const double *query, int64_t n_query, int32_t k,
                   int32_t *nbr, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Fused B/F + log-likelihood sweep over locations i0 .. i0 + n_rows - 1.
 * Replaces the per-location stubs of class NNGP:
 *   _CNs  nngp.py:78-82   C_{N(s_i)}       (covariance among the neighbours, + tau2 I)
 *   _Ccross nngp.py:84-86 C_{s_i, N(s_i)}  (location vs neighbours)
 *   _Cs   nngp.py:92-96   C_{s_i, s_i}     (sigma2 + tau2)
 *   _Bsi  nngp.py:73-76   B_i = C_{s_i,N} C_N^{-1}       -> B (n_rows, m), 0 in -1 slots
 *   _Fsi  nngp.py:88-90   F_i = C_ii - B_i C_{N,s_i}     -> F (n_rows,)
 * and the log-likelihood sweep consumed by oneSample (nngp.py:98-101, absent):
 *   partials[0] = sum_i log F_i
 *   partials[1] = sum_i (v_i - B_i v_N(i))^2 / F_i        (0 when values == NULL)
 *   partials[2] = first location index whose Cholesky pivot or F_i is not > 0, else -1
 *   partials[3] = first location index with an invalid neighbour index (>= n_points, or
 *                 negative other than the -1 padding), else -1; such a row's slot is
 *                 decoupled (a far-away point), so its B / F / log-lik terms are finite but
 *                 meaningless: callers check the flag (nngp_check_partials)
 *   log-lik = -1/2 (n_rows log 2 pi + partials[0] + partials[1]).
 * Rows flagged in partials[2] get B = F = NaN.  The sum order is fixed, so the
 * partials are bit-reproducible run to run.
 * coords: (n_points, dim); nbr: (n_rows, m); order: NULL (row t of nbr is location
 * i0 + t) or the nngp_row_order layout (row t of nbr is location i0 + order[t],
 * i.e. pass nbr_sorted); values: (n_points,) or NULL;
 * B, F: may be NULL (log-lik only); R: NULL or (n_rows,) residuals
 * r_i = v_i - B_i v_N(i) (needs values; the Gibbs w-update keeps them current);
 * partials: 4 doubles, or NULL to defer the final fold: the per-block records stay in
 * the workspace and nngp_bf_finalize (same n_rows, m, kind, dim, algo) folds them later,
 * e.g. on another stream while the next sweep (with another workspace) runs.
 * workspace: nngp_bf_sweep_workspace_bytes(n_rows, m, kind, dim, algo) bytes, 256-B aligned, its first
 * 256 bytes zeroed once before the first sweep that uses it (the pair kernel's header: its tile count
 * and the ticket of the fold a small sweep does in its last block, which every sweep leaves at zero;
 * the same holds for nngp_bf_cross and nngp_bf_sweep_blocks workspaces).
 * kind, sigma2 > 0, phi > 0, tau2 >= 0: the covariance (the reference's `cov`); nu: the smoothness
 * of NNGP_COV_MATERN (0 < nu <= 50), ignored by the other kinds.
 * ------------------------------------------------------------------------- */
size_t nngp_bf_sweep_workspace_bytes(int64_t n_rows, int32_t m, int32_t kind, int32_t dim, int32_t algo);
int nngp_bf_sweep(const double *coords, int64_t n_points, int32_t dim, const int32_t *nbr, const int32_t *order,
                  int64_t n_rows, int32_t m, int64_t i0, int32_t kind, double sigma2, double phi, double tau2,
                  double nu, const double *values, double *B, double *F, double *R, double *partials, void *workspace,
                  size_t workspace_bytes, int32_t algo, void *stream);
/* The deferred fold of a sweep run with partials == NULL (fixed order: the same
 * bits as the in-line fold).  n_rows, m, kind, dim and algo must be the sweep's (they select
 * the kernel, hence the record layout); workspace_bytes is checked against the size that
 * sweep needed, so a mismatched call fails with NNGP_EINVAL instead of reading past it. */
int nngp_bf_finalize(const void *workspace, size_t workspace_bytes, int64_t n_rows, int32_t m, int32_t kind,
                     int32_t dim, int32_t algo, double *partials, void *stream);

/* ---------------------------------------------------------------------------
 * Analytic gradient of the log-likelihood in (sigma2, phi, tau2), one fused sweep over locations
 * i0 .. i0 + n_rows - 1 (S = T sweeps: coords, nbr, order, i0 and values as nngp_bf_sweep, values required).
 *   partials[4]: as nngp_bf_sweep (its own fixed fold order: equal to nngp_bf_sweep's to rounding, not bit
 *                for bit)
 *   grad[3]    = sum_i d l_i / d (sigma2, phi, tau2), a fixed-order fold: bit-reproducible run to run
 *   G          : NULL or (n_rows, 3), the term of location i0 + r in row r (r = order[t] for nbr row t, else t)
 * Rows flagged in partials[2] get NaN in G, and either flag makes grad meaningless (nngp_check_partials).
 * Slots without a point (-1 padding) and out-of-range indices contribute exactly 0 to every sum.
 * kind: NNGP_COV_EXPONENTIAL .. NNGP_COV_SPHERICAL (the general-nu Matern kind: NNGP_EUNSUP); 1 <= m <= 32
 * (else NNGP_EUNSUP); 1 <= dim <= 3.  workspace: nngp_bf_grad_workspace_bytes(n_rows, m) bytes (0 for an
 * unsupported m or n_rows < 0), 256-B aligned, no initialisation needed.
 * ------------------------------------------------------------------------- */
size_t nngp_bf_grad_workspace_bytes(int64_t n_rows, int32_t m);
int nngp_bf_grad(const double *coords, int64_t n_points, int32_t dim, const int32_t *nbr, const int32_t *order,
                 int64_t n_rows, int32_t m, int64_t i0, int32_t kind, double sigma2, double phi, double tau2,
                 const double *values, double *G, double *partials, double *grad, void *workspace,
                 size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Per-point noise: y_i = mu + w(s_i) + e_i with e_i ~ N(0, tau2 v_i), v_i >= 0 given per point (added within
 * revision 4; nothing earlier moved).  noise_var (n_points,) holds the weights v (v = 1 everywhere is the model
 * of nngp_bf_sweep / nngp_bf_grad).  The diagonal entry of every joint block is sigma2 + tau2 v_j of the point in
 * that slot -- the location's own entry included --, the weight gathered with the point's coordinates.  The
 * reference's `eps` ("measurement uncertainties in y", nngp.py:9) squared is v; it has no sweep of its own.
 *   nngp_bf_sweep_noise: the contract of nngp_bf_sweep (B, F, R, partials[4], order, i0, -1 padding, the two
 *     flags, NaN rows on a bad pivot, a fixed-order fold), without nu / algo and with partials required.
 *   nngp_bf_cross_noise: the contract of nngp_bf_cross; noise_ref (n_ref,) weighs the neighbour block,
 *     noise_query (n_query,) or NULL (1) the query point's own diagonal entry.
 *   nngp_bf_grad_noise: the contract of nngp_bf_grad (G, partials[4], grad[3] in (sigma2, phi, tau2)) with
 *     d/dtau2: dF = v_i + sum_j b_j^2 v_j, dr = sum_j a_j b_j v_j; d/dsigma2: dF = (F - tau2 dF_tau2) / sigma2,
 *     dr = -tau2 dr_tau2 / sigma2; d/dphi unchanged.
 * Scope: kinds NNGP_COV_EXPONENTIAL .. NNGP_COV_SPHERICAL, 1 <= m <= 32, 1 <= dim <= 3, else NNGP_EUNSUP.
 * workspace: nngp_bf_sweep_noise_workspace_bytes(n_rows, m) for the sweep and the cross form,
 * nngp_bf_grad_workspace_bytes(n_rows, m) for the gradient; 256-B aligned, no initialisation needed.
 * ------------------------------------------------------------------------- */
size_t nngp_bf_sweep_noise_workspace_bytes(int64_t n_rows, int32_t m);
int nngp_bf_sweep_noise(const double *coords, int64_t n_points, int32_t dim, const int32_t *nbr, const int32_t *order,
                        int64_t n_rows, int32_t m, int64_t i0, int32_t kind, double sigma2, double phi, double tau2,
                        const double *values, const double *noise_var, double *B, double *F, double *R,
                        double *partials, void *workspace, size_t workspace_bytes, void *stream);
int nngp_bf_cross_noise(const double *ref, int64_t n_ref, int32_t dim, const double *query, int64_t n_query,
                        const int32_t *nbr, const int32_t *order, int64_t n_rows, int32_t m, int64_t q0, int32_t kind,
                        double sigma2, double phi, double tau2, const double *ref_values, const double *query_values,
                        const double *noise_ref, const double *noise_query, double *B, double *F, double *R,
                        double *partials, void *workspace, size_t workspace_bytes, void *stream);
int nngp_bf_grad_noise(const double *coords, int64_t n_points, int32_t dim, const int32_t *nbr, const int32_t *order,
                       int64_t n_rows, int32_t m, int64_t i0, int32_t kind, double sigma2, double phi, double tau2,
                       const double *values, const double *noise_var, double *G, double *partials, double *grad,
                       void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Separable space-time covariance (added within revision 4; nothing earlier moved):
 *   C(a, b) = sigma2 rho_s(phi_s |a_s - b_s|) rho_t(phi_t |a_t - b_t|) + tau2 delta_ab.
 * The points are (n, dim) with dim = 2 or 3: the last column is time, the first dim - 1 columns are space.
 * kind_s and kind_t are the kinds of the two correlations, NNGP_COV_EXPONENTIAL .. NNGP_COV_SPHERICAL each.
 *   nngp_bf_sweep_sep: the contract of nngp_bf_sweep_noise (B, F, R, partials[4] required, order, i0, -1 padding,
 *     the two flags, NaN rows on a bad pivot, a fixed-order fold).
 *   nngp_bf_cross_sep: the contract of nngp_bf_cross_noise (reference points, query points).
 *   nngp_bf_grad_sep: the contract of nngp_bf_grad with G (n_rows, 4) and grad[4] in (sigma2, phi_s, phi_t, tau2):
 *     dC_ab/dphi_s = sigma2 (u_s rho_s'(u_s)) rho_t(u_t) / phi_s, dC_ab/dphi_t likewise; each is exactly 0 where
 *     that factor's distance is 0.
 * Scope: 1 <= m <= 32, dim 2 or 3, no general-nu factor, else NNGP_EUNSUP.  NNGP_EINVAL for sigma2 <= 0, tau2 < 0
 * or a non-positive or non-finite phi.
 * workspace: nngp_bf_sweep_sep_workspace_bytes(n_rows, m) serves all three (0 for unsupported arguments);
 * 256-B aligned, no initialisation needed.
 * ------------------------------------------------------------------------- */
size_t nngp_bf_sweep_sep_workspace_bytes(int64_t n_rows, int32_t m);
int nngp_bf_sweep_sep(const double *coords, int64_t n_points, int32_t dim, const int32_t *nbr, const int32_t *order,
                      int64_t n_rows, int32_t m, int64_t i0, int32_t kind_s, int32_t kind_t, double sigma2,
                      double phi_s, double phi_t, double tau2, const double *values, double *B, double *F, double *R,
                      double *partials, void *workspace, size_t workspace_bytes, void *stream);
int nngp_bf_cross_sep(const double *ref, int64_t n_ref, int32_t dim, const double *query, int64_t n_query,
                      const int32_t *nbr, const int32_t *order, int64_t n_rows, int32_t m, int64_t q0, int32_t kind_s,
                      int32_t kind_t, double sigma2, double phi_s, double phi_t, double tau2, const double *ref_values,
                      const double *query_values, double *B, double *F, double *R, double *partials, void *workspace,
                      size_t workspace_bytes, void *stream);
int nngp_bf_grad_sep(const double *coords, int64_t n_points, int32_t dim, const int32_t *nbr, const int32_t *order,
                     int64_t n_rows, int32_t m, int64_t i0, int32_t kind_s, int32_t kind_t, double sigma2,
                     double phi_s, double phi_t, double tau2, const double *values, double *G, double *partials,
                     double *grad, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Points in 4 .. NNGP_ND_MAX_DIM dimensions (added within revision 4; nothing earlier moved).  Every entry point
 * above keeps its 1 <= dim <= NNGP_MAX_DIM; these take 4 <= dim <= NNGP_ND_MAX_DIM and nothing else.
 *
 * Neighbour sets, exact, by tiled brute force (N^2 / 2 * dim for the prior form), the ordering key of nngp_knn_prior:
 *   nngp_knn_prior_nd: the contract of nngp_knn_prior (rows [q0, q1), coords[0:i] for row i, -1 padding);
 *   nngp_knn_query_nd: the contract of nngp_knn_query (every query searches all n_ref points).
 * 0 <= m (k) <= 32.  workspace: nngp_knn_nd_workspace_bytes(n_points, dim, m), 256-B aligned (the searches use
 * none of it; the size is 0 only for unsupported arguments).
 *
 * Sweeps under one decay per axis (ARD):
 *   C(a, b) = sigma2 rho(u) + tau2 delta_ab,  u = sqrt(sum_k (phi[k] (a_k - b_k))^2),
 * phi a HOST array of dim decays, kind NNGP_COV_EXPONENTIAL, MATERN32, MATERN52 or GAUSSIAN.  NNGP_COV_SPHERICAL is
 * refused with NNGP_EUNSUP: it is not positive definite above three dimensions.
 *   nngp_bf_sweep_nd: the contract of nngp_bf_sweep_noise without the weights (B, F, R, partials[4] required, order,
 *     i0, -1 padding, the two flags, NaN rows on a bad pivot, a fixed-order fold).
 *   nngp_bf_cross_nd: the contract of nngp_bf_cross_noise without the weights (reference points, query points).
 *   nngp_bf_grad_nd: the contract of nngp_bf_grad_aniso with G (n_rows, dim + 2) and grad[dim + 2] in
 *     (sigma2, phi_1..phi_dim, tau2): dC_ab/dphi_k = sigma2 rho'(u) (phi_k (a_k - b_k))^2 / (u phi_k), exactly 0 for
 *     coincident points.
 * Scope: 1 <= m <= 32, 4 <= dim <= NNGP_ND_MAX_DIM, kinds as above, else NNGP_EUNSUP.  NNGP_EINVAL for sigma2 <= 0,
 * tau2 < 0, a non-positive or non-finite phi[k], a null pointer.
 * workspace: nngp_bf_sweep_nd_workspace_bytes(n_rows, m, dim) serves all three (0 for unsupported arguments);
 * 256-B aligned, no initialisation needed.
 * ------------------------------------------------------------------------- */
size_t nngp_knn_nd_workspace_bytes(int64_t n_points, int32_t dim, int32_t m);
int nngp_knn_prior_nd(const double *coords, int64_t n_points, int32_t dim, int32_t m, int64_t q0, int64_t q1,
                      int32_t *nbr, void *workspace, size_t workspace_bytes, void *stream);
int nngp_knn_query_nd(const double *ref, int64_t n_ref, int32_t dim, const double *query, int64_t n_query, int32_t k,
                      int32_t *nbr, void *workspace, size_t workspace_bytes, void *stream);
size_t nngp_bf_sweep_nd_workspace_bytes(int64_t n_rows, int32_t m, int32_t dim);
int nngp_bf_sweep_nd(const double *coords, int64_t n_points, int32_t dim, const int32_t *nbr, const int32_t *order,
                     int64_t n_rows, int32_t m, int64_t i0, int32_t kind, double sigma2, const double *phi, double tau2,
                     const double *values, double *B, double *F, double *R, double *partials, void *workspace,
                     size_t workspace_bytes, void *stream);
int nngp_bf_cross_nd(const double *ref, int64_t n_ref, int32_t dim, const double *query, int64_t n_query,
                     const int32_t *nbr, const int32_t *order, int64_t n_rows, int32_t m, int64_t q0, int32_t kind,
                     double sigma2, const double *phi, double tau2, const double *ref_values,
                     const double *query_values, double *B, double *F, double *R, double *partials, void *workspace,
                     size_t workspace_bytes, void *stream);
int nngp_bf_grad_nd(const double *coords, int64_t n_points, int32_t dim, const int32_t *nbr, const int32_t *order,
                    int64_t n_rows, int32_t m, int64_t i0, int32_t kind, double sigma2, const double *phi, double tau2,
                    const double *values, double *G, double *partials, double *grad, void *workspace,
                    size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * The factors and their phi-derivatives, one fused sweep over locations i0 .. i0 + n_rows - 1 (coords, nbr,
 * order and i0 as nngp_bf_sweep).  With D_ab = sigma2 d_ab rho'(phi d_ab) and u = [-B_i; 1]:
 *   B  (n_rows, m), F (n_rows,): the factors of nngp_bf_sweep at this theta, equal to that sweep's to its own
 *                                tolerance (another elimination order: not bit for bit)
 *   dB (n_rows, m) = d B_i / d phi = C_N^-1 (D u)[:m]
 *   dF (n_rows,)   = d F_i / d phi = u^T D u
 *   partials[4]    = sum_i log F_i, sum_i dF_i / F_i, and the two flags of nngp_bf_sweep, folded in that sweep's
 *                    fixed order: bit-reproducible run to run
 * Slots without a point (-1 padding) and out-of-range indices hold exactly 0 in B and dB and add exactly 0 to
 * dF; rows flagged in partials[2] get NaN in all four arrays (nngp_check_partials reads the flags).
 * kind: NNGP_COV_EXPONENTIAL .. NNGP_COV_SPHERICAL (the general-nu Matern kind: NNGP_EUNSUP); 1 <= m <= 32
 * (else NNGP_EUNSUP); 1 <= dim <= 3.  workspace: nngp_bf_dphi_workspace_bytes(n_rows, m) bytes (0 for an
 * unsupported m or n_rows < 0), 256-B aligned, no initialisation needed.
 * ------------------------------------------------------------------------- */
size_t nngp_bf_dphi_workspace_bytes(int64_t n_rows, int32_t m);
int nngp_bf_dphi(const double *coords, int64_t n_points, int32_t dim, const int32_t *nbr, const int32_t *order,
                 int64_t n_rows, int32_t m, int64_t i0, int32_t kind, double sigma2, double phi, double tau2,
                 double *B, double *F, double *dB, double *dF, double *partials, void *workspace,
                 size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Fisher information of the NNGP log-likelihood in (sigma2, phi, tau2), with the log-likelihood's partials and
 * its gradient, one fused sweep over locations i0 .. i0 + n_rows - 1 (added within revision 4; coords, nbr, order,
 * i0 and values as nngp_bf_grad).  Row i's term is its expected information under the exact Gaussian law of its
 * joint block (location and neighbours), 1/2 tr(A^-1 dA_j A^-1 dA_k) - 1/2 tr(N^-1 dN_j N^-1 dN_k) with A the
 * joint block and N its neighbour block (Guinness 2021), positive semi-definite row by row.
 *   partials[4]: as nngp_bf_grad
 *   grad[3]    = sum_i d l_i / d (sigma2, phi, tau2)
 *   info[6]    = sum_i I_i, the upper triangle in the order (ss, sp, st, pp, pt, tt) for s = sigma2, p = phi,
 *                t = tau2; all three are fixed-order folds, bit-reproducible run to run
 *   I_rows     : NULL or (n_rows, 6), the term of location i0 + r in row r (r = order[t] for nbr row t, else t)
 *   G          : NULL or (n_rows, 3), the gradient's terms, rows as I_rows
 * values == NULL gives the information alone (it does not depend on the data): grad, G and partials[1] are
 * written as exactly 0, and info and I_rows hold the bits of the call with values.
 * Rows flagged in partials[2] get NaN in I_rows and G, and either flag makes the sums meaningless
 * (nngp_check_partials).  Slots without a point (-1 padding) and out-of-range indices contribute exactly 0 to
 * every sum.  kind: NNGP_COV_EXPONENTIAL .. NNGP_COV_SPHERICAL (the general-nu Matern kind: NNGP_EUNSUP);
 * 1 <= m <= 32 (else NNGP_EUNSUP); 1 <= dim <= 3.  workspace: nngp_bf_fisher_workspace_bytes(n_rows, m) bytes
 * (0 for an unsupported m or n_rows < 0), 256-B aligned, no initialisation needed.
 * ------------------------------------------------------------------------- */
size_t nngp_bf_fisher_workspace_bytes(int64_t n_rows, int32_t m);
int nngp_bf_fisher(const double *coords, int64_t n_points, int32_t dim, const int32_t *nbr, const int32_t *order,
                   int64_t n_rows, int32_t m, int64_t i0, int32_t kind, double sigma2, double phi, double tau2,
                   const double *values, double *I_rows, double *G, double *partials, double *grad, double *info,
                   void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Analytic gradient of the log-likelihood for a covariance with one decay per axis,
 * u = sqrt(sum_k (phi_k (a_k - b_k))^2), in (sigma2, phi_1 .. phi_dim, tau2): one fused sweep over locations
 * i0 .. i0 + n_rows - 1 (added within revision 4; coords -- the raw, unscaled coordinates --, nbr, order, i0 and
 * values as nngp_bf_grad).  B, F and the log-likelihood of this model are nngp_bf_sweep's at phi = 1 on the
 * coordinates scaled column by column; with delta_k the scaled coordinate difference,
 * dC_ab / dphi_k = sigma2 rho'(u) delta_k^2 / (u phi_k), exactly 0 for coincident points.
 *   phi          : HOST array of dim entries, read before the call returns
 *   partials[4]  : as nngp_bf_grad
 *   grad[dim + 2] = sum_i d l_i / d (sigma2, phi_1, .., phi_dim, tau2), a fixed-order fold: bit-reproducible run
 *                  to run
 *   G            : NULL or (n_rows, dim + 2), the term of location i0 + r in row r (r = order[t] for nbr row t,
 *                  else t)
 * Rows flagged in partials[2] get NaN in G, and either flag makes grad meaningless (nngp_check_partials).
 * Slots without a point (-1 padding) and out-of-range indices contribute exactly 0 to every sum.
 * kind: NNGP_COV_EXPONENTIAL .. NNGP_COV_SPHERICAL (the general-nu Matern kind: NNGP_EUNSUP); 1 <= m <= 32
 * (else NNGP_EUNSUP); 1 <= dim <= 3 (else NNGP_EUNSUP).  phi == NULL and any phi_k that is not positive and
 * finite: NNGP_EINVAL, as sigma2 <= 0 and tau2 < 0.  workspace: nngp_bf_grad_aniso_workspace_bytes(n_rows, m,
 * dim) bytes (0 for an unsupported m or dim, or n_rows < 0), 256-B aligned, no initialisation needed.
 * ------------------------------------------------------------------------- */
size_t nngp_bf_grad_aniso_workspace_bytes(int64_t n_rows, int32_t m, int32_t dim);
int nngp_bf_grad_aniso(const double *coords, int64_t n_points, int32_t dim, const int32_t *nbr, const int32_t *order,
                       int64_t n_rows, int32_t m, int64_t i0, int32_t kind, double sigma2,
                       const double *phi /* host, dim entries */, double tau2, const double *values, double *G,
                       double *partials, double *grad /* dim + 2 */, void *workspace, size_t workspace_bytes,
                       void *stream);

/* ---------------------------------------------------------------------------
 * Gradient sweep for the general-smoothness Matern kind (NNGP_COV_MATERN), with the smoothness as a fourth
 * parameter: the analytic gradient of the NNGP log-likelihood in (sigma2, phi, tau2, nu), one fused sweep over
 * locations i0 .. i0 + n_rows - 1 (added within revision 4; coords, nbr, order, i0 and values as nngp_bf_grad).
 * With rho_nu(u) = 2^(1-nu) / Gamma(nu) u^nu K_nu(u) and u = phi d,
 *   dC_ab / dphi = sigma2 h(u) / phi,  h(u) = u rho'(u) = -2^(1-nu) / Gamma(nu) u^(nu+1) K_{nu-1}(u),
 *   dC_ab / dnu  = sigma2 n(u),        n(u) = d rho_nu(u) / d nu,
 * both exactly 0 for coincident points.  The sweep reads rho, h and n from per-launch tables in t = u^2 that it
 * builds in the workspace, stream-ordered before the sweep.
 *   partials[4]  : as nngp_bf_grad
 *   grad[4]      = sum_i d l_i / d (sigma2, phi, tau2, nu), a fixed-order fold: bit-reproducible run to run
 *   G            : NULL or (n_rows, 4), the term of location i0 + r in row r (r = order[t] for nbr row t, else t)
 * Rows flagged in partials[2] get NaN in G, and either flag makes grad meaningless (nngp_check_partials).
 * Slots without a point (-1 padding) and out-of-range indices contribute exactly 0 to every sum.
 * 1 <= m <= 32 and 1 <= dim <= 3 (else NNGP_EUNSUP).  nu outside (0, 50], sigma2 <= 0, phi <= 0, tau2 < 0,
 * values == NULL or a short workspace: NNGP_EINVAL.  workspace: nngp_bf_grad_matern_workspace_bytes(n_rows, m)
 * bytes (the block records and room for the three tables; 0 for an unsupported m or n_rows < 0), 256-B aligned,
 * no initialisation needed; it may be reused across calls with different nu.
 *
 * nngp_matern_eval_d: h[k] = u rho'(u) and dnu[k] = d rho / d nu at n arguments u >= 0, elementwise, read through
 * the same derivative table and lookup as the sweep (0 < nu <= 50, else NNGP_EINVAL): a building block, and the
 * handle by which the tables are tested.  The table lives in stream-ordered memory (hipMallocAsync /
 * hipFreeAsync on `stream`) for the duration of the call's kernels; no host synchronisation.
 * ------------------------------------------------------------------------- */
size_t nngp_bf_grad_matern_workspace_bytes(int64_t n_rows, int32_t m);
int nngp_bf_grad_matern(const double *coords, int64_t n_points, int32_t dim, const int32_t *nbr, const int32_t *order,
                        int64_t n_rows, int32_t m, int64_t i0, double sigma2, double phi, double tau2, double nu,
                        const double *values, double *G /* NULL or (n_rows, 4) */, double *partials /* 4 */,
                        double *grad /* 4 */, void *workspace, size_t workspace_bytes, void *stream);
int nngp_matern_eval_d(const double *u, int64_t n, double nu, double *h /* u rho'(u) */, double *dnu, void *stream);

/* ---------------------------------------------------------------------------
 * Wave pair plans: the same sweep with every covariance a wavefront's locations share evaluated once.
 * The pair kernel (NNGP_ALGO_PAIRB) sweeps 32 consecutive rows per wavefront; in a spatial visiting
 * order neighbouring locations share most of their neighbours, so only ~46 % of a wave's joint-block
 * entries are distinct point pairs (N = 1e6, m = 15).  A plan -- built once per (nbr, order, i0,
 * n_points), like the neighbour sets -- lists per wave its distinct points and pairs and, per lane,
 * where each of its joint-block entries lives; nngp_bf_sweep_plan then evaluates each pair once into
 * the wave's LDS slice and factors every location's block from there.  Same reference methods as
 * nngp_bf_sweep (_CNs / _Ccross / _Cs / _Bsi / _Fsi, nngp.py:73-96); its B, F, R are bit-identical to
 * nngp_bf_sweep's with NNGP_ALGO_PAIRB on the same arguments, and so are its partials (tiles whose
 * waves exceed the LDS budget are swept by the unplanned kernel into the same records).
 * nngp_pair_plan_supported: 1 when plans serve (m, kind, dim): 2 <= m <= 17, kinds 0..4, dim 1..3.
 * nngp_pair_plan_bytes: the plan buffer's size (0: unsupported m).
 * nngp_pair_plan_build: builds the plan for the sweep's nbr / order / i0 / n_points (device
 * pointers as nngp_bf_sweep; 256-B aligned plan) on `stream`, then SYNCHRONISES the stream (a setup
 * call, the one exception to the no-synchronisation rule above) to fill the host array
 * info[NNGP_PLAN_INFO_LEN]: tiles swept through the plan, tiles swept directly, the geometry the
 * plan was built for (n_rows, m, dim, i0, n_points), a tag, and the nbr and order pointers.
 * nngp_bf_sweep_plan: nngp_bf_sweep's arguments (algo PAIRB implied; kinds 0..4, no nu) plus the
 * plan and its info; n_rows, m, dim, i0, n_points and the nbr / order pointers must be those in info
 * (checked: NNGP_EINVAL).  The plan is stale once the contents of nbr or order change: the kernel
 * re-derives a per-location checksum of the words it reads and flags a mismatching location in
 * partials[3] with B = F = R = NaN, so a stale plan never returns the old neighbour sets' results.
 * ------------------------------------------------------------------------- */
#define NNGP_PLAN_INFO_LEN 10
int nngp_pair_plan_supported(int32_t m, int32_t kind, int32_t dim);
size_t nngp_pair_plan_bytes(int64_t n_rows, int32_t m, int32_t dim);
int nngp_pair_plan_build(const int32_t *nbr, const int32_t *order, int64_t n_rows, int32_t m, int64_t i0,
                         int64_t n_points, int32_t dim, void *plan, size_t plan_bytes, int64_t *info, void *stream);
int nngp_bf_sweep_plan(const double *coords, int64_t n_points, int32_t dim, const int32_t *nbr, const int32_t *order,
                       int64_t n_rows, int32_t m, int64_t i0, int32_t kind, double sigma2, double phi, double tau2,
                       const double *values, double *B, double *F, double *R, double *partials, void *workspace,
                       size_t workspace_bytes, const void *plan, size_t plan_bytes, const int64_t *info,
                       void *stream);

/* ---------------------------------------------------------------------------
 * Neighbour-set certificates: the same sweep without the per-sweep index checks and distance clamps.
 * In real use (a theta scan, an MCMC chain) coords, nbr and order are fixed for the life of the model;
 * nngp_bf_sweep still range-checks every neighbour index and clamps every squared distance on every
 * launch.  A certificate -- built once per (coords, nbr, order, i0), like the neighbour sets -- records
 * per tile of the pair kernel whether any slot of its rows is < 0 or >= n_points (CHECKED: -1 padding and
 * bad indices alike; such tiles run exactly as in nngp_bf_sweep), and the squared diagonal of the
 * coordinates' bounding box, d2_span.  No reference counterpart (same methods as nngp_bf_sweep,
 * _CNs / _Ccross / _Cs / _Bsi / _Fsi, nngp.py:73-96); B, F, R, the tile records and the partials of
 * nngp_bf_sweep_cert are bit-identical to nngp_bf_sweep's on the same arguments: the trusted tiles leave
 * out only operations that are the identity on them.
 * nngp_nbr_cert_bytes: the certificate buffer's size for n_rows rows (0: n_rows < 0).
 * nngp_nbr_cert_build: builds it on `stream`, then SYNCHRONISES the stream (a setup call, as
 *   nngp_pair_plan_build) to fill the host array info[NNGP_CERT_INFO_LEN]: a tag, the coords / nbr / order
 *   pointers, n_points, dim, n_rows, m, i0, the tile count, the number of checked tiles, and d2_span (a
 *   double's bits).  NNGP_EINVAL for a non-finite coordinate.  1 <= m <= NNGP_MAX_M, cert 256-B aligned.
 * nngp_nbr_cert_trusted_tiles: a pure HOST function: the number of tiles a sweep of (kind, theta) runs
 *   trusted -- 0 when the clamp may bind (d2_span (1 + 2^-40) is not below the kind's clamp distance), when
 *   the kind is not one of 0..4, or m > 24.  The one place the theta-dependent decision is made;
 *   nngp_bf_sweep_cert calls it too.
 * nngp_bf_sweep_cert: nngp_bf_sweep's arguments plus the certificate and its info.  coords, nbr, order,
 *   n_points, dim, n_rows, m and i0 must be those in info (checked before any launch: NNGP_EINVAL, a caller
 *   bug).  When the resolved kernel is not the pair kernel or nngp_nbr_cert_trusted_tiles gives 0 it is
 *   exactly nngp_bf_sweep: the certificate is a hint.
 * CONTRACT: the caller does not modify the contents of nbr, order or coords after certifying them (the
 * trusted tiles read coords[nbr[..]] unchecked); rebuild the certificate after any change.
 * ------------------------------------------------------------------------- */
#define NNGP_CERT_INFO_LEN 16
size_t nngp_nbr_cert_bytes(int64_t n_rows);
int nngp_nbr_cert_build(const double *coords, int64_t n_points, int32_t dim, const int32_t *nbr, const int32_t *order,
                        int64_t n_rows, int32_t m, int64_t i0, void *cert, size_t cert_bytes, int64_t *info,
                        void *stream);
int64_t nngp_nbr_cert_trusted_tiles(const int64_t *info, int32_t kind, double sigma2, double phi, double tau2);
int nngp_bf_sweep_cert(const double *coords, int64_t n_points, int32_t dim, const int32_t *nbr, const int32_t *order,
                       int64_t n_rows, int32_t m, int64_t i0, int32_t kind, double sigma2, double phi, double tau2,
                       double nu, const double *values, double *B, double *F, double *R, double *partials,
                       void *workspace, size_t workspace_bytes, int32_t algo, const void *cert, size_t cert_bytes,
                       const int64_t *info, void *stream);

/* ---------------------------------------------------------------------------
 * B/F of query locations t against a reference set S (prediction / kriging at
 * t not in S).  SURVEY.md 8(f) row 2: the reference builds Nt for refType != 'S=T'
 * (NNGP._make_t_neighbor_sets, pyNNGP/nngp.py:64-71, KDTree(s).query(t, m)) but
 * never evaluates B_t / F_t; this is the same fused kernel as nngp_bf_sweep with
 * the location row taken from `query`:
 *   C_N = C(S_N) + tau2 I over the neighbours nbr[(q - q0) * m + k] (indices into
 *   ref; any of them, no prior restriction; -1 = unused slot), c = C(t_q, S_N),
 *   C_tt = sigma2 + tau2, B_t = c^T C_N^{-1}, F_t = C_tt - c^T C_N^{-1} c.
 * ref_values (nullable): v on S.  query_values (nullable; needs ref_values): v at t.
 * R[q] = query_values[q] - B_t v_N(t) (query_values NULL: 0 - B_t v_N(t), i.e. minus
 * the kriging mean).  partials as nngp_bf_sweep (with query_values: the
 * conditional log density of v_t given v_S).  Rows q in [q0, q0 + n_rows) of
 * n_query; order / workspace as nngp_bf_sweep (nngp_row_order on the query
 * coordinates; nngp_bf_sweep_workspace_bytes), kind / theta / nu as nngp_bf_sweep.  ref and
 * query are (n, dim).
 * ------------------------------------------------------------------------- */
int nngp_bf_cross(const double *ref, int64_t n_ref, int32_t dim, const double *query, int64_t n_query,
                  const int32_t *nbr, const int32_t *order, int64_t n_rows, int32_t m, int64_t q0, int32_t kind,
                  double sigma2, double phi, double tau2, double nu, const double *ref_values,
                  const double *query_values,
                  double *B, double *F, double *R, double *partials, void *workspace, size_t workspace_bytes,
                  int32_t algo, void *stream);

/* ---------------------------------------------------------------------------
 * A covariance of the caller's own (the reference's `cov` is an arbitrary plug-in,
 * pyNNGP/nngp.py:6,12, called on coordinate rows at :82,:96; SURVEY.md 8(b) asks for callables):
 * the caller evaluates its function on every joint block -- an isotropic function of
 * nngp_joint_dist's distances, or any cov(a, b) on the blocks' gathered coordinates -- and the
 * blocks drive the same fused sweep.
 * nngp_joint_dist: for nbr row t (location i = i0 + (order ? order[t] : t); joint rows
 *   a = 0..m-1 the neighbour slots, row m the location, from qcoords) the packed lower
 *   triangle of the joint block's distances, entry (a, b), b <= a, at
 *   dist[(a (a + 1) / 2 + b) * n_rows + t] -- nngp_joint_entries(m) = (m+1)(m+2)/2 entries
 *   per row, entry-major; 0 on the diagonal, +inf where a slot holds no point.  Distances are
 *   sqrt of the unfused sum of squared coordinate differences.
 * nngp_bf_sweep_blocks: the fused B/F + log-lik sweep (outputs, partials, order and values
 *   as nngp_bf_sweep / nngp_bf_cross: values (n_points,) of the neighbours, qvalues (n_locs,)
 *   of the locations, may be NULL) with the joint blocks' covariances read from `cov` in that
 *   layout -- cov[e] = C(dist[e]) plus the nugget on the diagonal entries; entries of slots
 *   without a point are ignored (decoupled exactly).  1 <= m <= 32 (the two-lane blocked
 *   kernel up to 24, the four-lane kernel for 25..32); workspace
 *   nngp_bf_sweep_blocks_workspace_bytes(n_rows), 256-B aligned; partials required.
 * ------------------------------------------------------------------------- */
/* out[k] = u^nu K_nu(u) / (2^(nu-1) Gamma(nu)) for n arguments u >= 0 (the Matern correlation
 * of NNGP_COV_MATERN, elementwise; 0 < nu <= 50): a building block for such covariances. */
int nngp_matern_eval(const double *u, int64_t n, double nu, double *out, void *stream);
int64_t nngp_joint_entries(int32_t m);
int nngp_joint_dist(const double *coords, int64_t n_points, int32_t dim, const double *qcoords, int64_t n_locs,
                    const int32_t *nbr, const int32_t *order, int64_t n_rows, int32_t m, int64_t i0, double *dist,
                    void *stream);
size_t nngp_bf_sweep_blocks_workspace_bytes(int64_t n_rows);
int nngp_bf_sweep_blocks(const double *cov, const int32_t *nbr, const int32_t *order, int64_t n_points, int64_t n_rows,
                         int32_t m, int64_t i0, int64_t n_locs, const double *values, const double *qvalues, double *B,
                         double *F, double *R, double *partials, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Visiting order for nngp_bf_sweep (a speed option; no reference counterpart:
 * the reference visits locations in input order, nngp.py:51).
 * order[t] = the t-th local row (0 .. n_rows-1) of locations i0 .. i0+n_rows-1
 * in Z-order of their coordinates, ties by row; if nbr_sorted is non-NULL it
 * receives nbr's rows in that order (nbr_sorted[t] = nbr[order[t]], (n_rows, m)).
 * Passing (nbr_sorted, order) to nngp_bf_sweep keeps each block's / XCD's
 * neighbour gathers spatially compact (L2 hits) and its index reads coalesced;
 * B and F are bit-identical with or without it (still written at their natural
 * rows), the partials' summation order follows it.
 * Workspace: nngp_row_order_workspace_bytes(n_rows).
 * ------------------------------------------------------------------------- */
size_t nngp_row_order_workspace_bytes(int64_t n_rows);
int nngp_row_order(const double *coords, int64_t n_points, int32_t dim, const int32_t *nbr, int32_t m, int64_t i0,
                   int64_t n_rows, int32_t *order, int32_t *nbr_sorted, void *workspace, size_t workspace_bytes,
                   void *stream);

/* ---------------------------------------------------------------------------
 * Model order of the points: the levelled max-min (nested-net) order (no reference counterpart: the reference
 * takes the caller's row order, nngp.py:51).  Added within ABI revision 4 (nothing earlier moved).
 * The order is defined in DESIGN.md 4.4a and restated in tests/order_ref.py; a call reproduces it index for
 * index and bit for bit from run to run.  In short: p1 is the point nearest the centre of the bounding box,
 * R the distance of the farthest point from p1; level l = 1 .. 19 selects, in rounds, points that keep a
 * distance >= R 2^-l from everything selected before them until every point has a selected point closer than
 * that; the points no level selects (coincident points, and points closer than R 2^-19 to an earlier one) are
 * the tail, level 20.  Inside a level, and in the tail, points are sorted by
 * key(i) = mix32(i + seed * 0x9e3779b9) << 32 | i (mix32: the murmur3 finaliser).
 *   coords (n, dim) fp64 row-major, finite, 1 <= dim <= 3, 1 <= n < 2^31.
 *   perm_out int64 (n,): perm_out[k] = the input row at position k.   level_out int32 (n,): level_out[k] = the
 *   level (0 for p1, 1 .. 19, 20 for the tail) of the point at position k, non-decreasing in k.
 * NNGP_EINVAL for a NULL pointer, dim outside [1, 3], n < 1, a short or misaligned workspace, a coordinate that
 * is not finite or a squared distance that overflows.
 * workspace: nngp_order_maxmin_workspace_bytes(n, dim) bytes (0 for bad arguments), 256-B aligned, no
 * initialisation needed.  On return its first 64 int32 hold what the call did: launches enqueued, count reads,
 * the last level entered, the tail's size, then 20 each of rounds, accept/retire iterations and points selected
 * per level (index = level).
 * A SETUP CALL: it synchronises `stream` once per round (the host sizes the next launches by one 256-byte read),
 * so it cannot be captured into a graph.
 * ------------------------------------------------------------------------- */
size_t nngp_order_maxmin_workspace_bytes(int64_t n, int32_t dim);
int nngp_order_maxmin(const double *coords, int64_t n, int32_t dim, uint32_t seed, int64_t *perm_out,
                      int32_t *level_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Multi-GPU: fold the all-gathered partials of `world` ranks (device array
 * (world, 4), rank-major, e.g. from an RCCL all-gather) in rank order:
 * partials[0..1] = sums, partials[2..3] = smallest non-negative flag or -1.
 * Every rank gets the bit-identical result.  No reference counterpart (the
 * reference is single-process).
 * nngp_combine_partials_batch: the same fold for n_slots independent sweeps exchanged in ONE
 * all-gather: gathered (world, n_slots, 4) rank-major (each rank contributed its (n_slots, 4)
 * block), partials (n_slots, 4); slot k's result is bit-identical to nngp_combine_partials of
 * that sweep alone.
 * ------------------------------------------------------------------------- */
int nngp_combine_partials(const double *gathered, int32_t world, double *partials, void *stream);
int nngp_combine_partials_batch(const double *gathered, int32_t world, int64_t n_slots, double *partials,
                                void *stream);

/* ---------------------------------------------------------------------------
 * Gibbs sampler for the response model y = X beta + w + eps (SURVEY.md 8(f)
 * row 1).  Replaces NNGP.oneSample, nngp.py:98-101, whose update_wt / update_ws /
 * update_y_unobserved do not exist in the reference; model of Datta et al. 2016
 * as named by the reference docstrings.  Whole-field (single-GPU) arrays.
 *
 * nngp_reverse_neighbors: CSR transpose of nbr (n, m): for location i the
 *   entries e in [off[i], off[i+1]) list the rows j = rev_j[e] whose neighbour
 *   slot rev_k[e] is i, ascending j.  off: n+1, rev_j / rev_k: n*m ints (device).
 * nngp_color_moral_graph (HOST pointers, host computation): greedy colouring
 *   of the moral graph (i ~ N(i); co-parents of a child ~ each other) in index
 *   order; returns the number of colours (or a negative NNGP_E* code).
 * nngp_color_moral_graph_dev: the same colouring (bit for bit: node i takes the smallest colour
 *   no moral neighbour k < i holds) on the device, in parallel rounds (nbr, off, rev_j, color:
 *   device; workspace: >= 256 device bytes); a setup call that synchronises the stream once per 16
 *   rounds.  Returns the number of colours, or a negative NNGP_E* code (NNGP_EUNSUP past 256
 *   colours: use the host version).
 * nngp_gibbs_prepare: fold the factors of the unit-variance field (sigma2 = 1,
 *   tau2 = 0; B (n, m) and Ft (n,) from nngp_bf_sweep) into reverse-list order for
 *   the w sweeps: B_{j,i} and B_{j,i}/F_j per reverse entry, sum_e B_{j,i}^2/F_j and
 *   1/F_i per location, into `prep` (device, nngp_gibbs_prep_bytes(n, m) bytes,
 *   256-B aligned).  Call it again whenever B / Ft change (a new phi accepted).
 *   order: unused (accepted for compatibility; the preparation streams the reverse
 *   lists in their own order).
 * nngp_gibbs_member_rows: member_rows[g] = (members[g], off[members[g]], off[members[g] + 1], 0)
 *   (device int32 (n, 4), 16-B aligned) for `members` (device), the locations grouped by
 *   colour -- built once per colouring; the colour steps then start with one coalesced
 *   16-B load per member instead of two dependent loads.
 * nngp_gibbs_w_sweep: one sweep of w_i | rest over the colours in order;
 *   `member_rows` (nngp_gibbs_member_rows) lists the locations grouped by colour,
 *   color_off_host (host, n_colors + 1) delimits them.  r (n,) holds the residuals
 *   w_i - B_i w_N(i) (nngp_bf_sweep's R), kept current in place with w.
 *   yres = y - X beta.  noise_w: NULL (homoscedastic noise, variance tau2) or n
 *   positive weights h_i, the noise variance of location i being tau2 / h_i (e.g.
 *   h_i = 1 / eps_i^2 for the reference's per-point measurement sigmas, nngp.py:9).
 *   z: NULL (Philox4x32-10 normals keyed by seed, counter
 *   (location, sweep)) or n given standard normals (for testing).
 * nngp_gibbs_normals: z[i] = the Philox4x32-10 normal the sweep would draw for
 *   (seed, location i, sweep), for all n locations in one parallel pass; passing it
 *   as nngp_gibbs_w_sweep's z gives the bit-identical chain with shorter colour steps.
 * nngp_gibbs_w_sweep_chains: nngp_gibbs_w_sweep for `chains` (1..8) independent chains of the same
 *   field -- the same member_rows / colours / rev_j / noise_w, each chain c its own prep[c] (its
 *   phi's factors), sigma2[c], tau2[c] (host arrays), yres[c], w[c], r[c] and given normals z[c]
 *   (host arrays of device pointers) -- in ONE launch per colour; chain c's result is bit-identical
 *   to nngp_gibbs_w_sweep on its own arguments (with z given).
 * nngp_gibbs_w_sweep_chains_il: the same with every chain's w and r interleaved in two (n, chains)
 *   row-major, 16-byte aligned arrays (chain c of location i at [i * chains + c]): a child's r_j of all chains is one
 *   contiguous run, so the colour steps' scattered accesses move one sector for all chains; the
 *   results are the per-chain call's, bit for bit.
 * nngp_gibbs_stats: out[0] = sum r_i^2 / Ft_i, out[1] = sum h_i (yres_i - w_i)^2,
 *   out[2 + c] = sum_i h_i X[i, c] (y_i - w_i) for c < p (X row-major (n, p));
 *   h_i = noise_w[i], or 1 when noise_w is NULL.
 *
 * One chain sharded over ranks (the w sweep's per-colour exchange;
 * pynngp_amd.gibbs.ShardedSeqNNGP): rank r owns the storage rows [row0, row1) and keeps
 * replicas of w and r, exact on its own rows, their out-of-shard children (halo) and the
 * parents of both.
 * nngp_gibbs_prepare_range: nngp_gibbs_prepare for the rows [row0, row1) only (their
 *   reverse entries [off[row0], off[row1]), P and 1/F); B / Ft must be current on those
 *   rows and their children.  The full range is nngp_gibbs_prepare.
 * nngp_gibbs_w_color: ONE colour step over member_rows (n_members rows of
 *   nngp_gibbs_member_rows, e.g. the run of one colour this rank owns), arguments as
 *   nngp_gibbs_w_sweep; w_out (NULL or n_members doubles) receives each member's new
 *   w, the values the other ranks replay.
 * nngp_gibbs_w_color_dev: the same step with (sigma2, tau2) read from device memory
 *   var[0], var[1] (the kernel forms 1/var exactly as the host would: the same bits) and
 *   the given normals z (required) -- launch arguments that stay fixed across iterations,
 *   so a captured HIP graph of the colour loop replays with each iteration's values.
 * nngp_gibbs_w_apply: replay other ranks' draws of one colour: rows (device int32
 *   (n_rows, 4), 16-B aligned) = (location i, off[i], off[i + 1], src); w_src[src] is the
 *   owner's new w_i.  dw = w_src[src] - w[i] (this rank's replica: the owner's operands),
 *   w[i] = w_src[src], r[i] += dw, r[j] -= B[j, rev_k[e]] dw over the children -- the
 *   owner's arithmetic, so every replica stays bit-identical to the owner's values.
 * ------------------------------------------------------------------------- */
size_t nngp_reverse_workspace_bytes(int64_t n, int32_t m);
int nngp_reverse_neighbors(const int32_t *nbr, int64_t n, int32_t m, int32_t *off, int32_t *rev_j, int32_t *rev_k,
                           void *workspace, size_t workspace_bytes, void *stream);
int64_t nngp_color_moral_graph(const int32_t *nbr_host, const int32_t *off_host, const int32_t *rev_j_host,
                               int64_t n, int32_t m, int32_t *color_host);
int64_t nngp_color_moral_graph_dev(const int32_t *nbr, const int32_t *off, const int32_t *rev_j, int64_t n, int32_t m,
                                   int32_t *color, void *workspace, size_t workspace_bytes, void *stream);
size_t nngp_gibbs_prep_bytes(int64_t n, int32_t m);
int nngp_gibbs_prepare(const double *B, const double *Ft, const int32_t *off, const int32_t *rev_j,
                       const int32_t *rev_k, const int32_t *order, int64_t n, int32_t m, void *prep,
                       size_t prep_bytes, void *stream);
int nngp_gibbs_member_rows(const int32_t *members, int64_t n, const int32_t *off, int32_t *member_rows, void *stream);
int nngp_gibbs_w_sweep(const int32_t *member_rows, const int32_t *color_off_host, int32_t n_colors, const void *prep,
                       int64_t n, int32_t m, double sigma2, double tau2, const double *yres, const double *noise_w,
                       double *w, double *r, const int32_t *rev_j, const double *z, uint64_t seed, uint64_t sweep,
                       void *stream);
/* nngp_gibbs_w_sweep_tiles: the same w sweep, tiled (pynngp_amd/gibbs_tiles.py builds the plan): one launch
 *   per phase, one workgroup per tile of the phase holding its footprint's r and its rows' new w in LDS and
 *   running every colour of its rows in order, in steps; the tiles of a phase have disjoint footprints (each
 *   node and its children), so the sweep is a valid colour sweep in the plan's (level, phase, colour) order.
 *   The plan is contiguous: the storage order is the plan's node order.
 *   tiles: the tile ids of every phase, phase p's at [phase_off_host[p], phase_off_host[p + 1]) (host
 *   offsets); phase_lds_host[p]: its dynamic LDS bytes (gibbs_tiles.tile_lds_bytes of its largest tile);
 *   tinfo (n_tiles, 8) int32, 16-byte aligned: the tile's rows [n0, n1), its footprint range [f0, f1) in
 *   tfp, its step range [s0, s1) in tstep, two zeros; tstep: each step's first row (tile-local), a step
 *   being <= 64 rows of one colour with <= ecap reverse entries (ecap <= 2048); tfp: each tile's footprint
 *   (its rows first, then the halo); rev_loc (n_entries): the footprint-local index of reverse entry e's
 *   child; off: the reverse lists' offsets, n_entries = off[n]; z: the normals (nngp_gibbs_normals).
 *   Round 6. */
int nngp_gibbs_w_sweep_tiles(const int32_t *tiles, const int32_t *phase_off_host, const int32_t *phase_lds_host,
                             int32_t n_phases, const int32_t *tinfo, const int32_t *tstep, int32_t ecap,
                             const int32_t *tfp, const int32_t *off, const int32_t *rev_loc, const void *prep,
                             int64_t n, int32_t m, int64_t n_entries, double sigma2, double tau2, const double *yres,
                             const double *noise_w, double *w, double *r, const double *z, void *stream);
int nngp_gibbs_w_sweep_chains(const int32_t *member_rows, const int32_t *color_off_host, int32_t n_colors,
                              int32_t chains, const void *const *prep, int64_t n, int32_t m, const double *sigma2,
                              const double *tau2, const double *const *yres, const double *noise_w, double *const *w,
                              double *const *r, const int32_t *rev_j, const double *const *z, void *stream);
int nngp_gibbs_w_sweep_chains_il(const int32_t *member_rows, const int32_t *color_off_host, int32_t n_colors,
                                 int32_t chains, const void *const *prep, int64_t n, int32_t m, const double *sigma2,
                                 const double *tau2, const double *const *yres, const double *noise_w, double *w_il,
                                 double *r_il, const int32_t *rev_j, const double *const *z, void *stream);
int nngp_gibbs_normals(int64_t n, uint64_t seed, uint64_t sweep, double *z, void *stream);
int nngp_gibbs_prepare_range(const double *B, const double *Ft, const int32_t *off, const int32_t *rev_j,
                             const int32_t *rev_k, int64_t n, int32_t m, int64_t row0, int64_t row1, void *prep,
                             size_t prep_bytes, void *stream);
int nngp_gibbs_w_color(const int32_t *member_rows, int64_t n_members, const void *prep, int64_t n, int32_t m,
                       double sigma2, double tau2, const double *yres, const double *noise_w, double *w, double *r,
                       const int32_t *rev_j, const double *z, uint64_t seed, uint64_t sweep, double *w_out,
                       void *stream);
int nngp_gibbs_w_color_dev(const int32_t *member_rows, int64_t n_members, const void *prep, int64_t n, int32_t m,
                           const double *var, const double *yres, const double *noise_w, double *w, double *r,
                           const int32_t *rev_j, const double *z, double *w_out, void *stream);
int nngp_gibbs_w_apply(const int32_t *rows, int64_t n_rows, const double *w_src, const double *B, int64_t n, int32_t m,
                       double *w, double *r, const int32_t *rev_j, const int32_t *rev_k, void *stream);
size_t nngp_gibbs_stats_workspace_bytes(int64_t n, int32_t p);
int nngp_gibbs_stats(int64_t n, const double *r, const double *Ft, const double *yres, const double *y,
                     const double *X, int32_t p, const double *w, const double *noise_w, double *out,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Binomial / logistic response by Polya-Gamma augmentation (Polson, Scott and Windle 2013; spNNGP's
 * family = "binomial" -- the reference has no such model): s_i ~ Binomial(b_i, logistic(x_i beta + w_i)).
 * With omega_i ~ PG(b_i, x_i beta + w_i) the update of w is the Gaussian one of nngp_gibbs_w_sweep with
 * tau2 = 1, noise_w = omega and yres_i = kappa_i / omega_i - x_i beta, kappa_i = s_i - b_i / 2.
 * (pynngp_amd/csrc/polya_gamma.h: Devroye's exact PG(1, c) sampler, PG(b, c) the sum of b draws.)
 * Added within ABI revision 4 (nothing earlier moved).
 *
 * nngp_polya_gamma: omega[i] ~ PG(trials[i], c[i]), 0 <= trials[i] <= NNGP_PG_MAX_TRIALS (trials = 0: exactly 0).
 *   Philox4x32-10, key = seed, counter (i, sweep | 1 << 62 | j << 40) for the location's j-th 128-bit block
 *   (sweep < 2^40): a draw depends on (seed, sweep, i, trials[i], c[i]) alone, and shares no block with
 *   nngp_gibbs_normals at any sweep (bit 62).  Faults are data: a location whose c is not finite, whose trials is
 *   out of range or whose sampler hit one of its loop caps gets NaN, and status[0] (one device int32, zeroed by
 *   the call) receives the smallest such index + 1; 0 = clean.
 * nngp_gibbs_pg_update: one sampler iteration's draw, fused: c_i = xb[i] + w[i], omega as nngp_polya_gamma on
 *   that c (bit for bit), yres[i] = kappa[i] / omega[i] - xb[i]; trials[i] = 0: omega[i] = 0 and yres[i] = 0.
 * nngp_gibbs_pg_stats: out[0] = sum r_i^2 / Ft_i, then the upper triangle of X' diag(omega) X row by row
 *   (p (p + 1) / 2 values), then X' (kappa - omega w) (p values); X row-major (n, p), 0 <= p <= 62.  Per-block
 *   records folded in a fixed order, as nngp_gibbs_stats: the same bits on every call.  workspace: at least
 *   nngp_gibbs_pg_stats_workspace_bytes(n, p) bytes.
 * ------------------------------------------------------------------------- */
#define NNGP_PG_MAX_TRIALS 1024
int nngp_polya_gamma(int64_t n, const int32_t *trials, const double *c, uint64_t seed, uint64_t sweep,
                     double *omega, int32_t *status, void *stream);
int nngp_gibbs_pg_update(int64_t n, const int32_t *trials, const double *kappa, const double *xb,
                         const double *w, uint64_t seed, uint64_t sweep,
                         double *omega, double *yres, int32_t *status, void *stream);
size_t nngp_gibbs_pg_stats_workspace_bytes(int64_t n, int32_t p);
int nngp_gibbs_pg_stats(int64_t n, const double *r, const double *Ft, const double *omega,
                        const double *kappa, const double *X, int32_t p, const double *w,
                        double *out, void *workspace, void *stream);

/* ---------------------------------------------------------------------------
 * Latent-field posterior at fixed theta (S = T).  The reference keeps the latent state as ws / wt
 * (pyNNGP/nngp.py:42-47) and only names a sampler for it (oneSample, nngp.py:98-101); for fixed
 * (sigma2, phi, tau2) the posterior is Gaussian and explicit,
 *   A = (I - B)^T (sigma2 F)^-1 (I - B) + diag(d),   d_i = h_i / tau2,   b = h (y - X beta) / tau2,
 *   w | y, theta ~ N(A^-1 b, A^-1),
 * with B (n, m) and F the unit-variance factors of nngp_bf_sweep (sigma2 = 1, tau2 = 0) and h_i the noise
 * weight (0 at a location without an observation).  A is never assembled.  Geometry arguments of every
 * call: nbr (n, m) and B (n, m) as nngp_bf_sweep's, off / rev_j / rev_k from nngp_reverse_neighbors of nbr,
 * prep from nngp_gibbs_prepare of (B, F) (nngp_gibbs_prep_bytes(n, m) bytes, 256-B aligned); 1 <= m <=
 * NNGP_MAX_M, sigma2 > 0; d: NULL (the prior precision alone) or (n,) non-negative.  rev_k is accepted for
 * symmetry with the Gibbs calls and not read (prep already holds B in reverse-list order).
 * nngp_precision_apply: out = A x, two stream-ordered launches without atomics: a gather over nbr
 *   (t = (I - B) x scaled by 1 / (sigma2 F)), then a gather over the reverse lists ((I - B)^T t + d x).
 *   Slots holding -1 contribute exactly 0.  Every sum has a fixed order that depends on m and the list's
 *   length only, so out is bit-identical run to run.  workspace: nngp_precision_workspace_bytes(n) bytes,
 *   256-B aligned; x and out must not alias.
 * nngp_precision_sqrt_t_apply: out = (I - B)^T (sigma2 F)^-1/2 z1 + sqrt(d) z2, the perturbation of exact
 *   posterior draws: Cov(out) = A for standard normal z1, z2 (z2 may be NULL when d is).  Same workspace.
 * nngp_latent_cg: Jacobi-preconditioned conjugate gradients for A x = b (M = diag(A) = d + (invF + P) /
 *   sigma2, straight from prep), x: the start on entry, the solution on return.  Stops when
 *   |r|^2 <= rtol^2 |b|^2 (r the recurrence residual) or after max_iter iterations; alpha and beta stay on
 *   the device and every dot is a fixed-order fold of per-block records, so a solve is bit-reproducible.
 *   A SOLVER CALL THAT SYNCHRONISES the stream once per chunk of check_every iterations (as the setup calls
 *   nngp_pair_plan_build and nngp_nbr_cert_build do once): each chunk ends with one small device-to-host
 *   copy.  info_host (HOST, 4 doubles): iterations done, converged (1; 0: max_iter reached; -1: breakdown,
 *   p.Ap not above 0 or not finite, e.g. NaN in B), |r|^2, |b|^2 -- numerical outcomes are data, the
 *   return code stays NNGP_OK.  0 < rtol < 1, max_iter >= 0, check_every >= 1; workspace:
 *   nngp_latent_cg_workspace_bytes(n) bytes (0 for n < 0), 256-B aligned, no initialisation needed.
 * These three calls are the _batch calls below at nrhs = 1, and their workspace sizes are the one-column
 * batched sizes (nngp_precision_batch_workspace_bytes(n, 1), nngp_latent_cg_batch_workspace_bytes(n, 1)):
 * query them, do not compute them.
 * ------------------------------------------------------------------------- */
size_t nngp_precision_workspace_bytes(int64_t n);
int nngp_precision_apply(const int32_t *nbr, const double *B, const int32_t *off, const int32_t *rev_j,
                         const int32_t *rev_k, const void *prep, int64_t n, int32_t m, double sigma2, const double *d,
                         const double *x, double *out, void *workspace, size_t workspace_bytes, void *stream);
int nngp_precision_sqrt_t_apply(const int32_t *nbr, const double *B, const int32_t *off, const int32_t *rev_j,
                                const int32_t *rev_k, const void *prep, int64_t n, int32_t m, double sigma2,
                                const double *d, const double *z1, const double *z2, double *out, void *workspace,
                                size_t workspace_bytes, void *stream);
size_t nngp_latent_cg_workspace_bytes(int64_t n);
int nngp_latent_cg(const int32_t *nbr, const double *B, const int32_t *off, const int32_t *rev_j,
                   const int32_t *rev_k, const void *prep, int64_t n, int32_t m, double sigma2, const double *d,
                   const double *b, double *x, double rtol, int64_t max_iter, int32_t check_every, double *info_host,
                   void *workspace, size_t workspace_bytes, void *stream);

/* Several right-hand sides at once.  Vectors are (n, nrhs) row-major, 1 <= nrhs <= NNGP_LATENT_MAX_RHS: each
 * index and coefficient is read once for all columns and a gather fetches nrhs contiguous doubles.  Geometry,
 * prep, sigma2, d and the argument checks are those of the calls above (nrhs outside its range: NNGP_EINVAL).
 * THE CONTRACT: column c of every result is bit-identical to the single call on that column alone, for every
 * nrhs and whatever the other columns hold (one kernel family serves every nrhs; the lane groups, tiles,
 * grids and each column's expression sequence do not depend on it).
 * nngp_precision_apply_batch / nngp_precision_sqrt_t_apply_batch: out = A x / the square-root operator, per
 *   column; workspace: nngp_precision_batch_workspace_bytes(n, nrhs) bytes (0 for n < 0 or a bad nrhs); x
 *   (z1 / z2) and out must not alias.
 * nngp_latent_cg_batch: nrhs Jacobi-PCG recurrences in lock step, one set of launches per iteration.  Each
 *   column has its own alpha, beta, dots, tolerance, iteration count and status; a column that has converged
 *   or broken down is frozen from that iteration on (its x is no longer written) and does not disturb the
 *   others; the launches become no-ops once every column is finished.  Synchronises as nngp_latent_cg does,
 *   once per check_every iterations.  info_host (HOST, nrhs x 4 doubles): one row per column with
 *   nngp_latent_cg's meaning; the return code stays NNGP_OK.  n = 0: nothing is launched, every row reads
 *   converged.  workspace: nngp_latent_cg_batch_workspace_bytes(n, nrhs) bytes.
 * nngp_precision_diag: out_i = A_ii = d_i + (invF_i + P_i) / sigma2 (d NULL: 0), the very expression whose
 *   reciprocal preconditions the CG; one stream-ordered launch, no workspace. */
#define NNGP_LATENT_MAX_RHS 8
size_t nngp_precision_batch_workspace_bytes(int64_t n, int32_t nrhs);
int nngp_precision_apply_batch(const int32_t *nbr, const double *B, const int32_t *off, const int32_t *rev_j,
                               const int32_t *rev_k, const void *prep, int64_t n, int32_t m, double sigma2,
                               const double *d, int32_t nrhs, const double *x, double *out, void *workspace,
                               size_t workspace_bytes, void *stream);
int nngp_precision_sqrt_t_apply_batch(const int32_t *nbr, const double *B, const int32_t *off, const int32_t *rev_j,
                                      const int32_t *rev_k, const void *prep, int64_t n, int32_t m, double sigma2,
                                      const double *d, int32_t nrhs, const double *z1, const double *z2, double *out,
                                      void *workspace, size_t workspace_bytes, void *stream);
size_t nngp_latent_cg_batch_workspace_bytes(int64_t n, int32_t nrhs);
int nngp_latent_cg_batch(const int32_t *nbr, const double *B, const int32_t *off, const int32_t *rev_j,
                         const int32_t *rev_k, const void *prep, int64_t n, int32_t m, double sigma2, const double *d,
                         int32_t nrhs, const double *b, double *x, double rtol, int64_t max_iter, int32_t check_every,
                         double *info_host, void *workspace, size_t workspace_bytes, void *stream);
int nngp_precision_diag(const void *prep, int64_t n, int32_t m, double sigma2, const double *d, double *out,
                        void *stream);

/* ---------------------------------------------------------------------------
 * Latent-field posterior on a reference set (S != T), the leaves integrated out.  The reference's refType
 * ('subset', nRef) / ('random', nRef, bounds) puts the field on n_s reference points; a data location outside
 * S is a leaf whose parents are all reference points.  Nodes 0 .. n_s - 1 are the reference points, n_s ..
 * n - 1 the leaves; every entry of nbr (n, m) indexes a reference point or is -1 (an index >= n_s is treated
 * as -1 on the device).  B, F, off / rev_j / rev_k and prep are those of the n-node DAG, built by
 * nngp_bf_sweep / nngp_bf_cross, nngp_reverse_neighbors and nngp_gibbs_prepare as they stand; d (n,) or NULL
 * holds h / tau2 per node, 0 on a node without an observation.  With f_r = invF_r / sigma2, v the centred
 * response and, per leaf j, g_j = f_j d_j / (f_j + d_j) (exactly 0 where d_j = 0), the leaves drop out in
 * closed form and
 *   A_S = (I - B_S)^T diag(f_S) (I - B_S) + diag(d_S) + B_L^T diag(g) B_L,   b_S = d_S v_S + B_L^T (g v_L),
 *   w_S | y ~ N(A_S^-1 b_S, A_S^-1),   w_j | w_S, y ~ N((f_j B_j w_S + d_j v_j) / (f_j + d_j), 1 / (f_j + d_j)),
 * the S-marginal of the posterior over all n nodes.  Vectors on S are (n_s, nrhs) row-major, vectors on all
 * nodes (n, nrhs), vectors on the leaves (n - n_s, nrhs); 1 <= nrhs <= NNGP_LATENT_MAX_RHS, nrhs = 1 being the
 * single call.  Checks as the calls above, and 0 <= n_s <= n.  The same kernel family serves these calls (the
 * row scale is f on a reference row and g on a leaf row, a leaf row has no self term, the reverse-list phase
 * runs over the first n_s nodes): sums keep a fixed order that depends on (m, the list's length, n, n_s) only,
 * no atomics, and column c of every result is bit-identical to the one-column call.
 * THE CONTRACT: with n_s = n every call below equals its _batch counterpart above bit for bit.
 * nngp_precision_ref_apply_batch: out = A_S x.  workspace: nngp_precision_ref_batch_workspace_bytes(n, n_s,
 *   nrhs) bytes (0 for bad arguments), 256-B aligned; it serves the next three calls too.
 * nngp_precision_ref_sqrt_t_apply_batch: out = (I - B_S)^T f_S^1/2 z1_S + B_L^T g^1/2 z1_L + d_S^1/2 z2 with z1
 *   (n, nrhs) and z2 (n_s, nrhs) (NULL allowed when d is): Cov(out) = A_S for standard normals.
 * nngp_precision_ref_fold_batch: out = d_S v_S + B_L^T (g v_L) for v (n, nrhs): b_S of the centred response.
 * nngp_precision_ref_diag: out (n_s,) = diag(A_S)_i = d_i + f_i + sum over children c of B_ci^2 s_c (s = f for a
 *   reference child, g for a leaf), summed in the reverse-list phase's order; workspace as at nrhs = 1.
 * nngp_latent_ref_cg_batch: nngp_latent_cg_batch on A_S x = b, preconditioned by that diagonal: the same four
 *   launches per iteration, per-column state, freezing, check_every and info_host (HOST, nrhs x 4).  workspace:
 *   nngp_latent_ref_cg_batch_workspace_bytes(n, n_s, nrhs) bytes: one (n, nrhs) and four (n_s, nrhs) vectors
 *   where the n-node system needs six (n, nrhs).
 * nngp_latent_ref_cg_batch_trace: nngp_latent_ref_cg_batch that also records the solver's scalars (n_s = n: S = T;
 *   nrhs = 1: the single call).  trace: NULL -- the call is then nngp_latent_ref_cg_batch, bit for bit -- or DEVICE
 *   doubles (nrhs, trace_len, 2) with trace_len >= max_iter (else NNGP_EINVAL), not aliasing b or x.  After
 *   iteration k of column c completes (the column was active and did not break down in it), trace[c][k] =
 *   (alpha_k, beta_k), beta_k = r_k+1.z_k+1 / r_k.z_k.  Entries at k >= that column's final iteration count
 *   (info_host row c, word 0) are never written: a frozen column writes nothing, a breakdown leaves no entry for the
 *   breaking iteration, and the caller's fill of the array survives there.  One thread writes them, stream-ordered,
 *   from the scalars the direction launch already holds; x, info_host and the workspace are the same bits with and
 *   without a trace.  With M = diag(A_S) and the start x = 0 the scalars are the Lanczos tridiagonal T of A^ =
 *   M^-1/2 A_S M^-1/2 for the start vector M^-1/2 b:
 *     T[j,j] = 1 / alpha_j + beta_j-1 / alpha_j-1 (the second term absent at j = 0),  T[j,j+1] = sqrt(beta_j) / alpha_j,
 *   and (M^-1/2 b)^T f(A^) (M^-1/2 b) ~ |M^-1/2 b|^2 e_1^T f(T_k) e_1 is the k-point Gauss quadrature: f = 1 / t gives
 *   b^T x, f = log with probes b = M^1/2 z gives log det A_S = sum_i log M_ii + E_z[z^T log(A^) z].
 * nngp_latent_ref_leaves_batch: the leaves given x (n_s, nrhs) on S: out = (f a + d v) / (f + d) [+ z /
 *   sqrt(f + d)], a = B_L x summed as the row phase sums; v, z: (n - n_s, nrhs) or NULL (v NULL: 0; z NULL: the
 *   conditional mean, else a conditional draw for standard normal z).  d NULL: out = a [+ z / sqrt(f)], kriging
 *   of nrhs fields to unobserved leaves -- prediction points are such leaves.  One launch, no workspace; off,
 *   rev_j and rev_k are not read.
 * ------------------------------------------------------------------------- */
size_t nngp_precision_ref_batch_workspace_bytes(int64_t n, int64_t n_s, int32_t nrhs);
int nngp_precision_ref_apply_batch(const int32_t *nbr, const double *B, const int32_t *off, const int32_t *rev_j,
                                   const int32_t *rev_k, const void *prep, int64_t n, int64_t n_s, int32_t m,
                                   double sigma2, const double *d, int32_t nrhs, const double *x, double *out,
                                   void *workspace, size_t workspace_bytes, void *stream);
int nngp_precision_ref_sqrt_t_apply_batch(const int32_t *nbr, const double *B, const int32_t *off,
                                          const int32_t *rev_j, const int32_t *rev_k, const void *prep, int64_t n,
                                          int64_t n_s, int32_t m, double sigma2, const double *d, int32_t nrhs,
                                          const double *z1, const double *z2, double *out, void *workspace,
                                          size_t workspace_bytes, void *stream);
int nngp_precision_ref_fold_batch(const int32_t *nbr, const double *B, const int32_t *off, const int32_t *rev_j,
                                  const int32_t *rev_k, const void *prep, int64_t n, int64_t n_s, int32_t m,
                                  double sigma2, const double *d, int32_t nrhs, const double *v, double *out,
                                  void *workspace, size_t workspace_bytes, void *stream);
int nngp_precision_ref_diag(const int32_t *nbr, const double *B, const int32_t *off, const int32_t *rev_j,
                            const int32_t *rev_k, const void *prep, int64_t n, int64_t n_s, int32_t m, double sigma2,
                            const double *d, double *out, void *workspace, size_t workspace_bytes, void *stream);
size_t nngp_latent_ref_cg_batch_workspace_bytes(int64_t n, int64_t n_s, int32_t nrhs);
int nngp_latent_ref_cg_batch(const int32_t *nbr, const double *B, const int32_t *off, const int32_t *rev_j,
                             const int32_t *rev_k, const void *prep, int64_t n, int64_t n_s, int32_t m, double sigma2,
                             const double *d, int32_t nrhs, const double *b, double *x, double rtol, int64_t max_iter,
                             int32_t check_every, double *info_host, void *workspace, size_t workspace_bytes,
                             void *stream);
int nngp_latent_ref_cg_batch_trace(const int32_t *nbr, const double *B, const int32_t *off, const int32_t *rev_j,
                                   const int32_t *rev_k, const void *prep, int64_t n, int64_t n_s, int32_t m,
                                   double sigma2, const double *d, int32_t nrhs, const double *b, double *x,
                                   double rtol, int64_t max_iter, int32_t check_every, double *info_host,
                                   void *workspace, size_t workspace_bytes, double *trace, int64_t trace_len,
                                   void *stream);
int nngp_latent_ref_leaves_batch(const int32_t *nbr, const double *B, const int32_t *off, const int32_t *rev_j,
                                 const int32_t *rev_k, const void *prep, int64_t n, int64_t n_s, int32_t m,
                                 double sigma2, const double *d, int32_t nrhs, const double *x, const double *v,
                                 const double *z, double *out, void *stream);

/* Two weighted gathers over every node row of a reference-set DAG in one pass (the gradient of the latent
 * marginal likelihood in phi): for x (n_s, nrhs) on S and every row i < n, reference rows and leaves alike,
 *   p[i, c] = sum_s B[i,s] x[nbr[i,s], c],   q[i, c] = sum_s dB[i,s] x[nbr[i,s], c]      (both (n, nrhs))
 * with B and dB (n, m), e.g. those of nngp_bf_dphi.  An index is read once for both weights and all columns, the
 * sums run in the row phase's order, column c is bit-identical to the nrhs = 1 call on it, and a slot that is -1
 * or names a node >= n_s adds exactly 0.  One launch, no workspace; 1 <= nrhs <= NNGP_LATENT_MAX_RHS. */
int nngp_latent_rows_dot2_batch(const int32_t *nbr, const double *B, const double *dB, int64_t n, int64_t n_s,
                                int32_t m, int32_t nrhs, const double *x, double *p, double *q, void *stream);

/* ---------------------------------------------------------------------------
 * Binomial / logistic latent posterior by Laplace approximation (pynngp_amd/latent_binomial.py; spNNGP's
 * family = "binomial" without the sampler -- the reference has no such model): s_i ~ Binomial(b_i, logistic(eta_i)),
 * eta_i = offset_i + w_i, w ~ NNGP.  A Newton / IRLS step at w is the Gaussian latent solve of the calls above with
 * d = W (the working weights) and the right-hand side below; the posterior mode is its fixed point.
 * Added within ABI revision 4 (nothing earlier moved).
 *
 * nngp_binomial_newton_step: one launch over the n nodes, one lane per node, and a one-block fold of its block
 *   records.  trials int32 (n,), 0 = no observation; successes, offset (= X beta), w: (n,).  With e = exp(-|eta_i|),
 *   p_i = 1 / (1 + e) for eta_i >= 0 and e / (1 + e) below, q_i = 1 - p_i the other of the two:
 *     d[i]   = W_i = b_i e / (1 + e)^2                      (= b_i p_i (1 - p_i); underflows to exactly 0 past |eta| ~ 745)
 *     g[i]   = s_i - b_i p_i = s_i q_i - (b_i - s_i) p_i    (the score in w_i)
 *     rhs[i] = W_i w_i + g[i]                               (weight times working response, the offset left out)
 *     l_i    = s_i eta_i - b_i log(1 + exp(eta_i)) = -(eta_i >= 0 ? b_i - s_i : s_i) |eta_i| - b_i log1p(e)
 *   evaluated as written, without fused multiply-adds: no cancellation and no overflow for any finite eta.
 *   trials[i] = 0: d = rhs = g = l = 0 exactly, whatever the other inputs hold (they are not read).
 *   partials (4 doubles): sum_i l_i; max_i |g[i]|; the first node whose eta is not finite, + 1, or 0; the first node
 *   whose trials are negative, + 1, or 0.  Faults are data, as nngp_polya_gamma's: such a node gets NaN in d, rhs and
 *   g and takes no part in the sum and the maximum; nothing traps.  The sum is a fixed-order fold (per-wave butterfly,
 *   waves in order, block records folded by one block in index order): the same bits on every call.
 *   workspace: nngp_binomial_newton_step_workspace_bytes(n) bytes (0 for a bad n), 256-B aligned.  0 <= n < 2^31 - 1.
 * nngp_binomial_check_partials: host helper on HOST-resident partials of a finished call: NNGP_OK, or NNGP_EINVAL
 *   with "negative trials at node k" / "offset + w is not finite at node k" in nngp_last_error (trials live on the
 *   device, so this is where a negative count is refused); the out-params (either may be NULL) receive the two
 *   nodes, -1 when there is none.
 * nngp_logistic_normal: out[i] = E[logistic(mu[i] + s[i] Z)], Z ~ N(0, 1): the probability-scale mean of a Gaussian
 *   latent value.  Trapezoid rule with step 1/16 on [-7, 7], 225 nodes for every element (no data-dependent loop).
 *   Absolute error <= 1e-11 for 0 <= s <= 13 and every mu (measured against 30-digit quadrature); beyond, the
 *   logistic's poles at distance pi / s from the real axis let it grow like exp(-316 / s): 2.5e-9 at s = 17, 3.5e-8
 *   at 20, 1.2e-5 at 34, 2e-3 at 100, never above 0.0125.  s = 0: logistic(mu), the link kernel's p to the last
 *   bit.  s < 0 or NaN, or mu NaN: NaN.
 * ------------------------------------------------------------------------- */
size_t nngp_binomial_newton_step_workspace_bytes(int64_t n);
int nngp_binomial_newton_step(int64_t n, const int32_t *trials, const double *successes, const double *offset,
                              const double *w, double *d, double *rhs, double *g, double *partials,
                              void *workspace, size_t workspace_bytes, void *stream);
int nngp_binomial_check_partials(const double *partials_host, int64_t *first_nonfinite,
                                 int64_t *first_negative_trials);
int nngp_logistic_normal(int64_t n, const double *mu, const double *s, double *out, void *stream);

/* ---------------------------------------------------------------------------
 * Solves with the NNGP factor, and what is composed from them (pynngp_amd/factor.py; the reference simulates its
 * fields with a dense Cholesky and has no such call).  With B (n, m) and F the factors of nngp_bf_sweep,
 *   forward     (I - B) x = b:     x_i = b_i + sum_{k = 0 .. m-1} B[i,k] x[nbr[i,k]]
 *   transposed  (I - B)^T x = b:   x_j = b_j + sum over j's reverse list of B[i,k] x_i   (B in reverse-list order
 *                                  from prep, as the second phase of nngp_precision_apply reads it)
 * over any neighbour array whose valid indices are smaller than their row's index: S = T, and the reference-set
 * layout whose leaves n_s .. n - 1 point into 0 .. n_s - 1.  A slot that is negative or >= its row's index is
 * ignored as -1 (a reverse entry whose child is not above its node likewise).  Added within ABI revision 4
 * (nothing earlier moved).
 * nngp_factor_levels (HOST arrays, no GPU, once per neighbour set: the schedule does not depend on theta):
 *   trans = 0: level(i) = 0 without a valid neighbour, else 1 + max level(nbr[i,k]); trans = 1: level(j) = 0 when
 *   no row lists j, else 1 + max level(i) over the rows i that list j.  level_host (n,): each row's level;
 *   rows_host (n,): the rows sorted by (level, index); level_off_host (n + 1 entries of room, n_levels + 1
 *   written): level l is rows_host[level_off_host[l] .. level_off_host[l + 1]); *n_levels: the depth (0 for n = 0).
 *   The same shape of record as nngp_gibbs_w_sweep's member_rows / color_off_host.  NNGP_EINVAL for trans outside
 *   {0, 1}, m outside 1 .. NNGP_MAX_M, n < 0.
 * nngp_factor_solve_batch: x = (I - B)^-1 b (trans = 0) or (I - B)^-T b (trans = 1); b, x (n, nrhs) row-major,
 *   1 <= nrhs <= NNGP_LATENT_MAX_RHS, and b and x may be the same buffer.  rows (DEVICE (n,)) and level_off (DEVICE
 *   (n_levels + 1,)) are copies of nngp_factor_levels' outputs for the same trans; level_off_host is the host
 *   copy, which steers the launches.  A level of more than fuse_width rows is one launch; a run of consecutive
 *   levels of at most fuse_width rows each is one launch of a single workgroup that walks them with a workgroup
 *   barrier in between (0 <= fuse_width <= NNGP_FACTOR_MAX_FUSE_WIDTH; 0: one launch per level).  Stream-ordered
 *   launches only, no atomics, no graph, no workspace; nngp_factor_launch_counts (host) gives their number.
 *   Every sum runs in slot order (reverse-list order), b first, one fused multiply-add per slot, in every
 *   column: x is bit-identical for every fuse_width and column c for every nrhs, whatever the other columns hold.
 *   off, rev_j and prep are read by the transposed solve only (NULL otherwise); rev_k is accepted for symmetry.
 * nngp_factor_cov_apply_batch: out = sigma2 (I - B)^-1 F (I - B)^-T v, the covariance of the NNGP prior (the
 *   inverse of nngp_precision_apply's matrix with d = NULL): a transposed solve, a scaling by sigma2 F, a forward
 *   solve, all in out; v and out may alias.  Both schedules are passed (suffix _f: trans = 0, _t: trans = 1).
 * nngp_factor_prior_draw_batch: out = (I - B)^-1 (sigma2 F)^1/2 z, nrhs draws from the prior.  z: (n, nrhs)
 *   standard normals, or NULL: column c is nngp_gibbs_normals(n, seed, sweep = draw0 + c), so draw number k is the
 *   same field in whatever batch it is drawn.  z and out may alias.
 * ------------------------------------------------------------------------- */
#define NNGP_FACTOR_MAX_FUSE_WIDTH 1024
int nngp_factor_levels(const int32_t *nbr_host, int64_t n, int32_t m, int32_t trans, int32_t *level_host,
                       int32_t *rows_host, int32_t *level_off_host, int64_t *n_levels);
int nngp_factor_launch_counts(const int32_t *level_off_host, int64_t n_levels, int32_t fuse_width, int64_t *n_wide,
                              int64_t *n_runs);
int nngp_factor_solve_batch(const int32_t *nbr, const double *B, const int32_t *off, const int32_t *rev_j,
                            const int32_t *rev_k, const void *prep, const int32_t *rows, const int32_t *level_off,
                            const int32_t *level_off_host, int64_t n_levels, int64_t n, int32_t m, int32_t nrhs,
                            int32_t trans, int32_t fuse_width, const double *b, double *x, void *stream);
int nngp_factor_cov_apply_batch(const int32_t *nbr, const double *B, const double *F, const int32_t *off,
                                const int32_t *rev_j, const int32_t *rev_k, const void *prep, const int32_t *rows_f,
                                const int32_t *level_off_f, const int32_t *level_off_f_host, int64_t n_levels_f,
                                const int32_t *rows_t, const int32_t *level_off_t, const int32_t *level_off_t_host,
                                int64_t n_levels_t, int64_t n, int32_t m, double sigma2, int32_t nrhs,
                                int32_t fuse_width, const double *v, double *out, void *stream);
int nngp_factor_prior_draw_batch(const int32_t *nbr, const double *B, const double *F, const int32_t *rows,
                                 const int32_t *level_off, const int32_t *level_off_host, int64_t n_levels, int64_t n,
                                 int32_t m, double sigma2, int32_t nrhs, int32_t fuse_width, const double *z,
                                 uint64_t seed, uint64_t draw0, double *out, void *stream);

/* ---------------------------------------------------------------------------
 * Whitening of several columns by a stored factor, and the Gram matrix of the result: the response-model
 * regression y = X beta + w + eps (pynngp_amd/regression.py; the reference has no mean model).  With
 * Q = (I - B)^T F^-1 (I - B) the NNGP precision and V = [y, X], G = U^T U for U = F^-1/2 (I - B) V holds y'Qy, X'Qy
 * and X'QX: GLS beta and its covariance, the profile and restricted likelihoods, universal kriging and the
 * conjugate NNGP (spNNGP's spConjNNGP) follow from it on the host.  Added within ABI revision 4 (nothing earlier
 * moved).
 *   U[t, c] = (self[t, c] - sum_s B[t,s] V[nbr[t,s], c]) / sqrt(F[t]),     G[a, b] = sum_t U[t,a] U[t,b]
 * nbr (n_rows, m), B (n_rows, m), F (n_rows,): exactly as nngp_bf_sweep, nngp_bf_cross or nngp_bf_sweep_blocks wrote
 * them (any kind, 1 <= m <= NNGP_MAX_M).  order: NULL, or the nngp_row_order layout -- row t of nbr is then local row
 * order[t], whose B, F, Vq and U rows are at order[t] (the sweeps write B and F at their natural rows); an order[t]
 * outside [0, n_rows) is skipped.  V (n_points, ncol) row-major: the columns being gathered.  Vq: NULL -- the S = T
 * sweep, the row's own values are V[i0 + row] (needs i0 + n_rows <= n_points) -- or (n_rows, ncol), the values at
 * query rows against a reference set (i0 unused).  U (n_rows, ncol): required; must not alias V or Vq.  gram: NULL
 * (whiten only) or (ncol, ncol) row-major, both triangles written.  1 <= ncol <= NNGP_WHITEN_MAX_COLS.
 * The sum runs in slot order, one fused multiply-add per slot, from 0; a slot that is negative or >= n_points adds
 * exactly 0; a row whose F is NaN or not positive gets NaN in U (numerical outcomes are data).  G is summed over
 * tiles of 1,024 rows -- in each, four chains over the rows = 0..3 mod 4 in row order, one fused multiply-add per
 * row, folded ((0 + 1) + (2 + 3)) -- and the tile records are folded in tile order by one block: an order that
 * depends on n_rows alone, no atomics.
 * THE CONTRACT: column c of U is bit-identical to the ncol = 1 call on that column; G[a, b] is bit-identical to the
 * entry of the ncol = 2 call on columns (a, b) alone, whatever the other columns hold (a NaN in column c touches
 * row c and column c of G only); every output is the same bits run to run, and U the same with or without gram.
 * workspace: nngp_whiten_gram_workspace_bytes(n_rows, ncol) bytes (0 for bad arguments), 256-B aligned, no
 * initialisation needed.  n_rows = 0: nothing is launched and gram is zeroed.  One stream-ordered launch with
 * gram = NULL, three otherwise.
 * ------------------------------------------------------------------------- */
#define NNGP_WHITEN_MAX_COLS 16
size_t nngp_whiten_gram_workspace_bytes(int64_t n_rows, int32_t ncol);
int nngp_whiten_gram(const int32_t *nbr, const int32_t *order, const double *B, const double *F, int64_t n_rows,
                     int32_t m, int64_t i0, int64_t n_points, int32_t ncol, const double *V, const double *Vq,
                     double *U, double *gram, void *workspace, size_t workspace_bytes, void *stream);

/* Host helper for callers that synchronise ("-2 means a non-positive
 * pivot; report the first bad index through an out-param"): given host-resident
 * partials of a finished sweep, returns NNGP_OK, NNGP_ENOTPD with *first_bad_row = the
 * first location whose pivot / F was not > 0, or NNGP_EINVAL with *first_bad_index = the
 * first location with an out-of-range neighbour index (either out-param may be NULL;
 * -1 when not applicable). */
int nngp_check_partials(const double *partials_host, int64_t *first_bad_row, int64_t *first_bad_index);

/* Host helper: -1/2 (n_rows log 2 pi + p[0] + p[1]) from host-resident partials. */
double nngp_loglik_from_partials(const double *partials_host, int64_t n_rows);

#ifdef __cplusplus
}
#endif
#endif /* NNGP_H */
