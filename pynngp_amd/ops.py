"""PyTorch-ROCm operators ``torch.ops.nngp.*`` (native: ``libnngp_torch_ops.so``).

The operators are registered in C++ with ``TORCH_LIBRARY(nngp, ...)``
(``pynngp_amd/csrc/torch_ops.cpp``) and implemented for the CUDA (= HIP on ROCm)
dispatch key only, straight over the C ABI of ``libnngp_hip.so`` on torch's current
stream: CPU tensors raise, there is no fallback.  :func:`load` (called by
``pynngp_amd.load_ops()`` and by the classes that sweep through these ops) loads the
library, loudly failing when it is not built, and registers the fake (meta) kernels used
for tracing.

    torch.ops.nngp.knn_prior(coords, m, q0, q1) -> nbr
    torch.ops.nngp.knn_prior_rows(coords, m, rows) -> nbr
    torch.ops.nngp.knn_query(ref, query, k) -> nbr
    torch.ops.nngp.bf_sweep(coords, nbr, i0, kind, sigma2, phi, tau2, values, want_bf, algo, order=None, nu=-1.0)
        -> (B, F, partials)
    torch.ops.nngp.bf_sweep_out(coords, nbr, order, i0, kind, sigma2, phi, tau2, values, B, F, R, partials,
                                workspace, algo, nu=-1.0, plan=None, plan_info=None, cert=None, cert_info=None)
        -> ()                                                         # the hot path: caller-owned buffers
    torch.ops.nngp.bf_fisher(coords, nbr, order, i0, kind, sigma2, phi, tau2, values, want_rows)
        -> (partials, grad, info, I_rows, G)   # Fisher information in (sigma2, phi, tau2); values None: info alone
    torch.ops.nngp.nbr_cert(coords, nbr, order, i0) -> (cert, cert_info)   # neighbour-set certificate (setup)
    torch.ops.nngp.pair_plan(nbr, order, i0, n_points, dim) -> (plan, plan_info)   # wave pair plan (setup)
    torch.ops.nngp.bf_cross(ref, query, nbr, kind, sigma2, phi, tau2, ref_values, algo, nu=-1.0) -> (B, F, mean)
    torch.ops.nngp.bf_sweep_noise(coords, nbr, order, i0, kind, sigma2, phi, tau2, values, noise_var, want_bf)
        -> (B, F, R, partials)   # per-point noise tau2 * noise_var[j]; B, F empty without want_bf, R without values
    torch.ops.nngp.bf_grad_noise(coords, nbr, order, i0, kind, sigma2, phi, tau2, values, noise_var, want_rows)
        -> (partials, grad, G)                                         # bf_grad of that model
    torch.ops.nngp.bf_cross_noise(ref, query, nbr, kind, sigma2, phi, tau2, ref_values, noise_ref, noise_query)
        -> (B, F, mean)                                                # bf_cross of that model; noise_query None: 1
    torch.ops.nngp.bf_sweep_sep(coords, nbr, order, i0, kind_s, kind_t, sigma2, phi_s, phi_t, tau2, values, want_bf)
        -> (B, F, R, partials)   # separable space x time (time in the last column); B, F empty without want_bf
    torch.ops.nngp.bf_grad_sep(coords, nbr, order, i0, kind_s, kind_t, sigma2, phi_s, phi_t, tau2, values, want_rows)
        -> (partials, grad, G)                                         # grad (4,), G (rows, 4): sigma2, phi_s, phi_t, tau2
    torch.ops.nngp.bf_cross_sep(ref, query, nbr, kind_s, kind_t, sigma2, phi_s, phi_t, tau2, ref_values)
        -> (B, F, mean)                                                # bf_cross of that model
    torch.ops.nngp.knn_prior_nd(coords, m, q0, q1) -> nbr              # 4 <= dim <= 16: exact, tiled brute force
    torch.ops.nngp.knn_query_nd(ref, query, k) -> nbr
    torch.ops.nngp.bf_sweep_nd(coords, nbr, order, i0, kind, sigma2, phi, tau2, values, want_bf)
        -> (B, F, R, partials)   # 4 <= dim <= 16, phi a list of dim decays (ARD); B, F empty without want_bf
    torch.ops.nngp.bf_grad_nd(coords, nbr, order, i0, kind, sigma2, phi, tau2, values, want_rows)
        -> (partials, grad, G)   # grad (dim + 2,), G (rows, dim + 2): sigma2, phi_1..phi_dim, tau2
    torch.ops.nngp.bf_cross_nd(ref, query, nbr, kind, sigma2, phi, tau2, ref_values) -> (B, F, mean)
    torch.ops.nngp.row_order(coords, i0, rows, nbr) -> (order, nbr_sorted)
    torch.ops.nngp.order_maxmin(coords, seed) -> (perm, level)   # levelled max-min order (a setup call: it
        # synchronises once per round); perm int64 (n,) position -> row, level int32 (n,) by position
    torch.ops.nngp.combine_partials_out(gathered, out) -> ()
    torch.ops.nngp.precision_apply(nbr, B, off, rev_j, rev_k, prep, sigma2, d, x) -> A x   # latent-field precision
    torch.ops.nngp.latent_cg(nbr, B, off, rev_j, rev_k, prep, sigma2, d, b, x0=None, rtol=1e-8, max_iter=1000,
                             check_every=8) -> (x, info)                 # Jacobi-PCG for A x = b (a solver call)
    torch.ops.nngp.precision_apply_batch(nbr, B, off, rev_j, rev_k, prep, sigma2, d, x) -> A x   # x (n, nrhs <= 8)
    torch.ops.nngp.factor_solve(nbr, B, off, rev_j, rev_k, prep, rows, level_off, level_off_host, trans, fuse_width,
                                b) -> x          # (I - B) x = b, or (I - B)^T x = b for trans; b (n, nrhs <= 8); the
        # schedule (rows, level_off on the device, level_off_host a CPU copy) from pynngp_amd._lib.factor_levels
    torch.ops.nngp.factor_cov_apply(nbr, B, F, off, rev_j, rev_k, prep, rows_f, level_off_f, level_off_f_host, rows_t,
                                    level_off_t, level_off_t_host, sigma2, fuse_width, v) -> sigma2 (I-B)^-1 F (I-B)^-T v
    torch.ops.nngp.latent_cg_batch(nbr, B, off, rev_j, rev_k, prep, sigma2, d, b, x0=None, rtol=1e-8, max_iter=1000,
                                   check_every=8) -> (x, info)           # nrhs solves in lock step, info (nrhs, 4)
    torch.ops.nngp.latent_cg_batch_trace(nbr, B, off, rev_j, rev_k, prep, sigma2, d, b, x0=None, rtol=1e-8,
                                         max_iter=1000, check_every=8) -> (x, info, trace)   # and the CG scalars:
        # trace (nrhs, max_iter, 2), NaN but for trace[c, k] = (alpha_k, beta_k) of the iterations column c completed
    torch.ops.nngp.whiten_gram(nbr, order, B, F, i0, V, Vq, want_gram) -> (U, G)   # U = F^-1/2 (I - B) V for V
        # (n_points, ncol <= 16) and G = U^T U ((0, 0) without want_gram); Vq: the rows' own values (query rows), or None
    torch.ops.nngp.polya_gamma(trials, c, seed, sweep) -> (omega, status)   # omega_i ~ PG(trials_i, c_i); status (1,)
        # int32: 0, or the smallest index + 1 whose draw is NaN (non-finite c, trials outside [0, 1024])
    torch.ops.nngp.binomial_newton_step(trials, successes, offset, w) -> (d, rhs, g, partials)   # the binomial
        # Laplace mode's link step: d = b p (1 - p), g = s - b p, rhs = d w + g at eta = offset + w; partials (4,) =
        # (sum log-lik terms, max |g|, first non-finite node + 1 or 0, first negative-trials node + 1 or 0)
    torch.ops.nngp.logistic_normal(mu, s) -> E[logistic(mu + s Z)], Z ~ N(0, 1)   # s = 0: logistic(mu)

``kind`` / ``algo`` are the integer codes of include/nngp.h (:func:`kind_code`, :func:`algo_code`);
``nu`` is the smoothness of the ``matern`` kind (0 < nu <= 50; ignored by the other kinds).
"""
from __future__ import annotations

import os

import torch

from . import _lib

_KINDS = tuple(_lib.KIND_CODES)  # code order: exponential, matern32, matern52, gaussian, spherical, matern
_ALGOS = dict(_lib.ALGO_CODES)
# always the in-tree build; it binds to whichever libnngp_hip.so _lib loaded first (matched by
# SONAME, so an NNGP_LIB variant build is the one the operators call)
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_build", "libnngp_torch_ops.so")

_loaded = False


def load() -> None:
    """Load the operator library once (it links libnngp_hip.so); raise if it is not built."""
    global _loaded
    if _loaded:
        return
    if not os.path.exists(LIB_PATH):
        raise _lib.NNGPExtensionError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(pynngp_amd has no CPU fallback)")
    _lib.load()  # the libnngp_hip.so the op library links (one copy in the process)
    torch.ops.load_library(LIB_PATH)
    _register_fakes()
    _loaded = True


def _register_fakes() -> None:
    def fake(name):
        return torch.library.register_fake(f"nngp::{name}")

    @fake("knn_prior")
    def _(coords, m, q0, q1):
        return coords.new_empty((q1 - q0, m), dtype=torch.int32)

    @fake("knn_prior_rows")
    def _(coords, m, rows):
        return coords.new_empty((rows.shape[0], m), dtype=torch.int32)

    @fake("knn_query")
    def _(ref, query, k):
        return query.new_empty((query.shape[0], k), dtype=torch.int32)

    @fake("bf_sweep")
    def _(coords, nbr, i0, kind, sigma2, phi, tau2, values, want_bf, algo, order=None, nu=-1.0):
        rows, m = nbr.shape
        if want_bf:
            return coords.new_empty((rows, m)), coords.new_empty((rows,)), coords.new_empty((4,))
        return coords.new_empty((0, m)), coords.new_empty((0,)), coords.new_empty((4,))

    @fake("bf_grad")
    def _(coords, nbr, order, i0, kind, sigma2, phi, tau2, values, want_rows):
        return (coords.new_empty((4,)), coords.new_empty((3,)),
                coords.new_empty((nbr.shape[0] if want_rows else 0, 3)))

    @fake("bf_grad_aniso")
    def _(coords, nbr, order, i0, kind, sigma2, phi, tau2, values, want_rows):
        k = coords.shape[1] + 2
        return (coords.new_empty((4,)), coords.new_empty((k,)),
                coords.new_empty((nbr.shape[0] if want_rows else 0, k)))

    @fake("bf_grad_matern")
    def _(coords, nbr, order, i0, sigma2, phi, tau2, nu, values, want_rows):
        return (coords.new_empty((4,)), coords.new_empty((4,)),
                coords.new_empty((nbr.shape[0] if want_rows else 0, 4)))

    @fake("matern_eval_d")
    def _(u, nu):
        return torch.empty_like(u), torch.empty_like(u)

    @fake("bf_fisher")
    def _(coords, nbr, order, i0, kind, sigma2, phi, tau2, values, want_rows):
        rows = nbr.shape[0] if want_rows else 0
        return (coords.new_empty((4,)), coords.new_empty((3,)), coords.new_empty((6,)), coords.new_empty((rows, 6)),
                coords.new_empty((rows, 3)))

    @fake("bf_sweep_out")
    def _(coords, nbr, order, i0, kind, sigma2, phi, tau2, values, B, F, R, partials, workspace, algo, nu=-1.0,
          plan=None, plan_info=None, cert=None, cert_info=None):
        return None

    @fake("nbr_cert")
    def _(coords, nbr, order, i0):
        raise RuntimeError("nbr_cert is a setup call (it synchronises to read its tile counts): build it eagerly")

    @fake("pair_plan")
    def _(nbr, order, i0, n_points, dim):
        raise RuntimeError("pair_plan is a setup call (it synchronises to read its tile counts): build it eagerly")

    @fake("bf_cross")
    def _(ref, query, nbr, kind, sigma2, phi, tau2, ref_values, algo, nu=-1.0):
        rows, m = nbr.shape
        return query.new_empty((rows, m)), query.new_empty((rows,)), query.new_empty((rows,))

    @fake("bf_sweep_noise")
    def _(coords, nbr, order, i0, kind, sigma2, phi, tau2, values, noise_var, want_bf):
        rows, m = nbr.shape
        return (coords.new_empty((rows if want_bf else 0, m)), coords.new_empty((rows if want_bf else 0,)),
                coords.new_empty((rows if values is not None else 0,)), coords.new_empty((4,)))

    @fake("bf_grad_noise")
    def _(coords, nbr, order, i0, kind, sigma2, phi, tau2, values, noise_var, want_rows):
        return (coords.new_empty((4,)), coords.new_empty((3,)),
                coords.new_empty((nbr.shape[0] if want_rows else 0, 3)))

    @fake("bf_cross_noise")
    def _(ref, query, nbr, kind, sigma2, phi, tau2, ref_values, noise_ref, noise_query):
        rows, m = nbr.shape
        return query.new_empty((rows, m)), query.new_empty((rows,)), query.new_empty((rows,))

    @fake("bf_sweep_sep")
    def _(coords, nbr, order, i0, kind_s, kind_t, sigma2, phi_s, phi_t, tau2, values, want_bf):
        rows, m = nbr.shape
        return (coords.new_empty((rows if want_bf else 0, m)), coords.new_empty((rows if want_bf else 0,)),
                coords.new_empty((rows if values is not None else 0,)), coords.new_empty((4,)))

    @fake("bf_grad_sep")
    def _(coords, nbr, order, i0, kind_s, kind_t, sigma2, phi_s, phi_t, tau2, values, want_rows):
        return (coords.new_empty((4,)), coords.new_empty((4,)),
                coords.new_empty((nbr.shape[0] if want_rows else 0, 4)))

    @fake("bf_cross_sep")
    def _(ref, query, nbr, kind_s, kind_t, sigma2, phi_s, phi_t, tau2, ref_values):
        rows, m = nbr.shape
        return query.new_empty((rows, m)), query.new_empty((rows,)), query.new_empty((rows,))

    @fake("knn_prior_nd")
    def _(coords, m, q0, q1):
        return coords.new_empty((q1 - q0, m), dtype=torch.int32)

    @fake("knn_query_nd")
    def _(ref, query, k):
        return ref.new_empty((query.shape[0], k), dtype=torch.int32)

    @fake("bf_sweep_nd")
    def _(coords, nbr, order, i0, kind, sigma2, phi, tau2, values, want_bf):
        rows, m = nbr.shape
        return (coords.new_empty((rows if want_bf else 0, m)), coords.new_empty((rows if want_bf else 0,)),
                coords.new_empty((rows if values is not None else 0,)), coords.new_empty((4,)))

    @fake("bf_grad_nd")
    def _(coords, nbr, order, i0, kind, sigma2, phi, tau2, values, want_rows):
        d = coords.shape[1]
        return (coords.new_empty((4,)), coords.new_empty((d + 2,)),
                coords.new_empty((nbr.shape[0] if want_rows else 0, d + 2)))

    @fake("bf_cross_nd")
    def _(ref, query, nbr, kind, sigma2, phi, tau2, ref_values):
        rows, m = nbr.shape
        return query.new_empty((rows, m)), query.new_empty((rows,)), query.new_empty((rows,))

    @fake("row_order")
    def _(coords, i0, rows, nbr):
        srt = torch.empty_like(nbr) if nbr is not None else coords.new_empty((0, 0), dtype=torch.int32)
        return coords.new_empty((rows,), dtype=torch.int32), srt

    @fake("order_maxmin")
    def _(coords, seed):
        n = coords.shape[0]
        return coords.new_empty((n,), dtype=torch.int64), coords.new_empty((n,), dtype=torch.int32)

    @fake("combine_partials_out")
    def _(gathered, out):
        return None

    @fake("precision_apply")
    def _(nbr, B, off, rev_j, rev_k, prep, sigma2, d, x):
        return torch.empty_like(x)

    @fake("latent_cg")
    def _(nbr, B, off, rev_j, rev_k, prep, sigma2, d, b, x0=None, rtol=1e-8, max_iter=1000, check_every=8):
        raise RuntimeError("latent_cg is a solver call (it synchronises once per chunk of iterations): run it eagerly")

    @fake("precision_apply_batch")
    def _(nbr, B, off, rev_j, rev_k, prep, sigma2, d, x):
        return torch.empty_like(x)

    @fake("factor_solve")
    def _(nbr, B, off, rev_j, rev_k, prep, rows, level_off, level_off_host, trans, fuse_width, b):
        return torch.empty_like(b)

    @fake("factor_cov_apply")
    def _(nbr, B, F, off, rev_j, rev_k, prep, rows_f, level_off_f, level_off_f_host, rows_t, level_off_t,
          level_off_t_host, sigma2, fuse_width, v):
        return torch.empty_like(v)

    @fake("latent_cg_batch")
    def _(nbr, B, off, rev_j, rev_k, prep, sigma2, d, b, x0=None, rtol=1e-8, max_iter=1000, check_every=8):
        raise RuntimeError("latent_cg_batch is a solver call (it synchronises once per chunk of iterations): run it "
                           "eagerly")

    @fake("latent_cg_batch_trace")
    def _(nbr, B, off, rev_j, rev_k, prep, sigma2, d, b, x0=None, rtol=1e-8, max_iter=1000, check_every=8):
        raise RuntimeError("latent_cg_batch_trace is a solver call (it synchronises once per chunk of iterations): "
                           "run it eagerly")

    @fake("whiten_gram")
    def _(nbr, order, B, F, i0, V, Vq, want_gram):
        ncol = V.shape[1]
        return V.new_empty((nbr.shape[0], ncol)), V.new_empty((ncol, ncol) if want_gram else (0, 0))

    @fake("polya_gamma")
    def _(trials, c, seed, sweep):
        return torch.empty_like(c), c.new_empty((1,), dtype=torch.int32)

    @fake("binomial_newton_step")
    def _(trials, successes, offset, w):
        return torch.empty_like(w), torch.empty_like(w), torch.empty_like(w), w.new_empty((4,))

    @fake("logistic_normal")
    def _(mu, s):
        return torch.empty_like(mu)


def kind_code(kind: str) -> int:
    try:
        return _KINDS.index(kind)
    except ValueError:
        raise ValueError(f"unknown covariance kind {kind!r}; expected one of {_KINDS}") from None


def algo_code(algo: str) -> int:
    try:
        return _ALGOS[algo]
    except KeyError:
        raise ValueError(f"unknown algo {algo!r}; expected one of {tuple(_ALGOS)}") from None


def bf_sweep_out(coords, nbr, order, i0, kind: str, theta, values, B, F, R, partials, workspace,
                 algo: str = "auto", plan=None, cert=None) -> None:
    """The fused sweep into caller-owned buffers through ``torch.ops.nngp.bf_sweep_out``
    (stream-ordered on torch's current stream, no host synchronisation).  ``theta`` =
    (sigma2, phi, tau2), or (sigma2, phi, tau2, nu) for the ``matern`` kind.  ``plan``: a
    ``(plan, plan_info)`` pair from :func:`pair_plan` for this nbr / order / i0.  ``cert``: a
    ``(cert, cert_info)`` pair from :func:`nbr_cert` for these coords / nbr / order / i0 (same bits, fewer
    instructions: trusted tiles skip the index checks and clamps)."""
    load()
    nu = float(theta[3]) if len(theta) > 3 else -1.0
    pbuf, pinfo = plan if plan is not None else (None, None)
    cbuf, cinfo = cert if cert is not None else (None, None)
    torch.ops.nngp.bf_sweep_out(coords, nbr, order, int(i0), kind_code(kind), float(theta[0]), float(theta[1]),
                                float(theta[2]), values, B, F, R, partials, workspace, algo_code(algo), nu, pbuf,
                                pinfo, cbuf, cinfo)


def bf_fisher(coords, nbr, order, i0: int, kind: str, theta, values=None, want_rows: bool = False):
    """The Fisher information sweep through ``torch.ops.nngp.bf_fisher`` (stream-ordered, no host
    synchronisation): ``(partials (4,), grad (3,), info (6,), I_rows, G)`` at ``theta`` = (sigma2, phi, tau2), the
    information's upper triangle in the order (ss, sp, st, pp, pt, tt); ``I_rows`` (rows, 6) and ``G`` (rows, 3) with
    ``want_rows``, else empty.  ``values=None``: the information alone (``grad`` exactly 0).  Kinds exponential ..
    spherical, 1 <= m <= 32; CPU tensors raise."""
    load()
    return torch.ops.nngp.bf_fisher(coords, nbr, order, int(i0), kind_code(kind), float(theta[0]), float(theta[1]),
                                    float(theta[2]), values, bool(want_rows))


def nbr_cert(coords, nbr, order, i0: int):
    """The neighbour-set certificate of a sweep over ``(coords, nbr, order, i0)`` (``torch.ops.nngp.nbr_cert``):
    ``(cert, cert_info)``.  A setup call (one host synchronisation).  The contract: coords, nbr and order are
    not modified afterwards (rebuild the certificate if they are)."""
    load()
    return torch.ops.nngp.nbr_cert(coords, nbr, order, int(i0))


def nbr_cert_trusted_tiles(cert_info, kind: str, theta) -> int:
    """Tiles a sweep of ``kind`` at ``theta`` = (sigma2, phi, tau2) runs trusted (``nngp_nbr_cert_trusted_tiles``,
    a host function): 0 when the distance clamp may bind or the kind is not one of the five fused ones."""
    import ctypes

    info = (ctypes.c_int64 * _lib.CERT_INFO_LEN)(*[int(v) for v in cert_info.tolist()])
    return int(_lib.load().nngp_nbr_cert_trusted_tiles(info, _lib.KIND_CODES.get(kind, 99), float(theta[0]),
                                                       float(theta[1]), float(theta[2])))


def cert_default() -> bool:
    """Whether models certify their neighbour sets at construction: on unless NNGP_NBR_CERT=0 (an A/B switch)."""
    return os.environ.get("NNGP_NBR_CERT", "1") != "0"


def pair_plan(nbr, order, i0: int, n_points: int, dim: int):
    """The wave pair plan of a sweep over ``nbr`` (``torch.ops.nngp.pair_plan``): ``(plan, plan_info)``.
    A setup call (one host synchronisation); stale once nbr or order change."""
    load()
    return torch.ops.nngp.pair_plan(nbr, order, int(i0), int(n_points), int(dim))


def pair_plan_supported(m: int, kind: str, dim: int) -> bool:
    return _lib.pair_plan_supported(m, kind, dim)

