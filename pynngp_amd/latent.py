"""``LatentPosterior``: the latent field w given noisy y at fixed (sigma2, phi, tau2), on the GPU.

The reference carries the latent state as ``ws`` / ``wt`` (pyNNGP/nngp.py:42-47) and names only a sampler for
it (``oneSample``, nngp.py:98-101).  Once theta is fixed -- e.g. by ``NNGP.fit`` -- the posterior of the
response model y = X beta + w + e, e_i ~ N(0, tau2 eps_i^2), w ~ NNGP(0, sigma2 R(phi)) is Gaussian and explicit:

    A = (I - B)^T (sigma2 F)^-1 (I - B) + diag(h / tau2),   b = h (y - X beta) / tau2,   h_i = 1 / eps_i^2
    w | y, theta ~ N(A^-1 b, A^-1)

(B, F the unit-variance factors of the fused sweep; h_i = 0 where y_i is NaN, i.e. unobserved).  A is sparse,
symmetric positive definite and never assembled: one product with it is two gathers (``nngp_precision_apply``),
the mean is a Jacobi-preconditioned conjugate-gradient solve (``nngp_latent_cg``, some tens of operator
applications instead of thousands of Gibbs sweeps), and exact draws come from the same solver by perturbation:
w = A^-1 (b + eta), eta = (I - B)^T (sigma2 F)^-1/2 z1 + (h / tau2)^1/2 z2 has covariance A.

A reference set (``ref=``; the reference's refType ('subset', nRef) / ('random', nRef, bounds)): the field
lives on the n_S points of S, and a data location outside S is a leaf whose parents are its m nearest points of S
(``SeqNNGP``'s node DAG).  A leaf is conditionally independent of everything else given w_S, so it is integrated
out in closed form instead of being carried through the solver: with f = 1 / (sigma2 F), d = h / tau2, v the
centred response and g_j = f_j d_j / (f_j + d_j) per leaf,

    A_S = (I - B_S)^T f_S (I - B_S) + d_S + B_L^T g B_L,   b_S = d_S v_S + B_L^T (g v_L)
    w_S | y ~ N(A_S^-1 b_S, A_S^-1),   w_j | w_S, y ~ N((f_j B_j w_S + d_j v_j) / (f_j + d_j), 1 / (f_j + d_j))

Every CG vector has n_S entries however many data locations hang off S (``nngp_precision_ref_*``,
``nngp_latent_ref_cg_batch``, ``nngp_latent_ref_leaves_batch``).  A prediction point is an unobserved leaf of the
same kind: :meth:`LatentPosterior.predict` gives the latent mean, its variance and draws at new locations for
both S = T and S != T.

How plausible theta is: :meth:`LatentPosterior.log_marginal` is log p(y | theta) of this latent model (not the
response model of ``NNGP.loglik``), for S = T and S != T alike.  Its quadratic form is one more solve, log det Q_S a
sum over F, and log det A_S comes from the solver itself: the Jacobi-PCG's alpha_k, beta_k are the Lanczos
tridiagonal of M^-1/2 A_S M^-1/2 (``nngp_latent_ref_cg_batch_trace`` records them), which turns every solve into a
Gauss quadrature (:func:`lanczos_quadrature`) and a handful of probe solves into log det A_S with a standard error
(stochastic Lanczos quadrature, :meth:`LatentPosterior.logdet`).  :meth:`LatentPosterior.fit` maximises it.
"""
from __future__ import annotations

import dataclasses
import math
import warnings
from typing import Optional

import numpy as np
import torch

from . import _lib
from .nngp import AnisotropicCovariance, Covariance, NNGPNumericalError, _default_device, _raise_on_bad

CHECK_EVERY = 8  # CG iterations between host synchronisations
DEFAULT_BATCH = _lib.LATENT_MAX_RHS  # right-hand sides per batched call where the caller does not say


@dataclasses.dataclass(frozen=True)
class SolveInfo:
    """Outcome of one CG solve: iterations done, ``converged``, and the squared norms of the final recurrence
    residual and of the right-hand side (the stopping rule is ``residual2 <= rtol^2 rhs2``)."""

    iterations: int
    converged: bool
    residual2: float
    rhs2: float


@dataclasses.dataclass(frozen=True)
class LogDet:
    """log det A_S by stochastic Lanczos quadrature: ``value`` = sum log diag(A_S) + the mean of ``per_probe``, its
    standard error ``se`` (the probes' sample standard deviation / sqrt(P); inf for one probe), the P estimates of
    z^T log(M^-1/2 A_S M^-1/2) z and the CG iterations each probe's quadrature rests on."""

    value: float
    se: float
    per_probe: np.ndarray
    iterations: np.ndarray


def lanczos_quadrature(alpha, beta, f=np.log) -> float:
    """e_1^T f(T) e_1 for the Lanczos tridiagonal T of a Jacobi-PCG solve's scalars alpha_0 .. alpha_k-1 and beta_0 ..
    (at least k - 1 of them; ``nngp_latent_ref_cg_batch_trace``):

        T[j, j] = 1 / alpha_j + beta_j-1 / alpha_j-1 (the second term absent at j = 0),  T[j, j+1] = sqrt(beta_j) / alpha_j.

    For the solve of A x = b from x = 0 with M = diag(A), |M^-1/2 b|^2 times this is the k-point Gauss quadrature of
    (M^-1/2 b)^T f(M^-1/2 A M^-1/2) (M^-1/2 b): f = 1 / t gives b^T x, f = log the log-determinant's probe term.  Host
    fp64 (``scipy.linalg.eigh_tridiagonal``); ``f`` maps an array of eigenvalues to an array."""
    a = np.asarray(alpha, dtype=np.float64).reshape(-1)
    b = np.asarray(beta, dtype=np.float64).reshape(-1)
    k = a.size
    if k < 1 or b.size < k - 1:
        raise ValueError(f"need k >= 1 alphas and at least k - 1 betas, got {k} and {b.size}")
    if not (np.all(np.isfinite(a)) and np.all(a > 0) and np.all(np.isfinite(b[:k - 1])) and np.all(b[:k - 1] >= 0)):
        raise ValueError("alpha must be positive and beta non-negative, all finite (an unwritten trace entry?)")
    diag = 1.0 / a
    diag[1:] += b[:k - 1] / a[:k - 1]
    if k == 1:
        return float(np.asarray(f(diag))[0])
    from scipy.linalg import eigh_tridiagonal

    w, V = eigh_tridiagonal(diag, np.sqrt(b[:k - 1]) / a[:k - 1])
    return float(np.sum(V[0] ** 2 * f(w)))


def _check_cov(cov) -> Covariance:
    if not isinstance(cov, Covariance):
        from .nngp import _refuse_sep

        _refuse_sep(cov, "LatentPosterior")
        if isinstance(cov, AnisotropicCovariance):
            raise TypeError("LatentPosterior does not serve an AnisotropicCovariance (per-axis ranges); it takes a "
                            "pynngp_amd.Covariance")
        if callable(cov):
            raise NotImplementedError("LatentPosterior takes a fused covariance kind (pynngp_amd.Covariance); a "
                                      "callable covariance is not served")
        raise TypeError(f"cov must be a pynngp_amd.Covariance, got {type(cov).__name__}")
    if not cov.tau2 > 0:
        raise ValueError("tau2 = 0: with noise-free data the posterior of w is the data itself (nothing to solve)")
    return cov


class LatentPosterior:
    """Posterior of the latent field on the data locations (S = T) at a fixed ``cov`` (see the module docstring).

    ``coords`` (N, d), 1 <= d <= 3; ``y`` (N,), NaN = unobserved; ``cov`` a :class:`Covariance` of any fused kind
    (exponential .. spherical, or ``matern`` with its ``nu``) with tau2 > 0; ``X`` (N, p) covariates or None (zero
    mean); ``eps`` per-location measurement sigmas (noise variance tau2 eps_i^2) or None; ``nbr``: prior neighbour
    sets to reuse (int32 (N, m) device tensor in the order of ``coords``), default: built here.

    Construction builds the neighbour sets, the unit-variance B / F, the reverse lists and the Gibbs ``prep``
    buffer once.  Internally every per-location array is kept in Z-order storage (as ``SeqNNGP``), so that the
    operator's gathers stay in cache; vectors go in and come out in the order of ``coords``.  Methods take and
    return numpy arrays, or device tensors when given device tensors.

    ``ref`` (n_S, d): the reference set S the field lives on (default None: S = T, the data locations).  The nodes
    are ``SeqNNGP``'s: the points of ``ref``, then the data locations outside it as leaves linked to their m
    nearest points of S (-1 padded when n_S < m); a data location that coincides with a reference point carries
    its observation on that node (``node_of_t`` maps data rows to nodes).  Storage holds the reference nodes in
    Z-order, then the leaves in Z-order.  The leaves are integrated out (module docstring): the vectors of
    :meth:`matvec` / :meth:`solve` / :meth:`solve_many` have n_S entries in the order of ``ref``, and field-valued
    results take ``where="data"`` (one value per row of ``coords``, the default) or ``where="ref"``.  ``X_ref``
    (n_S, p): covariates at S, accepted as ``SeqNNGP`` does; a node without an observation has no weight in any
    estimate here, so they change nothing.  ``nbr`` is for S = T only.
    """

    def __init__(self, coords, y, cov, m: int = 15, X=None, eps=None, device=None, nbr=None, ref=None, X_ref=None):
        cov = _check_cov(cov)
        self.m = int(m)
        if not 1 <= self.m <= _lib.MAX_M:
            raise ValueError(f"m={m} outside [1, {_lib.MAX_M}]")
        c_host = np.ascontiguousarray(coords.detach().cpu().numpy() if isinstance(coords, torch.Tensor) else coords,
                                      dtype=np.float64)
        if c_host.ndim == 1:
            c_host = c_host[:, None]
        if c_host.ndim != 2 or not 1 <= c_host.shape[1] <= _lib.MAX_DIM or c_host.shape[0] < 1:
            raise ValueError(f"coords must be (N >= 1, d) with 1 <= d <= {_lib.MAX_DIM}, got {c_host.shape}")
        if not np.all(np.isfinite(c_host)):
            raise ValueError("coords must be finite")
        n = c_host.shape[0]
        y_host = np.asarray(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y, dtype=np.float64)
        if y_host.shape != (n,):
            raise ValueError(f"y must hold one response per location ({n},), got {y_host.shape}")
        if np.any(np.isinf(y_host)):
            raise ValueError("y must be finite or NaN (NaN = unobserved)")
        observed = np.isfinite(y_host)
        if not observed.any():
            raise ValueError("no observed responses (y is all NaN)")
        if X is None:
            X_host = np.zeros((n, 0))
        else:
            X_host = np.asarray(X, dtype=np.float64)
            if X_host.ndim == 1:
                X_host = X_host[:, None]
            if X_host.ndim != 2 or X_host.shape[0] != n or not np.all(np.isfinite(X_host)):
                raise ValueError(f"X must be finite ({n}, p), got {X_host.shape}")
        if eps is None:
            h_host = np.ones(n)
        else:
            ev = np.asarray(eps, dtype=np.float64).reshape(-1)
            if ev.shape != (n,) or not np.all(np.isfinite(ev)) or not np.all(ev > 0):
                raise ValueError(f"eps must hold {n} positive finite measurement sigmas")
            h_host = 1.0 / ev ** 2
        h_host = np.where(observed, h_host, 0.0)
        if nbr is not None and (not isinstance(nbr, torch.Tensor) or nbr.dtype != torch.int32
                                or tuple(nbr.shape) != (n, self.m)):
            raise ValueError(f"nbr must be an int32 ({n}, {self.m}) device tensor")

        s_host = None
        if ref is not None:
            if nbr is not None:
                raise ValueError("nbr (prior neighbour sets of the data locations) is for S = T; with ref the "
                                 "neighbour sets are built on the reference set")
            s_host = np.ascontiguousarray(ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else ref,
                                          dtype=np.float64)
            if s_host.ndim == 1:
                s_host = s_host[:, None]
            if s_host.ndim != 2 or s_host.shape[0] < 1 or not np.all(np.isfinite(s_host)):
                raise ValueError(f"ref must be finite (n_S >= 1, d), got {s_host.shape}")
            if s_host.shape[1] != c_host.shape[1]:
                raise ValueError(f"reference set has dimension {s_host.shape[1]}, locations {c_host.shape[1]}")
            if X_ref is not None:
                xr = np.asarray(X_ref, dtype=np.float64)
                xr = xr[:, None] if xr.ndim == 1 else xr
                if xr.shape != (s_host.shape[0], X_host.shape[1]) or not np.all(np.isfinite(xr)):
                    raise ValueError(f"X_ref must be finite ({s_host.shape[0]}, {X_host.shape[1]}), got {xr.shape}")
        elif X_ref is not None:
            raise ValueError("X_ref needs ref")

        self.device = dev = _default_device(device)
        self.n, self.p = n, X_host.shape[1]
        to = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(dev)  # noqa: E731
        self._ref = s_host is not None  # the caller gave ref=: nothing below the constructor depends on it
        self._prior_in = (c_host, s_host, nbr)  # what sample_prior's NNGPFactor is built from, on first use
        self._prior = None
        if self._ref:
            coords0, nbr0, n_s, node_of_t = self._ref_nodes(to(c_host), to(s_host))
        else:  # S = T: the reference set is the data locations, and there is no leaf
            coords0, n_s, node_of_t = to(c_host), n, np.arange(n)
            nbr0 = _lib.knn_prior(coords0, self.m) if nbr is None else nbr.to(dev)
        # Z-order storage: slot s holds node perm[s], the reference nodes in the first n_s slots and the leaves
        # behind them; neighbour sets relabelled into storage labels
        n_nodes = coords0.shape[0]
        self.n_nodes, self.n_s = n_nodes, n_s
        self.node_of_t = node_of_t.astype(np.int64)  # node (reference points, then leaves) of each data row
        parts = [_lib.row_order(coords0[:n_s])[0].long()]
        if n_nodes > n_s:
            parts.append(_lib.row_order(coords0[n_s:])[0].long() + n_s)
        self.perm = torch.cat(parts)
        self.pos = torch.empty_like(self.perm)
        self.pos[self.perm] = torch.arange(n_nodes, device=dev)
        self.perm_s = self.perm[:n_s].contiguous()  # reference point held by storage slot s < n_s
        self.slot_of_ref = self.pos[:n_s].contiguous()
        self.slot_of_t = self.pos[torch.from_numpy(self.node_of_t).to(dev)]
        self.coords = coords0[self.perm].contiguous()
        nb = nbr0[self.perm].long()
        self.nbr = torch.where(nb >= 0, self.pos[nb.clamp(min=0)], -1).to(torch.int32).contiguous()
        self.off, self.rev_j, self.rev_k = _lib.reverse_neighbors(self.nbr)
        # a node's data: that of the data row it carries; none (h = 0) on a node without an observation
        h_n, y_n, X_n = np.zeros(n_nodes), np.zeros(n_nodes), np.zeros((n_nodes, self.p))
        h_n[node_of_t[observed]] = h_host[observed]
        y_n[node_of_t[observed]] = y_host[observed]
        X_n[node_of_t] = X_host
        self.h = to(h_n)[self.perm].contiguous()
        self.y = to(y_n)[self.perm].contiguous()
        self.X = to(X_n)[self.perm].contiguous()
        self.B = torch.empty((n_nodes, self.m), dtype=torch.float64, device=dev)
        self.F = torch.empty(n_nodes, dtype=torch.float64, device=dev)
        self._prep = None
        self._ws_batch = None  # the operator's and solver's workspace, made on first use for the widest chunk so far
        self.update(cov)

    def _ref_nodes(self, t_dev, s_dev):
        """The node DAG of a reference set, as ``SeqNNGP`` builds it (gibbs.py): ``(coords, nbr, n_s, node_of_t)``
        over the nodes [S; the data locations outside S]."""
        dev, n_s = self.device, s_dev.shape[0]
        nbr_s = _lib.knn_prior(s_dev, self.m)
        if n_s > 1:  # a repeated reference point makes C_N singular
            j1 = nbr_s[1:, 0].long()
            dup = torch.nonzero((s_dev[1:] == s_dev[j1]).all(dim=1)).flatten()
            if dup.numel() > 0:
                k = int(dup[0]) + 1
                raise ValueError(f"reference set point {k} repeats point {int(j1[k - 1])} (C_N would be singular; "
                                 "e.g. ('subset', nRef) draws with replacement)")
        # data locations that coincide with a reference point carry their data on that node
        j0 = _lib.knn_query(s_dev, t_dev, 1)[:, 0].long()
        hit = (t_dev == s_dev[j0]).all(dim=1).cpu().numpy()
        j0h = j0.cpu().numpy()
        if np.unique(j0h[hit]).size != int(hit.sum()):
            raise ValueError("two data locations coincide with the same reference point")
        out_idx = np.nonzero(~hit)[0]
        node_of_t = np.where(hit, j0h, 0)
        node_of_t[out_idx] = n_s + np.arange(out_idx.size)
        k = min(self.m, n_s)
        t_out = t_dev[torch.from_numpy(out_idx).to(dev)]
        nbr_t = (_lib.knn_query(s_dev, t_out, k) if out_idx.size
                 else torch.empty((0, k), dtype=torch.int32, device=dev))
        if k < self.m:
            nbr_t = torch.cat([nbr_t, torch.full((nbr_t.shape[0], self.m - k), -1, dtype=torch.int32, device=dev)],
                              dim=1)
        return torch.cat([s_dev, t_out]).contiguous(), torch.cat([nbr_s, nbr_t]).contiguous(), n_s, node_of_t

    # -- theta -----------------------------------------------------------------
    def update(self, cov) -> "LatentPosterior":
        """A new theta on the same neighbour sets: one B / F sweep and one ``prepare``."""
        cov = _check_cov(cov)
        _, _, p = _lib.bf_sweep(self.coords, self.nbr, 0, cov.kind, 1.0, cov.phi, 0.0, B=self.B, F=self.F,
                                nu=cov.nu_arg)
        _raise_on_bad(p.cpu().numpy())
        self._prep = _lib.gibbs_prepare(self.B, self.F, self.off, self.rev_j, self.rev_k, prep=self._prep)
        self.cov = cov
        self.d = (self.h / cov.tau2).contiguous()
        self._beta_hat = None
        return self

    # -- vectors in / out ------------------------------------------------------
    # The solver's vectors have one entry per reference point (S = T: per data location), in the caller's order.
    # Everything below is written for a reference set; S = T is the one whose nodes are the data locations, without
    # a leaf (n_nodes == n_s), which the library serves with the S = T launches.
    def _in(self, v, what="vector"):
        t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.array(v, dtype=np.float64))
        if t.dtype != torch.float64 or tuple(t.shape) != (self.n_s,):
            raise ValueError(f"{what} must be float64 ({self.n_s},), got {t.dtype} {tuple(t.shape)}")
        return t.to(self.device)[self.perm_s].contiguous()

    def _out(self, t, like):
        o = t[self.slot_of_ref]
        return o if isinstance(like, torch.Tensor) else o.cpu().numpy()

    def _rgeom(self):
        return (self.nbr, self.B, self.off, self.rev_j, self.rev_k, self._prep, self.n_s, self.cov.sigma2)

    def _geom(self):
        """The geometry without n_s, as the S = T library calls take it: all nodes as one S = T system."""
        return (self.nbr, self.B, self.off, self.rev_j, self.rev_k, self._prep, self.cov.sigma2)

    @staticmethod
    def _check_where(where):
        if where not in ("data", "ref"):
            raise ValueError(f"where must be 'data' or 'ref', got {where!r}")

    def _rows_of(self, where):
        """Storage slots of the rows a field-valued result reports (S = T: the same rows either way)."""
        return self.slot_of_t if where == "data" else self.slot_of_ref

    def _has_leaves(self):
        return self.n_nodes > self.n_s

    def _apply_cols(self, X):
        """A_S X for storage-order columns."""
        return _lib.precision_ref_apply_batch(*self._rgeom(), X, d=self.d, workspace=self._batch_ws(X.shape[1]))

    def _leaf_cols(self, XS, V=None, Z=None):
        """The leaves given the storage-order columns XS on S: conditional means (+ noise for normals Z)."""
        return _lib.latent_ref_leaves_batch(*self._rgeom(), XS, v=V, z=Z, d=self.d)

    def _node_cols(self, XS, V=None, Z=None):
        """(n_nodes, k) columns over all storage slots from the columns on S."""
        return torch.cat([XS, self._leaf_cols(XS, V, Z)]) if self._has_leaves() else XS

    def _yres(self, beta):
        return self.y if self.p == 0 else self.y - self.X @ torch.as_tensor(beta, dtype=torch.float64,
                                                                           device=self.device)

    def _leaf_v(self, beta, k):
        """The centred response on the leaves as k equal columns (the leaves kernel's v); None without leaves."""
        return self._yres(beta)[self.n_s:, None].expand(-1, k).contiguous() if self._has_leaves() else None

    # -- the operator and the solver -------------------------------------------
    def matvec(self, x):
        """A x (two gathers, bit-reproducible); with a reference set A_S x, x in the order of ``ref``."""
        return self._out(self._apply_cols(self._in(x, "x")[:, None])[:, 0], x)

    def _cg_args(self, rtol, max_iter):
        """The iteration cap of a solve, after the check of its rtol."""
        if not 0.0 < rtol < 1.0:
            raise ValueError(f"rtol must be in (0, 1), got {rtol}")
        return min(max(2 * self.n_s, 1000), 20000) if max_iter is None else max_iter

    def _solve(self, rhs, rtol, max_iter, x0=None):
        """Storage-order solve: (x, SolveInfo); raises on a breakdown, warns on non-convergence."""
        X, info = self._solve_cols(rhs[:, None], rtol, self._cg_args(rtol, max_iter),
                                   None if x0 is None else x0[:, None])
        x, info = X[:, 0], [float(v) for v in info[0]]
        if info[1] < 0:
            raise NNGPNumericalError(f"CG breakdown after {int(info[0])} iterations: p.Ap is not positive and finite "
                                     "(NaN or inf in the factors or the right-hand side?)")
        si = SolveInfo(int(info[0]), info[1] > 0, info[2], info[3])
        if not si.converged:
            warnings.warn(f"latent CG did not reach rtol={rtol:g} in {si.iterations} iterations "
                          f"(|r| / |b| = {math.sqrt(si.residual2 / si.rhs2) if si.rhs2 > 0 else float('nan'):.3g})",
                          RuntimeWarning, stacklevel=3)
        return x, si

    def solve(self, rhs, rtol: float = 1e-8, max_iter: Optional[int] = None, x0=None):
        """Solve A x = rhs by Jacobi-preconditioned CG: ``(x, info)``.  Stops at |r| <= rtol |rhs|.  Raises
        :class:`NNGPNumericalError` on a breakdown; warns with ``RuntimeWarning`` and returns
        ``info.converged = False`` when ``max_iter`` runs out first."""
        x, si = self._solve(self._in(rhs, "rhs"), rtol, max_iter, None if x0 is None else self._in(x0, "x0"))
        return self._out(x, rhs), si

    # -- several right-hand sides at once ---------------------------------------
    @staticmethod
    def _batch(batch) -> int:
        b = DEFAULT_BATCH if batch is None else int(batch)
        if not 1 <= b <= _lib.LATENT_MAX_RHS:
            raise ValueError(f"batch must be in [1, {_lib.LATENT_MAX_RHS}], got {batch}")
        return b

    def _batch_ws(self, nrhs):
        need = _lib.load().nngp_latent_ref_cg_batch_workspace_bytes(self.n_nodes, self.n_s, nrhs)
        if self._ws_batch is None or self._ws_batch.numel() < need:
            self._ws_batch = _lib._workspace(need, self.device)
        return self._ws_batch

    def _in_rows(self, v, what="rhs"):
        """(K, n_S) rows in the caller's order -> (K, n_S) device rows in storage order."""
        t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.array(v, dtype=np.float64))
        if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != self.n_s:
            raise ValueError(f"{what} must be float64 (K, {self.n_s}), got {t.dtype} {tuple(t.shape)}")
        return t.to(self.device)[:, self.perm_s]

    def _solve_cols(self, R, rtol, max_iter, X0=None, trace=None):
        """One batched solve of the storage-order columns R (n, k <= LATENT_MAX_RHS): (X, info (k, 4)).  ``trace``:
        a device (k, >= max_iter, 2) tensor that receives each column's (alpha, beta)."""
        X = torch.zeros_like(R) if X0 is None else X0.clone()
        if trace is not None:
            return _lib.latent_ref_cg_batch_trace(*self._rgeom(), R, X, d=self.d, rtol=rtol, max_iter=int(max_iter),
                                                  check_every=CHECK_EVERY, workspace=self._batch_ws(R.shape[1]),
                                                  trace=trace)
        return _lib.latent_ref_cg_batch(*self._rgeom(), R, X, d=self.d, rtol=rtol, max_iter=int(max_iter),
                                        check_every=CHECK_EVERY, workspace=self._batch_ws(R.shape[1]))

    def _report(self, info, rtol, first=0):
        """[SolveInfo] of the (K, 4) info rows (of the right-hand sides first, first + 1, ...); raises on a
        breakdown, warns once on non-convergence."""
        infos = [SolveInfo(int(r[0]), bool(r[1] > 0), float(r[2]), float(r[3])) for r in info]
        broken = [k for k, r in enumerate(info) if r[1] < 0]
        if broken:
            raise NNGPNumericalError(f"CG breakdown in column(s) {[first + k for k in broken]} after "
                                     f"{[infos[k].iterations for k in broken]} iterations: p.Ap is not positive and "
                                     "finite (NaN or inf in the factors or the right-hand side?)")
        slow = [k for k, si in enumerate(infos) if not si.converged]
        if slow:
            warnings.warn(f"latent CG did not reach rtol={rtol:g} in column(s) {[first + k for k in slow]} "
                          f"({[infos[k].iterations for k in slow]} iterations)", RuntimeWarning, stacklevel=3)
        return infos

    def _solve_rows(self, rows, rtol, max_iter, batch, x0=None):
        """Storage-order rows (K, n) on the device -> (solutions (K, n), info (K, 4)), ``batch`` columns per
        solve; the transposes stay on the device."""
        max_iter = self._cg_args(rtol, max_iter)
        K = rows.shape[0]
        out = torch.empty((K, self.n_s), dtype=torch.float64, device=self.device)
        info = np.zeros((K, 4))
        for k0 in range(0, K, batch):
            k1 = min(K, k0 + batch)
            X, info[k0:k1] = self._solve_cols(rows[k0:k1].t().contiguous(), rtol, max_iter,
                                              None if x0 is None else x0[k0:k1].t().contiguous())
            out[k0:k1] = X.t()
        return out, info

    def solve_many(self, rhs, rtol: float = 1e-8, max_iter: Optional[int] = None, x0=None, batch=None):
        """Solve A x_k = rhs[k] for the K >= 0 rows of ``rhs`` (K, N): ``(x (K, N), [SolveInfo] * K)``.  The rows
        go through the batched solver ``batch`` at a time (default ``LATENT_MAX_RHS``; every index and coefficient
        of A is read once per chunk instead of once per row), and row k equals ``solve(rhs[k])`` bit for bit.
        A breakdown raises :class:`NNGPNumericalError` naming the rows; rows that run out of ``max_iter`` are
        named in one ``RuntimeWarning``."""
        batch = self._batch(batch)
        rows = self._in_rows(rhs, "rhs")
        starts = None if x0 is None else self._in_rows(x0, "x0")
        if starts is not None and starts.shape != rows.shape:
            raise ValueError(f"x0 must have the shape of rhs {tuple(rows.shape)}, got {tuple(starts.shape)}")
        x, info = self._solve_rows(rows, rtol, max_iter, batch, starts)
        infos = self._report(info, rtol)
        x = x[:, self.slot_of_ref]
        return (x if isinstance(rhs, torch.Tensor) else x.cpu().numpy()), infos

    # -- posterior mean --------------------------------------------------------
    def _rhs(self, beta):
        return self._fold_cols(self._yres(beta)[:, None])[:, 0]

    def _fold_cols(self, V):
        """d_S V_S + B_L^T (g V_L) for storage-order columns V on all nodes: the right-hand sides on S.  Without
        leaves it is the product d V (the fold kernel's values, with the product's sign of a zero where d = 0, and
        two launches fewer)."""
        if not self._has_leaves():
            return (self.d[:, None] * V).contiguous()
        return _lib.precision_ref_fold_batch(*self._rgeom(), V.contiguous(), d=self.d,
                                             workspace=self._batch_ws(V.shape[1]))

    def gls_beta(self, rtol: float = 1e-8, max_iter: Optional[int] = None, batch=None) -> np.ndarray:
        """GLS beta under V = C~ + tau2 H^-1 (C~ the NNGP covariance): V^-1 v = H v / tau2 - H A^-1 H v / tau4,
        one solve per column of X, ``batch`` columns per batched solve; rows with h = 0 drop out."""
        if self.p == 0:
            return np.zeros(0)
        # A_aug^-1 (D v) = [x_S; leaf mean(x_S, v)] with x_S = A_S^-1 fold(v), per column v of X
        batch = self._batch(batch)
        max_iter = self._cg_args(rtol, max_iter)
        S = torch.empty_like(self.X)
        for k0 in range(0, self.p, batch):
            V = self.X[:, k0:k0 + batch].contiguous()
            XS, info = self._solve_cols(self._fold_cols(V), rtol, max_iter)
            self._report(info, rtol, first=k0)
            S[:, k0:k0 + batch] = self._node_cols(XS, V[self.n_s:].contiguous())
        W = self.d[:, None] * (self.X - S)  # V^-1 X
        G = (self.X.t() @ W).cpu().numpy()
        g = (W.t() @ self.y).cpu().numpy()
        return np.linalg.solve(0.5 * (G + G.T), g)

    def mean(self, beta=None, rtol: float = 1e-8, max_iter: Optional[int] = None, where: str = "data"):
        """Posterior mean ``(w_hat, beta_hat)``: w_hat = A^-1 h (y - X beta) / tau2 as a numpy array.  With ``X``
        and no ``beta``, beta_hat is the GLS estimate (:meth:`gls_beta`; p + 1 solves in all); without ``X`` it
        is empty.  With a reference set, ``where="data"`` gives the mean at every row of ``coords`` (a leaf's is its
        conditional mean given w_hat on S) and ``where="ref"`` the mean on S.  At new locations: :meth:`predict`."""
        self._check_where(where)
        if beta is None:
            beta = self._beta_hat = self.gls_beta(rtol, max_iter)
        beta = np.asarray(beta, dtype=np.float64).reshape(-1)
        if beta.shape != (self.p,):
            raise ValueError(f"beta must hold {self.p} coefficients")
        w, _ = self._solve(self._rhs(beta), rtol, max_iter)
        w = self._node_cols(w[:, None], self._leaf_v(beta, 1))[:, 0]
        return w[self._rows_of(where)].cpu().numpy(), beta

    # -- exact draws -----------------------------------------------------------
    def _beta_for_draws(self, beta, rtol, max_iter):
        if beta is None:
            beta = self._beta_hat if self._beta_hat is not None else self.gls_beta(rtol, max_iter)
            self._beta_hat = beta
        return np.asarray(beta, dtype=np.float64).reshape(-1)

    LEAF_STREAM = 1 << 40   # sweep index of draw k's third Philox stream (the leaves' conditional noise)
    QUERY_STREAM = 1 << 41  # ... of predict's conditional noise
    RESPONSE_STREAM = 3 << 40  # ... of predict's response noise (every stream is keyed by the draw's k alone)
    PROBE_STREAM = 1 << 42  # ... of logdet's probe k (its signs); no draw's stream

    def _nodes_in(self, a, n_draws, part):
        """Given test normals (n_draws, len) in model order -> storage-order device rows; part: "n" all nodes
        (reference points, then the data locations outside S in their order), "s" S, "l" the leaves."""
        size = {"n": self.n_nodes, "s": self.n_s, "l": self.n_nodes - self.n_s}[part]
        t = torch.from_numpy(np.asarray(a, dtype=np.float64).reshape(n_draws, size)).to(self.device)
        idx = {"n": self.perm, "s": self.perm_s, "l": self.perm[self.n_s:] - self.n_s}[part]
        return t[:, idx]

    def _draw_chunks(self, n_draws, seed, z, b, rtol, max_iter, batch):
        """Yields ``(k0, W)``: the draws k0 .. k0 + W.shape[1] - 1 of w_S as storage-order columns (n_s, k <= batch)
        on the device.  Draw k takes the Philox streams of sweep indices 2k and 2k + 1, whatever the chunking; z1
        has one normal per node, z2 one per reference point."""
        n, n_s = self.n_nodes, self.n_s
        if z is not None:
            z1, z2 = self._nodes_in(z[0], n_draws, "n"), self._nodes_in(z[1], n_draws, "s")
        zz1 = torch.empty(n, dtype=torch.float64, device=self.device)
        zz2 = torch.empty(n_s, dtype=torch.float64, device=self.device)
        for k0 in range(0, n_draws, batch):
            kc = min(batch, n_draws - k0)
            Z1 = torch.empty((n, kc), dtype=torch.float64, device=self.device)
            Z2 = torch.empty((n_s, kc), dtype=torch.float64, device=self.device)
            for c in range(kc):
                if z is None:
                    Z1[:, c] = _lib.gibbs_normals(zz1, seed, 2 * (k0 + c))
                    Z2[:, c] = _lib.gibbs_normals(zz2, seed, 2 * (k0 + c) + 1)
                else:
                    Z1[:, c], Z2[:, c] = z1[k0 + c], z2[k0 + c]
            eta = _lib.precision_ref_sqrt_t_apply_batch(*self._rgeom(), Z1, Z2, d=self.d,
                                                        workspace=self._batch_ws(kc))
            W, info = self._solve_rows((b[:, None] + eta).t(), rtol, max_iter, kc)
            self._report(info, rtol, first=k0)
            yield k0, W.t().contiguous()

    def _leaf_normals(self, k0, kc, n_draws, seed, z3, stream, size=None):
        """(size, kc) standard normals of draws k0 .. k0 + kc - 1: given rows, or Philox stream ``stream + k``."""
        size = self.n_nodes - self.n_s if size is None else size
        Z = torch.empty((size, kc), dtype=torch.float64, device=self.device)
        zz = torch.empty(size, dtype=torch.float64, device=self.device)
        for c in range(kc):
            Z[:, c] = z3[k0 + c] if z3 is not None else _lib.gibbs_normals(zz, seed, stream + k0 + c)
        return Z

    def sample(self, n_draws: int, seed: int = 0, z=None, beta=None, rtol: float = 1e-8,
               max_iter: Optional[int] = None, batch=None, where: str = "data") -> np.ndarray:
        """``(n_draws, N)`` exact posterior draws w = A^-1 (b + eta), eta = (I - B)^T (sigma2 F)^-1/2 z1 +
        (h / tau2)^1/2 z2, ``batch`` draws per batched square-root application and solve (default
        ``LATENT_MAX_RHS``; the draws do not depend on it).  The normals are Philox streams keyed by ``seed``
        (``nngp_gibbs_normals``; one seed repeats bit for bit), or ``z = (z1, z2)``, each (n_draws, N), for
        testing.  ``beta``: as :meth:`mean`.

        With a reference set the draws are of w_S (eta = (I - B_S)^T f_S^1/2 z1_S + B_L^T g^1/2 z1_L + d_S^1/2 z2),
        and every leaf adds its conditional noise from a third Philox stream per draw (streams 2k and 2k + 1 are
        those of S = T); ``where`` as :meth:`mean`; ``z = (z1 (n_draws, n_nodes), z2 (n_draws, n_S), z3 (n_draws,
        n_nodes - n_S))`` in node order (the points of ``ref``, then the data locations outside it)."""
        n_draws = int(n_draws)
        if n_draws < 0:
            raise ValueError("n_draws must be >= 0")
        batch = self._batch(batch)
        self._check_where(where)
        beta = self._beta_for_draws(beta, rtol, max_iter)
        b = self._rhs(beta)
        rows = self._rows_of(where)
        out = np.empty((n_draws, rows.shape[0]))
        leaves = where == "data" and self._has_leaves()
        z3 = self._nodes_in(z[2], n_draws, "l") if z is not None and self._has_leaves() else None
        for k0, W in self._draw_chunks(n_draws, seed, z, b, rtol, max_iter, batch):
            if leaves:
                kc = W.shape[1]
                W = self._node_cols(W, self._leaf_v(beta, kc),
                                    self._leaf_normals(k0, kc, n_draws, seed, z3, self.LEAF_STREAM))
            out[k0:k0 + W.shape[1]] = W[rows].t().cpu().numpy()
        return out

    def sample_prior(self, n_draws: int, seed: int = 0, where: str = "data") -> np.ndarray:
        """``(n_draws, N)`` draws of w from the NNGP PRIOR at ``cov`` (no data enter): w = (I - B)^-1 (sigma2 F)^1/2 z
        by the level-scheduled triangular solve of :class:`pynngp_amd.NNGPFactor`, built on first use on the same
        locations, neighbour-set rule and reference set, in the caller's order (not the Z-order storage, whose
        neighbours do not precede their rows).  With a reference set the leaves are drawn through the same DAG;
        ``where`` as :meth:`mean`.  Philox normals keyed by (``seed``, draw, node)."""
        self._check_where(where)
        from .factor import NNGPFactor

        c_host, s_host, nbr = self._prior_in
        if self._prior is None:
            self._prior = NNGPFactor(c_host, self.cov, m=self.m, nbr=nbr, device=self.device, ref=s_host)
        elif self._prior.cov != self.cov:
            self._prior.update(self.cov)
        if where == "data":
            return self._prior.sample_prior_at_data(n_draws, seed=seed)
        return self._prior.sample_prior(n_draws, seed=seed)[:, :self.n_s]

    # -- posterior uncertainty ---------------------------------------------------
    def marginal_variance(self, n_draws: int = 64, seed: int = 0, z=None, beta=None, rtol: float = 1e-8,
                          max_iter: Optional[int] = None, batch=None, where: str = "data") -> np.ndarray:
        """``(N,)`` posterior variances of w by the Rao-Blackwellised estimator over ``n_draws`` >= 2 exact draws.
        Given the rest of a draw w, w_i is Gaussian with mean c_i = w_i - (A w - b)_i / A_ii and variance 1 / A_ii,
        so Var(w_i | y) = 1 / A_ii + Var(c_i), estimated by

            v_i = 1 / A_ii + sum_k (c_i^(k) - c_bar_i)^2 / (K - 1).

        Only the second part carries Monte-Carlo error (relative standard deviation sqrt(2 / (K - 1)) of that
        part).  A w is one batched operator application per chunk of ``batch`` draws, A_ii comes from
        ``nngp_precision_diag``; the sums run on the device, draw by draw in draw order (shifted by the first
        draw's c, so nothing cancels), hence the result does not depend on ``batch``.  Arguments as :meth:`sample`.

        With a reference set the estimator above runs on A_S for the reference nodes; a leaf j, Gaussian given w_S
        with variance 1 / (f_j + d_j), gets v_j = 1 / (f_j + d_j) + the sample variance of its conditional mean
        over the draws of w_S (``z = (z1, z2)``: no leaf noise is drawn)."""
        n_draws = int(n_draws)
        if n_draws < 2:
            raise ValueError("marginal_variance needs n_draws >= 2")
        batch = self._batch(batch)
        self._check_where(where)
        beta = self._beta_for_draws(beta, rtol, max_iter)
        b = self._rhs(beta)
        base = aii = _lib.precision_ref_diag(*self._rgeom(), d=self.d, workspace=self._batch_ws(1))
        if self._has_leaves():
            base = torch.cat([aii, self.d[self.n_s:] + 1.0 / (self.cov.sigma2 * self.F[self.n_s:])])
        shift = None
        s1 = torch.zeros(self.n_nodes, dtype=torch.float64, device=self.device)
        s2 = torch.zeros_like(s1)
        for _, W in self._draw_chunks(n_draws, seed, z, b, rtol, max_iter, batch):
            AW = self._apply_cols(W)
            C = W - (AW - b[:, None]) / aii[:, None]
            if self._has_leaves():  # a leaf's conditional mean given this draw of w_S
                C = torch.cat([C, self._leaf_cols(W, self._leaf_v(beta, W.shape[1]))])
            if shift is None:
                shift = C[:, 0].clone()
            for c in range(C.shape[1]):
                dev = C[:, c] - shift
                s1 += dev
                s2 += dev * dev
        v = 1.0 / base + (s2 - s1 * s1 / n_draws) / (n_draws - 1)
        return v[self._rows_of(where)].cpu().numpy()

    # -- new locations -----------------------------------------------------------
    def predict(self, query, n_draws: int = 0, seed: int = 0, response: bool = False, beta=None, rtol: float = 1e-8,
                max_iter: Optional[int] = None, batch=None, z=None, zq=None):
        """The latent field at the points ``query`` (Q, d): ``(mean, var, draws)``.  A query point is an unobserved
        leaf of the reference set (S = T: of the data locations): its parents are its m nearest reference points
        (``nngp_knn_query``), its B_q / F_q the unit-variance factors without a nugget (``nngp_bf_cross``),
        factorised once per call, and all columns go through ``nngp_latent_ref_leaves_batch``, ``batch`` at a time.

        mean = B_q w_hat_S.  var = sigma2 F_q + the sample variance over the draws of B_q w_S^(k) (the law of total
        variance; None when n_draws < 2).  draws (n_draws, Q): B_q w_S^(k) + (sigma2 F_q)^1/2 z_k, exact draws of
        the latent field at the query points; ``response=True`` adds the noise of a new observation, tau2.  The
        draws of w_S are those of :meth:`sample` for this ``seed``; ``z`` as there, ``zq`` (n_draws, Q): given
        normals for the conditional noise (testing).  No covariate term is added: the mean is of w alone."""
        n_draws = int(n_draws)
        if n_draws < 0:
            raise ValueError("n_draws must be >= 0")
        batch = self._batch(batch)
        q_host = np.ascontiguousarray(query.detach().cpu().numpy() if isinstance(query, torch.Tensor) else query,
                                      dtype=np.float64)
        if q_host.ndim == 1:
            q_host = q_host[:, None]
        if q_host.ndim != 2 or q_host.shape[1] != self.coords.shape[1] or not np.all(np.isfinite(q_host)):
            raise ValueError(f"query must be finite (Q, {self.coords.shape[1]}), got {q_host.shape}")
        Q, n_s, dev, cov = q_host.shape[0], self.n_s, self.device, self.cov
        if zq is not None:
            zq = torch.from_numpy(np.asarray(zq, dtype=np.float64).reshape(n_draws, Q)).to(dev)
        beta = self._beta_for_draws(beta, rtol, max_iter)
        b = self._rhs(beta)
        w_hat, _ = self._solve(b, rtol, max_iter)
        if Q == 0:
            return np.zeros(0), (np.zeros(0) if n_draws >= 2 else None), np.zeros((n_draws, 0))
        # the prediction DAG: the query points as leaves of the reference points they name
        q = torch.from_numpy(q_host).to(dev)
        s_coords = self.coords[:n_s].contiguous()
        k = min(self.m, n_s)
        nbr_q = _lib.knn_query(s_coords, q, k)
        B_q, F_q, p = _lib.bf_cross(s_coords, q, nbr_q, cov.kind, 1.0, cov.phi, 0.0, nu=cov.nu_arg)
        _raise_on_bad(p.cpu().numpy())
        if k < self.m:
            nbr_q = torch.cat([nbr_q, torch.full((Q, self.m - k), -1, dtype=torch.int32, device=dev)], dim=1)
            B_q = torch.cat([B_q, torch.zeros((Q, self.m - k), dtype=torch.float64, device=dev)], dim=1)
        # The leaves call reads a leaf row's nbr / B / invF and x at its parents, nothing of the reference rows: the
        # DAG handed to it keeps only the u <= Q m distinct parents, as parentless nodes, and x is gathered to them.
        # Its size, and that of its reverse lists and prep, does not depend on n_S; a row's slots, hence its sum,
        # are what they would be over all of S.
        valid = nbr_q >= 0
        parents, inv = torch.unique(nbr_q[valid].long(), return_inverse=True)
        n_u = parents.numel()
        nbr_c = torch.full_like(nbr_q, -1)
        nbr_c[valid] = inv.to(torch.int32)
        nbr_a = torch.cat([torch.full((n_u, self.m), -1, dtype=torch.int32, device=dev), nbr_c]).contiguous()
        B_a = torch.cat([torch.zeros((n_u, self.m), dtype=torch.float64, device=dev), B_q]).contiguous()
        F_a = torch.cat([torch.ones(n_u, dtype=torch.float64, device=dev), F_q]).contiguous()
        off, rev_j, rev_k = _lib.reverse_neighbors(nbr_a)
        prep = _lib.gibbs_prepare(B_a, F_a, off, rev_j, rev_k)
        geom = (nbr_a, B_a, off, rev_j, rev_k, prep, n_u, cov.sigma2)
        mean = _lib.latent_ref_leaves_batch(*geom, w_hat[parents][:, None].contiguous())[:, 0].cpu().numpy()
        draws = np.empty((n_draws, Q))
        shift = None
        s1 = torch.zeros(Q, dtype=torch.float64, device=dev)
        s2 = torch.zeros_like(s1)
        for k0, W in self._draw_chunks(n_draws, seed, z, b, rtol, max_iter, batch):
            kc = W.shape[1]
            W = W[parents].contiguous()
            M = _lib.latent_ref_leaves_batch(*geom, W)  # B_q w_S^(k)
            D = _lib.latent_ref_leaves_batch(*geom, W, z=self._leaf_normals(k0, kc, n_draws, seed, zq,
                                                                           self.QUERY_STREAM, size=Q))
            if response:
                D = D + math.sqrt(cov.tau2) * self._leaf_normals(k0, kc, n_draws, seed, None,
                                                                 self.RESPONSE_STREAM, size=Q)
            draws[k0:k0 + kc] = D.t().cpu().numpy()
            if shift is None:
                shift = M[:, 0].clone()
            for c in range(kc):
                dev_c = M[:, c] - shift
                s1 += dev_c
                s2 += dev_c * dev_c
        var = None
        if n_draws >= 2:
            var = (cov.sigma2 * F_q + (s2 - s1 * s1 / n_draws) / (n_draws - 1)).cpu().numpy()
        return mean, var, draws

    # -- the marginal likelihood of theta ------------------------------------------
    def _probe_rows(self, n_probes, seed, z):
        """(P, n_S) storage-order probes on the device: the given rows ``z`` (model order), else Rademacher signs --
        those of the Philox normals of stream ``PROBE_STREAM + k``, so probe k depends on (seed, k) alone."""
        if z is not None:
            return self._in_rows(z, "z").contiguous()
        n_probes = int(n_probes)
        if n_probes < 1:
            raise ValueError("n_probes must be >= 1")
        Z = torch.empty((n_probes, self.n_s), dtype=torch.float64, device=self.device)
        zz = torch.empty(self.n_s, dtype=torch.float64, device=self.device)
        one = torch.ones((), dtype=torch.float64, device=self.device)
        for k in range(n_probes):
            Z[k] = torch.where(_lib.gibbs_normals(zz, seed, self.PROBE_STREAM + k) < 0, -one, one)
        return Z

    def logdet(self, n_probes: int = 32, seed: int = 0, z=None, rtol: float = 1e-6, max_iter: Optional[int] = None,
               batch=None) -> LogDet:
        """log det A_S by stochastic Lanczos quadrature on the solver's own scalars (:class:`LogDet`).  With M =
        diag(A_S) and A^ = M^-1/2 A_S M^-1/2,

            log det A_S = sum_i log M_ii + E_z[z^T log(A^) z]      for probes with E z z^T = I,

        and one Jacobi-PCG solve of A_S x = M^1/2 z from x = 0 yields z^T log(A^) z ~ z^T z e_1^T log(T) e_1, T the
        Lanczos tridiagonal its alpha_k, beta_k spell (:func:`lanczos_quadrature`; the solution itself is not used).
        The probes go through the batched solver ``batch`` at a time (default ``LATENT_MAX_RHS``) with a trace;
        the quadrature uses the iterations a column completed, to ``rtol`` -- a Gauss quadrature's error is of the
        order of the squared residual, hence the loose default.  Probes: Rademacher signs from the Philox stream of
        (``seed``, probe index) alone, so the result depends neither on ``batch`` nor on the run; or the rows of
        ``z`` (P, n_S) in the order of ``ref`` (S = T: of ``coords``), each weighted by its z^T z -- the n_S rows of
        sqrt(n_S) I give the trace exactly.  A breakdown raises, a probe that ran out of ``max_iter`` is named in a
        ``RuntimeWarning`` (its quadrature then rests on ``max_iter`` points)."""
        return self._logdet_run(n_probes, seed, z, rtol, max_iter, batch)

    def _logdet_run(self, n_probes, seed, z, rtol, max_iter, batch, visit=None):
        """:meth:`logdet`'s loop.  ``visit(k0, Zc, root, X)``, when given, sees every chunk after its solve: the
        probes Zc (k, n_S) of rows k0 .. k0 + k - 1, root = diag(A_S)^1/2 and the solutions X (n_S, k) of A_S x =
        M^1/2 z -- the vectors a Hutchinson estimate of tr(A_S^-1 dA_S) needs (:meth:`log_marginal_grad`).  It takes
        no part in the log-determinant: the result is the same bits with or without it."""
        batch = self._batch(batch)
        max_iter = int(self._cg_args(rtol, max_iter))
        Z = self._probe_rows(n_probes, seed, z)
        P = Z.shape[0]
        if P < 1:
            raise ValueError("logdet needs at least one probe")
        diag = _lib.precision_ref_diag(*self._rgeom(), d=self.d, workspace=self._batch_ws(1))
        root = torch.sqrt(diag)
        weight = (Z * Z).sum(dim=1).cpu().numpy()
        per, info = np.zeros(P), np.zeros((P, 4))
        trace = torch.empty((min(batch, P), max_iter, 2), dtype=torch.float64, device=self.device)
        for k0 in range(0, P, batch):
            k1 = min(P, k0 + batch)
            tr = trace[:k1 - k0]
            tr.fill_(float("nan"))
            X, info[k0:k1] = self._solve_cols((Z[k0:k1] * root).t().contiguous(), rtol, max_iter, trace=tr)
            self._report(info[k0:k1], rtol, first=k0)
            if visit is not None:
                visit(k0, Z[k0:k1], root, X)
            its = info[k0:k1, 0].astype(np.int64)
            host = tr[:, :max(int(its.max()), 1)].cpu().numpy()
            for c, it in enumerate(its):
                if it > 0:  # no iteration: a zero probe, whose term is 0
                    per[k0 + c] = weight[k0 + c] * lanczos_quadrature(host[c, :it, 0], host[c, :it, 1])
        se = float(per.std(ddof=1) / math.sqrt(P)) if P > 1 else math.inf
        return LogDet(float(torch.log(diag).sum()) + float(per.mean()), se, per, info[:, 0].astype(np.int64))

    def log_marginal(self, beta=None, n_probes: int = 32, seed: int = 0, z=None, rtol: float = 1e-8,
                     max_iter: Optional[int] = None, batch=None, logdet_rtol: float = 1e-6):
        """``(value, se)``: log p(y | theta) of the latent model y = X beta + w + e at this theta, the field on S
        and the leaves integrated out.  With v the centred response, f = 1 / (sigma2 F), d = h / tau2 (0 where
        unobserved), g_j = f_j d_j / (f_j + d_j) per leaf and n_obs the nodes with d > 0,

            -2 log p = n_obs log 2 pi - sum_{S, d>0} log d_i - sum_{L, d>0} log g_j - sum_S log f_i + log det A_S
                       + (sum_S d_i v_i^2 + sum_L g_j v_j^2) - b_S^T A_S^-1 b_S,

        for S = T the dense log N(v; 0, Q^-1 + diag(1 / d)) on the observed rows.  The quadratic form is one solve
        to ``rtol``; log det A_S is :meth:`logdet` (``n_probes``, ``seed``, ``z``, ``batch``, ``logdet_rtol``), whose
        standard error, halved, is ``se`` -- everything else is exact to rounding.  With covariates and no ``beta``,
        v = y - X beta_hat with the GLS estimate (:meth:`gls_beta`): a plug-in (profiled) likelihood, not one with
        beta integrated out."""
        return self._log_marginal_run(beta, n_probes, seed, z, rtol, max_iter, batch, logdet_rtol)[:2]

    def _log_marginal_run(self, beta, n_probes, seed, z, rtol, max_iter, batch, logdet_rtol, visit=None, mean=None):
        """:meth:`log_marginal`: ``(value, se)``.  ``mean(v, x)`` sees the centred response and the mean solve's
        solution before the probes run, ``visit`` is :meth:`_logdet_run`'s; neither changes a bit of the value."""
        beta = self._beta_for_draws(beta, rtol, max_iter)
        if beta.shape != (self.p,):
            raise ValueError(f"beta must hold {self.p} coefficients")
        n_s = self.n_s
        v = self._yres(beta)
        b = self._rhs(beta)
        x, _ = self._solve(b, rtol, max_iter)
        if mean is not None:
            mean(v, x)
        d, f = self.d, 1.0 / (self.cov.sigma2 * self.F)
        obs = d > 0
        one = torch.ones_like(d)
        terms = -torch.log(torch.where(obs[:n_s], d[:n_s], one[:n_s])).sum() - torch.log(f[:n_s]).sum()
        quad = (d[:n_s] * v[:n_s] * v[:n_s]).sum() - torch.dot(b, x)
        if self._has_leaves():
            fl, dl, ol = f[n_s:], d[n_s:], obs[n_s:]
            g = torch.where(ol, fl * dl / (fl + dl), torch.zeros_like(dl))
            terms = terms - torch.log(torch.where(ol, g, one[n_s:])).sum()
            quad = quad + (g * v[n_s:] * v[n_s:]).sum()
        ld = self._logdet_run(n_probes, seed, z, logdet_rtol, max_iter, batch, visit)
        m2 = int(obs.sum()) * math.log(2.0 * math.pi) + float(terms) + ld.value + float(quad)
        return -0.5 * m2, 0.5 * ld.se

    GRAD_MAX_M = _lib.GRAD_MAX_M  # the phi-derivative sweep's range of m

    def _check_grad(self, cov):
        """The gradient's coverage, checked before any device work."""
        if cov.kind == "matern":
            raise ValueError("the gradient of the latent marginal likelihood serves the kinds exponential .. "
                             "spherical, not the general-nu matern kind")
        if self.m > self.GRAD_MAX_M:
            raise ValueError(f"the gradient of the latent marginal likelihood serves m <= {self.GRAD_MAX_M} "
                             f"(m={self.m})")

    def _grad_rows(self):
        """Per-row derivatives of (f_S, d_S, g_L) in (sigma2, phi, tau2) at the current theta, the phi-derivative
        of B, and the log terms' derivative: one ``nngp_bf_dphi`` sweep plus elementwise work."""
        cov, n_s = self.cov, self.n_s
        _, _, dB, dF, p = _lib.bf_dphi(self.coords, self.nbr, 0, cov.kind, 1.0, cov.phi, 0.0)
        _raise_on_bad(p.cpu().numpy())
        d, f = self.d, 1.0 / (cov.sigma2 * self.F)
        obs = d > 0
        zero, one = torch.zeros_like(d), torch.ones_like(d)
        df_all = (-f / cov.sigma2, -f * dF / self.F, zero)  # d f / d (sigma2, phi, tau2), every node
        dd_all = (zero, zero, -d / cov.tau2)
        rows = []
        for df, dd in zip(df_all, dd_all):
            fl, dl, ol = f[n_s:], d[n_s:], obs[n_s:]
            den = (fl + dl) * (fl + dl)
            dg = torch.where(ol, (df[n_s:] * dl * dl + dd[n_s:] * fl * fl) / den, zero[n_s:])
            g = torch.where(ol, fl * dl / (fl + dl), zero[n_s:])
            logs = (torch.where(obs[:n_s], dd[:n_s] / torch.where(obs[:n_s], d[:n_s], one[:n_s]), zero[:n_s]).sum()
                    + (df[:n_s] / f[:n_s]).sum() + torch.where(ol, dg / torch.where(ol, g, one[n_s:]), zero[n_s:]).sum())
            rows.append({"df": df[:n_s].contiguous(), "dd": dd[:n_s].contiguous(), "dg": dg, "logs": logs})
        fl, dl, ol = f[n_s:], d[n_s:], obs[n_s:]
        return dB, f[:n_s].contiguous(), torch.where(ol, fl * dl / (fl + dl), zero[n_s:]), rows

    def _grad_bilinear(self, dB, fS, g, rows, X, Y):
        """(3, k): column c holds X[:, c]^T (dA_S / d theta) Y[:, c] for theta = sigma2, phi, tau2 (module docstring
        of the gradient: DESIGN 4.6d), X and Y storage-order columns (n_S, k).  Also returns the two gathers of X."""
        n_s = self.n_s
        PX, QX = _lib.latent_rows_dot2_batch(self.nbr, self.B, dB, n_s, X.contiguous())
        if Y is X:
            PY, QY = PX, QX
        else:
            PY, QY = _lib.latent_rows_dot2_batch(self.nbr, self.B, dB, n_s, Y.contiguous())
        eX, eY = X - PX[:n_s], Y - PY[:n_s]
        pX, pY, qX, qY = PX[n_s:], PY[n_s:], QX[n_s:], QY[n_s:]
        out = []
        for k, r in enumerate(rows):
            tS = r["df"][:, None] * eX * eY + r["dd"][:, None] * X * Y
            tL = r["dg"][:, None] * pX * pY
            if k == 1:  # phi moves B as well
                tS = tS - fS[:, None] * (QX[:n_s] * eY + eX * QY[:n_s])
                tL = tL + g[:, None] * (qX * pY + pX * qY)
            out.append(self._col_sums(tS) + self._col_sums(tL))
        return torch.stack(out), (pX, qX)

    @staticmethod
    def _col_sums(T):
        """(k,) column sums of T (rows, k), each column summed on its own as a fresh contiguous vector: a column's
        sum then depends on neither k nor the other columns (a reduction over dim 0 picks its order by shape)."""
        return torch.stack([T[:, c].clone().sum() for c in range(T.shape[1])])

    def log_marginal_grad(self, beta=None, n_probes: int = 32, seed: int = 0, z=None, rtol: float = 1e-8,
                          max_iter: Optional[int] = None, batch=None, logdet_rtol: float = 1e-6):
        """``(value, se, grad, grad_se)``: :meth:`log_marginal` and its gradient in (sigma2, phi, tau2).  ``value`` and
        ``se`` are that method's at the same arguments, bit for bit, from the same solves: the gradient adds one
        ``nngp_bf_dphi`` sweep (dB / dphi, dF / dphi per row) and a few two-weight gathers
        (``nngp_latent_rows_dot2_batch``), no solve.  With x = A_S^-1 b_S and the row derivatives of f, d, g and B,

            d(-2 log p) = - sum dlog d - sum dlog g - sum_S dlog f + tr(A_S^-1 dA_S)
                          + sum_S dd v^2 + sum_L dg v^2 - 2 db_S^T x + x^T dA_S x,

        every term but the trace exact to rounding.  The trace is a Hutchinson estimate on the log-determinant's own
        probes: the solutions s_k of A_S s = M^1/2 z_k that :meth:`logdet` computes give s_k^T dA_S (M^-1/2 z_k), whose
        mean over the probes is the estimate and whose sample standard deviation / sqrt(P), halved, is ``grad_se``
        (inf for one probe).  The n_S rows of sqrt(n_S) I as ``z`` make it exact.  ``grad`` and ``grad_se`` are numpy
        (3,) arrays.  The probes are solved to ``logdet_rtol``, which bounds the trace's solver error.

        With covariates and no ``beta``, beta_hat is the GLS estimate, which maximises this likelihood in beta at
        theta: the gradient of the profiled value is the partial gradient at beta_hat held fixed (the envelope
        theorem), so no d beta_hat / d theta term appears.  Kinds exponential .. spherical, m <= 32 (``ValueError``
        otherwise, before any device work)."""
        self._check_grad(self.cov)
        n_s = self.n_s
        dB, fS, g, rows = self._grad_rows()
        acc = {"tr": []}

        def mean(v, x):
            X = x[:, None]
            bil, (pX, qX) = self._grad_bilinear(dB, fS, g, rows, X, X)
            vS, vL = v[:n_s], v[n_s:]
            fixed = []
            for k, r in enumerate(rows):
                db_x = (r["dd"] * vS * x).sum() + (vL * r["dg"] * pX[:, 0]).sum()
                if k == 1:
                    db_x = db_x + (vL * g * qX[:, 0]).sum()
                fixed.append(-r["logs"] + (r["dd"] * vS * vS).sum() + (r["dg"] * vL * vL).sum() - 2.0 * db_x
                             + bil[k, 0])
            acc["fixed"] = torch.stack(fixed)

        def visit(k0, Zc, root, X):
            W = (Zc / root).t().contiguous()
            acc["tr"].append(self._grad_bilinear(dB, fS, g, rows, X, W)[0])

        value, se = self._log_marginal_run(beta, n_probes, seed, z, rtol, max_iter, batch, logdet_rtol, visit, mean)
        per = torch.cat(acc["tr"], dim=1).cpu().numpy()  # (3, P)
        P = per.shape[1]
        tr = per.mean(axis=1)
        tr_se = per.std(axis=1, ddof=1) / math.sqrt(P) if P > 1 else np.full(3, math.inf)
        grad = -0.5 * (acc["fixed"].cpu().numpy() + tr)
        return value, se, grad, 0.5 * tr_se

    def fit(self, x0=None, fix_tau2: Optional[float] = None, n_probes: int = 32, seed: int = 0,
            method: Optional[str] = None, maxiter: int = 200, z=None, rtol: float = 1e-8, batch=None,
            gradient: bool = False):
        """Empirical-Bayes theta: maximise :meth:`log_marginal` over log (sigma2, phi, tau2) (``fix_tau2``: over log
        (sigma2, phi) at that nugget) from ``x0`` -- a :class:`Covariance` of this kind or (sigma2, phi, tau2),
        default the current ``cov``.  Every evaluation uses the same probes (common random numbers), so the
        objective is a deterministic function of theta; theta moves by :meth:`update` on the same neighbour sets,
        and beta, with covariates, is re-estimated by GLS at each theta.  Derivative-free by default
        (``scipy.optimize.minimize``, ``method`` -- Nelder-Mead unless given --, at most ``maxiter`` iterations).
        Leaves the object at the best theta seen and returns ``(cov, result)``: the fitted :class:`Covariance` and the
        optimiser's result (``result.fun`` = -log_marginal there).

        ``gradient=True``: every evaluation is :meth:`log_marginal_grad`, chain-ruled to log theta (d / d log theta_i
        = theta_i d / d theta_i), and the default method is L-BFGS-B.  With Rademacher probes the value is a
        stochastic-Lanczos-quadrature estimate and the gradient a Hutchinson estimate on the same probes: both are
        deterministic functions of theta, but they agree only up to probe noise, so the line search may stop on
        noise of the order of ``se``.  With basis probes (``z`` = the rows of sqrt(n_S) I) they agree exactly.  The
        general-nu ``matern`` kind (and m > 32) has no gradient: ``ValueError`` before any device work."""
        from scipy.optimize import minimize

        base = self.cov
        if gradient:
            self._check_grad(base)
        if method is None:
            method = "L-BFGS-B" if gradient else "Nelder-Mead"
        if isinstance(x0, Covariance):
            th0 = x0.theta
        else:
            th0 = tuple(float(t) for t in x0) if x0 is not None else base.theta
        if len(th0) != 3 or not all(t > 0 and math.isfinite(t) for t in th0[:2]):
            raise ValueError(f"x0 must be (sigma2, phi, tau2) with positive sigma2 and phi, got {th0}")
        free_tau = fix_tau2 is None
        if not free_tau and not float(fix_tau2) > 0:
            raise ValueError("fix_tau2 must be positive (tau2 = 0 leaves nothing to solve)")
        z0 = [math.log(th0[0]), math.log(th0[1])] + ([math.log(max(th0[2], 1e-6))] if free_tau else [])
        Z = None if z is None else np.array(z, dtype=np.float64)
        best = {"ll": -math.inf, "cov": None}

        def obj(lz):
            g = None
            fail = (1e300, np.zeros(len(z0))) if gradient else 1e300
            try:
                cov = base.replace(sigma2=math.exp(lz[0]), phi=math.exp(lz[1]),
                                   tau2=math.exp(lz[2]) if free_tau else float(fix_tau2))
                self.update(cov)
                if gradient:
                    ll, _, g, _ = self.log_marginal_grad(n_probes=n_probes, seed=seed, z=Z, rtol=rtol, batch=batch)
                else:
                    ll, _ = self.log_marginal(n_probes=n_probes, seed=seed, z=Z, rtol=rtol, batch=batch)
            except (NNGPNumericalError, OverflowError):
                return fail
            if not math.isfinite(ll) or (gradient and not np.all(np.isfinite(g))):
                return fail
            if ll > best["ll"]:
                best.update(ll=ll, cov=cov)
            if gradient:
                return -ll, -(g * np.array(cov.theta))[:len(z0)]
            return -ll

        opts = {"maxiter": int(maxiter)}
        if method == "Nelder-Mead":
            opts.update(xatol=1e-4, fatol=1e-6)
        res = minimize(obj, np.array(z0), method=method, jac=True if gradient else None, options=opts)
        if best["cov"] is None:
            self.update(base)
            raise NNGPNumericalError("log_marginal could not be evaluated at any theta the optimiser tried")
        self.update(best["cov"])
        res.x, res.fun = np.log([getattr(best["cov"], k) for k in ("sigma2", "phi", "tau2")][:len(z0)]), -best["ll"]
        return best["cov"], res
