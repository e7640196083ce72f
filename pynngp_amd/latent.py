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

The latent mean at new locations is kriging of w_hat without a nugget:
``NNGP.predict(values=w_hat, cov=cov.replace(tau2=0), query=...)``.
"""
from __future__ import annotations

import dataclasses
import math
import warnings
from typing import Optional

import numpy as np
import torch

from . import _lib
from .nngp import Covariance, NNGPNumericalError, _default_device, _raise_on_bad

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


def _check_cov(cov) -> Covariance:
    if not isinstance(cov, Covariance):
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
    """

    def __init__(self, coords, y, cov, m: int = 15, X=None, eps=None, device=None, nbr=None):
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

        self.device = dev = _default_device(device)
        self.n, self.p = n, X_host.shape[1]
        to = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(dev)  # noqa: E731
        coords0 = to(c_host)
        nbr0 = _lib.knn_prior(coords0, self.m) if nbr is None else nbr.to(dev)
        # Z-order storage: slot s holds location perm[s]; neighbour sets relabelled into storage labels
        self.perm = _lib.row_order(coords0)[0].long()
        self.pos = torch.empty_like(self.perm)
        self.pos[self.perm] = torch.arange(n, device=dev)
        self.coords = coords0[self.perm].contiguous()
        nb = nbr0[self.perm].long()
        self.nbr = torch.where(nb >= 0, self.pos[nb.clamp(min=0)], -1).to(torch.int32).contiguous()
        self.off, self.rev_j, self.rev_k = _lib.reverse_neighbors(self.nbr)
        self.h = to(h_host)[self.perm].contiguous()
        self.y = to(np.where(observed, y_host, 0.0))[self.perm].contiguous()
        self.X = to(X_host)[self.perm].contiguous()
        self.B = torch.empty((n, self.m), dtype=torch.float64, device=dev)
        self.F = torch.empty(n, dtype=torch.float64, device=dev)
        self._prep = None
        self._ws_batch = None  # the operator's and solver's workspace, made on first use for the widest chunk so far
        self.update(cov)

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
    def _in(self, v, what="vector"):
        t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.array(v, dtype=np.float64))
        if t.dtype != torch.float64 or tuple(t.shape) != (self.n,):
            raise ValueError(f"{what} must be float64 ({self.n},), got {t.dtype} {tuple(t.shape)}")
        return t.to(self.device)[self.perm].contiguous()

    def _out(self, t, like):
        o = t[self.pos]
        return o if isinstance(like, torch.Tensor) else o.cpu().numpy()

    def _geom(self):
        return (self.nbr, self.B, self.off, self.rev_j, self.rev_k, self._prep, self.cov.sigma2)

    # -- the operator and the solver -------------------------------------------
    def matvec(self, x):
        """A x (two gathers, bit-reproducible)."""
        return self._out(_lib.precision_apply(*self._geom(), self._in(x, "x"), d=self.d, workspace=self._batch_ws(1)),
                         x)

    def _solve(self, rhs, rtol, max_iter, x0=None):
        """Storage-order solve: (x, SolveInfo); raises on a breakdown, warns on non-convergence."""
        if not 0.0 < rtol < 1.0:
            raise ValueError(f"rtol must be in (0, 1), got {rtol}")
        if max_iter is None:
            max_iter = min(max(2 * self.n, 1000), 20000)
        x = torch.zeros_like(rhs) if x0 is None else x0.clone()
        _, info = _lib.latent_cg(*self._geom(), rhs, x, d=self.d, rtol=rtol, max_iter=int(max_iter),
                                 check_every=CHECK_EVERY, workspace=self._batch_ws(1))
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
        need = _lib.load().nngp_latent_cg_batch_workspace_bytes(self.n, nrhs)
        if self._ws_batch is None or self._ws_batch.numel() < need:
            self._ws_batch = _lib._workspace(need, self.device)
        return self._ws_batch

    def _in_rows(self, v, what="rhs"):
        """(K, N) rows in the order of ``coords`` -> (K, N) device rows in storage order."""
        t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.array(v, dtype=np.float64))
        if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != self.n:
            raise ValueError(f"{what} must be float64 (K, {self.n}), got {t.dtype} {tuple(t.shape)}")
        return t.to(self.device)[:, self.perm]

    def _solve_cols(self, R, rtol, max_iter, X0=None):
        """One batched solve of the storage-order columns R (n, k <= LATENT_MAX_RHS): (X, info (k, 4))."""
        X = torch.zeros_like(R) if X0 is None else X0.clone()
        return _lib.latent_cg_batch(*self._geom(), R, X, d=self.d, rtol=rtol, max_iter=int(max_iter),
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
        if not 0.0 < rtol < 1.0:
            raise ValueError(f"rtol must be in (0, 1), got {rtol}")
        if max_iter is None:
            max_iter = min(max(2 * self.n, 1000), 20000)
        K = rows.shape[0]
        out = torch.empty((K, self.n), dtype=torch.float64, device=self.device)
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
        x = x[:, self.pos]
        return (x if isinstance(rhs, torch.Tensor) else x.cpu().numpy()), infos

    # -- posterior mean --------------------------------------------------------
    def _rhs(self, beta):
        yres = self.y if self.p == 0 else self.y - self.X @ torch.as_tensor(beta, dtype=torch.float64,
                                                                           device=self.device)
        return (self.d * yres).contiguous()

    def gls_beta(self, rtol: float = 1e-8, max_iter: Optional[int] = None, batch=None) -> np.ndarray:
        """GLS beta under V = C~ + tau2 H^-1 (C~ the NNGP covariance): V^-1 v = H v / tau2 - H A^-1 H v / tau4,
        one solve per column of X, ``batch`` columns per batched solve; rows with h = 0 drop out."""
        if self.p == 0:
            return np.zeros(0)
        rows = (self.d[:, None] * self.X).t()
        S, info = self._solve_rows(rows, rtol, max_iter, self._batch(batch))
        self._report(info, rtol)
        S = S.t().contiguous()
        W = self.d[:, None] * (self.X - S)  # V^-1 X
        G = (self.X.t() @ W).cpu().numpy()
        g = (W.t() @ self.y).cpu().numpy()
        return np.linalg.solve(0.5 * (G + G.T), g)

    def mean(self, beta=None, rtol: float = 1e-8, max_iter: Optional[int] = None):
        """Posterior mean ``(w_hat, beta_hat)``: w_hat = A^-1 h (y - X beta) / tau2 as a numpy array.  With ``X``
        and no ``beta``, beta_hat is the GLS estimate (:meth:`gls_beta`; p + 1 solves in all); without ``X`` it
        is empty.  The latent mean at new locations: ``NNGP.predict(values=w_hat, cov=cov.replace(tau2=0))``."""
        if beta is None:
            beta = self._beta_hat = self.gls_beta(rtol, max_iter)
        beta = np.asarray(beta, dtype=np.float64).reshape(-1)
        if beta.shape != (self.p,):
            raise ValueError(f"beta must hold {self.p} coefficients")
        w, _ = self._solve(self._rhs(beta), rtol, max_iter)
        return w[self.pos].cpu().numpy(), beta

    # -- exact draws -----------------------------------------------------------
    def _beta_for_draws(self, beta, rtol, max_iter):
        if beta is None:
            beta = self._beta_hat if self._beta_hat is not None else self.gls_beta(rtol, max_iter)
            self._beta_hat = beta
        return np.asarray(beta, dtype=np.float64).reshape(-1)

    def _draw_chunks(self, n_draws, seed, z, b, rtol, max_iter, batch):
        """Yields ``(k0, W)``: the draws k0 .. k0 + W.shape[1] - 1 as storage-order columns (n, k <= batch) on the
        device.  Draw k takes the Philox streams of sweep indices 2k and 2k + 1, whatever the chunking."""
        if z is not None:
            z1, z2 = (np.asarray(a, dtype=np.float64).reshape(n_draws, self.n) for a in z)
        zz = torch.empty(self.n, dtype=torch.float64, device=self.device)
        for k0 in range(0, n_draws, batch):
            kc = min(batch, n_draws - k0)
            Z1 = torch.empty((self.n, kc), dtype=torch.float64, device=self.device)
            Z2 = torch.empty_like(Z1)
            for c in range(kc):
                if z is None:
                    Z1[:, c] = _lib.gibbs_normals(zz, seed, 2 * (k0 + c))
                    Z2[:, c] = _lib.gibbs_normals(zz, seed, 2 * (k0 + c) + 1)
                else:
                    Z1[:, c], Z2[:, c] = self._in(z1[k0 + c], "z1"), self._in(z2[k0 + c], "z2")
            eta = _lib.precision_sqrt_t_apply_batch(*self._geom(), Z1, Z2, d=self.d, workspace=self._batch_ws(kc))
            W, info = self._solve_rows((b[:, None] + eta).t(), rtol, max_iter, kc)
            self._report(info, rtol, first=k0)
            yield k0, W.t().contiguous()

    def sample(self, n_draws: int, seed: int = 0, z=None, beta=None, rtol: float = 1e-8,
               max_iter: Optional[int] = None, batch=None) -> np.ndarray:
        """``(n_draws, N)`` exact posterior draws w = A^-1 (b + eta), eta = (I - B)^T (sigma2 F)^-1/2 z1 +
        (h / tau2)^1/2 z2, ``batch`` draws per batched square-root application and solve (default
        ``LATENT_MAX_RHS``; the draws do not depend on it).  The normals are Philox streams keyed by ``seed``
        (``nngp_gibbs_normals``; one seed repeats bit for bit), or ``z = (z1, z2)``, each (n_draws, N), for
        testing.  ``beta``: as :meth:`mean`."""
        n_draws = int(n_draws)
        if n_draws < 0:
            raise ValueError("n_draws must be >= 0")
        batch = self._batch(batch)
        b = self._rhs(self._beta_for_draws(beta, rtol, max_iter))
        out = np.empty((n_draws, self.n))
        for k0, W in self._draw_chunks(n_draws, seed, z, b, rtol, max_iter, batch):
            out[k0:k0 + W.shape[1]] = W[self.pos].t().cpu().numpy()
        return out

    # -- posterior uncertainty ---------------------------------------------------
    def marginal_variance(self, n_draws: int = 64, seed: int = 0, z=None, beta=None, rtol: float = 1e-8,
                          max_iter: Optional[int] = None, batch=None) -> np.ndarray:
        """``(N,)`` posterior variances of w by the Rao-Blackwellised estimator over ``n_draws`` >= 2 exact draws.
        Given the rest of a draw w, w_i is Gaussian with mean c_i = w_i - (A w - b)_i / A_ii and variance 1 / A_ii,
        so Var(w_i | y) = 1 / A_ii + Var(c_i), estimated by

            v_i = 1 / A_ii + sum_k (c_i^(k) - c_bar_i)^2 / (K - 1).

        Only the second part carries Monte-Carlo error (relative standard deviation sqrt(2 / (K - 1)) of that
        part).  A w is one batched operator application per chunk of ``batch`` draws, A_ii comes from
        ``nngp_precision_diag``; the sums run on the device, draw by draw in draw order (shifted by the first
        draw's c, so nothing cancels), hence the result does not depend on ``batch``.  Arguments as :meth:`sample`."""
        n_draws = int(n_draws)
        if n_draws < 2:
            raise ValueError("marginal_variance needs n_draws >= 2")
        batch = self._batch(batch)
        b = self._rhs(self._beta_for_draws(beta, rtol, max_iter))
        aii = _lib.precision_diag(self._prep, self.n, self.m, self.cov.sigma2, d=self.d)
        shift = None
        s1 = torch.zeros(self.n, dtype=torch.float64, device=self.device)
        s2 = torch.zeros_like(s1)
        for _, W in self._draw_chunks(n_draws, seed, z, b, rtol, max_iter, batch):
            AW = _lib.precision_apply_batch(*self._geom(), W, d=self.d, workspace=self._batch_ws(W.shape[1]))
            C = W - (AW - b[:, None]) / aii[:, None]
            if shift is None:
                shift = C[:, 0].clone()
            for c in range(C.shape[1]):
                dev = C[:, c] - shift
                s1 += dev
                s2 += dev * dev
        v = 1.0 / aii + (s2 - s1 * s1 / n_draws) / (n_draws - 1)
        return v[self.pos].cpu().numpy()
