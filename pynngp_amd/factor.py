"""``NNGPFactor``: solves with the NNGP factor on the GPU -- prior draws and covariance products.

The NNGP prior on n nodes is w = (I - B)^-1 (sigma2 F)^1/2 z with B (n, m) and F the unit-variance factors of the
fused sweep: its precision Q = (I - B)^T (sigma2 F)^-1 (I - B) is what ``nngp_precision_apply`` multiplies by, and
its covariance C = sigma2 (I - B)^-1 F (I - B)^-T needs the two triangular solves (I - B) x = b and
(I - B)^T x = b.  The recurrence x_i = b_i + sum_k B[i,k] x[nbr[i,k]] is sequential in index order, but its
dependency DAG is shallow for spatial input, so the solves run level by level (``nngp_factor_levels`` on the host,
once per neighbour set; ``nngp_factor_solve_batch`` on the GPU).  A row's sum runs in slot order whatever the
schedule, so results are bit-identical for every ``fuse_width`` and batch size.

Unlike ``LatentPosterior`` the nodes keep the caller's order (no Z-order storage): the level schedule is that of
the order in which the neighbour sets were built, every neighbour preceding its row.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from .nngp import AnisotropicCovariance, Covariance, _default_device, _raise_on_bad

# Rows per level up to which consecutive levels share one single-workgroup launch (chosen from the
# fuse_width sweep of tools/bench_factor.py at N = 1e6, m = 15)
DEFAULT_FUSE_WIDTH = 64


def _check_cov(cov) -> Covariance:
    if not isinstance(cov, Covariance):
        from .nngp import _refuse_sep

        _refuse_sep(cov, "NNGPFactor")
        if isinstance(cov, AnisotropicCovariance):
            raise TypeError("NNGPFactor does not serve an AnisotropicCovariance (per-axis ranges); it takes a "
                            "pynngp_amd.Covariance")
        if callable(cov):
            raise NotImplementedError("NNGPFactor takes a fused covariance kind (pynngp_amd.Covariance); a callable "
                                      "covariance is not served")
        raise TypeError(f"cov must be a pynngp_amd.Covariance, got {type(cov).__name__}")
    return cov


def _host(a, what):
    h = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    if h.ndim == 1:
        h = h[:, None]
    if h.ndim != 2 or not 1 <= h.shape[1] <= _lib.MAX_DIM or h.shape[0] < 1:
        raise ValueError(f"{what} must be (N >= 1, d) with 1 <= d <= {_lib.MAX_DIM}, got {h.shape}")
    if not np.all(np.isfinite(h)):
        raise ValueError(f"{what} must be finite")
    return h


class NNGPFactor:
    """The factor (B, F) of the NNGP prior at ``cov`` with the level schedules of its two triangular solves.

    ``coords`` (N, d), 1 <= d <= 3; ``cov`` a :class:`Covariance` of any fused kind (``matern`` with its ``nu``
    included; tau2 is not used by the prior); ``nbr``: prior neighbour sets to reuse (int32 (N, m), every valid
    index below its row's, -1 padded), default: built here; ``ref`` (n_S, d): a reference set -- the nodes are then
    the points of ``ref`` followed by the data locations outside it as leaves linked to their m nearest points of
    S, exactly ``LatentPosterior``'s nodes, ``node_of_t`` mapping the rows of ``coords`` to nodes (without ``ref``
    the nodes are the rows of ``coords``).  Vectors are (n_nodes,) or (n_nodes, k) columns in node order; numpy in
    gives numpy out, device tensors in give device tensors out.

    ``depth`` / ``depth_t``: the levels of the forward / transposed schedule.  ``fuse_width``: consecutive levels
    of at most that many rows share one single-workgroup launch (0: one launch per level); results do not depend
    on it.  ``n_launches``: the launches one solve makes at the current ``fuse_width``.
    """

    def __init__(self, coords, cov, m: int = 15, nbr=None, device=None, ref=None,
                 fuse_width: int = DEFAULT_FUSE_WIDTH):
        cov = _check_cov(cov)
        self.m = int(m)
        if not 1 <= self.m <= _lib.MAX_M:
            raise ValueError(f"m={m} outside [1, {_lib.MAX_M}]")
        c_host = _host(coords, "coords")
        n = c_host.shape[0]
        self.device = dev = _default_device(device)
        to = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
        if ref is not None:
            if nbr is not None:
                raise ValueError("nbr is for S = T; with ref the neighbour sets are built on the reference set")
            s_host = _host(ref, "ref")
            if s_host.shape[1] != c_host.shape[1]:
                raise ValueError(f"reference set has dimension {s_host.shape[1]}, locations {c_host.shape[1]}")
            from .latent import LatentPosterior

            # LatentPosterior's node DAG (it reads .device and .m only): [S; the data locations outside S]
            self.coords, self.nbr, self.n_s, node_of_t = LatentPosterior._ref_nodes(self, to(c_host), to(s_host))
        else:
            self.coords, self.n_s, node_of_t = to(c_host), n, np.arange(n)
            if nbr is None:
                self.nbr = _lib.knn_prior(self.coords, self.m)
            else:
                if not isinstance(nbr, torch.Tensor) or nbr.dtype != torch.int32 or tuple(nbr.shape) != (n, self.m):
                    raise ValueError(f"nbr must be an int32 ({n}, {self.m}) device tensor")
                self.nbr = nbr.to(dev).contiguous()
        self.n = n
        self.n_nodes = self.coords.shape[0]
        self.node_of_t = np.asarray(node_of_t, dtype=np.int64)
        self._node_of_t_dev = torch.from_numpy(self.node_of_t).to(dev)
        self.off, self.rev_j, self.rev_k = _lib.reverse_neighbors(self.nbr)
        nbr_host = self.nbr.cpu().numpy()
        self.sched = _lib.factor_levels(nbr_host, False, device=dev)
        self.sched_t = _lib.factor_levels(nbr_host, True, device=dev)
        self.depth, self.depth_t = self.sched.depth, self.sched_t.depth
        self.fuse_width = fuse_width
        self.B = torch.empty((self.n_nodes, self.m), dtype=torch.float64, device=dev)
        self.F = torch.empty(self.n_nodes, dtype=torch.float64, device=dev)
        self._prep = None
        self.update(cov)

    # -- theta and the schedule ------------------------------------------------
    def update(self, cov) -> "NNGPFactor":
        """A new theta on the same neighbour sets: one B / F sweep and one ``prepare``; the schedules stay."""
        cov = _check_cov(cov)
        _, _, p = _lib.bf_sweep(self.coords, self.nbr, 0, cov.kind, 1.0, cov.phi, 0.0, B=self.B, F=self.F,
                                nu=cov.nu_arg)
        _raise_on_bad(p.cpu().numpy())
        self._prep = _lib.gibbs_prepare(self.B, self.F, self.off, self.rev_j, self.rev_k, prep=self._prep)
        self.cov = cov
        return self

    @property
    def fuse_width(self) -> int:
        return self._fuse_width

    @fuse_width.setter
    def fuse_width(self, w):
        w = int(w)
        if not 0 <= w <= _lib.FACTOR_MAX_FUSE_WIDTH:
            raise ValueError(f"fuse_width={w} outside [0, {_lib.FACTOR_MAX_FUSE_WIDTH}]")
        self._fuse_width = w

    @property
    def n_launches(self) -> dict:
        """Launches of one solve at the current ``fuse_width``: ``wide`` / ``runs`` (wide levels and narrow runs of
        the forward solve), ``wide_t`` / ``runs_t`` (the transposed one), and their sums ``forward`` /
        ``transposed``."""
        w, r = self.sched.launch_counts(self._fuse_width)
        wt, rt = self.sched_t.launch_counts(self._fuse_width)
        return {"wide": w, "runs": r, "wide_t": wt, "runs_t": rt, "forward": w + r, "transposed": wt + rt}

    # -- vectors in / out ------------------------------------------------------
    def _in(self, v, what="vector"):
        t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.array(v, dtype=np.float64))
        if t.dtype != torch.float64 or t.dim() not in (1, 2) or t.shape[0] != self.n_nodes:
            raise ValueError(f"{what} must be float64 ({self.n_nodes},) or ({self.n_nodes}, k), got {t.dtype} "
                             f"{tuple(t.shape)}")
        return (t[:, None] if t.dim() == 1 else t).to(self.device)

    @staticmethod
    def _out(t, like, squeeze):
        o = t[:, 0] if squeeze else t
        return o if isinstance(like, torch.Tensor) else o.cpu().numpy()

    def _chunks(self, V, fn):
        """``fn`` on column chunks of at most LATENT_MAX_RHS columns; the results side by side."""
        k = V.shape[1]
        if k == 0:
            return torch.empty_like(V)
        parts = [fn(V[:, c0:c0 + _lib.LATENT_MAX_RHS].contiguous()) for c0 in range(0, k, _lib.LATENT_MAX_RHS)]
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)

    def _geom(self):
        return (self.nbr, self.B, self.off, self.rev_j, self.rev_k, self._prep)

    # -- the operations --------------------------------------------------------
    def solve(self, b, trans: bool = False):
        """x with (I - B) x = b, or (I - B)^T x = b for ``trans``: (n_nodes,) or (n_nodes, k) columns."""
        V = self._in(b, "b")
        X = self._chunks(V, lambda c: _lib.factor_solve_batch(*self._geom(), self.sched_t if trans else self.sched,
                                                              c, trans=trans, fuse_width=self._fuse_width))
        return self._out(X, b, np.ndim(b) == 1)

    def cov_apply(self, v):
        """C v = sigma2 (I - B)^-1 F (I - B)^-T v: the covariance the model uses, the inverse of
        :meth:`precision_apply`'s matrix."""
        V = self._in(v, "v")
        X = self._chunks(V, lambda c: _lib.factor_cov_apply_batch(
            self.nbr, self.B, self.F, self.off, self.rev_j, self.rev_k, self._prep, self.sched, self.sched_t,
            self.cov.sigma2, c, fuse_width=self._fuse_width))
        return self._out(X, v, np.ndim(v) == 1)

    def precision_apply(self, v):
        """Q v = (I - B)^T (sigma2 F)^-1 (I - B) v over all nodes (``nngp_precision_apply_batch`` with d = None)."""
        V = self._in(v, "v")
        X = self._chunks(V, lambda c: _lib.precision_apply_batch(*self._geom(), self.cov.sigma2, c))
        return self._out(X, v, np.ndim(v) == 1)

    def _draws(self, n_draws, seed, z):
        """(n_nodes, n_draws) device columns of prior draws."""
        n_draws = int(n_draws)
        if n_draws < 0:
            raise ValueError(f"n_draws={n_draws} is negative")
        Z = None
        if z is not None:
            zt = z if isinstance(z, torch.Tensor) else torch.from_numpy(np.array(z, dtype=np.float64))
            if zt.dtype != torch.float64 or tuple(zt.shape) != (n_draws, self.n_nodes):
                raise ValueError(f"z must be float64 ({n_draws}, {self.n_nodes}), got {zt.dtype} {tuple(zt.shape)}")
            Z = zt.to(self.device).t()
        out = torch.empty((self.n_nodes, n_draws), dtype=torch.float64, device=self.device)
        for k0 in range(0, n_draws, _lib.LATENT_MAX_RHS):
            kc = min(_lib.LATENT_MAX_RHS, n_draws - k0)
            out[:, k0:k0 + kc] = _lib.factor_prior_draw_batch(
                self.nbr, self.B, self.F, self.sched, self.cov.sigma2, kc, fuse_width=self._fuse_width,
                z=None if Z is None else Z[:, k0:k0 + kc].contiguous(), seed=seed, draw0=k0)
        return out

    def sample_prior(self, n_draws: int, seed: int = 0, z=None):
        """``(n_draws, n_nodes)`` draws w = (I - B)^-1 (sigma2 F)^1/2 z from the NNGP prior.  ``z`` (n_draws,
        n_nodes): the standard normals to use; default: Philox normals keyed by (``seed``, draw index, node) -- the
        generator behind ``nngp_gibbs_normals`` -- so draw k is the same field however many are drawn with it."""
        W = self._draws(n_draws, seed, z).t().contiguous()
        return W if isinstance(z, torch.Tensor) else W.cpu().numpy()

    def sample_prior_at_data(self, n_draws: int, seed: int = 0, z=None):
        """:meth:`sample_prior` reported per row of ``coords``: ``(n_draws, N)`` (with ``ref`` a data location is a
        leaf, or the reference point it coincides with)."""
        W = self._draws(n_draws, seed, z)[self._node_of_t_dev].t().contiguous()
        return W if isinstance(z, torch.Tensor) else W.cpu().numpy()
