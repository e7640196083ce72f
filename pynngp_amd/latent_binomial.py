"""``BinomialLatentPosterior``: the latent field given binomial / logistic data at fixed (sigma2, phi), by Laplace
approximation on the GPU -- the deterministic counterpart of ``BinomialSeqNNGP`` (Polya-Gamma Gibbs), in the style
of INLA.

    s_i ~ Binomial(b_i, logistic(x_i beta + w_i)),   w ~ NNGP(0, sigma2 R(phi)),   beta flat, no tau2,

on the node DAG of :class:`LatentPosterior` (S = T, or a reference set with the data locations outside it as
leaves).  With Q = (I - B)^T (sigma2 F)^-1 (I - B) over all nodes and l_i the binomial log-likelihood terms, the
log posterior is Phi(beta, w) = sum_i l_i(x_i beta + w_i) - w^T Q w / 2, concave in (beta, w).  A Newton step at
(beta, w) has W_i = b_i p_i (1 - p_i) and g_i = s_i - b_i p_i and maximises the quadratic model, which is the
Gaussian latent problem with noise precision d = W and weighted response W w + g - W X dbeta:

    (Q + W) w' = W w + g - W X dbeta,    (X^T W (X - U)) dbeta = X^T (W w + g - W u0),
    u0 = (Q + W)^-1 (W w + g),   U = (Q + W)^-1 W X,   w' = u0 - U dbeta                       (the GLS step).

These are p + 1 right-hand sides of the system :class:`LatentPosterior` already solves, so this class only swaps its
``d`` and right-hand sides: the link quantities come from one launch of ``nngp_binomial_newton_step``, the operator,
the batched Jacobi-PCG, the leaf elimination, the perturbation sampler and the Lanczos log-determinant are the
parent's.  At the mode (beta_hat, w_hat) the Laplace approximation is w | s ~ N(w_hat, (Q + W_hat)^-1) at beta_hat,
the parent's posterior for the working response y = X beta_hat + w_hat + g / W_hat with noise precision W_hat; the
Laplace evidence is

    log p(s | theta) ~ l(w_hat, beta_hat) - w_hat^T Q w_hat / 2 - sum_i log(sigma2 F_i) / 2 - log det(Q + W_hat) / 2,

log det(Q + W) = log det A_S + sum over leaves of log(f_j + W_j); probabilities are E[logistic(mu + s Z)] of the
latent mean and standard deviation (``nngp_logistic_normal``).
"""
from __future__ import annotations

import dataclasses
import math
import warnings
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .latent import LatentPosterior
from .nngp import Covariance, NNGPNumericalError, _raise_on_bad

W_FLOOR = 1e-200  # a working weight below this is an unobserved node of the Gaussian approximation (g / W overflows)


@dataclasses.dataclass(frozen=True)
class ModeInfo:
    """Outcome of :meth:`BinomialLatentPosterior.mode`: Newton steps taken, the CG iterations of each step's
    solve for w (``cg_iterations[k]``; the GLS columns run in the same batched solve), the final
    max-norm of the log posterior's gradient over (beta, all nodes), ``converged`` (that norm <= gtol max(1, max
    trials)) and the log posterior at the returned point."""

    newton_steps: int
    cg_iterations: Tuple[int, ...]
    grad_norm: float
    converged: bool
    log_posterior: float


def _check_counts(successes, trials, n):
    """``(s, b, observed)`` as ``BinomialSeqNNGP`` validates them, without its cap on trials (int32 range)."""
    s = np.asarray(successes.detach().cpu().numpy() if isinstance(successes, torch.Tensor) else successes,
                   dtype=np.float64).reshape(-1)
    b_in = np.asarray(trials.detach().cpu().numpy() if isinstance(trials, torch.Tensor) else trials)
    if b_in.dtype.kind == "f":
        if not np.all(np.isfinite(b_in)) or np.any(b_in != np.round(b_in)):
            raise ValueError("trials must be integers")
    elif b_in.dtype.kind not in "iu":
        raise ValueError("trials must be integers")
    b = b_in.reshape(-1).astype(np.int64)
    if s.shape != (n,):
        raise ValueError(f"successes must hold one count per location ({n},), got {s.shape}")
    if b.shape != (n,):
        raise ValueError(f"trials must hold one count per location ({n}), got {b.shape}")
    if np.any(b < 0) or np.any(b > np.iinfo(np.int32).max):
        raise ValueError(f"trials must lie in [0, {np.iinfo(np.int32).max}]")
    if np.any(np.isinf(s)):
        raise ValueError("successes must be finite or NaN (NaN = unobserved)")
    observed = np.isfinite(s) & (b > 0)
    so = s[observed]
    if np.any(so != np.round(so)):
        raise ValueError("successes must be integers")
    if np.any(so < 0) or np.any(so > b[observed]):
        raise ValueError("successes must lie in [0, trials]")
    return s, b, observed


class BinomialLatentPosterior(LatentPosterior):
    """Laplace approximation of the latent field given binomial data (see the module docstring).

    ``coords`` (N, d); ``successes`` (N,) integers in [0, trials], NaN = unobserved; ``trials`` (N,) non-negative
    integers (0 = unobserved; Bernoulli data: 1; no cap beyond int32); ``cov`` a :class:`Covariance` carrying
    (sigma2, phi[, nu]) -- its tau2 is ignored, the model has none; ``X`` (N, p) covariates or None (no mean);
    ``ref`` / ``X_ref`` as :class:`LatentPosterior` (``X_ref`` is used by ``probability(where="ref")``).  Storage
    order, neighbour sets, operator and solver are the parent's; ``matvec`` / ``solve`` / ``solve_many`` act on Q_S
    + W at the current working weights.  Methods that need the mode compute it on first use (:meth:`mode`)."""

    def __init__(self, coords, successes, trials, cov, m: int = 15, X=None, device=None, ref=None, X_ref=None):
        n = int(np.asarray(coords.detach().cpu().numpy() if isinstance(coords, torch.Tensor) else coords).shape[0])
        s, b, observed = _check_counts(successes, trials, n)
        if not isinstance(cov, Covariance):
            raise TypeError(f"cov must be a pynngp_amd.Covariance, got {type(cov).__name__}")
        if not observed.any():
            raise ValueError("no observed responses (trials = 0 or successes NaN everywhere)")
        self._w = self._beta = self._U_S = self._mode = None
        y0 = np.where(observed, 0.0, np.nan)  # the parent's response only marks the observed rows here
        super().__init__(coords, y0, cov.replace(tau2=1.0), m=m, X=X, device=device, ref=ref, X_ref=X_ref)
        dev, nn = self.device, self.n_nodes
        b_n, s_n = np.zeros(nn, dtype=np.int32), np.zeros(nn)
        b_n[self.node_of_t[observed]] = b[observed]
        s_n[self.node_of_t[observed]] = s[observed]
        self.max_trials = int(b_n.max())
        self.trials = torch.from_numpy(b_n).to(dev)[self.perm].contiguous()
        self.successes = torch.from_numpy(s_n).to(dev)[self.perm].contiguous()
        self._has_x_ref = X_ref is not None
        if self._has_x_ref and self.p > 0:  # covariates of the reference nodes that carry no data row
            xr = np.asarray(X_ref, dtype=np.float64)
            X_n = np.zeros((nn, self.p))
            X_n[:self.n_s] = xr[:, None] if xr.ndim == 1 else xr
            X_n[self.node_of_t] = self.X[self.slot_of_t].cpu().numpy()
            self.X = torch.from_numpy(X_n).to(dev)[self.perm].contiguous()
        self._link_ws = _lib._workspace(_lib.load().nngp_binomial_newton_step_workspace_bytes(nn), dev)
        self._apply_ws = None

    # -- theta -----------------------------------------------------------------
    def update(self, cov) -> "BinomialLatentPosterior":
        """A new (sigma2, phi[, nu]) on the same neighbour sets (tau2 ignored).  The mode is forgotten as a result and
        kept as the next :meth:`mode`'s starting point."""
        if not isinstance(cov, Covariance):
            raise TypeError(f"cov must be a pynngp_amd.Covariance, got {type(cov).__name__}")
        super().update(cov.replace(tau2=1.0))
        self._mode = None
        return self

    # -- the link step and the log posterior -------------------------------------
    def _xb(self, beta):
        if self.p == 0:
            return torch.zeros(self.n_nodes, dtype=torch.float64, device=self.device)
        return (self.X @ torch.as_tensor(beta, dtype=torch.float64, device=self.device)).contiguous()

    def _link(self, beta, w):
        """The link kernel at (beta, w) and the log posterior there: a dict of d, rhs, g (storage order), the sum of
        the log-likelihood terms, max |g|, the prior's quadratic form and ``lp``.  Raises on a non-finite eta."""
        d, rhs, g, part = _lib.binomial_newton_step(self.trials, self.successes, self._xb(beta), w,
                                                    workspace=self._link_ws)
        f = 1.0 / (self.cov.sigma2 * self.F)
        Bw, _ = _lib.latent_rows_dot2_batch(self.nbr, self.B, self.B, self.n_s, w[:self.n_s, None].contiguous())
        r = w - Bw[:, 0]
        quad = float((f * r * r).sum())
        ph = part.cpu().numpy()
        bad, neg = _lib.binomial_check_partials(ph)
        if neg >= 0:
            raise ValueError(f"negative trials at node {int(self.perm[neg])}")
        if bad >= 0:
            raise NNGPNumericalError(f"x beta + w is not finite at node {int(self.perm[bad])} (nodes: the reference "
                                     "points, then the data locations outside them); NaN or inf in X, beta0 or w0?")
        return {"d": d, "rhs": rhs, "g": g, "ll": float(ph[0]), "gmax": float(ph[1]), "quad": quad,
                "lp": float(ph[0]) - 0.5 * quad}

    def _grad(self, st, w):
        """(grad in w over all nodes, grad in beta) of the log posterior at the point of ``st``: g - Q w and X^T g."""
        nn = self.n_nodes
        need = _lib.load().nngp_precision_batch_workspace_bytes(nn, 1)
        if self._apply_ws is None or self._apply_ws.numel() < need:
            self._apply_ws = _lib._workspace(need, self.device)
        Qw = _lib.precision_apply_batch(*self._geom(), w[:, None].contiguous(), d=None, workspace=self._apply_ws)[:, 0]
        gw = st["g"] - Qw
        gb = (self.X.t() @ st["g"]) if self.p else torch.zeros(0, dtype=torch.float64, device=self.device)
        return gw, gb

    # -- the mode ------------------------------------------------------------------
    def mode(self, gtol: float = 1e-8, max_newton: int = 50, rtol: float = 1e-8, beta0=None, w0=None,
             max_iter: Optional[int] = None, where: str = "data", warm_start: bool = True):
        """The joint posterior mode ``(beta_hat, w_hat, info)`` by Newton / IRLS steps (module docstring), each one
        link-kernel launch, one batched CG solve of p + 1 columns on S warm-started from the previous iterate, the
        leaves recovered in closed form, and step halving on the log posterior (evaluated over all nodes), so that
        no step descends.  Stops when the max-norm of the gradient over (beta, all nodes) is <= ``gtol`` max(1, max
        trials); otherwise warns after ``max_newton`` steps (``info.converged`` False).  ``rtol``: the CG's relative
        tolerance; a step tightens it to 0.1 of the gradient target over |right-hand side| when that is smaller, since
        the solver's residual is the gradient the step leaves behind.  ``beta0`` (p,), ``w0`` (n_nodes,) in node
        order (reference points, then data locations outside them): the start, default the last mode (any theta),
        else zero.  ``w_hat`` is returned at the rows of ``coords`` (``where="data"``) or of the reference set
        (``"ref"``); ``w_hat_nodes`` holds it in node order.  ``warm_start=False`` starts every CG solve from zero (for
        measurement; the result agrees to the tolerances).  A non-finite x beta + w raises
        :class:`NNGPNumericalError` naming the node."""
        self._check_where(where)
        if not gtol > 0 or int(max_newton) < 0:
            raise ValueError("gtol must be positive and max_newton >= 0")
        max_iter = self._cg_args(rtol, max_iter)
        dev, n_s, p = self.device, self.n_s, self.p
        tol = gtol * max(1.0, float(self.max_trials))
        if beta0 is not None:
            beta = np.array(beta0, dtype=np.float64).reshape(-1)
            if beta.shape != (p,):
                raise ValueError(f"beta0 must hold {p} coefficients")
        else:
            beta = np.zeros(p) if self._beta is None else self._beta.copy()
        if w0 is not None:
            w = self._nodes_in(w0, 1, "n")[0].contiguous()
        else:
            w = torch.zeros(self.n_nodes, dtype=torch.float64, device=dev) if self._w is None else self._w.clone()
        US = self._U_S if self._U_S is not None else torch.zeros((n_s, p), dtype=torch.float64, device=dev)
        st = self._link(beta, w)
        cg_its, steps, converged, gn = [], 0, False, math.inf
        while True:
            gw, gb = self._grad(st, w)
            gn = max(float(gw.abs().max()), float(gb.abs().max()) if p else 0.0)
            if gn <= tol:
                converged = True
                break
            if steps >= int(max_newton):
                break
            # the working system at this point: noise precision W, weighted responses [W w + g, W X]
            self.d = d = st["d"]
            pos = d > 0
            C = torch.cat([st["rhs"][:, None], d[:, None] * self.X], dim=1)
            V = torch.where(pos[:, None], C / torch.where(pos, d, torch.ones_like(d))[:, None], torch.zeros_like(C))
            new = torch.empty_like(C)
            its, rt = 0, None
            for k0 in range(0, p + 1, _lib.LATENT_MAX_RHS):
                Ck, Vk = C[:, k0:k0 + _lib.LATENT_MAX_RHS], V[:, k0:k0 + _lib.LATENT_MAX_RHS].contiguous()
                RS = Ck[:n_s].contiguous()
                if self._has_leaves():
                    Vz = Vk.clone()
                    Vz[:n_s] = 0.0
                    RS = RS + self._fold_cols(Vz)
                X0 = None
                if warm_start:
                    X0 = torch.cat([w[:n_s, None], US], dim=1)[:, k0:k0 + _lib.LATENT_MAX_RHS].contiguous()
                if rt is None:  # column 0 is the solve for w: its residual is the gradient the step leaves
                    bn = float(torch.linalg.vector_norm(RS[:, 0]))
                    rt = min(rtol, max(0.1 * tol / bn, 1e-14)) if bn > 0 else rtol
                XS, info = self._solve_cols(RS, rt, max_iter, X0)
                self._report(info, rt, first=k0)
                if k0 == 0:
                    its = int(info[0][0])
                new[:, k0:k0 + _lib.LATENT_MAX_RHS] = self._node_cols(XS, Vk[n_s:].contiguous())
            u0, U = new[:, 0], new[:, 1:]
            if p:
                G = (self.X.t() @ (d[:, None] * (self.X - U))).cpu().numpy()
                r = (self.X.t() @ (st["rhs"] - d * u0)).cpu().numpy()
                dbeta = np.linalg.solve(0.5 * (G + G.T), r)
                w_new = u0 - U @ torch.from_numpy(dbeta).to(dev)
                US = U[:n_s].contiguous()
            else:
                dbeta, w_new = np.zeros(0), u0
            dw = w_new - w
            t, accepted = 1.0, None
            slack = 1e-12 * max(1.0, abs(st["lp"]))
            for _ in range(40):
                bt, wt = beta + t * dbeta, (w + t * dw).contiguous()
                cand = self._link(bt, wt)
                if cand["lp"] >= st["lp"] - slack:
                    accepted = (bt, wt, cand)
                    break
                t *= 0.5
            cg_its.append(its)
            if accepted is None:  # no ascent along the step: rounding has taken over
                break
            beta, w, st = accepted
            steps += 1
        if not converged:
            warnings.warn(f"the Newton iteration for the binomial mode stopped after {steps} steps at gradient norm "
                          f"{gn:.3g} > {tol:.3g}", RuntimeWarning, stacklevel=2)
        self._beta, self._w, self._U_S = beta.copy(), w, US
        self._set_gaussian(beta, w, st)
        info = ModeInfo(steps, tuple(cg_its), gn, converged, st["lp"])
        self._mode = {"st": st, "info": info, "args": (gtol, max_newton, rtol)}
        return beta.copy(), w[self._rows_of(where)].cpu().numpy(), info

    def _set_gaussian(self, beta, w, st):
        """Make the parent's Gaussian machinery that of the Laplace approximation at (beta, w): d = W_hat, y the
        working response (so that d (y - X beta) = W w + g, whose solve returns w), beta_hat = beta."""
        d = torch.where(st["d"] < W_FLOOR, torch.zeros_like(st["d"]), st["d"]).contiguous()
        pos = d > 0
        self.d = d
        self.y = torch.where(pos, self._xb(beta) + w + st["g"] / torch.where(pos, d, torch.ones_like(d)),
                             torch.zeros_like(d)).contiguous()
        self._beta_hat = beta.copy()

    def _ensure_mode(self):
        if self._mode is None:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                _, _, info = self.mode()
            if not info.converged:
                warnings.warn(f"the binomial mode did not converge (gradient norm {info.grad_norm:.3g}); call mode() "
                              "with more steps", RuntimeWarning, stacklevel=3)
        return self._mode

    @property
    def beta_hat(self) -> np.ndarray:
        self._ensure_mode()
        return self._beta.copy()

    @property
    def w_hat_nodes(self) -> np.ndarray:
        """The mode of w over all nodes, in node order (the reference points, then the data locations outside them)."""
        self._ensure_mode()
        return self._w[self.pos].cpu().numpy()

    # -- the Gaussian approximation: draws, variances ------------------------------------
    def mean(self, *a, **k):
        raise NotImplementedError("BinomialLatentPosterior has no Gaussian response: use mode()")

    def gls_beta(self, *a, **k):
        raise NotImplementedError("BinomialLatentPosterior estimates beta jointly with w: use mode()")

    def sample(self, n_draws: int, seed: int = 0, z=None, rtol: float = 1e-8, max_iter: Optional[int] = None,
               batch=None, where: str = "data") -> np.ndarray:
        """``(n_draws, N)`` draws of w from the Laplace approximation N(w_hat, (Q + W_hat)^-1) at beta_hat: the
        parent's perturbation sampler (:meth:`LatentPosterior.sample`) at d = W_hat, same streams and arguments."""
        self._ensure_mode()
        return super().sample(n_draws, seed=seed, z=z, beta=self._beta, rtol=rtol, max_iter=max_iter, batch=batch,
                              where=where)

    def marginal_variance(self, n_draws: int = 64, seed: int = 0, z=None, rtol: float = 1e-8,
                          max_iter: Optional[int] = None, batch=None, where: str = "data") -> np.ndarray:
        """``(N,)`` variances of w under the Laplace approximation: :meth:`LatentPosterior.marginal_variance` (the
        Rao-Blackwellised estimator over ``n_draws`` draws) at d = W_hat."""
        self._ensure_mode()
        return super().marginal_variance(n_draws, seed=seed, z=z, beta=self._beta, rtol=rtol, max_iter=max_iter,
                                         batch=batch, where=where)

    # -- probabilities --------------------------------------------------------------------
    def _logistic_normal(self, mu, var):
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.device)  # noqa: E731
        return _lib.logistic_normal(to(mu), to(np.sqrt(np.maximum(var, 0.0)))).cpu().numpy()

    def probability(self, where: str = "data", n_draws: int = 64, seed: int = 0, rtol: float = 1e-8,
                    max_iter: Optional[int] = None, batch=None) -> np.ndarray:
        """Posterior mean success probability E[logistic(x beta_hat + w)] at every row of ``coords`` (unobserved rows
        included) or, ``where="ref"``, of the reference set (with covariates that needs ``X_ref``): the latent mode
        and :meth:`marginal_variance` (``n_draws``, ``seed``) through ``nngp_logistic_normal``."""
        self._check_where(where)
        self._ensure_mode()
        if where == "ref" and self._ref and self.p > 0 and not self._has_x_ref:
            raise ValueError("probability(where='ref') with covariates needs X_ref")
        rows = self._rows_of(where)
        mu = (self._xb(self._beta) + self._w)[rows].cpu().numpy()
        var = self.marginal_variance(n_draws, seed=seed, rtol=rtol, max_iter=max_iter, batch=batch, where=where)
        return self._logistic_normal(mu, var)

    def _query_variance(self, q_host, rtol, max_iter, batch):
        """Exact latent variances at query points, as unobserved leaves: sigma2 F_q + B_q A_S^-1 B_q^T, one solve
        per point, ``batch`` at a time."""
        dev, n_s, cov = self.device, self.n_s, self.cov
        q = torch.from_numpy(q_host).to(dev)
        s_coords = self.coords[:n_s].contiguous()
        k = min(self.m, n_s)
        nbr_q = _lib.knn_query(s_coords, q, k)
        B_q, F_q, part = _lib.bf_cross(s_coords, q, nbr_q, cov.kind, 1.0, cov.phi, 0.0, nu=cov.nu_arg)
        _raise_on_bad(part.cpu().numpy())
        idx = nbr_q.long().clamp(min=0)
        Bv = torch.where(nbr_q >= 0, B_q, torch.zeros_like(B_q))
        Q = q_host.shape[0]
        var = cov.sigma2 * F_q
        max_iter = self._cg_args(rtol, max_iter)
        for k0 in range(0, Q, batch):
            k1 = min(Q, k0 + batch)
            R = torch.zeros((n_s, k1 - k0), dtype=torch.float64, device=dev)
            cols = torch.arange(k1 - k0, device=dev)[:, None].expand(-1, k)
            R.index_put_((idx[k0:k1], cols), Bv[k0:k1], accumulate=True)
            XS, info = self._solve_cols(R, rtol, max_iter)
            self._report(info, rtol, first=k0)
            var[k0:k1] += (Bv[k0:k1] * XS[idx[k0:k1], cols]).sum(dim=1)
        return var.cpu().numpy()

    EXACT_VAR_MAX_Q = 256  # predict's default: exact variances (one solve per point) up to this many query points

    def predict(self, query, n_draws: int = 0, seed: int = 0, X_query=None, var_draws: Optional[int] = None,
                rtol: float = 1e-8, max_iter: Optional[int] = None, batch=None):
        """Success probabilities at new locations ``query`` (Q, d): ``(prob, draws)``.  A query point is an unobserved
        leaf of the reference set, as in :meth:`LatentPosterior.predict`, which supplies the latent mean B_q w_hat_S
        and the latent draws; ``prob`` = E[logistic(x_q beta_hat + w_q)] under the Laplace approximation through
        ``nngp_logistic_normal``, ``draws`` (n_draws, Q) = logistic(x_q beta_hat + w_q^(k)).  The latent variance is
        exact -- sigma2 F_q + B_q A_S^-1 B_q^T, one solve per point -- for ``var_draws=0`` (the default up to
        ``EXACT_VAR_MAX_Q`` points) or the parent's estimate over ``var_draws`` >= 2 draws (the default, 64, beyond).
        ``X_query`` (Q, p): covariates at the query points, required when the model has covariates."""
        n_draws = int(n_draws)
        if n_draws < 0:
            raise ValueError("n_draws must be >= 0")
        batch = self._batch(batch)
        self._ensure_mode()
        q_host = np.ascontiguousarray(query.detach().cpu().numpy() if isinstance(query, torch.Tensor) else query,
                                      dtype=np.float64)
        if q_host.ndim == 1:
            q_host = q_host[:, None]
        Q = q_host.shape[0]
        if self.p > 0:
            if X_query is None:
                raise ValueError("the model has covariates: predict needs X_query")
            xq = np.asarray(X_query, dtype=np.float64)
            xq = xq[:, None] if xq.ndim == 1 else xq
            if xq.shape != (Q, self.p) or not np.all(np.isfinite(xq)):
                raise ValueError(f"X_query must be finite ({Q}, {self.p}), got {xq.shape}")
            off = xq @ self._beta
        else:
            off = np.zeros(Q)
        if var_draws is None:
            var_draws = 0 if Q <= self.EXACT_VAR_MAX_Q else 64
        var_draws = int(var_draws)
        if var_draws == 1 or var_draws < 0:
            raise ValueError("var_draws must be 0 (exact) or >= 2")
        k_all = max(n_draws, var_draws)
        mean, var, draws = super().predict(q_host, n_draws=k_all, seed=seed, beta=self._beta, rtol=rtol,
                                           max_iter=max_iter, batch=batch)
        if Q == 0:
            return np.zeros(0), np.zeros((n_draws, 0))
        if var_draws == 0:
            var = self._query_variance(q_host, rtol, max_iter, batch)
        t = off[None, :] + draws[:n_draws]
        e = np.exp(-np.abs(t))
        return self._logistic_normal(off + mean, var), np.where(t >= 0, 1.0 / (1.0 + e), e / (1.0 + e))

    # -- the Laplace evidence ---------------------------------------------------------------
    def log_marginal(self, n_probes: int = 32, seed: int = 0, z=None, rtol: float = 1e-8,
                     max_iter: Optional[int] = None, batch=None, logdet_rtol: float = 1e-6):
        """``(value, se)``: the Laplace evidence log p(s | theta) (module docstring) at the mode.  log det A_S is the
        parent's stochastic Lanczos quadrature at d = W_hat (:meth:`LatentPosterior.logdet`; ``n_probes``, ``seed``,
        ``z``, ``batch``, ``logdet_rtol``), whose standard error, halved, is ``se``; the leaves' part of log det(Q + W)
        is the closed form sum log(f_j + W_j); everything else is exact to rounding.  beta is at its mode (a plug-in,
        as the parent's)."""
        st = self._ensure_mode()["st"]
        n_s = self.n_s
        f = 1.0 / (self.cov.sigma2 * self.F)
        ld = self._logdet_run(n_probes, seed, z, logdet_rtol, max_iter, batch)
        logdet = ld.value
        if self._has_leaves():
            logdet += float(torch.log(f[n_s:] + self.d[n_s:]).sum())
        value = st["ll"] - 0.5 * st["quad"] + 0.5 * float(torch.log(f).sum()) - 0.5 * logdet
        return value, 0.5 * ld.se

    def log_marginal_grad(self, *a, **k):
        raise NotImplementedError("the gradient of the Laplace evidence in theta needs the third-derivative term of "
                                  "the mode's dependence on theta (DESIGN 9); fit() is derivative-free")

    def fit(self, x0=None, n_probes: int = 32, seed: int = 0, method: str = "Nelder-Mead", maxiter: int = 200,
            maxfev: Optional[int] = None, z=None, rtol: float = 1e-8, batch=None, gtol: float = 1e-8,
            max_newton: int = 50):
        """Empirical-Bayes (sigma2, phi): maximise :meth:`log_marginal` over log (sigma2, phi) from ``x0`` -- a
        :class:`Covariance` of this kind or (sigma2, phi), default the current ``cov``.  Derivative-free
        (``scipy.optimize.minimize``, ``method``, at most ``maxiter`` iterations and ``maxfev`` evaluations) with
        common random numbers: every evaluation uses the same probes, so the objective is a deterministic function of
        theta and one seed gives one answer.  Each evaluation moves theta by :meth:`update` and starts its Newton
        iteration from the previous evaluation's mode.  Leaves the object at the best theta seen, its mode computed,
        and returns ``(cov, result)`` (``result.fun`` = -log_marginal there, ``result.se`` its standard error)."""
        from scipy.optimize import minimize

        base = self.cov
        if isinstance(x0, Covariance):
            th0 = x0.theta[:2]
        else:
            th0 = tuple(float(t) for t in x0)[:2] if x0 is not None else base.theta[:2]
        if len(th0) != 2 or not all(t > 0 and math.isfinite(t) for t in th0):
            raise ValueError(f"x0 must be (sigma2, phi), both positive, got {th0}")
        Z = None if z is None else np.array(z, dtype=np.float64)
        best = {"ll": -math.inf, "cov": None, "se": math.inf}

        def obj(lz):
            try:
                cov = base.replace(sigma2=math.exp(lz[0]), phi=math.exp(lz[1]))
                self.update(cov)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)
                    _, _, info = self.mode(gtol=gtol, max_newton=max_newton, rtol=rtol)
                if not info.converged:
                    return 1e300
                ll, se = self.log_marginal(n_probes=n_probes, seed=seed, z=Z, rtol=rtol, batch=batch)
            except (NNGPNumericalError, OverflowError, np.linalg.LinAlgError):
                self._beta = self._w = self._U_S = None
                return 1e300
            if not math.isfinite(ll):
                return 1e300
            if ll > best["ll"]:
                best.update(ll=ll, cov=cov, se=se)
            return -ll

        opts = {"maxiter": int(maxiter)}
        if maxfev is not None:
            opts["maxfev"] = int(maxfev)
        if method == "Nelder-Mead":
            opts.update(xatol=1e-4, fatol=1e-6)
        res = minimize(obj, np.log(np.array(th0)), method=method, options=opts)
        if best["cov"] is None:
            self.update(base)
            raise NNGPNumericalError("log_marginal could not be evaluated at any theta the optimiser tried")
        self.update(best["cov"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            self.mode(gtol=gtol, max_newton=max_newton, rtol=rtol)
        res.x, res.fun, res.se = np.log([best["cov"].sigma2, best["cov"].phi]), -best["ll"], best["se"]
        return best["cov"], res
