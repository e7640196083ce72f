"""``BinomialSeqNNGP``: Gibbs sampler for a binomial / logistic NNGP model on the GPU.

The reference's models are Gaussian in the response; spNNGP offers binary and count responses as
``family = "binomial"``.  This is that model on :class:`SeqNNGP`'s machinery:

    s_i ~ Binomial(b_i, logistic(x_i beta + w_i)),   w ~ NNGP(0, sigma2 R(phi))
    beta ~ flat,  sigma2 ~ IG(a_s, b_s),  phi ~ U(phi_lo, phi_hi)          (no tau2)

With Polya-Gamma augmentation (Polson, Scott and Windle 2013), omega_i ~ PG(b_i, x_i beta + w_i), the model is
conditionally Gaussian: given omega the update of w is :class:`SeqNNGP`'s colour sweep with the
heteroscedastic noise precision omega_i (``noise_w`` = omega, tau2 = 1) and the pseudo-response
kappa_i / omega_i, kappa_i = s_i - b_i / 2.  One iteration (``step``):

  1. phi | w, sigma2      -- Metropolis-Hastings, unchanged (it depends on w only);
  2. sigma2 | w, phi      -- unchanged;
  3. omega | beta, w      -- one launch (nngp_gibbs_pg_update: Devroye's exact sampler per location, Philox
                             counters of their own; it also writes yres = kappa / omega - X beta);
  4. w | omega, rest      -- update_wt, update_ws: the existing colour sweep;
  5. statistics           -- nngp_gibbs_pg_stats: sum r^2/F, X' Omega X, X'(kappa - Omega w);
  6. beta | omega, w      -- N(V X'(kappa - Omega w), V), V = (X' Omega X)^-1, on the host (a p x p Cholesky);
  7. X beta refreshed;
  8. ``prob_unobserved`` = logistic(x beta + w) at the unobserved nodes, and ``y_unobserved`` ~
     Binomial(b*, .) there when ``trials_unobserved`` was given.

omega is redrawn from (w, beta) at the top of every step, so a checkpoint is :class:`SeqNNGP`'s (plus X beta,
recomputed from beta): a resumed chain continues bit for bit.
"""
from __future__ import annotations

import hashlib
from typing import Optional

import numpy as np
import torch

from . import _lib
from .gibbs import Priors, SeqNNGP
from .nngp import NNGPNumericalError


def polya_gamma(trials: torch.Tensor, c: torch.Tensor, seed: int = 0, sweep: int = 0,
                status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """omega[i] ~ PG(trials[i], c[i]): exact Polya-Gamma draws on the GPU, one per location.

    ``trials``: int32 (n,) in [0, 1024] (0 gives exactly 0; refused outside the range, before any launch);
    ``c``: float64 (n,).  A draw depends on (seed, sweep, i, trials[i], c[i]) alone.  A non-finite c[i] makes
    omega[i] NaN: with ``status`` None that raises :class:`NNGPNumericalError` naming the first such location;
    with ``status`` an int32 (1,) device tensor the call returns and status holds 0 or that location + 1
    (faults as data, no exception).  CPU tensors raise NotImplementedError (there is no CPU path)."""
    omega, st = _lib.polya_gamma(trials, c, seed, sweep, status=status)
    if status is None:
        _raise_on_status(st)
    return omega


def _raise_on_status(status: torch.Tensor, what: str = "c") -> None:
    k = int(status.item())
    if k != 0:
        raise NNGPNumericalError(f"Polya-Gamma draw failed at location {k - 1}: {what} is not finite there (or the "
                                 "sampler hit a loop cap); omega is NaN at every such location")


class BinomialSeqNNGP(SeqNNGP):
    """Binomial / logistic NNGP Gibbs sampler (see module docstring).

    ``successes`` (n,) integers in [0, trials]; ``trials`` (n,) integers in [0, 1024] (Bernoulli data:
    trials = 1).  ``trials = 0`` or a NaN in ``successes`` marks a location as unobserved: it enters no
    likelihood term and gets ``prob_unobserved`` (and ``y_unobserved`` ~ Binomial(trials_unobserved, .) when
    ``trials_unobserved`` -- a scalar or one count per unobserved node, ``unobserved_t`` then
    ``unobserved_ref`` -- is given).  Everything else (``ref``, ``X_ref``, ``kind``, ``priors``, ``fix_phi``, ...)
    is :class:`SeqNNGP`'s; there is no tau2, and ``eps``, ``sweep="tiled"`` and a callable ``cov`` are refused."""

    family = "binomial"

    def __init__(self, coords, successes, trials, X=None, m: int = 15, kind: str = "exponential",
                 priors: Optional[Priors] = None, sigma2: float = 1.0, phi: Optional[float] = None,
                 phi_tuning: float = 0.05, seed: int = 0, device=None, algo: str = "auto", w_init=None, ref=None,
                 X_ref=None, nu: Optional[float] = None, fix_phi: bool = False, fix_sigma2: bool = False,
                 trials_unobserved=None, **refused):
        for k in refused:
            if k == "eps" and refused[k] is not None:
                raise ValueError("the binomial model has no measurement sigmas (eps): its noise precision is the "
                                 "Polya-Gamma omega")
            if k == "sweep" and refused[k] != "colour":
                raise NotImplementedError("the binomial sampler runs the colour sweep (sweep='tiled' is Gaussian only)")
            if k == "cov" and refused[k] is not None:
                raise NotImplementedError("the binomial sampler runs the built-in covariance kinds, not a callable cov")
            if k in ("tau2", "fix_tau2"):
                raise ValueError("the binomial model has no tau2")
            if k not in ("eps", "sweep", "cov"):
                raise TypeError(f"unexpected argument {k!r}")
        s = np.asarray(successes, dtype=np.float64).reshape(-1)
        b_in = np.asarray(trials)
        if b_in.dtype.kind == "f":
            if not np.all(np.isfinite(b_in)) or np.any(b_in != np.round(b_in)):
                raise ValueError("trials must be integers")
        elif b_in.dtype.kind not in "iu":
            raise ValueError("trials must be integers")
        b = b_in.reshape(-1).astype(np.int64)
        n_t = s.shape[0]
        if b.shape != (n_t,):
            raise ValueError(f"trials must hold one count per location ({n_t}), got {b.shape}")
        if np.any(b < 0) or np.any(b > _lib.PG_MAX_TRIALS):
            raise ValueError(f"trials must lie in [0, {_lib.PG_MAX_TRIALS}]")
        if np.any(np.isinf(s)):
            raise ValueError("successes must be finite or NaN (NaN = unobserved)")
        observed = np.isfinite(s) & (b > 0)
        so = s[observed]
        if np.any(so != np.round(so)):
            raise ValueError("successes must be integers")
        if np.any(so < 0) or np.any(so > b[observed]):
            raise ValueError("successes must lie in [0, trials]")
        # the parent's response: the empirical logits (NaN = unobserved).  It only seeds the start -- beta by
        # least squares, w by the 5-NN mean of the residuals -- and enters the data fingerprint.
        y0 = np.full(n_t, np.nan)
        y0[observed] = np.log((so + 0.5) / (b[observed] - so + 0.5))
        super().__init__(coords, y0, X, m=m, kind=kind, priors=priors, sigma2=sigma2, tau2=1.0, phi=phi,
                         phi_tuning=phi_tuning, seed=seed, device=device, algo=algo, w_init=w_init, eps=None,
                         fix_tau2=True, ref=ref, X_ref=X_ref, nu=nu, cov=None, fix_phi=fix_phi,
                         fix_sigma2=fix_sigma2, sweep="colour")
        if self.p < 1:
            raise ValueError("X needs at least one column")
        dev, n = self.device, self.n
        # per node, storage order: trials (0 = no observation) and kappa = s - b / 2
        node = self.node_of_t.cpu().numpy()
        b_n, s_n = np.zeros(n, dtype=np.int32), np.zeros(n)
        b_n[node[observed]] = b[observed]
        s_n[node[observed]] = so
        self._data_hash = hashlib.sha256(b_n.tobytes() + s_n.tobytes()).hexdigest()
        self.trials = torch.from_numpy(b_n).to(dev)[self.perm].contiguous()
        self.kappa = (torch.from_numpy(s_n).to(dev)[self.perm] - 0.5 * self.trials.double()).contiguous()
        k_un = self._un_nodes.numel()
        self._un_trials = None
        if trials_unobserved is not None:
            tu = np.broadcast_to(np.asarray(trials_unobserved), (k_un,)).astype(np.float64)
            if np.any(tu < 0) or np.any(tu != np.round(tu)):
                raise ValueError("trials_unobserved must hold non-negative integers")
            self._un_trials = torch.from_numpy(np.ascontiguousarray(tu)).to(dev)
        self.prob_unobserved = torch.zeros(k_un, dtype=torch.float64, device=dev)
        # buffers of the step: omega (the w sweep's noise_w), yres (the parent's buffer), X beta, the statistics
        self.omega = torch.zeros(n, dtype=torch.float64, device=dev)
        self.noise_w = self.omega
        self.xb = torch.empty(n, dtype=torch.float64, device=dev)
        self._pg_status = torch.zeros(1, dtype=torch.int32, device=dev)
        self._nv = 1 + self.p * (self.p + 1) // 2 + self.p
        self._pg_stats_buf = torch.empty(self._nv, dtype=torch.float64, device=dev)
        self._pg_stats_ws = _lib._workspace(_lib.load().nngp_gibbs_pg_stats_workspace_bytes(n, self.p), dev)
        self._iu = np.triu_indices(self.p)
        self._refresh_xb()
        self._update_unobserved()

    # ------------------------------------------------------------------ pieces
    def _refresh_xb(self):
        """X beta per node (storage order), column by column as the parent forms y - X beta."""
        torch.mul(self._Xcols[0], float(self.beta[0]), out=self.xb)
        for c in range(1, self.p):
            self.xb.add_(self._Xcols[c], alpha=float(self.beta[c]))

    def _draw_omega(self):
        """omega | beta, w and the w sweep's pseudo-residuals yres = kappa / omega - X beta, one launch."""
        _lib.gibbs_pg_update(self.trials, self.kappa, self.xb, self.w, self.seed, self.iteration, omega=self.omega,
                             yres=self.yres, status=self._pg_status, checked=True)

    def _stats_dev(self):
        return _lib.gibbs_pg_stats(self.r, self.Ft, self.omega, self.kappa, self.X, self.w, out=self._pg_stats_buf,
                                   workspace=self._pg_stats_ws)

    def _update_unobserved(self, draw: bool = True):
        """prob_unobserved = logistic(x beta + w) at the unobserved nodes; y_unobserved ~ Binomial(b*, .)."""
        if self._un_nodes.numel() == 0:
            return
        eta = self._un_X @ torch.as_tensor(self.beta, dtype=torch.float64, device=self.device) + self.w[self._un_nodes]
        torch.sigmoid(eta, out=self.prob_unobserved)
        if draw and self._un_trials is not None:
            # a generator keyed by (seed, iteration): a resumed chain draws the same counts
            g = torch.Generator(device=self.device)
            g.manual_seed((self.seed * 0x9E3779B97F4A7C15 + self.iteration) % (2 ** 63))
            self.y_unobserved.copy_(torch.binomial(self._un_trials, self.prob_unobserved, generator=g))

    def update_y_unobserved(self):
        self._update_unobserved()

    def step(self):
        """One iteration: phi; sigma2; omega; update_wt; update_ws; beta; the unobserved probabilities."""
        self.update_phi()
        self._before_w()
        self._draw_omega()
        self.update_wt()
        self.update_ws()
        self._after_w(self._stats())

    def _after_w(self, st):
        """beta | omega, w from the host statistics ``st`` of the new w; X beta; the unobserved nodes."""
        k = int(self._pg_status.item())  # (the statistics' copy has synchronised the stream already)
        if k != 0:
            raise NNGPNumericalError(f"Polya-Gamma draw failed at storage row {k - 1} (node {int(self.perm[k - 1])}) "
                                     f"in iteration {self.iteration}: x beta + w is not finite there")
        self.quad = float(st[0])
        p = self.p
        A = np.zeros((p, p))
        A[self._iu] = st[1:1 + p * (p + 1) // 2]
        A = A + np.triu(A, 1).T
        rhs = st[1 + p * (p + 1) // 2:]
        try:
            if not (np.all(np.isfinite(A)) and np.all(np.isfinite(rhs))):
                raise np.linalg.LinAlgError("non-finite statistics")
            L = np.linalg.cholesky(A)
            if not np.all(np.isfinite(L)) or np.min(np.diag(L)) ** 2 <= 1e-14 * np.max(np.diag(A)):
                raise np.linalg.LinAlgError("singular")
        except np.linalg.LinAlgError as e:
            raise NNGPNumericalError(f"X' Omega X is singular or not finite in iteration {self.iteration} ({e}): "
                                     "beta has no proper full conditional (collinear covariates over the observed "
                                     "locations, or complete separation without a field)") from None
        mean = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
        self.beta = mean + np.linalg.solve(L.T, self.rng.standard_normal(p))
        self._refresh_xb()
        self.iteration += 1
        self._update_unobserved()

    def probability(self, where: str = "data") -> torch.Tensor:
        """The current logistic(x beta + w): ``where`` = "data" (the data locations, input order), "nodes" (model
        node order) or "unobserved" (``prob_unobserved``)."""
        if where == "unobserved":
            return self.prob_unobserved
        pr = torch.sigmoid(self.xb + self.w)
        if where == "data":
            return pr[self.pos[self.node_of_t]]
        if where == "nodes":
            return pr[self.pos]
        raise ValueError("where must be 'data', 'nodes' or 'unobserved'")

    def clone(self, seed: int):
        raise NotImplementedError("multi-chain binomial runs are out of scope: build one BinomialSeqNNGP per chain")

    # ------------------------------------------------------------------ checkpoint / resume
    def _settings(self) -> dict:
        s = super()._settings()
        s["family"] = "binomial"
        s["binomial_data"] = getattr(self, "_data_hash", None)
        return s

    def _fingerprint(self, node_order: bool = True) -> str:
        # noise_w is omega here: state, redrawn every step, not data (trials and successes enter by _settings)
        keep, self.noise_w = self.noise_w, None
        try:
            return super()._fingerprint(node_order)
        finally:
            self.noise_w = keep

    def restore(self, path) -> "BinomialSeqNNGP":
        super().restore(path)
        self.tau2 = 1.0
        self.noise_w = self.omega
        self._refresh_xb()
        self._update_unobserved(draw=False)  # y_unobserved came back with the checkpoint
        return self

    def load(self, path) -> "BinomialSeqNNGP":
        """Resume from :meth:`save` (= :meth:`restore`): the sampler must be built on the same data and settings."""
        return self.restore(path)

    # ------------------------------------------------------------------ runs
    def run(self, n_iter: int, burn: int = 0):
        """Run ``n_iter`` iterations and summarise the ``n_iter - burn`` kept ones: the draws of beta, sigma2 and
        phi (as :meth:`SeqNNGP.sample` returns them), ``summary[name]`` = mean and the 2.5 / 50 / 97.5 % quantiles
        of each, and the posterior mean and sd of the probabilities at the data locations (``prob_mean``,
        ``prob_sd``; input order) and at the unobserved nodes (``prob_unobserved_mean``) -- running moments: the
        draws of a field of 1e6 probabilities are not kept, so the probabilities get no quantiles."""
        if not 0 <= burn < n_iter:
            raise ValueError("need 0 <= burn < n_iter")
        out = {"beta": [], "sigma2": [], "phi": []}
        p1, p2 = torch.zeros_like(self.w), torch.zeros_like(self.w)
        pu = torch.zeros_like(self.prob_unobserved)
        yu = torch.zeros_like(self.y_unobserved)
        for k in range(n_iter):
            self.step()
            if k >= burn:
                out["beta"].append(self.beta.copy())
                out["sigma2"].append(self.sigma2)
                out["phi"].append(self.phi)
                pr = torch.sigmoid(self.xb + self.w)
                p1 += pr
                p2.addcmul_(pr, pr)
                pu += self.prob_unobserved
                yu += self.y_unobserved
        kept = n_iter - burn
        res = {k: np.asarray(v) for k, v in out.items()}
        q = lambda a: {"mean": a.mean(axis=0), "q025": np.quantile(a, 0.025, axis=0),  # noqa: E731
                       "q50": np.quantile(a, 0.5, axis=0), "q975": np.quantile(a, 0.975, axis=0)}
        res["summary"] = {k: q(res[k]) for k in ("beta", "sigma2", "phi")}
        res["phi_accept_rate"] = self.n_accept / max(self.iteration, 1)
        idx = self.pos[self.node_of_t]
        mean = p1 / kept
        res["prob_mean"] = mean[idx].cpu().numpy()
        res["prob_sd"] = torch.sqrt(torch.clamp(p2 / kept - mean * mean, min=0.0))[idx].cpu().numpy()
        if self.prob_unobserved.numel():
            res["prob_unobserved_mean"] = (pu / kept).cpu().numpy()
            if self._un_trials is not None:
                res["y_unobserved_mean"] = (yu / kept).cpu().numpy()
        return res
