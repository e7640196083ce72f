"""Nonstationary NNGP: :class:`NonstationaryCovariance` and :class:`NonstationaryNNGP`.

Every point carries its own variance, decay and nugget (Paciorek & Schervish 2006 with kernel matrices phi_i^-2 I)::

    C(i, j) = sigma_i sigma_j x^(d/2) rho(u) + tau2_i delta_ij,
    x = 2 phi_i phi_j / (phi_i^2 + phi_j^2),   u^2 = 2 |s_i - s_j|^2 phi_i^2 phi_j^2 / (phi_i^2 + phi_j^2)

with rho the exponential, Matern-3/2, Matern-5/2 or gaussian correlation, 1..3 coordinate columns and 1 <= m <= 32
neighbours.  The covariance depends on the points' fields, so :class:`pynngp_amd.NNGP` cannot hold it; the factors
come from ``nngp_bf_sweep_ns`` / ``nngp_bf_cross_ns``.  The neighbour sets are the prior sets on the
raw coordinates, or the caller's.  There is no analytic gradient yet: :meth:`NonstationaryNNGP.fit` differences the
sweep.
"""
import dataclasses
import math

import numpy as np
import torch

from . import _lib, regression
from .nngp import LOG_2PI, NNGPNumericalError, _default_device, _raise_on_bad


@dataclasses.dataclass(frozen=True, eq=False)
class NonstationaryCovariance:
    """``kind`` one of exponential, matern32, matern52, gaussian; ``sigma2`` > 0, ``phi`` > 0 and ``tau2`` >= 0 each
    an (n,) array (numpy or a device tensor), one value per point in the caller's row order, or a scalar that is
    broadcast.  The values are checked on the device by the sweep."""

    kind: str
    sigma2: object
    phi: object
    tau2: object = 0.0

    def __post_init__(self):
        _lib._ns_checks(self.kind, 1)

    def fields(self, n: int, device):
        """The three fields as contiguous float64 (n,) tensors on ``device``."""
        out = []
        for name in ("sigma2", "phi", "tau2"):
            f = torch.as_tensor(getattr(self, name), dtype=torch.float64).to(device)
            if f.dim() > 1 or (f.dim() == 1 and f.shape[0] != n):
                raise ValueError(f"{name} must be a scalar or ({n},), got {tuple(f.shape)}")
            out.append(f.expand(n).contiguous())
        return tuple(out)


def _raise_on_flags(p):
    if p[3] >= 0:
        raise ValueError(f"location {int(p[3])} holds a point whose sigma2 or phi is not positive and finite or whose "
                         "tau2 is negative, or a neighbour index out of range")
    _raise_on_bad(p)


class NonstationaryNNGP:
    """NNGP for ``y`` (N,) at the points ``t`` (N, 1..3) under a :class:`NonstationaryCovariance`; ``X`` (N, p),
    optional, is the design of a linear mean (the caller adds the intercept column).  ``ordering`` None, "random",
    "maxmin" or a permutation: rows are held in that order (``perm`` maps positions to input rows; the covariance's
    fields stay in input order).  ``nbr``: int32 (N, m) prior neighbour sets in the held order to use instead of
    the m nearest earlier points."""

    def __init__(self, t, y, m, cov: NonstationaryCovariance, X=None, ordering=None, nbr=None, device=None):
        if not isinstance(cov, NonstationaryCovariance):
            raise TypeError("cov must be a NonstationaryCovariance")
        t, y = (np.array(a, dtype=np.float64, order="C") for a in (t, y))
        t = t[:, None] if t.ndim == 1 else t
        if t.ndim != 2 or not 1 <= t.shape[1] <= _lib.MAX_DIM:
            raise NotImplementedError(f"the nonstationary model serves 1 .. {_lib.MAX_DIM} coordinate columns, t is "
                                      f"{t.shape}")
        n = t.shape[0]
        if y.shape != (n,):
            raise ValueError(f"y must be ({n},), got {y.shape}")
        if not (np.all(np.isfinite(t)) and np.all(np.isfinite(y))):
            raise ValueError("Input contains NaN or infinity")
        self.m = int(m)
        _lib._ns_checks(cov.kind, self.m)
        self.cov = cov
        self.device = _default_device(device)
        self.perm = None
        if ordering is not None:
            from . import ordering as _ordering

            self.perm = _ordering.resolve(ordering, torch.as_tensor(t).to(self.device))
            t, y = np.ascontiguousarray(t[self.perm]), np.ascontiguousarray(y[self.perm])
            X = None if X is None else np.asarray(X, dtype=np.float64)[self.perm]
        self._perm_dev = None if self.perm is None else torch.as_tensor(self.perm).to(self.device)
        self.t, self.y = t, y
        self._t_dev = torch.as_tensor(t).to(self.device)
        self._y_dev = torch.as_tensor(y).to(self.device)
        self._x_dev = None if X is None else regression.design(self, np.ascontiguousarray(X), n)
        if nbr is None:
            self.nbr = _lib.knn_prior(self._t_dev, self.m)
        else:
            self.nbr = torch.as_tensor(nbr, dtype=torch.int32).to(self.device).contiguous()
            if tuple(self.nbr.shape) != (n, self.m):
                raise ValueError(f"nbr must be int32 ({n}, {self.m}), got {tuple(self.nbr.shape)}")
        self._B = self._F = None

    # -- helpers -------------------------------------------------------------------------------------------------
    def _held(self, a):
        """A per-point array in input order, in the held order."""
        return a if self._perm_dev is None else a[self._perm_dev].contiguous()

    def _model(self, cov):
        """(kind, the three fields in the held order) of ``cov`` (default the instance's)."""
        cv = self.cov if cov is None else cov
        if not isinstance(cv, NonstationaryCovariance):
            raise TypeError("cov must be a NonstationaryCovariance")
        return cv.kind, tuple(self._held(f) for f in cv.fields(self.t.shape[0], self.device))

    def _design(self, mean):
        if mean is None:
            return None
        if mean == "constant":
            return torch.ones((self.t.shape[0], 1), dtype=torch.float64, device=self.device)
        if mean != "linear":
            raise ValueError(f"mean must be None, 'constant' or 'linear', got {mean!r}")
        if self._x_dev is None:
            raise ValueError("mean='linear' needs the design matrix X (the constructor's X=)")
        return self._x_dev

    def _gls(self, kind, fields, X, v):
        """One sweep that writes B and F, then one ``nngp_whiten_gram`` on [v, X]."""
        B, F, _, p = _lib.bf_sweep_ns(self._t_dev, self.nbr, 0, kind, fields, want_bf=True)
        V = torch.cat([v[:, None], X], dim=1).contiguous()
        _, G = _lib.whiten_gram(self.nbr, B, F, V, 0)
        host = torch.cat([p, G.reshape(-1)]).cpu().numpy()  # one copy: the partials and the Gram matrix
        _raise_on_flags(host[:4])
        k = V.shape[1]
        return regression.gls_from_gram(host[4:].reshape(k, k).copy(), float(host[0]), v.shape[0])

    def _loglik(self, kind, fields, X):
        if X is not None:
            return self._gls(kind, fields, X, self._y_dev).loglik
        _, _, _, p = _lib.bf_sweep_ns(self._t_dev, self.nbr, 0, kind, fields, values=self._y_dev, want_bf=False)
        h = p.cpu().numpy()
        _raise_on_flags(h)
        return -0.5 * (self.nbr.shape[0] * LOG_2PI + h[0] + h[1])

    # -- the served methods --------------------------------------------------------------------------------------
    def compute_BF(self, cov=None):
        """B (N, m) and F (N,) on the GPU at ``cov`` (default the instance's; then cached as ``B`` and ``F``)."""
        kind, fields = self._model(cov)
        B, F, _, p = _lib.bf_sweep_ns(self._t_dev, self.nbr, 0, kind, fields, want_bf=True)
        _raise_on_flags(p.cpu().numpy())
        if cov is None:
            self._B, self._F = B, F
        return B, F

    @property
    def B(self):
        return self.compute_BF()[0] if self._B is None else self._B

    @property
    def F(self):
        return self.compute_BF()[1] if self._F is None else self._F

    def loglik(self, cov=None, mean=None) -> float:
        """The NNGP log-likelihood of y at ``cov``; ``mean`` None (zero), "constant" or "linear" (X beta profiled
        out by ``nngp_whiten_gram`` on this sweep's B and F)."""
        return self._loglik(*self._model(cov), self._design(mean))

    def gls(self, cov=None, mean="linear"):
        """GLS of y on X (or on the constant) under the NNGP precision at ``cov``: a
        :class:`pynngp_amd.regression.GLSResult`."""
        return self._gls(*self._model(cov), self._design(mean), self._y_dev)

    def profile_loglik(self, cov=None, mean="linear"):
        """``(loglik, beta)`` with the mean profiled out at ``cov``."""
        res = self.gls(cov, mean)
        return res.loglik, res.beta

    def predict(self, query, cov_query: NonstationaryCovariance, X_query=None, noise: bool = True, cov=None):
        """Kriging of y at ``query`` (n_q, dim) from each point's m nearest data points: numpy ``(mean, var)``.
        ``cov_query`` holds the fields at the query points (its ``tau2`` is left out of the variance with ``noise``
        False).  With an ``X`` on the instance, ``X_query`` (n_q, p) is required and the mean is
        x_q' beta + B_q (y - X beta)_N at the GLS beta."""
        kind, fields = self._model(cov)
        q = np.ascontiguousarray(query, dtype=np.float64)
        q = q[:, None] if q.ndim == 1 else q
        if q.ndim != 2 or q.shape[1] != self.t.shape[1]:
            raise ValueError(f"query must be (n_q, {self.t.shape[1]}), got {q.shape}")
        qd = torch.as_tensor(q).to(self.device)
        if not isinstance(cov_query, NonstationaryCovariance) or cov_query.kind != kind:
            raise ValueError(f"cov_query must be a NonstationaryCovariance of kind {kind!r}")
        fq = cov_query.fields(q.shape[0], self.device)
        if not noise:
            fq = (fq[0], fq[1], torch.zeros_like(fq[2]))
        v, shift = self._y_dev, 0.0
        if (self._x_dev is None) != (X_query is None):
            raise ValueError("X_query goes with the instance's X: give both or neither")
        if X_query is not None:
            beta = torch.from_numpy(self._gls(kind, fields, self._x_dev, self._y_dev).beta).to(self.device)
            Xq = regression.design(self, X_query, q.shape[0], "X_query")
            v, shift = (self._y_dev - self._x_dev @ beta).contiguous(), Xq @ beta
        _, F, R, p = _lib.bf_cross_ns(self._t_dev, qd, _lib.knn_query(self._t_dev, qd, self.m), kind, fields, fq,
                                      ref_values=v, want_r=True)
        _raise_on_flags(p.cpu().numpy())
        return (shift - R).cpu().numpy(), F.cpu().numpy()

    def simulate(self, n_draws: int = 1, seed: int = 0, cov=None):
        """``(n_draws, N)`` draws of y (zero mean, the nuggets included) from the NNGP of ``cov`` in input row order:
        w = (I - B)^-1 F^1/2 z by the factor's level-scheduled solve (:class:`pynngp_amd.NNGPFactor`'s draw kernel)
        on this sweep's B and F, z Philox normals keyed by ``seed``."""
        B, F = self.compute_BF(cov)
        sched = _lib.factor_levels(self.nbr.cpu().numpy(), False, device=self.device)
        out = torch.empty((self.t.shape[0], int(n_draws)), dtype=torch.float64, device=self.device)
        for k0 in range(0, int(n_draws), _lib.LATENT_MAX_RHS):
            kc = min(_lib.LATENT_MAX_RHS, int(n_draws) - k0)
            out[:, k0:k0 + kc] = _lib.factor_prior_draw_batch(self.nbr, B, F, sched, 1.0, kc, seed=seed, draw0=k0)
        if self._perm_dev is not None:
            out = torch.empty_like(out).index_copy_(0, self._perm_dev, out)
        return out.t().cpu().numpy()

    def fit(self, Z_sigma2=None, Z_phi=None, Z_tau2=None, start=None, method: str = "L-BFGS-B", fix_tau2=None,
            maxiter: int = 200) -> dict:
        """Maximum likelihood of the log-linear field model log sigma2 = Z_sigma2 alpha, log phi = Z_phi gamma,
        log tau2 = Z_tau2 delta.  Each Z is (N, k) in input row order -- covariates or basis functions, the intercept
        column included -- or None: one column of ones, a constant field.  ``fix_tau2``: a scalar nugget held fixed
        (no delta).  ``start``: a dict with any of ``alpha``, ``gamma``, ``delta``; default the flat fields at the
        means of the instance's log fields.  ``method`` "L-BFGS-B" (on central differences of the sweep) or
        "Nelder-Mead".  The linear mean is profiled out when the instance has an ``X``.  The fields are recomputed on
        the device, one matmul each per evaluation.  Returns a dict with ``alpha``, ``gamma``, ``delta``, ``cov`` (the
        fitted fields, in input row order), ``loglik``, ``n_evals``, ``converged``; the instance's covariance becomes
        the estimate."""
        from scipy.optimize import minimize

        if method not in ("L-BFGS-B", "Nelder-Mead"):
            raise ValueError(f"method must be 'L-BFGS-B' or 'Nelder-Mead', got {method!r}")
        n, kind = self.t.shape[0], self.cov.kind
        names = ("alpha", "gamma") + (() if fix_tau2 is not None else ("delta",))
        Zs, x0 = [], []
        for name, Z, f in zip(names, (Z_sigma2, Z_phi, Z_tau2), self.cov.fields(n, self.device)):
            Z = (torch.ones((n, 1), dtype=torch.float64, device=self.device) if Z is None else
                 self._held(regression.design(self, Z, n, "Z_" + name)))
            c = np.zeros(Z.shape[1])
            c[0] = float(torch.log(f.clamp_min(1e-12)).mean())
            if start is not None and name in start:
                c = np.asarray(start[name], dtype=np.float64).reshape(Z.shape[1])
            Zs.append(Z)
            x0.append(c)
        cuts = np.cumsum([len(c) for c in x0])[:-1]
        X = self._x_dev
        tau_fixed = None if fix_tau2 is None else torch.full((n,), float(fix_tau2), dtype=torch.float64,
                                                             device=self.device)
        count = [0]

        def held_fields(x):
            parts = np.split(np.asarray(x, dtype=np.float64), cuts)
            f = [torch.exp(Z @ torch.from_numpy(c).to(self.device)) for Z, c in zip(Zs, parts)]
            return tuple(f) if tau_fixed is None else (f[0], f[1], tau_fixed)

        def nll(x):
            count[0] += 1
            try:
                return -self._loglik(kind, held_fields(x), X)
            except (NNGPNumericalError, ValueError, OverflowError):
                return 1e300

        def grad(x):  # central differences; the analytic gradient sweep is not built
            g = np.empty_like(x)
            for k in range(len(x)):
                h = 1e-4 * max(1.0, abs(x[k]))
                e = np.zeros_like(x)
                e[k] = h
                g[k] = (nll(x + e) - nll(x - e)) / (2.0 * h)
            return g

        x0 = np.concatenate(x0)
        if method == "L-BFGS-B":
            res = minimize(nll, x0, jac=grad, method="L-BFGS-B", options={"maxiter": maxiter, "ftol": 1e-12})
        else:
            res = minimize(nll, x0, method="Nelder-Mead",
                           options={"maxiter": 400 * len(x0), "xatol": 1e-6, "fatol": 1e-9, "adaptive": True})
        if not math.isfinite(res.fun) or res.fun >= 1e300:
            raise NNGPNumericalError("fit: no parameter value the optimiser tried was positive definite")
        fields = held_fields(res.x)
        if self._perm_dev is not None:  # back to input row order
            fields = tuple(torch.empty_like(f).index_copy_(0, self._perm_dev, f) for f in fields)
        self.cov = NonstationaryCovariance(kind, *fields)
        self._B = self._F = None
        out = dict(zip(names, np.split(res.x, cuts)))
        out.update(cov=self.cov, loglik=-float(res.fun), n_evals=count[0], converged=bool(res.success))
        return out
