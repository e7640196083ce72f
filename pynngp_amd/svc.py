"""Spatially varying coefficients: :class:`SVCCovariance` and :class:`SVCNNGP`.

The model (spBayes' ``spSVC``, ``varycoef``)::

    y(s) = x(s)' beta + sum_{k=1..r} z_k(s) w_k(s) + eps(s),   w_k ~ GP(0, sigma2_k rho(phi_k |.|)) independent,
    C(a, b) = sum_k z_ak z_bk sigma2_k rho(phi_k d_ab) + tau2 delta_ab

with ``Z`` (N, r) the covariates whose coefficients vary over space (a column of ones: the spatially varying
intercept), 1 <= r <= 4, one kind (exponential .. spherical) for every component, 1..3 coordinate columns and
1 <= m <= 32 neighbours.  The covariance depends on the points' covariates, so :class:`pynngp_amd.NNGP` cannot hold it;
the factors come from ``nngp_bf_sweep_svc`` / ``nngp_bf_cross_svc`` and the gradient in
(sigma2_1..r, phi_1..r, tau2) from ``nngp_bf_grad_svc``.  The neighbour sets are the prior sets on
the raw coordinates: the components have different ranges, so there is no single metric to search in.

A reference set other than the data, per-component kinds, the general-nu kind, per-point noise, the restricted
likelihood and the latent / Gibbs forms are not built: they raise ``NotImplementedError`` naming this scope.
"""
import dataclasses
import math

import numpy as np
import torch

from . import _lib, regression
from .nngp import LOG_2PI, NNGP, Covariance, NNGPNumericalError, _default_device, _raise_on_bad

SVC_SCOPE = (f"the varying-coefficient model serves S = T, 1 <= r <= {_lib.SVC_MAX_R} components of one kind among "
             f"{', '.join(_lib.SVC_KINDS)}, 1 .. {_lib.MAX_DIM} coordinate columns, 1 <= m <= {_lib.GRAD_MAX_M}, a zero "
             "or a linear mean, and the methods loglik, compute_BF, gls, profile_loglik, loglik_grad, fit, predict and "
             "coef")


def _refuse(what: str):
    raise NotImplementedError(f"{what} is not served: {SVC_SCOPE}")


@dataclasses.dataclass(frozen=True)
class SVCCovariance:
    """``kind`` one of exponential .. spherical (every component the same); ``sigma2`` (r,) >= 0 and ``phi`` (r,) > 0,
    the variance and decay of each coefficient surface; ``tau2`` >= 0 the noise variance; 1 <= r <= 4.  Called as
    ``cov(a, za, b, zb)`` on host coordinate rows and their covariates it returns the dense cross-covariance without
    the nugget."""

    kind: str
    sigma2: tuple
    phi: tuple
    tau2: float = 0.0

    def __post_init__(self):
        if self.kind not in _lib.KIND_CODES:
            raise ValueError(f"unknown covariance kind {self.kind!r}")
        if self.kind not in _lib.SVC_KINDS:
            _refuse(f"the {self.kind!r} kind")
        sigma2 = tuple(float(x) for x in np.ravel(self.sigma2))
        phi = tuple(float(x) for x in np.ravel(self.phi))
        if not 1 <= len(phi) <= _lib.SVC_MAX_R:
            _refuse(f"r={len(phi)} components")
        if len(sigma2) != len(phi):
            raise ValueError(f"sigma2 and phi must both hold r numbers, got {len(sigma2)} and {len(phi)}")
        if not all(x >= 0 and math.isfinite(x) for x in sigma2):
            raise ValueError(f"every sigma2_k must be non-negative and finite, got {sigma2}")
        if not all(x > 0 and math.isfinite(x) for x in phi):
            raise ValueError(f"every phi_k must be positive and finite, got {phi}")
        if not (self.tau2 >= 0 and math.isfinite(self.tau2)):
            raise ValueError("need tau2 >= 0 (finite)")
        object.__setattr__(self, "sigma2", sigma2)
        object.__setattr__(self, "phi", phi)
        object.__setattr__(self, "tau2", float(self.tau2))

    @property
    def r(self) -> int:
        return len(self.phi)

    @property
    def theta(self):
        """(sigma2_1..r, phi_1..r, tau2), (2 r + 1,)."""
        return (*self.sigma2, *self.phi, self.tau2)

    def replace(self, **kw) -> "SVCCovariance":
        return dataclasses.replace(self, **kw)

    def __call__(self, a, za, b, zb):
        a, b = np.atleast_2d(np.asarray(a, dtype=np.float64)), np.atleast_2d(np.asarray(b, dtype=np.float64))
        za, zb = np.atleast_2d(np.asarray(za, dtype=np.float64)), np.atleast_2d(np.asarray(zb, dtype=np.float64))
        out = np.zeros((a.shape[0], b.shape[0]))
        for k in range(self.r):
            out += np.outer(za[:, k], zb[:, k]) * Covariance(self.kind, self.sigma2[k], self.phi[k], 0.0)(a, b)
        return out


def _from_log(kind: str, r: int, x) -> SVCCovariance:
    e = np.exp(np.asarray(x, dtype=np.float64))
    return SVCCovariance(kind, e[:r], e[r:2 * r], float(e[2 * r]))


class SVCNNGP:
    """NNGP for ``y`` (N,) at the points ``t`` (N, 1..3) with the spatially varying covariates ``Z`` (N, r) under an
    :class:`SVCCovariance`; ``X`` (N, p), optional, is the design of the fixed part x' beta (the caller adds the
    intercept column; a column of Z usually appears in X too, its coefficient's mean).  ``ordering`` None, "random",
    "maxmin" or a permutation, as for :class:`pynngp_amd.MultivariateNNGP`: rows are held in that order (``perm``
    maps positions to input rows)."""

    def __init__(self, t, y, Z, m, cov: SVCCovariance, X=None, ordering=None, device=None):
        if not isinstance(cov, SVCCovariance):
            raise TypeError("cov must be an SVCCovariance")
        t, y, Z = (np.array(a, dtype=np.float64, order="C") for a in (t, y, Z))  # copies: the instance owns its rows
        t = t[:, None] if t.ndim == 1 else t
        Z = Z[:, None] if Z.ndim == 1 else Z
        if t.ndim != 2 or not 1 <= t.shape[1] <= _lib.MAX_DIM:
            _refuse(f"t of shape {t.shape}")
        n = t.shape[0]
        if y.shape != (n,) or Z.shape != (n, cov.r):
            raise ValueError(f"y must be ({n},) and Z ({n}, {cov.r}), got {y.shape} and {Z.shape}")
        if X is not None:
            X = np.ascontiguousarray(X, dtype=np.float64)
            X = X[:, None] if X.ndim == 1 else X
            if X.ndim != 2 or X.shape[0] != n:
                raise ValueError(f"X must be ({n}, p), got {X.shape}")
        if not all(np.all(np.isfinite(a)) for a in (t, y, Z) + (() if X is None else (X,))):
            raise ValueError("Input contains NaN or infinity")
        self.m = int(m)
        if not 1 <= self.m <= _lib.GRAD_MAX_M:
            _refuse(f"m={m}")
        self.cov, self.r = cov, cov.r
        self.device = _default_device(device)
        self.perm = None
        if ordering is not None:
            from . import ordering as _ordering

            self.perm = _ordering.resolve(ordering, torch.as_tensor(t).to(self.device))
            t, y, Z = (np.ascontiguousarray(a[self.perm]) for a in (t, y, Z))
            X = None if X is None else np.ascontiguousarray(X[self.perm])
        self.t, self.y, self.Z, self.X = t, y, Z, X
        self._t_dev = torch.as_tensor(t).to(self.device)
        self._z_dev = torch.as_tensor(Z).to(self.device)
        self._y_dev = torch.as_tensor(y).to(self.device)
        self._x_dev = None if X is None else regression.design(self, X, n)
        self.nbr = _lib.knn_prior(self._t_dev, self.m)
        self._B = self._F = None

    # -- helpers -------------------------------------------------------------------------------------------------
    def _model(self, cov) -> SVCCovariance:
        cv = self.cov if cov is None else cov
        if not isinstance(cv, SVCCovariance):
            raise TypeError("cov must be an SVCCovariance")
        if cv.r != self.r:
            raise ValueError(f"the covariance has {cv.r} components, Z has {self.r} columns")
        return cv

    def _values(self, values):
        if values is None:
            return self._y_dev
        v = torch.as_tensor(np.asarray(values, dtype=np.float64) if not isinstance(values, torch.Tensor) else values,
                            dtype=torch.float64).to(self.device)
        if v.shape != self._y_dev.shape:
            raise ValueError(f"one value per location is needed ({self._y_dev.shape[0]}, 1-D)")
        return v.contiguous()

    def _design(self, mean):
        if mean is None:
            return None
        if mean != "linear":
            _refuse(f"mean={mean!r}")
        if self._x_dev is None:
            raise ValueError("mean='linear' needs the design matrix X (the constructor's X=)")
        return self._x_dev

    def _sweep(self, cv, values=None, want_bf=False, want_r=False):
        B, F, R, p = _lib.bf_sweep_svc(self._t_dev, self._z_dev, self.nbr, 0, cv.kind, cv.sigma2, cv.phi, cv.tau2,
                                       values=values, want_bf=want_bf, want_r=want_r)
        return B, F, R, p

    # -- the served methods --------------------------------------------------------------------------------------
    def compute_BF(self, cov=None):
        """B (N, m) and F (N,) on the GPU at ``cov`` (default the instance's; then cached as ``B`` and ``F``)."""
        B, F, _, p = self._sweep(self._model(cov), want_bf=True)
        _raise_on_bad(p.cpu().numpy())
        if cov is None:
            self._B, self._F = B, F
        return B, F

    @property
    def B(self):
        return self.compute_BF()[0] if self._B is None else self._B

    @property
    def F(self):
        return self.compute_BF()[1] if self._F is None else self._F

    def gls(self, cov=None, values=None):
        """GLS of ``values`` (default y) on X under the NNGP precision at ``cov``: one sweep that writes B and F, then
        one ``nngp_whiten_gram`` on [y, X].  Returns a :class:`pynngp_amd.regression.GLSResult`."""
        X = self._design("linear")
        v = self._values(values)
        B, F, _, p = self._sweep(self._model(cov), want_bf=True)
        V = torch.cat([v[:, None], X], dim=1).contiguous()
        _, G = _lib.whiten_gram(self.nbr, B, F, V, 0)
        host = torch.cat([p, G.reshape(-1)]).cpu().numpy()  # one copy: the partials and the Gram matrix
        _raise_on_bad(host[:4])
        k = V.shape[1]
        res = regression.gls_from_gram(host[4:].reshape(k, k).copy(), float(host[0]), v.shape[0])
        res.objective = res.loglik
        return res

    def loglik(self, cov=None, mean=None, values=None) -> float:
        """The NNGP log-likelihood of ``values`` (default y) at ``cov``; ``mean`` None (zero) or "linear" (X beta
        profiled out by :meth:`gls`)."""
        if self._design(mean) is not None:
            return self.gls(cov, values).loglik
        _, _, _, p = self._sweep(self._model(cov), values=self._values(values))
        h = p.cpu().numpy()
        _raise_on_bad(h)
        return -0.5 * (self.nbr.shape[0] * LOG_2PI + h[0] + h[1])

    def profile_loglik(self, cov=None, values=None):
        """``(loglik, beta)`` with the linear mean X beta profiled out at ``cov``."""
        res = self.gls(cov, values)
        return res.loglik, res.beta

    def loglik_grad(self, cov=None, mean=None, values=None):
        """:meth:`loglik` and its gradient (2 r + 1,) in ``cov.theta``'s order from one ``nngp_bf_grad_svc`` sweep:
        ``(loglik, grad)``.  With ``mean="linear"`` the sweep runs at the GLS residual y - X beta: the gradient of the
        profile likelihood (beta maximises it, so its own derivative drops out), returned as
        ``(loglik, beta, grad)``."""
        cv = self._model(cov)
        v = self._values(values)
        beta = None
        if self._design(mean) is not None:
            beta = self.gls(cv, v).beta
            v = (v - self._x_dev @ torch.from_numpy(beta).to(self.device)).contiguous()
        p, g, _ = _lib.bf_grad_svc(self._t_dev, self._z_dev, self.nbr, 0, cv.kind, cv.sigma2, cv.phi, cv.tau2, v)
        h = torch.cat([p, g]).cpu().numpy()
        _raise_on_bad(h[:4])
        ll = -0.5 * (self.nbr.shape[0] * LOG_2PI + h[0] + h[1])
        return (ll, h[4:].copy()) if beta is None else (ll, beta, h[4:].copy())

    def fit(self, gradient: bool = True, mean="auto", start=None, maxiter: int = 500, tol: float = 1e-8) -> dict:
        """Maximum likelihood over the log-parameters of (sigma2_1..r, phi_1..r, tau2), the linear mean profiled out
        when the instance has an ``X`` (``mean="auto"``; None forces a zero mean).  ``gradient=True``: L-BFGS-B on the
        analytic gradient (one :meth:`loglik_grad` per evaluation); ``gradient=False``: Nelder-Mead on the sweep.
        Returns a dict with ``cov``, ``theta``, ``beta``, ``loglik``, ``n_evals``, ``converged``, ``message``; the
        instance's covariance becomes the estimate."""
        from scipy.optimize import minimize

        if mean == "auto":
            mean = "linear" if self._x_dev is not None else None
        self._design(mean)
        kind, r = self.cov.kind, self.r
        th0 = np.array((self.cov if start is None else self._model(start)).theta)
        x0 = np.log(np.maximum(th0, 1e-8))
        best = {"ll": -math.inf}
        count = [0]

        def keep(cv, ll, beta):
            if ll > best["ll"]:
                best.update(ll=ll, cov=cv, beta=beta)

        def value_and_grad(x):
            count[0] += 1
            try:
                cv = _from_log(kind, r, x)
                out = self.loglik_grad(cv, mean)
            except (NNGPNumericalError, ValueError, OverflowError):
                return 1e300, np.zeros_like(x)
            ll, g = out[0], out[-1]
            keep(cv, ll, out[1] if len(out) == 3 else None)
            return -ll, -g * np.array(cv.theta)

        def value(x):
            count[0] += 1
            try:
                cv = _from_log(kind, r, x)
                if mean is None:
                    ll, beta = self.loglik(cv), None
                else:
                    ll, beta = self.profile_loglik(cv)
            except (NNGPNumericalError, ValueError, OverflowError):
                return 1e300
            keep(cv, ll, beta)
            return -ll

        if gradient:
            res = minimize(value_and_grad, x0, jac=True, method="L-BFGS-B",
                           options={"maxiter": maxiter, "ftol": 1e-15, "gtol": tol})
        else:
            res = minimize(value, x0, method="Nelder-Mead",
                           options={"maxiter": 400 * len(x0), "xatol": 1e-6, "fatol": 1e-9, "adaptive": True})
        if "cov" not in best:
            raise NNGPNumericalError("fit: no parameter value the optimiser tried was positive definite")
        self.cov = best["cov"]
        self._B = self._F = None
        return {"cov": self.cov, "theta": self.cov.theta, "beta": best["beta"], "loglik": best["ll"],
                "n_evals": count[0], "converged": bool(res.success), "message": str(res.message)}

    def _queries(self, query):
        q = self.t if query is None else np.ascontiguousarray(query, dtype=np.float64)
        q = q[:, None] if q.ndim == 1 else q
        if q.ndim != 2 or q.shape[1] != self.t.shape[1]:
            raise ValueError(f"query must be (n_q, {self.t.shape[1]}), got {q.shape}")
        qd = torch.as_tensor(q).to(self.device)
        return qd, _lib.knn_query(self._t_dev, qd, self.m)

    def predict(self, query, Z_query, X_query=None, noise: bool = True, cov=None):
        """Kriging of y at ``query`` (n_q, dim) with covariates ``Z_query`` (n_q, r) from each point's m nearest data
        points: numpy ``(mean, var)``.  With an ``X`` on the instance, ``X_query`` (n_q, p) is required and the mean
        is x_q' beta + B_q (y - X beta)_N at the GLS beta (the variance is the conditional one at that beta).
        ``noise`` False predicts the noiseless surface."""
        cv = self._model(cov)
        qd, nbr = self._queries(query)
        zq = torch.as_tensor(np.ascontiguousarray(np.reshape(Z_query, (qd.shape[0], self.r)), dtype=np.float64)).to(
            self.device)
        v, shift = self._y_dev, 0.0
        if (self._x_dev is None) != (X_query is None):
            raise ValueError("X_query goes with the instance's X: give both or neither")
        if X_query is not None:
            beta = torch.from_numpy(self.gls(cv).beta).to(self.device)
            Xq = regression.design(self, X_query, qd.shape[0], "X_query")
            if Xq.shape[1] != self._x_dev.shape[1]:
                raise ValueError(f"X_query has {Xq.shape[1]} columns, X has {self._x_dev.shape[1]}")
            v, shift = (self._y_dev - self._x_dev @ beta).contiguous(), Xq @ beta
        _, F, R, p = _lib.bf_cross_svc(self._t_dev, self._z_dev, qd, zq, nbr, cv.kind, cv.sigma2, cv.phi, cv.tau2,
                                       ref_values=v, target_noise=noise, want_r=True)
        _raise_on_bad(p.cpu().numpy())
        return (shift - R).cpu().numpy(), F.cpu().numpy()

    def coef(self, query=None, cov=None):
        """The coefficient surfaces: numpy ``(mean (n_q, r), var (n_q, r))`` of w_k at ``query`` (default the data
        sites) given each point's m nearest data points.  One cross sweep per component with z_query = e_k and no
        target noise, because Cov(w_k(s0), y_j) = z_jk sigma2_k rho(phi_k d) is the model's covariance at that z; the
        variance is the kriging variance.  With an ``X`` the data are y - X beta at the GLS beta."""
        cv = self._model(cov)
        qd, nbr = self._queries(query)
        v = self._y_dev
        if self._x_dev is not None:
            v = (v - self._x_dev @ torch.from_numpy(self.gls(cv).beta).to(self.device)).contiguous()
        mean, var = np.empty((qd.shape[0], self.r)), np.empty((qd.shape[0], self.r))
        for k in range(self.r):
            zq = torch.zeros((qd.shape[0], self.r), dtype=torch.float64, device=self.device)
            zq[:, k] = 1.0
            _, F, R, p = _lib.bf_cross_svc(self._t_dev, self._z_dev, qd, zq, nbr, cv.kind, cv.sigma2, cv.phi, cv.tau2,
                                           ref_values=v, target_noise=False, want_r=True)
            _raise_on_bad(p.cpu().numpy())
            mean[:, k], var[:, k] = (-R).cpu().numpy(), F.cpu().numpy()
        return mean, var


def _refuser(name: str):
    def method(self, *args, **kw):
        _refuse(f"SVCNNGP.{name}")

    method.__name__ = name
    method.__doc__ = f"Not served by the varying-coefficient model: raises ``NotImplementedError`` ({SVC_SCOPE})."
    return method


for _name, _attr in list(vars(NNGP).items()):
    if callable(_attr) and not _name.startswith("_") and _name not in vars(SVCNNGP):
        setattr(SVCNNGP, _name, _refuser(_name))
del _name, _attr
