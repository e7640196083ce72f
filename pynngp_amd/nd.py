"""Points in 4 .. 16 dimensions: :class:`ARDCovariance` and the :class:`NNGP` instance that serves it.

``NNGP(t, y, eps, "S=T", m, cov)`` with ``t`` of 4 .. 16 columns returns an :class:`NNGPnd`: a second, self-contained
path over C entry points of its own (``nngp_knn_prior_nd``, ``nngp_knn_query_nd``,
``nngp_bf_sweep_nd``, ``nngp_bf_cross_nd``, ``nngp_bf_grad_nd``).  The covariance is
``sigma2 rho(sqrt(sum_k (phi_k d_k)^2)) + tau2 delta`` with one decay per coordinate column (ARD; the "scaled
Vecchia" setting: the neighbour sets are searched in the metric of the decays).  It serves ``loglik``,
``compute_BF`` / ``B`` / ``F``, ``predict(query=)``, ``profile_loglik`` and ``profile_loglik_grad`` (constant or zero
mean), ``loglik_grad``, ``fit`` and ``rebuild_neighbors``; every other method of :class:`NNGP` raises
``NotImplementedError`` naming this scope.
"""
import dataclasses
import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from .nngp import LOG_2PI, NNGP, Covariance, NNGPNumericalError, _default_device, _raise_on_bad

ND_SCOPE = (f"an NNGP over {_lib.ND_MIN_DIM} .. {_lib.ND_MAX_DIM} coordinate columns serves refType='S=T', an "
            f"ARDCovariance or a Covariance of kind {', '.join(_lib.ND_KINDS)}, 1 <= m <= {_lib.GRAD_MAX_M}, "
            "ordering None, 'random' or a permutation, and the methods loglik, compute_BF, B, F, predict(query=), "
            "profile_loglik / profile_loglik_grad (mean 'constant' or 'zero'), loglik_grad, fit and rebuild_neighbors")


def _refuse_nd(what: str):
    raise NotImplementedError(f"{what} is not served: {ND_SCOPE}")


@dataclasses.dataclass(frozen=True)
class ARDCovariance:
    """One decay per input column, for 4 .. 16 columns: u = sqrt(sum_k (phi_k (a_k - b_k))^2) and
    C = sigma2 rho(u) + tau2 delta (automatic relevance determination; space, time and covariates as coordinates).
    Kinds ``exponential``, ``matern32``, ``matern52``, ``gaussian`` (the spherical correlation is not positive
    definite above three dimensions).  Up to three columns are :class:`AnisotropicCovariance`'s.  The gradient in
    (sigma2, phi_1 .. phi_dim, tau2) comes from ``nngp_bf_grad_nd``.  Called as ``cov(a, b)`` on coordinate rows it
    returns the cross-covariance matrix without the nugget."""

    kind: str
    sigma2: float
    phi: tuple
    tau2: float = 0.0

    def __post_init__(self):
        if self.kind == "spherical":
            raise ValueError("ARDCovariance does not serve the spherical kind: it is not positive definite above "
                             "three dimensions")
        if self.kind not in _lib.ND_KINDS:
            raise ValueError(f"ARDCovariance serves the kinds {_lib.ND_KINDS}, got {self.kind!r}")
        try:
            phi = tuple(float(p) for p in self.phi)
        except TypeError:
            raise ValueError("phi must be a sequence with one decay per coordinate column") from None
        if len(phi) < _lib.ND_MIN_DIM:
            raise ValueError(f"ARDCovariance takes {_lib.ND_MIN_DIM} .. {_lib.ND_MAX_DIM} decays, got {len(phi)}: up to "
                             f"{_lib.MAX_DIM} coordinate columns are served by AnisotropicCovariance")
        if len(phi) > _lib.ND_MAX_DIM:
            raise ValueError(f"ARDCovariance takes {_lib.ND_MIN_DIM} .. {_lib.ND_MAX_DIM} decays, got {len(phi)}")
        if not all(p > 0 and math.isfinite(p) for p in phi):
            raise ValueError(f"every phi_k must be positive and finite, got {phi}")
        if not (self.sigma2 > 0 and math.isfinite(self.sigma2) and self.tau2 >= 0 and math.isfinite(self.tau2)):
            raise ValueError("need sigma2 > 0, tau2 >= 0 (finite)")
        object.__setattr__(self, "phi", phi)

    nu = None
    nu_arg = None

    @property
    def dim(self) -> int:
        return len(self.phi)

    @property
    def theta(self):
        return (float(self.sigma2), *self.phi, float(self.tau2))

    def replace(self, **kw) -> "ARDCovariance":
        return dataclasses.replace(self, **kw)

    def __call__(self, a, b):
        lib = torch if isinstance(a, torch.Tensor) else np
        d = self.dim
        if (a.ndim > 1 and a.shape[-1] != d) or (b.ndim > 1 and b.shape[-1] != d):
            raise ValueError(f"coordinate rows must have {d} columns (len(phi))")
        s = torch.tensor(self.phi, dtype=a.dtype, device=a.device) if lib is torch else np.array(self.phi)
        return Covariance(self.kind, self.sigma2, 1.0, 0.0)(a.reshape(-1, d) * s, b.reshape(-1, d) * s)


def check_points_nd(a, what: str) -> np.ndarray:
    """``a`` as finite float64 (n, d) host points, ND_MIN_DIM <= d <= ND_MAX_DIM."""
    p = np.ascontiguousarray(a, dtype=np.float64)
    if p.ndim != 2 or not _lib.ND_MIN_DIM <= p.shape[1] <= _lib.ND_MAX_DIM:
        raise ValueError(f"{what} must be (N, d) with {_lib.ND_MIN_DIM} <= d <= {_lib.ND_MAX_DIM}, got {tuple(p.shape)}")
    if not np.all(np.isfinite(p)):
        raise ValueError(f"Input contains NaN or infinity ({what})")
    return p


def is_nd_points(t) -> bool:
    """Whether ``t`` is a 2-D array with more columns than the 1 .. 3-dimensional path takes."""
    shape = getattr(t, "shape", None)
    if shape is None:
        try:
            shape = np.shape(t)
        except Exception:
            return False
    return len(shape) == 2 and shape[1] > _lib.MAX_DIM


def ard_model(cov, dim: int, m: int) -> ARDCovariance:
    """``cov`` as the :class:`ARDCovariance` an n-dimensional instance runs: an isotropic :class:`Covariance` of the
    four kinds becomes all decays equal.  No GPU is touched."""
    if cov is None:
        _refuse_nd("a call without a covariance (the instance was built with cov=None)")
    if isinstance(cov, ARDCovariance):
        if cov.dim != dim:
            raise ValueError(f"ARDCovariance has {cov.dim} decays for {dim}-dimensional coordinates (len(phi) must "
                             "equal the number of coordinate columns)")
        out = cov
    elif type(cov) is Covariance:
        if cov.kind == "spherical":
            raise NotImplementedError("the spherical correlation is not positive definite above three dimensions; "
                                      + ND_SCOPE)
        if cov.kind not in _lib.ND_KINDS:
            _refuse_nd(f"the {cov.kind!r} kind")
        out = ARDCovariance(cov.kind, cov.sigma2, (cov.phi,) * dim, cov.tau2)
    else:
        _refuse_nd(f"a {type(cov).__name__}")
    if not 1 <= m <= _lib.GRAD_MAX_M:
        _refuse_nd(f"m={m}")
    return out


class NNGPnd(NNGP):
    """The :class:`NNGP` over 4 .. 16 coordinate columns (module docstring).  ``NNGP(...)`` returns one when ``t`` has
    that many columns."""

    def __init__(self, t, y, eps, refType, m, cov, device=None, ordering=None):
        if isinstance(refType, (tuple, list)) or refType != "S=T":
            _refuse_nd(f"refType={refType!r}")
        if isinstance(ordering, str) and ordering == "maxmin":
            raise NotImplementedError("ordering='maxmin' is a 1 .. 3-dimensional construction (the levelled order "
                                      "works on a grid of cells); " + ND_SCOPE)
        t_host = check_points_nd(t, "ordinates t")
        self.m = int(m)
        if not 0 <= self.m <= _lib.MAX_M:
            raise ValueError(f"m={m} outside [0, {_lib.MAX_M}]")
        if cov is not None:
            ard_model(cov, t_host.shape[1], self.m)
        elif not 1 <= self.m <= _lib.GRAD_MAX_M:
            _refuse_nd(f"m={m}")
        self.t, self.y, self.eps, self.refType, self.cov = t, y, eps, refType, cov
        self.device = _default_device(device)
        self.perm = None
        self._ordering = ordering
        n = t_host.shape[0]
        y_host = np.asarray(y)
        if y_host.shape[:1] != (n,):
            raise ValueError(f"y must have one row per ordinate ({n}), got {tuple(y_host.shape)}")
        if ordering is not None:
            from . import ordering as _ordering

            perm = _ordering.resolve(ordering, torch.as_tensor(t_host[:, :1]).to(self.device))
            self.perm = torch.as_tensor(perm).to(self.device)
            t_host = np.ascontiguousarray(t_host[perm])
            self.t, self.y = t_host, y_host[perm]
            if eps is not None and np.ndim(eps) >= 1 and np.shape(eps)[0] == n:
                self.eps = np.asarray(eps)[perm]
        self.s = self.t
        self._t_dev = self._s_dev = torch.as_tensor(t_host).to(self.device)
        self._order = None
        self.wt = np.copy(self.y)
        k = 5
        if n < k:
            raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, n_samples_fit = {n}")
        idx = _lib.knn_query_nd(self._t_dev, self._s_dev, k).long()
        yd = torch.as_tensor(np.asarray(self.y, dtype=np.float64)).to(self.device)
        self.ws = yd[idx].mean(dim=1).cpu().numpy()
        self._B = self._F = None
        self.rebuild_neighbors(cov)

    # -- the model -----------------------------------------------------------------
    def _model(self, cov) -> ARDCovariance:
        return ard_model(self.cov if cov is None else cov, self._s_dev.shape[1], self.m)

    def _scaled(self, cov, pts: torch.Tensor) -> torch.Tensor:
        """``pts`` in the metric of ``cov``'s decays (the coordinates themselves for cov None or equal decays)."""
        if cov is None:
            return pts
        phi = self._model(cov).phi
        if all(p == phi[0] for p in phi):
            return pts
        return (pts * torch.tensor(phi, dtype=torch.float64, device=pts.device)).contiguous()

    def rebuild_neighbors(self, cov=None):
        """The ordered prior neighbour sets in the metric of ``cov`` (default the instance's covariance; the plain
        coordinates without one): ``nngp_knn_prior_nd`` on the coordinates scaled by the decays."""
        cv = self.cov if cov is None else cov
        self._nbr_cov = cv
        self.nbr = self._nbr_sorted = _lib.knn_prior_nd(self._scaled(cv, self._s_dev), self.m)
        self._Ns = self._Nt = None
        self._B = self._F = None
        return self.nbr

    def clear_cache(self):
        self._B = self._F = None

    def _values_dev(self, values):
        v = self.y if values is None else values
        v = torch.as_tensor(np.asarray(v, dtype=np.float64) if not isinstance(v, torch.Tensor) else v,
                            dtype=torch.float64).to(self.device)
        if v.dim() != 1 or v.shape[0] != self.nbr.shape[0]:
            raise ValueError(f"one value per location is needed ({self.nbr.shape[0]}, 1-D)")
        return v.contiguous()

    def _sweep(self, cv: ARDCovariance, values=None, want_bf=False, want_r=False):
        return _lib.bf_sweep_nd(self._s_dev, self.nbr, 0, cv.kind, cv.sigma2, cv.phi, cv.tau2, values=values,
                                want_bf=want_bf, want_r=want_r)

    # -- the served methods --------------------------------------------------------
    def compute_BF(self, algo: str = "auto"):
        """B (n, m) and F (n,) at the instance's covariance (device tensors, cached)."""
        cv = self._model(None)
        B, F, _, p = self._sweep(cv, want_bf=True)
        _raise_on_bad(p.cpu().numpy())
        self._B, self._F = B, F
        return B, F

    @property
    def B(self):
        if self._B is None:
            self.compute_BF()
        return self._B

    @property
    def F(self):
        if self._F is None:
            self.compute_BF()
        return self._F

    def loglik(self, values=None, cov=None, algo: str = "auto", noise=None) -> float:
        """NNGP log-likelihood of ``values`` (default y) with mean zero at ``cov`` (one ``nngp_bf_sweep_nd``)."""
        if noise is not None:
            _refuse_nd("per-point noise (noise=)")
        cv = self._model(cov)
        _, _, _, p = self._sweep(cv, values=self._values_dev(values))
        h = p.cpu().numpy()
        _raise_on_bad(h)
        return -0.5 * (self.nbr.shape[0] * LOG_2PI + h[0] + h[1])

    def loglik_grad(self, values=None, cov=None, noise=None):
        """:meth:`loglik` and its gradient from one ``nngp_bf_grad_nd`` sweep: ``(loglik, grad)``.  An
        :class:`ARDCovariance` gives (sigma2, phi_1 .. phi_dim, tau2), (dim + 2,); an isotropic :class:`Covariance`
        (sigma2, phi, tau2) with the phi component the sum of the per-axis ones."""
        if noise is not None:
            _refuse_nd("per-point noise (noise=)")
        src = self.cov if cov is None else cov
        cv = self._model(cov)
        p, g, _ = _lib.bf_grad_nd(self._s_dev, self.nbr, 0, cv.kind, cv.sigma2, cv.phi, cv.tau2,
                                  self._values_dev(values))
        h = torch.cat([p, g]).cpu().numpy()
        _raise_on_bad(h[:4])
        grad = h[4:].copy()
        if not isinstance(src, ARDCovariance):
            grad = np.array([grad[0], grad[1:-1].sum(), grad[-1]])
        return -0.5 * (self.nbr.shape[0] * LOG_2PI + h[0] + h[1]), grad

    def profile_loglik(self, cov, values=None, mean: str = "constant", algo: str = "auto", X=None, noise=None):
        """As :meth:`NNGP.profile_loglik` for a constant or zero mean: ``(loglik, mu)``."""
        if noise is not None:
            _refuse_nd("per-point noise (noise=)")
        if mean == "linear" or X is not None:
            _refuse_nd("mean='linear' (gls)")
        if mean == "zero":
            return self.loglik(values, cov), 0.0
        if mean != "constant":
            raise ValueError("mean must be 'constant' or 'zero'")
        cv = self._model(cov)
        v = self._values_dev(values)
        _, F, ry, py = self._sweep(cv, values=v, want_bf=True, want_r=True)
        _, _, r1, p1 = self._sweep(cv, values=torch.ones_like(v), want_bf=True, want_r=True)
        sums = torch.stack([py[0], py[1], p1[1], torch.sum(ry * r1 / F), py[2], py[3]]).cpu().numpy()
        _raise_on_bad(np.array([0.0, 0.0, sums[4], sums[5]]))
        logF, qyy, q11, qy1 = sums[:4]
        mu = qy1 / q11
        return -0.5 * (v.shape[0] * LOG_2PI + logF + qyy - 2.0 * mu * qy1 + mu * mu * q11), float(mu)

    def profile_loglik_grad(self, cov, values=None, mean: str = "constant", X=None, noise=None):
        """:meth:`profile_loglik` and its gradient (the plain gradient at ``values - mu``): ``(loglik, mu, grad)``."""
        if noise is not None:
            _refuse_nd("per-point noise (noise=)")
        if mean == "linear" or X is not None:
            _refuse_nd("mean='linear' (gls)")
        v = self._values_dev(values)
        if mean == "zero":
            ll, g = self.loglik_grad(v, cov)
            return ll, 0.0, g
        ll, mu = self.profile_loglik(cov, v, mean=mean)
        return ll, mu, self.loglik_grad(v - mu, cov)[1]

    def predict(self, values=None, cov=None, query=None, algo: str = "auto", X=None, X_query=None, noise=None,
                noise_query=None):
        """Kriging at the points ``query`` (default ``t``) from ``values`` on S (default ``ws``): numpy ``(mean, var)``
        with var the conditional variance F (tau2 included).  Neighbours: the m nearest points of S to each query
        point in the metric of ``cov``'s decays (``nngp_knn_query_nd``), then one ``nngp_bf_cross_nd``."""
        if X is not None or X_query is not None:
            _refuse_nd("universal kriging (X, X_query)")
        if noise is not None or noise_query is not None:
            _refuse_nd("per-point noise (noise=)")
        cv = self._model(cov)
        v = self._values_dev(self.ws if values is None else values)
        q = self._s_dev if query is None else torch.as_tensor(check_points_nd(query, "query")).to(self.device)
        if q.shape[1] != self._s_dev.shape[1]:
            raise ValueError(f"query must have {self._s_dev.shape[1]} columns, got {q.shape[1]}")
        nbr = _lib.knn_query_nd(self._scaled(cv, self._s_dev), self._scaled(cv, q), self.m)
        _, F, R, p = _lib.bf_cross_nd(self._s_dev, q, nbr, cv.kind, cv.sigma2, cv.phi, cv.tau2, ref_values=v,
                                      want_r=True)
        _raise_on_bad(p.cpu().numpy())
        return (-R).cpu().numpy(), F.cpu().numpy()

    def fit(self, kind: Optional[str] = None, x0=None, mean: str = "constant", fix_tau2: Optional[float] = None,
            method: Optional[str] = None, maxiter: int = 200, reneighbor: int = 0, tol: Optional[float] = None,
            gradient: Optional[bool] = None, **other) -> dict:
        """Maximum likelihood over the free log-parameters of (sigma2, phi_1 .. phi_dim, tau2), the mean profiled
        out: L-BFGS-B on the analytic gradient (``nngp_bf_grad_nd``), or Nelder-Mead on the forward sweep with
        ``gradient=False``.  An isotropic :class:`Covariance` instance is fitted in (sigma2, phi, tau2).
        ``reneighbor`` rounds rebuild the neighbour sets in the metric of the current estimate, as the anisotropic
        fit does; ``tol`` bounds the projected gradient (in the log-parameters).  Returns a dict with ``theta``,
        ``sigma2``, ``phi``, ``tau2``, ``mu``, ``loglik``, ``grad``, ``n_evals``, ``n_grad_evals``, ``converged``,
        ``message``, ``rounds``; the instance's covariance becomes the estimate."""
        from scipy.optimize import minimize

        for k, val in other.items():
            if val not in (None, False, "auto"):
                _refuse_nd(f"fit({k}={val!r})")
        if mean not in ("constant", "zero"):
            _refuse_nd(f"fit(mean={mean!r})")
        if reneighbor < 0:
            raise ValueError("reneighbor must be >= 0")
        gradient = True if gradient is None else bool(gradient)
        base = self.cov
        if base is None:
            _refuse_nd("fit on an instance built with cov=None")
        self._model(base)
        iso = not isinstance(base, ARDCovariance)
        if kind is not None and kind != base.kind:
            base = base.replace(kind=kind)
            self._model(base)
        d = self._s_dev.shape[1]
        npar = 3 if iso else d + 2
        if x0 is not None and len(x0) != npar:
            raise ValueError(f"x0 must hold {npar} values (sigma2, phi{'' if iso else '_1 .. phi_dim'}, tau2)")
        th0 = [float(x) for x in (x0 if x0 is not None else base.theta[:3] if iso else base.theta)]
        free_tau = fix_tau2 is None
        nz = npar - (0 if free_tau else 1)
        th0[-1] = max(th0[-1], 1e-6) if free_tau else float(fix_tau2)

        def cov_of(z):
            tau2 = math.exp(z[-1]) if free_tau else float(fix_tau2)
            if iso:
                return Covariance(base.kind, math.exp(z[0]), math.exp(z[1]), tau2)
            return ARDCovariance(base.kind, math.exp(z[0]), tuple(math.exp(x) for x in z[1:1 + d]), tau2)

        if method is None:
            method = "L-BFGS-B" if gradient else "Nelder-Mead"
        options = {"maxiter": maxiter}
        if gradient and tol is not None:
            options.update(gtol=float(tol), **({"ftol": 1e-15} if method == "L-BFGS-B" else {}))
        if not gradient and method == "Nelder-Mead":
            options.update(xatol=1e-6 if tol is None else float(tol), fatol=1e-9)
        start = cov_of(np.log(np.array(th0[:nz])))
        n_evals = n_grad = 0
        for rnd in range(reneighbor + 1):
            if rnd > 0:
                self.rebuild_neighbors(start)
            best, seen, last_failed = {"ll": -math.inf}, {}, [False]

            def evaluate(z, want_grad):
                try:
                    cv = cov_of(z)
                    if want_grad:
                        return (cv,) + tuple(self.profile_loglik_grad(cv, mean=mean))
                    return (cv,) + tuple(self.profile_loglik(cv, mean=mean))
                except IndexError:  # a bad neighbour index is no property of theta
                    raise
                except (OverflowError, ValueError, NNGPNumericalError):
                    return None

            def obj_grad(z):
                out = evaluate(z, True)
                last_failed[0] = out is None
                if out is None:
                    return 1e300, np.zeros(len(z))
                cv, ll, mu, g = out
                th = cv.theta
                gz = np.array([th[k] * g[k] for k in range(len(z))])
                seen[tuple(z)] = gz
                if ll > best["ll"]:
                    best.update(ll=ll, mu=mu, cov=cv, grad=gz)
                return -ll, -gz

            def obj(z):
                out = evaluate(z, False)
                if out is None:
                    return 1e300
                cv, ll, mu = out
                if ll > best["ll"]:
                    best.update(ll=ll, mu=mu, cov=cv)
                return -ll

            z0 = np.log(np.array(start.theta[:nz]))
            if gradient:
                res = minimize(obj_grad, z0, jac=True, method=method, options=options)
            else:
                res = minimize(obj, z0, method=method, options=options)
            n_evals += int(res.nfev)
            n_grad += len(seen)
            if "cov" not in best:
                raise NNGPNumericalError("fit: no parameter value the optimiser tried was positive definite")
            start = best["cov"]
        self.cov = start
        self._B = self._F = None
        if reneighbor > 0:  # the sets in the estimate's own metric, the likelihood on them
            self.rebuild_neighbors(start)
            best["ll"], best["mu"] = self.profile_loglik(start, mean=mean)
        out = {"theta": start.theta, "sigma2": start.sigma2, "phi": start.phi, "tau2": start.tau2, "mu": best["mu"],
               "loglik": best["ll"], "n_evals": n_evals, "n_grad_evals": n_grad,
               "converged": bool(res.success) and not last_failed[0], "message": str(res.message),
               "rounds": reneighbor + 1}
        if gradient:
            out["grad"] = best["grad"]  # at the reported theta (the best point seen, the last round's)
        return out


_SERVED = {"compute_BF", "loglik", "loglik_grad", "profile_loglik", "profile_loglik_grad", "predict", "fit",
           "rebuild_neighbors", "clear_cache", "to_model_order", "to_input_order"}


def _refuser(name: str):
    def method(self, *args, **kw):
        _refuse_nd(f"NNGP.{name}")

    method.__name__ = name
    method.__doc__ = f"Not served over 4 .. 16 coordinate columns: raises ``NotImplementedError`` ({ND_SCOPE})."
    return method


for _name, _attr in list(vars(NNGP).items()):
    if callable(_attr) and not _name.startswith("_") and _name not in _SERVED and _name not in vars(NNGPnd):
        setattr(NNGPnd, _name, _refuser(_name))
del _name, _attr
