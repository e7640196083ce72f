"""Response-model regression ``y = X beta + w + eps`` on the B/F sweep.

Everything here follows from one small matrix.  With Q = (I - B)^T F^-1 (I - B) the NNGP precision of the response
at ``cov`` and U = F^-1/2 (I - B) [y, X] the whitened columns, the Gram matrix

    G = U^T U = [[y'Qy, y'QX], [X'Qy, X'QX]]                       ((p + 1) x (p + 1), p + 1 <= 16)

comes from one sweep that writes B and F plus one ``nngp_whiten_gram`` (two gather passes and a fixed-order fold on
the GPU); the p x p algebra below runs on the host in fp64 by Cholesky.

* :func:`gls_from_gram`: GLS beta and its covariance, the profile and the restricted log-likelihood.
* :func:`nig_from_gram`: the conjugate NNGP of Finley et al. (spNNGP's ``spConjNNGP``): at a fixed (phi, alpha =
  tau2 / sigma2) and the unit-variance covariance, beta and sigma2 integrate out in closed form -- a Normal-inverse-
  gamma posterior and the log evidence ``log p(y | phi, alpha)``.
* :func:`gls`, :func:`universal_kriging`, :func:`conjugate`, :func:`conjugate_grid`: the GPU side for an
  :class:`pynngp_amd.NNGP` instance (its methods ``gls`` / ``predict(X=, X_query=)`` / ``conjugate`` /
  ``conjugate_grid`` call these).
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional

import numpy as np
import torch

from . import _lib

LOG_2PI = math.log(2.0 * math.pi)
EPS = float(np.finfo(np.float64).eps)


def _numerical_error(msg: str):
    from .nngp import NNGPNumericalError

    return NNGPNumericalError(msg)


@dataclasses.dataclass
class GLSResult:
    """GLS under the NNGP precision Q: ``beta`` (p,), ``cov_beta`` = (X'QX)^-1 (times nothing: sigma2 is inside Q),
    ``loglik`` = -1/2 [n log 2pi + sum log F + y'Qy - beta' X'QX beta], ``reml`` = the restricted likelihood (n - p in
    the 2 pi term and -1/2 log det X'QX added), ``gram`` the (p + 1, p + 1) matrix of [y, X], ``quad`` the residual
    quadratic form and ``sum_log_f`` = sum log F.  ``objective``: the one of ``loglik`` / ``reml`` the caller asked
    :func:`gls` to maximise (``reml=`` there)."""
    beta: np.ndarray
    cov_beta: np.ndarray
    loglik: float
    reml: float
    gram: np.ndarray
    quad: float
    sum_log_f: float
    n: int
    objective: Optional[float] = None


def _spd_factor(A: np.ndarray, what: str):
    """Cholesky of the symmetric A after scaling it to unit diagonal: ``(d, L)`` with A = D L L' D, D = diag(d).
    Raises NNGPNumericalError when A is not numerically positive definite (a rank-deficient design)."""
    p = A.shape[0]
    d = np.sqrt(np.diag(A))
    if not np.all(np.isfinite(A)) or not np.all(d > 0.0):
        raise _numerical_error(f"{what} is not positive definite (a zero, negative or non-finite diagonal)")
    C = A / np.outer(d, d)
    try:
        L = np.linalg.cholesky(C)
    except np.linalg.LinAlgError:
        raise _numerical_error(f"{what} is not positive definite: the design matrix is rank deficient") from None
    # the scaled matrix has unit diagonal, so a pivot^2 at rounding level means a column in the span of the others
    if np.min(np.diag(L)) ** 2 <= 64.0 * p * EPS:
        raise _numerical_error(f"{what} is numerically singular: the design matrix is rank deficient")
    return d, L


def _solve_lower(L, b):
    from scipy.linalg import solve_triangular

    return solve_triangular(L, b, lower=True)


def _solve_upper(U, b):
    from scipy.linalg import solve_triangular

    return solve_triangular(U, b, lower=False)


def _spd_inverse(d, L):
    Li = _solve_lower(L, np.eye(L.shape[0]))
    return (Li.T @ Li) / np.outer(d, d)


def gls_from_gram(gram, sum_log_f: float, n: int) -> GLSResult:
    """The GLS quantities from the Gram matrix of the whitened ``[y, X]`` (host, fp64)."""
    G = np.asarray(gram, dtype=np.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1] or G.shape[0] < 2:
        raise ValueError(f"gram must be (p + 1, p + 1) with p >= 1, got {G.shape}")
    p = G.shape[0] - 1
    yy, Xy, XX = G[0, 0], G[1:, 0], G[1:, 1:]
    if not np.isfinite(yy):
        raise _numerical_error("y'Qy is not finite")
    d, L = _spd_factor(XX, "X'QX")
    z = _solve_lower(L, Xy / d)            # beta' X'QX beta = |z|^2
    beta = _solve_upper(L.T, z) / d
    quad = float(yy - z @ z)
    logdet = 2.0 * float(np.sum(np.log(np.diag(L))) + np.sum(np.log(d)))
    ll = -0.5 * (n * LOG_2PI + sum_log_f + quad)
    reml = -0.5 * ((n - p) * LOG_2PI + sum_log_f + quad + logdet)
    return GLSResult(beta=beta, cov_beta=_spd_inverse(d, L), loglik=float(ll), reml=float(reml), gram=G, quad=quad,
                     sum_log_f=float(sum_log_f), n=int(n))


@dataclasses.dataclass
class NIGPosterior:
    """Normal-inverse-gamma posterior of (beta, sigma2): beta | sigma2, y ~ N(mu, sigma2 V), sigma2 | y ~ IG(a, b),
    and ``log_evidence`` = log p(y | phi, alpha) (with a flat prior on beta: up to the improper prior's constant)."""
    mu: np.ndarray
    V: np.ndarray
    a: float
    b: float
    log_evidence: float


def nig_from_gram(gram, sum_log_f: float, n: int, prior: Optional[dict] = None) -> NIGPosterior:
    """Conjugate update from the Gram matrix of the whitened ``[y, X]`` at the unit-variance covariance
    (sigma2 = 1, nugget alpha).  ``prior``: dict with ``a``, ``b`` (sigma2 ~ IG(a, b); default 2, 1) and optionally
    ``mu``, ``V`` (beta | sigma2 ~ N(mu, sigma2 V)); without them the prior is flat in beta."""
    G = np.asarray(gram, dtype=np.float64)
    p = G.shape[0] - 1
    prior = dict(prior or {})
    a0, b0 = float(prior.get("a", 2.0)), float(prior.get("b", 1.0))
    if not (a0 > 0.0 and b0 > 0.0):
        raise ValueError("the inverse-gamma prior needs a > 0 and b > 0")
    yy, Xy, XX = G[0, 0], G[1:, 0], G[1:, 1:]
    if ("mu" in prior) != ("V" in prior):
        raise ValueError("give both mu and V of the prior on beta, or neither (flat)")
    if "V" in prior:
        m0 = np.asarray(prior["mu"], dtype=np.float64).reshape(p)
        V0 = np.asarray(prior["V"], dtype=np.float64).reshape(p, p)
        d0, L0 = _spd_factor(V0, "the prior covariance V")
        P0 = _spd_inverse(d0, L0)
        prec, rhs = P0 + XX, P0 @ m0 + Xy
        prior_quad = float(m0 @ P0 @ m0)
        prior_logdet = 2.0 * float(np.sum(np.log(np.diag(L0))) + np.sum(np.log(d0)))
        n_eff = n
    else:
        prec, rhs, prior_quad, prior_logdet, n_eff = XX, Xy, 0.0, 0.0, n - p
    if n_eff <= 0:
        raise ValueError("a flat prior on beta needs n > p")
    d, L = _spd_factor(prec, "the posterior precision of beta")
    z = _solve_lower(L, rhs / d)
    mu = _solve_upper(L.T, z) / d
    logdet_prec = 2.0 * float(np.sum(np.log(np.diag(L))) + np.sum(np.log(d)))
    a1 = a0 + 0.5 * n_eff
    b1 = b0 + 0.5 * float(yy + prior_quad - z @ z)
    if not b1 > 0.0:
        raise _numerical_error("the posterior scale b is not positive")
    ev = (-0.5 * n_eff * LOG_2PI - 0.5 * sum_log_f - 0.5 * logdet_prec - 0.5 * prior_logdet + a0 * math.log(b0)
          - a1 * math.log(b1) + math.lgamma(a1) - math.lgamma(a0))
    return NIGPosterior(mu=mu, V=_spd_inverse(d, L), a=float(a1), b=float(b1), log_evidence=float(ev))


# -- the GPU side ---------------------------------------------------------------------------------------------------
def design(nngp, X, n: int, name: str = "X") -> torch.Tensor:
    """``X`` as a contiguous float64 (n, p) device tensor, 1 <= p <= WHITEN_MAX_COLS - 1.  A tensor that already is
    one passes through without a copy: callers that evaluate many thetas convert once."""
    X = torch.as_tensor(np.asarray(X, dtype=np.float64) if not isinstance(X, torch.Tensor) else X,
                        dtype=torch.float64).to(nngp.device)
    if X.dim() == 1:
        X = X[:, None]
    if X.dim() != 2 or X.shape[0] != n or not 1 <= X.shape[1] <= _lib.WHITEN_MAX_COLS - 1:
        raise ValueError(f"{name} must be ({n}, p) with 1 <= p <= {_lib.WHITEN_MAX_COLS - 1} (the caller adds the "
                         f"intercept column), got {tuple(X.shape)}")
    return X.contiguous()


def whitened_gram(nngp, cov, X: torch.Tensor, v: torch.Tensor, algo: str = "auto"):
    """One B/F-writing sweep at ``cov`` and one ``nngp_whiten_gram`` on ``[v, X]``: ``(sum log F, G (host), B, F)``."""
    from .nngp import _raise_on_bad, _sweep_any

    cv, sc = nngp._sweep_cov(cov)  # an AnisotropicCovariance: its isotropic form on the scaled coordinates
    if nngp.m < 1:
        raise ValueError("the regression needs m >= 1")
    B, F, p = _sweep_any(cv, sc, nngp._nbr_sorted, 0, algo=algo, order=nngp._order,
                         blocks=nngp._field_blocks(cv))
    V = torch.cat([v[:, None], X], dim=1).contiguous()
    _, G = _lib.whiten_gram(nngp._nbr_sorted, B, F, V, 0, order=nngp._order)
    host = torch.cat([p, G.reshape(-1)]).cpu().numpy()  # one copy: the partials and the Gram matrix
    _raise_on_bad(host[:4], cv)
    k = V.shape[1]
    return float(host[0]), host[4:].reshape(k, k).copy(), B, F


def gls(nngp, cov, X, values=None, reml: bool = False, algo: str = "auto") -> GLSResult:
    v = nngp._values_dev(values)
    Xd = design(nngp, X, v.shape[0])
    slf, G, _, _ = whitened_gram(nngp, cov, Xd, v, algo)
    res = gls_from_gram(G, slf, v.shape[0])
    res.objective = res.reml if reml else res.loglik
    return res


def _query(nngp, query):
    q = nngp._t_dev if query is None else torch.as_tensor(np.ascontiguousarray(query, dtype=np.float64)).to(
        nngp.device)
    if q.dim() == 1:
        q = q[:, None]
    return q.contiguous()


def cross_terms(nngp, cv, q: torch.Tensor, resid: torch.Tensor, X: torch.Tensor, Xq: torch.Tensor, algo: str = "auto"):
    """At the query points ``q``: ``(B_q resid_N, F_q, h_q)`` with h_q = x_q - B_q X_N from ``nngp_whiten_gram`` in
    cross mode with F = 1 (device tensors); the neighbours are the m nearest reference points."""
    from .nngp import _raise_on_bad, _sweep_any

    q = nngp._query_scale(cv, q)
    cv, sc = nngp._sweep_cov(cv)
    k = min(nngp.m, sc.shape[0])
    nbr = _lib.knn_query(sc, q, k)
    R = torch.empty(q.shape[0], dtype=torch.float64, device=nngp.device)
    Bq, Fq, p = _sweep_any(cv, sc, nbr, 0, values=resid, algo=algo, R=R, qcoords=q)
    _raise_on_bad(p.cpu().numpy())
    h, _ = _lib.whiten_gram(nbr, Bq, torch.ones_like(Fq), X, Vq=Xq, want_gram=False)
    return -R, Fq, h


def universal_kriging(nngp, cov, X, X_query, values=None, query=None, algo: str = "auto"):
    """Universal kriging at ``query``: mean x_q' beta + B_q (y - X beta)_N and variance F_q + h_q' cov_beta h_q, the
    second term the uncertainty of the GLS beta.  Returns numpy ``(mean, var, GLSResult)``."""
    from .nngp import AnisotropicCovariance

    cv = nngp.cov if cov is None else cov
    if not isinstance(cv, AnisotropicCovariance):
        cv = nngp._covariance(cov)
    v = nngp._values_dev(values)
    Xd = design(nngp, X, v.shape[0])
    q = _query(nngp, query)
    Xq = design(nngp, X_query, q.shape[0], "X_query")
    if Xq.shape[1] != Xd.shape[1]:
        raise ValueError(f"X_query has {Xq.shape[1]} columns, X has {Xd.shape[1]}")
    slf, G, _, _ = whitened_gram(nngp, cv, Xd, v, algo)
    res = gls_from_gram(G, slf, v.shape[0])
    beta = torch.from_numpy(res.beta).to(nngp.device)
    Vb = torch.from_numpy(res.cov_beta).to(nngp.device)
    kr, Fq, h = cross_terms(nngp, cv, q, v - Xd @ beta, Xd, Xq, algo)
    mean = Xq @ beta + kr
    var = Fq + ((h @ Vb) * h).sum(dim=1)
    return mean.cpu().numpy(), var.cpu().numpy(), res


class ConjugateNNGP:
    """The conjugate NNGP at fixed (phi, alpha): the :class:`NIGPosterior` fields ``mu``, ``V``, ``a``, ``b``,
    ``log_evidence`` and :meth:`predict`.  ``cov`` is the unit-variance covariance the factors were computed at."""

    def __init__(self, nngp, cov, X: torch.Tensor, v: torch.Tensor, post: NIGPosterior, gram: np.ndarray):
        self._nngp, self.cov, self._X, self._v = nngp, cov, X, v
        self.posterior, self.gram = post, gram
        self.mu, self.V, self.a, self.b, self.log_evidence = post.mu, post.V, post.a, post.b, post.log_evidence

    @property
    def sigma2_mean(self) -> float:
        """E[sigma2 | y] = b / (a - 1) (a > 1)."""
        return self.b / (self.a - 1.0)

    def predict(self, query, X_query, algo: str = "auto"):
        """The Student-t predictive of y at ``query``: numpy ``(location, scale, df)`` with location x_q' mu + B_q (y -
        X mu)_N, scale^2 = (b / a) (F_q + h_q' V h_q) (F_q includes the nugget alpha) and df = 2 a."""
        g = self._nngp
        q = _query(g, query)
        Xq = design(g, X_query, q.shape[0], "X_query")
        if Xq.shape[1] != self._X.shape[1]:
            raise ValueError(f"X_query has {Xq.shape[1]} columns, X has {self._X.shape[1]}")
        mu = torch.from_numpy(self.mu).to(g.device)
        V = torch.from_numpy(self.V).to(g.device)
        kr, Fq, h = cross_terms(g, self.cov, q, self._v - self._X @ mu, self._X, Xq, algo)
        loc = Xq @ mu + kr
        scale = torch.sqrt((self.b / self.a) * (Fq + ((h @ V) * h).sum(dim=1)))
        return loc.cpu().numpy(), scale.cpu().numpy(), 2.0 * self.a


def conjugate(nngp, kind: str, phi: float, alpha: float, X, prior: Optional[dict] = None, nu: Optional[float] = None,
              values=None, algo: str = "auto") -> ConjugateNNGP:
    from .nngp import Covariance

    cv = Covariance(kind, 1.0, float(phi), float(alpha), nu=nu)
    v = nngp._values_dev(values)
    Xd = design(nngp, X, v.shape[0])
    slf, G, _, _ = whitened_gram(nngp, cv, Xd, v, algo)
    return ConjugateNNGP(nngp, cv, Xd, v, nig_from_gram(G, slf, v.shape[0], prior), G)


def conjugate_grid(nngp, phis, alphas, kind: str, X, prior: Optional[dict] = None, nu: Optional[float] = None,
                   values=None, algo: str = "auto") -> dict:
    """The evidence surface ``log p(y | phi, alpha)`` over the grid: dict with ``log_evidence`` (len(phis),
    len(alphas); -inf where the factorisation failed), ``phi`` / ``alpha`` its argmax and ``best`` the
    :class:`ConjugateNNGP` there."""
    from .nngp import NNGPNumericalError

    phis, alphas = [float(x) for x in phis], [float(x) for x in alphas]
    if not phis or not alphas:
        raise ValueError("phis and alphas must be non-empty")
    surf = np.full((len(phis), len(alphas)), -np.inf)
    fits = {}
    for i, phi in enumerate(phis):
        for j, al in enumerate(alphas):
            try:
                c = conjugate(nngp, kind, phi, al, X, prior=prior, nu=nu, values=values, algo=algo)
            except NNGPNumericalError:
                continue
            surf[i, j] = c.log_evidence
            fits[i, j] = c
    if not fits:
        raise _numerical_error("no grid point could be factorised")
    i, j = (int(k) for k in np.unravel_index(int(np.argmax(surf)), surf.shape))
    return {"log_evidence": surf, "phi": phis[i], "alpha": alphas[j], "best": fits[i, j]}
