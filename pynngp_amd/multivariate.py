"""Several correlated outcomes at the same sites: :class:`LMCCovariance` and :class:`MultivariateNNGP`.

The model is the linear model of coregionalisation (spBayes' ``spMvLM``), q outcomes (2..4) all observed at every
location::

    Cov(y_a(s), y_b(s')) = sum_k A[a, k] A[b, k] rho(phi_k |s - s'|) + tau2_a delta_ab delta_ss'

with A lower-triangular.  The conditioning sets are the ordinary prior neighbour sets on the coordinates (the
components share one Euclidean metric), and the factors come from ``nngp_bf_sweep_mv`` / ``nngp_bf_cross_mv``: one
wavefront per location, the joint block of (m + 1) q <= 64 rows factorised on the fp64 matrix instruction
(DESIGN.md 4.3j).  The analytic gradient in the LMC parameters is one more fused sweep, ``nngp_bf_grad_mv`` (DESIGN.md
4.3k): :meth:`MultivariateNNGP.loglik_grad`, and ``fit(gradient=True)``; ``fit`` differences the sweep by default.

Outcomes missing at some sites (NaN in ``Y``; co-kriging, spBayes' ``spMisalignLM``) run on the packed-row sweep
``nngp_bf_sweep_mv_obs`` / ``nngp_bf_cross_mv_obs``: a location conditions on its neighbours'
*observed* outcomes only, at most 64 of them over m <= 63 neighbour sites; :meth:`MultivariateNNGP.impute` predicts the
missing entries, and the analytic gradient on such data is ``nngp_bf_grad_mv_obs``:
``loglik_grad(missing="packed")`` and ``fit(gradient=True)``.  A reference set other than the data, per-component kinds, per-point noise and the latent / Gibbs
forms are not built.
"""
import dataclasses
import math

import numpy as np
import torch

from . import _lib
from .nngp import LOG_2PI, Covariance, NNGPNumericalError, _default_device, _raise_on_bad


@dataclasses.dataclass(frozen=True)
class LMCCovariance:
    """``kind`` one of exponential, matern32, matern52, gaussian (every component the same); ``A`` (q, q)
    lower-triangular with a positive diagonal; ``phi`` (q,) > 0; ``tau2`` (q,) >= 0; 2 <= q <= 4.  Called as
    ``cov(a, b)`` on host coordinate rows it returns the dense (n_a q, n_b q) cross-covariance, point-major (a point's
    q outcomes adjacent), without the nugget."""

    kind: str
    A: tuple
    phi: tuple
    tau2: tuple

    def __post_init__(self):
        if self.kind not in _lib.KIND_CODES:
            raise ValueError(f"unknown covariance kind {self.kind!r}")
        if self.kind not in _lib.MV_KINDS:
            raise NotImplementedError(f"LMCCovariance serves the kinds {_lib.MV_KINDS}, not {self.kind!r}")
        A = np.array(self.A, dtype=np.float64)
        phi = tuple(float(p) for p in np.ravel(self.phi))
        tau2 = tuple(float(t) for t in np.ravel(self.tau2))
        q = len(phi)
        if not 2 <= q <= _lib.MV_MAX_Q:
            raise NotImplementedError(f"LMCCovariance serves 2 <= q <= {_lib.MV_MAX_Q} outcomes (q={q})")
        if A.shape != (q, q) or len(tau2) != q:
            raise ValueError(f"A must be ({q}, {q}) and tau2 ({q},) for {q} decays")
        if not np.all(np.isfinite(A)) or not np.all(np.diag(A) > 0):
            raise ValueError("A must be finite with a positive diagonal")
        if np.any(np.triu(A, 1) != 0):
            raise ValueError("A must be lower-triangular")
        if not all(p > 0 and math.isfinite(p) for p in phi):
            raise ValueError(f"every phi_k must be positive and finite, got {phi}")
        if not all(t >= 0 and math.isfinite(t) for t in tau2):
            raise ValueError(f"every tau2_a must be non-negative and finite, got {tau2}")
        object.__setattr__(self, "A", tuple(tuple(float(x) for x in row) for row in A))
        object.__setattr__(self, "phi", phi)
        object.__setattr__(self, "tau2", tau2)

    @property
    def q(self) -> int:
        return len(self.phi)

    @property
    def theta(self):
        """Flat: A's lower triangle row-major, phi, tau2."""
        return (*(self.A[a][b] for a in range(self.q) for b in range(a + 1)), *self.phi, *self.tau2)

    def replace(self, **kw) -> "LMCCovariance":
        return dataclasses.replace(self, **kw)

    def __call__(self, a, b):
        a, b = np.atleast_2d(np.asarray(a, dtype=np.float64)), np.atleast_2d(np.asarray(b, dtype=np.float64))
        A, q = np.array(self.A), self.q
        out = np.zeros((a.shape[0], q, b.shape[0], q))
        for k in range(q):
            rho = Covariance(self.kind, 1.0, self.phi[k], 0.0)(a, b)
            out += rho[:, None, :, None] * np.outer(A[:, k], A[:, k])[None, :, None, :]
        return out.reshape(a.shape[0] * q, b.shape[0] * q)


def _from_theta(kind: str, q: int, x) -> LMCCovariance:
    """The optimiser's vector (A: log diagonal, raw below it, row-major; log phi; log tau2) as a covariance."""
    A = np.zeros((q, q))
    k = 0
    for a in range(q):
        for b in range(a + 1):
            A[a, b] = math.exp(x[k]) if a == b else x[k]
            k += 1
    return LMCCovariance(kind, A, np.exp(x[k:k + q]), np.exp(x[k + q:k + 2 * q]))


def _to_theta(cov: LMCCovariance) -> np.ndarray:
    q = cov.q
    x = [math.log(cov.A[a][b]) if a == b else cov.A[a][b] for a in range(q) for b in range(a + 1)]
    return np.array(x + [math.log(p) for p in cov.phi] + [math.log(max(t, 1e-12)) for t in cov.tau2])


class MultivariateNNGP:
    """NNGP for ``Y`` (N, q) at the points ``t`` (N, 1..3) under an :class:`LMCCovariance`, ``(m + 1) q <= 64``.
    ``ordering`` None, "random", "maxmin" or a permutation, as for :class:`NNGP`; rows are held in that order
    (``perm`` maps positions to input rows).

    NaN in ``Y`` means "not observed" (``self.obs`` (N,) uint8 holds the masks, bit a for outcome a).  Such an
    instance serves ``m <= 63`` and at most 64 observed neighbour rows per location; ``loglik``, ``compute_BF``,
    ``predict``, ``fit()``, ``fit(gradient=True)``, ``loglik_grad(missing="packed")`` and :meth:`impute` work on it,
    ``simulate`` does not yet.  ``nbr``
    (N, m) int32, -1 padded, replaces the m nearest prior sites as the conditioning sets (indices in the instance's
    row order, every entry below its row), e.g. with sets chosen per outcome."""

    def __init__(self, t, Y, m, cov: LMCCovariance, ordering=None, device=None, nbr=None):
        if not isinstance(cov, LMCCovariance):
            raise TypeError("cov must be an LMCCovariance")
        t = np.ascontiguousarray(t, dtype=np.float64)
        t = t[:, None] if t.ndim == 1 else t
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if t.ndim != 2 or not 1 <= t.shape[1] <= _lib.MAX_DIM or Y.shape != (t.shape[0], cov.q):
            raise ValueError(f"t must be (N, 1..{_lib.MAX_DIM}) and Y (N, {cov.q}), got {t.shape} and {Y.shape}")
        if not (np.all(np.isfinite(t)) and not np.any(np.isinf(Y))):
            raise ValueError("Input contains NaN or infinity")
        self.m, self.cov, self.q = int(m), cov, cov.q
        self.misaligned = bool(np.isnan(Y).any())
        if self.misaligned and not 1 <= self.m <= _lib.MV_OBS_MAX_M:
            raise NotImplementedError(f"outcomes missing at some sites: 1 <= m <= {_lib.MV_OBS_MAX_M} (m={self.m})")
        _lib._mv_checks(cov.kind, 1 if self.misaligned else self.m, cov.A, cov.phi, cov.tau2)
        self.device = _default_device(device)
        self.perm = None
        if ordering is not None:
            from . import ordering as _ordering

            self.perm = _ordering.resolve(ordering, torch.as_tensor(t).to(self.device))
            t, Y = np.ascontiguousarray(t[self.perm]), np.ascontiguousarray(Y[self.perm])
        self.t, self.Y = t, Y
        self._mask = ~np.isnan(Y)
        self.obs = (self._mask << np.arange(self.q)).sum(axis=1).astype(np.uint8)
        self.n_obs = int(self._mask.sum())
        if nbr is not None:
            nbr = np.ascontiguousarray(nbr)
            if nbr.dtype != np.int32 or nbr.shape != (t.shape[0], self.m):
                raise ValueError(f"nbr must be int32 ({t.shape[0]}, {self.m}), got {nbr.dtype} {nbr.shape}")
            if np.any(nbr < -1) or np.any(nbr >= np.arange(t.shape[0])[:, None]):
                raise ValueError("nbr must hold prior indices: -1 <= nbr[i, s] < i")
        self._t_dev = torch.as_tensor(t).to(self.device)
        self._nbr = _lib.knn_prior(self._t_dev, self.m) if nbr is None else torch.as_tensor(nbr).to(self.device)
        self._B = self._LF = None
        if self.misaligned:
            self._obs_dev = torch.as_tensor(self.obs).to(self.device)
            self._rows_max = self._rows_bound(self._nbr, "location")

    def _rows_bound(self, nbr, what):
        """The largest number of observed neighbour rows over ``nbr``'s rows, refused above 64 before any launch."""
        rows = _lib.mv_obs_rows(nbr, self._obs_dev)
        worst = int(rows.argmax()) if rows.numel() else 0
        count = int(rows[worst]) if rows.numel() else 0
        if count > _lib.MV_MAX_ROWS:
            raise ValueError(f"{what} {worst} conditions on {count} observed neighbour rows; the packed-row sweep "
                             f"serves at most {_lib.MV_MAX_ROWS}: use a smaller m or pass nbr=")
        return max(count, 1)

    def _refuse_misaligned(self, what):
        if self.misaligned:
            raise NotImplementedError(f"{what} is not built for outcomes missing at some sites (NaN in Y): the "
                                      "packed-row sweeps serve loglik, loglik_grad(missing=\"packed\"), compute_BF, "
                                      "predict, impute and fit()")

    def _sweep(self, cov, cols, want_b=False, want_lf=False):
        """One sweep over every location with the value columns ``cols`` (N, q, c); raises on either flag."""
        cov = self.cov if cov is None else cov
        vals = torch.as_tensor(np.ascontiguousarray(cols)).to(self.device)
        if self.misaligned:
            B, LF, E, p = _lib.bf_sweep_mv_obs(self._t_dev, self._nbr, 0, cov.kind, cov.A, cov.phi, cov.tau2,
                                               self._obs_dev, self._rows_max, vals, want_b=want_b, want_lf=want_lf)
        else:
            B, LF, E, p = _lib.bf_sweep_mv(self._t_dev, self._nbr, 0, cov.kind, cov.A, cov.phi, cov.tau2, vals,
                                           want_b=want_b, want_lf=want_lf)
        ph = p.cpu().numpy()
        _raise_on_bad(ph, cov)
        return B, LF, E, ph

    def loglik(self, cov=None, mean=None):
        """The NNGP log-likelihood of Y.  ``mean`` None (zero), an array broadcastable to (N, q) in the instance's
        row order, or "constant": a per-outcome GLS mean from one sweep over Y and the q indicator columns, whitened
        together; then ``(loglik, mu)`` is returned."""
        n, q = self.Y.shape
        if isinstance(mean, str):
            if mean != "constant":
                raise ValueError(f"mean must be None, 'constant' or an array, got {mean!r}")
            cols = np.zeros((n, q, 1 + q))
            cols[:, :, 0] = self.Y
            cols[:, np.arange(q), 1 + np.arange(q)] = self._mask  # E is 0 in the rows that are not observed
            _, _, E, ph = self._sweep(cov, cols)
            E = E.reshape(n * q, 1 + q)
            G = (E.T @ E).cpu().numpy()  # [[y'y, y'X], [X'y, X'X]] in the whitened metric
            mu = np.linalg.solve(G[1:, 1:], G[1:, 0])
            quad = G[0, 0] - G[0, 1:] @ mu
            return -0.5 * (self.n_obs * LOG_2PI + ph[0] + quad), mu
        resid = self.Y if mean is None else self.Y - np.broadcast_to(np.asarray(mean, dtype=np.float64), (n, q))
        ph = self._sweep(cov, resid[:, :, None])[3]
        return -0.5 * (self.n_obs * LOG_2PI + ph[0] + ph[1])

    def loglik_grad(self, cov=None, mean=None, missing=None):
        """:meth:`loglik` and its gradient (P,) in ``cov.theta``'s order (A's lower triangle row-major, phi, tau2) from
        one ``nngp_bf_grad_mv`` sweep: ``(loglik, grad)``.  ``mean`` as in :meth:`loglik`; for "constant" the GLS mean
        comes from the whitening sweep and the gradient sweep runs on Y - mu: the gradient of the profile likelihood
        (mu maximises it, so its own derivative drops out), returned as ``(loglik, mu, grad)``.

        With NaN in ``Y`` pass ``missing="packed"``: the packed-row gradient sweep ``nngp_bf_grad_mv_obs`` over the
        observed entries.  Without the keyword such data is refused, as before that sweep existed."""
        if missing not in (None, "packed"):
            raise ValueError(f"missing must be None or 'packed', got {missing!r}")
        if self.misaligned and missing is None:
            raise NotImplementedError("loglik_grad on outcomes missing at some sites (NaN in Y) runs the packed-row "
                                      "gradient sweep on request: pass missing=\"packed\"")
        cov = self.cov if cov is None else cov
        n, q = self.Y.shape
        mu = None
        if isinstance(mean, str):
            mu = self.loglik(cov, mean)[1]
        resid = self.Y - (0.0 if mean is None else np.broadcast_to(np.asarray(mu if mu is not None else mean,
                                                                              dtype=np.float64), (n, q)))
        vals = torch.as_tensor(np.ascontiguousarray(resid[:, :, None])).to(self.device)
        if self.misaligned:
            p, g, _ = _lib.bf_grad_mv_obs(self._t_dev, self._nbr, 0, cov.kind, cov.A, cov.phi, cov.tau2, self._obs_dev,
                                          self._rows_max, vals)
        else:
            p, g, _ = _lib.bf_grad_mv(self._t_dev, self._nbr, 0, cov.kind, cov.A, cov.phi, cov.tau2, vals)
        ph = p.cpu().numpy()
        _raise_on_bad(ph, cov)
        ll, g = -0.5 * (self.n_obs * LOG_2PI + ph[0] + ph[1]), g.cpu().numpy()
        return (ll, g) if mu is None else (ll, mu, g)

    def compute_BF(self, cov=None):
        """B (N, q, m q) and LF (N, q, q) on the GPU (also the properties ``B`` and ``LF``)."""
        self._B, self._LF, _, _ = self._sweep(cov, self.Y[:, :, None], want_b=True, want_lf=True)
        return self._B, self._LF

    @property
    def B(self):
        if self._B is None:
            self.compute_BF()
        return self._B

    @property
    def LF(self):
        if self._LF is None:
            self.compute_BF()
        return self._LF

    def predict(self, query, noise=True, cov=None, mean=None):
        """Conditional mean (n_q, q) and covariance (n_q, q, q) at ``query`` given each point's m nearest data
        points; ``noise`` False predicts the noiseless field.  ``mean`` (q,) is subtracted from Y and added back."""
        cov = self.cov if cov is None else cov
        query = np.ascontiguousarray(query, dtype=np.float64)
        query = query[:, None] if query.ndim == 1 else query
        qd = torch.as_tensor(query).to(self.device)
        mu = np.zeros(self.q) if mean is None else np.asarray(mean, dtype=np.float64)
        vals = torch.as_tensor(np.ascontiguousarray((self.Y - mu)[:, :, None])).to(self.device)
        nbr = _lib.knn_query(self._t_dev, qd, self.m)
        if self.misaligned:
            _, LF, pm, p = _lib.bf_cross_mv_obs(self._t_dev, qd, nbr, cov.kind, cov.A, cov.phi, cov.tau2,
                                                self._obs_dev, self._rows_bound(nbr, "query"), vals,
                                                target_noise=noise)
        else:
            _, LF, pm, p = _lib.bf_cross_mv(self._t_dev, qd, nbr, cov.kind, cov.A, cov.phi, cov.tau2, vals,
                                            target_noise=noise)
        _raise_on_bad(p.cpu().numpy(), cov)
        return pm[:, :, 0].cpu().numpy() + mu, (LF @ LF.transpose(1, 2)).cpu().numpy()

    def impute(self, noise=True, cov=None, mean=None):
        """The entries of ``Y`` that are not observed, predicted at their own site from its m nearest data sites'
        observed outcomes; the site itself is among them, so what is observed there enters at distance 0 (co-located
        co-kriging).  Returns ``(mean (N, q), sd (N, q))`` in the instance's row order: observed entries as they are
        with sd 0.  ``noise``, ``cov`` and ``mean`` as in :meth:`predict`."""
        out, sd = self.Y.copy(), np.zeros_like(self.Y)
        rows = np.nonzero(~self._mask.all(axis=1))[0]
        if rows.size:
            pm, pc = self.predict(self.t[rows], noise=noise, cov=cov, mean=mean)
            miss = ~self._mask[rows]
            out[rows] = np.where(miss, pm, out[rows])
            sd[rows] = np.where(miss, np.sqrt(np.diagonal(pc, axis1=1, axis2=2)), 0.0)
        return out, sd

    def fit(self, start=None, tol=1e-6, maxiter=200, step=1e-5, gradient=False):
        """Maximum likelihood (zero mean) by L-BFGS-B on log diag A, raw off-diagonal A, log phi, log tau2, with
        central differences of the sweep (2 (q (q + 1) / 2 + 2 q) sweeps per gradient), or with ``gradient=True`` on
        the analytic gradient: one :meth:`loglik_grad` sweep per evaluation gives the value and the gradient (the
        packed-row sweep when ``Y`` has NaN).  Sets and
        returns ``self.cov``; ``self.fit_result`` keeps scipy's result and ``self.fit_sweeps`` the number of sweep
        launches."""
        from scipy import optimize

        kind, q = self.cov.kind, self.q
        self.fit_sweeps = 0

        def value_and_grad(x):
            self.fit_sweeps += 1
            try:
                cov = _from_theta(kind, q, x)
                ll, g = self.loglik_grad(cov, missing="packed" if self.misaligned else None)
            except (NNGPNumericalError, ValueError, OverflowError):
                return 1e300, np.zeros_like(x)
            # the optimiser's vector: x A_aa for log diag A, x phi_k, x tau2_a
            scale = [cov.A[a][a] if a == b else 1.0 for a in range(q) for b in range(a + 1)]
            return -ll, -g * np.array(scale + list(cov.phi) + list(cov.tau2))

        if gradient:
            x0 = _to_theta(self.cov if start is None else start)
            self.fit_result = optimize.minimize(value_and_grad, x0, jac=True, method="L-BFGS-B",
                                                options={"maxiter": maxiter, "ftol": tol, "gtol": tol})
            self.cov = _from_theta(kind, q, self.fit_result.x)
            self._B = self._LF = None
            return self.cov

        def nll(x):
            self.fit_sweeps += 1
            try:
                return -self.loglik(_from_theta(kind, q, x))
            except (NNGPNumericalError, ValueError, OverflowError):
                return 1e300

        def grad(x):
            g = np.empty_like(x)
            for k in range(x.size):
                e = np.zeros_like(x)
                e[k] = step
                g[k] = (nll(x + e) - nll(x - e)) / (2.0 * step)
            return g

        x0 = _to_theta(self.cov if start is None else start)
        self.fit_result = optimize.minimize(nll, x0, jac=grad, method="L-BFGS-B",
                                            options={"maxiter": maxiter, "ftol": tol, "gtol": tol})
        self.cov = _from_theta(kind, q, self.fit_result.x)
        self._B = self._LF = None
        return self.cov

    def simulate(self, seed=0, cov=None):
        """A sequential draw (N, q) from the NNGP prior of ``cov``, from B and LF on the host."""
        self._refuse_misaligned("simulate")
        B, LF, _, _ = self._sweep(cov, self.Y[:, :, None], want_b=True, want_lf=True)
        B, LF, nbr = B.cpu().numpy(), LF.cpu().numpy(), self._nbr.cpu().numpy()
        z = np.random.default_rng(seed).standard_normal(self.Y.shape)
        out = np.zeros_like(self.Y)
        for i in range(out.shape[0]):
            yn = np.where(nbr[i, :, None] >= 0, out[np.maximum(nbr[i], 0)], 0.0).reshape(-1)
            out[i] = B[i] @ yn + LF[i] @ z[i]
        return out
