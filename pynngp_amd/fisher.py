"""Host side of the Fisher information sweep (``nngp_bf_fisher``): the 3 x 3 matrix of its six sums, the
log-parameter forms, the covariance of an estimate and the Fisher-scoring iteration of ``NNGP.fit(method="fisher")``.

Pure numpy: the iteration sees the model only through a callable, so it runs on any objective (the tests drive it
with a quadratic).

Fisher scoring (Guinness 2021) on z = log theta, one iteration:

1. ``(ll, g, I) = evaluate(z)``: the (profiled) log-likelihood, its gradient and the expected information in z;
2. ``step = solve(I, g)`` (:func:`scoring_step`, ridge rule below); the decrement is ``|g . step|``;
3. stop, converged, when the decrement is below ``tol``;
4. try z + step, z + step / 2, ... (at most ``max_halvings`` halvings) until the log-likelihood does not fall below
   the current one; an evaluation that fails numerically counts as a fall.  When no trial is accepted the
   iteration stops, not converged.

Ridge rule of :func:`scoring_step`: I is scaled to unit diagonal, S = D^-1/2 I D^-1/2 (a non-positive diagonal
entry is replaced by 1); when its smallest eigenvalue is below ``RIDGE_RCOND`` times its largest, the multiple of the
identity that lifts it to exactly that bound is added to S.  A well-conditioned I is solved as it is.
"""
from __future__ import annotations

import math
from typing import Callable, Optional, Sequence, Tuple

import numpy as np

TRIU = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # the sweep's order: ss, sp, st, pp, pt, tt
RIDGE_RCOND = 1e-10
DEFAULT_TOL = 1e-10
DEFAULT_MAXITER = 100
MAX_HALVINGS = 20


def info_matrix(info6) -> np.ndarray:
    """The symmetric (3, 3) matrix of the sweep's six sums (or (..., 3, 3) of (..., 6) rows)."""
    a = np.asarray(info6, dtype=np.float64)
    out = np.empty(a.shape[:-1] + (3, 3))
    for k, (i, j) in enumerate(TRIU):
        out[..., i, j] = out[..., j, i] = a[..., k]
    return out


def info_rows_scale(rows6, theta) -> np.ndarray:
    """(n, 6) rows of the information in theta -> in log theta: entry (j, k) times theta_j theta_k."""
    th = np.asarray(theta, dtype=np.float64)
    return np.asarray(rows6, dtype=np.float64) * np.array([th[i] * th[j] for i, j in TRIU])


def to_log(info, grad, theta) -> Tuple[np.ndarray, np.ndarray]:
    """diag(theta) I diag(theta) and theta * g: the information and gradient in log theta."""
    th = np.asarray(theta, dtype=np.float64)
    return np.asarray(info) * np.outer(th, th), np.asarray(grad) * th


def scoring_step(info_log: np.ndarray, grad_log: np.ndarray) -> Tuple[np.ndarray, float]:
    """``(step, ridge)``: the solution of I step = g under the module's ridge rule and the ridge that was added
    to the unit-diagonal form of I (0.0 for a well-conditioned I)."""
    I = np.asarray(info_log, dtype=np.float64)
    g = np.asarray(grad_log, dtype=np.float64)
    if not (np.all(np.isfinite(I)) and np.all(np.isfinite(g))):
        raise FloatingPointError("non-finite information or gradient")
    d = np.diag(I).copy()
    d[~(d > 0.0)] = 1.0
    s = 1.0 / np.sqrt(d)
    S = I * np.outer(s, s)
    S = 0.5 * (S + S.T)
    ev = np.linalg.eigvalsh(S)
    floor = RIDGE_RCOND * max(ev[-1], 1.0)
    ridge = float(max(0.0, floor - ev[0]))
    if ridge > 0.0:
        S = S + ridge * np.eye(len(g))
    return s * np.linalg.solve(S, s * g), ridge


def fisher_scoring(evaluate: Callable, z0: Sequence[float], loglik_only: Optional[Callable] = None,
                   tol: float = DEFAULT_TOL, maxiter: int = DEFAULT_MAXITER, max_halvings: int = MAX_HALVINGS) -> dict:
    """Maximise a log-likelihood by Fisher scoring from ``z0`` (the module docstring has the iteration).

    ``evaluate(z) -> (ll, grad, info)`` or None where the objective cannot be evaluated; ``loglik_only(z) -> ll`` or
    None, the cheaper call of the step-halving trials (default: ``evaluate``'s first entry).  Returns a dict with
    ``z``, ``loglik``, ``grad``, ``info`` at the last accepted point, ``n_iter`` (accepted steps), ``n_evals``
    (calls of ``evaluate``), ``n_loglik_evals``, ``decrement``, ``ridge`` (the largest added) and ``converged``."""
    z = np.array(z0, dtype=np.float64)
    cur = evaluate(z)
    n_evals, n_ll = 1, 0
    if cur is None:
        raise FloatingPointError("the objective cannot be evaluated at the starting point")
    ll, g, I = cur
    n_iter, ridge_max, dec, converged = 0, 0.0, math.inf, False
    while True:
        step, ridge = scoring_step(I, g)
        ridge_max = max(ridge_max, ridge)
        dec = abs(float(np.dot(g, step)))
        if dec < tol:
            converged = True
            break
        if n_iter >= maxiter:
            break
        accepted = None
        scale = 1.0
        for _ in range(max_halvings + 1):
            zt = z + scale * step
            if loglik_only is not None:
                lt = loglik_only(zt)
                n_ll += 1
            else:
                nxt = evaluate(zt)
                n_evals += 1
                lt = None if nxt is None else nxt[0]
            if lt is not None and math.isfinite(lt) and lt >= ll:
                accepted = zt
                break
            scale *= 0.5
        if accepted is None:
            break
        if loglik_only is not None:
            nxt = evaluate(accepted)
            n_evals += 1
            if nxt is None:
                break
        z = accepted
        ll, g, I = nxt
        n_iter += 1
    return {"z": z, "loglik": float(ll), "grad": np.asarray(g, dtype=np.float64), "info": np.asarray(I, dtype=np.float64),
            "n_iter": n_iter, "n_evals": n_evals, "n_loglik_evals": n_ll, "decrement": dec, "ridge": ridge_max,
            "converged": converged}


def theta_cov(info_theta_free: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``(cov_theta, se)`` of the free parameters from their block of the information in theta: the inverse of
    the log-parameter block carried back by the delta method, which is the inverse of the theta block itself; the
    inverse is taken on the unit-diagonal form.  ``se`` is its root diagonal."""
    I = np.asarray(info_theta_free, dtype=np.float64)
    s = 1.0 / np.sqrt(np.diag(I))
    cov = np.linalg.inv(I * np.outer(s, s)) * np.outer(s, s)
    cov = 0.5 * (cov + cov.T)
    return cov, np.sqrt(np.diag(cov))
