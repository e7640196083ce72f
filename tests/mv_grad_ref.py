"""Dense fp64 restatement of the multivariate gradient sweep: per location the joint block K from
LMCCovariance.__call__, S = alpha alpha^T - a a^T - Z^T Z, and d l_i = 1/2 tr(S dK) in the order of
LMCCovariance.theta (A's lower triangle row-major, phi, tau2).  Slots that are -1 or out of range are left out."""
import numpy as np

from pynngp_amd.nngp import Covariance


# rho'(u) of the four kinds (Covariance.__call__: e^-u, (1 + u) e^-u, (1 + u + u^2 / 3) e^-u, e^-u^2)
DRHO = {"exponential": lambda u: -np.exp(-u), "matern32": lambda u: -u * np.exp(-u),
        "matern52": lambda u: -(u / 3.0) * (1.0 + u) * np.exp(-u), "gaussian": lambda u: -2.0 * u * np.exp(-u * u)}


def row_logdens(cov, coords, nbr_row, i, Y):
    """The log-density of location i given its valid neighbours, and the pieces the gradient needs."""
    q = cov.q
    js = nbr_row[(nbr_row >= 0) & (nbr_row < len(coords))]
    pts = np.concatenate([coords[js], coords[i:i + 1]])
    K = cov(pts, pts) + np.kron(np.eye(len(pts)), np.diag(cov.tau2))
    nn = len(js) * q
    y = np.concatenate([Y[js].reshape(-1), Y[i]])
    B = np.linalg.solve(K[:nn, :nn], K[:nn, nn:]).T if nn else np.zeros((q, 0))
    F = K[nn:, nn:] - B @ K[:nn, nn:]
    r = y[nn:] - B @ y[:nn]
    ld, qd = np.linalg.slogdet(F)[1], r @ np.linalg.solve(F, r)
    return -0.5 * (ld + qd + q * np.log(2 * np.pi)), (ld, qd, pts, K, B, F, r, y, nn)


def row_grad(cov, coords, nbr_row, i, Y):
    """(log det F_i, the quadratic form, the P gradient terms of the log-density) of location i."""
    q, A = cov.q, np.array(cov.A)
    ld, qd, pts, K, B, F, r, y, nn = row_logdens(cov, coords, nbr_row, i, Y)[1]
    LF = np.linalg.cholesky(F)
    a = np.concatenate([np.linalg.solve(K[:nn, :nn], y[:nn]) if nn else np.zeros(0), np.zeros(q)])
    g = np.linalg.solve(F, r)
    alpha = a + np.concatenate([-B.T @ g, g])
    Z = np.linalg.solve(LF, np.hstack([-B, np.eye(q)]))
    S = (np.outer(alpha, alpha) - np.outer(a, a) - Z.T @ Z).reshape(len(pts), q, len(pts), q)
    d = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    gA, gphi = np.zeros((q, q)), np.zeros(q)
    for k in range(q):
        rho = Covariance(cov.kind, 1.0, cov.phi[k], 0.0)(pts, pts)
        drho = d * DRHO[cov.kind](cov.phi[k] * d)  # d rho(phi_k d) / d phi_k
        gA[:, k] = np.einsum("saSb,sS->ab", S, rho) @ A[:, k]
        gphi[k] = 0.5 * A[:, k] @ np.einsum("saSb,sS->ab", S, drho) @ A[:, k]
    gtau = 0.5 * np.einsum("sasa->a", S)
    return ld, qd, np.concatenate([gA[np.tril_indices(q)], gphi, gtau])


def reference(cov, coords, nbr, Y):
    """Per row: log det F (rows,), the quadratic form (rows,), G (rows, P)."""
    out = [row_grad(cov, coords, nbr[i], i, Y) for i in range(len(nbr))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])
