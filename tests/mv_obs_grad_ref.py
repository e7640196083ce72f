"""Dense fp64 restatement of the packed-row multivariate gradient sweep: per location the joint block K
over the *observed* rows (neighbours point-major, the target's last) from LMCCovariance.__call__,
S = alpha alpha^T - a a^T - Z^T Z on that block, scattered with zeros to the full (point, outcome) grid, and
d l_i = 1/2 tr(S dK) in the order of LMCCovariance.theta.  ``ob`` (N, q) bool: outcome a observed at point p.  Slots that
are -1 or out of range are left out."""
import numpy as np

from mv_grad_ref import DRHO
from pynngp_amd.nngp import Covariance


def row_logdens(cov, coords, nbr_row, i, Y, ob):
    """The log-density of location i's observed outcomes given its neighbours' observed ones, and the pieces."""
    js = nbr_row[(nbr_row >= 0) & (nbr_row < len(coords))]
    pts = np.concatenate([coords[js], coords[i:i + 1]])
    sel = np.concatenate([ob[js].ravel(), ob[i]])
    K = (cov(pts, pts) + np.kron(np.eye(len(pts)), np.diag(cov.tau2)))[np.ix_(sel, sel)]
    y = np.concatenate([Y[js].ravel(), Y[i]])[sel]
    nn, nt = int(ob[js].sum()), int(ob[i].sum())
    if nt == 0:
        return 0.0, None
    B = np.linalg.solve(K[:nn, :nn], K[:nn, nn:]).T if nn else np.zeros((nt, 0))
    F = K[nn:, nn:] - B @ K[:nn, nn:]
    r = y[nn:] - B @ y[:nn]
    ld, qd = np.linalg.slogdet(F)[1], r @ np.linalg.solve(F, r)
    return -0.5 * (ld + qd + nt * np.log(2 * np.pi)), (ld, qd, pts, sel, K, B, F, r, y, nn)


def row_grad(cov, coords, nbr_row, i, Y, ob):
    """(log det F_i, the quadratic form, the P gradient terms of the log-density) of location i."""
    q, A = cov.q, np.array(cov.A)
    pieces = row_logdens(cov, coords, nbr_row, i, Y, ob)[1]
    if pieces is None:
        return 0.0, 0.0, np.zeros(q * (q + 1) // 2 + 2 * q)
    ld, qd, pts, sel, K, B, F, r, y, nn = pieces
    nt = len(y) - nn
    LF = np.linalg.cholesky(F)
    a = np.concatenate([np.linalg.solve(K[:nn, :nn], y[:nn]) if nn else np.zeros(0), np.zeros(nt)])
    g = np.linalg.solve(F, r)
    alpha = a + np.concatenate([-B.T @ g, g])
    Z = np.linalg.solve(LF, np.hstack([-B, np.eye(nt)]))
    S = np.zeros((len(sel), len(sel)))
    S[np.ix_(sel, sel)] = np.outer(alpha, alpha) - np.outer(a, a) - Z.T @ Z
    S = S.reshape(len(pts), q, len(pts), q)
    d = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    gA, gphi = np.zeros((q, q)), np.zeros(q)
    for k in range(q):
        rho = Covariance(cov.kind, 1.0, cov.phi[k], 0.0)(pts, pts)
        drho = d * DRHO[cov.kind](cov.phi[k] * d)  # d rho(phi_k d) / d phi_k
        gA[:, k] = np.einsum("saSb,sS->ab", S, rho) @ A[:, k]
        gphi[k] = 0.5 * A[:, k] @ np.einsum("saSb,sS->ab", S, drho) @ A[:, k]
    gtau = 0.5 * np.einsum("sasa->a", S)
    return ld, qd, np.concatenate([gA[np.tril_indices(q)], gphi, gtau])


def reference(cov, coords, nbr, Y, ob):
    """Per row: log det F (rows,), the quadratic form (rows,), G (rows, P)."""
    out = [row_grad(cov, coords, nbr[i], i, Y, ob) for i in range(len(nbr))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])
