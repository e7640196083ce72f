"""Numpy restatement of the Gneiting space-time sweeps (nngp_bf_sweep_gneiting / _cross_gneiting / _grad_gneiting), shared
by test_gneiting_host.py and test_gpu_gneiting.py (not a conftest).  C(a, b) = sigma2 rho(c h psi^(-beta/2)) / psi +
tau2 delta_ab, psi = 1 + (a u)^2, time in the last column; joint block, empty slots, F, r, G and the error scales are
sep_ref's, with per pair, dv = v rho'(v) and L = ln psi:  D_c = sigma2 dv / (psi c) (exactly 0 where h = 0),
D_a = -2 sigma2 (psi - 1) / (a psi^2) (rho + beta dv / 2),  D_beta = -sigma2 dv L / (2 psi) (both exactly 0 where u = 0).
``rows`` returns sep_ref.rows' object with G (n, 5) in (sigma2, c, a, beta, tau2); inputs are sep_ref's (a u <= 3)."""
import functools

import numpy as np

from bf_precision_ref import BF_K, U, Ref
from fisher_ref import bwd, chol, fwd, rho_drho
from sep_ref import LD, LOG_2PI, M_ALL, M_EDGES, N, field, neighbours, query, query_neighbours, scaled  # noqa: F401

KINDS = ("exponential", "matern32", "matern52", "gaussian")
BETAS = (0.0, 0.5, 1.0)
# the GPU cases (dim, kind, beta, m): every m, every kind x beta at the lane-group edges, dim 2
CASES = ([(3, "exponential", 0.5, m) for m in M_ALL] +
         [(3, k, b, m) for k in KINDS for b in BETAS for m in M_EDGES if (k, b) != ("exponential", 0.5)] +
         [(2, "exponential", 0.5, m) for m in (7, 15, 20, 32)])


def theta_of(beta):
    """(sigma2, c, a, beta, tau2)"""
    return (1.3, 6.0, 3.0, beta, 0.05)


def pair_terms(pts_a, pts_b, kind, theta, dtype):
    """(rho / psi, D_c, D_a, D_beta) at sigma2 = 1 between point arrays broadcast against each other."""
    _, c, a, beta, _ = (dtype(x) for x in theta)
    diff2 = (pts_a - pts_b) ** 2
    h = np.sqrt(diff2[..., :-1].sum(axis=-1))
    x = a * a * diff2[..., -1]
    psi = 1 + x
    L = np.log1p(x)
    with np.errstate(all="ignore"):
        v = c * h * np.exp(-beta / 2 * L)
        rho, drho = rho_drho(kind, v)
        dv = np.where(h > 0, v * drho, dtype(0))
    return rho / psi, dv / (psi * c), -2 * x / (a * psi * psi) * (rho + beta / 2 * dv), -dv * L / (2 * psi)


def rows(ref, loc, nbr, kind, theta, y_ref, y_loc, dtype=LD):
    ref, loc = np.asarray(ref, dtype=dtype), np.asarray(loc, dtype=dtype)
    n, m = nbr.shape
    s2, t2 = dtype(theta[0]), dtype(theta[4])
    ok = (nbr >= 0) & (nbr < len(ref))
    j = np.where(ok, nbr, 0)
    pts = np.concatenate([ref[j], loc[:n, None, :]], axis=1)
    valid = np.concatenate([ok, np.ones((n, 1), dtype=bool)], axis=1)
    eye = np.eye(m + 1, dtype=bool)[None]
    off = valid[:, :, None] & valid[:, None, :] & ~eye
    terms = pair_terms(pts[:, :, None, :], pts[:, None, :, :], kind, theta, dtype)
    diag = np.where(valid, s2 + t2, dtype(1))
    C = np.where(off, s2 * terms[0], dtype(0)) + diag[:, :, None] * eye.astype(dtype)
    D = [np.where(off, s2 * t, dtype(0)) for t in terms[1:]]
    yl = np.zeros(n, dtype) if y_loc is None else np.asarray(y_loc, dtype=dtype)[:n]
    yN = np.where(ok, np.asarray(y_ref, dtype=dtype)[j], dtype(0))
    CN, cc = C[:, :m, :m], C[:, :m, m]
    with np.errstate(all="ignore"):
        Lc = chol(CN)
        sol = bwd(Lc, fwd(Lc, np.stack([cc, yN], axis=-1)))
    b, al_ = np.where(ok, sol[..., 0], dtype(0)), np.where(ok, sol[..., 1], dtype(0))
    out = Ref()
    out.b, out.pad = b, ~ok
    out.F = diag[:, m] - (b * cc).sum(axis=1)
    out.r = yl - (b * yN).sum(axis=1)
    with np.errstate(all="ignore"):
        out.logF, out.q = np.log(out.F), out.r * out.r / out.F
    out.ll = -0.5 * (dtype(LOG_2PI) + out.logF + out.q)
    u = np.concatenate([-b, np.ones((n, 1), dtype)], axis=1)
    al = np.concatenate([al_, np.zeros((n, 1), dtype)], axis=1)
    dFt = 1 + (b * b).sum(axis=1)
    drt = (al_ * b).sum(axis=1)
    Du = [np.einsum("nab,nb->na", Dk, u) for Dk in D]
    dF = [(out.F - t2 * dFt) / s2] + [(u * d).sum(axis=1) for d in Du] + [dFt]
    dr = [-t2 * drt / s2] + [-(al * d).sum(axis=1) for d in Du] + [drt]
    with np.errstate(all="ignore"):
        out.G = np.stack([-0.5 * ((dF[k] / out.F) * (1 - out.q) + 2 * out.r * dr[k] / out.F) for k in range(5)], axis=1)
    ev = np.linalg.eigvalsh(CN.astype(np.float64)) if m else np.ones((n, 1))
    dmax = diag.max(axis=1).astype(np.float64)
    b1 = 1.0 + np.abs(b).sum(axis=1).astype(np.float64)
    with np.errstate(all="ignore"):
        out.lam_min = ev[:, 0]
        out.cond = np.where(ev[:, 0] > 0, ev[:, -1] / ev[:, 0], np.inf)
        out.sB = np.where(ev[:, 0] > 0, dmax * b1 / ev[:, 0], np.inf)
        out.sF = dmax * b1 * b1
        out.sR = out.sB * np.linalg.norm(yN.astype(np.float64), axis=1) + np.abs(out.r.astype(np.float64))
    out.resolved = BF_K * U * out.cond < 1.0
    return out


def cov_matrix(a, b, kind, theta):
    """sigma2 rho / psi between the rows of a and b (no nugget), fp64."""
    return theta[0] * pair_terms(a[:, None, :], b[None, :, :], kind, theta, np.float64)[0]


def dense_loglik(coords, kind, theta, y):
    n = len(y)
    K = cov_matrix(coords, coords, kind, theta) + theta[4] * np.eye(n)
    return -0.5 * (n * LOG_2PI + np.linalg.slogdet(K)[1] + y @ np.linalg.solve(K, y))


@functools.lru_cache(maxsize=64)
def prior_reference(dim, m, kind, beta):
    coords, y = field(dim)
    return rows(coords, coords, neighbours(dim, m), kind, theta_of(beta), y, y)


@functools.lru_cache(maxsize=64)
def cross_reference(dim, m, kind, beta):
    coords, y = field(dim)
    q, yq = query(dim)
    return rows(coords, q, query_neighbours(dim, m), kind, theta_of(beta), y, yq)
