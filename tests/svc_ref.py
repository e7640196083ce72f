"""Numpy restatement of the spatially-varying-coefficient sweeps (nngp_bf_sweep_svc / _cross_svc / _grad_svc), shared
by test_svc_host.py and test_gpu_svc.py (not a conftest).

Model: C(a, b) = sum_k z_ak z_bk sigma2_k rho(phi_k d_ab) + tau2 delta_ab; theta = (sigma2 (r,), phi (r,), tau2).  Per
row the joint block holds the neighbours and the location last; slots without a point (-1 or out of range) are
decoupled identity rows with b = 0.  With C_N = L L^T (fisher_ref's column-loop Cholesky, so the same code runs in
``np.longdouble``), b = C_N^-1 c, a = C_N^-1 y_N, u = [-b; 1], alpha = [a; 0]:

    F = C_ii - b.c,  r = y_i - b.y_N
    sigma2_k: D_ab = z_ak z_bk rho_k, the diagonal z_ak^2 included
    phi_k:    D_ab = z_ak z_bk sigma2_k d_ab rho_k'(phi_k d_ab)  (exactly 0 where d_ab = 0 and on the diagonal)
    tau2:     D = I
    dF = u^T D u, dr = -alpha^T D u,  G = -1/2 [(dF / F) (1 - r^2 / F) + 2 r dr / F]

``rows`` returns an object with bf_precision_ref.Ref's fields (so ``check_sweep`` takes it unchanged) plus ``G``
(n, 2 r + 1) and ``ll`` per row.  The error scales are bf_precision_ref's with (sigma2 + tau2) replaced by the joint
block's largest diagonal entry.

Inputs.  ``field(dim, r)``: n = 96 uniform points in the unit cube, Z a column of ones then standard normal columns,
standard normal values; tau2 = 0.1, sigma2 of order 1, distinct decays.  The decays started at (6, 3, 9, 4.5); there
the fp64 restatement's B reached 1.50 x U sB on the smooth kinds in one dimension at m = 31 (BF_K / 8 = 1.5), so the
ranges were shortened to (9, 5, 14, 7): 1.41 at worst (tests/test_svc_host.py).
"""
import functools

import numpy as np

from bf_precision_ref import BF_K, U, Ref
from fisher_ref import KINDS, bwd, chol, fwd, rho_drho  # noqa: F401
from oracle import nngp_oracle as O

LD = np.longdouble
N = 96
N_QUERY = 40
LOG_2PI = float(np.log(2.0 * np.pi))
M_ALL = tuple(range(1, 33))
M_EDGES = (8, 9, 15, 16, 23, 24, 31, 32)  # the lane-group edges
SIGMA2 = (1.3, 0.8, 1.1, 0.6)
PHI = (9.0, 5.0, 14.0, 7.0)
PHI_SPHERICAL = (1.7, 1.2, 2.1, 1.5)  # the ranges kept long, as sep_ref does
TAU2 = 0.1


def theta_of(kind, r):
    return (SIGMA2[:r], (PHI_SPHERICAL if kind == "spherical" else PHI)[:r], TAU2)


def rows(ref, zref, loc, zloc, nbr, kind, theta, y_ref, y_loc, target_noise=True, dtype=LD):
    """Rows ``loc`` (n, dim), covariates ``zloc`` (n, r), with neighbours ``nbr`` (n, m) indexing ``ref`` / ``zref``;
    y_loc (n,) belongs to the rows (None: 0)."""
    ref, loc = np.asarray(ref, dtype=dtype), np.asarray(loc, dtype=dtype)
    zref, zloc = np.asarray(zref, dtype=dtype), np.asarray(zloc, dtype=dtype)
    n, m = nbr.shape
    s2, ph, t2 = [dtype(x) for x in theta[0]], [dtype(x) for x in theta[1]], dtype(theta[2])
    nr = len(ph)
    ok = (nbr >= 0) & (nbr < len(ref))
    j = np.where(ok, nbr, 0)
    pts = np.concatenate([ref[j], loc[:n, None, :]], axis=1)
    zz = np.concatenate([np.where(ok[..., None], zref[j], dtype(0)), zloc[:n, None, :]], axis=1)
    valid = np.concatenate([ok, np.ones((n, 1), dtype=bool)], axis=1)
    d = np.sqrt(((pts[:, :, None, :] - pts[:, None, :, :]) ** 2).sum(axis=-1))
    eye = np.eye(m + 1, dtype=bool)[None]
    off = valid[:, :, None] & valid[:, None, :] & ~eye
    noise = np.full((n, m + 1), t2)
    if not target_noise:
        noise[:, m] = 0
    C = (noise * valid)[:, :, None] * eye + (~valid)[:, :, None] * eye.astype(dtype)
    D = []
    for k in range(nr):
        rho, drho = rho_drho(kind, ph[k] * d)
        w = zz[:, :, None, k] * zz[:, None, :, k]
        Ds = np.where(off | (eye & valid[:, :, None]), w * rho, dtype(0))
        C = C + s2[k] * Ds
        D.append((Ds, np.where(off & (d > 0), w * s2[k] * d * drho, dtype(0))))
    yl = np.zeros(n, dtype) if y_loc is None else np.asarray(y_loc, dtype=dtype)[:n]
    yN = np.where(ok, np.asarray(y_ref, dtype=dtype)[j], dtype(0))
    CN, c = C[:, :m, :m], C[:, :m, m]
    with np.errstate(all="ignore"):
        L = chol(CN)
        sol = bwd(L, fwd(L, np.stack([c, yN], axis=-1)))
    b, a = np.where(ok, sol[..., 0], dtype(0)), np.where(ok, sol[..., 1], dtype(0))
    out = Ref()
    out.b, out.pad = b, ~ok
    out.F = C[:, m, m] - (b * c).sum(axis=1)
    out.r = yl - (b * yN).sum(axis=1)
    with np.errstate(all="ignore"):
        out.logF, out.q = np.log(out.F), out.r * out.r / out.F
    out.ll = -0.5 * (dtype(LOG_2PI) + out.logF + out.q)
    u = np.concatenate([-b, np.ones((n, 1), dtype)], axis=1)
    al = np.concatenate([a, np.zeros((n, 1), dtype)], axis=1)
    mats = [Dk[0] for Dk in D] + [Dk[1] for Dk in D] + [np.broadcast_to(eye.astype(dtype), C.shape)]
    G = []
    with np.errstate(all="ignore"):
        for Dm in mats:
            Du = np.einsum("nab,nb->na", Dm, u)
            dF, dr = (u * Du).sum(axis=1), -(al * Du).sum(axis=1)
            G.append(-0.5 * ((dF / out.F) * (1 - out.q) + 2 * out.r * dr / out.F))
    out.G = np.stack(G, axis=1)
    # error scales (bf_precision_ref's, the largest diagonal entry of the joint block for sigma2 + tau2)
    ev = np.linalg.eigvalsh(CN.astype(np.float64)) if m else np.ones((n, 1))
    dmax = np.diagonal(C, axis1=1, axis2=2).max(axis=1).astype(np.float64)
    b1 = 1.0 + np.abs(b).sum(axis=1).astype(np.float64)
    with np.errstate(all="ignore"):
        out.lam_min = ev[:, 0]
        out.cond = np.where(ev[:, 0] > 0, ev[:, -1] / ev[:, 0], np.inf)
        out.sB = np.where(ev[:, 0] > 0, dmax * b1 / ev[:, 0], np.inf)
        out.sF = dmax * b1 * b1
        out.sR = out.sB * np.linalg.norm(yN.astype(np.float64), axis=1) + np.abs(out.r.astype(np.float64))
    out.resolved = BF_K * U * out.cond < 1.0
    return out


def dense_cov(a, za, b, zb, kind, theta, dtype=LD):
    """sum_k z_ak z_bk sigma2_k rho_k between the rows of a and b (no nugget)."""
    a, b, za, zb = (np.asarray(x, dtype=dtype) for x in (a, b, za, zb))
    d = np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))
    return sum(dtype(theta[0][k]) * np.outer(za[:, k], zb[:, k]) * rho_drho(kind, dtype(theta[1][k]) * d)[0]
               for k in range(len(theta[1])))


def dense_loglik(coords, Z, kind, theta, y, dtype=LD):
    """The dense N(0, C) log density of y (Cholesky in ``dtype``)."""
    n = len(y)
    K = dense_cov(coords, Z, coords, Z, kind, theta, dtype) + dtype(theta[2]) * np.eye(n, dtype=dtype)
    L = chol(K[None])[0]
    w = fwd(L[None], np.asarray(y, dtype=dtype)[None, :, None])[0, :, 0]
    return float(-0.5 * (n * dtype(LOG_2PI) + 2 * np.log(np.diag(L)).sum() + (w * w).sum()))


def conditional(coords, Z, y, idx, q, zq, kind, theta, noise):
    """Mean and variance of the target with covariates ``zq`` at ``q`` (1, dim) given y at the points ``idx``, dense,
    long double; ``noise`` adds tau2 to the target."""
    K = dense_cov(coords[idx], Z[idx], coords[idx], Z[idx], kind, theta) + LD(theta[2]) * np.eye(len(idx), dtype=LD)
    c = dense_cov(coords[idx], Z[idx], q, zq, kind, theta)[:, 0]
    L = chol(K[None])
    b = bwd(L, fwd(L, c[None, :, None]))[0, :, 0]
    var = dense_cov(q, zq, q, zq, kind, theta)[0, 0] + (LD(theta[2]) if noise else 0) - b @ c
    return float(b @ np.asarray(y, dtype=LD)[idx]), float(var)


# ---------------------------------------------------------------- the inputs both test files use (read-only)
@functools.lru_cache(maxsize=None)
def field(dim, r, n=N):
    """(coords, Z with a column of ones then standard normal columns, values)."""
    rng = np.random.default_rng(1700 + dim + 7 * n)
    coords = rng.uniform(0.0, 1.0, (n, dim))
    y = rng.standard_normal(n)
    Z = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, 3))], axis=1)[:, :r].copy()
    for a in (coords, y, Z):
        a.setflags(write=False)
    return coords, Z, y


@functools.lru_cache(maxsize=None)
def neighbours(dim, m, n=N):
    nbr = O.c_knn_prior(field(dim, 1, n)[0], m)
    nbr.setflags(write=False)
    return nbr


@functools.lru_cache(maxsize=None)
def query(dim, r):
    """(query points (N_QUERY, dim), their covariates, their values): the first 10 are copies of reference points
    with other covariates."""
    a = field(dim, r)[0]
    rng = np.random.default_rng(6100 + dim)
    q = rng.uniform(-0.05, 1.05, (N_QUERY, dim))
    q[:10] = a[rng.choice(N, 10, replace=False)]
    yq = rng.standard_normal(N_QUERY)
    zq = np.concatenate([np.ones((N_QUERY, 1)), rng.standard_normal((N_QUERY, 3))], axis=1)[:, :r].copy()
    for x in (q, yq, zq):
        x.setflags(write=False)
    return q, zq, yq


@functools.lru_cache(maxsize=None)
def query_neighbours(dim, m):
    nbr = O.knn_all(query(dim, 1)[0], field(dim, 1)[0], m).astype(np.int32)
    nbr.setflags(write=False)
    return nbr


@functools.lru_cache(maxsize=64)
def prior_reference(dim, m, kind, r, dtype=LD):
    coords, Z, y = field(dim, r)
    return rows(coords, Z, coords, Z, neighbours(dim, m), kind, theta_of(kind, r), y, y, dtype=dtype)


@functools.lru_cache(maxsize=64)
def cross_reference(dim, m, kind, r, dtype=LD):
    coords, Z, y = field(dim, r)
    q, zq, yq = query(dim, r)
    return rows(coords, Z, q, zq, query_neighbours(dim, m), kind, theta_of(kind, r), y, yq, dtype=dtype)
