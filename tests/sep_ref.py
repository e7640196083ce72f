"""Numpy restatement of the separable space-time sweeps (nngp_bf_sweep_sep / _cross_sep / _grad_sep), shared by
test_sep_host.py and test_gpu_sep.py (not a conftest).

Model: C(a, b) = sigma2 rho_s(phi_s |a_s - b_s|) rho_t(phi_t |a_t - b_t|) + tau2 delta_ab; the last coordinate column
is time, the first dim - 1 are space.  Per row the joint block holds the neighbours and the location last; slots
without a point (-1 or out of range) are decoupled identity rows with b = 0.  With C_N = L L^T (fisher_ref's
column-loop Cholesky, so the same code runs in ``np.longdouble``), b = C_N^-1 c, a = C_N^-1 y_N, u = [-b; 1],
alpha = [a; 0] and dv(u) = u rho'(u) per factor:

    F = C_ii - b.c,  r = y_i - b.y_N
    tau2:    dF = 1 + |b|^2                              dr = a.b
    sigma2:  dF = (F - tau2 dF_tau2) / sigma2            dr = -tau2 dr_tau2 / sigma2
    phi_s:   D_ab = sigma2 dv_s(u_s) rho_t(u_t) / phi_s  (exactly 0 where d_s = 0), zero diagonal
    phi_t:   D_ab = sigma2 rho_s(u_s) dv_t(u_t) / phi_t  (exactly 0 where d_t = 0)
             dF = u^T D u, dr = -alpha^T D u
    G_k = -1/2 [(dF_k / F) (1 - r^2 / F) + 2 r dr_k / F],  k in (sigma2, phi_s, phi_t, tau2)

``rows`` returns an object with bf_precision_ref.Ref's fields (so ``check_sweep`` takes it unchanged) plus ``G`` (n, 4)
and ``ll`` = -1/2 (log 2 pi + log F + r^2 / F) per row.  The error scales are bf_precision_ref's (sigma2 + tau2 on the
diagonal).

Inputs.  ``field(dim)``: n = 96 uniform points in the unit cube (time in the last column), standard normal values;
theta from ``theta_of``.
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


def theta_of(kind_s, kind_t):
    """(sigma2, phi_s, phi_t, tau2): fisher_ref.theta_of's decays per factor (the spherical range kept long)."""
    return (1.3, 1.7 if kind_s == "spherical" else 6.0, 1.2 if kind_t == "spherical" else 3.0, 0.05)


def rows(ref, loc, nbr, kind_s, kind_t, theta, y_ref, y_loc, dtype=LD):
    """Rows ``loc`` (n, dim) with neighbours ``nbr`` (n, m) indexing ``ref``; y_loc (n,) belongs to the rows (None:
    0).  S = T rows i0 .. i0 + n: pass the slices of the field as loc, y_loc."""
    ref, loc = np.asarray(ref, dtype=dtype), np.asarray(loc, dtype=dtype)
    n, m = nbr.shape
    s2, ps, pt, t2 = (dtype(x) for x in theta)
    ok = (nbr >= 0) & (nbr < len(ref))
    j = np.where(ok, nbr, 0)
    pts = np.concatenate([ref[j], loc[:n, None, :]], axis=1)
    valid = np.concatenate([ok, np.ones((n, 1), dtype=bool)], axis=1)
    diff2 = (pts[:, :, None, :] - pts[:, None, :, :]) ** 2
    ds = np.sqrt(diff2[..., :-1].sum(axis=-1))
    dt = np.sqrt(diff2[..., -1])
    rs, drs = rho_drho(kind_s, ps * ds)
    rt, drt = rho_drho(kind_t, pt * dt)
    eye = np.eye(m + 1, dtype=bool)[None]
    off = valid[:, :, None] & valid[:, None, :] & ~eye
    diag = np.where(valid, s2 + t2, dtype(1))
    C = np.where(off, s2 * rs * rt, dtype(0)) + diag[:, :, None] * eye.astype(dtype)
    # dC/dphi_s = sigma2 (u_s rho_s') rho_t / phi_s = sigma2 d_s rho_s' rho_t; exactly 0 where d_s = 0
    Ds = np.where(off & (ds > 0), s2 * ds * drs * rt, dtype(0))
    Dt = np.where(off & (dt > 0), s2 * rs * dt * drt, dtype(0))
    yl = np.zeros(n, dtype) if y_loc is None else np.asarray(y_loc, dtype=dtype)[:n]
    yN = np.where(ok, np.asarray(y_ref, dtype=dtype)[j], dtype(0))
    CN, c = C[:, :m, :m], C[:, :m, m]
    with np.errstate(all="ignore"):
        L = chol(CN)
        sol = bwd(L, fwd(L, np.stack([c, yN], axis=-1)))
    b, a = np.where(ok, sol[..., 0], dtype(0)), np.where(ok, sol[..., 1], dtype(0))
    out = Ref()
    out.b, out.pad = b, ~ok
    out.F = diag[:, m] - (b * c).sum(axis=1)
    out.r = yl - (b * yN).sum(axis=1)
    with np.errstate(all="ignore"):
        out.logF, out.q = np.log(out.F), out.r * out.r / out.F
    out.ll = -0.5 * (dtype(LOG_2PI) + out.logF + out.q)
    u = np.concatenate([-b, np.ones((n, 1), dtype)], axis=1)
    al = np.concatenate([a, np.zeros((n, 1), dtype)], axis=1)
    dFt = 1 + (b * b).sum(axis=1)
    drt_ = (a * b).sum(axis=1)
    Dsu = np.einsum("nab,nb->na", Ds, u)
    Dtu = np.einsum("nab,nb->na", Dt, u)
    dF = [(out.F - t2 * dFt) / s2, (u * Dsu).sum(axis=1), (u * Dtu).sum(axis=1), dFt]
    dr = [-t2 * drt_ / s2, -(al * Dsu).sum(axis=1), -(al * Dtu).sum(axis=1), drt_]
    with np.errstate(all="ignore"):
        out.G = np.stack([-0.5 * ((dF[k] / out.F) * (1 - out.q) + 2 * out.r * dr[k] / out.F) for k in range(4)], axis=1)
    # error scales (bf_precision_ref's)
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


def cov_matrix(a, b, kind_s, kind_t, theta):
    """sigma2 rho_s rho_t between the rows of a and b (no nugget), fp64."""
    ds = np.sqrt(((a[:, None, :-1] - b[None, :, :-1]) ** 2).sum(-1))
    dt = np.abs(a[:, None, -1] - b[None, :, -1])
    return theta[0] * rho_drho(kind_s, theta[1] * ds)[0] * rho_drho(kind_t, theta[2] * dt)[0]


def dense_loglik(coords, kind_s, kind_t, theta, y):
    """The dense N(0, sigma2 R_s o R_t + tau2 I) log density of y, fp64."""
    n = len(y)
    K = cov_matrix(coords, coords, kind_s, kind_t, theta) + theta[3] * np.eye(n)
    return -0.5 * (n * LOG_2PI + np.linalg.slogdet(K)[1] + y @ np.linalg.solve(K, y))


def scaled(coords, theta):
    """The coordinates in the neighbour search's metric: (phi_s, .., phi_s, phi_t) column by column."""
    return coords * np.array([theta[1]] * (coords.shape[1] - 1) + [theta[2]])


# ---------------------------------------------------------------- the inputs both test files use (read-only)
@functools.lru_cache(maxsize=None)
def field(dim, n=N):
    rng = np.random.default_rng(900 + dim + 7 * n)
    coords = rng.uniform(0.0, 1.0, (n, dim))
    y = rng.standard_normal(n)
    coords.setflags(write=False)
    y.setflags(write=False)
    return coords, y


@functools.lru_cache(maxsize=None)
def neighbours(dim, m, n=N):
    nbr = O.c_knn_prior(field(dim, n)[0], m)
    nbr.setflags(write=False)
    return nbr


@functools.lru_cache(maxsize=None)
def query(dim):
    """(query points (N_QUERY, dim), their values): the first 10 are copies of reference points."""
    a = field(dim)[0]
    rng = np.random.default_rng(5900 + dim)
    q = rng.uniform(-0.05, 1.05, (N_QUERY, dim))
    q[:10] = a[rng.choice(N, 10, replace=False)]
    q.setflags(write=False)
    yq = rng.standard_normal(N_QUERY)
    yq.setflags(write=False)
    return q, yq


@functools.lru_cache(maxsize=None)
def query_neighbours(dim, m):
    nbr = O.knn_all(query(dim)[0], field(dim)[0], m).astype(np.int32)
    nbr.setflags(write=False)
    return nbr


@functools.lru_cache(maxsize=64)
def prior_reference(dim, m, kind_s, kind_t):
    coords, y = field(dim)
    return rows(coords, coords, neighbours(dim, m), kind_s, kind_t, theta_of(kind_s, kind_t), y, y)


@functools.lru_cache(maxsize=64)
def cross_reference(dim, m, kind_s, kind_t):
    coords, y = field(dim)
    q, yq = query(dim)
    return rows(coords, q, query_neighbours(dim, m), kind_s, kind_t, theta_of(kind_s, kind_t), y, yq)
