"""Numpy restatement of the per-point noise sweeps (nngp_bf_sweep_noise / _cross_noise / _grad_noise), shared by
test_het_host.py and test_gpu_het.py (not a conftest).

Model: y_i = mu + w(s_i) + e_i, e_i ~ N(0, tau2 v_i).  Per row the joint block is C = sigma2 rho(phi d) off the
diagonal and sigma2 + tau2 v_a on it (a: the point in that slot, the location last); slots without a point (-1 or
out of range) are decoupled identity rows with b = 0.  With C_N = L L^T (fisher_ref's column-loop Cholesky, so the
same code runs in ``np.longdouble``), b = C_N^-1 c, a = C_N^-1 y_N, u = [-b; 1], alpha = [a; 0]:

    F = C_ii - b.c,  r = y_i - b.y_N
    tau2:    dF = v_i + sum_j b_j^2 v_j                  dr = sum_j a_j b_j v_j
    sigma2:  dF = (F - tau2 dF_tau2) / sigma2            dr = -tau2 dr_tau2 / sigma2
    phi:     dF = u^T D u, D_ab = sigma2 d_ab rho'(phi d_ab) (zero diagonal)      dr = -alpha^T D u
    G_k = -1/2 [(dF_k / F) (1 - r^2 / F) + 2 r dr_k / F]

``rows`` returns an object with bf_precision_ref.Ref's fields (so ``check_sweep`` takes it unchanged) plus ``G`` (n, 3)
and ``ll`` = -1/2 (log 2 pi + log F + r^2 / F) per row.  The error scales are bf_precision_ref's with sigma2 + tau2
replaced by the row's largest diagonal entry.

Inputs.  ``case`` builds what both test files use: n = 600 uniform points, standard normal values, sigmas log-uniform on
[0.2, 5] (v = sigma^2 spans 625x), theta fisher_ref.theta_of(kind) (tau2 = 0.05).
"""
import functools

import numpy as np

from bf_precision_ref import BF_K, U, Ref
from fisher_ref import KINDS, bwd, chol, fwd, rho_drho, theta_of  # noqa: F401
from oracle import nngp_oracle as O

LD = np.longdouble
N = 600
N_QUERY = 100
DIMS = (1, 2, 3)
# the lane-group widths (2, 4, 8, 16, 64 lanes), the pair kernel's left-looking switch at 18 and the four-lane range
M_LIST = (1, 2, 3, 7, 8, 15, 16, 17, 18, 24, 25, 31, 32)
LOG_2PI = float(np.log(2.0 * np.pi))


def rows(ref, loc, nbr, kind, theta, y_ref, y_loc, v_ref, v_loc, dtype=LD):
    """Rows ``loc`` (n, dim) with neighbours ``nbr`` (n, m) indexing ``ref``; y_loc / v_loc (n,) belong to the rows
    (None: value 0 / weight 1).  S = T rows i0 .. i0 + n: pass the slices of the field as loc, y_loc, v_loc."""
    ref, loc = np.asarray(ref, dtype=dtype), np.asarray(loc, dtype=dtype)
    n, m = nbr.shape
    s2, phi, t2 = (dtype(x) for x in theta)
    ok = (nbr >= 0) & (nbr < len(ref))
    j = np.where(ok, nbr, 0)
    pts = np.concatenate([ref[j], loc[:n, None, :]], axis=1)
    valid = np.concatenate([ok, np.ones((n, 1), dtype=bool)], axis=1)
    d = np.sqrt(((pts[:, :, None, :] - pts[:, None, :, :]) ** 2).sum(axis=-1))
    r_, dr_ = rho_drho(kind, phi * d)
    eye = np.eye(m + 1, dtype=bool)[None]
    off = valid[:, :, None] & valid[:, None, :] & ~eye
    vl = np.ones(n, dtype) if v_loc is None else np.asarray(v_loc, dtype=dtype)[:n]
    vv = np.concatenate([np.where(ok, np.asarray(v_ref, dtype=dtype)[j], dtype(0)), vl[:, None]], axis=1)
    diag = np.where(valid, s2 + t2 * vv, dtype(1))
    C = np.where(off, s2 * r_, dtype(0)) + diag[:, :, None] * eye.astype(dtype)
    D = np.where(off, s2 * d * dr_, dtype(0))
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
    # the three gradient terms
    u = np.concatenate([-b, np.ones((n, 1), dtype)], axis=1)
    al = np.concatenate([a, np.zeros((n, 1), dtype)], axis=1)
    vN = vv[:, :m]
    dFt = vl + (b * b * vN).sum(axis=1)
    drt = (a * b * vN).sum(axis=1)
    Du = np.einsum("nab,nb->na", D, u)
    dF = [(out.F - t2 * dFt) / s2, (u * Du).sum(axis=1), dFt]
    dr = [-t2 * drt / s2, -(al * Du).sum(axis=1), drt]
    with np.errstate(all="ignore"):
        out.G = np.stack([-0.5 * ((dF[k] / out.F) * (1 - out.q) + 2 * out.r * dr[k] / out.F) for k in range(3)], axis=1)
    # error scales (bf_precision_ref's, the row's largest diagonal entry for sigma2 + tau2)
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


# ---------------------------------------------------------------- the inputs both test files use (read-only)
@functools.lru_cache(maxsize=None)
def field(dim, zeros=False):
    """(coords (N, dim), y, sigmas e, v = e^2); ``zeros``: every 7th weight is 0 (an exactly known value)."""
    rng = np.random.default_rng(700 + dim)
    coords = rng.uniform(0.0, 1.0, (N, dim))
    y = rng.standard_normal(N)
    e = np.exp(rng.uniform(np.log(0.2), np.log(5.0), N))
    if zeros:
        e[::7] = 0.0
    out = (coords, y, e, e * e)
    for arr in out:
        arr.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def neighbours(dim, m):
    nbr = O.c_knn_prior(field(dim)[0], m)
    nbr.setflags(write=False)
    return nbr


@functools.lru_cache(maxsize=None)
def query(dim):
    """(query points (N_QUERY, dim), their values, their weights): the first 30 are copies of reference points."""
    a = field(dim)[0]
    rng = np.random.default_rng(4700 + dim)
    q = rng.uniform(-0.05, 1.05, (N_QUERY, dim))
    q[:30] = a[rng.choice(N, 30, replace=False)]
    out = (q, rng.standard_normal(N_QUERY), np.exp(rng.uniform(np.log(0.2), np.log(5.0), N_QUERY)) ** 2)
    for arr in out:
        arr.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def query_neighbours(dim, m):
    nbr = O.knn_all(query(dim)[0], field(dim)[0], m).astype(np.int32)
    nbr.setflags(write=False)
    return nbr


@functools.lru_cache(maxsize=8)
def prior_reference(dim, m, kind, zeros=False):
    coords, y, _, v = field(dim, zeros)
    return rows(coords, coords, neighbours(dim, m), kind, theta_of(kind), y, y, v, v)


@functools.lru_cache(maxsize=8)
def cross_reference(dim, m, kind):
    coords, y, _, v = field(dim)
    q, yq, vq = query(dim)
    return rows(coords, q, query_neighbours(dim, m), kind, theta_of(kind), y, yq, v, vq)


def dense_loglik_grad(coords, kind, theta, y, v):
    """The dense N(0, sigma2 R + tau2 diag(v)) log density of y and its gradient in (sigma2, phi, tau2), fp64."""
    n = len(y)
    d = np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(-1))
    r_, dr_ = rho_drho(kind, theta[1] * d)
    K = theta[0] * r_ + theta[2] * np.diag(v)
    Ki = np.linalg.inv(K)
    al = Ki @ y
    D = theta[0] * d * dr_
    np.fill_diagonal(D, 0.0)
    ll = -0.5 * (n * LOG_2PI + np.linalg.slogdet(K)[1] + y @ al)
    g = np.array([0.5 * al @ dK @ al - 0.5 * np.trace(Ki @ dK) for dK in (r_, D, np.diag(v))])
    return ll, g
