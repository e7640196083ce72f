"""Numpy restatement of the nonstationary sweeps (nngp_bf_sweep_ns / nngp_bf_cross_ns), shared by test_ns_host.py and
test_gpu_ns.py (not a conftest).

Per row the joint block is C(a, b) = sigma_a sigma_b x^(d/2) rho(u) off the diagonal and sigma2_a + tau2_a on it, with
x = 2 phi_a phi_b / (phi_a^2 + phi_b^2) and u^2 = 2 |s_a - s_b|^2 phi_a^2 phi_b^2 / (phi_a^2 + phi_b^2) (a: the point in
that slot, the location last); slots without a point (-1 or out of range) are decoupled identity rows with b = 0.  With
C_N = L L^T (fisher_ref's column-loop Cholesky, so the same code runs in ``np.longdouble``): b = C_N^-1 c,
F = C_ii - b.c, r = y_i - b.y_N.  ``rows`` returns an object with bf_precision_ref.Ref's fields (``check_sweep`` takes
it unchanged) plus ``ll`` per row; the error scales are bf_precision_ref's with sigma2 + tau2 replaced by the row's
largest diagonal entry.

Inputs: N uniform points in the unit cube, smooth fields sigma2 in [0.5, 2], phi in [3, 12], tau2 in [0.02, 0.2].
"""
import functools

import numpy as np

from bf_precision_ref import BF_K, U, Ref
from fisher_ref import bwd, chol, fwd, rho_drho
from oracle import nngp_oracle as O

LD = np.longdouble
N, N_QUERY = 200, 50
KINDS = ("exponential", "matern32", "matern52", "gaussian")
LOG_2PI = float(np.log(2.0 * np.pi))
# the lane-group widths (2, 4, 8, 16, 64 lanes) and their edges; every (dim, m) with the kinds dealt round
M_LIST = (1, 2, 7, 15, 16, 17, 24, 31, 32)
CASES = [(dim, KINDS[(k + dim) % 4], m) for k, m in enumerate(M_LIST) for dim in (1, 2, 3)]
CROSS_CASES = [(dim, KINDS[(k + dim) % 4], m) for k, m in enumerate((7, 16, 32)) for dim in (1, 2, 3)]


def fields_at(x):
    """The smooth test fields (sigma2, phi, tau2) at the points x (n, dim)."""
    s = x.mean(axis=1)
    return (0.5 + 1.5 * np.sin(1.3 * s + 0.2) ** 2, 3.0 + 9.0 * (0.5 + 0.5 * np.cos(2.1 * x[:, 0] + 0.4)),
            0.02 + 0.18 * np.clip(x[:, -1], 0.0, 1.0) ** 2)


def cov(pa, fa, pb, fb, kind, dtype=LD):
    """The cross-covariance (na, nb) between points pa with fields fa and pb with fb, without the nuggets."""
    pa, pb = np.asarray(pa, dtype=dtype), np.asarray(pb, dtype=dtype)
    (s2a, pha, _), (s2b, phb, _) = ([np.asarray(f, dtype=dtype) for f in fs] for fs in (fa, fb))
    d2 = ((pa[..., :, None, :] - pb[..., None, :, :]) ** 2).sum(axis=-1)
    den = pha[..., :, None] ** 2 + phb[..., None, :] ** 2
    x = 2 * pha[..., :, None] * phb[..., None, :] / den
    u = np.sqrt(2 * d2 * (pha[..., :, None] * phb[..., None, :]) ** 2 / den)
    amp = np.sqrt(s2a)[..., :, None] * np.sqrt(s2b)[..., None, :]
    return amp * x ** (dtype(pa.shape[-1]) / 2) * rho_drho(kind, u)[0]


def rows(ref, loc, nbr, kind, f_ref, f_loc, y_ref, y_loc, dtype=LD):
    """Rows ``loc`` (n, dim) with neighbours ``nbr`` (n, m) indexing ``ref``; f_* the (sigma2, phi, tau2) fields of
    the reference points and of the rows, y_loc (n,) the rows' values (None: 0)."""
    ref, loc = np.asarray(ref, dtype=dtype), np.asarray(loc, dtype=dtype)
    n, m = nbr.shape
    ok = (nbr >= 0) & (nbr < len(ref))
    j = np.where(ok, nbr, 0)
    pts = np.concatenate([ref[j], loc[:n, None, :]], axis=1)
    fl = [np.concatenate([np.asarray(a, dtype=dtype)[j], np.asarray(b, dtype=dtype)[:n, None]], axis=1)
          for a, b in zip(f_ref, f_loc)]
    valid = np.concatenate([ok, np.ones((n, 1), dtype=bool)], axis=1)
    eye = np.eye(m + 1, dtype=bool)[None]
    off = valid[:, :, None] & valid[:, None, :] & ~eye
    diag = np.where(valid, fl[0] + fl[2], dtype(1))
    C = np.where(off, cov(pts, fl, pts, fl, kind, dtype), dtype(0)) + diag[:, :, None] * eye.astype(dtype)
    yl = np.zeros(n, dtype) if y_loc is None else np.asarray(y_loc, dtype=dtype)[:n]
    yN = np.where(ok, np.asarray(y_ref, dtype=dtype)[j], dtype(0))
    CN, c = C[:, :m, :m], C[:, :m, m]
    with np.errstate(all="ignore"):
        L = chol(CN)
        b = np.where(ok, bwd(L, fwd(L, c[..., None]))[..., 0], dtype(0))
    out = Ref()
    out.b, out.pad = b, ~ok
    out.F = diag[:, m] - (b * c).sum(axis=1)
    out.r = yl - (b * yN).sum(axis=1)
    with np.errstate(all="ignore"):
        out.logF, out.q = np.log(out.F), out.r * out.r / out.F
    out.ll = -0.5 * (dtype(LOG_2PI) + out.logF + out.q)
    ev = np.linalg.eigvalsh(CN.astype(np.float64))
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
def field(dim):
    """(coords (N, dim), y, fields, query points (N_QUERY, dim), their fields)."""
    rng = np.random.default_rng(900 + dim)
    coords, y, q = rng.uniform(0.0, 1.0, (N, dim)), rng.standard_normal(N), rng.uniform(0.0, 1.0, (N_QUERY, dim))
    out = (coords, y, fields_at(coords), q, fields_at(q))
    for arr in (coords, y, q, *out[2], *out[4]):
        arr.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def neighbours(dim, m, cross=False):
    coords, _, _, q, _ = field(dim)
    nbr = O.knn_all(q, coords, m).astype(np.int32) if cross else O.c_knn_prior(coords, m)
    nbr.setflags(write=False)
    return nbr


@functools.lru_cache(maxsize=16)
def reference(dim, m, kind, cross=False):
    coords, y, f, q, fq = field(dim)
    if cross:
        return rows(coords, q, neighbours(dim, m, True), kind, f, fq, y, None)
    return rows(coords, coords, neighbours(dim, m), kind, f, f, y, y)
