"""numpy restatement of the general-nu Matern gradient sweep (nngp_bf_grad_matern): tests/test_gpu_grad.py::ref_rows'
scalar-loop structure with two derivative blocks, D_phi = sigma2 h(u) / phi and D_nu = sigma2 n(u).  Shared by
test_grad_matern_host.py (which pins it) and test_gpu_grad_matern.py (which compares the GPU with it).

rho(u) and h(u) = u rho'(u) = -2^(1-nu)/Gamma(nu) u^(nu+1) K_{nu-1}(u) come from scipy.special.kv.
n(u) = d rho / d nu comes from mpmath (``mp.diff`` at 30 digits), cached per (nu, u): ``dnu_mp``.  A block of
many distinct distances (the GPU parity tests: tens of thousands per case) takes ``dnu_quad`` instead, the
integral K_nu(u) = int e^(-u cosh s) cosh(nu s) ds differentiated under the integral sign, by the trapezoid
rule in numpy longdouble with step 1/16; test_grad_matern_host.py pins dnu_quad to dnu_mp."""
import mpmath as mp
import numpy as np
from scipy import special

from test_gpu_grad import chol_solve

_DNU_CACHE = {}


def rho_mp(nu, u):
    return mp.mpf(2) ** (1 - nu) / mp.gamma(nu) * u ** nu * mp.besselk(nu, u)


def h_mp(nu, u):
    nu, u = mp.mpf(nu), mp.mpf(u)
    return -mp.mpf(2) ** (1 - nu) / mp.gamma(nu) * u ** (nu + 1) * mp.besselk(nu - 1, u)


def dnu_mp(nu, u, dps=30):
    """d rho_nu(u) / d nu by mpmath, cached."""
    key = (float(nu), float(u), dps)
    if key not in _DNU_CACHE:
        with mp.workdps(dps):
            _DNU_CACHE[key] = float(mp.diff(lambda v: rho_mp(v, mp.mpf(float(u))), mp.mpf(float(nu)))) if u > 0 else 0.0
    return _DNU_CACHE[key]


def rho_h(nu, u):
    """rho(u) and h(u) elementwise from scipy's K_nu (u >= 0; the limits 1 and 0 at u = 0 and past underflow)."""
    u = np.asarray(u, dtype=np.float64)
    us = np.where(u > 0, u, 1.0)
    lc = (1.0 - nu) * np.log(2.0) - special.gammaln(nu)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        k0, k1 = special.kv(nu, us), special.kv(nu - 1.0, us)
        r = np.exp(lc + nu * np.log(us) + np.log(k0))
        h = -np.exp(lc + (nu + 1.0) * np.log(us) + np.log(k1))
    ok0, ok1 = (u > 0) & np.isfinite(k0) & (k0 > 0), (u > 0) & np.isfinite(k1) & (k1 > 0)
    return np.where(ok0, r, np.where(u > 0, 0.0, 1.0)), np.where(ok1, h, 0.0)


def dnu_quad(nu, u):
    """n(u) elementwise (any shape) by the longdouble trapezoid rule, step 1/16."""
    L = np.longdouble
    u = np.asarray(u, dtype=np.float64)
    out = np.zeros(u.shape, dtype=np.float64)
    flat, res = u.reshape(-1), out.reshape(-1)
    pos = np.nonzero(flat > 0)[0]
    if pos.size == 0:
        return out
    uu = flat[pos].astype(L)[:, None]
    nul = L(nu)
    with mp.workdps(40):
        kk = L(str(mp.log(2) + mp.digamma(mp.mpf(float(nu)))))
        cst = L(str((1 - mp.mpf(float(nu))) * mp.log(2) - mp.loggamma(mp.mpf(float(nu)))))
    step = L(1) / L(16)
    smax = float(np.log(2.0 * (800.0 + 60.0 * nu) / flat[pos].min()) + 3.0)
    s = (np.arange(int(np.ceil(smax / float(step))) + 1).astype(L) * step)[None, :]
    w = np.full(s.shape, L(0.5))
    w[0, 0] = L(0.25)
    lu = np.log(uu)
    with np.errstate(over="ignore", under="ignore"):
        uc = uu * np.cosh(s)
        ap, am = lu + s, lu - s
        f = (ap - kk) * np.exp(nul * ap + cst - uc) + (am - kk) * np.exp(nul * am + cst - uc)
    res[pos] = ((f * w).sum(1) * step).astype(np.float64)
    return out


def corr_fns(nu, u, dnu="quad"):
    r, h = rho_h(nu, u)
    if dnu == "mp":
        n = np.vectorize(lambda x: dnu_mp(nu, x), otypes=[np.float64])(np.asarray(u, dtype=np.float64))
    else:
        n = dnu_quad(nu, u)
    return r, h, n


def pair_tables(coords, theta, dnu="quad"):
    """(rho, h, n) for every pair of points, (N, N) each: computed once and shared by the cases of a parity test."""
    d = np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(-1))
    iu = np.triu_indices(d.shape[0], 1)  # d is symmetric bit for bit: each pair once
    out = []
    for v in corr_fns(float(theta[3]), theta[1] * d[iu], dnu):
        a = np.zeros_like(d)
        a[iu] = v
        a = a + a.T
        out.append(a)
    out[0][np.diag_indices_from(d)] = 1.0
    return tuple(out)


def ref_rows_matern(coords, nbr, theta, y, rows=None, dtype=np.float64, dnu="quad", tables=None):
    """Per-location (log F, r^2/F, G[4]) for theta = (sigma2, phi, tau2, nu): dense numpy algebra on each joint
    block in ``dtype`` (fp64 or its ``np.longdouble`` twin on the same correlation values).  ``tables``:
    :func:`pair_tables` of the same coords and theta, else the functions are evaluated block by block."""
    s2, phi, t2 = (dtype(x) for x in theta[:3])
    nu = float(theta[3])
    cd, y = coords.astype(dtype), y.astype(dtype)
    rows = range(coords.shape[0]) if rows is None else rows
    out = np.zeros((len(rows), 6), dtype=dtype)
    for t, i in enumerate(rows):
        nb = [j for j in nbr[i] if j >= 0]
        k = len(nb)
        idx = nb + [i]
        X = cd[idx]
        d = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
        if tables is not None:
            r_, h_, n_ = (a[np.ix_(idx, idx)].astype(dtype) for a in tables)
        else:
            r_, h_, n_ = (a.astype(dtype) for a in corr_fns(nu, (phi * d).astype(np.float64), dnu))
        C = s2 * r_ + t2 * np.eye(k + 1, dtype=dtype)
        Dp, Dn = s2 * h_ / phi, s2 * n_
        np.fill_diagonal(Dp, 0.0)
        np.fill_diagonal(Dn, 0.0)
        yy = y[idx]
        if k:
            sol = chol_solve(C[:k, :k], np.stack([C[:k, k], yy[:k]], 1))
            b, a = sol[:, 0], sol[:, 1]
        else:
            b = a = np.zeros(0, dtype=dtype)
        u = np.append(-b, dtype(1.0))
        al = np.append(a, dtype(0.0))
        F = u @ C @ u
        r = yy[k] - b @ yy[:k]
        nb2, adb = b @ b, a @ b
        dF = [(F - t2 * (1 + nb2)) / s2, u @ Dp @ u, 1 + nb2, u @ Dn @ u]
        dr = [-t2 * adb / s2, -(al @ Dp @ u), adb, -(al @ Dn @ u)]
        out[t, 0], out[t, 1] = np.log(F), r * r / F
        for p in range(4):
            out[t, 2 + p] = -0.5 * ((dF[p] / F) * (1 - r * r / F) + 2 * r * dr[p] / F)
    return out


def field(n, dim=2, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (n, dim)), rng.standard_normal(n)


def prior_nbr(coords, m):
    """The m nearest earlier points of each location (-1 padded), ties by index: the library's sets for such
    points, restated here so that the host tests need no GPU."""
    n = coords.shape[0]
    nbr = np.full((n, m), -1, dtype=np.int32)
    for i in range(1, n):
        d = ((coords[:i] - coords[i]) ** 2).sum(1)
        o = np.argsort(d, kind="stable")[:m]
        nbr[i, :len(o)] = o
    return nbr


# the GPU parity test's inputs (test_gpu_grad_matern.py) and the host test that conditions its tolerance
PARITY_N = 300
PARITY_SEED = 1
PARITY_NUS = (0.3, 1.0, 1.3, 2.5)
# every m at which grad_lanes(m) (bf_grad.h: 2 lanes to 8, 4 to 15, 8 to 23, 16 to 31, 64 at 32) or the local-row
# count S = ceil((m + 1) / P) changes, and the m just below it, plus 1, 15, 32
def _lanes(m):
    return 2 if m <= 8 else 4 if m <= 15 else 8 if m <= 23 else 16 if m <= 31 else 64


def _s_rows(m):
    return -(-(m + 1) // _lanes(m))


PARITY_MS = sorted({1, 15, 32} | {k for m in range(2, 33) if (_lanes(m), _s_rows(m)) != (_lanes(m - 1), _s_rows(m - 1))
                                  for k in (m - 1, m)})


def parity_theta(nu, dim=2):
    return (1.3, 6.0 if dim > 1 else 12.0, 0.05, nu)
