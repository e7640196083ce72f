"""Helpers of tests/test_bf_precision_host.py and tests/test_gpu_bf_precision.py (not a conftest): the forward sweep
(B, F, residual, the two log-likelihood sums) restated in np.longdouble, its first-order error scales, the inputs and the
comparison the two files share.

Reference.  ``bf_reference`` is vectorised over the rows with a scalar-loop Cholesky over the block
(tests/test_latent_grad_host.py::_chol_solve's style); the covariance is the closed form in long double
(tests/test_bf_matrix_host.py::rho_longdouble).  A slot that is -1 or out of range is a decoupled diagonal entry with
B = 0.  One code serves the prior form (row i against earlier points) and the cross form (a query point against a
reference set).

Scales.  An entry-wise perturbation U (sigma2 + tau2) of the (m + 1) x (m + 1) block passes through C_N^-1 into b and
through F = u^T C u, u = [-b; 1]:

    sB_i = (sigma2 + tau2) (1 + |b_i|_1) / lambda_min(C_N,i)
    sF_i = (sigma2 + tau2) (1 + |b_i|_1)^2
    sR_i = sB_i |y_N|_2 + |r_i|

(lambda_min and cond from the fp64 ``eigvalsh`` of the long-double block).  Two of them differ from the first draft of
these scales, both on the evidence of the fp64 oracle alone:

* sF had a further term cond_i |F_i|.  b minimises u^T C u, so F's first-order perturbation is u^T dC u with no factor
  cond, and a Cholesky's backward error is such a dC: without the term the oracle's worst ratio is 1.45 (0.90 with
  it), at cond = 1e13 as at cond = 10.  With it BF_K U sF / F is 2e-12 on the easy thetas (cond up to 860) -- looser
  than the 1e-12 the bound is required to bite at -- so the tighter scale is the one kept.
* sR lacked |r_i|, the rounding of the residual itself: at m = 1 a row with |y_N| << |y_i| put the oracle at 36 x
  U sB |y_N|; with the term the worst ratio is 0.88.

Hard thetas.  The issue's starting points, kept, except Matern-5/2 in d = 1: (1, 4, 0) leaves 29 .. 88 % of the rows
resolved there (cond up to 1e15), so d = 1 uses tau2 = 1e-9 with the same range -- HARD_THETAS_D1.
"""
import functools

import numpy as np

from oracle import nngp_oracle as O
from test_bf_matrix_host import DIMS, KINDS, M_PRECISION, N, THETAS, fields, neighbours, rho_longdouble  # noqa: F401

LD = np.longdouble
U = 2.0 ** -52
BF_K = 12.0  # 8 x the largest oracle ratio (1.45, F) rounded up: tests/test_bf_precision_host.py has the figures
RESOLVED_SHARE = 0.95
M_PAIRB = M_ALL = M_PRECISION
M_WAVE = (15, 24, 33, 40, 63)
HARD_THETAS = {
    "exponential": (1.0, 2.0, 0.0),
    "matern32": (1.0, 3.0, 0.0),
    "matern52": (1.0, 4.0, 0.0),
    "gaussian": (1.0, 3.0, 1e-6),
    "spherical": (1.0, 0.7, 0.0),
}
HARD_THETAS_D1 = {"matern52": (1.0, 4.0, 1e-9)}  # the one case whose starting point misses the 95 % cap
CROSS_THETAS = {k: (t[0], t[1], 0.05) for k, t in THETAS.items()}  # tau2 = 0.05: coincident query points stay regular
N_QUERY, N_COINCIDENT = 100, 30
# the general-nu kind at the half-integers, where the long-double closed forms are the reference
MATERN_CLOSED = {0.5: "exponential", 1.5: "matern32", 2.5: "matern52"}
MATERN_THETA = (1.0, 10.0, 0.1)
# tests/test_matern.py pins the table path to 2e-15 of mpmath (absolute, sigma2 = 1) and the oracle's integral to 1e-15
EPS_NU = 2e-15


def theta_of(kind, which, dim):
    """The easy or hard theta of a kind in a dimension."""
    if which == "easy":
        return THETAS[kind]
    return HARD_THETAS_D1[kind] if dim == 1 and kind in HARD_THETAS_D1 else HARD_THETAS[kind]


@functools.lru_cache(maxsize=None)
def cross_sets(dim):
    """(query (100, dim), query values, neighbour source): 100 query points against field A, the first 30 exact
    copies of reference points.  Read-only."""
    a = fields(dim)[0]
    rng = np.random.default_rng(4242 + dim)
    q = rng.uniform(-0.05, 1.05, (N_QUERY, dim))
    q[:N_COINCIDENT] = a[rng.choice(N, N_COINCIDENT, replace=False)]
    yq = rng.standard_normal(N_QUERY)
    for arr in (q, yq):
        arr.setflags(write=False)
    return q, yq


@functools.lru_cache(maxsize=None)
def cross_neighbours(dim, m):
    nbr = O.knn_all(cross_sets(dim)[0], fields(dim)[0], m).astype(np.int32)
    nbr.setflags(write=False)
    return nbr


def _chol_solve(A, R):
    """A^-1 R for a batch of SPD A (n, k, k) and right-hand sides R (n, k), by a scalar-loop Cholesky in A's dtype."""
    n, k, _ = A.shape
    L = np.zeros_like(A)
    for j in range(k):
        L[:, j, j] = np.sqrt(A[:, j, j] - (L[:, j, :j] ** 2).sum(axis=1))
        for i in range(j + 1, k):
            L[:, i, j] = (A[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(axis=1)) / L[:, j, j]
    Y = np.zeros_like(R)
    for i in range(k):
        Y[:, i] = (R[:, i] - (L[:, i, :i] * Y[:, :i]).sum(axis=1)) / L[:, i, i]
    X = np.zeros_like(R)
    for i in range(k - 1, -1, -1):
        X[:, i] = (Y[:, i] - (L[:, i + 1:, i] * X[:, i + 1:]).sum(axis=1)) / L[:, i, i]
    return X


class Ref:
    """Per row, np.longdouble: b (n, m), F, r, logF, q = r^2 / F; fp64: lam_min, cond, sB, sF, sR, pad (n, m)."""


def _blocks(ref, loc, nbr, kind, theta):
    """(C (n, m + 1, m + 1) long double, the valid slots ok (n, m), their indices j): the neighbours' block bordered by
    the location's column; an invalid slot is a decoupled diagonal entry."""
    ref, loc = np.asarray(ref, dtype=LD), np.asarray(loc, dtype=LD)
    n, m = nbr.shape
    ok = (nbr >= 0) & (nbr < len(ref))
    j = np.where(ok, nbr, 0)
    pts = np.concatenate([ref[j], loc[:n, None, :]], axis=1)
    valid = np.concatenate([ok, np.ones((n, 1), dtype=bool)], axis=1)
    dist = np.sqrt(((pts[:, :, None, :] - pts[:, None, :, :]) ** 2).sum(axis=-1))
    pair = valid[:, :, None] & valid[:, None, :] & ~np.eye(m + 1, dtype=bool)[None]
    s2, ph, t2 = LD(theta[0]), LD(theta[1]), LD(theta[2])
    C = np.where(pair, s2 * rho_longdouble(kind, ph * dist), LD(0)) + (s2 + t2) * np.eye(m + 1, dtype=LD)[None]
    return C, ok, j


def block_cond(ref, loc, nbr, kind, theta):
    """cond(C_N) per row from the fp64 ``eigvalsh`` of the long-double block alone (what ``resolved`` is judged by)."""
    C, _, _ = _blocks(ref, loc, nbr, kind, theta)
    ev = np.linalg.eigvalsh(C[:, :-1, :-1].astype(np.float64))
    with np.errstate(all="ignore"):
        return np.where(ev[:, 0] > 0, ev[:, -1] / ev[:, 0], np.inf)


def bf_reference(ref, loc, nbr, kind, theta, y_ref, y_loc):
    """The sweep of locations ``loc`` (rows, dim) against neighbours ``nbr`` (rows, m) indexing ``ref`` in long double,
    with the error scales (module docstring).  Prior form: loc = ref = the field; cross form: loc the query points."""
    C, ok, j = _blocks(ref, loc, nbr, kind, theta)
    n, m = nbr.shape
    s2, t2 = LD(theta[0]), LD(theta[2])
    CN, c = C[:, :m, :m], C[:, :m, m]
    with np.errstate(all="ignore"):
        b = _chol_solve(CN, c)
    b = np.where(ok, b, LD(0))
    out = Ref()
    out.b, out.pad = b, ~ok
    out.F = (s2 + t2) - (b * c).sum(axis=1)
    yN = np.where(ok, np.asarray(y_ref, dtype=LD)[j], LD(0))
    out.r = np.asarray(y_loc, dtype=LD)[:n] - (b * yN).sum(axis=1)
    with np.errstate(all="ignore"):
        out.logF, out.q = np.log(out.F), out.r * out.r / out.F
    ev = np.linalg.eigvalsh(CN.astype(np.float64))
    d = float(s2 + t2)
    b1 = 1.0 + np.abs(b).sum(axis=1).astype(np.float64)
    with np.errstate(all="ignore"):
        out.lam_min = ev[:, 0]
        out.cond = np.where(ev[:, 0] > 0, ev[:, -1] / ev[:, 0], np.inf)
        out.sB = np.where(ev[:, 0] > 0, d * b1 / ev[:, 0], np.inf)
        out.sF = d * b1 * b1
        out.sR = out.sB * np.linalg.norm(yN.astype(np.float64), axis=1) + np.abs(out.r.astype(np.float64))
    out.resolved = BF_K * U * out.cond < 1.0
    return out


@functools.lru_cache(maxsize=None)
def prior_reference(dim, m, kind, theta, which):
    """The reference of one (dim, m, kind, theta, field) case; shared, never modified."""
    coords, y = fields(dim)[which], fields(dim)[2]
    return bf_reference(coords, coords, neighbours(dim, m, which), kind, theta, y, y)


@functools.lru_cache(maxsize=None)
def cross_reference(dim, m, kind, theta):
    a, _, y = fields(dim)
    q, yq = cross_sets(dim)
    return bf_reference(a, q, cross_neighbours(dim, m), kind, theta, y, yq)


def ratios(ref, B, F, R, u=U):
    """The largest |got - reference| / (u x scale) over the resolved rows, for (B, F, R); 0 without resolved rows."""
    ok = ref.resolved
    tiny = np.finfo(np.float64).tiny
    with np.errstate(all="ignore"):
        eB = np.abs(B - ref.b).max(axis=1).astype(np.float64) / np.maximum(u * ref.sB, tiny)
        eF = np.abs(F - ref.F).astype(np.float64) / np.maximum(u * ref.sF, tiny)
        eR = np.abs(R - ref.r).astype(np.float64) / np.maximum(u * ref.sR, tiny)
    # a row without a neighbour has sR = 0 and R = y_i exactly
    return tuple(float(np.max(e[ok], initial=0.0)) for e in (eB, eF, eR))


def oracle_residual(Bo, nbr, y_ref, y_loc):
    """r = y_i - B_i y_N in fp64 from the oracle's B (the oracle keeps its own residual to itself)."""
    ok = (nbr >= 0) & (nbr < len(y_ref))
    return y_loc[:len(nbr)] - np.einsum("ij,ij->i", np.where(ok, Bo, 0.0), np.where(ok, y_ref[np.where(ok, nbr, 0)], 0.0))


def check_sweep(ref, B, F, R, p, where, u=U, i0=0):
    """The assertions of one sweep (fp64 host arrays B (n, m), F, R and partials p (4,)) against ``ref``; ``u`` is the
    unit in the scales (U, or U + EPS_NU for the table kind).  Returns the worst ratios (B, F, R) over the resolved
    rows.

    Resolved rows: no NaN; |B - b| <= BF_K u sB, |F - F_ref| <= BF_K u sF, |R - r| <= BF_K u sR; B == 0 exactly in the
    padded slots.  Unresolved rows: flagged (F and the whole B row NaN) or finite; nothing is compared.  Flags: p[2] ==
    -1 exactly when no row is NaN, else it names a NaN row; p[3] == -1.  Sums, when no row is NaN: |p[0] - sum log
    F_ref| <= 4 n U sum |log F| + sum BF_K u sF / F, and |p[1] - sum q_ref| <= 4 n U sum q + sum_i [(|r| + eR)^2 / (F
    - eF) - q]_i with eR, eF the row bounds (the largest r^2 / F those bounds allow; a case with eF >= F on some row
    has no bound on p[1] and is not compared).  An unresolved finite row enters the reference sums with the sweep's own
    F and R: the rule compares nothing there, and the fold of what the sweep wrote is still checked."""
    n, m = ref.b.shape
    ok = ref.resolved
    nanF = np.isnan(F)
    nanB = np.isnan(B).any(axis=1) if m else np.zeros(n, dtype=bool)
    assert not (nanF | nanB | np.isnan(R))[ok].any(), (where, "NaN on a resolved row", np.nonzero((nanF | nanB) & ok)[0][:5])
    rB, rF, rR = ratios(ref, B, F, R, u)
    print(f"{where}: ratios B {rB:.3g} F {rF:.3g} R {rR:.3g} (bound {BF_K:g}); resolved {ok.mean():.3f}, "
          f"max cond {ref.cond[ok].max(initial=1.0):.3g}")
    assert rB <= BF_K, (where, "B", rB)
    assert rF <= BF_K, (where, "F", rF)
    assert rR <= BF_K, (where, "R", rR)
    assert np.all(B[ref.pad & ~nanB[:, None]] == 0.0), (where, "padded slots")
    # unresolved rows: flagged as a whole, or finite
    flagged = nanF & ~ok
    assert np.all(np.isnan(B[flagged][~ref.pad[flagged]])), (where, "a flagged row keeps part of B")
    fin = ~ok & ~nanF
    assert np.all(np.isfinite(B[fin])) and np.all(np.isfinite(F[fin])), (where, "an unflagged row is not finite")
    assert p[3] == -1, (where, p)
    if not nanF.any():
        assert p[2] == -1, (where, p)
    else:
        assert p[2] >= i0 and p[2] == int(p[2]) and nanF[int(p[2]) - i0], (where, p)
        return rB, rF, rR
    F64, r64 = ref.F.astype(np.float64), np.abs(ref.r.astype(np.float64))
    eF, eR = BF_K * u * ref.sF, BF_K * u * ref.sR
    logF = np.where(ok, ref.logF.astype(np.float64), np.log(np.where(ok, 1.0, F)))
    q = np.where(ok, ref.q.astype(np.float64), np.where(ok, 0.0, R * R / F))
    slack0 = 4 * n * U * np.abs(logF).sum() + (eF / F64)[ok].sum()
    assert abs(p[0] - logF.sum()) <= slack0, (where, "sum log F", p[0], logF.sum(), slack0)
    if np.all(eF[ok] < F64[ok]):
        slack1 = 4 * n * U * q.sum() + ((r64 + eR) ** 2 / (F64 - eF) - r64 * r64 / F64)[ok].sum()
        assert abs(p[1] - q.sum()) <= slack1, (where, "sum r^2 / F", p[1], q.sum(), slack1)
    return rB, rF, rR
