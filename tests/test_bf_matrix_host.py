"""CPU: the inputs of tests/test_gpu_bf_matrix.py (the pair-sweep instantiations m = 1 .. 24; the kernel is
instantiated to m = 32, and tests/test_gpu_bf_precision.py covers M_PRECISION = 1 .. 32 on these fields) and the
precondition of its tolerances.

The GPU file compares the pair kernel with the C oracle (oracle/nngp_oracle.c, fp64) at |dF| <= 1e-10 F and
|dB| <= 1e-9 (1 + |B|).  Those figures measure the kernel only where the oracle's own fp64 rounding is far below
them, so here the oracle's B and F are compared with an ``np.longdouble`` restatement (closed-form covariance in
extended precision -- tests/test_gpu_bf.py::test_bf_m1_covariance_ulp's convention -- and a scalar Cholesky of the
(m + 1) x (m + 1) block) on the very inputs of the GPU file: the oracle must sit within 1 % of each tolerance,
1e-12 F and 1e-11 (1 + |B|).

Measured with the inputs below (n = 300, both fields, d = 1, 2, 3, m = 1 .. 24, 8 rows per case; the test prints
them per (dim, kind)): the largest |dF| / F is 6.5e-15 and the largest |dB| / (1 + |B|) 4.0e-15, both Matern-3/2
in d = 1; more than two orders below the 1 % marks.  No input had to be changed to meet the precondition.
"""
import functools

import numpy as np
import pytest

from oracle import nngp_oracle as O

N = 300
DIMS = (1, 2, 3)
M_ALL = tuple(range(1, 25))
M_PRECISION = tuple(range(1, 33))  # the precision files' range (tests/bf_precision_ref.py): every pair instantiation
SEED = 24
# one theta per kind; tau2 >= 0.05 keeps the blocks of field B (exact duplicates) positive definite
THETAS = {
    "exponential": (1.0, 12.0, 0.05),
    "matern32": (1.2, 9.0, 0.1),
    "matern52": (1.0, 8.0, 0.1),
    "gaussian": (1.0, 4.0, 0.2),
    "spherical": (0.9, 3.0, 0.05),
}
KINDS = tuple(THETAS)
DUP_ROWS, DUP_OF = slice(290, 294), 250


@functools.lru_cache(maxsize=None)
def fields(dim, seed=SEED):
    """(coords A, coords B, y): field A has no coincident points; field B is field A with rows 290 .. 293 exact
    copies of row 250 (d2 = 0: the kernel's 2^-1000 floor, the clamp path).  Read-only: shared by every case."""
    rng = np.random.default_rng(1000 * seed + dim)
    a = rng.uniform(0.0, 1.0, (N, dim))
    y = rng.standard_normal(N)
    assert len(np.unique(a, axis=0)) == N
    b = a.copy()
    b[DUP_ROWS] = b[DUP_OF]
    for arr in (a, b, y):
        arr.setflags(write=False)
    return a, b, y


@functools.lru_cache(maxsize=None)
def neighbours(dim, m, which):
    nbr = O.c_knn_prior(fields(dim)[which], m)
    nbr.setflags(write=False)
    return nbr


def rho_longdouble(kind, u):
    if kind == "exponential":
        return np.exp(-u)
    if kind == "matern32":
        return (1 + u) * np.exp(-u)
    if kind == "matern52":
        return (1 + u + u * u / 3) * np.exp(-u)
    if kind == "gaussian":
        return np.exp(-u * u)
    if kind == "spherical":
        return np.where(u < 1, 1 - 1.5 * u + 0.5 * u ** 3, np.longdouble(0))
    raise ValueError(kind)


def chol_solve_longdouble(A, rhs):
    """A^-1 rhs by a scalar-loop Cholesky (rows of L by dot products), everything np.longdouble."""
    k = A.shape[0]
    L = np.zeros_like(A)
    for j in range(k):
        L[j, j] = np.sqrt(A[j, j] - np.dot(L[j, :j], L[j, :j]))
        for i in range(j + 1, k):
            L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    x = rhs.copy()
    for i in range(k):
        x[i] = (x[i] - np.dot(L[i, :i], x[:i])) / L[i, i]
    for i in range(k - 1, -1, -1):
        x[i] = (x[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
    return x


def bf_row_longdouble(coords, nbr_row, i, kind, theta):
    """(B_i (m,) with 0 in the padded slots, F_i) of one location in np.longdouble."""
    ld = np.longdouble
    s2, phi, t2 = (ld(x) for x in theta)
    ok = nbr_row >= 0
    idx = list(nbr_row[ok]) + [i]
    k = len(idx) - 1
    X = coords[idx].astype(ld)
    d = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=-1))
    C = s2 * rho_longdouble(kind, phi * d) + t2 * np.eye(k + 1, dtype=ld)
    B = np.zeros(len(nbr_row), dtype=ld)
    if k == 0:
        return B, s2 + t2
    b = chol_solve_longdouble(C[:k, :k], C[:k, k])
    B[ok] = b
    return B, C[k, k] - np.dot(C[:k, k], b)


def sample_rows(dim, m):
    """Rows m - 1 (the last padded one), m (the first full one), 150, 292 (a duplicate in field B), 299 and three
    random ones."""
    rng = np.random.default_rng(7919 * dim + m)
    extra = rng.choice(np.setdiff1d(np.arange(N), [m - 1, m, 150, 292, 299]), 3, replace=False)
    return [m - 1, m, 150, 292, 299] + sorted(int(r) for r in extra)


@pytest.mark.skipif(np.finfo(np.longdouble).eps >= 2.0 ** -60, reason="np.longdouble is no wider than fp64 here")
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", DIMS)
def test_oracle_within_one_percent_of_the_matrix_tolerances(dim, kind):
    """Every (dim, kind, m) of test_gpu_bf_matrix.py::test_pairb_matrix_vs_oracle, both fields, 8 rows each: the C
    oracle's F within 1e-12 F and its B within 1e-11 (1 + |B|) of the np.longdouble restatement (module docstring:
    6.5e-15 and 4.0e-15 at the worst; no input had to be changed)."""
    theta = THETAS[kind]
    worst_f, worst_b = (0.0, None), (0.0, None)
    for m in M_ALL:
        rows = sample_rows(dim, m)
        assert len(set(rows)) >= 8
        for which in (0, 1):
            coords, nbr = fields(dim)[which], neighbours(dim, m, which)
            Bo, Fo, po = O.c_bf_sweep(coords, nbr, kind, theta, None)
            assert po[2] == -1
            for i in rows:
                Bx, Fx = bf_row_longdouble(coords, nbr[i], i, kind, theta)
                eF = float(abs(Fo[i] - Fx) / Fx)
                eB = float(np.max(np.abs(Bo[i] - Bx) / (1 + np.abs(Bx))))
                assert eF <= 1e-12, (dim, kind, m, "AB"[which], i, eF)
                assert eB <= 1e-11, (dim, kind, m, "AB"[which], i, eB)
                if eF > worst_f[0]:
                    worst_f = (eF, (m, "AB"[which], i))
                if eB > worst_b[0]:
                    worst_b = (eB, (m, "AB"[which], i))
    print(f"d={dim} {kind}: oracle vs longdouble: max |dF| / F = {worst_f[0]:.3g} at (m, field, row) {worst_f[1]}, "
          f"max |dB| / (1 + |B|) = {worst_b[0]:.3g} at {worst_b[1]}")


def test_fields_are_what_the_matrix_needs():
    """Field B's duplicates are exact and are neighbours of one another (so d2 = 0 reaches a kernel at every m >= 1);
    the first m rows, and only those, are padded."""
    for dim in DIMS:
        a, b, _ = fields(dim)
        assert np.all(b[DUP_ROWS] == b[DUP_OF]) and np.array_equal(np.delete(a, np.r_[DUP_ROWS], 0),
                                                                   np.delete(b, np.r_[DUP_ROWS], 0))
        for m in (1, 2, 13, 24):
            nbr = neighbours(dim, m, 1)
            assert np.array_equal((nbr < 0).any(axis=1), np.arange(N) < m)
            assert set(nbr[293, :min(m, 4)]) <= {250, 290, 291, 292} and nbr[290, 0] == 250
