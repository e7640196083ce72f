"""Inputs and references shared by the 4 .. 16-dimensional tests (test_nd_host.py, test_gpu_nd.py, test_gpu_knn_nd.py).

The references are the project's dimension-generic ones: ``oracle.nngp_oracle.knn_prior`` / ``knn_all``,
``grad_aniso_ref.ref_rows_aniso`` (fp64 and its long-double twin) and ``bf_precision_ref.bf_reference`` on the
coordinates scaled by the decays (the model is the isotropic one at phi = 1 there).  Uniform points in [0, 1]^d sit
about sqrt(d / 6) apart, so the decays are of order 0.3 .. 3, unequal across the axes, one of them 10x the others."""
import functools

import numpy as np

from oracle import nngp_oracle as O

import bf_precision_ref as P
from grad_aniso_ref import ref_rows_aniso

KINDS = ("exponential", "matern32", "matern52", "gaussian")
DIMS = (4, 8, 16)
MS = (1, 2, 7, 8, 9, 15, 16, 23, 24, 31, 32)  # the lane-width edges of grad_lanes
N = 600
N_QUERY = 60
SIGMA2, TAU2 = 1.3, 0.05
GRAD_ROWS = tuple(range(0, 40)) + tuple(range(40, N, 7))  # the first rows (fewer than m neighbours) and a spread


def phis(dim, kind="exponential"):
    """Unequal decays of order 0.3 .. 3 / sqrt(dim / 4), the second 10x the smallest scale."""
    base = np.array([0.3 + 0.17 * ((3 * k) % 7) for k in range(dim)])
    base[1] = 10.0 * 0.3
    scale = {"exponential": 1.0, "matern32": 1.6, "matern52": 2.0, "gaussian": 0.9}[kind]
    return tuple(float(x) for x in base * scale / np.sqrt(dim / 4.0))


def theta(dim, kind):
    return (SIGMA2, *phis(dim, kind), TAU2)


@functools.lru_cache(maxsize=None)
def field(dim):
    rng = np.random.default_rng(100 + dim)
    c, y = rng.uniform(0.0, 1.0, (N, dim)), rng.standard_normal(N)
    q, yq = rng.uniform(0.0, 1.0, (N_QUERY, dim)), rng.standard_normal(N_QUERY)
    q[:10] = c[rng.choice(N, 10, replace=False)]  # coincident query points
    for a in (c, y, q, yq):
        a.setflags(write=False)
    return c, y, q, yq


@functools.lru_cache(maxsize=None)
def neighbours(dim, kind, m):
    """Prior sets in the metric of the decays (what NNGP builds); the first m rows carry -1 padding."""
    c = field(dim)[0] * np.array(phis(dim, kind))
    nbr = O.knn_prior(c, m).astype(np.int32)
    nbr.setflags(write=False)
    return nbr


@functools.lru_cache(maxsize=None)
def cross_neighbours(dim, kind, m):
    c, _, q, _ = field(dim)
    s = np.array(phis(dim, kind))
    nbr = O.knn_all(q * s, c * s, m).astype(np.int32)
    nbr.setflags(write=False)
    return nbr


def iso_theta():
    return (SIGMA2, 1.0, TAU2)


@functools.lru_cache(maxsize=None)
def prior_reference(dim, kind, m):
    c, y, _, _ = field(dim)
    s = c * np.array(phis(dim, kind))
    return P.bf_reference(s, s, neighbours(dim, kind, m), kind, iso_theta(), y, y)


@functools.lru_cache(maxsize=None)
def cross_reference(dim, kind, m):
    c, y, q, yq = field(dim)
    s = np.array(phis(dim, kind))
    return P.bf_reference(c * s, q * s, cross_neighbours(dim, kind, m), kind, iso_theta(), y, yq)


def fp64_sweep(dim, kind, m):
    """The fp64 restatement of the forward sweep (the oracle's) on the same inputs: (B, F, R)."""
    c, y, _, _ = field(dim)
    s = c * np.array(phis(dim, kind))
    nbr = neighbours(dim, kind, m)
    B, F, _ = O.bf_sweep(s, nbr, kind, iso_theta(), y)
    return B, F, P.oracle_residual(B, nbr, y, y)


@functools.lru_cache(maxsize=None)
def grad_rows(dim, kind, m, long_double=False):
    c, y, _, _ = field(dim)
    return ref_rows_aniso(c, neighbours(dim, kind, m), kind, theta(dim, kind), y, rows=list(GRAD_ROWS),
                          dtype=np.longdouble if long_double else np.float64)


def neighbour_correlations(dim, kind, m=15):
    """rho(u) between every location and its neighbours (what must stay away from 0 and 1)."""
    c = field(dim)[0] * np.array(phis(dim, kind))
    nbr = neighbours(dim, kind, m)[m:]
    d = np.sqrt(((c[m:, None, :] - c[nbr]) ** 2).sum(-1))
    return O.cov_fn(kind, d, 1.0, 1.0)


@functools.lru_cache(maxsize=None)
def grad_all(dim, kind, m):
    """Every row of the fp64 restatement (what the GPU rows and sums are compared with)."""
    c, y, _, _ = field(dim)
    out = ref_rows_aniso(c, neighbours(dim, kind, m), kind, theta(dim, kind), y)
    out.setflags(write=False)
    return out
