"""GPU: every forward-sweep kernel family (B, F, residual, the two log-likelihood sums) against extended precision at
rounding level: |got - reference| <= BF_K U scale per row, the reference an np.longdouble restatement and the scales
first-order bounds (tests/bf_precision_ref.py: ``bf_reference``, ``check_sweep``, the inputs).  BF_K is measured on the
CPU from the fp64 oracle against the same reference (tests/test_bf_precision_host.py), never from a kernel.

Two thetas per kind: the easy ones of tests/test_bf_matrix_host.py (cond(C_N) <= ~5e2; the bound is a few hundred ulp,
1e4 tighter than the fixed 1e-10 / 1e-9 tolerances of the older files) on field A and on field B (exact duplicates),
and the hard ones (tau2 -> 0, ranges longer than the neighbour spacing, cond up to ~5e12) on field A, where a row's
pivot test decides between NaN and a number.  Rows with BF_K U cond >= 1 are unresolved: a sweep may flag them (F and the
whole B row NaN) or return finite numbers, and nothing is compared there; the host file asserts that at least 95 % of
every case's rows are resolved.

Every sweep writes into NaN-prefilled buffers.  Each test prints its worst ratio per case.

General-nu Matern: nu = 0.5, 1.5, 2.5, where the long-double closed forms are the reference.  The table's covariance is
not rounding-level: tests/test_matern.py pins it to EPS_NU = 2e-15 (absolute, sigma2 = 1) of mpmath, so this kind alone
uses (U + EPS_NU) in place of U in the scales.  Other nu would need an extended-precision K_nu and are left out.
"""
import numpy as np
import pytest
import torch

import bf_precision_ref as P

pytestmark = pytest.mark.gpu

TRUSTED_M = (6, 13, 14, 18, 19, 22, 23, 24, 27, 32)  # one odd and one even m per structural class
CROSS_CASES = (("pairb", 10), ("pairb", 15), ("pairb", 20), ("pairb", 28), ("quad", 28), ("lane", 5), ("wave", 40))


@pytest.fixture(scope="module")
def lib():
    from pynngp_amd import _lib

    return _lib


def _dt(a, dev):
    # (a copy: the shared inputs are read-only arrays)
    return torch.from_numpy(np.array(a, order="C")).to(dev)


def _nan(dev, *shape):
    return torch.full(shape, np.nan, dtype=torch.float64, device=dev)


def _sweep(lib, c, nbr, kind, theta, v, algo, cert=None, nu=None):
    """One sweep into fresh NaN-filled buffers: host (B, F, R, partials)."""
    dev = c.device
    rows, m = nbr.shape
    B, F, R, p = _nan(dev, rows, m), _nan(dev, rows), _nan(dev, rows), _nan(dev, 4)
    lib.bf_sweep(c, nbr, 0, kind, *theta, values=v, algo=algo, B=B, F=F, R=R, partials=p, cert=cert, nu=nu)
    return tuple(t.cpu().numpy() for t in (B, F, R, p))


def _cross(lib, ref, q, nbr, kind, theta, vr, vq, algo):
    dev = ref.device
    rows, m = nbr.shape
    B, F, R, p = _nan(dev, rows, m), _nan(dev, rows), _nan(dev, rows), _nan(dev, 4)
    lib.bf_cross(ref, q, nbr, kind, *theta, ref_values=vr, query_values=vq, algo=algo, B=B, F=F, R=R, partials=p)
    return tuple(t.cpu().numpy() for t in (B, F, R, p))


def _prior_cases(lib, dev, algo, dim, m, kinds, trusted=False):
    """Easy theta on fields A and B and the hard theta on field A, per kind; the worst ratios are printed."""
    a, b, y = P.fields(dim)
    v = _dt(y, dev)
    worst = np.zeros(3)
    for fld, coords in ((0, a), (1, b)):
        c, nb = _dt(coords, dev), _dt(P.neighbours(dim, m, fld), dev)
        cert = lib.nbr_cert(c, nb, 0) if trusted else None
        for kind in kinds:
            for which in ("easy", "hard") if fld == 0 else ("easy",):
                theta = P.theta_of(kind, which, dim)
                if trusted:
                    # three tiles of 100 rows: the padded rows' tile is checked, the other two run trusted -- up to
                    # m = 24 (nbr_cert.h kCertMaxM); above, a certified sweep runs the checked body in every tile
                    tiles = lib.load().nngp_nbr_cert_trusted_tiles(cert[1], lib.KIND_CODES[kind], *theta)
                    assert tiles == (2 if m <= 24 else 0), (kind, theta, tiles)
                got = _sweep(lib, c, nb, kind, theta, v, algo, cert=cert)
                ref = P.prior_reference(dim, m, kind, theta, fld)
                where = f"{algo}{' trusted' if trusted else ''} d={dim} m={m} {kind} {which} field {'AB'[fld]}"
                worst = np.maximum(worst, P.check_sweep(ref, *got, where))
        if trusted:
            break  # the certificate's body is bit-identical to the checked one (test_gpu_bf_matrix.py): field A only
    print(f"{algo} d={dim} m={m}: worst ratios B {worst[0]:.3g} F {worst[1]:.3g} R {worst[2]:.3g}")


@pytest.mark.parametrize("m", P.M_PAIRB)
@pytest.mark.parametrize("dim", P.DIMS)
def test_pairb_rounding_level(lib, dev, dim, m):
    """Every pair-kernel instantiation m = 1 .. 32, the five closed-form kinds."""
    assert lib.resolve_algo("pairb", m, "exponential", dim) == "pairb"
    _prior_cases(lib, dev, "pairb", dim, m, P.KINDS)


@pytest.mark.parametrize("m", TRUSTED_M)
@pytest.mark.parametrize("dim", P.DIMS)
def test_pairb_trusted_body_rounding_level(lib, dev, dim, m):
    """The sweep under a certificate, field A, both thetas: tiles 1 and 2 run the TRUSTED body for m <= 24; at m = 27
    and 32 there is no trusted instantiation and the certified sweep is the checked body."""
    _prior_cases(lib, dev, "pairb", dim, m, P.KINDS, trusted=True)


@pytest.mark.parametrize("m", range(25, 33))
@pytest.mark.parametrize("dim", P.DIMS)
def test_quad_rounding_level(lib, dev, dim, m):
    _prior_cases(lib, dev, "quad", dim, m, P.KINDS)


@pytest.mark.parametrize("m", [1, 2, 8, 15, 16])
def test_lane_rounding_level(lib, dev, m):
    """The lane kernel serves 2-D exponential and Matern-3/2."""
    _prior_cases(lib, dev, "lane", 2, m, ("exponential", "matern32"))


@pytest.mark.parametrize("m", [15, 24, 33, 40, 63])
@pytest.mark.parametrize("dim", P.DIMS)
def test_wave_rounding_level(lib, dev, dim, m):
    _prior_cases(lib, dev, "wave", dim, m, P.KINDS)


@pytest.mark.parametrize("dim,algo,m", [(d, a, m) for d in P.DIMS for a, m in CROSS_CASES if a != "lane" or d == 2])
def test_bf_cross_rounding_level(lib, dev, dim, algo, m):
    """100 query points against field A, 30 of them exact copies of reference points, tau2 = 0.05 (the lane kernel
    is 2-D only)."""
    a, _, y = P.fields(dim)
    q, yq = P.cross_sets(dim)
    nbr = P.cross_neighbours(dim, m)
    args = [_dt(x, dev) for x in (a, q, nbr)]
    vr, vq = _dt(y, dev), _dt(yq, dev)
    kinds = ("exponential", "matern32") if algo == "lane" else P.KINDS
    worst = np.zeros(3)
    for kind in kinds:
        theta = P.CROSS_THETAS[kind]
        got = _cross(lib, *args, kind, theta, vr, vq, algo)
        ref = P.cross_reference(dim, m, kind, theta)
        assert ref.resolved.all()
        worst = np.maximum(worst, P.check_sweep(ref, *got, f"cross {algo} d={dim} m={m} {kind}"))
    print(f"cross {algo} d={dim} m={m}: worst ratios B {worst[0]:.3g} F {worst[1]:.3g} R {worst[2]:.3g}")


@pytest.mark.parametrize("algo,m", [("pairb", 6), ("pairb", 15), ("pairb", 18), ("pairb", 24), ("quad", 25), ("quad", 32)])
@pytest.mark.parametrize("dim", P.DIMS)
def test_matern_table_rounding_level(lib, dev, dim, algo, m):
    """The general-nu kind at nu = 0.5, 1.5, 2.5 on field A against the long-double closed forms, with (U + EPS_NU)
    for U in the scales (module docstring)."""
    a, _, y = P.fields(dim)
    c, nb, v = _dt(a, dev), _dt(P.neighbours(dim, m, 0), dev), _dt(y, dev)
    worst = np.zeros(3)
    for nu, closed in P.MATERN_CLOSED.items():
        assert lib.resolve_algo("auto", m, "matern", dim, nu=nu) == algo
        got = _sweep(lib, c, nb, "matern", P.MATERN_THETA, v, algo, nu=nu)
        ref = P.prior_reference(dim, m, closed, P.MATERN_THETA, 0)
        assert ref.resolved.all()
        worst = np.maximum(worst, P.check_sweep(ref, *got, f"matern nu={nu} {algo} d={dim} m={m}", u=P.U + P.EPS_NU))
    print(f"matern {algo} d={dim} m={m}: worst ratios B {worst[0]:.3g} F {worst[1]:.3g} R {worst[2]:.3g}")
