"""GPU: every instantiation of the two-lane pair kernel up to m = 24 (``launch_pairb_if<M, D>`` in
pynngp_amd/csrc/bf_pairb.h: one code object per (M, KIND, D), and for the five closed-form kinds a second, TRUSTED
body in each) against the C oracle.

The kernel's structure changes with all three parameters -- looking direction, waves per SIMD, factor rows in LDS,
the last pair (odd / even m), the point load per dimension -- so every (dim, kind, m) is a case of its own and a
failure names it.

n = 300 throughout (tests/test_gpu_cert.py's shape): three tiles of 100 rows in blocks of 128 row slots (idle lanes
in every block); tile 0 holds all the padded rows, tiles 1 and 2 are full and run trusted under a certificate.
Inputs, thetas and the precondition of the tolerances (the oracle within 1 % of them against np.longdouble on these
very inputs) are in tests/test_bf_matrix_host.py.  Tolerances: tests/test_gpu_bf.py's.

Every sweep writes into NaN-prefilled buffers, so a row that a kernel skips fails its case.  No test sweeps with a
certificate built for other contents (that would be an unchecked out-of-range read).
"""
import numpy as np
import pytest
import torch

from test_bf_matrix_host import DIMS, KINDS, M_ALL, N, THETAS, fields, neighbours

pytestmark = pytest.mark.gpu

RTOL_F = 1e-10
ATOL_B = 1e-9
RTOL_LL = 1e-12
ATOL_R = 1e-9
MATERN_THETA = (1.0, 10.0, 0.1)
MATERN_NUS = (0.3, 0.8, 1.7, 2.9)  # by (m + dim) % 4: every nu meets both looking directions and every dimension


@pytest.fixture(scope="module")
def lib():
    from pynngp_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ops():
    from pynngp_amd import load_ops

    return load_ops()


def _dt(a, dev):
    # (a copy: the shared inputs are read-only arrays)
    return torch.from_numpy(np.array(a, order="C")).to(dev)


def _sweep(lib, ops, c, nbr, kind, theta, v, i0=0, order=None, cert=None, nu=-1.0):
    """One sweep on the pair kernel into fresh NaN-filled buffers: (B, F, R, partials)."""
    dev = c.device
    rows, m = nbr.shape
    B = torch.full((rows, m), np.nan, dtype=torch.float64, device=dev)
    F = torch.full((rows,), np.nan, dtype=torch.float64, device=dev)
    R = torch.full((rows,), np.nan, dtype=torch.float64, device=dev)
    p = torch.full((4,), np.nan, dtype=torch.float64, device=dev)
    ws = lib.bf_workspace(rows, m, "pairb", dev, kind=kind, dim=c.shape[1])
    cb, ci = cert if cert is not None else (None, None)
    torch.ops.nngp.bf_sweep_out(c, nbr, order, i0, ops.kind_code(kind), *theta, v, B, F, R, p, ws,
                                ops.algo_code("pairb"), nu, None, None, cb, ci)
    return B, F, R, p


def _same(a, b):
    # (NaN-aware: the bits are compared)
    return all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a, b))


def _against_oracle(got, O, coords, nbr, kind, theta_oracle, y, where):
    B, F, R, p = (t.cpu().numpy() for t in got)
    Bo, Fo, po = O.c_bf_sweep(coords, nbr, kind, theta_oracle, y)
    assert po[2] == -1
    assert not np.isnan(B).any() and not np.isnan(F).any() and not np.isnan(R).any(), where
    eF, eB = np.abs(F - Fo) / Fo, np.abs(B - Bo) / (1 + np.abs(Bo))
    Ro = y - np.einsum("ij,ij->i", Bo, np.where(nbr >= 0, y[np.maximum(nbr, 0)], 0.0))
    eR = np.abs(R - Ro)
    ll, llo = O.loglik_from_partials(p, N), O.loglik_from_partials(po, N)
    kappa = float(np.max((theta_oracle[0] + theta_oracle[2]) / Fo))
    print(f"{where}: max |dF| / F {eF.max():.3g}, |dB| / (1 + |B|) {eB.max():.3g}, |dR| {eR.max():.3g}, "
          f"|dl| / |l| {abs(ll - llo) / abs(llo):.3g} (kappa {kappa:.3g})")
    assert p[2] == -1 and p[3] == -1, where
    assert np.all(eF <= RTOL_F), (where, int(eF.argmax()), eF.max())
    assert np.all(eB <= ATOL_B), (where, int(eB.max(axis=1).argmax()), eB.max())
    assert np.all(B[nbr < 0] == 0.0), where
    assert np.all(eR <= ATOL_R), (where, int(eR.argmax()), eR.max())
    assert abs(ll - llo) <= max(RTOL_LL, 1e-15 * kappa) * abs(llo), (where, ll, llo, kappa)


@pytest.mark.parametrize("m", M_ALL)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", DIMS)
def test_pairb_matrix_vs_oracle(lib, ops, dev, c_oracle, dim, kind, m):
    """The checked body of (m, kind, dim) on field A (no coincident points) and field B (exact duplicates: d2 = 0, the
    distance floor) against the oracle; then, on field A, the TRUSTED body under a certificate: tiles 1 and 2 run
    it, and the sweep returns the uncertified sweep's bits."""
    assert lib.resolve_algo("auto", m, kind, dim) == "pairb"
    theta = THETAS[kind]
    a, b, y = fields(dim)
    v = _dt(y, dev)
    plain = None
    for which, coords in ((0, a), (1, b)):
        nbr = neighbours(dim, m, which)
        c, nb = _dt(coords, dev), _dt(nbr, dev)
        got = _sweep(lib, ops, c, nb, kind, theta, v)
        _against_oracle(got, c_oracle, coords, nbr, kind, theta, y, f"d={dim} {kind} m={m} field {'AB'[which]}")
        if which == 0:
            plain, c_a, nb_a = got, c, nb
    cert = ops.nbr_cert(c_a, nb_a, None, 0)
    info = cert[1].tolist()
    assert info[9] == 3 and info[10] == 1  # three tiles, the padded rows' tile checked
    assert ops.nbr_cert_trusted_tiles(cert[1], kind, theta) == 2
    certified = _sweep(lib, ops, c_a, nb_a, kind, theta, v, cert=cert)
    torch.cuda.synchronize()
    assert _same(plain, certified)


@pytest.mark.parametrize("m", M_ALL)
@pytest.mark.parametrize("dim", DIMS)
def test_pairb_matern_table_matrix_vs_oracle(lib, ops, dev, c_oracle, dim, m):
    """The general-nu Matern table kernel of (m, dim) on field A (left-looking at m = 18, right-looking elsewhere)."""
    nu = MATERN_NUS[(m + dim) % 4]
    assert lib.resolve_algo("auto", m, "matern", dim, nu=nu) == "pairb"
    a, _, y = fields(dim)
    nbr = neighbours(dim, m, 0)
    c, nb, v = _dt(a, dev), _dt(nbr, dev), _dt(y, dev)
    got = _sweep(lib, ops, c, nb, "matern", MATERN_THETA, v, nu=nu)
    _against_oracle(got, c_oracle, a, nbr, "matern", MATERN_THETA + (nu,), y, f"d={dim} matern nu={nu} m={m}")


@pytest.mark.parametrize("m", [6, 13, 14, 18, 19, 22, 23, 24])  # one odd and one even m per structural class
@pytest.mark.parametrize("kind", ["matern52", "spherical"])
@pytest.mark.parametrize("dim", [1, 3])
def test_pairb_matrix_row_order_and_offset(lib, ops, dev, dim, kind, m):
    """Rows [100, 300) with i0 = 100, visited through a ``row_order`` permutation, are the full sweep's rows bit for
    bit (field B: the duplicates lie in the swept range)."""
    theta = THETAS[kind]
    _, b, y = fields(dim)
    nbr = neighbours(dim, m, 1)
    c, nb, v = _dt(b, dev), _dt(nbr, dev), _dt(y, dev)
    Bf, Ff, Rf, pf = _sweep(lib, ops, c, nb, kind, theta, v)
    i0, rows = 100, N - 100
    order, srt = lib.row_order(c, i0, rows, nb[i0:])
    oh = order.cpu().numpy()
    assert np.array_equal(np.sort(oh), np.arange(rows)) and not np.array_equal(oh, np.arange(rows))
    assert torch.equal(srt, nb[i0:][order.long()])
    Bs, Fs, Rs, ps = _sweep(lib, ops, c, srt.contiguous(), kind, theta, v, i0=i0, order=order)
    torch.cuda.synchronize()
    assert pf[2].item() == -1 and pf[3].item() == -1 and ps[2].item() == -1 and ps[3].item() == -1
    assert not torch.isnan(Ff).any() and not torch.isnan(Bf).any() and not torch.isnan(Rf).any()
    assert _same((Bf[i0:], Ff[i0:], Rf[i0:]), (Bs, Fs, Rs))
