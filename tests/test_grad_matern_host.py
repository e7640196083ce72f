"""CPU: the general-nu Matern gradient (nngp_bf_grad_matern, nngp_matern_eval_d): the two derivative functions of
the correlation, their table fit, the numpy restatement the GPU tests compare against, and every refusal that
needs no GPU.

h(u) = u rho'(u) and n(u) = d rho / d nu from pynngp_amd/csrc/nngp_math.h (host build, tests/host/
matern_drho_check.cpp) against mpmath at 50 digits.  Measured worst absolute errors:
  evaluator  h 3.9e-15 (nu = 50, u = 9.4, |h| ~ 10)   n 1.1e-14 (nu = 0.05, |n| ~ 5)
  table      h 6.4e-15 (nu = 49)                       n 1.4e-14 (nu = 0.05)
The bounds below are four times those (under the 1e-13 ceiling).
"""
import ctypes
import os
import subprocess

import mpmath as mp
import numpy as np
import pytest

import grad_matern_ref as R
from test_matern import NUS

HERE = os.path.dirname(os.path.abspath(__file__))
EVAL_NUS = tuple(NUS) + (0.05, 1.0, 2.0, 50.0)
BOUND_EVAL_H, BOUND_EVAL_N = 4 * 3.9e-15, 4 * 1.1e-14
BOUND_TAB_H, BOUND_TAB_N = 4 * 6.4e-15, 4 * 1.4e-14
assert max(BOUND_EVAL_H, BOUND_EVAL_N, BOUND_TAB_H, BOUND_TAB_N) <= 1e-13


def ref_hn(nu, u):
    mp.mp.dps = 50
    if u == 0:
        return mp.mpf(0), mp.mpf(0)
    return R.h_mp(nu, u), mp.diff(lambda v: R.rho_mp(v, mp.mpf(u)), mp.mpf(nu))


@pytest.fixture(scope="module")
def drho(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("matern_d") / "matern_drho_check")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", os.path.join(HERE, "host", "matern_drho_check.cpp"),
                    "-o", exe, "-lm"], check=True)

    def run(mode, pairs):
        inp = "\n".join(f"{mode} {float(nu)!r} {float(u)!r}" for nu, u in pairs) + "\n"
        out = subprocess.run([exe], input=inp, check=True, capture_output=True, text=True).stdout.strip().split("\n")
        assert len(out) == len(pairs)
        rows = [r.split() for r in out]
        return [(float.fromhex(r[0]), float.fromhex(r[1]), int(r[2]), int(r[3])) for r in rows]

    return run


def _worst(run, mode, pairs):
    got = run(mode, pairs)
    wh = wn = 0.0
    for (nu, u), g in zip(pairs, got):
        h, n = ref_hn(nu, u)
        wh, wn = max(wh, float(abs(g[0] - h))), max(wn, float(abs(g[1] - n)))
    return wh, wn


def test_evaluators_vs_mpmath(drho):
    """nngp_matern_drho on test_matern.py's grid for rho, plus nu in {0.05, 1, 2, 50} and u in {1e-9, 40}."""
    rng = np.random.default_rng(3)
    pairs = []
    for nu in EVAL_NUS:
        us = list(10 ** rng.uniform(-8, 1.3, 12)) + [1e-150, 1e-30, 1e-9, 1e-3, 1.4999, 1.5, 1.5001, 2.0, 40.0, 300.0,
                                                     700.0]
        pairs += [(nu, u) for u in us]
    wh, wn = _worst(drho, "e", pairs)
    print("evaluator worst |dh|, |dn|:", wh, wn)
    assert wh <= BOUND_EVAL_H and wn <= BOUND_EVAL_N, (wh, wn)


def test_table_fit_vs_mpmath(drho):
    """The fitted derivative table (nngp_matern_tab_d) at random t inside the table, at both ends, and below the
    table for a series nu (0.3)."""
    rng = np.random.default_rng(9)
    pairs = []
    for nu in (0.05, 0.3, 0.5, 1.0, 1.3, 2.5, 7.3, 20.3, 50.0):
        us = list(10 ** rng.uniform(-8, 1.3, 25)) + [1e-3, 0.7, 1.5, 40.0, 300.0]
        pairs += [(nu, u) for u in us]
        e0, noct = drho("t", [(nu, 1.0)])[0][2:]
        # the table's first and last fitted octaves, and just outside both
        for e in (e0 - 0.5, e0 + 0.01, e0 + 0.99, e0 + noct - 2.01, e0 + noct - 1.5):
            pairs.append((nu, 2.0 ** (0.5 * e)))
    pairs += [(0.3, 2.0 ** -e) for e in (32.01, 33, 40, 60, 100, 200)] + [(0.3, 1e-12)]
    wh, wn = _worst(drho, "t", pairs)
    print("table worst |dh|, |dn|:", wh, wn)
    assert wh <= BOUND_TAB_H and wn <= BOUND_TAB_N, (wh, wn)


def test_outside_the_table_is_negligible(drho):
    """|h| and |n| just outside the table (where the end octaves hold 0) are below what a gradient needs:
    O(nu 1e-18) and O(1e-18 |ln t|) below it, under 1e-15 above it."""
    for nu in (0.95, 1.0, 1.3, 2.5, 7.3, 50.0):
        e0, noct = drho("t", [(nu, 1.0)])[0][2:]
        lo, hi = 2.0 ** (0.5 * (e0 - 1)), 2.0 ** (0.5 * (e0 + noct - 2))
        for u in (lo, hi):
            h, n = ref_hn(nu, u)
            print(nu, u, float(h), float(n))
            assert abs(h) <= 1e-15 and abs(n) <= 1e-15, (nu, u, h, n)


def test_limits_and_closed_forms(drho):
    """h(0) = n(0) = 0 exactly, from the evaluator and the table (coincident points, the floor 2^-1000), for a
    series nu and a plain one; h against the closed forms at nu = 1/2, 3/2, 5/2 to 4 ulp of the bracket."""
    for mode in "et":
        for nu in (0.3, 1.3, 50.0):
            g = drho(mode, [(nu, 0.0)])[0]
            assert g[0] == 0.0 and g[1] == 0.0, (mode, nu, g)
    us = [1e-12, 1e-4, 0.03, 0.4, 1.0, 1.49, 1.51, 3.0, 11.0, 40.0]
    forms = {0.5: lambda u: -u, 1.5: lambda u: -u * u, 2.5: lambda u: -(u * u / 3) * (1 + u)}
    for nu, br in forms.items():
        got = drho("e", [(nu, u) for u in us])
        for u, g in zip(us, got):
            ul = np.longdouble(u)
            exact = float(br(ul) * np.exp(-ul))
            assert abs(g[0] - exact) <= 4 * np.spacing(abs(float(br(ul)))), (nu, u, g[0], exact)


def test_reference_quadrature_vs_mpmath():
    """The restatement's longdouble quadrature for n(u) agrees with mp.diff to 1e-16 absolute."""
    u = 10 ** np.random.default_rng(0).uniform(-6, 1.5, 40)
    for nu in R.PARITY_NUS + (0.5, 7.3):
        a = R.dnu_quad(nu, u)
        b = np.array([R.dnu_mp(nu, x) for x in u])
        assert np.abs(a - b).max() <= 1e-16, (nu, np.abs(a - b).max())


def test_reference_gradient_vs_mpmath_dense_gp():
    """N = 12, m = 11: the NNGP density is the exact Gaussian density, whose gradient in (sigma2, phi, tau2, nu)
    mpmath gives by differentiating the dense log-density."""
    coords, y = R.field(12, seed=5)
    th = (1.3, 4.0, 0.05, 1.3)
    nbr = np.array([[j if j < i else -1 for j in range(11)] for i in range(12)], dtype=np.int32)
    g = R.ref_rows_matern(coords, nbr, th, y, dnu="mp")[:, 2:].sum(0)
    d = np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(-1))

    def ll(s2, phi, t2, nu):
        K = mp.matrix(12, 12)
        for a in range(12):
            for b in range(12):
                K[a, b] = s2 * (R.rho_mp(nu, phi * mp.mpf(d[a, b])) if a != b else 1) + (t2 if a == b else 0)
        yv = mp.matrix([mp.mpf(v) for v in y])
        return -0.5 * (mp.log(mp.det(K)) + (yv.T * mp.lu_solve(K, yv))[0])

    with mp.workdps(40):
        for p in range(4):
            f = lambda x, p=p: ll(*[x if k == p else mp.mpf(th[k]) for k in range(4)])
            gd = float(mp.diff(f, mp.mpf(th[p])))
            assert abs(g[p] - gd) <= 1e-9 * (1 + abs(gd)), (p, g[p], gd)


@pytest.mark.skipif(np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps, reason="no extended precision here")
def test_restatement_against_longdouble_twin():
    """Conditions the GPU parity tolerance: on the parity inputs the fp64 restatement sits within 1e-11 (1 + |G|)
    of its longdouble twin in every component, the nu component included (measured: below 2e-12), so the GPU rows
    get the 1e-9 (1 + |G|) of test_gpu_grad.py, the same multiple, in all four."""
    coords, y = R.field(R.PARITY_N, seed=R.PARITY_SEED)
    worst = 0.0
    for nu in R.PARITY_NUS:
        th = R.parity_theta(nu)
        T = R.pair_tables(coords, th)
        for m in (1, 15, 32):
            nbr = R.prior_nbr(coords, m)
            rows = range(0, R.PARITY_N, 5)
            r64 = R.ref_rows_matern(coords, nbr, th, y, rows=rows, tables=T)[:, 2:]
            rld = R.ref_rows_matern(coords, nbr, th, y, rows=rows, tables=T, dtype=np.longdouble)[:, 2:]
            err = np.max(np.abs(r64 - rld) / (1 + np.abs(rld)), axis=0).astype(np.float64)
            print(nu, m, "fp64 vs longdouble per component:", err)
            worst = max(worst, float(err.max()))
    assert worst <= 1e-11, worst


# ---------------------------------------------------------------- refusals without a GPU
def _lib():
    from pynngp_amd import _lib

    return _lib, _lib.load()


def test_capi_refusals():
    _l, lib = _lib()
    EINVAL, EUNSUP = -1, -4  # include/nngp.h
    assert lib.nngp_bf_grad_matern_workspace_bytes(100, 0) == 0
    assert lib.nngp_bf_grad_matern_workspace_bytes(100, 33) == 0
    assert lib.nngp_bf_grad_matern_workspace_bytes(-1, 10) == 0
    need = lib.nngp_bf_grad_matern_workspace_bytes(100, 10)
    assert need >= 3 * 160 * 640 and need % 256 == 0
    buf = (ctypes.c_double * 64)()
    nb = (ctypes.c_int32 * 64)()
    ws = ctypes.c_void_p(1 << 20)  # 256-byte aligned; every case below is refused before it is touched
    p = ctypes.addressof

    def call(dim=2, m=4, s2=1.0, phi=2.0, t2=0.1, nu=1.3, values=True, wsb=None, n_rows=8):
        return lib.nngp_bf_grad_matern(p(buf), 8, dim, p(nb), None, n_rows, m, 0, s2, phi, t2, nu,
                                       p(buf) if values else None, None, p(buf), p(buf), ws,
                                       need if wsb is None else wsb, None)

    for m in (0, 33, -1):
        assert call(m=m) == EUNSUP, m
    for dim in (0, 4):
        assert call(dim=dim) == EUNSUP, dim
    for nu in (0.0, -1.0, 50.5, float("nan"), float("inf")):
        assert call(nu=nu) == EINVAL, nu
    assert call(s2=0.0) == EINVAL and call(s2=-1.0) == EINVAL
    assert call(phi=0.0) == EINVAL and call(phi=float("inf")) == EINVAL
    assert call(t2=-1e-3) == EINVAL
    assert call(values=False) == EINVAL
    assert call(wsb=need - 256) == EINVAL
    assert call(n_rows=9) == EINVAL  # rows outside the points
    assert lib.nngp_matern_eval_d(p(buf), 4, 0.0, p(buf), p(buf), None) == EINVAL
    assert lib.nngp_matern_eval_d(p(buf), 4, 51.0, p(buf), p(buf), None) == EINVAL
    assert lib.nngp_matern_eval_d(None, 4, 1.3, p(buf), p(buf), None) == EINVAL
    assert lib.nngp_matern_eval_d(p(buf), -1, 1.3, p(buf), p(buf), None) == EINVAL


def test_python_refusals():
    import torch

    import pynngp_amd
    from pynngp_amd import MaternCovariance, load_ops

    for bad in (None, 0.0, -1.0, 51.0):
        with pytest.raises(ValueError, match="nu"):
            MaternCovariance(1.0, 2.0, 0.0, bad)
    cv = MaternCovariance(1.0, 8.0, 0.1, 1.3)
    assert cv.kind == "matern" and cv.theta == (1.0, 8.0, 0.1, 1.3) and cv.nu_arg == 1.3
    assert isinstance(cv, pynngp_amd.Covariance) and cv.replace(nu=2.0).theta == (1.0, 8.0, 0.1, 2.0)
    load_ops()
    c = torch.zeros((50, 2), dtype=torch.float64)
    with pytest.raises(NotImplementedError):
        torch.ops.nngp.bf_grad_matern(c, torch.zeros((50, 4), dtype=torch.int32), None, 0, 1.0, 5.0, 0.0, 1.3,
                                      torch.zeros(50, dtype=torch.float64), False)
    with pytest.raises(NotImplementedError):
        torch.ops.nngp.matern_eval_d(torch.zeros(5, dtype=torch.float64), 1.3)
    from pynngp_amd import _lib

    with pytest.raises(_lib.NNGPExtensionError):
        _lib.matern_eval_d(torch.zeros(5, dtype=torch.float64), 1.3)
    with pytest.raises(ValueError, match="theta"):
        pynngp_amd.loglik_matern(c, torch.zeros((50, 4), dtype=torch.int32), torch.ones(3, dtype=torch.float64),
                                 torch.zeros(50, dtype=torch.float64))


def test_fit_estimate_nu_refusals():
    """estimate_nu with reml, anisotropic, method='fisher' or stderr raises before anything runs."""
    from pynngp_amd.nngp import NNGP

    model = object.__new__(NNGP)  # fit() refuses these combinations before it touches the model
    for kw, name in (({"reml": True}, "reml"), ({"anisotropic": True}, "anisotropic"),
                     ({"method": "fisher"}, "fisher"), ({"stderr": True}, "stderr")):
        for est in (True, False):
            with pytest.raises(NotImplementedError, match=name):
                model.fit(kind="matern", nu=0.8, estimate_nu=est, **kw)
