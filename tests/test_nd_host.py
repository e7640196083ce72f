"""CPU: the 4 .. 16-dimensional path without a GPU -- the C entry points' refusals through ctypes, ARDCovariance,
the NotImplementedError scope of an NNGPnd, the conditioning of the GPU tests' tolerances on exactly their inputs,
the reference gradient against central differences, and nd_host.h under AddressSanitizer and UBSan in a stand-alone
program (tests/host/nd_check.cpp; never loaded into Python)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import bf_precision_ref as P
import nd_ref as R
from grad_aniso_ref import ref_rows_aniso

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL, EUNSUP = -1, -4


@pytest.fixture(scope="module")
def lib():
    from pynngp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build()")
    return _lib.load()


def _buf(n=4096):
    raw = ctypes.create_string_buffer(n + 256)
    addr = (ctypes.addressof(raw) + 255) & ~255
    return raw, ctypes.c_void_p(addr)


def _sweep(lib, dim=8, m=15, kind=0, sigma2=1.0, phi=None, tau2=0.1, coords=True, ws=True, partials=True, which="sweep"):
    """One call that must stop at the argument checks (host pointers: nothing may be launched)."""
    raw, w = _buf()
    c = (ctypes.c_double * 64)()
    nbr = (ctypes.c_int32 * 32)(*([-1] * 32))
    p = (ctypes.c_double * 4)()
    ph = (ctypes.c_double * 16)(*([1.0] * 16)) if phi is None else phi
    cp = ctypes.cast(c, ctypes.c_void_p) if coords else None
    wp = w if ws else None
    pp = ctypes.cast(p, ctypes.c_void_p) if partials else None
    nb = ctypes.cast(nbr, ctypes.c_void_p)
    if which == "sweep":
        return lib.nngp_bf_sweep_nd(cp, 2, dim, nb, None, 1, m, 0, kind, sigma2, ph, tau2, None, None, None, None, pp, wp,
                                    4096, None)
    if which == "cross":
        return lib.nngp_bf_cross_nd(cp, 2, dim, cp, 2, nb, None, 1, m, 0, kind, sigma2, ph, tau2, None, None, None, None,
                                    None, pp, wp, 4096, None)
    g = (ctypes.c_double * 18)()
    return lib.nngp_bf_grad_nd(cp, 2, dim, nb, None, 1, m, 0, kind, sigma2, ph, tau2, cp, None, pp,
                               ctypes.cast(g, ctypes.c_void_p), wp, 4096, None)


@pytest.mark.parametrize("which", ["sweep", "cross", "grad"])
def test_sweep_entry_points_refuse(lib, which):
    def phi_with(bad):
        a = (ctypes.c_double * 8)(*([1.0] * 8))
        a[5] = bad
        return a

    for dim in (3, 17, 0):
        assert _sweep(lib, dim=dim, which=which) == EUNSUP
        assert b"dim" in lib.nngp_last_error()
    for m in (0, 33):
        assert _sweep(lib, m=m, which=which) == EUNSUP
    assert _sweep(lib, kind=4, which=which) == EUNSUP
    assert b"positive definite above three dimensions" in lib.nngp_last_error()
    assert _sweep(lib, kind=5, which=which) == EUNSUP
    assert _sweep(lib, kind=7, which=which) == EINVAL
    for kw in (dict(coords=False), dict(ws=False), dict(partials=False), dict(phi=ctypes.c_void_p(None)),
               dict(sigma2=0.0), dict(sigma2=float("nan")), dict(sigma2=float("inf")), dict(tau2=-1.0),
               dict(tau2=float("nan")), dict(phi=phi_with(0.0)), dict(phi=phi_with(-2.0)),
               dict(phi=phi_with(float("nan"))), dict(phi=phi_with(float("inf")))):
        assert _sweep(lib, which=which, **kw) == EINVAL, kw


def test_knn_entry_points_refuse(lib):
    raw, w = _buf()
    c = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)
    out = ctypes.cast((ctypes.c_int32 * 64)(), ctypes.c_void_p)
    for dim in (3, 17):
        assert lib.nngp_knn_prior_nd(c, 2, dim, 5, 0, 2, out, w, 4096, None) == EUNSUP
        assert lib.nngp_knn_query_nd(c, 2, dim, c, 2, 5, out, w, 4096, None) == EUNSUP
        assert lib.nngp_knn_nd_workspace_bytes(2, dim, 5) == 0
    assert lib.nngp_knn_prior_nd(c, 2, 8, 33, 0, 2, out, w, 4096, None) == EUNSUP
    assert lib.nngp_knn_prior_nd(None, 2, 8, 5, 0, 2, out, w, 4096, None) == EINVAL
    assert lib.nngp_knn_prior_nd(c, 2, 8, 5, 0, 2, out, None, 4096, None) == EINVAL
    assert lib.nngp_knn_prior_nd(c, 2, 8, 5, 0, 2, None, w, 4096, None) == EINVAL
    assert lib.nngp_knn_prior_nd(c, 2, 8, 5, 1, 3, out, w, 4096, None) == EINVAL
    assert lib.nngp_knn_query_nd(c, 2, 8, None, 2, 5, out, w, 4096, None) == EINVAL
    assert lib.nngp_knn_nd_workspace_bytes(100, 8, 15) == 256
    # the 1 .. 3-dimensional entry points keep refusing four columns
    assert lib.nngp_knn_workspace_bytes(100, 4, 15) == 0


def test_workspace_sizes(lib):
    from pynngp_amd import _lib

    assert _lib.ND_MAX_DIM == 16 and _lib.ND_MIN_DIM == _lib.MAX_DIM + 1 == 4
    assert lib.nngp_bf_sweep_nd_workspace_bytes(1000, 15, 3) == 0
    assert lib.nngp_bf_sweep_nd_workspace_bytes(1000, 15, 17) == 0
    assert lib.nngp_bf_sweep_nd_workspace_bytes(1000, 33, 8) == 0
    blocks = (1000 * 4 + 255) // 256
    assert lib.nngp_bf_sweep_nd_workspace_bytes(1000, 15, 8) == (blocks * 14 * 8 + 255) // 256 * 256
    assert lib.nngp_bf_sweep_nd_workspace_bytes(0, 15, 8) == 256


def test_ard_covariance():
    from pynngp_amd import ARDCovariance, Covariance

    c = ARDCovariance("matern32", 1.5, [0.5, 1.0, 2.0, 4.0, 8.0], 0.1)
    assert c.dim == 5 and c.theta == (1.5, 0.5, 1.0, 2.0, 4.0, 8.0, 0.1)
    assert c.replace(tau2=0.0).tau2 == 0.0 and c.replace(phi=(1.0,) * 6).dim == 6
    rng = np.random.default_rng(0)
    a, b = rng.uniform(size=(3, 5)), rng.uniform(size=(4, 5))
    s = np.array(c.phi)
    want = Covariance("matern32", 1.5, 1.0, 0.0)(a * s, b * s)
    assert np.array_equal(c(a, b), want) and c(a, b).shape == (3, 4)
    with pytest.raises(ValueError, match="AnisotropicCovariance"):
        ARDCovariance("exponential", 1.0, (1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match="4 .. 16"):
        ARDCovariance("exponential", 1.0, (1.0,) * 17)
    with pytest.raises(ValueError, match="spherical"):
        ARDCovariance("spherical", 1.0, (1.0,) * 4)
    with pytest.raises(ValueError, match="kinds"):
        ARDCovariance("matern", 1.0, (1.0,) * 4)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="positive and finite"):
            ARDCovariance("exponential", 1.0, (1.0, 1.0, bad, 1.0))
    with pytest.raises(ValueError):
        ARDCovariance("exponential", 0.0, (1.0,) * 4)
    with pytest.raises(ValueError):
        ARDCovariance("exponential", 1.0, (1.0,) * 4, -0.1)
    with pytest.raises(ValueError, match="rows must have 4 columns"):
        ARDCovariance("exponential", 1.0, (1.0,) * 4)(a, b)


def test_scope_without_a_gpu():
    """What an NNGP over four or more columns refuses, checked before any GPU work."""
    import pynngp_amd as A
    from pynngp_amd import nd

    t, y = np.random.default_rng(0).uniform(size=(20, 5)), np.zeros(20)
    cov = A.ARDCovariance("exponential", 1.0, (1.0,) * 5, 0.1)
    with pytest.raises(NotImplementedError, match="refType"):
        A.NNGP(t, y, None, ("subset", 5), 3, cov)
    with pytest.raises(NotImplementedError, match="maxmin"):
        A.NNGP(t, y, None, "S=T", 3, cov, ordering="maxmin")
    with pytest.raises(NotImplementedError, match="positive definite"):
        A.NNGP(t, y, None, "S=T", 3, A.Covariance("spherical", 1.0, 1.0, 0.1))
    with pytest.raises(NotImplementedError, match="matern"):
        A.NNGP(t, y, None, "S=T", 3, A.MaternCovariance(1.0, 1.0, 0.1, 0.7))
    with pytest.raises(NotImplementedError, match="SeparableCovariance"):
        A.NNGP(t, y, None, "S=T", 3, A.SeparableCovariance("exponential", "exponential", 1.0, 1.0, 1.0, 0.1))
    with pytest.raises(NotImplementedError, match="m=40"):
        A.NNGP(t, y, None, "S=T", 40, cov)
    with pytest.raises(ValueError, match="5-dimensional"):
        A.NNGP(t, y, None, "S=T", 3, A.ARDCovariance("exponential", 1.0, (1.0,) * 4))
    with pytest.raises(ValueError, match="NaN or infinity"):
        A.NNGP(np.full((20, 5), np.nan), y, None, "S=T", 3, cov)
    # seventeen columns are nobody's
    with pytest.raises(Exception, match="ROCm GPU|1 <= d <= 3"):
        A.NNGP(np.zeros((20, 17)), y, None, "S=T", 3, cov)
    # the methods outside the scope, on an instance that never saw a GPU
    inst = object.__new__(nd.NNGPnd)
    for name in ("gls", "conjugate", "conjugate_grid", "fisher_information", "latent_posterior", "latent_loglik",
                 "latent_fit", "latent_mean", "latent_sample", "latent_sd", "prior_factor", "simulate", "oneSample",
                 "set_neighbor_sets"):
        with pytest.raises(NotImplementedError, match="4 .. 16 coordinate columns"):
            getattr(inst, name)()
    inst.cov, inst.m = cov, 3
    for call in (lambda: inst.loglik(noise="eps"), lambda: inst.loglik_grad(noise="eps"),
                 lambda: inst.profile_loglik(cov, mean="linear", X=np.ones((20, 1))),
                 lambda: inst.profile_loglik_grad(cov, mean="linear"), lambda: inst.predict(X=1, X_query=1),
                 lambda: inst.predict(noise="eps"), lambda: inst.fit(mean="linear"), lambda: inst.fit(stderr=True),
                 lambda: inst.fit(method_opts=None, estimate_nu=True)):
        with pytest.raises(NotImplementedError, match="4 .. 16 coordinate columns"):
            call()
    assert A.NNGPnd is nd.NNGPnd and issubclass(nd.NNGPnd, A.NNGP)


def test_loglik_ard_checks():
    import torch

    import pynngp_amd as A

    c, nbr = torch.zeros((10, 5), dtype=torch.float64), torch.zeros((10, 3), dtype=torch.int32)
    th, v = torch.ones(7, dtype=torch.float64), torch.zeros(10, dtype=torch.float64)
    with pytest.raises(NotImplementedError):
        A.loglik_ard(c, nbr, "spherical", th, v)
    with pytest.raises(NotImplementedError):
        A.loglik_ard(c[:, :3], nbr, "exponential", th, v)
    with pytest.raises(ValueError):
        A.loglik_ard(c, nbr, "exponential", th[:5], v)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("dim", R.DIMS)
def test_inputs_keep_correlations_inside(dim, kind):
    """The decays keep the neighbour correlations well away from 0 and 1 (the issue's rule for the inputs)."""
    rho = R.neighbour_correlations(dim, kind)
    assert 0.02 < np.median(rho) < 0.98 and np.quantile(rho, 0.1) > 1e-3 and np.quantile(rho, 0.9) < 0.999, \
        (np.median(rho), np.quantile(rho, [0.1, 0.9]))
    ph = np.array(R.phis(dim, kind))
    assert len(set(ph)) > 3 and ph.max() >= 10 * ph.min() * (1 - 1e-12)  # unequal, one of them 10x the smallest


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("dim,m", [(4, 32), (8, 15), (16, 32), (16, 8)])
def test_forward_tolerance_is_conditioned(dim, kind, m):
    """The fp64 restatement against the long-double reference, in bf_precision_ref's scales, on the GPU tests' inputs:
    below BF_K / 8 for B, F and R."""
    ref = R.prior_reference(dim, kind, m)
    B, F, Rr = R.fp64_sweep(dim, kind, m)
    got = P.ratios(ref, B, F, Rr)
    print(dim, kind, m, got, int(ref.resolved.sum()))
    assert ref.resolved.mean() >= P.RESOLVED_SHARE
    assert max(got) < P.BF_K / 8.0, got


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("dim,m", [(4, 32), (8, 15), (16, 24)])
def test_gradient_tolerance_is_conditioned(dim, kind, m):
    """ref_rows_aniso in fp64 against its long-double twin on the GPU tests' inputs and rows: below 1/8 of
    1e-9 (1 + |G|)."""
    lo, hi = R.grad_rows(dim, kind, m), R.grad_rows(dim, kind, m, True)
    err = np.abs(lo[:, 2:] - hi[:, 2:].astype(np.float64)) / (1.0 + np.abs(lo[:, 2:]))
    print(dim, kind, m, err.max())
    assert err.max() < 1e-9 / 8.0


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_gradient_matches_central_differences(kind):
    rng = np.random.default_rng(5)
    n, dim, m = 60, 5, 6
    from oracle import nngp_oracle as O

    c, y = rng.uniform(size=(n, dim)), rng.standard_normal(n)
    th = np.array((1.3, 0.9, 3.0, 0.5, 1.4, 0.7, 0.05))
    nbr = O.knn_prior(c * th[1:-1], m).astype(np.int32)

    def ll(t):
        r = ref_rows_aniso(c, nbr, kind, tuple(t), y)
        return -0.5 * (r[:, 0].sum() + r[:, 1].sum())

    g = ref_rows_aniso(c, nbr, kind, tuple(th), y)[:, 2:].sum(0)
    for k in range(dim + 2):
        h = 1e-5 * th[k]
        e = np.zeros_like(th)
        e[k] = h
        fd = (ll(th + e) - ll(th - e)) / (2 * h)
        assert abs(fd - g[k]) <= 1e-6 * (1.0 + abs(g[k])), (k, fd, g[k])


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_host_checks_under_sanitizers(tmp_path, lib):
    """nd_host.h (workspace size and argument checks) in a stand-alone program built with
    -fsanitize=address,undefined; the size it prints is the library's."""
    exe = tmp_path / "nd_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "pynngp_amd", "csrc"), os.path.join(HERE, "host", "nd_check.cpp"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out[0] == "ok" and int(out[1]) == lib.nngp_bf_sweep_nd_workspace_bytes(1000, 15, 8)
