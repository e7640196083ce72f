"""Per-axis gradient sweep (nngp_bf_grad_aniso), host side (no GPU): the numpy restatement of grad_aniso_ref.py pinned
by the dense GP's gradient, by central differences of the oracle on scaled coordinates and by Euler's identity against
the isotropic restatement; its fp64 error on the GPU parity test's inputs; the C entry points' refusals before any
HIP call; AnisotropicCovariance's validation and the refusals of everything that does not serve it."""
import numpy as np
import pytest
import torch

from grad_aniso_ref import KINDS, PARITY_SEED, field, parity_theta, ref_rows_aniso
from oracle import nngp_oracle as O
from pynngp_amd import _lib
from pynngp_amd import nngp as N
from test_gpu_grad import ref_rows, rho_drho


# ---------------------------------------------------------------- the restatement
def dense_grad_aniso(coords, kind, theta, y):
    s2, t2 = theta[0], theta[-1]
    phi = np.array(theta[1:-1])
    n = len(y)
    X = coords * phi
    delta2 = (X[:, None, :] - X[None, :, :]) ** 2
    u = np.sqrt(delta2.sum(-1))
    r_, dr_ = rho_drho(kind, u)
    K = s2 * r_ + t2 * np.eye(n)
    Ki = np.linalg.inv(K)
    al = Ki @ y
    w = np.where(u > 0, s2 * dr_ / np.where(u > 0, u, 1.0), 0.0)
    dKs = [r_] + [w * delta2[:, :, k] / phi[k] for k in range(len(phi))] + [np.eye(n)]
    return np.array([0.5 * al @ dK @ al - 0.5 * np.trace(Ki @ dK) for dK in dKs])


THETAS = {2: (1.3, 3.0, 9.0, 0.05), 3: (1.3, 3.0, 9.0, 0.7, 0.05)}


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_dense(kind, dim):
    coords, y = field(40, dim=dim, seed=3)
    th = parity_theta(kind, THETAS[dim][1:-1])
    full = np.array([[j if j < i else -1 for j in range(39)] for i in range(40)], dtype=np.int32)
    g = ref_rows_aniso(coords, full, kind, th, y)[:, 2:].sum(0)
    gd = dense_grad_aniso(coords, kind, th, y)
    assert np.allclose(g, gd, rtol=1e-8, atol=1e-8), (g, gd)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_central_differences(kind, dim):
    """The oracle is the isotropic one, evaluated at phi = 1 on the scaled coordinates."""
    coords, y = field(40, dim=dim, seed=3)
    th = parity_theta(kind, THETAS[dim][1:-1])
    nbr = O.c_knn_prior(coords * np.array(th[1:-1]), 10)
    g = ref_rows_aniso(coords, nbr, kind, th, y)[:, 2:].sum(0)

    def ll(t):
        return O.nngp_loglik(coords * np.array(t[1:-1]), nbr, kind, (t[0], 1.0, t[-1]), y)

    for p in range(dim + 2):
        h = 1e-6 * th[p]
        tp, tm = list(th), list(th)
        tp[p] += h
        tm[p] -= h
        fd = (ll(tp) - ll(tm)) / (2 * h)
        assert abs(fd - g[p]) <= 1e-6 * max(1.0, abs(g[p])), (kind, p, fd, g[p])


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_euler_identity(kind, dim):
    """With all phi_k = phi the model is the isotropic one: sum_k phi_k g_k = phi g_phi on every row, and the
    sigma2 / tau2 entries and the two sums are the isotropic restatement's.  Relative as everywhere in the rows'
    tests: |difference| <= 1e-12 (1 + |value|) (a row's gradient is a difference of terms of order 1, so its own
    size is no scale for its rounding)."""
    coords, y = field(60, dim=dim, seed=4)
    phi = 1.7 if kind == "spherical" else 6.0
    nbr = O.c_knn_prior(coords, 10)
    iso = ref_rows(coords, nbr, kind, (1.3, phi, 0.05), y)
    an = ref_rows_aniso(coords, nbr, kind, (1.3,) + (phi,) * dim + (0.05,), y)
    lhs = phi * an[:, 3:3 + dim].sum(1)
    rhs = phi * iso[:, 3]
    err = np.abs(lhs - rhs) / (1 + np.abs(rhs))
    print(kind, dim, "Euler:", err.max())
    assert err.max() <= 1e-12
    for a, b in ((an[:, 0], iso[:, 0]), (an[:, 1], iso[:, 1]), (an[:, 2], iso[:, 2]), (an[:, 3 + dim], iso[:, 4])):
        assert np.all(np.abs(a - b) <= 1e-12 * (1 + np.abs(b)))


def parity_cases():
    """(kind, dim, theta, m list): the inputs of test_gpu_grad_aniso.py's per-row parity tests."""
    every = list(range(1, 33))
    some = [10, 17, 24, 32]
    out = [(k, 2, parity_theta(k), every) for k in ("exponential", "matern52")]
    out += [(k, 2, parity_theta(k), some) for k in ("matern32", "gaussian", "spherical")]
    out += [("spherical", 2, (1.3, 3.0, 9.0, 0.05), some)]  # ranges 1/3 and 1/9: many pairs beyond u = 1
    out += [(k, 1, (1.3, 5.0, 0.05), some) for k in ("exponential", "matern52")]
    out += [(k, 3, (1.3, 3.0, 9.0, 0.7, 0.05), some) for k in ("exponential", "matern52")]
    return out


@pytest.mark.skipif(np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps, reason="no extended precision here")
@pytest.mark.parametrize("case", parity_cases(), ids=lambda c: f"{c[0]}-d{c[1]}-{len(c[3])}m-{c[2][1]}")
def test_restatement_against_longdouble_twin(case):
    """The GPU test's 1e-9 (1 + |G|) parity tolerance is a condition on the inputs: for every m of that test the fp64
    restatement must sit within 1e-11 (1 + |G|) of its longdouble twin on the same inputs."""
    kind, dim, th, ms = case
    coords, y = field(96, dim=dim, seed=PARITY_SEED)
    for m in ms:
        nbr = O.c_knn_prior(coords * np.array(th[1:-1]), m)
        r64 = ref_rows_aniso(coords, nbr, kind, th, y)[:, 2:]
        rld = ref_rows_aniso(coords, nbr, kind, th, y, dtype=np.longdouble)[:, 2:]
        err = float(np.max(np.abs(r64 - rld) / (1 + np.abs(rld))))
        print(kind, dim, m, "fp64 vs longdouble:", err)
        assert err <= 1e-11, (kind, dim, m, err)


# ---------------------------------------------------------------- C ABI refusals (fake addresses, never dereferenced)
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _codes():
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nngp.h")).read()
    out = {}
    for name in ("NNGP_OK", "NNGP_EINVAL", "NNGP_EUNSUP"):
        mm = re.search(r"#define\s+" + name + r"\s+\(?(-?\d+)", hdr)
        assert mm, name
        out[name] = int(mm.group(1))
    return out


_DEFAULT = object()


def _call(lib, *, coords=256, n_points=100, dim=2, nbr=512, order=None, n_rows=100, m=10, i0=0, kind=0, sigma2=1.0,
          phi=_DEFAULT, tau2=0.1, values=768, G=None, partials=1024, grad=1280, workspace=4096, ws_bytes=None):
    import ctypes

    if ws_bytes is None:
        ws_bytes = lib.nngp_bf_grad_aniso_workspace_bytes(n_rows, m, dim) or 4096
    if phi is _DEFAULT:
        phi = (3.0, 9.0, 0.7)[:max(1, min(dim, 3))]
    phi_host = None if phi is None else (ctypes.c_double * len(phi))(*phi)
    return lib.nngp_bf_grad_aniso(coords, n_points, dim, nbr, order, n_rows, m, i0, kind, sigma2, phi_host, tau2,
                                  values, G, partials, grad, workspace, ws_bytes, None)


def test_workspace_bytes(lib):
    prev = 0
    for n in (0, 1, 63, 64, 65, 1000, 10**6, 10**7):
        for m in (1, 8, 9, 32):
            for dim in (1, 2, 3):
                assert lib.nngp_bf_grad_aniso_workspace_bytes(n, m, dim) % 256 == 0
        b = lib.nngp_bf_grad_aniso_workspace_bytes(n, 15, 2)
        assert b >= prev and b > 0
        prev = b
    for m in (0, 33, -1):
        assert lib.nngp_bf_grad_aniso_workspace_bytes(100, m, 2) == 0
    for dim in (0, 4):
        assert lib.nngp_bf_grad_aniso_workspace_bytes(100, 10, dim) == 0
    assert lib.nngp_bf_grad_aniso_workspace_bytes(-1, 10, 2) == 0


def test_unsupported(lib):
    c = _codes()
    assert _call(lib, kind=5) == c["NNGP_EUNSUP"]
    assert b"matern" in lib.nngp_last_error()
    assert _call(lib, m=0, ws_bytes=4096) == c["NNGP_EUNSUP"]
    assert _call(lib, m=33, ws_bytes=4096) == c["NNGP_EUNSUP"]
    assert _call(lib, dim=0) == c["NNGP_EUNSUP"]
    assert _call(lib, dim=4, phi=(1.0, 1.0, 1.0, 1.0)) == c["NNGP_EUNSUP"]


@pytest.mark.parametrize("kw", [
    dict(phi=None), dict(phi=(3.0, 0.0)), dict(phi=(-1.0, 9.0)), dict(phi=(3.0, float("nan"))),
    dict(phi=(float("inf"), 9.0)), dict(dim=3, phi=(3.0, 9.0, 0.0)), dict(dim=1, phi=(0.0,)),
    dict(values=None), dict(partials=None), dict(grad=None), dict(coords=None), dict(workspace=None), dict(nbr=None),
    dict(ws_bytes=255), dict(workspace=4097), dict(kind=-1), dict(kind=6), dict(n_rows=-1, ws_bytes=4096),
    dict(i0=-1), dict(i0=1), dict(n_points=0), dict(sigma2=0.0), dict(tau2=-0.1), dict(sigma2=float("nan")),
    dict(tau2=float("inf")),
])
def test_invalid(lib, kw):
    assert _call(lib, **kw) == _codes()["NNGP_EINVAL"], lib.nngp_last_error()


def test_short_workspace(lib):
    need = lib.nngp_bf_grad_aniso_workspace_bytes(10**6, 15, 2)
    assert need > 256
    assert _call(lib, n_points=10**6, n_rows=10**6, m=15, ws_bytes=need - 1) == _codes()["NNGP_EINVAL"]
    assert b"workspace" in lib.nngp_last_error()


def test_python_refusals():
    c = torch.zeros((40, 2), dtype=torch.float64)
    v = torch.zeros(40, dtype=torch.float64)
    nbr = torch.zeros((40, 5), dtype=torch.int32)
    with pytest.raises(ValueError):
        _lib.bf_grad_aniso(c, nbr, 0, "exponential", 1.0, (3.0, 9.0), 0.1, None)
    with pytest.raises(ValueError):
        _lib.bf_grad_aniso(c, nbr, 0, "exponential", 1.0, (3.0,), 0.1, v)
    with pytest.raises(ValueError):
        _lib.bf_grad_aniso(c, nbr, 0, "exponential", 1.0, (3.0, -9.0), 0.1, v)
    with pytest.raises(NotImplementedError):
        _lib.bf_grad_aniso(c, torch.zeros((40, 33), dtype=torch.int32), 0, "exponential", 1.0, (3.0, 9.0), 0.1, v)
    with pytest.raises(NotImplementedError):
        _lib.bf_grad_aniso(c, nbr, 0, "matern", 1.0, (3.0, 9.0), 0.1, v)
    with pytest.raises(_lib.NNGPExtensionError):  # CPU tensors: no fallback
        _lib.bf_grad_aniso(c, nbr, 0, "exponential", 1.0, (3.0, 9.0), 0.1, v)


# ---------------------------------------------------------------- AnisotropicCovariance
def test_anisotropic_covariance_validation():
    import pynngp_amd

    assert pynngp_amd.AnisotropicCovariance is N.AnisotropicCovariance
    cv = N.AnisotropicCovariance("matern32", 1.3, [3, 9], 0.05)
    assert cv.phi == (3.0, 9.0) and cv.dim == 2
    assert cv.theta == (1.3, 3.0, 9.0, 0.05)
    assert cv.replace(phi=(1.0, 2.0)).phi == (1.0, 2.0) and cv.replace(tau2=0.0).theta == (1.3, 3.0, 9.0, 0.0)
    iso, phi_vec = cv.scaled()
    assert iso == N.Covariance("matern32", 1.3, 1.0, 0.05) and np.array_equal(phi_vec, [3.0, 9.0])
    with pytest.raises(dataclasses_frozen_error()):
        cv.sigma2 = 2.0
    for bad in (dict(kind="matern"), dict(kind="nope"), dict(sigma2=0.0), dict(tau2=-1.0), dict(phi=()),
                dict(phi=(1.0, 2.0, 3.0, 4.0)), dict(phi=(1.0, 0.0)), dict(phi=(1.0, float("nan"))),
                dict(phi=(1.0, float("inf"))), dict(phi=3.0), dict(sigma2=float("inf"))):
        with pytest.raises(ValueError):
            N.AnisotropicCovariance(**{**dict(kind="exponential", sigma2=1.0, phi=(3.0, 9.0), tau2=0.1), **bad})


def dataclasses_frozen_error():
    import dataclasses

    return dataclasses.FrozenInstanceError


@pytest.mark.parametrize("kind", KINDS)
def test_anisotropic_covariance_call(kind):
    rng = np.random.default_rng(0)
    a, b = rng.uniform(0, 1, (7, 2)), rng.uniform(0, 1, (5, 2))
    cv = N.AnisotropicCovariance(kind, 1.3, (0.8, 2.5), 0.05)
    u = np.sqrt((((a[:, None, :] - b[None, :, :]) * np.array([0.8, 2.5])) ** 2).sum(-1))
    want = 1.3 * rho_drho(kind, u)[0]
    assert np.allclose(cv(a, b), want, rtol=1e-14, atol=1e-15)
    assert np.allclose(cv(torch.from_numpy(a), torch.from_numpy(b)).numpy(), want, rtol=1e-14, atol=1e-15)
    with pytest.raises(ValueError):
        cv(rng.uniform(0, 1, (7, 3)), rng.uniform(0, 1, (5, 3)))


# ---------------------------------------------------------------- everything that does not serve it says so
def _bare_model(cov, n=12, dim=2, m=3):
    """An NNGP with the attributes the refusals read and nothing built on a GPU: each one must come before any sweep."""
    model = object.__new__(N.NNGP)
    model.cov, model.m, model.refType, model.device = cov, m, "S=T", torch.device("cpu")
    model.t = model.s = np.zeros((n, dim))
    model.y, model.eps = np.zeros(n), None
    model._s_dev = model._t_dev = torch.zeros((n, dim), dtype=torch.float64)
    model.nbr = torch.zeros((n, m), dtype=torch.int32)
    return model


ANISO = N.AnisotropicCovariance("exponential", 1.0, (4.0, 16.0), 0.1)


@pytest.mark.parametrize("call", [
    lambda md: md.fisher_information(),
    lambda md: md.fisher_information(cov=ANISO, values=None),
    lambda md: md.fit(method="fisher"),
    lambda md: md.fit(stderr=True),
    lambda md: md.fit(),
    lambda md: md.fit(gradient=True),
    lambda md: md.latent_posterior(),
    lambda md: md.latent_mean(),
    lambda md: md.latent_sample(2),
    lambda md: md.latent_loglik(),
    lambda md: md.latent_fit(),
    lambda md: md.prior_factor(),
    lambda md: md.simulate(),
    lambda md: md.oneSample(),
    lambda md: md.conjugate("exponential", 6.0, 0.1, np.ones((12, 1))),
    lambda md: md.conjugate_grid([6.0], [0.1], "exponential", np.ones((12, 1))),
], ids=["fisher_information", "fisher_information_cov", "fit_fisher", "fit_stderr", "fit_plain", "fit_gradient",
        "latent_posterior", "latent_mean", "latent_sample", "latent_loglik", "latent_fit", "prior_factor",
        "simulate", "oneSample", "conjugate", "conjugate_grid"])
def test_methods_refuse_by_name(call):
    with pytest.raises(TypeError, match="AnisotropicCovariance"):
        call(_bare_model(ANISO))


def test_classes_refuse_by_name():
    import pynngp_amd

    coords, y = field(12)
    with pytest.raises(TypeError, match="AnisotropicCovariance"):
        pynngp_amd.LatentPosterior(coords, y, ANISO, m=3)
    with pytest.raises(TypeError, match="AnisotropicCovariance"):
        pynngp_amd.NNGPFactor(coords, ANISO, m=3)
    with pytest.raises(TypeError, match="AnisotropicCovariance"):
        pynngp_amd.BinomialLatentPosterior(coords, np.ones(12), np.ones(12), ANISO, m=3)
    with pytest.raises(TypeError, match="AnisotropicCovariance"):
        pynngp_amd.SeqNNGP(coords, y, m=3, cov=ANISO, device="cpu")


def test_fit_anisotropic_refusals():
    md = _bare_model(N.Covariance("exponential", 1.0, 8.0, 0.1))
    with pytest.raises(NotImplementedError):
        md.fit(anisotropic=True, stderr=True)
    with pytest.raises(NotImplementedError):
        md.fit(anisotropic=True, method="fisher")
    with pytest.raises(NotImplementedError):
        md.fit(anisotropic=True, reml=True)
    with pytest.raises(ValueError):
        md.fit(anisotropic=True, nu=0.7)
    with pytest.raises(ValueError):
        md.fit(reneighbor=1)
    with pytest.raises(ValueError):  # len(phi) must equal the coordinate dimension
        md.fit(anisotropic=True, x0=(1.0, (4.0, 16.0, 2.0), 0.1))
    with pytest.raises(ValueError):
        md.loglik_grad(cov=N.AnisotropicCovariance("exponential", 1.0, (4.0,), 0.1))
    with pytest.raises(NotImplementedError):
        _bare_model(ANISO, m=0).loglik_grad()


def test_loglik_theta_shapes():
    import pynngp_amd

    c = torch.zeros((12, 2), dtype=torch.float64)
    nbr = torch.zeros((12, 3), dtype=torch.int32)
    v = torch.zeros(12, dtype=torch.float64)
    for shape in (2, 5):
        with pytest.raises(ValueError):
            pynngp_amd.loglik(c, nbr, torch.ones(shape, dtype=torch.float64), v, "exponential")
    with pytest.raises(NotImplementedError):
        pynngp_amd.loglik(c, nbr, torch.ones(4, dtype=torch.float64), v, "matern")
