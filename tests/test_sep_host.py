"""tests/sep_ref.py (the restatement test_gpu_sep.py measures the separable space-time sweeps against) pinned by known
answers, its own fp64 rounding on the GPU test's inputs, and everything that must hold without a kernel launch: the
TypeError refusals on a bare model, the C ABI's NNGP_EUNSUP / NNGP_EINVAL codes and the workspace rules.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import fisher_ref as FR
import sep_ref as S
from bf_precision_ref import BF_K, ratios
from grad_aniso_ref import ref_rows_aniso
from pynngp_amd import _lib
from pynngp_amd import nngp as N

LD = np.longdouble
extended = pytest.mark.skipif(not FR.HAVE_EXTENDED, reason="no extended precision here")
PAIRS = [(a, b) for a in S.KINDS for b in S.KINDS]


def small(n, dim=3, seed=11):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (n, dim)), rng.standard_normal(n)


@pytest.mark.parametrize("ks,kt", PAIRS)
def test_full_sets_give_the_dense_density(ks, kt):
    """m = n - 1 at n = 40: the rows' log-likelihood terms sum to the dense Gaussian log density under the product
    covariance."""
    coords, y = small(40)
    th = S.theta_of(ks, kt)
    ref = S.rows(coords, coords, FR.full_sets(40), ks, kt, th, y, y, dtype=np.float64)
    ll = S.dense_loglik(coords, ks, kt, th, y)
    assert abs(ref.ll.sum() - ll) <= 1e-10 * abs(ll), (ref.ll.sum(), ll)


@pytest.mark.parametrize("dim", [2, 3])
def test_gaussian_product_is_the_metric_model(dim):
    """gaussian x gaussian equals the per-axis model at phi = (phi_s, .., phi_s, phi_t); the phi_s gradient is the
    sum of the spatial axes' entries."""
    coords, y = small(80, dim=dim, seed=5)
    th = (1.3, 2.5, 1.1, 0.05)
    nbr = FR.knn_prior(coords, 9)
    ref = S.rows(coords, coords, nbr, "gaussian", "gaussian", th, y, y, dtype=np.float64)
    an = ref_rows_aniso(coords, nbr, "gaussian", (th[0], *([th[1]] * (dim - 1)), th[2], th[3]), y)
    want = np.stack([an[:, 2], an[:, 3:2 + dim].sum(1), an[:, 2 + dim], an[:, 3 + dim]], axis=1)
    assert np.allclose(ref.logF, an[:, 0], rtol=0, atol=1e-12)
    assert np.all(np.abs(ref.G - want) <= 1e-11 * (1 + np.abs(want))), np.abs(ref.G - want).max()


@pytest.mark.parametrize("ks", S.KINDS)
def test_constant_time_is_the_spatial_model(ks):
    """All time coordinates equal: the rows are fisher_ref.rows_bf's for kind_s on the spatial columns, and the phi_t
    column is exactly 0."""
    coords, y = small(80, seed=6)
    coords[:, -1] = 0.37
    th = S.theta_of(ks, "matern32")
    nbr = FR.knn_prior(coords, 9)
    ref = S.rows(coords, coords, nbr, ks, "matern32", th, y, y, dtype=np.float64)
    hom = FR.rows_bf(coords[:, :-1], nbr, ks, (th[0], th[1], th[3]), y)
    assert np.allclose(ref.logF, hom["logF"], rtol=0, atol=1e-12)
    assert np.allclose(ref.q, hom["q"], rtol=1e-10, atol=1e-13)
    assert np.allclose(ref.G[:, [0, 1, 3]], hom["G"], rtol=1e-9, atol=1e-10)
    assert np.all(ref.G[:, 2] == 0.0)


@extended
@pytest.mark.parametrize("ks,kt", PAIRS)
def test_gradient_is_the_derivative_of_its_own_likelihood(ks, kt):
    """Central differences of the long-double likelihood (h = 1e-6 theta: truncation ~1e-12, rounding ~1e-13)."""
    coords, y = small(60, seed=12)
    nbr = FR.knn_prior(coords, 8)
    th = S.theta_of(ks, kt)
    g = S.rows(coords, coords, nbr, ks, kt, th, y, y).G.sum(0)
    for p in range(4):
        h = 1e-6 * th[p]
        tp, tm = list(th), list(th)
        tp[p], tm[p] = LD(th[p]) + LD(h), LD(th[p]) - LD(h)
        lp = S.rows(coords, coords, nbr, ks, kt, tp, y, y).ll.sum()
        lm = S.rows(coords, coords, nbr, ks, kt, tm, y, y).ll.sum()
        fd = (lp - lm) / (2 * LD(h))
        assert abs(fd - g[p]) <= 1e-8 * max(1.0, abs(g[p])), (ks, kt, p, fd, g[p])


@extended
@pytest.mark.parametrize("ks,kt", PAIRS)
def test_fp64_restatement_rounding_on_the_gpu_inputs(ks, kt):
    """BF_K was derived as 8 x the fp64 oracle's worst ratio against long double in bf_precision_ref's scales; the same
    must hold on the separable inputs: the fp64 restatement's worst ratio stays below BF_K / 8 on the cases
    test_gpu_sep.py runs for this pair of kinds."""
    coords, y = S.field(3)
    q, yq = S.query(3)
    th = S.theta_of(ks, kt)
    worst = 0.0
    for m in (S.M_ALL if (ks, kt) == ("exponential", "exponential") else S.M_EDGES):
        f64 = S.rows(coords, coords, S.neighbours(3, m), ks, kt, th, y, y, dtype=np.float64)
        worst = max(worst, *ratios(S.prior_reference(3, m, ks, kt), f64.b, f64.F, f64.r))
        f64 = S.rows(coords, q, S.query_neighbours(3, m), ks, kt, th, y, yq, dtype=np.float64)
        worst = max(worst, *ratios(S.cross_reference(3, m, ks, kt), f64.b, f64.F, f64.r))
    print(f"{ks} x {kt}: fp64 restatement vs long double, worst ratio {worst:.3g}")
    assert worst < BF_K / 8, worst


# ---------------------------------------------------------------- the class
def test_separable_covariance():
    import pynngp_amd

    assert pynngp_amd.SeparableCovariance is N.SeparableCovariance
    assert pynngp_amd.NNGPIndexError is N.NNGPIndexError
    assert issubclass(N.NNGPIndexError, N.NNGPNumericalError) and issubclass(N.NNGPIndexError, IndexError)
    cv = N.SeparableCovariance("matern32", "exponential", 1.3, 6, 3, 0.05)
    assert cv.theta == (1.3, 6.0, 3.0, 0.05)
    assert cv.replace(phi_t=2.0).theta == (1.3, 6.0, 2.0, 0.05)
    assert np.array_equal(cv.scaled(3), [6.0, 6.0, 3.0]) and np.array_equal(cv.scaled(2), [6.0, 3.0])
    for bad in (dict(kind_s="matern"), dict(kind_t="nope"), dict(sigma2=0.0), dict(phi_s=-1.0), dict(phi_t=0.0),
                dict(tau2=-0.1), dict(phi_t=float("inf")), dict(phi_s=float("nan"))):
        with pytest.raises(ValueError):
            cv.replace(**bad)
    rng = np.random.default_rng(0)
    for dim in (2, 3):
        a, b = rng.uniform(0, 1, (7, dim)), rng.uniform(0, 1, (5, dim))
        want = S.cov_matrix(a, b, "matern32", "exponential", cv.theta)
        assert np.allclose(cv(a, b), want, rtol=1e-14, atol=1e-15)
        assert np.allclose(cv(torch.from_numpy(a), torch.from_numpy(b)).numpy(), want, rtol=1e-14, atol=1e-15)


# ---------------------------------------------------------------- everything that does not serve it says so
SEP = N.SeparableCovariance("exponential", "exponential", 1.0, 6.0, 3.0, 0.1)


def _bare_model(cov, n=12, dim=3, m=3, refType="S=T"):
    """An NNGP with the attributes the refusals read and nothing built on a GPU: each one must come before any sweep."""
    model = object.__new__(N.NNGP)
    model.cov, model.m, model.refType, model.device = cov, m, refType, torch.device("cpu")
    model.t = model.s = np.zeros((n, dim))
    model.y, model.eps = np.zeros(n), np.ones(n)
    model._s_dev = model._t_dev = torch.zeros((n, dim), dtype=torch.float64)
    model.nbr = torch.zeros((n, m), dtype=torch.int32)
    return model


@pytest.mark.parametrize("call", [
    lambda md: md.fisher_information(),
    lambda md: md.fisher_information(cov=SEP, values=None),
    lambda md: md.fit(method="fisher"),
    lambda md: md.fit(stderr=True),
    lambda md: md.fit(reml=True),
    lambda md: md.fit(noise="eps"),
    lambda md: md.fit(anisotropic=True),
    lambda md: md.fit(estimate_nu=True),
    lambda md: md.gls(None, np.ones((12, 1)), reml=True),
    lambda md: md.loglik(noise="eps"),
    lambda md: md.loglik_grad(noise="eps"),
    lambda md: md.profile_loglik(SEP, noise="eps"),
    lambda md: md.predict(noise="eps"),
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
], ids=["fisher_information", "fisher_information_cov", "fit_fisher", "fit_stderr", "fit_reml", "fit_noise",
        "fit_anisotropic", "fit_estimate_nu", "gls_reml", "loglik_noise", "loglik_grad_noise", "profile_noise",
        "predict_noise", "latent_posterior", "latent_mean", "latent_sample", "latent_loglik", "latent_fit",
        "prior_factor", "simulate", "oneSample", "conjugate", "conjugate_grid"])
def test_methods_refuse_by_name(call):
    with pytest.raises(TypeError, match="SeparableCovariance"):
        call(_bare_model(SEP))


@pytest.mark.parametrize("call", [lambda md: md.loglik(), lambda md: md.loglik_grad(), lambda md: md.compute_BF(),
                                  lambda md: md.fit(), lambda md: md.rebuild_neighbors()],
                         ids=["loglik", "loglik_grad", "compute_BF", "fit", "rebuild_neighbors"])
def test_tuple_reftypes_refuse_by_name(call):
    with pytest.raises(TypeError, match="SeparableCovariance"):
        call(_bare_model(SEP, refType=("subset", 5)))


def test_classes_refuse_by_name():
    import pynngp_amd

    coords, y = small(12)
    with pytest.raises(TypeError, match="SeparableCovariance"):
        pynngp_amd.LatentPosterior(coords, y, SEP, m=3)
    with pytest.raises(TypeError, match="SeparableCovariance"):
        pynngp_amd.NNGPFactor(coords, SEP, m=3)
    with pytest.raises(TypeError, match="SeparableCovariance"):
        pynngp_amd.SeqNNGP(coords, y, m=3, cov=SEP, device="cpu")
    with pytest.raises(TypeError, match="SeparableCovariance"):
        pynngp_amd.ShardedLogLik.local_partials(object.__new__(pynngp_amd.ShardedLogLik), SEP, None)


def test_scope_refusals():
    with pytest.raises(NotImplementedError):
        _bare_model(SEP, m=33).loglik_grad()
    with pytest.raises(ValueError):
        _bare_model(SEP, dim=1).loglik()
    c = torch.zeros((12, 3), dtype=torch.float64)
    nbr = torch.zeros((12, 3), dtype=torch.int32)
    v = torch.zeros(12, dtype=torch.float64)
    with pytest.raises(NotImplementedError):
        _lib.bf_sweep_sep(c, nbr, 0, "matern", "exponential", 1.0, 6.0, 3.0, 0.1)
    with pytest.raises(NotImplementedError):
        _lib.bf_grad_sep(c[:, :1], nbr, 0, "exponential", "exponential", 1.0, 6.0, 3.0, 0.1, v)
    with pytest.raises(Exception, match="GPU"):  # CPU tensors are refused before any call
        _lib.bf_sweep_sep(c, nbr, 0, "exponential", "exponential", 1.0, 6.0, 3.0, 0.1)
    import pynngp_amd

    th = torch.tensor([1.0, 6.0, 3.0, 0.1], dtype=torch.float64)
    with pytest.raises(ValueError):
        pynngp_amd.loglik_sep(c, nbr, "exponential", "exponential", th[:3], v)
    with pytest.raises(NotImplementedError):
        pynngp_amd.loglik_sep(c, nbr, "matern", "exponential", th, v)
    with pytest.raises(NotImplementedError):
        pynngp_amd.loglik_sep(c[:, :1], nbr, "exponential", "exponential", th, v)


# ---------------------------------------------------------------- C ABI refusals (fake addresses, never dereferenced)
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _codes():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nngp.h")).read()
    out = {}
    for name in ("NNGP_OK", "NNGP_EINVAL", "NNGP_EUNSUP"):
        mm = re.search(r"#define\s+" + name + r"\s+\(?(-?\d+)", hdr)
        assert mm, name
        out[name] = int(mm.group(1))
    return out


def _call(lib, entry="grad", *, coords=256, n_points=100, dim=3, nbr=512, order=None, n_rows=100, m=10, i0=0, kind_s=0,
          kind_t=0, sigma2=1.0, phi_s=6.0, phi_t=3.0, tau2=0.1, values=768, partials=1024, grad=1280, workspace=4096,
          ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.nngp_bf_sweep_sep_workspace_bytes(n_rows, m) or 4096
    th = (kind_s, kind_t, sigma2, phi_s, phi_t, tau2)
    if entry == "grad":
        return lib.nngp_bf_grad_sep(coords, n_points, dim, nbr, order, n_rows, m, i0, *th, values, None, partials, grad,
                                    workspace, ws_bytes, None)
    if entry == "sweep":
        return lib.nngp_bf_sweep_sep(coords, n_points, dim, nbr, order, n_rows, m, i0, *th, values, None, None, None,
                                     partials, workspace, ws_bytes, None)
    return lib.nngp_bf_cross_sep(coords, n_points, dim, coords, n_points, nbr, order, n_rows, m, i0, *th, values, None,
                                 None, None, None, partials, workspace, ws_bytes, None)


ENTRIES = ("sweep", "cross", "grad")


def test_workspace_bytes(lib):
    prev = 0
    for n in (0, 1, 63, 64, 65, 1000, 10**6, 10**7):
        for m in (1, 8, 9, 15, 16, 23, 24, 31, 32):
            assert lib.nngp_bf_sweep_sep_workspace_bytes(n, m) % 256 == 0
        b = lib.nngp_bf_sweep_sep_workspace_bytes(n, 15)
        assert b >= prev and b > 0
        prev = b
    for m in (0, 33, -1):
        assert lib.nngp_bf_sweep_sep_workspace_bytes(100, m) == 0
    assert lib.nngp_bf_sweep_sep_workspace_bytes(-1, 10) == 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_unsupported(lib, entry):
    c = _codes()
    for kw in (dict(kind_s=5), dict(kind_t=5)):
        assert _call(lib, entry, **kw) == c["NNGP_EUNSUP"]
        assert b"matern" in lib.nngp_last_error()
    for kw in (dict(m=0), dict(m=33), dict(dim=1), dict(dim=0), dict(dim=4)):
        assert _call(lib, entry, **kw) == c["NNGP_EUNSUP"], kw


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kw", [
    dict(sigma2=0.0), dict(sigma2=-1.0), dict(sigma2=float("nan")), dict(tau2=-0.1), dict(tau2=float("inf")),
    dict(phi_s=0.0), dict(phi_s=-1.0), dict(phi_s=float("nan")), dict(phi_s=float("inf")), dict(phi_t=0.0),
    dict(phi_t=-2.0), dict(phi_t=float("nan")), dict(phi_t=float("inf")), dict(kind_s=-1), dict(kind_t=6),
    dict(partials=None), dict(coords=None), dict(workspace=None), dict(nbr=None), dict(workspace=4096 + 8),
    dict(i0=1), dict(n_rows=-1),
], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_invalid(lib, entry, kw):
    assert _call(lib, entry, **kw) == _codes()["NNGP_EINVAL"], lib.nngp_last_error()


def test_invalid_gradient_arguments(lib):
    c = _codes()
    assert _call(lib, "grad", values=None) == c["NNGP_EINVAL"]
    assert _call(lib, "grad", grad=None) == c["NNGP_EINVAL"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_short_workspace(lib, entry):
    need = lib.nngp_bf_sweep_sep_workspace_bytes(10**6, 15)
    assert need > 256
    assert _call(lib, entry, n_points=10**6, n_rows=10**6, m=15, ws_bytes=need - 1) == _codes()["NNGP_EINVAL"]
    assert b"workspace" in lib.nngp_last_error()
