"""tests/svc_ref.py (the restatement test_gpu_svc.py measures the varying-coefficient sweeps against) pinned by known
answers and by its own fp64 rounding on the GPU test's inputs, and what must hold without a kernel launch: the C ABI's
NNGP_EUNSUP / NNGP_EINVAL codes, the workspace rule and the Python refusals.  No GPU."""
import ctypes

import numpy as np
import pytest

import fisher_ref as FR
import svc_ref as S
from bf_precision_ref import BF_K, ratios
from pynngp_amd import _lib, svc

LD = np.longdouble
extended = pytest.mark.skipif(not FR.HAVE_EXTENDED, reason="no extended precision here")


def small(n, r, dim=2, seed=11):
    rng = np.random.default_rng(seed)
    Z = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, 3))], axis=1)[:, :r]
    return rng.uniform(0.0, 1.0, (n, dim)), Z, rng.standard_normal(n)


@pytest.mark.parametrize("kind", S.KINDS)
def test_full_sets_give_the_dense_density(kind):
    """m = n - 1 at n = 30, r = 3: the rows' terms sum to the dense Gaussian log density of the SVC covariance."""
    coords, Z, y = small(30, 3)
    th = S.theta_of(kind, 3)
    ref = S.rows(coords, Z, coords, Z, FR.full_sets(30), kind, th, y, y, dtype=np.float64)
    ll = S.dense_loglik(coords, Z, kind, th, y, dtype=np.float64)
    assert abs(ref.ll.sum() - ll) <= 1e-10 * abs(ll), (ref.ll.sum(), ll)


@pytest.mark.parametrize("kind", S.KINDS)
def test_one_constant_covariate_is_the_isotropic_model(kind):
    """r = 1, Z = 1: fisher_ref.rows_bf's rows, the gradient in (sigma2, phi, tau2) included."""
    coords, _, y = small(80, 1, seed=6)
    th = FR.theta_of(kind)
    nbr = FR.knn_prior(coords, 9)
    ref = S.rows(coords, np.ones((80, 1)), coords, np.ones((80, 1)), nbr, kind, ((th[0],), (th[1],), th[2]), y, y,
                 dtype=np.float64)
    hom = FR.rows_bf(coords, nbr, kind, th, y)
    assert np.allclose(ref.logF, hom["logF"], rtol=0, atol=1e-12)
    assert np.allclose(ref.q, hom["q"], rtol=1e-10, atol=1e-13)
    assert np.allclose(ref.G, hom["G"], rtol=1e-9, atol=1e-10)


@extended
@pytest.mark.parametrize("kind", S.KINDS)
def test_gradient_is_the_derivative_of_its_own_likelihood(kind):
    """Central differences of the long-double likelihood in every parameter (h = 1e-6 theta), r = 2."""
    coords, Z, y = small(60, 2, seed=12)
    nbr = FR.knn_prior(coords, 8)
    th = S.theta_of(kind, 2)
    flat = [*th[0], *th[1], th[2]]
    g = S.rows(coords, Z, coords, Z, nbr, kind, th, y, y).G.sum(0)
    for p in range(5):
        h = LD(1e-6 * flat[p])
        ll = []
        for sgn in (1, -1):
            t = [LD(x) for x in flat]
            t[p] += sgn * h
            ll.append(S.rows(coords, Z, coords, Z, nbr, kind, (t[:2], t[2:4], t[4]), y, y).ll.sum())
        fd = (ll[0] - ll[1]) / (2 * h)
        assert abs(fd - g[p]) <= 1e-8 * max(1.0, abs(g[p])), (kind, p, fd, g[p])


@extended
@pytest.mark.parametrize("kind", S.KINDS)
def test_fp64_restatement_rounding_on_the_gpu_inputs(kind):
    """BF_K is 8 x the fp64 oracle's worst ratio against long double in bf_precision_ref's scales; the same must hold
    on these inputs: the fp64 restatement stays below BF_K / 8 on the cases test_gpu_svc.py runs for this kind."""
    cases = [(r, dim, m) for r in (1, 3, 4) for dim in (1, 2, 3) for m in S.M_EDGES]
    if kind == "exponential":
        cases += [(2, 2, m) for m in S.M_ALL]
    worst = 0.0
    for r, dim, m in cases:
        for fn in (S.prior_reference, S.cross_reference):
            f64 = fn(dim, m, kind, r, np.float64)
            worst = max(worst, *ratios(fn(dim, m, kind, r), f64.b, f64.F, f64.r))
    print(f"{kind}: fp64 restatement vs long double, worst ratio {worst:.3g}")
    assert worst < BF_K / 8, worst


# ---------------------------------------------------------------- the classes, without a GPU
def test_covariance_and_refusals():
    import pynngp_amd

    assert pynngp_amd.SVCCovariance is svc.SVCCovariance and pynngp_amd.SVCNNGP is svc.SVCNNGP
    cv = svc.SVCCovariance("matern32", (1.0, 0.5), (6, 3), 0.1)
    assert cv.r == 2 and cv.theta == (1.0, 0.5, 6.0, 3.0, 0.1)
    for bad in (dict(phi=(6.0, 0.0)), dict(phi=(6.0, float("inf"))), dict(sigma2=(-1.0, 1.0)), dict(tau2=-0.1),
                dict(sigma2=(1.0,)), dict(kind="nope")):
        with pytest.raises(ValueError):
            cv.replace(**bad)
    for bad in (dict(kind="matern"), dict(sigma2=(1.0,) * 5, phi=(1.0,) * 5)):
        with pytest.raises(NotImplementedError, match="varying-coefficient"):
            cv.replace(**bad)
    coords, Z, _ = small(7, 2)
    want = S.dense_cov(coords, Z, coords[:5], Z[:5], "matern32", (cv.sigma2, cv.phi, cv.tau2), np.float64)
    assert np.allclose(cv(coords, Z, coords[:5], Z[:5]), want, rtol=1e-13, atol=1e-15)
    with pytest.raises(TypeError):
        svc.SVCNNGP(coords, np.zeros(7), Z, 3, pynngp_amd.Covariance("exponential", 1.0, 6.0, 0.1))
    with pytest.raises(NotImplementedError, match="varying-coefficient"):
        svc.SVCNNGP(coords, np.zeros(7), Z, 33, cv)
    with pytest.raises(NotImplementedError, match="varying-coefficient"):
        object.__new__(svc.SVCNNGP).latent_posterior()


# ---------------------------------------------------------------- C ABI refusals (fake addresses, never dereferenced)
def _call(lib, entry, *, coords=256, n_points=100, dim=2, Z=512, r=2, nbr=768, n_rows=100, m=10, i0=0, kind=0,
          sigma2=(1.0, 0.5, 1.0, 1.0), phi=(6.0, 3.0, 1.0, 1.0), tau2=0.1, values=1024, partials=1280, grad=1536,
          workspace=4096):
    s2 = None if sigma2 is None else (ctypes.c_double * 4)(*sigma2)
    ph = None if phi is None else (ctypes.c_double * 4)(*phi)
    wb = lib.nngp_bf_sweep_svc_workspace_bytes(n_rows, m, r) or 4096
    if entry == "grad":
        return lib.nngp_bf_grad_svc(coords, n_points, dim, Z, r, nbr, None, n_rows, m, i0, kind, s2, ph, tau2, values,
                                    None, partials, grad, workspace, wb, None)
    if entry == "sweep":
        return lib.nngp_bf_sweep_svc(coords, n_points, dim, Z, r, nbr, None, n_rows, m, i0, kind, s2, ph, tau2, values,
                                     None, None, None, partials, workspace, wb, None)
    return lib.nngp_bf_cross_svc(coords, n_points, dim, Z, r, coords, Z, n_points, nbr, None, n_rows, m, i0, kind, s2, ph,
                                 tau2, 1, values, None, None, None, None, partials, workspace, wb, None)


@pytest.mark.parametrize("entry", ("sweep", "cross", "grad"))
def test_c_abi_refusals(entry):
    lib = _lib.load()
    EINVAL, EUNSUP = -1, -4  # include/nngp.h (tests/test_capi_host.py pins the two codes)
    for kw in (dict(m=0), dict(m=33), dict(r=0), dict(r=5), dict(kind=5), dict(dim=0), dict(dim=4)):
        assert _call(lib, entry, **kw) == EUNSUP, (kw, lib.nngp_last_error())
    for kw in (dict(coords=None), dict(Z=None), dict(nbr=None), dict(partials=None), dict(workspace=None),
               dict(sigma2=None), dict(phi=None), dict(phi=(6.0, 0.0, 1.0, 1.0)), dict(phi=(6.0, float("inf"), 1.0, 1.0)),
               dict(phi=(float("nan"), 3.0, 1.0, 1.0)), dict(sigma2=(1.0, -0.5, 1.0, 1.0)), dict(tau2=-0.1),
               dict(kind=-1), dict(i0=1), dict(workspace=4096 + 8)):
        assert _call(lib, entry, **kw) == EINVAL, (kw, lib.nngp_last_error())
    if entry == "grad":
        assert _call(lib, entry, values=None) == EINVAL and _call(lib, entry, grad=None) == EINVAL
    for n, m, r in ((100, 0, 2), (100, 33, 2), (100, 10, 0), (100, 10, 5), (-1, 10, 2)):  # unsupported: no workspace
        assert lib.nngp_bf_sweep_svc_workspace_bytes(n, m, r) == 0
    assert all(lib.nngp_bf_sweep_svc_workspace_bytes(n, 15, 4) % 256 == 0 for n in (0, 1, 1000, 10**6))
    assert lib.nngp_bf_sweep_svc_workspace_bytes(0, 15, 4) > 0

