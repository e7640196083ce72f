"""tests/ns_ref.py (the restatement test_gpu_ns.py measures the nonstationary sweeps against) pinned by known answers,
its own fp64 rounding measured on exactly the inputs of the GPU test, and the argument checks of the two C entry
points.  No GPU."""
import ctypes

import numpy as np
import pytest

import fisher_ref as FR
import het_ref as H
import ns_ref as NS
from bf_precision_ref import BF_K, ratios

extended = pytest.mark.skipif(not FR.HAVE_EXTENDED, reason="no extended precision here")


@pytest.mark.parametrize("dim,kind", [(1, "matern32"), (2, "exponential"), (3, "matern52"), (2, "gaussian")])
def test_full_sets_give_the_dense_density(dim, kind):
    """m = n - 1: the rows' terms sum to the dense normal log density under the full nonstationary covariance."""
    rng = np.random.default_rng(31 + dim)
    n = 40
    coords, y = rng.uniform(0.0, 1.0, (n, dim)), rng.standard_normal(n)
    f = NS.fields_at(coords)
    ref = NS.rows(coords, coords, FR.full_sets(n), kind, f, f, y, y, dtype=np.float64)
    K = NS.cov(coords, f, coords, f, kind, np.float64) + np.diag(f[2])
    ll = -0.5 * (n * NS.LOG_2PI + np.linalg.slogdet(K)[1] + y @ np.linalg.solve(K, y))
    assert abs(ref.ll.sum() - ll) <= 1e-10 * abs(ll), (ref.ll.sum(), ll)


@pytest.mark.parametrize("kind", NS.KINDS)
def test_constant_fields_are_the_stationary_rows(kind):
    rng = np.random.default_rng(5)
    coords, y = rng.uniform(0.0, 1.0, (80, 2)), rng.standard_normal(80)
    nbr, th, one = FR.knn_prior(coords, 9), H.theta_of(kind), np.ones(80)
    f = tuple(np.full(80, t) for t in th)
    ref = NS.rows(coords, coords, nbr, kind, f, f, y, y, dtype=np.float64)
    het = H.rows(coords, coords, nbr, kind, th, y, y, one, one, dtype=np.float64)
    assert np.allclose(ref.b, het.b, rtol=0, atol=1e-12)
    assert np.allclose(ref.logF, het.logF, rtol=0, atol=1e-12)
    assert np.allclose(ref.q, het.q, rtol=1e-10, atol=1e-13)


@extended
@pytest.mark.parametrize("cross", [False, True])
def test_fp64_restatement_rounding_on_the_gpu_inputs(cross):
    """BF_K = 12 is 8 x the fp64 oracle's worst ratio against long double in bf_precision_ref's scales; the same must
    hold here (largest diagonal entry in the scales) on every case test_gpu_ns.py runs."""
    worst = 0.0
    for dim, kind, m in (NS.CROSS_CASES if cross else NS.CASES):
        coords, y, f, q, fq = NS.field(dim)
        nbr = NS.neighbours(dim, m, cross)
        f64 = (NS.rows(coords, q, nbr, kind, f, fq, y, None, dtype=np.float64) if cross else
               NS.rows(coords, coords, nbr, kind, f, f, y, y, dtype=np.float64))
        r = max(ratios(NS.reference(dim, m, kind, cross), f64.b, f64.F, f64.r))
        print(f"d{dim} {kind} m{m} cross={cross}: fp64 restatement vs long double {r:.3g}")
        worst = max(worst, r)
    assert worst <= BF_K / 8, worst


def _call(lib, cross, **kw):
    a = dict(coords=1, n=10, dim=2, nbr=1, n_rows=10, m=15, kind=0, fields=1, partials=1, workspace=256,
             workspace_bytes=1 << 20)
    a.update(kw)
    P = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731
    f = [P(a["fields"])] * 3
    tail = (None, None, None, P(a["partials"]), P(a["workspace"]), a["workspace_bytes"], None)
    if cross:
        return lib.nngp_bf_cross_ns(P(a["coords"]), a["n"], a["dim"], P(a["coords"]), a["n"], P(a["nbr"]), None,
                                    a["n_rows"], a["m"], 0, a["kind"], *f, *f, None, None, *tail)
    return lib.nngp_bf_sweep_ns(P(a["coords"]), a["n"], a["dim"], P(a["nbr"]), None, a["n_rows"], a["m"], 0,
                                a["kind"], *f, None, *tail)


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("kw,code", [
    (dict(m=0), -4), (dict(m=33), -4), (dict(dim=0), -4), (dict(dim=4), -4),
    (dict(kind=4), -4), (dict(kind=5), -4), (dict(kind=9), -4),
    (dict(coords=None), -1), (dict(fields=None), -1), (dict(partials=None), -1), (dict(nbr=None), -1),
    (dict(workspace=None), -1), (dict(workspace=257), -1), (dict(workspace_bytes=None), -1),
])
def test_entry_points_reject_before_any_device_call(cross, kw, code):
    from pynngp_amd import _lib

    lib = _lib.load()
    if "workspace_bytes" in kw:  # one byte short of the stated size
        kw = dict(workspace_bytes=lib.nngp_bf_sweep_ns_workspace_bytes(10, 15) - 1)
    assert lib.nngp_bf_sweep_ns_workspace_bytes(10, 15) >= 256 and lib.nngp_bf_sweep_ns_workspace_bytes(10, 33) == 0
    assert _call(lib, cross, **kw) == code, lib.nngp_last_error().decode()
