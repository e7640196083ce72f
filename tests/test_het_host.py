"""tests/het_ref.py (the restatement test_gpu_het.py measures the per-point noise sweeps against) pinned by known
answers, and its own fp64 rounding measured on exactly the inputs of the GPU test.  No GPU."""
import numpy as np
import pytest

import fisher_ref as FR
import het_ref as H
from bf_precision_ref import BF_K, ratios

LD = np.longdouble
extended = pytest.mark.skipif(not FR.HAVE_EXTENDED, reason="no extended precision here")


def small(n, dim=2, seed=11):
    rng = np.random.default_rng(seed)
    coords = rng.uniform(0.0, 1.0, (n, dim))
    return coords, rng.standard_normal(n), np.exp(rng.uniform(np.log(0.2), np.log(5.0), n)) ** 2


@pytest.mark.parametrize("kind", H.KINDS)
def test_full_sets_give_the_dense_density(kind):
    """m = n - 1: the rows' log-likelihood terms sum to the dense N(0, sigma2 R + tau2 diag(v)) density, and the
    gradient terms to its gradient."""
    coords, y, v = small(24)
    th = H.theta_of(kind)
    ref = H.rows(coords, coords, FR.full_sets(24), kind, th, y, y, v, v, dtype=np.float64)
    ll, g = H.dense_loglik_grad(coords, kind, th, y, v)
    assert abs(ref.ll.sum() - ll) <= 1e-10 * abs(ll), (ref.ll.sum(), ll)
    assert np.allclose(ref.G.sum(0), g, rtol=1e-8, atol=1e-8), (ref.G.sum(0), g)


@pytest.mark.parametrize("kind", H.KINDS)
def test_unit_weights_are_the_homoscedastic_rows(kind):
    coords, y, _ = small(80)
    nbr = FR.knn_prior(coords, 9)
    th = H.theta_of(kind)
    one = np.ones(80)
    ref = H.rows(coords, coords, nbr, kind, th, y, y, one, one, dtype=np.float64)
    hom = FR.rows_bf(coords, nbr, kind, th, y)
    assert np.allclose(ref.logF, hom["logF"], rtol=0, atol=1e-12)
    assert np.allclose(ref.q, hom["q"], rtol=1e-10, atol=1e-13)
    assert np.allclose(ref.G, hom["G"], rtol=1e-9, atol=1e-10)


@extended
@pytest.mark.parametrize("kind", H.KINDS)
def test_gradient_is_the_derivative_of_its_own_likelihood(kind):
    """Central differences of the long-double likelihood (h = 1e-6 theta: truncation ~1e-12, rounding ~1e-13)."""
    coords, y, v = small(60, seed=12)
    nbr = FR.knn_prior(coords, 8)
    th = H.theta_of(kind)
    g = H.rows(coords, coords, nbr, kind, th, y, y, v, v).G.sum(0)
    for p in range(3):
        h = 1e-6 * th[p]
        tp, tm = list(th), list(th)
        tp[p], tm[p] = LD(th[p]) + LD(h), LD(th[p]) - LD(h)
        lp = H.rows(coords, coords, nbr, kind, tp, y, y, v, v).ll.sum()
        lm = H.rows(coords, coords, nbr, kind, tm, y, y, v, v).ll.sum()
        fd = (lp - lm) / (2 * LD(h))
        assert abs(fd - g[p]) <= 1e-8 * max(1.0, abs(g[p])), (kind, p, fd, g[p])


def _fp64_ratio(ld, f64, where):
    rB, rF, rR = ratios(ld, f64.b, f64.F, f64.r)
    print(f"{where}: fp64 restatement vs long double: B {rB:.3g} F {rF:.3g} R {rR:.3g}; resolved "
          f"{ld.resolved.mean():.3f}")
    return max(rB, rF, rR)


@extended
@pytest.mark.parametrize("kind", H.KINDS)
@pytest.mark.parametrize("dim", H.DIMS)
def test_fp64_restatement_rounding_on_the_gpu_inputs(dim, kind):
    """BF_K = 12 was derived as 8 x the fp64 oracle's worst ratio against long double in bf_precision_ref's scales;
    the same must hold on the per-point noise inputs (largest diagonal entry in the scales): the fp64 restatement's
    worst ratio stays <= BF_K / 8 on every case test_gpu_het.py runs."""
    coords, y, _, v = H.field(dim)
    q, yq, vq = H.query(dim)
    th = H.theta_of(kind)
    worst = 0.0
    for m in H.M_LIST:
        nbr = H.neighbours(dim, m)
        f64 = H.rows(coords, coords, nbr, kind, th, y, y, v, v, dtype=np.float64)
        worst = max(worst, _fp64_ratio(H.prior_reference(dim, m, kind), f64, f"prior d{dim} {kind} m{m}"))
        qn = H.query_neighbours(dim, m)
        f64 = H.rows(coords, q, qn, kind, th, y, yq, v, vq, dtype=np.float64)
        worst = max(worst, _fp64_ratio(H.cross_reference(dim, m, kind), f64, f"cross d{dim} {kind} m{m}"))
    assert worst <= BF_K / 8, worst


@extended
def test_fp64_restatement_rounding_with_zero_weights():
    coords, y, _, v = H.field(2, zeros=True)
    assert np.count_nonzero(v == 0.0) > 50
    for m in (3, 15, 18, 32):
        f64 = H.rows(coords, coords, H.neighbours(2, m), "exponential", H.theta_of("exponential"), y, y, v, v,
                     dtype=np.float64)
        ld = H.prior_reference(2, m, "exponential", True)
        assert _fp64_ratio(ld, f64, f"zeros m{m}") <= BF_K / 8
