"""GPU: the latent-field posterior at fixed theta -- the precision operator A = (I - B)^T (sigma2 F)^-1 (I - B) +
diag(d) applied matrix-free, the Jacobi-preconditioned CG on it, exact draws and the GLS mean.

Ground truth: the dense algebra of oracle/nngp_gibbs_oracle.py (``precision``, ``dag_posterior``) with B and F
from ``oracle.nngp_oracle.bf_sweep``.  The reference keeps the latent state as ws / wt (pyNNGP/nngp.py:42-47)
and has no estimator for it, so parity is against the model's exact Gaussian posterior.

Tolerances.  Operator: |out - A x|_i <= 4 (m + deg_i + 4) 2^-52 (|A| |x|)_i, deg_i the node's child count -- the
standard rounding bound of the two dot products behind out_i (m terms in the row phase, deg_i in the column
phase, a few scalings); derived, not measured.  Solves: |w - w*| <= 2 cond(A) rtol |w*| (the residual rule
|r| <= rtol |b| bounds the relative error by cond(A) rtol; 2 for the recurrence residual's drift and the
GPU's own B / F), with cond(A) from the dense A.
"""
import functools
import math
import warnings

import numpy as np
import pytest
import torch

from oracle import nngp_gibbs_oracle as G
from oracle import nngp_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
SIGMA2 = 1.3
CHECK_EVERY = 8


# ---------------------------------------------------------------- helpers
def _device_geometry(dev, nbr, B, F):
    """The operator's arguments on the device from host (nbr, B, F)."""
    from pynngp_amd import _lib

    nbr_d = torch.from_numpy(np.array(nbr, dtype=np.int32)).to(dev)  # copies: the shared fields are read-only
    B_d = torch.from_numpy(np.array(B, dtype=np.float64)).to(dev)
    F_d = torch.from_numpy(np.array(F, dtype=np.float64)).to(dev)
    off, rev_j, rev_k = _lib.reverse_neighbors(nbr_d)
    prep = _lib.gibbs_prepare(B_d, F_d, off, rev_j, rev_k)
    return nbr_d, B_d, off, rev_j, rev_k, prep


def _deg(nbr):
    return np.bincount(nbr[nbr >= 0], minlength=nbr.shape[0])


def _random_d(rng, n):
    return rng.uniform(0.1, 10.0, n) * (rng.uniform(size=n) >= 0.3)  # 30 % zeros


def _check_operator(dev, nbr, B, F, rng):
    """precision_apply against the dense A, with d NULL and with a random d, within the derived bound."""
    from pynngp_amd import _lib

    n, m = nbr.shape
    geom = _device_geometry(dev, nbr, B, F)
    Q = G.precision(nbr, B, F * SIGMA2)
    deg = _deg(nbr)
    for d in (None, _random_d(rng, n)):
        A = Q if d is None else Q + np.diag(d)
        x = rng.standard_normal(n)
        out = _lib.precision_apply(*geom, SIGMA2, torch.from_numpy(x).to(dev),
                                   d=None if d is None else torch.from_numpy(d).to(dev)).cpu().numpy()
        bound = 4.0 * (m + deg + 4) * U * (np.abs(A) @ np.abs(x))
        err = np.abs(out - A @ x)
        worst = int(np.argmax(err - bound))
        print(f"operator n={n} m={m} d={'yes' if d is not None else 'no'}: max err/bound "
              f"{(err / np.maximum(bound, 1e-300)).max():.3g}")
        assert np.all(err <= bound), (n, m, worst, err[worst], bound[worst])


@functools.lru_cache(maxsize=None)
def _field(n, m, dim, kind, phi, seed=0):
    """Uniform coordinates, oracle neighbour sets and oracle unit-variance B / F (shared, read-only)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(size=(n, dim))
    y = rng.standard_normal(n)
    nbr = O.knn_prior(c, m)
    theta = (1.0, phi, 0.0, 1.5) if kind == "matern" else (1.0, phi, 0.0)
    B, F, _ = O.bf_sweep(c, nbr, kind, theta)
    for a in (c, y, nbr, B, F):
        a.setflags(write=False)
    return c, y, nbr, B, F


def _numpy_pcg_iterations(A, b, rtol, max_iter=20000):
    """Iterations a plain numpy Jacobi-PCG needs for |r| <= rtol |b| (the GPU solver's rule)."""
    Mi = 1.0 / np.diag(A)
    x = np.zeros_like(b)
    r = b.copy()
    z = Mi * r
    p = z.copy()
    rz, bb = r @ z, b @ b
    for k in range(max_iter):
        if r @ r <= rtol * rtol * bb:
            return k
        q = A @ p
        a = rz / (p @ q)
        x += a * p
        r -= a * q
        z = Mi * r
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return max_iter


# ---------------------------------------------------------------- 1. operator on real neighbour sets
@pytest.mark.parametrize("n,m,dim", [(1, 1, 2), (2, 1, 1), (16, 15, 2), (257, 32, 2), (400, 8, 2), (300, 15, 3),
                                     (130, 63, 2)])
def test_operator_matches_dense_precision(dev, n, m, dim):
    _, _, nbr, B, F = _field(n, m, dim, "exponential", 6.0)
    _check_operator(dev, nbr, B, F, np.random.default_rng(n + m))


# ---------------------------------------------------------------- 2. operator on handmade DAGs
def _handmade(nbr, rng):
    n, m = nbr.shape
    return rng.uniform(-0.3, 0.3, (n, m)), rng.uniform(0.1, 2.0, n)


def test_operator_hub(dev):
    """Node 0 is a parent of every other row: one reverse list of 2999 entries (the block-cooperative path)."""
    rng = np.random.default_rng(1)
    n, m = 3000, 4
    nbr = np.full((n, m), -1, dtype=np.int32)
    for j in range(1, n):
        nbr[j, 0] = 0
        k = min(m - 1, j - 1)
        if k > 0:
            nbr[j, 1:1 + k] = 1 + rng.choice(j - 1, size=k, replace=False)
    assert _deg(nbr)[0] == n - 1
    _check_operator(dev, nbr, *_handmade(nbr, rng), rng)


def test_operator_chain(dev):
    rng = np.random.default_rng(2)
    n = 1000
    nbr = (np.arange(n, dtype=np.int32) - 1)[:, None]
    _check_operator(dev, nbr, *_handmade(nbr, rng), rng)


def test_operator_holes_in_rows(dev):
    """Rows whose valid slots are not a prefix (-1 in the middle); B in a -1 slot must contribute exactly 0."""
    rng = np.random.default_rng(3)
    n, m = 700, 6
    nbr = np.full((n, m), -1, dtype=np.int32)
    for j in range(1, n):
        k = min(m, j)
        slots = rng.choice(m, size=int(rng.integers(1, k + 1)), replace=False)
        nbr[j, slots] = rng.choice(j, size=len(slots), replace=False)
    assert np.any((nbr[:, :-1] < 0) & (nbr[:, 1:] >= 0))
    B, F = _handmade(nbr, rng)  # random B in the -1 slots too
    _check_operator(dev, nbr, B, F, rng)


# ---------------------------------------------------------------- 3. bit reproducibility
def test_matvec_and_solve_are_bit_reproducible(dev):
    from pynngp_amd import Covariance, LatentPosterior

    c, y, _, _, _ = _field(400, 8, 2, "exponential", 6.0)
    lp = LatentPosterior(c, y, Covariance("exponential", SIGMA2, 6.0, 0.1), m=8, device=dev)
    x = torch.from_numpy(np.random.default_rng(5).standard_normal(400)).to(dev)
    assert torch.equal(lp.matvec(x), lp.matvec(x))
    (s1, i1), (s2, i2) = lp.solve(x), lp.solve(x)
    assert torch.equal(s1, s2) and i1 == i2 and i1.converged
    # the hub's block-cooperative sum too
    rng = np.random.default_rng(1)
    n, m = 3000, 4
    nbr = np.full((n, m), -1, dtype=np.int32)
    nbr[1:, 0] = 0
    B, F = _handmade(nbr, rng)
    from pynngp_amd import _lib

    geom = _device_geometry(dev, nbr, B, F)
    xh = torch.from_numpy(rng.standard_normal(n)).to(dev)
    assert torch.equal(_lib.precision_apply(*geom, SIGMA2, xh), _lib.precision_apply(*geom, SIGMA2, xh))


def test_torch_ops_match_the_binding(dev):
    from pynngp_amd import _lib, load_ops

    load_ops()
    _, _, nbr, B, F = _field(400, 8, 2, "exponential", 6.0)
    geom = _device_geometry(dev, nbr, B, F)
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.standard_normal(400)).to(dev)
    d = torch.from_numpy(_random_d(rng, 400) + 0.5).to(dev)
    assert torch.equal(torch.ops.nngp.precision_apply(*geom, SIGMA2, d, x), _lib.precision_apply(*geom, SIGMA2, x, d=d))
    xs, info = torch.ops.nngp.latent_cg(*geom, SIGMA2, d, x, None, 1e-9, 500, 8)
    ref, info_ref = _lib.latent_cg(*geom, SIGMA2, x, torch.zeros_like(x), d=d, rtol=1e-9, max_iter=500)
    assert torch.equal(xs, ref) and info.tolist() == info_ref and info_ref[1] == 1.0
    assert info.device.type == "cpu" and tuple(info.shape) == (4,)


# ---------------------------------------------------------------- 4. symmetry, positive definiteness
def test_operator_symmetric_positive_definite(dev):
    from pynngp_amd import Covariance, LatentPosterior

    c, yv, _, _, _ = _field(400, 8, 2, "exponential", 6.0)
    lp = LatentPosterior(c, yv, Covariance("exponential", SIGMA2, 6.0, 0.1), m=8, device=dev)
    rng = np.random.default_rng(7)
    x, y = rng.standard_normal(400), rng.standard_normal(400)
    Ax, Ay = lp.matvec(x), lp.matvec(y)
    assert abs(x @ Ay - y @ Ax) <= 1e-12 * max(abs(x @ Ay), abs(y @ Ax))
    assert x @ Ax > 0 and y @ Ay > 0


# ---------------------------------------------------------------- 5. CG mean against dag_posterior
CASES = {
    "exp": dict(n=400, m=8, dim=2, kind="exponential", phi=6.0, tau2=0.1),
    "exp_unobserved": dict(n=400, m=8, dim=2, kind="exponential", phi=6.0, tau2=0.1, unobserved=0.3),
    "matern32": dict(n=600, m=10, dim=2, kind="matern32", phi=12.0, tau2=0.05),
    "exp_1d": dict(n=500, m=5, dim=1, kind="exponential", phi=20.0, tau2=1.0),
}


def _case(name):
    k = CASES[name]
    c, y, nbr, B, F = _field(k["n"], k["m"], k["dim"], k["kind"], k["phi"])
    y = y.copy()
    if "unobserved" in k:
        y[np.random.default_rng(11).uniform(size=k["n"]) < k["unobserved"]] = np.nan
    h = np.isfinite(y).astype(np.float64)
    return k, c, y, nbr, B, F, h


@pytest.mark.parametrize("name", list(CASES))
def test_cg_mean_matches_dense_posterior(dev, name):
    from pynngp_amd import Covariance, LatentPosterior

    k, c, y, nbr, B, F, h = _case(name)
    rtol = 1e-10
    A, b, w_ref, _ = G.dag_posterior(nbr, B, F, SIGMA2, k["tau2"], h, np.where(h > 0, y, 0.0))
    it_np = _numpy_pcg_iterations(A, b, rtol)
    cond = np.linalg.cond(A)
    lp = LatentPosterior(c, y, Covariance(k["kind"], SIGMA2, k["phi"], k["tau2"]), m=k["m"], device=dev)
    w, info = lp.solve(b, rtol=rtol)
    cap = math.ceil(1.1 * it_np) + CHECK_EVERY
    err = np.linalg.norm(w - w_ref) / np.linalg.norm(w_ref)
    print(f"{name}: numpy PCG {it_np} iterations, GPU {info.iterations} (cap {cap}), cond(A) {cond:.3g}, "
          f"rel err {err:.3g} (bound {2 * cond * rtol:.3g})")
    assert info.converged and info.iterations <= cap
    assert info.residual2 <= rtol * rtol * info.rhs2
    assert err <= 2.0 * cond * rtol
    w_mean, beta = lp.mean(rtol=rtol)  # no X: the same system, b formed on the device
    assert beta.shape == (0,)
    assert np.linalg.norm(w_mean - w_ref) <= 2.0 * cond * rtol * np.linalg.norm(w_ref)


# ---------------------------------------------------------------- 6. non-convergence is reported
def test_non_convergence_is_reported(dev):
    from pynngp_amd import Covariance, LatentPosterior

    n, m, phi, tau2 = 600, 10, 10.0, 0.05
    c, y, nbr, B, F = _field(n, m, 2, "gaussian", phi)
    A, b, w_ref, _ = G.dag_posterior(nbr, B, F, SIGMA2, tau2, np.ones(n), y)
    lp = LatentPosterior(c, y, Covariance("gaussian", SIGMA2, phi, tau2), m=m, device=dev)
    with pytest.warns(RuntimeWarning, match="did not reach"):
        w, info = lp.solve(b, rtol=1e-10, max_iter=50)
    assert info.converged is False and info.iterations == 50
    e = w - w_ref
    print(f"gaussian: A-norm error^2 after 50 iterations {e @ A @ e:.4g}, of the zero start {w_ref @ A @ w_ref:.4g}")
    assert e @ A @ e < w_ref @ A @ w_ref


def test_breakdown_raises(dev):
    from pynngp_amd import Covariance, LatentPosterior, NNGPNumericalError

    c, y, _, _, _ = _field(400, 8, 2, "exponential", 6.0)
    lp = LatentPosterior(c, y, Covariance("exponential", SIGMA2, 6.0, 0.1), m=8, device=dev)
    lp.B[:, 0] = float("nan")
    with pytest.raises(NNGPNumericalError, match="breakdown"):
        lp.solve(y)


# ---------------------------------------------------------------- 7. exact draws
def test_sample_with_given_normals_matches_dense(dev):
    from pynngp_amd import Covariance, LatentPosterior

    k, c, y, nbr, B, F, h = _case("exp_unobserved")
    n, tau2, rtol = k["n"], k["tau2"], 1e-10
    A, b, _, _ = G.dag_posterior(nbr, B, F, SIGMA2, tau2, h, np.where(h > 0, y, 0.0))
    cond = np.linalg.cond(A)
    rng = np.random.default_rng(13)
    z1, z2 = rng.standard_normal((2, n)), rng.standard_normal((2, n))
    IB = np.eye(n) - G.dense_B(nbr, B)
    lp = LatentPosterior(c, y, Covariance(k["kind"], SIGMA2, k["phi"], tau2), m=k["m"], device=dev)
    draws = lp.sample(2, z=(z1, z2), rtol=rtol)
    assert draws.shape == (2, n)
    for t in range(2):
        eta = IB.T @ (z1[t] / np.sqrt(SIGMA2 * F)) + np.sqrt(h / tau2) * z2[t]
        ref = np.linalg.solve(A, b + eta)
        assert np.linalg.norm(draws[t] - ref) <= 2.0 * cond * rtol * np.linalg.norm(ref)


def test_sqrt_operator_squares_to_the_precision(dev):
    """S = [(I - B)^T (sigma2 F)^-1/2, d^1/2] assembled from the 2N unit vectors: S S^T = A pins the law of the
    draws (Cov(eta) = A) without a statistical threshold."""
    from pynngp_amd import _lib

    n = 64
    _, _, nbr, B, F = _field(n, 8, 2, "exponential", 6.0)
    geom = _device_geometry(dev, nbr, B, F)
    d = _random_d(np.random.default_rng(17), n)
    d_d = torch.from_numpy(d).to(dev)
    eye = torch.eye(n, dtype=torch.float64, device=dev)
    zero = torch.zeros(n, dtype=torch.float64, device=dev)
    cols = [_lib.precision_sqrt_t_apply(*geom, SIGMA2, eye[k].contiguous(), zero, d=d_d) for k in range(n)]
    cols += [_lib.precision_sqrt_t_apply(*geom, SIGMA2, zero, eye[k].contiguous(), d=d_d) for k in range(n)]
    S = torch.stack(cols, dim=1).cpu().numpy()
    A = G.precision(nbr, B, F * SIGMA2) + np.diag(d)
    assert np.abs(S @ S.T - A).max() <= 64 * U * np.abs(A).max()
    # d NULL: the prior part alone, z2 not needed
    S0 = torch.stack([_lib.precision_sqrt_t_apply(*geom, SIGMA2, eye[k].contiguous()) for k in range(n)], dim=1)
    S0 = S0.cpu().numpy()
    Q = G.precision(nbr, B, F * SIGMA2)
    assert np.abs(S0 @ S0.T - Q).max() <= 64 * U * np.abs(Q).max()


def test_philox_draws_repeat_per_seed(dev):
    from pynngp_amd import Covariance, LatentPosterior

    c, y, _, _, _ = _field(400, 8, 2, "exponential", 6.0)
    lp = LatentPosterior(c, y, Covariance("exponential", SIGMA2, 6.0, 0.1), m=8, device=dev)
    a, b, a2 = lp.sample(2, seed=1), lp.sample(2, seed=2), lp.sample(2, seed=1)
    np.testing.assert_array_equal(a, a2)
    assert not np.array_equal(a, b) and not np.array_equal(a[0], a[1])
    assert np.all(np.isfinite(a))


# ---------------------------------------------------------------- 8. GLS beta
def test_gls_beta_matches_dense(dev):
    from pynngp_amd import Covariance, LatentPosterior

    n, m, phi, tau2 = 400, 8, 6.0, 0.1
    c, z, nbr, B, F = _field(n, m, 2, "exponential", phi)
    X = np.column_stack([np.ones(n), c[:, 0]])
    y = X @ np.array([2.0, -1.0]) + 0.7 * z
    V = np.linalg.inv(G.precision(nbr, B, F * SIGMA2)) + tau2 * np.eye(n)
    assert np.linalg.cond(V) < 1e3
    Vi = np.linalg.inv(V)
    beta_ref = np.linalg.solve(X.T @ Vi @ X, X.T @ Vi @ y)
    lp = LatentPosterior(c, y, Covariance("exponential", SIGMA2, phi, tau2), m=m, X=X, device=dev)
    w, beta = lp.mean(rtol=1e-10)
    print(f"GLS beta {beta} (dense {beta_ref})")
    np.testing.assert_allclose(beta, beta_ref, rtol=1e-6, atol=0)
    _, _, w_ref, _ = G.dag_posterior(nbr, B, F, SIGMA2, tau2, np.ones(n), y - X @ beta_ref)
    np.testing.assert_allclose(w, w_ref, rtol=0, atol=1e-6 * np.abs(w_ref).max())


# ---------------------------------------------------------------- 9. wrappers
def test_nngp_wrappers_and_update(dev):
    from pynngp_amd import NNGP, Covariance, LatentPosterior

    n, m = 400, 8
    c, y, _, _, _ = _field(n, m, 2, "exponential", 6.0)
    y = y.copy()
    y[::7] = np.nan
    eps = np.random.default_rng(19).uniform(0.5, 2.0, n)
    cov = Covariance("exponential", SIGMA2, 6.0, 0.1)
    model = NNGP(c, y, eps, "S=T", m, cov, device=dev)
    w, beta = model.latent_mean()
    lp = LatentPosterior(c, y, cov, m=m, X=np.ones((n, 1)), eps=eps, device=dev)
    w_ref, beta_ref = lp.mean()
    np.testing.assert_allclose(w, w_ref, rtol=1e-12, atol=0)
    np.testing.assert_allclose(beta, beta_ref, rtol=1e-12, atol=0)
    assert model.latent_sample(2, seed=3).shape == (2, n)
    # a new theta on the same neighbour sets equals a fresh object there
    cov2 = Covariance("matern32", 0.8, 9.0, 0.3)
    w_up, beta_up = lp.update(cov2).mean()
    w_new, beta_new = LatentPosterior(c, y, cov2, m=m, X=np.ones((n, 1)), eps=eps, device=dev).mean()
    np.testing.assert_allclose(w_up, w_new, rtol=1e-12, atol=0)
    np.testing.assert_allclose(beta_up, beta_new, rtol=1e-12, atol=0)
    w2, _ = model.latent_mean(cov2)  # the wrapper follows the new theta through update()
    np.testing.assert_allclose(w2, w_new, rtol=1e-12, atol=0)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        model.latent_mean(cov2, mean="zero")
