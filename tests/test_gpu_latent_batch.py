"""GPU: the latent solver for several right-hand sides -- the batched precision operator, square-root operator
and lock-step CG (vectors (n, nrhs) row-major), diag(A), and what LatentPosterior builds on them (solve_many,
batched sample / gls_beta, marginal_variance, NNGP.latent_sd).

The contract under test: column c of every batched call is BIT-IDENTICAL to the single-RHS call on that column
alone, for every nrhs and whatever the other columns hold (the single kernels are pinned against the dense
algebra by tests/test_gpu_latent.py).  On top of that the batched results are compared with the dense algebra
of oracle/nngp_gibbs_oracle.py directly, with that file's derived bounds:
  operator  |out - A x|_i <= 4 (m + deg_i + 4) 2^-52 (|A| |x|)_i
  solves    |w - w*| <= 2 cond(A) rtol |w*|
"""
import functools
import warnings

import numpy as np
import pytest
import torch

from oracle import nngp_gibbs_oracle as G
from oracle import nngp_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
SIGMA2 = 1.3
NRHS = (1, 2, 3, 5, 8)


# ---------------------------------------------------------------- helpers (as tests/test_gpu_latent.py)
def _device_geometry(dev, nbr, B, F):
    from pynngp_amd import _lib

    nbr_d = torch.from_numpy(np.array(nbr, dtype=np.int32)).to(dev)
    B_d = torch.from_numpy(np.array(B, dtype=np.float64)).to(dev)
    F_d = torch.from_numpy(np.array(F, dtype=np.float64)).to(dev)
    off, rev_j, rev_k = _lib.reverse_neighbors(nbr_d)
    prep = _lib.gibbs_prepare(B_d, F_d, off, rev_j, rev_k)
    return nbr_d, B_d, off, rev_j, rev_k, prep


def _deg(nbr):
    return np.bincount(nbr[nbr >= 0], minlength=nbr.shape[0])


def _random_d(rng, n):
    return rng.uniform(0.1, 10.0, n) * (rng.uniform(size=n) >= 0.3)  # 30 % zeros


@functools.lru_cache(maxsize=None)
def _field(n, m, dim, kind, phi, seed=0):
    """Uniform coordinates, oracle neighbour sets and oracle unit-variance B / F (shared, read-only)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(size=(n, dim))
    y = rng.standard_normal(n)
    nbr = O.knn_prior(c, m)
    B, F, _ = O.bf_sweep(c, nbr, kind, (1.0, phi, 0.0))
    for a in (c, y, nbr, B, F):
        a.setflags(write=False)
    return c, y, nbr, B, F


def _handmade(nbr, rng):
    n, m = nbr.shape
    return rng.uniform(-0.3, 0.3, (n, m)), rng.uniform(0.1, 2.0, n)


@functools.lru_cache(maxsize=None)
def _hub():
    """Node 0 is the first parent of every other row: its reverse list has 699 entries (> 512: the block path)."""
    rng = np.random.default_rng(1)
    n, m = 700, 4
    nbr = np.full((n, m), -1, dtype=np.int32)
    for j in range(1, n):
        nbr[j, 0] = 0
        k = min(m - 1, j - 1)
        if k > 0:
            nbr[j, 1:1 + k] = 1 + rng.choice(j - 1, size=k, replace=False)
    assert _deg(nbr)[0] == n - 1 > 512
    return (nbr,) + _handmade(nbr, rng)


@functools.lru_cache(maxsize=None)
def _holes():
    """Rows whose valid slots are not a prefix (-1 in the middle), random B in the -1 slots too."""
    rng = np.random.default_rng(3)
    n, m = 300, 6
    nbr = np.full((n, m), -1, dtype=np.int32)
    for j in range(1, n):
        slots = rng.choice(m, size=int(rng.integers(1, min(m, j) + 1)), replace=False)
        nbr[j, slots] = rng.choice(j, size=len(slots), replace=False)
    assert np.any((nbr[:, :-1] < 0) & (nbr[:, 1:] >= 0))
    return (nbr,) + _handmade(nbr, rng)


def _columns(rng, n, nrhs):
    """(n, nrhs) standard normals, the columns on scales from 1e-6 to 1e6."""
    return rng.standard_normal((n, nrhs)) * 10.0 ** rng.integers(-6, 7, nrhs)


def _dt(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check_column_contract(dev, nbr, B, F, seed):
    """Every column of the two batched operators equals the single call on it, d given and d None."""
    from pynngp_amd import _lib

    n = nbr.shape[0]
    geom = _device_geometry(dev, nbr, B, F)
    rng = np.random.default_rng(seed)
    for nrhs in NRHS:
        for d in (None, _dt(_random_d(rng, n), dev)):
            X, Z2 = _dt(_columns(rng, n, nrhs), dev), _dt(_columns(rng, n, nrhs), dev)
            out = _lib.precision_apply_batch(*geom, SIGMA2, X, d=d).cpu().numpy()
            sq = _lib.precision_sqrt_t_apply_batch(*geom, SIGMA2, X, None if d is None else Z2, d=d).cpu().numpy()
            for c in range(nrhs):
                xc, zc = X[:, c].contiguous(), Z2[:, c].contiguous()
                np.testing.assert_array_equal(out[:, c], _lib.precision_apply(*geom, SIGMA2, xc, d=d).cpu().numpy(),
                                              err_msg=f"apply n={n} nrhs={nrhs} column {c}")
                ref = _lib.precision_sqrt_t_apply(*geom, SIGMA2, xc, None if d is None else zc, d=d).cpu().numpy()
                np.testing.assert_array_equal(sq[:, c], ref, err_msg=f"sqrt n={n} nrhs={nrhs} column {c}")


# ---------------------------------------------------------------- 1. column contract, operator
@pytest.mark.parametrize("n,m,dim", [(1, 1, 2), (2, 1, 1), (16, 15, 2), (257, 32, 2), (400, 4, 2), (400, 8, 2),
                                     (130, 63, 2)])
def test_operator_columns_equal_single_calls(dev, n, m, dim):
    _, _, nbr, B, F = _field(n, m, dim, "exponential", 6.0)
    _check_column_contract(dev, nbr, B, F, n + m)


def test_operator_columns_equal_single_calls_hub(dev):
    _check_column_contract(dev, *_hub(), 21)


def test_operator_columns_equal_single_calls_holes(dev):
    _check_column_contract(dev, *_holes(), 22)


# ---------------------------------------------------------------- 2. operator against the dense matrix
@pytest.mark.parametrize("which", ["field_257_32", "hub"])
def test_batched_operator_matches_dense_precision(dev, which):
    from pynngp_amd import _lib

    nbr, B, F = _field(257, 32, 2, "exponential", 6.0)[2:] if which == "field_257_32" else _hub()
    n, m = nbr.shape
    geom = _device_geometry(dev, nbr, B, F)
    Q = G.precision(nbr, B, F * SIGMA2)
    deg = _deg(nbr)
    rng = np.random.default_rng(31)
    for d in (None, _random_d(rng, n)):
        A = Q if d is None else Q + np.diag(d)
        X = rng.standard_normal((n, 8))
        out = _lib.precision_apply_batch(*geom, SIGMA2, _dt(X, dev), d=_dt(d, dev)).cpu().numpy()
        bound = 4.0 * (m + deg + 4)[:, None] * U * (np.abs(A) @ np.abs(X))
        err = np.abs(out - A @ X)
        print(f"{which} d={'yes' if d is not None else 'no'}: max err/bound "
              f"{(err / np.maximum(bound, 1e-300)).max():.3g}")
        assert np.all(err <= bound)


# ---------------------------------------------------------------- 3./4. column contract, CG
@functools.lru_cache(maxsize=None)
def _posterior_400(dev):
    """LatentPosterior on (400, 8, 2) with 30 % unobserved responses (d = 0 there)."""
    from pynngp_amd import Covariance, LatentPosterior

    c, y, _, _, _ = _field(400, 8, 2, "exponential", 6.0)
    y = y.copy()
    y[np.random.default_rng(11).uniform(size=400) < 0.3] = np.nan
    lp = LatentPosterior(c, y, Covariance("exponential", SIGMA2, 6.0, 0.1), m=8, device=dev)
    assert 0.2 < float((lp.d == 0).double().mean()) < 0.4
    return lp


def _single_solves(lp, Bm, X0, rtol, max_iter, check_every):
    from pynngp_amd import _lib

    xs, infos = [], []
    for c in range(Bm.shape[1]):
        x, info = _lib.latent_cg(*lp._geom(), Bm[:, c].contiguous(), X0[:, c].contiguous(), d=lp.d, rtol=rtol,
                                 max_iter=max_iter, check_every=check_every)
        xs.append(x.cpu().numpy())
        infos.append(info)
    return np.stack(xs, axis=1), np.array(infos)


@pytest.mark.parametrize("check_every", [1, 8])
def test_cg_columns_equal_single_solves(dev, check_every):
    """Columns that finish at different iterations: b = 0 (0 iterations, converged), a start at a converged
    solution, random columns on scales 1e-6 .. 1e6.  x, iterations, status, |r|^2 and |b|^2 equal the single
    solve exactly; then max_iter = 5 on random columns, where none converges and all report 5."""
    from pynngp_amd import _lib

    lp = _posterior_400(dev)
    n, rng = lp.n, np.random.default_rng(41)
    Bh = _columns(rng, n, 8)
    Bh[:, 0] = 0.0
    Bm = _dt(Bh, dev)
    X0 = torch.zeros_like(Bm)
    X0[:, 1] = _lib.latent_cg(*lp._geom(), Bm[:, 1].contiguous(), torch.zeros(n, dtype=torch.float64, device=dev),
                              d=lp.d, rtol=1e-8, max_iter=1000)[0]
    ref_x, ref_info = _single_solves(lp, Bm, X0, 1e-8, 1000, check_every)
    x, info = _lib.latent_cg_batch(*lp._geom(), Bm, X0.clone(), d=lp.d, rtol=1e-8, max_iter=1000,
                                   check_every=check_every)
    print("iterations per column", info[:, 0].astype(int).tolist())
    np.testing.assert_array_equal(info, ref_info)
    np.testing.assert_array_equal(x.cpu().numpy(), ref_x)
    assert info[0].tolist() == [0.0, 1.0, 0.0, 0.0] and np.all(x[:, 0].cpu().numpy() == 0.0)
    assert np.all(info[:, 1] == 1.0) and len(set(info[:, 0])) >= 2

    Bm = _dt(_columns(rng, n, 8), dev)
    X0 = torch.zeros_like(Bm)
    ref_x, ref_info = _single_solves(lp, Bm, X0, 1e-10, 5, check_every)
    x, info = _lib.latent_cg_batch(*lp._geom(), Bm, X0.clone(), d=lp.d, rtol=1e-10, max_iter=5,
                                   check_every=check_every)
    np.testing.assert_array_equal(info, ref_info)
    np.testing.assert_array_equal(x.cpu().numpy(), ref_x)
    assert np.all(info[:, 0] == 5.0) and np.all(info[:, 1] == 0.0)


def test_breakdown_stays_in_its_column(dev):
    from pynngp_amd import NNGPNumericalError, _lib

    lp = _posterior_400(dev)
    n, rng = lp.n, np.random.default_rng(43)
    Bh = rng.standard_normal((n, 5))
    Bh[17, 2] = np.nan
    Bm = _dt(Bh, dev)
    X0 = torch.zeros_like(Bm)
    x, info = _lib.latent_cg_batch(*lp._geom(), Bm, X0.clone(), d=lp.d, rtol=1e-8, max_iter=1000)
    assert info[2, 1] == -1.0 and np.all(info[[0, 1, 3, 4], 1] == 1.0)
    good = [0, 1, 3, 4]
    ref_x, ref_info = _single_solves(lp, Bm[:, good].contiguous(), X0[:, good].contiguous(), 1e-8, 1000, 8)
    np.testing.assert_array_equal(x.cpu().numpy()[:, good], ref_x)
    np.testing.assert_array_equal(info[good], ref_info)
    # the broken column as the single solver leaves it
    _, bad_info = _lib.latent_cg(*lp._geom(), Bm[:, 2].contiguous(), X0[:, 2].contiguous(), d=lp.d, rtol=1e-8,
                                 max_iter=1000)
    assert bad_info[0] == info[2, 0] and bad_info[1] == -1.0
    with pytest.raises(NNGPNumericalError, match=r"column\(s\) \[2\]"):
        lp.solve_many(Bh.T)


# ---------------------------------------------------------------- 5. grid-stride paths
def test_cg_columns_equal_single_solves_beyond_the_grids(dev):
    """n = 270,000 > 1024 * 256 and > 2048 * 16: every kernel walks more than one tile / stride per block.  No
    dense reference at this size: the single solver (pinned by tests/test_gpu_latent.py) is the yardstick."""
    from pynngp_amd import _lib

    rng = np.random.default_rng(51)
    n, m = 270_000, 4
    offs = rng.permuted(np.tile(np.arange(1, 65, dtype=np.int32), (n, 1)), axis=1)[:, :m]
    nbr = np.arange(n, dtype=np.int32)[:, None] - offs
    nbr[nbr < 0] = -1
    B, F = rng.uniform(-0.2, 0.2, (n, m)), rng.uniform(0.5, 2.0, n)
    geom = _device_geometry(dev, nbr, B, F)
    d = _dt(rng.uniform(0.1, 1.0, n), dev)
    Bm = _dt(_columns(rng, n, 3), dev)
    x, info = _lib.latent_cg_batch(*geom, SIGMA2, Bm, torch.zeros_like(Bm), d=d, rtol=1e-8, max_iter=24)
    print("n=270000:", info.tolist())
    assert np.all(np.isfinite(info)) and np.all(info[:, 1] >= 0)
    for c in range(3):
        xc, ic = _lib.latent_cg(*geom, SIGMA2, Bm[:, c].contiguous(), torch.zeros(n, dtype=torch.float64, device=dev),
                                d=d, rtol=1e-8, max_iter=24)
        assert ic == info[c].tolist()
        assert torch.equal(x[:, c], xc)


# ---------------------------------------------------------------- 6. batched solutions against the dense posterior
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
def test_solve_many_matches_dense_posterior(dev, name):
    from pynngp_amd import Covariance, LatentPosterior

    k, c, y, nbr, B, F, h = _case(name)
    rtol = 1e-10
    A, b, _, _ = G.dag_posterior(nbr, B, F, SIGMA2, k["tau2"], h, np.where(h > 0, y, 0.0))
    cond = np.linalg.cond(A)
    rng = np.random.default_rng(61)
    rhs = np.vstack([b, rng.standard_normal((4, k["n"])) * 10.0 ** rng.integers(-3, 4, 4)[:, None]])
    ref = np.linalg.solve(A, rhs.T).T
    lp = LatentPosterior(c, y, Covariance(k["kind"], SIGMA2, k["phi"], k["tau2"]), m=k["m"], device=dev)
    x, infos = lp.solve_many(rhs, rtol=rtol)
    assert x.shape == rhs.shape and len(infos) == 5
    for r in range(5):
        err = np.linalg.norm(x[r] - ref[r]) / np.linalg.norm(ref[r])
        print(f"{name} row {r}: {infos[r].iterations} iterations, rel err {err:.3g} (bound {2 * cond * rtol:.3g})")
        assert infos[r].converged and infos[r].residual2 <= rtol * rtol * infos[r].rhs2
        assert err <= 2.0 * cond * rtol
    # row k is solve(rhs[k]) bit for bit, whatever the chunking; K = 0 is served
    for batch in (2, 8):
        xb, ib = lp.solve_many(rhs, rtol=rtol, batch=batch)
        np.testing.assert_array_equal(xb, x)
        assert ib == infos
    x1, i1 = lp.solve(rhs[3], rtol=rtol)
    np.testing.assert_array_equal(x[3], x1)
    assert infos[3] == i1
    x0, i0 = lp.solve_many(np.zeros((0, k["n"])))
    assert x0.shape == (0, k["n"]) and i0 == []


def test_solve_many_names_the_rows_that_did_not_converge(dev):
    lp = _posterior_400(dev)
    rhs = np.random.default_rng(63).standard_normal((3, lp.n))
    rhs[1] = 0.0
    with pytest.warns(RuntimeWarning, match=r"column\(s\) \[0, 2\]") as rec:
        _, infos = lp.solve_many(rhs, rtol=1e-12, max_iter=3)
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert [si.converged for si in infos] == [False, True, False] and [si.iterations for si in infos] == [3, 0, 3]


# ---------------------------------------------------------------- 7. diag(A)
@pytest.mark.parametrize("which", ["field_400_8", "hub"])
def test_precision_diag_matches_dense(dev, which):
    from pynngp_amd import _lib

    nbr, B, F = _field(400, 8, 2, "exponential", 6.0)[2:] if which == "field_400_8" else _hub()
    n, m = nbr.shape
    prep = _device_geometry(dev, nbr, B, F)[5]
    Q = G.precision(nbr, B, F * SIGMA2)
    for d in (None, _random_d(np.random.default_rng(71), n)):
        ref = np.diag(Q) + (0.0 if d is None else d)
        got = _lib.precision_diag(prep, n, m, SIGMA2, d=_dt(d, dev)).cpu().numpy()
        assert np.all(np.abs(got - ref) <= 8 * U * ref)


# ---------------------------------------------------------------- 8. marginal variance, given normals
def test_marginal_variance_with_given_normals_matches_dense(dev):
    """The estimator v_i = 1 / A_ii + sum_k (c_i^(k) - c_bar_i)^2 / (K - 1), c^(k) = w^(k) - (A w^(k) - b) / diag(A),
    evaluated in numpy on the dense A with the same normals.

    Tolerance.  The solver's bound gives ||dw^(k)|| <= eps ||w^(k)||, eps = 2 cond(A) rtol.  b cancels in
    dc = dw - (A dw) / diag(A), so |dc_i| <= ||dw|| (1 + ||A||_2 / min_i A_ii); the operator's own rounding adds
    at most 4 (m + deg_i + 4) u (|A| |w| + |b|)_i / A_ii.  Let delta be the largest such |dc_i| over draws and
    locations.  A deviation e = c - c_bar moves by at most 2 delta, so sum_k e^2 moves by at most
    4 delta sum_k |e_i^(k)| + 4 K delta^2, which is divided by K - 1; 1 / A_ii and the final sums add a few ulp
    of v_i (16 u v_i allowed).
    """
    from pynngp_amd import Covariance, LatentPosterior

    n, m, K, rtol, tau2 = 300, 8, 6, 1e-10, 0.1
    c, y, nbr, B, F = _field(n, m, 2, "exponential", 6.0)
    A, b, _, _ = G.dag_posterior(nbr, B, F, SIGMA2, tau2, np.ones(n), y)
    rng = np.random.default_rng(81)
    z1, z2 = rng.standard_normal((K, n)), rng.standard_normal((K, n))
    IB = np.eye(n) - G.dense_B(nbr, B)
    eta = (z1 / np.sqrt(SIGMA2 * F)) @ IB + np.sqrt(1.0 / tau2) * z2  # rows: (I - B)^T (sigma2 F)^-1/2 z1 + d^1/2 z2
    W = np.linalg.solve(A, (b + eta).T).T
    aii = np.diag(A)
    C = W - (W @ A - b) / aii
    E = C - C.mean(axis=0)
    ref = 1.0 / aii + (E ** 2).sum(axis=0) / (K - 1)

    eps = 2.0 * np.linalg.cond(A) * rtol
    dw = eps * np.linalg.norm(W, axis=1).max()
    rounding = (4.0 * (m + _deg(nbr) + 4) * U * (np.abs(W) @ np.abs(A) + np.abs(b)) / aii).max()
    delta = dw * (1.0 + np.linalg.norm(A, 2) / aii.min()) + rounding
    tol = (4.0 * delta * np.abs(E).sum(axis=0) + 4.0 * K * delta ** 2) / (K - 1) + 16 * U * ref

    lp = LatentPosterior(c, y, Covariance("exponential", SIGMA2, 6.0, tau2), m=m, device=dev)
    v = lp.marginal_variance(K, z=(z1, z2), rtol=rtol)
    assert v.shape == (n,)
    print(f"marginal variance: max |v - ref| / tol {(np.abs(v - ref) / tol).max():.3g}, "
          f"max tol / ref {(tol / ref).max():.3g}")
    assert np.all(np.abs(v - ref) <= tol)
    # the sums run draw by draw in draw order: the chunking changes nothing
    np.testing.assert_array_equal(lp.marginal_variance(K, z=(z1, z2), rtol=rtol, batch=4), v)
    np.testing.assert_array_equal(lp.marginal_variance(K, z=(z1, z2), rtol=rtol, batch=1), v)


# ---------------------------------------------------------------- 9. statistical sanity
def test_marginal_variance_is_the_posterior_variance(dev):
    """Philox normals, K = 256: |v_i / (A^-1)_ii - 1| <= 6 sqrt(2 / (K - 1)) at every location -- the estimator's
    deviation is that of a scaled chi^2_{K-1} on a part of the variance, so at most that relative standard
    deviation; 6 sigma over 300 locations leaves no realistic false alarm.  Wide on purpose: it catches a missing
    1 / A_ii, a wrong ddof or mixed-up columns, not rounding."""
    from pynngp_amd import Covariance, LatentPosterior

    n, m, K, tau2 = 300, 8, 256, 0.1
    c, y, nbr, B, F = _field(n, m, 2, "exponential", 6.0)
    A, _, _, _ = G.dag_posterior(nbr, B, F, SIGMA2, tau2, np.ones(n), y)
    ref = np.diag(np.linalg.inv(A))
    lp = LatentPosterior(c, y, Covariance("exponential", SIGMA2, 6.0, tau2), m=m, device=dev)
    v = lp.marginal_variance(K, seed=5)
    dev_rel = np.abs(v / ref - 1.0)
    print(f"K={K}: max |v / (A^-1)_ii - 1| = {dev_rel.max():.3g} (bound {6 * np.sqrt(2 / (K - 1)):.3g})")
    assert np.all(dev_rel <= 6.0 * np.sqrt(2.0 / (K - 1)))


# ---------------------------------------------------------------- 10. gls_beta and sample through the batched path
@pytest.mark.parametrize("batch", [1, 3, 8])
def test_gls_beta_and_sample_equal_loops_of_single_solves(dev, batch):
    from pynngp_amd import Covariance, LatentPosterior, _lib

    n, m = 400, 8
    c, zv, _, _, _ = _field(n, m, 2, "exponential", 6.0)
    X = np.column_stack([np.ones(n), c[:, 0], c[:, 1], c[:, 0] ** 2, c[:, 0] * c[:, 1]])
    y = X @ np.array([2.0, -1.0, 0.5, 0.3, -0.7]) + 0.7 * zv
    lp = LatentPosterior(c, y, Covariance("exponential", SIGMA2, 6.0, 0.1), m=m, X=X, device=dev)
    # GLS beta from one single solve per column of X, assembled as before the batched solver existed
    S = torch.stack([lp._solve((lp.d * lp.X[:, k]).contiguous(), 1e-8, None)[0] for k in range(lp.p)], dim=1)
    Wm = lp.d[:, None] * (lp.X - S)
    Gm = (lp.X.t() @ Wm).cpu().numpy()
    beta_ref = np.linalg.solve(0.5 * (Gm + Gm.T), (Wm.t() @ lp.y).cpu().numpy())
    beta = lp.gls_beta(batch=batch)
    np.testing.assert_array_equal(beta, beta_ref)
    # 5 draws: Philox streams 2k, 2k + 1, the single square-root operator and the single solver per draw
    b = lp._rhs(beta_ref)
    ref = np.empty((5, n))
    z1, z2 = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    for k in range(5):
        _lib.gibbs_normals(z1, 3, 2 * k)
        _lib.gibbs_normals(z2, 3, 2 * k + 1)
        eta = _lib.precision_sqrt_t_apply(*lp._geom(), z1, z2, d=lp.d)
        ref[k] = lp._solve(b + eta, 1e-8, None)[0][lp.pos].cpu().numpy()
    np.testing.assert_array_equal(lp.sample(5, seed=3, beta=beta_ref, batch=batch), ref)


# ---------------------------------------------------------------- 11. torch ops
def test_torch_ops_match_the_binding_and_repeat(dev):
    from pynngp_amd import _lib, load_ops

    load_ops()
    _, _, nbr, B, F = _field(400, 8, 2, "exponential", 6.0)
    geom = _device_geometry(dev, nbr, B, F)
    rng = np.random.default_rng(91)
    X = _dt(_columns(rng, 400, 5), dev)
    d = _dt(_random_d(rng, 400) + 0.5, dev)
    out = _lib.precision_apply_batch(*geom, SIGMA2, X, d=d)
    assert torch.equal(torch.ops.nngp.precision_apply_batch(*geom, SIGMA2, d, X), out)
    assert torch.equal(_lib.precision_apply_batch(*geom, SIGMA2, X, d=d), out)
    assert torch.equal(torch.ops.nngp.precision_apply_batch(*geom, SIGMA2, None, X),
                       _lib.precision_apply_batch(*geom, SIGMA2, X))
    xs, info = torch.ops.nngp.latent_cg_batch(*geom, SIGMA2, d, X, None, 1e-9, 500, 8)
    ref, info_ref = _lib.latent_cg_batch(*geom, SIGMA2, X, torch.zeros_like(X), d=d, rtol=1e-9, max_iter=500)
    assert torch.equal(xs, ref) and np.array_equal(info.numpy(), info_ref) and np.all(info_ref[:, 1] == 1.0)
    assert info.device.type == "cpu" and tuple(info.shape) == (5, 4)
    again, info_again = _lib.latent_cg_batch(*geom, SIGMA2, X, torch.zeros_like(X), d=d, rtol=1e-9, max_iter=500)
    assert torch.equal(again, ref) and np.array_equal(info_again, info_ref)
    x0 = ref * 0.5
    xs, info = torch.ops.nngp.latent_cg_batch(*geom, SIGMA2, d, X, x0, 1e-9, 500, 8)
    ref0, info0 = _lib.latent_cg_batch(*geom, SIGMA2, X, x0.clone(), d=d, rtol=1e-9, max_iter=500)
    assert torch.equal(xs, ref0) and np.array_equal(info.numpy(), info0)


# ---------------------------------------------------------------- 12. the NNGP wrapper
def test_nngp_latent_sd(dev):
    from pynngp_amd import NNGP, Covariance

    n, m = 400, 8
    c, y, _, _, _ = _field(n, m, 2, "exponential", 6.0)
    y = y.copy()
    y[::7] = np.nan
    model = NNGP(c, y, None, "S=T", m, Covariance("exponential", SIGMA2, 6.0, 0.1), device=dev)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        sd = model.latent_sd(16, seed=2)
    assert sd.shape == (n,) and np.all(np.isfinite(sd)) and np.all(sd > 0)
    # unobserved locations are less certain than their observed neighbours on average
    assert sd[::7].mean() > np.delete(sd, np.arange(0, n, 7)).mean()
    np.testing.assert_array_equal(model.latent_sd(16, seed=2), sd)
