"""CPU: the reference-set (S != T) latent entry points -- nngp_precision_ref_*, nngp_latent_ref_cg_batch,
nngp_latent_ref_leaves_batch -- are exported and bound, reject bad arguments before any GPU call and size their
workspaces sanely; the Python layer refuses what it does not serve; and the algebra the kernels implement (the
leaves integrated out in closed form) is the S-marginal of the dense posterior over all nodes."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import nngp_gibbs_oracle as G
from oracle import nngp_oracle as O

NEW = ("nngp_precision_ref_batch_workspace_bytes", "nngp_precision_ref_apply_batch",
       "nngp_precision_ref_sqrt_t_apply_batch", "nngp_precision_ref_fold_batch", "nngp_precision_ref_diag",
       "nngp_latent_ref_cg_batch_workspace_bytes", "nngp_latent_ref_cg_batch", "nngp_latent_ref_leaves_batch")


@pytest.fixture(scope="module")
def lib():
    from pynngp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build()")
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    from pynngp_amd import _lib

    for s in NEW:
        assert s in _lib.SYMBOLS, s
        fn = getattr(lib, s)
        assert fn.argtypes is not None, s
    assert lib.nngp_abi_version() == 4  # pure additions


P = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731

# fake non-null, 256-byte aligned "device" addresses: every case below must fail before any launch
GEOM = dict(nbr=256, B=256, off=256, rev_j=256, rev_k=256, prep=256, n=10, n_s=4, m=4, sigma2=1.0, d=None, nrhs=3,
            workspace=256, workspace_bytes=1 << 20)


def _head(a):
    return (P(a["nbr"]), P(a["B"]), P(a["off"]), P(a["rev_j"]), P(a["rev_k"]), P(a["prep"]), a["n"], a["n_s"], a["m"],
            a["sigma2"], P(a["d"]))


def _apply(lib, **kw):
    a = dict(GEOM, x=256, out=512)
    a.update(kw)
    return lib.nngp_precision_ref_apply_batch(*_head(a), a["nrhs"], P(a["x"]), P(a["out"]), P(a["workspace"]),
                                              a["workspace_bytes"], None)


def _sqrt(lib, **kw):
    a = dict(GEOM, z1=256, z2=256, out=512)
    a.update(kw)
    return lib.nngp_precision_ref_sqrt_t_apply_batch(*_head(a), a["nrhs"], P(a["z1"]), P(a["z2"]), P(a["out"]),
                                                     P(a["workspace"]), a["workspace_bytes"], None)


def _fold(lib, **kw):
    a = dict(GEOM, v=256, out=512)
    a.update(kw)
    return lib.nngp_precision_ref_fold_batch(*_head(a), a["nrhs"], P(a["v"]), P(a["out"]), P(a["workspace"]),
                                             a["workspace_bytes"], None)


def _diag(lib, **kw):
    a = dict(GEOM, out=512)
    a.update(kw)
    return lib.nngp_precision_ref_diag(*_head(a), P(a["out"]), P(a["workspace"]), a["workspace_bytes"], None)


def _cg(lib, **kw):
    a = dict(GEOM, b=256, x=512, rtol=1e-8, max_iter=10, check_every=8)
    a.update(kw)
    info = (ctypes.c_double * 32)() if a.get("info", True) else None
    return lib.nngp_latent_ref_cg_batch(*_head(a), a["nrhs"], P(a["b"]), P(a["x"]), a["rtol"], a["max_iter"],
                                        a["check_every"], info, P(a["workspace"]), a["workspace_bytes"], None)


def _leaves(lib, **kw):
    a = dict(GEOM, x=256, v=None, z=None, out=512)
    a.update(kw)
    return lib.nngp_latent_ref_leaves_batch(*_head(a), a["nrhs"], P(a["x"]), P(a["v"]), P(a["z"]), P(a["out"]), None)


COMMON_BAD = [
    (dict(nbr=None), "non-null"),
    (dict(B=None), "non-null"),
    (dict(prep=None), "non-null"),
    (dict(n=-1), "n_s"),
    (dict(n_s=-1), "n_s"),
    (dict(n_s=11), "n_s"),
    (dict(m=0), "m=0"),
    (dict(m=64), "m=64"),
    (dict(sigma2=0.0), "sigma2"),
    (dict(sigma2=float("nan")), "sigma2"),
    (dict(prep=264), "aligned"),
]
WITH_WS_BAD = [
    (dict(off=None), "non-null"),
    (dict(rev_j=None), "non-null"),
    (dict(workspace=None), "non-null"),
    (dict(workspace_bytes=16), "workspace too small"),
    (dict(workspace=264), "aligned"),
]
NRHS_BAD = [(dict(nrhs=0), "nrhs"), (dict(nrhs=9), "nrhs"), (dict(nrhs=-1), "nrhs")]


@pytest.mark.parametrize("call", [_apply, _sqrt, _fold, _diag, _cg, _leaves])
@pytest.mark.parametrize("kw,msg", COMMON_BAD)
def test_bad_geometry_is_einval(lib, call, kw, msg):
    assert call(lib, **kw) == -1, (call.__name__, kw)
    assert msg in lib.nngp_last_error().decode()


@pytest.mark.parametrize("call", [_apply, _sqrt, _fold, _diag, _cg])
@pytest.mark.parametrize("kw,msg", WITH_WS_BAD)
def test_bad_workspace_is_einval(lib, call, kw, msg):
    assert call(lib, **kw) == -1, (call.__name__, kw)
    assert msg in lib.nngp_last_error().decode()


@pytest.mark.parametrize("call", [_apply, _sqrt, _fold, _cg, _leaves])
@pytest.mark.parametrize("kw,msg", NRHS_BAD)
def test_bad_nrhs_is_einval(lib, call, kw, msg):
    assert call(lib, **kw) == -1, (call.__name__, kw)
    assert msg in lib.nngp_last_error().decode()


@pytest.mark.parametrize("call,kw,msg", [
    (_apply, dict(x=None), "non-null"),
    (_apply, dict(out=None), "non-null"),
    (_apply, dict(out=256), "alias"),
    (_sqrt, dict(z1=None), "non-null"),
    (_sqrt, dict(out=256), "alias"),
    (_sqrt, dict(d=256, z2=None), "z2"),
    (_fold, dict(v=None), "non-null"),
    (_fold, dict(out=256), "alias"),
    (_diag, dict(out=None), "non-null"),
    (_cg, dict(b=None), "non-null"),
    (_cg, dict(x=256), "alias"),
    (_cg, dict(info=False), "non-null"),
    (_cg, dict(rtol=0.0), "rtol"),
    (_cg, dict(rtol=1.0), "rtol"),
    (_cg, dict(max_iter=-1), "max_iter"),
    (_cg, dict(check_every=0), "check_every"),
    (_leaves, dict(x=None), "non-null"),
    (_leaves, dict(out=None), "non-null"),
    (_leaves, dict(out=256), "alias"),
    (_leaves, dict(v=512), "alias"),
])
def test_call_specific_bad_arguments(lib, call, kw, msg):
    assert call(lib, **kw) == -1, (call.__name__, kw)
    assert msg in lib.nngp_last_error().decode()


def test_workspace_sizes(lib):
    n = 10 ** 6
    for fn, old in ((lib.nngp_latent_ref_cg_batch_workspace_bytes, lib.nngp_latent_cg_batch_workspace_bytes),
                    (lib.nngp_precision_ref_batch_workspace_bytes, lib.nngp_precision_batch_workspace_bytes)):
        for bad in (0, 9, -1):
            assert fn(1000, 10, bad) == 0
        for n_s in (-1, 1001):
            assert fn(1000, n_s, 1) == 0
        assert fn(-1, 0, 1) == 0 and fn(-1, -1, 1) == 0
        n_ss = (0, 1, 31, 1000, 10 ** 5, n - 1, n)
        table = np.array([[fn(n, n_s, k) for k in range(1, 9)] for n_s in n_ss], dtype=np.int64)
        assert np.all(table % 256 == 0) and np.all(table > 0)
        assert np.all(np.diff(table, axis=0) >= 0) and np.all(np.diff(table, axis=1) >= 0)  # monotone in n_s, nrhs
        for k in range(1, 9):
            assert fn(n, n, k) >= old(n, k)  # n_s = n is served by the S = T call
    for k in range(1, 9):
        # the solver's vectors have n_s rows: one (n, k) and four (n_s, k), against six (n, k)
        small = lib.nngp_latent_ref_cg_batch_workspace_bytes(n, n // 10, k)
        assert small >= 8 * (n * k + 4 * (n // 10) * k)
        assert small < 0.5 * lib.nngp_latent_cg_batch_workspace_bytes(n, k)


# ---------------------------------------------------------------- Python refusals (no GPU needed)
def _cpu_geometry(n=6, m=2):
    nbr = torch.full((n, m), -1, dtype=torch.int32)
    B = torch.zeros((n, m), dtype=torch.float64)
    off = torch.zeros(n + 1, dtype=torch.int32)
    rev = torch.zeros(n * m, dtype=torch.int32)
    prep = torch.zeros(1 << 16, dtype=torch.uint8)
    return nbr, B, off, rev, rev.clone(), prep


def test_lib_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from pynngp_amd import _lib

    g = _cpu_geometry()
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.precision_ref_apply_batch(*g, 4, 1.0, f64(4, 3))
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.precision_ref_sqrt_t_apply_batch(*g, 4, 1.0, f64(6, 3))
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.precision_ref_fold_batch(*g, 4, 1.0, f64(6, 3))
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.precision_ref_diag(*g, 4, 1.0)
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.latent_ref_cg_batch(*g, 4, 1.0, f64(4, 2), f64(4, 2))
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.latent_ref_leaves_batch(*g, 4, 1.0, f64(4, 2))
    for n_s in (-1, 7):
        with pytest.raises(ValueError, match="n_s"):
            _lib.precision_ref_apply_batch(*g, n_s, 1.0, f64(4, 3))
    # vectors on S have n_s rows, vectors on all nodes n, vectors on the leaves n - n_s; 1 <= nrhs <= 8
    for bad in (f64(6, 3), f64(4, 9), f64(4, 0), f64(4), torch.zeros((4, 3), dtype=torch.float32), f64(3, 4).t()):
        with pytest.raises(ValueError):
            _lib.precision_ref_apply_batch(*g, 4, 1.0, bad)
        with pytest.raises(ValueError):
            _lib.latent_ref_cg_batch(*g, 4, 1.0, bad, f64(4, 3))
        with pytest.raises(ValueError):
            _lib.latent_ref_leaves_batch(*g, 4, 1.0, bad)
    with pytest.raises(ValueError):
        _lib.precision_ref_sqrt_t_apply_batch(*g, 4, 1.0, f64(4, 3))  # z1 is per node
    with pytest.raises(ValueError):
        _lib.precision_ref_sqrt_t_apply_batch(*g, 4, 1.0, f64(6, 3), z2=f64(6, 3))  # z2 is per reference point
    with pytest.raises(ValueError):
        _lib.precision_ref_fold_batch(*g, 4, 1.0, f64(4, 3))
    with pytest.raises(ValueError):
        _lib.precision_ref_fold_batch(*g, 4, 1.0, f64(6, 3), out=f64(6, 3))
    with pytest.raises(ValueError):
        _lib.latent_ref_leaves_batch(*g, 4, 1.0, f64(4, 3), v=f64(4, 3))  # v is per leaf
    with pytest.raises(ValueError):
        _lib.latent_ref_leaves_batch(*g, 4, 1.0, f64(4, 3), z=f64(2, 2))
    with pytest.raises(ValueError):
        _lib.precision_ref_apply_batch(*g, 4, 1.0, f64(4, 3), d=f64(4))  # d is per node
    with pytest.raises(ValueError):
        _lib.precision_ref_diag(*g, 4, 1.0, out=f64(6))


def test_latent_posterior_ref_argument_errors():
    """Everything here is refused before a device is touched."""
    from pynngp_amd import Covariance, LatentPosterior

    cov = Covariance("exponential", 1.0, 6.0, 0.1)
    rng = np.random.default_rng(0)
    t, y, s = rng.uniform(size=(12, 2)), rng.standard_normal(12), rng.uniform(size=(5, 2))
    with pytest.raises(ValueError, match="dimension"):
        LatentPosterior(t, y, cov, m=3, ref=rng.uniform(size=(5, 3)))
    with pytest.raises(ValueError, match="ref must be"):
        LatentPosterior(t, y, cov, m=3, ref=np.zeros((0, 2)))
    with pytest.raises(ValueError, match="ref must be"):
        LatentPosterior(t, y, cov, m=3, ref=np.full((5, 2), np.nan))
    with pytest.raises(ValueError, match="X_ref"):
        LatentPosterior(t, y, cov, m=3, X=np.ones((12, 1)), ref=s, X_ref=np.ones((4, 1)))
    with pytest.raises(ValueError, match="X_ref"):
        LatentPosterior(t, y, cov, m=3, X=np.ones((12, 1)), X_ref=np.ones((5, 1)))
    with pytest.raises(ValueError, match="nbr"):
        LatentPosterior(t, y, cov, m=3, ref=s, nbr=torch.zeros((12, 3), dtype=torch.int32))


def _hollow_ref_posterior(n=7, n_s=3):
    from pynngp_amd import LatentPosterior

    lp = LatentPosterior.__new__(LatentPosterior)
    lp._ref = True
    lp.n, lp.n_nodes, lp.n_s, lp.p, lp.m = n, n, n_s, 0, 2
    lp.device = torch.device("cpu")
    lp.perm = lp.pos = torch.arange(n)
    lp.perm_s = lp.slot_of_ref = torch.arange(n_s)
    return lp


def test_ref_posterior_vector_and_where_errors():
    lp = _hollow_ref_posterior()
    for call in (lp.mean, lambda where: lp.sample(2, where=where), lambda where: lp.marginal_variance(4, where=where)):
        with pytest.raises(ValueError, match="where"):
            call(where="leaves")
    with pytest.raises(ValueError, match=r"\(3,\)"):  # the solver's vectors live on S
        lp.solve(np.zeros(7))
    with pytest.raises(ValueError, match=r"\(K, 3\)"):
        lp.solve_many(np.zeros((2, 7)))
    with pytest.raises(ValueError, match=r"\(3,\)"):
        lp.matvec(np.zeros(7))
    with pytest.raises(ValueError, match="n_draws"):
        lp.predict(np.zeros((2, 2)), n_draws=-1)
    with pytest.raises(ValueError, match="batch"):
        lp.predict(np.zeros((2, 2)), batch=9)


def test_nngp_latent_posterior_checks_mean_before_any_device_work():
    from pynngp_amd import NNGP, Covariance

    obj = NNGP.__new__(NNGP)
    obj.refType = ("subset", 5)
    obj.cov = Covariance("exponential", 1.0, 6.0, 0.1)
    with pytest.raises(ValueError, match="mean"):
        obj.latent_posterior(mean="linear")
    with pytest.raises(NotImplementedError, match="S=T"):  # the S = T conveniences stay as they were
        obj.latent_mean()


# ---------------------------------------------------------------- the algebra, densely
def dense_ref_system(nbr, B, F, n_s, sigma2, d, v):
    """A_S, b_S, diag(A_S), L = [(I - B_S); -B_L] and the row scale s, from the issue's formulas."""
    n = nbr.shape[0]
    Bd = G.dense_B(nbr, B)
    L = np.concatenate([np.eye(n_s) - Bd[:n_s, :n_s], -Bd[n_s:, :n_s]])
    f = 1.0 / (sigma2 * F)
    g = np.where(d[n_s:] > 0, f[n_s:] * d[n_s:] / (f[n_s:] + d[n_s:]), 0.0)
    s = np.concatenate([f[:n_s], g])
    A = L.T @ (s[:, None] * L) + np.diag(d[:n_s])
    b = d[:n_s] * v[:n_s] + Bd[n_s:, :n_s].T @ (g * v[n_s:])
    diag = d[:n_s] + f[:n_s] + (Bd[:, :n_s] ** 2 * s[:, None]).sum(axis=0)
    return A, b, diag, L, s


@pytest.mark.parametrize("n_s,n_out,m,dim", [(30, 80, 5, 2), (3, 20, 5, 2), (1, 10, 1, 2), (20, 0, 4, 2),
                                             (25, 60, 6, 1), (25, 60, 6, 3)])
def test_eliminated_system_is_the_s_marginal_of_the_dense_posterior(n_s, n_out, m, dim):
    rng = np.random.default_rng(100 * n_s + n_out)
    coords, nbr = G.reference_dag(rng.uniform(size=(n_s, dim)), rng.uniform(size=(n_out, dim)), m)
    n = n_s + n_out
    B, F, _ = O.bf_sweep(coords, nbr, "exponential", (1.0, 6.0, 0.0))
    sigma2, tau2 = 1.7, 0.3
    h = np.where(rng.uniform(size=n) < 0.3, 0.0, 1.0 / rng.uniform(0.5, 2.0, n) ** 2)
    h[0] = 1.0
    v = rng.standard_normal(n)
    _, _, mean, cov = G.dag_posterior(nbr, B, F, sigma2, tau2, h, v)
    A, b, diag, _, _ = dense_ref_system(nbr, B, F, n_s, sigma2, h / tau2, v)
    Ainv = np.linalg.inv(A)
    assert np.abs(Ainv - cov[:n_s, :n_s]).max() <= 1e-10 * np.abs(cov[:n_s, :n_s]).max()
    assert np.abs(Ainv @ b - mean[:n_s]).max() <= 1e-10 * np.abs(mean[:n_s]).max()
    assert np.allclose(np.diag(A), diag, rtol=1e-13, atol=0)
    # a leaf given w_S: mean (f B w_S + d v) / (f + d), variance 1 / (f + d); together with the S-marginal this is
    # the dense posterior's mean and marginal variance on the leaves
    if n_out:
        Bd = G.dense_B(nbr, B)[n_s:, :n_s]
        f, d = 1.0 / (sigma2 * F[n_s:]), h[n_s:] / tau2
        leaf_mean = (f * (Bd @ mean[:n_s]) + d * v[n_s:]) / (f + d)
        assert np.abs(leaf_mean - mean[n_s:]).max() <= 1e-10 * np.abs(mean).max()
        W = (f / (f + d))[:, None] * Bd
        leaf_var = 1.0 / (f + d) + np.einsum("ij,jk,ik->i", W, Ainv, W)
        assert np.abs(leaf_var - np.diag(cov)[n_s:]).max() <= 1e-10 * np.diag(cov).max()


def test_predictive_variance_is_the_expectation_of_the_estimator():
    """predict's var = sigma2 F_q + sample variance over draws of B_q w_S: with draws w_S ~ N(w_hat, A_S^-1) its
    expectation is sigma2 F_q + diag(B_q A_S^-1 B_q^T), the exact predictive variance.  Dense, many draws."""
    rng = np.random.default_rng(5)
    n_s, n_out, m, Q = 15, 30, 4, 6
    s = rng.uniform(size=(n_s, 2))
    coords, nbr = G.reference_dag(s, rng.uniform(size=(n_out, 2)), m)
    n = n_s + n_out
    B, F, _ = O.bf_sweep(coords, nbr, "exponential", (1.0, 6.0, 0.0))
    sigma2, tau2 = 1.3, 0.2
    A, _, _, _, _ = dense_ref_system(nbr, B, F, n_s, sigma2, np.ones(n) / tau2, np.zeros(n))
    cq, nq = G.reference_dag(s, rng.uniform(size=(Q, 2)), m)
    Bq_rows, Fq, _ = O.bf_sweep(cq, nq, "exponential", (1.0, 6.0, 0.0))
    Bq = G.dense_B(nq, Bq_rows)[n_s:, :n_s]
    exact = sigma2 * Fq[n_s:] + np.einsum("ij,jk,ik->i", Bq, np.linalg.inv(A), Bq)
    K = 200000
    W = np.linalg.cholesky(np.linalg.inv(A)) @ rng.standard_normal((n_s, K))
    est = sigma2 * Fq[n_s:] + (Bq @ W).var(axis=1, ddof=1)
    # the sample variance of K normals has relative standard deviation sqrt(2 / (K - 1)): 6 of them
    assert np.all(np.abs(est - exact) <= 6 * np.sqrt(2.0 / (K - 1)) * exact)
