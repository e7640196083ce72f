"""CPU: the gradient of the latent marginal likelihood -- nngp_bf_dphi and nngp_latent_rows_dot2_batch are exported
and bound and reject bad arguments before any GPU call, the Python layer refuses what it does not serve, and the
closed forms the GPU tests compare against (``host_dphi``: dB / dphi and dF / dphi per row; ``dense_grad``: the
gradient of the dense log N(v; 0, C_obs + diag(1 / d))) are pinned against central differences of the oracle.

Measured here (python tests/test_latent_grad_host.py prints them):

* ``host_dphi`` against central differences of ``oracle.c_bf_sweep`` in phi (n = 120, m = 6, d = 2, phi = 6, theta =
  (1.7, 6, 0.3), the five kinds): the relative step 1e-5 minimises the difference (steps 1e-3 .. 1e-7 tried); largest
  max|FD - closed form| / max|closed form| over the kinds 2.4e-10 (dB) and 2.3e-10 (dF); the bound is 10 x that, FD_RTOL
  = 2.4e-9 (below the cap 1e-5).
* ``dense_grad`` against central differences of the dense evaluation (40 reference points, 120 leaves, m = 6,
  exponential, theta = (1.3, 6, 0.25), a quarter of y missing, eps): relative step 1e-5 (1e-3 .. 1e-7 tried), largest
  |FD - closed form| / |closed form| over the three components 4.6e-10; GRAD_FD_RTOL = 4.6e-9.
* DPHI_K = 224: the fp64 ``host_dphi`` (LAPACK solves) against the same formula in np.longdouble (Cholesky by hand)
  differs by at most 27.6 x U cond(C_N) |C_N^-1| (|D_c| + |D_N| |b|) per row in dB over n = 300 uniform points, d = 1,
  2, 3, the five kinds, phi = 6, (sigma2, tau2) in {(1, 0), (1.7, 0.3)}, m in {1, 2, 8, 9, 15, 16, 23, 24, 31, 32}
  (3.8 in d = 1, 27.6 in d = 2 and 3; and 3.5 x U cond(C_N) |D| |u|^2 in dF), over the rows fp64 resolves (32 U cond(C_N)
  < 1, a superset of ``resolved``'s); K = 8 x the larger, rounded up to a multiple of 32.
"""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import nngp_gibbs_oracle as G
from oracle import nngp_oracle as O

U = 2.0 ** -52
NEW = ("nngp_bf_dphi_workspace_bytes", "nngp_bf_dphi", "nngp_latent_rows_dot2_batch")
KINDS = ("exponential", "matern32", "matern52", "gaussian", "spherical")
FD_STEP, FD_RTOL = 1e-5, 2.4e-9
GRAD_FD_STEP, GRAD_FD_RTOL = 1e-5, 4.6e-9
DPHI_K = 224.0


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
        assert getattr(lib, s).argtypes is not None, s
    assert lib.nngp_abi_version() == 4 and _lib.ABI_VERSION == 4  # pure additions


P = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731
EINVAL, EUNSUP = -1, -4

# fake non-null, 256-byte aligned "device" addresses: every case below must fail before any launch
DPHI = dict(coords=256, n_points=50, dim=2, nbr=512, order=None, n_rows=50, m=5, i0=0, kind=0, sigma2=1.0, phi=6.0,
            tau2=0.1, B=768, F=1024, dB=1280, dF=1536, partials=1792, workspace=2048, workspace_bytes=1 << 20)


def _dphi(lib, **kw):
    a = dict(DPHI)
    a.update(kw)
    return lib.nngp_bf_dphi(P(a["coords"]), a["n_points"], a["dim"], P(a["nbr"]), P(a["order"]), a["n_rows"], a["m"],
                            a["i0"], a["kind"], a["sigma2"], a["phi"], a["tau2"], P(a["B"]), P(a["F"]), P(a["dB"]),
                            P(a["dF"]), P(a["partials"]), P(a["workspace"]), a["workspace_bytes"], None)


DOT2 = dict(nbr=256, B=512, dB=768, n=10, n_s=4, m=4, nrhs=3, x=1024, p=1280, q=1536)


def _dot2(lib, **kw):
    a = dict(DOT2)
    a.update(kw)
    return lib.nngp_latent_rows_dot2_batch(P(a["nbr"]), P(a["B"]), P(a["dB"]), a["n"], a["n_s"], a["m"], a["nrhs"],
                                           P(a["x"]), P(a["p"]), P(a["q"]), None)


@pytest.mark.parametrize("kw,code", [
    (dict(coords=None), EINVAL), (dict(workspace=None), EINVAL), (dict(partials=None), EINVAL),
    (dict(nbr=None), EINVAL), (dict(B=None), EINVAL), (dict(F=None), EINVAL), (dict(dB=None), EINVAL),
    (dict(dF=None), EINVAL),
    (dict(m=0), EUNSUP), (dict(m=33), EUNSUP), (dict(kind=5), EUNSUP), (dict(kind=6), EINVAL), (dict(kind=-1), EINVAL),
    (dict(dim=0), EUNSUP), (dict(dim=4), EUNSUP),
    (dict(workspace_bytes=8), EINVAL), (dict(workspace=2049), EINVAL),
    (dict(phi=0.0), EINVAL), (dict(sigma2=float("nan")), EINVAL), (dict(tau2=-1.0), EINVAL),
    (dict(n_rows=51), EINVAL), (dict(i0=-1), EINVAL), (dict(dB=768), EINVAL),
])
def test_bf_dphi_rejects_bad_arguments_before_any_launch(lib, kw, code):
    assert _dphi(lib, **kw) == code, (kw, lib.nngp_last_error())
    assert lib.nngp_last_error()


def test_bf_dphi_workspace_sizes(lib):
    from pynngp_amd import _lib

    assert lib.nngp_bf_dphi_workspace_bytes(1000, 0) == 0 and lib.nngp_bf_dphi_workspace_bytes(1000, 33) == 0
    assert lib.nngp_bf_dphi_workspace_bytes(-1, 5) == 0
    for m in (1, 8, 9, 15, 16, 23, 24, 31, 32):
        lanes = 2 if m <= 8 else 4 if m <= 15 else 8 if m <= 23 else 16 if m <= 31 else 64
        blocks = (1000 * lanes + 255) // 256
        got = lib.nngp_bf_dphi_workspace_bytes(1000, m)
        assert got % 256 == 0 and got >= blocks * 32, (m, got)
    assert lib.nngp_bf_dphi_workspace_bytes(0, 5) > 0
    assert _lib.GRAD_MAX_M == 32


@pytest.mark.parametrize("kw", [dict(nbr=None), dict(B=None), dict(dB=None), dict(x=None), dict(p=None),
                                dict(q=None), dict(nrhs=0), dict(nrhs=9), dict(n_s=11), dict(n_s=-1), dict(n=-1),
                                dict(m=0), dict(m=64), dict(q=1280), dict(p=1024)])
def test_rows_dot2_rejects_bad_arguments_before_any_launch(lib, kw):
    assert _dot2(lib, **kw) == EINVAL, (kw, lib.nngp_last_error())
    assert lib.nngp_last_error()


def test_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    from pynngp_amd import _lib

    f64 = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    coords, nbr = f64(6, 2), torch.full((6, 2), -1, dtype=torch.int32)
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.bf_dphi(coords, nbr, 0, "exponential", 1.0, 6.0, 0.0)
    with pytest.raises(NotImplementedError):
        _lib.bf_dphi(coords, nbr, 0, "matern", 1.0, 6.0, 0.0)
    with pytest.raises(NotImplementedError):
        _lib.bf_dphi(coords, torch.full((6, 33), -1, dtype=torch.int32), 0, "exponential", 1.0, 6.0, 0.0)
    with pytest.raises(ValueError):
        _lib.bf_dphi(coords, nbr.long(), 0, "exponential", 1.0, 6.0, 0.0)
    with pytest.raises(ValueError):
        _lib.bf_dphi(coords, nbr, 0, "cubic", 1.0, 6.0, 0.0)
    B, dB = f64(6, 2), f64(6, 2)
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.latent_rows_dot2_batch(nbr, B, dB, 4, f64(4, 3))
    for bad in (f64(6, 3), f64(4, 9), f64(4, 0), f64(4), torch.zeros((4, 3), dtype=torch.float32), f64(3, 4).t()):
        with pytest.raises(ValueError):
            _lib.latent_rows_dot2_batch(nbr, B, dB, 4, bad)
    with pytest.raises(ValueError):
        _lib.latent_rows_dot2_batch(nbr, B, f64(6, 3), 4, f64(4, 3))
    with pytest.raises(ValueError):
        _lib.latent_rows_dot2_batch(nbr, f64(5, 2), dB, 4, f64(4, 3))
    for n_s in (-1, 7):
        with pytest.raises(ValueError, match="n_s"):
            _lib.latent_rows_dot2_batch(nbr, B, dB, n_s, f64(4, 3))


def test_general_nu_has_no_gradient_and_says_so_before_any_device_work():
    from pynngp_amd import Covariance, LatentPosterior

    lp = LatentPosterior.__new__(LatentPosterior)  # no device behind it: anything past the check would fail
    lp.m = 5
    lp.cov = Covariance("matern", 1.0, 6.0, 0.1, nu=1.2)
    with pytest.raises(ValueError, match="matern"):
        lp.log_marginal_grad()
    with pytest.raises(ValueError, match="matern"):
        lp.fit(gradient=True)
    lp.cov, lp.m = Covariance("exponential", 1.0, 6.0, 0.1), 33
    with pytest.raises(ValueError, match="m <= 32"):
        lp.log_marginal_grad()


# ---------------------------------------------------------------- the closed forms
def _rho_prime(kind, u):
    """rho'(u) of the five kinds (u = phi d)."""
    if kind == "exponential":
        return -np.exp(-u)
    if kind == "matern32":
        return -u * np.exp(-u)
    if kind == "matern52":
        return -(u + u * u) / 3 * np.exp(-u)
    if kind == "gaussian":
        return -2 * u * np.exp(-u * u)
    if kind == "spherical":
        return np.where(u < 1, -1.5 + 1.5 * u * u, 0 * u)
    raise ValueError(kind)


def _rho(kind, u):
    if kind == "exponential":
        return np.exp(-u)
    if kind == "matern32":
        return (1 + u) * np.exp(-u)
    if kind == "matern52":
        return (1 + u + u * u / 3) * np.exp(-u)
    if kind == "gaussian":
        return np.exp(-u * u)
    if kind == "spherical":
        return np.where(u < 1, 1 - 1.5 * u + 0.5 * u * u * u, 0 * u)
    raise ValueError(kind)


def _chol_solve(A, R):
    """A^-1 R for a batch of SPD A (n, k, k) and right-hand sides R (n, k, r), by Cholesky in A's own dtype (numpy's
    LAPACK calls stop at fp64)."""
    n, k, _ = A.shape
    L = np.zeros_like(A)
    for j in range(k):
        s = A[:, j, j] - (L[:, j, :j] ** 2).sum(axis=1)
        L[:, j, j] = np.sqrt(s)
        for i in range(j + 1, k):
            L[:, i, j] = (A[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(axis=1)) / L[:, j, j]
    Y = np.zeros_like(R)
    for i in range(k):
        Y[:, i] = (R[:, i] - (L[:, i, :i, None] * Y[:, :i]).sum(axis=1)) / L[:, i, i, None]
    X = np.zeros_like(R)
    for i in range(k - 1, -1, -1):
        X[:, i] = (Y[:, i] - (L[:, i + 1:, i, None] * X[:, i + 1:]).sum(axis=1)) / L[:, i, i, None]
    return X


def _solve64(A, R):
    """np.linalg.solve over the batch; a row whose matrix LAPACK calls singular gets NaN instead of an exception."""
    try:
        return np.linalg.solve(A, R)
    except np.linalg.LinAlgError:
        out = np.full_like(R, np.nan)
        for i in range(len(A)):
            try:
                out[i] = np.linalg.solve(A[i], R[i])
            except np.linalg.LinAlgError:
                pass
        return out


def host_dphi(coords, nbr, kind, sigma2, phi, tau2, dtype=np.float64, want_scale=False):
    """(B, F, dB, dF) per row from the issue's formulas: dB_i = C_N^-1 (D_c - D_N b_i), dF_i = u^T D u, u = [-b; 1],
    D_ab = sigma2 d_ab rho'(phi d_ab).  A slot that is -1 or out of range is a decoupled diagonal entry (0 in B and
    dB, nothing in dF).  ``dtype`` np.longdouble runs the same formulas in extended precision.  ``want_scale``: also
    the two per-row error scales cond(C_N) |C_N^-1| (|D_c| + |D_N| |b|) and cond(C_N) |D| |u|^2 (2-norms, fp64) and
    cond(C_N) itself.  Where DPHI_K U cond(C_N) >= 1 (``resolved`` is False) the block is singular to fp64 -- a
    Gaussian kernel on 32 close neighbours without a nugget, say -- and no fp64 result means anything: the bounds
    exceed the values, and a sweep may or may not flag the row."""
    coords = np.asarray(coords, dtype=dtype)
    if coords.ndim == 1:
        coords = coords[:, None]
    n, m = nbr.shape
    ok = (nbr >= 0) & (nbr < len(coords))
    j = np.where(ok, nbr, 0)
    pts = np.concatenate([coords[j], coords[:n, None, :]], axis=1)  # (n, m + 1, dim): the neighbours, then the point
    valid = np.concatenate([ok, np.ones((n, 1), dtype=bool)], axis=1)
    dist = np.sqrt(((pts[:, :, None, :] - pts[:, None, :, :]) ** 2).sum(axis=-1))
    pair = valid[:, :, None] & valid[:, None, :] & ~np.eye(m + 1, dtype=bool)[None]
    s2, ph, t2 = dtype(sigma2), dtype(phi), dtype(tau2)
    u = ph * dist
    C = np.where(pair, s2 * _rho(kind, u), 0) + (s2 + t2) * np.eye(m + 1, dtype=dtype)[None]
    D = np.where(pair, s2 * dist * _rho_prime(kind, u), 0).astype(dtype)
    CN, c = C[:, :m, :m], C[:, :m, m]
    if dtype == np.float64:
        solve = _solve64
    else:
        solve = _chol_solve
    b = solve(CN, c[:, :, None])[:, :, 0]
    F = (s2 + t2) - (b * c).sum(axis=1)
    uvec = np.concatenate([-b, np.ones((n, 1), dtype=dtype)], axis=1)
    Du = (D * uvec[:, None, :]).sum(axis=2)
    dB = solve(CN, Du[:, :m, None])[:, :, 0]
    dF = (uvec * Du).sum(axis=1)
    b, dB = np.where(ok, b, 0), np.where(ok, dB, 0)
    if not want_scale:
        return b, F, dB, dF
    CN64, D64, b64 = CN.astype(np.float64), D.astype(np.float64), b.astype(np.float64)
    ev = np.linalg.eigvalsh(CN64)
    with np.errstate(all="ignore"):
        cond = np.where(ev[:, 0] > 0, ev[:, -1] / ev[:, 0], np.inf)
        inv = 1.0 / ev[:, 0]
        nrm = lambda M: np.linalg.norm(M, 2, axis=(1, 2))  # noqa: E731
        b64 = np.nan_to_num(b64)
        sB = cond * inv * (np.linalg.norm(D64[:, :m, m], axis=1) + nrm(D64[:, :m, :m]) * np.linalg.norm(b64, axis=1))
        sF = cond * nrm(D64) * (1.0 + (b64 * b64).sum(axis=1))
    return b, F, dB, dF, sB, sF, cond


def resolved(cond):
    """Rows whose neighbour block fp64 resolves: DPHI_K U cond(C_N) < 1."""
    return DPHI_K * U * cond < 1.0


@functools.lru_cache(maxsize=None)
def _fd_case():
    rng = np.random.default_rng(120)
    coords = rng.uniform(size=(120, 2))
    return coords, O.c_knn_prior(coords, 6)


def fd_dphi_errors(step):
    """max|FD - closed form| / max|closed form| for dB and dF per kind, FD the central difference of the oracle's
    B / F at phi (1 +- step)."""
    coords, nbr = _fd_case()
    sigma2, phi, tau2 = 1.7, 6.0, 0.3
    out = {}
    for kind in KINDS:
        h = phi * step
        Bp, Fp, _ = O.c_bf_sweep(coords, nbr, kind, (sigma2, phi + h, tau2))
        Bm, Fm, _ = O.c_bf_sweep(coords, nbr, kind, (sigma2, phi - h, tau2))
        B0, F0, _ = O.c_bf_sweep(coords, nbr, kind, (sigma2, phi, tau2))
        B, F, dB, dF = host_dphi(coords, nbr, kind, sigma2, phi, tau2)
        assert np.allclose(B, B0, rtol=0, atol=1e-11) and np.allclose(F, F0, rtol=1e-11, atol=0)
        h2 = (phi + h) - (phi - h)
        out[kind] = (np.abs((Bp - Bm) / h2 - dB).max() / np.abs(dB).max(),
                     np.abs((Fp - Fm) / h2 - dF).max() / np.abs(dF).max())
    return out


def test_host_dphi_is_the_derivative_of_the_oracle_factors():
    """(Module docstring: step 1e-5, observed 2.4e-10 / 2.3e-10, bound 10 x.)"""
    assert FD_RTOL <= 1e-5
    for kind, (eB, eF) in fd_dphi_errors(FD_STEP).items():
        print(f"{kind}: dB {eB:.3g} dF {eF:.3g} (bound {FD_RTOL:.3g})")
        assert eB <= FD_RTOL and eF <= FD_RTOL, kind


def test_host_dphi_masks_padding_and_bad_indices():
    coords, nbr = _fd_case()
    nb = nbr.copy()
    nb[50, 2] = 10 ** 6
    B, F, dB, dF = host_dphi(coords, nb, "matern32", 1.7, 6.0, 0.3)
    assert np.all(dB[nb < 0] == 0) and np.all(B[nb < 0] == 0) and dB[50, 2] == 0 and dF[0] == 0
    keep = [0, 1, 3, 4, 5]
    sub = host_dphi(coords, np.concatenate([nb[:, keep], np.full((120, 1), -1, dtype=nb.dtype)], axis=1), "matern32",
                    1.7, 6.0, 0.3)
    np.testing.assert_allclose(dB[50, keep], sub[2][50, :5], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(dF[50], sub[3][50], rtol=1e-12)


def dphi_precision_ratios(n, dim, m, kind, sigma2, tau2, seed=300):
    """The largest ratios of |fp64 - longdouble| to U x the two error scales over the rows (dB, dF)."""
    rng = np.random.default_rng(seed + dim)
    coords = rng.uniform(size=(n, dim))
    nbr = O.c_knn_prior(coords, m)
    _, _, dB, dF, sB, sF, cond = host_dphi(coords, nbr, kind, sigma2, 6.0, tau2, want_scale=True)
    with np.errstate(all="ignore"):
        _, _, dBx, dFx = host_dphi(coords, nbr, kind, sigma2, 6.0, tau2, dtype=np.longdouble)
    ok = resolved(cond)
    eB, eF = np.abs(dB - dBx).max(axis=1).astype(np.float64)[ok], np.abs(dF - dFx).astype(np.float64)[ok]
    tiny = np.finfo(np.float64).tiny  # a row without a pair (the first one; past the spherical range) has no error
    return (eB / np.maximum(U * sB[ok], tiny)).max(), (eF / np.maximum(U * sF[ok], tiny)).max()


@pytest.mark.skipif(np.finfo(np.longdouble).eps >= 2.0 ** -60, reason="np.longdouble is no wider than fp64 here")
def test_dphi_k_covers_fp64_against_extended_precision():
    """A sample of the inputs DPHI_K was measured on (module docstring): 8 x the observed ratio stays below it."""
    worst = 0.0
    for dim, m, kind, (sigma2, tau2) in ((2, 15, "exponential", (1.0, 0.0)), (1, 9, "gaussian", (1.7, 0.3)),
                                         (3, 32, "matern52", (1.0, 0.0)), (2, 24, "spherical", (1.7, 0.3))):
        rB, rF = dphi_precision_ratios(100, dim, m, kind, sigma2, tau2)
        print(f"d={dim} m={m} {kind}: dB ratio {rB:.3g} dF ratio {rF:.3g}")
        worst = max(worst, rB, rF)
    assert 8 * worst <= DPHI_K


# ---------------------------------------------------------------- the dense gradient
def dense_log_marginal(nbr, B, F, d, sigma2, v):
    """log N(v_obs; 0, C_obs + diag(1 / d_obs)), C the covariance of the node DAG
    (tests/test_gpu_latent_logdet.py::_dense_log_marginal's computation)."""
    C = np.linalg.inv(G.precision(nbr, B, F * sigma2))
    o = d > 0
    V = C[np.ix_(o, o)] + np.diag(1.0 / d[o])
    _, ld = np.linalg.slogdet(V)
    q = v[o] @ np.linalg.solve(V, v[o])
    return -0.5 * (o.sum() * math.log(2.0 * math.pi) + ld + q)


def dense_grad_parts(nbr, B, F, dB, dF, n_s, sigma2, tau2, d, v):
    """What the gradient is made of, densely: A_S, x = A_S^-1 b_S, and per parameter (sigma2, phi, tau2) the matrix
    dA_S, the vector db_S and the scalar derivative of the remaining terms of -2 log p (with the sum of their
    magnitudes).  L = [(I - B_S); -B_L], s = [f_S; g], A_S = L^T s L + d_S."""
    n = nbr.shape[0]
    Bd, dBd = G.dense_B(nbr, B)[:, :n_s], G.dense_B(nbr, dB)[:, :n_s]
    L = np.concatenate([np.eye(n_s) - Bd[:n_s], -Bd[n_s:]])
    dL = -dBd
    f = 1.0 / (sigma2 * F)
    obs = d > 0
    oS, oL = obs[:n_s], obs[n_s:]
    fl, dl, vl = f[n_s:], d[n_s:], v[n_s:]
    g = np.where(oL, fl * dl / (fl + dl), 0.0)
    s = np.concatenate([f[:n_s], g])
    A = L.T @ (s[:, None] * L) + np.diag(d[:n_s])
    b = d[:n_s] * v[:n_s] - L[n_s:].T @ (g * vl)
    x = np.linalg.solve(A, b)
    zero = np.zeros(n)
    parts = []
    for k, (df, dd) in enumerate(((-f / sigma2, zero), (-f * dF / F, zero), (zero, -d / tau2))):
        dg = np.where(oL, (df[n_s:] * dl * dl + dd[n_s:] * fl * fl) / (fl + dl) ** 2, 0.0)
        ds = np.concatenate([df[:n_s], dg])
        dA = L.T @ (ds[:, None] * L) + np.diag(dd[:n_s])
        db = dd[:n_s] * v[:n_s] - L[n_s:].T @ (dg * vl)
        if k == 1:
            dA = dA + dL.T @ (s[:, None] * L) + L.T @ (s[:, None] * dL)
            db = db - dL[n_s:].T @ (g * vl)
        terms = np.concatenate([-dd[:n_s][oS] / d[:n_s][oS], -dg[oL] / g[oL], -df[:n_s] / f[:n_s],
                                dd[:n_s] * v[:n_s] ** 2, dg * vl ** 2])
        parts.append(dict(dA=dA, db=db, rest=terms.sum(), rest_abs=np.abs(terms).sum()))
    return A, b, x, parts


def dense_grad(nbr, B, F, dB, dF, n_s, sigma2, tau2, d, v):
    """(grad (3,), the sum of the magnitudes of each component's terms (3,), cond(A_S)): the gradient of the dense log
    N(v; 0, C_obs + diag(1 / d)) in (sigma2, phi, tau2) from the issue's formulas, the trace through A_S^-1."""
    A, b, x, parts = dense_grad_parts(nbr, B, F, dB, dF, n_s, sigma2, tau2, d, v)
    Ai = np.linalg.inv(A)
    grad, mag = np.zeros(3), np.zeros(3)
    for k, p in enumerate(parts):
        m2 = p["rest"] + (Ai * p["dA"]).sum() - 2.0 * p["db"] @ x + x @ p["dA"] @ x
        grad[k] = -0.5 * m2
        mag[k] = 0.5 * (p["rest_abs"] + np.abs(Ai * p["dA"]).sum() + 2.0 * np.abs(p["db"]) @ np.abs(x)
                        + np.abs(x) @ np.abs(p["dA"]) @ np.abs(x))
    return grad, mag, np.linalg.cond(A)


@functools.lru_cache(maxsize=None)
def _grad_fd_case():
    rng = np.random.default_rng(40120)
    s, t = rng.uniform(size=(40, 2)), rng.uniform(size=(120, 2))
    coords, nbr = G.reference_dag(s, t, 6)
    n = len(coords)
    h = np.where(rng.uniform(size=n) < 0.25, 0.0, 1.0 / rng.uniform(0.5, 2.0, n) ** 2)
    h[0] = 1.0
    return coords, nbr, h, rng.standard_normal(n)


def grad_fd_errors(step, kind="exponential", theta=(1.3, 6.0, 0.25)):
    coords, nbr, h, v = _grad_fd_case()
    n_s = 40

    def value(th):
        B, F, _ = O.c_bf_sweep(coords, nbr, kind, (1.0, th[1], 0.0))
        return dense_log_marginal(nbr, B, F, h / th[2], th[0], v)

    B, F, dB, dF = host_dphi(coords, nbr, kind, 1.0, theta[1], 0.0)
    grad, _, _ = dense_grad(nbr, B, F, dB, dF, n_s, theta[0], theta[2], h / theta[2], v)
    err = np.zeros(3)
    for k in range(3):
        hk = theta[k] * step
        up, dn = list(theta), list(theta)
        up[k], dn[k] = theta[k] + hk, theta[k] - hk
        fd = (value(up) - value(dn)) / (up[k] - dn[k])
        err[k] = abs(fd - grad[k]) / abs(grad[k])
    return err


def test_dense_grad_is_the_derivative_of_the_dense_log_marginal():
    """(Module docstring: step 1e-5, observed 4.6e-10, bound 10 x.)"""
    assert GRAD_FD_RTOL <= 1e-5
    err = grad_fd_errors(GRAD_FD_STEP)
    print("relative differences (sigma2, phi, tau2):", err, "bound", GRAD_FD_RTOL)
    assert np.all(err <= GRAD_FD_RTOL)


def hutchinson_ratios(A, dAs, exact_tr, Z):
    """|estimate - exact| / se per parameter of the trace estimate mean_k s_k^T dA (M^-1/2 z_k), A s_k = M^1/2 z_k."""
    root = np.sqrt(np.diag(A))
    S = np.linalg.solve(A, (Z * root).T)
    W = (Z / root).T
    out = []
    for dA, ex in zip(dAs, exact_tr):
        per = (S * (dA @ W)).sum(axis=0)
        out.append(abs(per.mean() - ex) / (per.std(ddof=1) / math.sqrt(len(per))))
    return np.array(out)


if __name__ == "__main__":  # the measurements quoted in the module docstring
    for st in (1e-3, 1e-4, 1e-5, 1e-6, 1e-7):
        e = fd_dphi_errors(st)
        print("dphi step", st, "dB", max(v[0] for v in e.values()), "dF", max(v[1] for v in e.values()))
    for st in (1e-3, 1e-4, 1e-5, 1e-6, 1e-7):
        print("grad step", st, grad_fd_errors(st))
    worst = [0.0, 0.0]
    for dim in (1, 2, 3):
        for kind in KINDS:
            for th in ((1.0, 0.0), (1.7, 0.3)):
                for m in (1, 2, 8, 9, 15, 16, 23, 24, 31, 32):
                    r = dphi_precision_ratios(300, dim, m, kind, *th)
                    worst = [max(worst[0], r[0]), max(worst[1], r[1])]
        print("dim", dim, "worst ratios so far (dB, dF)", worst, flush=True)
