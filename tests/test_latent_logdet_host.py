"""CPU: the pieces of the latent marginal likelihood that need no device -- ``lanczos_quadrature`` against dense
algebra through a numpy restatement of the Jacobi-PCG (whose alpha_k, beta_k are the Lanczos tridiagonal of
M^-1/2 A M^-1/2), the C-ABI argument checks of nngp_latent_ref_cg_batch_trace, and the Python layer's refusals.

Tolerances.  The restatement below, on the two dense systems of this file (n = 48, m = 5 and n = 64, m = 8) with the
n basis probes sqrt(n) e_i and rtol 1e-6, 1e-10 and 1e-13, gave relative errors of 0 .. 2.3e-14 for sum log M + mean
against numpy.linalg.slogdet (the largest at rtol 1e-6) and, as the worst probe of each run, 1.2e-14 .. 5.1e-14 for
the identity b^T x = |M^-1/2 b|^2 e_1^T T^-1 e_1 (each run prints its values).  The assertions leave two orders of
magnitude over the largest: 2.5e-12 and 5e-12."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import nngp_gibbs_oracle as G
from oracle import nngp_oracle as O

LOGDET_RTOL = 2.5e-12  # 100 x the largest relative error the restatement showed against slogdet (2.3e-14)
IDENTITY_RTOL = 5e-12  # 100 x the largest for b.x against the f = 1 / t quadrature (5.1e-14)


def pcg_trace(A, b, rtol, max_iter):
    """The device's recurrence in numpy fp64: Jacobi-PCG from x = 0; (x, alpha, beta) of the completed iterations."""
    M = np.diag(A).copy()
    x = np.zeros_like(b)
    r = b.copy()
    z = r / M
    p = z.copy()
    rz, tol2 = r @ z, rtol * rtol * (b @ b)
    alpha, beta = [], []
    for _ in range(max_iter):
        if r @ r <= tol2:
            break
        q = A @ p
        a = rz / (p @ q)
        x += a * p
        r -= a * q
        z = r / M
        rz_new = r @ z
        alpha.append(a)
        beta.append(rz_new / rz)
        p = z + beta[-1] * p
        rz = rz_new
    return x, np.array(alpha), np.array(beta)


@functools.lru_cache(maxsize=None)
def dense_system(n, m, sigma2=1.3, phi=6.0, tau2=0.25):
    """A = (I - B)^T (sigma2 F)^-1 (I - B) + diag(d) of a small NNGP, some d = 0 (read-only)."""
    rng = np.random.default_rng(100 * n + m)
    coords = rng.uniform(size=(n, 2))
    nbr = O.knn_prior(coords, m)
    B, F, _ = O.bf_sweep(coords, nbr, "exponential", (1.0, phi, 0.0))
    h = np.where(rng.uniform(size=n) < 0.3, 0.0, 1.0 / rng.uniform(0.5, 2.0, n) ** 2)
    A = G.precision(nbr, B, F * sigma2) + np.diag(h / tau2)
    A.setflags(write=False)
    return A


@pytest.mark.parametrize("n,m", [(48, 5), (64, 8)])
@pytest.mark.parametrize("rtol", [1e-6, 1e-10, 1e-13])
def test_lanczos_quadrature_gives_logdet_and_the_solve_identity(n, m, rtol):
    from pynngp_amd import lanczos_quadrature

    A = dense_system(n, m)
    M = np.diag(A)
    _, exact = np.linalg.slogdet(A)
    per, worst_id = np.zeros(n), 0.0
    for i in range(n):  # the columns of sqrt(n) I: E z z^T = I exactly, so the mean is the trace of log(A^)
        zv = np.zeros(n)
        zv[i] = np.sqrt(n)
        b = np.sqrt(M) * zv
        x, al, be = pcg_trace(A, b, rtol, 4 * n)
        assert 1 <= len(al) <= n + 8
        w = zv @ zv
        per[i] = w * lanczos_quadrature(al, be)
        quad = w * lanczos_quadrature(al, be, f=lambda t: 1.0 / t)
        worst_id = max(worst_id, abs(quad - b @ x) / abs(b @ x))
    got = np.log(M).sum() + per.mean()
    print(f"n={n} rtol={rtol:g}: logdet rel err {abs(got - exact) / abs(exact):.3g}, identity rel err {worst_id:.3g}")
    assert abs(got - exact) <= LOGDET_RTOL * abs(exact)
    assert worst_id <= IDENTITY_RTOL


def test_lanczos_quadrature_general_start_vector():
    """A dense start vector: (M^-1/2 b)^T A^^-1 (M^-1/2 b) = b^T A^-1 b from the trace alone."""
    from pynngp_amd import lanczos_quadrature

    A = dense_system(48, 5)
    M = np.diag(A)
    b = np.random.default_rng(3).standard_normal(48)
    x, al, be = pcg_trace(A, b, 1e-12, 400)
    u = b / np.sqrt(M)
    quad = (u @ u) * lanczos_quadrature(al, be, f=lambda t: 1.0 / t)
    assert abs(quad - b @ np.linalg.solve(A, b)) <= 1e-10 * abs(quad)
    assert abs(quad - b @ x) <= IDENTITY_RTOL * abs(quad)


def test_lanczos_quadrature_one_point_and_bad_input():
    from pynngp_amd import lanczos_quadrature

    # k = 1: T = [1 / alpha_0]; beta_0 may be there (it links to an iteration that was not run) or not
    assert lanczos_quadrature([0.25], []) == np.log(4.0)
    assert lanczos_quadrature([0.25], [0.7]) == np.log(4.0)
    assert lanczos_quadrature([0.25], [], f=lambda t: 1.0 / t) == 0.25
    # a diagonal system converges in one step with alpha = 1 (A^ = I): log 1 = 0
    A = np.diag([2.0, 5.0, 0.5])
    _, al, be = pcg_trace(A, np.array([1.0, -2.0, 3.0]), 1e-12, 10)
    assert len(al) == 1 and lanczos_quadrature(al, be) == 0.0
    # k = 2 by hand: T = [[1/a0, sqrt(b0)/a0], [., 1/a1 + b0/a0]]
    a0, a1, b0 = 0.5, 0.8, 0.3
    T = np.array([[1 / a0, np.sqrt(b0) / a0], [np.sqrt(b0) / a0, 1 / a1 + b0 / a0]])
    w, V = np.linalg.eigh(T)
    assert abs(lanczos_quadrature([a0, a1], [b0, 0.1]) - (V[0] ** 2 * np.log(w)).sum()) <= 1e-15
    assert abs(lanczos_quadrature([a0, a1], [b0], f=lambda t: 1.0 / t) - np.linalg.inv(T)[0, 0]) <= 1e-15
    for al, be in (([], []), ([0.5, 0.5], []), ([0.5, float("nan")], [0.1]), ([0.5, -1.0], [0.1]),
                   ([0.5, 0.5], [float("nan")])):
        with pytest.raises(ValueError):
            lanczos_quadrature(al, be)


# ---------------------------------------------------------------- the C ABI, without a device
@pytest.fixture(scope="module")
def lib():
    from pynngp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build()")
    return _lib.load()


P = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731

# fake non-null, 256-byte aligned "device" addresses: every failing case must fail before any launch, and the
# accepted ones have n = 0, where nothing is launched
GEOM = dict(nbr=256, B=256, off=256, rev_j=256, rev_k=256, prep=256, n=10, n_s=4, m=4, sigma2=1.0, d=None, nrhs=3,
            workspace=256, workspace_bytes=1 << 20, b=256, x=512, rtol=1e-8, max_iter=10, check_every=8, trace=1024,
            trace_len=10)


def _cg_trace(lib, **kw):
    a = dict(GEOM)
    a.update(kw)
    info = (ctypes.c_double * 32)()
    rc = lib.nngp_latent_ref_cg_batch_trace(
        P(a["nbr"]), P(a["B"]), P(a["off"]), P(a["rev_j"]), P(a["rev_k"]), P(a["prep"]), a["n"], a["n_s"], a["m"],
        a["sigma2"], P(a["d"]), a["nrhs"], P(a["b"]), P(a["x"]), a["rtol"], a["max_iter"], a["check_every"], info,
        P(a["workspace"]), a["workspace_bytes"], P(a["trace"]), a["trace_len"], None)
    return rc, list(info)


def test_trace_symbol_exported_and_bound(lib):
    from pynngp_amd import _lib

    assert "nngp_latent_ref_cg_batch_trace" in _lib.SYMBOLS
    assert len(lib.nngp_latent_ref_cg_batch_trace.argtypes) == len(lib.nngp_latent_ref_cg_batch.argtypes) + 2
    assert lib.nngp_abi_version() == 4  # a pure addition


@pytest.mark.parametrize("kw,msg", [
    (dict(trace_len=9), "trace_len"),          # a trace shorter than max_iter
    (dict(trace_len=0), "trace_len"),
    (dict(trace_len=-1, max_iter=0), "trace_len"),
    (dict(trace=256), "alias"),                # b
    (dict(trace=512), "alias"),                # x
    # the shared checks of the CG entry points
    (dict(b=None), "non-null"),
    (dict(x=256), "alias"),
    (dict(rtol=0.0), "rtol"),
    (dict(max_iter=-1), "max_iter"),
    (dict(check_every=0), "check_every"),
    (dict(nrhs=0), "nrhs"),
    (dict(nrhs=9), "nrhs"),
    (dict(n_s=11), "n_s"),
    (dict(m=0), "m=0"),
    (dict(sigma2=0.0), "sigma2"),
    (dict(workspace=None), "non-null"),
    (dict(workspace_bytes=16), "workspace too small"),
    (dict(workspace=264), "aligned"),
])
def test_trace_call_bad_arguments_are_einval(lib, kw, msg):
    rc, _ = _cg_trace(lib, **kw)
    assert rc == -1, kw
    assert msg in lib.nngp_last_error().decode()


def test_null_trace_is_accepted_and_a_long_enough_one(lib):
    # n = 0: the checks pass and nothing is launched; every column reads converged after 0 iterations
    for kw in (dict(trace=None, trace_len=0), dict(trace=None, trace_len=-5), dict(trace_len=10), dict(trace_len=11),
               dict(max_iter=0, trace_len=0)):
        rc, info = _cg_trace(lib, n=0, n_s=0, **kw)
        assert rc == 0, (kw, lib.nngp_last_error().decode())
        assert info[:12] == [0.0, 1.0, 0.0, 0.0] * 3
    # a NULL trace skips the length check with n > 0 too: the next check is what fails
    rc, _ = _cg_trace(lib, trace=None, trace_len=0, workspace_bytes=16)
    assert rc == -1 and "workspace too small" in lib.nngp_last_error().decode()


# ---------------------------------------------------------------- Python refusals (no GPU needed)
def _cpu_geometry(n=6, m=2):
    nbr = torch.full((n, m), -1, dtype=torch.int32)
    B = torch.zeros((n, m), dtype=torch.float64)
    off = torch.zeros(n + 1, dtype=torch.int32)
    rev = torch.zeros(n * m, dtype=torch.int32)
    prep = torch.zeros(1 << 16, dtype=torch.uint8)
    return nbr, B, off, rev, rev.clone(), prep


def test_lib_wrapper_and_operator_refuse_cpu_tensors():
    from pynngp_amd import _lib, load_ops

    g = _cpu_geometry()
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.latent_ref_cg_batch_trace(*g, 4, 1.0, f64(4, 2), f64(4, 2), trace=f64(2, 1000, 2))
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.latent_ref_cg_batch_trace(*g, 4, 1.0, f64(4, 2), f64(4, 2))
    with pytest.raises(ValueError):  # vectors on S have n_s rows
        _lib.latent_ref_cg_batch_trace(*g, 4, 1.0, f64(6, 2), f64(6, 2))
    load_ops()
    with pytest.raises(NotImplementedError):  # no CPU kernel is registered
        torch.ops.nngp.latent_cg_batch_trace(*g, 1.0, None, f64(6, 3))
    schema = str(torch.ops.nngp.latent_cg_batch_trace.default._schema)
    assert "check_every=8" in schema and "max_iter=1000" in schema and "-> (Tensor, Tensor, Tensor)" in schema


def test_trace_shape_checks():
    """_LatentCall.check_trace, on an instance made without a device."""
    from pynngp_amd import _lib

    c = _lib._LatentCall.__new__(_lib._LatentCall)
    c.nrhs, c.dev = 3, torch.device("cpu")
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    assert c.check_trace(f64(3, 10, 2), 10).shape == (3, 10, 2)
    for bad in (f64(2, 10, 2), f64(3, 10, 3), f64(3, 10), torch.zeros((3, 10, 2), dtype=torch.float32),
                f64(3, 2, 10).transpose(1, 2), np.zeros((3, 10, 2))):
        with pytest.raises(ValueError, match="trace"):
            c.check_trace(bad, 10)
    with pytest.raises(ValueError, match="max_iter"):
        c.check_trace(f64(3, 9, 2), 10)


def test_probe_stream_is_its_own_and_methods_check_arguments_first():
    from pynngp_amd import LatentPosterior, LogDet

    L = LatentPosterior
    streams = [L.LEAF_STREAM, L.QUERY_STREAM, L.RESPONSE_STREAM, L.PROBE_STREAM]
    assert len(set(streams)) == 4 and L.PROBE_STREAM < 1 << 62
    # 2^40 probes, or draws, fit between any two of them
    assert min(abs(a - b) for i, a in enumerate(streams) for b in streams[:i]) >= 1 << 40
    lp = L.__new__(L)
    lp.n = lp.n_nodes = lp.n_s = 5
    lp.p, lp.m, lp.device = 0, 2, torch.device("cpu")
    lp.perm_s = lp.slot_of_ref = torch.arange(5)
    with pytest.raises(ValueError, match="batch"):
        lp.logdet(batch=9)
    with pytest.raises(ValueError, match="rtol"):
        lp.logdet(rtol=0.0)
    with pytest.raises(ValueError, match=r"\(K, 5\)"):
        lp.logdet(z=np.zeros((2, 4)))
    with pytest.raises(ValueError, match="n_probes"):
        lp.logdet(n_probes=0)
    assert [f.name for f in LogDet.__dataclass_fields__.values()] == ["value", "se", "per_probe", "iterations"]


def test_nngp_latent_loglik_checks_mean_before_any_device_work():
    from pynngp_amd import NNGP, Covariance

    obj = NNGP.__new__(NNGP)
    obj.refType = ("subset", 5)
    obj.cov = Covariance("exponential", 1.0, 6.0, 0.1)
    with pytest.raises(ValueError, match="mean"):
        obj.latent_loglik(mean="linear")
    with pytest.raises(ValueError, match="mean"):
        obj.latent_fit(mean="linear")
