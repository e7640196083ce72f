"""GPU: the CG's trace (nngp_latent_ref_cg_batch_trace), log det A_S by stochastic Lanczos quadrature
(LatentPosterior.logdet), the latent marginal likelihood (log_marginal) and its maximiser (fit), against dense
algebra on the CPU.

Tolerances come from tests/test_latent_logdet_host.py, whose numpy restatement of the recurrence fixes what fp64
leaves of the two identities: LOGDET_RTOL = 2.5e-12 for sum log M + mean against slogdet and IDENTITY_RTOL = 5e-12
for b^T x against the f = 1 / t quadrature, each 100 x the restatement's own largest error.  The device sums its
dots (r.z, p.q, and the host's b^T x) in another order than the restatement; a dot of n terms moves by at most n u
of its magnitude, u = 2^-52, which at n = 600 is 1.3e-13: added once per side (2 n u) where a bound below is used
at another n than the host test's.  The log-determinant is the sum of two parts of opposite sign (sum log M_ii > 0
and the trace of log(A^) < 0), so its bound is relative to the larger of |log det| and sum |log M_ii|."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch

from oracle import nngp_gibbs_oracle as G
from oracle import nngp_oracle as O
from test_latent_logdet_host import IDENTITY_RTOL, LOGDET_RTOL, pcg_trace
from test_latent_ref_host import dense_ref_system

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
SIGMA2, PHI, TAU2 = 1.3, 6.0, 0.25
NAN = float("nan")


def _dt(a, dev):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)


# ---------------------------------------------------------------- the raw call on an S = T system, n = 600
@functools.lru_cache(maxsize=None)
def _case600():
    """n = 600, m = 10 (S = T), the oracle's B / F, d with ~30 % zeros, the dense A, and three right-hand sides of
    which the middle one lies in a two-dimensional Krylov space (two eigenvectors of A^ = M^-1/2 A M^-1/2): it
    converges after two iterations while its neighbours need tens."""
    rng = np.random.default_rng(600)
    n, m = 600, 10
    coords = rng.uniform(size=(n, 2))
    nbr = O.c_knn_prior(coords, m)
    B, F, _ = O.c_bf_sweep(coords, nbr, "exponential", (1.0, PHI, 0.0))
    h = np.where(rng.uniform(size=n) < 0.3, 0.0, 1.0 / rng.uniform(0.5, 2.0, n) ** 2)
    d = h / TAU2
    A = G.precision(nbr, B, F * SIGMA2) + np.diag(d)
    M = np.diag(A).copy()
    _, V = np.linalg.eigh(A / np.sqrt(M)[:, None] / np.sqrt(M)[None, :])
    Bm = rng.standard_normal((n, 3))
    Bm[:, 1] = np.sqrt(M) * (V[:, 5] + 0.5 * V[:, n - 7])
    out = dict(n=n, m=m, nbr=nbr, B=B, F=F, d=d, A=A, M=M, Bm=Bm)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _geom(dev, c, n_s=None):
    from pynngp_amd import _lib

    nbr_d, B_d, F_d = _dt(c["nbr"].astype(np.int32), dev), _dt(c["B"], dev), _dt(c["F"], dev)
    off, rev_j, rev_k = _lib.reverse_neighbors(nbr_d)
    prep = _lib.gibbs_prepare(B_d, F_d, off, rev_j, rev_k)
    return nbr_d, B_d, off, rev_j, rev_k, prep, (c["n"] if n_s is None else n_s)


def _run(geom, Bm, d, rtol, max_iter, trace_len=None, sigma2=SIGMA2):
    """One traced call on a zeroed workspace and a NaN-filled trace: (x, info, workspace, trace) as numpy."""
    from pynngp_amd import _lib

    n, n_s, K = geom[0].shape[0], geom[6], Bm.shape[1]
    ws = torch.zeros(_lib.load().nngp_latent_ref_cg_batch_workspace_bytes(n, n_s, K), dtype=torch.uint8,
                     device=Bm.device)
    tr = None
    if trace_len is not None:
        tr = torch.full((K, trace_len, 2), NAN, dtype=torch.float64, device=Bm.device)
    x, info = _lib.latent_ref_cg_batch_trace(*geom, sigma2, Bm, torch.zeros_like(Bm), d=d, rtol=rtol,
                                             max_iter=max_iter, workspace=ws, trace=tr)
    return x.cpu().numpy(), info, ws.cpu().numpy(), None if tr is None else tr.cpu().numpy()


def _assert_written_exactly(trace, info):
    """Exactly the entries at k < iterations(c) are finite (and alpha > 0, beta >= 0); the rest is still NaN."""
    for c in range(trace.shape[0]):
        it = int(info[c, 0])
        assert np.all(np.isfinite(trace[c, :it])), (c, it)
        assert np.all(np.isnan(trace[c, it:])), (c, it)
        assert np.all(trace[c, :it, 0] > 0) and np.all(trace[c, :it, 1] >= 0)


def test_trace_leaves_the_solve_alone_and_writes_only_completed_iterations(dev):
    from pynngp_amd import _lib

    c = _case600()
    geom = _geom(dev, c)
    d_d = _dt(c["d"], dev)
    Bm = _dt(c["Bm"], dev)
    Bn = Bm.clone()
    Bn[5, 1] = NAN  # breaks column 1 down in its first iteration
    # (right-hand sides, rtol, max_iter, trace_len)
    runs = {"converged": (Bm, 1e-9, 500, 500), "cut": (Bm, 1e-14, 3, 7), "breakdown": (Bn, 1e-9, 500, 500)}
    for name, (R, rtol, max_iter, trace_len) in runs.items():
        x0, info0, ws0, _ = _run(geom, R, d_d, rtol, max_iter)  # the NULL trace
        x1, info1, ws1, tr = _run(geom, R, d_d, rtol, max_iter, trace_len)
        xe, infoe = _lib.latent_ref_cg_batch(*geom, SIGMA2, R, torch.zeros_like(R), d=d_d, rtol=rtol,
                                             max_iter=max_iter)
        np.testing.assert_array_equal(x1, x0, err_msg=name)
        np.testing.assert_array_equal(info1, info0, err_msg=name)
        np.testing.assert_array_equal(ws1, ws0, err_msg=name)  # r, z, p, q, M^-1, the records and the state words
        np.testing.assert_array_equal(x0, xe.cpu().numpy(), err_msg=name)
        np.testing.assert_array_equal(info0, infoe, err_msg=name)
        _assert_written_exactly(tr, info1)
        print(name, "iterations", info1[:, 0], "status", info1[:, 1])
        if name == "converged":
            # column 1 froze after its two iterations (a third when rounding leaves a residue) among slower ones
            assert np.all(info1[:, 1] == 1) and 1 <= info1[1, 0] <= 3 and info1[0, 0] > 10 and info1[2, 0] > 10
        elif name == "cut":
            assert np.all(info1[[0, 2], 0] == 3) and np.all(info1[[0, 2], 1] == 0)
        else:
            assert info1[1, 1] == -1 and info1[1, 0] == 0 and np.all(np.isnan(tr[1]))  # no entry at the breaking k
            assert info1[0, 1] == 1 and info1[2, 1] == 1


@functools.lru_cache(maxsize=None)
def _ref_case():
    """A reference-set system with every reverse list above 512 entries (the whole-block path): 6 knots on a hexagon,
    700 leaves, m = 5 (tests/test_gpu_latent_ref.py's shape)."""
    rng = np.random.default_rng(6700)
    ang = 2.0 * np.pi * (np.arange(6) + 0.25) / 6.0
    s = 0.5 + 0.3 * np.column_stack([np.cos(ang), np.sin(ang)])
    coords, nbr = G.reference_dag(s, rng.uniform(size=(700, 2)), 5)
    B, F, _ = O.c_bf_sweep(coords, nbr, "exponential", (1.0, PHI, 0.0))
    n = len(coords)
    d = np.where(rng.uniform(size=n) < 0.3, 0.0, 1.0 / rng.uniform(0.5, 2.0, n) ** 2) / TAU2
    assert np.all(np.bincount(nbr[nbr >= 0], minlength=n)[:6] > 512)
    return dict(n=n, n_s=6, m=5, nbr=nbr, B=B, F=F, d=d)


@pytest.mark.parametrize("which", ["st-600", "ref-6-700"])
def test_trace_columns_equal_one_column_calls_and_repeat(dev, which):
    c = _case600() if which == "st-600" else _ref_case()
    n_s = c.get("n_s", c["n"])
    geom = _geom(dev, c, n_s)
    d_d = _dt(c["d"], dev)
    rng = np.random.default_rng(11)
    max_iter = 200
    for K in (3, 8):
        R = rng.standard_normal((n_s, K)) * 10.0 ** rng.integers(-6, 7, K)
        if which == "st-600":
            R[:, 1] = c["Bm"][:, 1]  # a column that freezes early
        Rd = _dt(R, dev)
        x, info, _, tr = _run(geom, Rd, d_d, 1e-9, max_iter, max_iter)
        x2, info2, _, tr2 = _run(geom, Rd, d_d, 1e-9, max_iter, max_iter)
        np.testing.assert_array_equal(tr, tr2)  # NaN where unwritten in both
        np.testing.assert_array_equal(x, x2)
        np.testing.assert_array_equal(info, info2)
        _assert_written_exactly(tr, info)
        for k in range(K):
            x1, info1, _, tr1 = _run(geom, Rd[:, k:k + 1].contiguous(), d_d, 1e-9, max_iter, max_iter)
            np.testing.assert_array_equal(tr[k], tr1[0], err_msg=f"K={K} column {k}")
            np.testing.assert_array_equal(x[:, k], x1[:, 0])
            np.testing.assert_array_equal(info[k], info1[0])


def test_trace_is_the_lanczos_tridiagonal(dev):
    """b^T x_k = |M^-1/2 b|^2 e_1^T T_k^-1 e_1 from the device's own x and trace, for converged solves and for ones cut
    after five iterations (the identity holds at every k).  Bound: the host test's, plus 2 n u for the dots' order."""
    from pynngp_amd import lanczos_quadrature

    c = _case600()
    n = c["n"]
    geom = _geom(dev, c)
    d_d = _dt(c["d"], dev)
    Bm = c["Bm"]
    tol = IDENTITY_RTOL + 2 * n * U
    inv = lambda t: 1.0 / t  # noqa: E731
    for rtol, max_iter in ((1e-10, 500), (1e-14, 5)):
        x, info, _, tr = _run(geom, _dt(Bm, dev), d_d, rtol, max_iter, max_iter)
        for k in range(3):
            it = int(info[k, 0])
            assert it >= 1
            b = Bm[:, k]
            w = (b * b / c["M"]).sum()
            quad = w * lanczos_quadrature(tr[k, :it, 0], tr[k, :it, 1], f=inv)
            bx = b @ x[:, k]
            # the restatement on the same system and right-hand side: what the CPU recurrence leaves of the identity
            xc, al, be = pcg_trace(c["A"], b, rtol, max_iter)
            cpu = abs(w * lanczos_quadrature(al, be, f=inv) - b @ xc) / abs(b @ xc)
            print(f"max_iter={max_iter} column {k}: {it} iterations, identity rel err {abs(quad - bx) / abs(bx):.3g} "
                  f"(CPU restatement {cpu:.3g}, {len(al)} iterations)")
            assert abs(quad - bx) <= tol * abs(bx)
            if max_iter == 500:  # and it is b^T A^-1 b to the solve's accuracy
                exact = b @ np.linalg.solve(c["A"], b)
                assert abs(quad - exact) <= 2 * np.linalg.cond(c["A"]) * rtol * abs(exact)


# ---------------------------------------------------------------- LatentPosterior: dense comparisons
def _device_system(lp):
    """The node DAG, its unit-variance factors and d = h / tau2 as the device holds them, in MODEL node order."""
    perm = lp.perm.cpu().numpy()
    nbs = lp.nbr.cpu().numpy()
    n, m = nbs.shape
    nbr, B, F, d = np.full((n, m), -1, dtype=np.int32), np.zeros((n, m)), np.zeros(n), np.zeros(n)
    nbr[perm] = np.where(nbs >= 0, perm[np.maximum(nbs, 0)], -1)
    B[perm] = lp.B.cpu().numpy()
    F[perm] = lp.F.cpu().numpy()
    d[perm] = lp.d.cpu().numpy()
    return nbr, B, F, d


def _node_data(lp, y, X=None):
    """(v or y, X) per node in model order: zeros on nodes without an observation."""
    n = lp.n_nodes
    obs = np.isfinite(y)
    yn = np.zeros(n)
    yn[lp.node_of_t[obs]] = y[obs]
    Xn = None
    if X is not None:
        Xn = np.zeros((n, X.shape[1]))
        Xn[lp.node_of_t] = X
    return yn, Xn


def _dense_log_marginal(nbr, B, F, d, sigma2, v):
    """log N(v_obs; 0, C_obs + diag(1 / d_obs)), C the covariance of the node DAG (over all nodes: on the leaves it is
    B_L Q_S^-1 B_L^T + diag(1 / f)), and what bounds its own error."""
    C = np.linalg.inv(G.precision(nbr, B, F * sigma2))
    o = d > 0
    V = C[np.ix_(o, o)] + np.diag(1.0 / d[o])
    _, ld = np.linalg.slogdet(V)
    q = v[o] @ np.linalg.solve(V, v[o])
    value = -0.5 * (o.sum() * math.log(2.0 * math.pi) + ld + q)
    return value, 100.0 * U * np.linalg.cond(V) * (abs(ld) + q)


def _check_logdet_and_marginal(lp, y, X, rtol=1e-10, beta=None):
    """logdet with the basis probes against slogdet(A_S), log_marginal against the dense Gaussian log-density."""
    n_s, n = lp.n_s, lp.n_nodes
    nbr, B, F, d = _device_system(lp)
    sigma2 = lp.cov.sigma2
    yn, Xn = _node_data(lp, y, X)
    v = yn if beta is None or X is None else yn - Xn @ beta
    A, b, diag, _, _ = dense_ref_system(nbr, B, F, n_s, sigma2, d, v)
    _, exact = np.linalg.slogdet(A)
    Z = math.sqrt(n_s) * np.eye(n_s)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        ld = lp.logdet(z=Z, rtol=rtol)
    scale = max(abs(exact), np.abs(np.log(diag)).sum())
    tol_ld = (LOGDET_RTOL + 2 * n * U) * scale
    print(f"n_s={n_s} n={n}: logdet {ld.value:.12g} exact {exact:.12g} err/tol {abs(ld.value - exact) / tol_ld:.3g} "
          f"se {ld.se:.3g} iterations max {ld.iterations.max()}")
    assert abs(ld.value - exact) <= tol_ld
    assert math.isfinite(ld.se) and ld.per_probe.shape == (n_s,) and ld.iterations.shape == (n_s,)
    assert np.all(ld.iterations >= 1) and np.all(ld.iterations <= n_s + 8)
    assert lp.logdet(z=Z, rtol=rtol, batch=3).value == ld.value
    # the marginal likelihood: its log-determinant term to tol_ld, its quadratic form through one CG solve to rtol
    # (relative error of x at most cond rtol, as the solves of tests/test_gpu_latent_ref.py), its plain sums of at
    # most n terms to n u of their magnitudes, and the dense side to its own bound
    dense, tol_dense = _dense_log_marginal(nbr, B, F, d, sigma2, v)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        got, se = lp.log_marginal(beta=beta if X is not None else None, z=Z, rtol=rtol, logdet_rtol=rtol)
    f = 1.0 / (sigma2 * F)
    sums = np.abs(np.log(d[d > 0])).sum() + np.abs(np.log(f)).sum() + (d * v * v).sum()
    tol = 0.5 * (tol_ld + 2 * np.linalg.cond(A) * rtol * (b @ np.linalg.solve(A, b)) + 4 * n * U * sums) + tol_dense
    print(f"    log_marginal {got:.12g} dense {dense:.12g} err/tol {abs(got - dense) / tol:.3g}")
    assert abs(got - dense) <= tol
    assert se == 0.5 * ld.se


@pytest.mark.parametrize("n,m", [(48, 5), (64, 8)])
def test_exact_logdet_and_log_marginal_s_equals_t(dev, n, m):
    from pynngp_amd import Covariance, LatentPosterior

    rng = np.random.default_rng(n)
    t, y = rng.uniform(size=(n, 2)), rng.standard_normal(n)
    y[rng.uniform(size=n) < 0.25] = np.nan
    y[0] = 0.4
    eps = rng.uniform(0.5, 2.0, n)
    lp = LatentPosterior(t, y, Covariance("exponential", SIGMA2, PHI, TAU2), m=m, eps=eps, device=dev)
    assert lp.n_s == lp.n_nodes == n and (lp.nbr.cpu().numpy() < 0).any()  # the first rows are -1 padded
    _check_logdet_and_marginal(lp, y, None)


def _knots_and_leaves(rng):
    """8 knots -- four about the centre, four in the corners -- and 700 data locations, m = 4: the central knots are
    parents of most leaves, so their reverse lists pass 512 entries (the whole-block path)."""
    s = np.array([[0.42, 0.45], [0.58, 0.44], [0.45, 0.57], [0.57, 0.58], [0.02, 0.03], [0.97, 0.02], [0.03, 0.98],
                  [0.98, 0.97]])
    return s, rng.uniform(size=(700, 2))


@pytest.mark.parametrize("case", ["A-40-120", "A-with-X", "B-8-700"])
def test_exact_logdet_and_log_marginal_reference_set(dev, case):
    from pynngp_amd import Covariance, LatentPosterior

    rng = np.random.default_rng(5)
    X = None
    if case.startswith("A"):  # 40 reference points, 120 data locations of which 10 coincide with reference points
        s = rng.uniform(size=(40, 2))
        t = np.concatenate([s[rng.choice(40, size=10, replace=False)], rng.uniform(size=(110, 2))])
        t = t[rng.permutation(120)]
        m = 6
        if case == "A-with-X":
            X = np.column_stack([np.ones(120), rng.standard_normal(120)])
    else:
        s, t = _knots_and_leaves(rng)
        m = 4
    N = len(t)
    y = rng.standard_normal(N) + (X @ np.array([0.7, -0.4]) if X is not None else 0.0)
    y[rng.uniform(size=N) < 0.25] = np.nan  # h = 0 on some reference nodes and some leaves
    y[0] = 0.3
    eps = rng.uniform(0.5, 2.0, N)
    lp = LatentPosterior(t, y, Covariance("exponential", SIGMA2, PHI, TAU2), m=m, X=X, eps=eps, device=dev, ref=s)
    assert lp.n_s == len(s) and lp.n_nodes == len(s) + N - (10 if case.startswith("A") else 0)
    if case == "B-8-700":
        off = lp.off.cpu().numpy()
        assert (np.diff(off)[:lp.n_s] > 512).sum() >= 2
    beta = None
    if X is not None:  # beta_hat plugged in on both sides
        beta = lp.gls_beta(rtol=1e-10)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            Z = math.sqrt(lp.n_s) * np.eye(lp.n_s)
            assert lp.log_marginal(z=Z, rtol=1e-10, logdet_rtol=1e-10) == \
                lp.log_marginal(beta=beta, z=Z, rtol=1e-10, logdet_rtol=1e-10)
    _check_logdet_and_marginal(lp, y, X, beta=beta)


# ---------------------------------------------------------------- the stochastic estimator
def test_rademacher_estimator_and_batch_independence(dev):
    """n = 600, m = 10, phi = 12, tau2 = 0.1, 32 Rademacher probes: |value - slogdet| <= 4 se and se / |value| <= 0.01.
    (The numpy restatement of tests/test_latent_logdet_host.py with numpy's own signs on this very system gave
    |error| = 0.84, 0.61, 0.20 and 0.02 se and se / |value| = 7.4e-4 .. 8.9e-4 over four seeds, 13 or 14 iterations
    per probe; the device's probes are Philox signs, which numpy cannot restate, so the seed is the default one.)"""
    from pynngp_amd import Covariance, LatentPosterior

    rng = np.random.default_rng(12)
    n, m = 600, 10
    t, y = rng.uniform(size=(n, 2)), rng.standard_normal(n)
    lp = LatentPosterior(t, y, Covariance("exponential", 1.0, 12.0, 0.1), m=m, device=dev)
    nbr, B, F, d = _device_system(lp)
    A, _, _, _, _ = dense_ref_system(nbr, B, F, n, 1.0, d, np.zeros(n))
    _, exact = np.linalg.slogdet(A)
    ld = lp.logdet(n_probes=32, seed=0)
    print(f"logdet {ld.value:.8g} +- {ld.se:.3g}, exact {exact:.8g}: error {abs(ld.value - exact) / ld.se:.3g} se, "
          f"se/|value| {ld.se / abs(ld.value):.3g}, iterations {ld.iterations.min()}..{ld.iterations.max()}")
    assert abs(ld.value - exact) <= 4 * ld.se
    assert ld.se / abs(ld.value) <= 0.01
    assert ld.per_probe.shape == (32,) and ld.iterations.shape == (32,)
    for batch in (1, 3, 8):
        other = lp.logdet(n_probes=32, seed=0, batch=batch)
        assert other.value == ld.value and other.se == ld.se
        np.testing.assert_array_equal(other.per_probe, ld.per_probe)
    assert lp.logdet(n_probes=32, seed=1).value != ld.value
    # probe k is keyed by (seed, k) alone: fewer probes are a prefix
    np.testing.assert_array_equal(lp.logdet(n_probes=5, seed=0).per_probe, ld.per_probe[:5])


# ---------------------------------------------------------------- fit
def test_fit_moves_toward_the_truth(dev):
    from pynngp_amd import NNGP, Covariance, LatentPosterior

    rng = np.random.default_rng(2000)
    n, m = 2000, 10
    truth = Covariance("exponential", 1.5, 8.0, 0.2)
    t = rng.uniform(size=(n, 2))
    # a draw from the latent model itself: w from the NNGP prior of these neighbour sets, y = w + noise
    nbr = O.c_knn_prior(t, m)
    Bt, Ft, _ = O.c_bf_sweep(t, nbr, "exponential", (1.0, truth.phi, 0.0))
    w = O.c_nngp_simulate(nbr, Bt, Ft * truth.sigma2, rng.standard_normal(n))
    y = w + math.sqrt(truth.tau2) * rng.standard_normal(n)
    start = Covariance("exponential", truth.sigma2 * 3.0, truth.phi / 3.0, truth.tau2 * 3.0)
    lp = LatentPosterior(t, y, start, m=m, device=dev)
    kw = dict(n_probes=16, seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ll_start, _ = lp.log_marginal(**kw)
        ll_truth, _ = lp.update(truth).log_marginal(**kw)
        lp.update(start)
        cov, res = lp.fit(maxiter=40, **kw)
        ll_fit, _ = lp.log_marginal(**kw)
    print(f"start {ll_start:.3f} truth {ll_truth:.3f} fit {ll_fit:.3f} at {cov.theta} after {res.nfev} evaluations")
    assert lp.cov == cov and ll_fit == -res.fun  # the object is left at the optimum; the objective is deterministic
    assert ll_fit > ll_start
    assert ll_fit >= ll_truth
    # the thin callers on NNGP, for a reference set too
    model = NNGP(t[:300], y[:300], None, ("random", 60, [(0.0, 1.0), (0.0, 1.0)]), 6, start, device=dev)
    val, se = model.latent_loglik(mean="zero", n_probes=8)
    assert math.isfinite(val) and se > 0
    cov2, res2 = model.latent_fit(mean="zero", n_probes=8, maxiter=5)
    assert model.cov == cov2 and -res2.fun >= val
