"""Analytic log-likelihood gradient sweep (nngp_bf_grad) against a numpy fp64 restatement of its formulas.

The restatement (``ref_rows``: scalar-loop Cholesky per location) is pinned here by the dense-GP gradient
1/2 a^T dK a - 1/2 tr(K^-1 dK) at m = N - 1, N = 40, and by central differences of
``oracle.nngp_oracle.nngp_loglik``.  The partials come from the gradient kernel's own block records and fold,
not bf_sweep's record layout, so they are compared with bf_sweep's at the log-likelihood tolerance of
test_gpu_bf.py (1e-11 relative), not bit for bit.
"""
import numpy as np
import pytest
import torch

from oracle import nngp_oracle as O
from pynngp_amd import _lib

KINDS = ("exponential", "matern32", "matern52", "gaussian", "spherical")
THETA = (1.3, 6.0, 0.05)


def theta_of(kind):
    return (1.3, 1.7, 0.05) if kind == "spherical" else THETA


def rho_drho(kind, u):
    e = np.exp(-u)
    if kind == "exponential":
        return e, -e
    if kind == "matern32":
        return (1 + u) * e, -u * e
    if kind == "matern52":
        return (1 + u + u * u / 3) * e, -(u / 3) * (1 + u) * e
    if kind == "gaussian":
        g = np.exp(-u * u)
        return g, -2 * u * g
    inside = u < 1
    return np.where(inside, 1 - 1.5 * u + 0.5 * u**3, 0.0), np.where(inside, -1.5 + 1.5 * u * u, 0.0)


def chol_solve(A, rhs):
    """Scalar-loop Cholesky of A and the solves A^-1 rhs (rhs (k, r))."""
    k = A.shape[0]
    L = np.zeros_like(A)
    for j in range(k):
        s = A[j, j] - np.dot(L[j, :j], L[j, :j])
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, k):
            L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    x = rhs.astype(A.dtype).copy()
    for i in range(k):
        x[i] = (x[i] - L[i, :i] @ x[:i]) / L[i, i]
    for i in range(k - 1, -1, -1):
        x[i] = (x[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def ref_rows(coords, nbr, kind, theta, y, rows=None, dtype=np.float64):
    """Per-location (log F, r^2/F, G[3]) by the formulas of the gradient sweep, fp64 (or its ``np.longdouble``
    twin: the same code on extended-precision inputs)."""
    coords, y = coords.astype(dtype), y.astype(dtype)
    s2, phi, t2 = (dtype(x) for x in theta)
    rows = range(coords.shape[0]) if rows is None else rows
    out = np.zeros((len(rows), 5), dtype=dtype)
    for t, i in enumerate(rows):
        nb = [j for j in nbr[i] if j >= 0]
        k = len(nb)
        idx = nb + [i]
        X = coords[idx]
        d = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
        r_, dr_ = rho_drho(kind, phi * d)
        C = s2 * r_ + t2 * np.eye(k + 1, dtype=dtype)
        D = s2 * d * dr_
        np.fill_diagonal(D, 0.0)
        yy = y[idx]
        if k:
            sol = chol_solve(C[:k, :k], np.stack([C[:k, k], yy[:k]], 1))
            b, a = sol[:, 0], sol[:, 1]
        else:
            b = a = np.zeros(0, dtype=dtype)
        u = np.append(-b, dtype(1.0))
        al = np.append(a, dtype(0.0))
        F = u @ C @ u
        r = yy[k] - b @ yy[:k]
        nb2, adb = b @ b, a @ b
        dF = [(F - t2 * (1 + nb2)) / s2, u @ D @ u, 1 + nb2]
        dr = [-t2 * adb / s2, -(al @ D @ u), adb]
        out[t, 0], out[t, 1] = np.log(F), r * r / F
        for p in range(3):
            out[t, 2 + p] = -0.5 * ((dF[p] / F) * (1 - r * r / F) + 2 * r * dr[p] / F)
    return out


def field(n, dim=2, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (n, dim)), rng.standard_normal(n)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sweep(coords, nbr, kind, theta, y, i0=0, order=None, rows=True):
    p, g, G = _lib.bf_grad(dev(coords), dev(nbr), i0, kind, *theta, dev(y), want_rows=rows,
                           order=None if order is None else order)
    torch.cuda.synchronize()
    return p.cpu().numpy(), g.cpu().numpy(), None if G is None else G.cpu().numpy()


def close_rows(G, ref):
    err = np.abs(G - ref) / (1 + np.abs(ref))
    print("max |dG| / (1 + |G|) =", err.max())
    return err.max() <= 1e-9


# ---------------------------------------------------------------- the restatement itself (CPU)
def dense_grad(coords, kind, theta, y):
    s2, phi, t2 = theta
    n = len(y)
    d = np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(-1))
    r_, dr_ = rho_drho(kind, phi * d)
    K = s2 * r_ + t2 * np.eye(n)
    Ki = np.linalg.inv(K)
    al = Ki @ y
    D = s2 * d * dr_
    np.fill_diagonal(D, 0.0)
    return np.array([0.5 * al @ dK @ al - 0.5 * np.trace(Ki @ dK) for dK in (r_, D, np.eye(n))]), al


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_dense_and_central_differences(kind):
    coords, y = field(40, seed=3)
    th = theta_of(kind)
    full = np.array([[j if j < i else -1 for j in range(39)] for i in range(40)], dtype=np.int32)
    g = ref_rows(coords, full, kind, th, y)[:, 2:].sum(0)
    gd, _ = dense_grad(coords, kind, th, y)
    assert np.allclose(g, gd, rtol=1e-8, atol=1e-8), (g, gd)
    nbr = O.c_knn_prior(coords, 10)
    g = ref_rows(coords, nbr, kind, th, y)[:, 2:].sum(0)
    for p in range(3):
        h = 1e-6 * th[p]
        tp, tm = list(th), list(th)
        tp[p] += h
        tm[p] -= h
        fd = (O.nngp_loglik(coords, nbr, kind, tuple(tp), y) - O.nngp_loglik(coords, nbr, kind, tuple(tm), y)) / (2 * h)
        assert abs(fd - g[p]) <= 1e-6 * max(1.0, abs(g[p])), (kind, p, fd, g[p])


M_LIST = list(range(1, 33))  # every instantiation of bf_grad<M, P>


@pytest.mark.skipif(np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps, reason="no extended precision here")
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_against_longdouble_twin(kind):
    """The 1e-9 (1 + |G|) parity tolerance is a condition on the inputs: for every m of the GPU parity test the
    fp64 restatement must sit within 1e-11 (1 + |G|) of its longdouble twin on the same inputs."""
    coords, y = field(96, seed=1)
    th = theta_of(kind)
    for m in M_LIST:
        nbr = O.c_knn_prior(coords, m)
        r64 = ref_rows(coords, nbr, kind, th, y)[:, 2:]
        rld = ref_rows(coords, nbr, kind, th, y, dtype=np.longdouble)[:, 2:]
        err = float(np.max(np.abs(r64 - rld) / (1 + np.abs(rld))))
        print(kind, m, "fp64 vs longdouble:", err)
        assert err <= 1e-11, (kind, m, err)


# ---------------------------------------------------------------- per-location parity (GPU)
@pytest.fixture(scope="module")
def f96():
    coords, y = field(96, seed=1)
    return coords, y, {}


def nbr_of(cache, coords, m):
    if m not in cache:
        cache[m] = O.c_knn_prior(coords, m)
    return cache[m]


@pytest.mark.gpu
@pytest.mark.parametrize("m", M_LIST)
@pytest.mark.parametrize("kind", KINDS)
def test_rows_match_restatement(f96, kind, m):
    coords, y, cache = f96
    nbr = nbr_of(cache, coords, m)
    th = theta_of(kind)
    ref = ref_rows(coords, nbr, kind, th, y)
    p, g, G = sweep(coords, nbr, kind, th, y)
    assert p[2] == -1 and p[3] == -1
    assert close_rows(G, ref[:, 2:])
    assert abs(p[0] - ref[:, 0].sum()) <= 1e-11 * np.abs(ref[:, 0]).sum()
    assert abs(p[1] - ref[:, 1].sum()) <= 1e-11 * np.abs(ref[:, 1]).sum()
    assert np.all(np.abs(g - ref[:, 2:].sum(0)) <= 1e-9 * (1 + np.abs(ref[:, 2:])).sum(0))


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_dimensions(dim):
    """Every lane-group width from 4 up (grad_lanes: m = 10 -> 4 lanes, 17 -> 8, 24 -> 16, 32 -> 64)."""
    coords, y = field(96, dim=dim, seed=2)
    for m in (10, 17, 24, 32):
        nbr = O.c_knn_prior(coords, m)
        for kind in ("exponential", "matern52"):
            ref = ref_rows(coords, nbr, kind, THETA, y)
            _, _, G = sweep(coords, nbr, kind, THETA, y)
            assert close_rows(G, ref[:, 2:]), (dim, m, kind)


@pytest.mark.gpu
def test_row_subrange_and_order(f96):
    coords, y, cache = f96
    nbr = nbr_of(cache, coords, 10)
    i0, rows = 37, 41
    ref = ref_rows(coords, nbr, "matern32", THETA, y, rows=range(i0, i0 + rows))
    sub = np.ascontiguousarray(nbr[i0:i0 + rows])
    p, g, G = sweep(coords, sub, "matern32", THETA, y, i0=i0)
    assert close_rows(G, ref[:, 2:])
    order, nbr_sorted = _lib.row_order(dev(coords), i0, rows, dev(sub))
    p2, g2, G2 = _lib.bf_grad(dev(coords), nbr_sorted, i0, "matern32", *THETA, dev(y), want_rows=True, order=order)
    assert np.array_equal(G2.cpu().numpy(), G)  # bit for bit: only the visiting order changes
    # the block fold under a visiting order: the sums against the restatement, as without an order
    p2, g2 = p2.cpu().numpy(), g2.cpu().numpy()
    for pp, gg in ((p, g), (p2, g2)):
        assert pp[2] == -1 and pp[3] == -1
        assert abs(pp[0] - ref[:, 0].sum()) <= 1e-11 * np.abs(ref[:, 0]).sum()
        assert abs(pp[1] - ref[:, 1].sum()) <= 1e-11 * np.abs(ref[:, 1]).sum()
        assert np.all(np.abs(gg - ref[:, 2:].sum(0)) <= 1e-12 * np.abs(ref[:, 2:]).sum(0))


# ---------------------------------------------------------------- summed gradient
@pytest.mark.gpu
def test_summed_gradient_and_reproducibility():
    coords, y = field(2000, seed=5)
    nbr = O.c_knn_prior(coords, 15)
    th = (1.0, 12.0, 0.1)
    ref = ref_rows(coords, nbr, "exponential", th, y)
    p, g, G = sweep(coords, nbr, "exponential", th, y)
    p2, g2, G2 = sweep(coords, nbr, "exponential", th, y)
    assert np.array_equal(g, g2) and np.array_equal(p, p2) and np.array_equal(G, G2)
    # kappa as in test_gpu_bf.py is at most a few 1e5 for such sets: the floor 1e-12 of max(1e-12, 1e-15 kappa)
    # is asserted (the tighter of the two)
    tol = 1e-12 * np.abs(ref[:, 2:]).sum(0)
    print("grad err / sum|G| =", np.abs(g - ref[:, 2:].sum(0)) / np.abs(ref[:, 2:]).sum(0))
    assert np.all(np.abs(g - ref[:, 2:].sum(0)) <= tol)
    _, _, pb = _lib.bf_sweep(dev(coords), dev(nbr), 0, "exponential", *th, values=dev(y), want_bf=False)
    pb = pb.cpu().numpy()
    ll = -0.5 * (p[0] + p[1])
    llb = -0.5 * (pb[0] + pb[1])
    assert abs(ll - llb) <= 1e-11 * abs(llb)


# ---------------------------------------------------------------- dense known answer
@pytest.mark.gpu
def test_dense_known_answer():
    coords, y = field(32, seed=7)
    full = np.array([[j if j < i else -1 for j in range(31)] for i in range(32)], dtype=np.int32)
    th = (1.3, 6.0, 0.05)
    for kind in ("exponential", "gaussian"):
        gd, _ = dense_grad(coords, kind, th, y)
        _, g, G = sweep(coords, full, kind, th, y)
        S = np.abs(G).sum(0)
        print(kind, g, gd)
        assert np.all(np.abs(g - gd) <= 1e-9 * (1 + S))


# ---------------------------------------------------------------- flags
@pytest.mark.gpu
def test_not_pd_flag():
    coords, y = field(96, seed=1)
    coords[50] = coords[49]  # duplicate points, no nugget: C_N singular wherever both are neighbours
    nbr = O.c_knn_prior(coords, 5)
    p, g, G = sweep(coords, nbr, "exponential", (1.0, 6.0, 0.0), y)
    assert p[2] >= 0
    assert np.all(np.isnan(G[int(p[2])]))


@pytest.mark.gpu
def test_bad_index_flag(f96):
    coords, y, cache = f96
    nbr = nbr_of(cache, coords, 10).copy()
    nbr[60, 3] = 96  # one past the end
    p, g, G = sweep(coords, nbr, "exponential", THETA, y)
    assert p[3] == 60 and p[2] == -1
    assert np.all(np.isfinite(G))
    ok = nbr_of(cache, coords, 10)
    ref = ref_rows(coords, ok, "exponential", THETA, y)
    keep = np.arange(96) != 60
    assert close_rows(G[keep], ref[keep, 2:])


# ---------------------------------------------------------------- NNGP methods
@pytest.mark.gpu
def test_loglik_grad_methods():
    from pynngp_amd import nngp as N

    coords, y = field(300, seed=9)
    y = y + 0.7
    cov = N.Covariance("exponential", 1.0, 8.0, 0.1)
    model = N.NNGP(coords, y, None, "S=T", 10, cov)
    ll, g = model.loglik_grad()
    nbr = model.nbr.cpu().numpy()
    ref = ref_rows(coords, nbr, "exponential", (1.0, 8.0, 0.1), y)
    assert abs(ll - model.loglik()) <= 1e-11 * abs(ll)
    assert np.all(np.abs(g - ref[:, 2:].sum(0)) <= 1e-9 * (1 + np.abs(ref[:, 2:])).sum(0))
    pl, mu, pg = model.profile_loglik_grad(cov)
    th = (1.0, 8.0, 0.1)
    for k in range(3):
        h = 1e-6 * th[k]
        tp, tm = list(th), list(th)
        tp[k] += h
        tm[k] -= h
        fd = (model.profile_loglik(N.Covariance("exponential", *tp))[0]
              - model.profile_loglik(N.Covariance("exponential", *tm))[0]) / (2 * h)
        assert abs(fd - pg[k]) <= 1e-5 * max(1.0, abs(pg[k])), (k, fd, pg[k])
    with pytest.raises(NotImplementedError):
        model.loglik_grad(cov=N.Covariance("matern", 1.0, 8.0, 0.1, nu=0.7))
    with pytest.raises(N.NNGPNumericalError):
        c2 = coords.copy()
        c2[50] = c2[49]
        N.NNGP(c2, y, None, "S=T", 5, N.Covariance("exponential", 1.0, 8.0, 0.0)).loglik_grad()


# ---------------------------------------------------------------- refusals
def test_lib_refusals():
    c = torch.zeros((40, 2), dtype=torch.float64)
    v = torch.zeros(40, dtype=torch.float64)
    with pytest.raises(NotImplementedError):
        _lib.bf_grad(c, torch.zeros((40, 33), dtype=torch.int32), 0, "exponential", 1.0, 1.0, 0.1, v)
    with pytest.raises(NotImplementedError):
        _lib.bf_grad(c, torch.zeros((40, 0), dtype=torch.int32), 0, "exponential", 1.0, 1.0, 0.1, v)
    with pytest.raises(NotImplementedError):
        _lib.bf_grad(c, torch.zeros((40, 5), dtype=torch.int32), 0, "matern", 1.0, 1.0, 0.1, v)


@pytest.mark.gpu
def test_method_refusals():
    from pynngp_amd import nngp as N

    coords, y = field(60, seed=4)
    with pytest.raises(NotImplementedError):
        N.NNGP(coords, y, None, "S=T", 0, N.Covariance("exponential", 1.0, 8.0, 0.1)).loglik_grad()
    model = N.NNGP(coords, y, None, "S=T", 5, N.Covariance("exponential", 1.0, 8.0, 0.1))
    iso = N.IsotropicCovariance(lambda d: torch.exp(-3.0 * d), tau2=0.1)
    with pytest.raises(TypeError):
        model.loglik_grad(cov=iso)
    with pytest.raises(TypeError):
        N.NNGP(coords, y, None, "S=T", 5, lambda a, b: np.exp(-np.abs(a[:, None, 0] - b[None, :, 0]))).loglik_grad()
    with pytest.raises(NotImplementedError):
        model.fit(kind="matern", nu=0.7, gradient=True)


# ---------------------------------------------------------------- fit with the gradient
@pytest.mark.gpu
def test_fit_with_gradient():
    """N = 2000, exponential, true theta (1, 12, 0.1), maxiter 60: L-BFGS-B on the analytic gradient reaches a
    log-likelihood no lower than Nelder-Mead's (fit()'s default) minus 1e-6 |l|, in fewer objective evaluations."""
    from pynngp_amd import nngp as N

    rng = np.random.default_rng(11)
    n = 2000
    coords = rng.uniform(0.0, 1.0, (n, 2))
    d = np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(-1))
    K = 1.0 * np.exp(-12.0 * d) + 0.1 * np.eye(n)
    y = np.linalg.cholesky(K) @ rng.standard_normal(n) + 0.5
    start = N.Covariance("exponential", 0.5, 5.0, 0.3)
    nm = N.NNGP(coords, y, None, "S=T", 10, start).fit()
    lb = N.NNGP(coords, y, None, "S=T", 10, start).fit(gradient=True, maxiter=60)
    print("Nelder-Mead:", nm["loglik"], nm["n_evals"], "L-BFGS-B:", lb["loglik"], lb["n_evals"], lb["n_grad_evals"])
    assert lb["loglik"] >= nm["loglik"] - 1e-6 * abs(nm["loglik"])
    assert lb["n_evals"] < nm["n_evals"]
    assert lb["n_grad_evals"] >= 1


# ---------------------------------------------------------------- autograd
@pytest.mark.gpu
def test_autograd_theta():
    import pynngp_amd

    coords, y = field(300, seed=9)
    nbr = O.c_knn_prior(coords, 10)
    th = (1.0, 8.0, 0.1)
    theta = torch.tensor(th, dtype=torch.float64, requires_grad=True)
    ll = pynngp_amd.loglik(dev(coords), dev(nbr), theta, dev(y), "matern32")
    (2.0 * ll).backward()
    p, g, _ = sweep(coords, nbr, "matern32", th, y, rows=False)
    assert np.array_equal(theta.grad.numpy(), 2.0 * g)
    ref = ref_rows(coords, nbr, "matern32", th, y)
    want = -0.5 * (300 * np.log(2 * np.pi) + ref[:, 0].sum() + ref[:, 1].sum())
    assert abs(ll.item() - want) <= 1e-11 * abs(want)
    # with a visiting order: the same gradient to rounding
    order, nbs = _lib.row_order(dev(coords), 0, 300, dev(nbr))
    t2 = torch.tensor(th, dtype=torch.float64, requires_grad=True)
    pynngp_amd.loglik(dev(coords), nbs, t2, dev(y), "matern32", order=order).backward()
    assert np.all(np.abs(t2.grad.numpy() - g) <= 1e-12 * np.abs(ref[:, 2:]).sum(0))
    with pytest.raises(NotImplementedError):
        pynngp_amd.loglik(dev(coords), dev(nbr), theta, dev(y), "matern")


def test_dense_values_gradient_restatement_error():
    """-K^-1 y at N = 32, theta (1.3, 6, 0.05): fp64 (numpy solve) against its longdouble twin (scalar Cholesky)
    stays below 1e-11 (1 + |x|), so the GPU bound 1e-9 (1 + |x|) is a fair one for these inputs."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("no extended precision here")
    coords, y = field(32, seed=7)
    d = np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(-1))
    K = 1.3 * np.exp(-6.0 * d) + 0.05 * np.eye(32)
    x64 = -np.linalg.solve(K, y)
    dl = np.sqrt(((coords.astype(np.longdouble)[:, None, :] - coords.astype(np.longdouble)[None, :, :]) ** 2).sum(-1))
    Kl = np.longdouble(1.3) * np.exp(-np.longdouble(6.0) * dl) + np.longdouble(0.05) * np.eye(32, dtype=np.longdouble)
    xl = -chol_solve(Kl, y.astype(np.longdouble)[:, None])[:, 0]
    err = float(np.max(np.abs(x64 - xl) / (1 + np.abs(xl))))
    print("fp64 vs longdouble, -K^-1 y:", err)
    assert err <= 1e-11


@pytest.mark.gpu
def test_autograd_values_dense():
    import pynngp_amd

    coords, y = field(32, seed=7)
    full = np.array([[j if j < i else -1 for j in range(31)] for i in range(32)], dtype=np.int32)
    d = np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(-1))
    K = 1.3 * np.exp(-6.0 * d) + 0.05 * np.eye(32)
    want = -np.linalg.solve(K, y)
    theta = torch.tensor((1.3, 6.0, 0.05), dtype=torch.float64, requires_grad=True)
    v = dev(y).requires_grad_(True)
    pynngp_amd.loglik(dev(coords), dev(full), theta, v, "exponential").backward()
    got = v.grad.cpu().numpy()
    err = np.abs(got - want) / (1 + np.abs(want))
    print("values.grad err:", err.max())
    assert err.max() <= 1e-9
    gd, _ = dense_grad(coords, "exponential", (1.3, 6.0, 0.05), y)
    assert np.all(np.abs(theta.grad.numpy() - gd) <= 1e-9 * (1 + np.abs(gd)))
    # the same through a visiting order (sorted rows + order): B, F and R sit at natural rows
    order, nbs = _lib.row_order(dev(coords), 0, 32, dev(full))
    assert not np.array_equal(order.cpu().numpy(), np.arange(32))
    v2 = dev(y).requires_grad_(True)
    t2 = torch.tensor((1.3, 6.0, 0.05), dtype=torch.float64)
    pynngp_amd.loglik(dev(coords), nbs, t2, v2, "exponential", order=order).backward()
    err = np.abs(v2.grad.cpu().numpy() - want) / (1 + np.abs(want))
    print("values.grad err with order:", err.max())
    assert err.max() <= 1e-9
