"""Fisher information sweep (nngp_bf_fisher) on the GPU against the numpy restatement of tests/fisher_ref.py
(pinned on the host by test_fisher_host.py), its siblings nngp_bf_grad, the dense GP's information, and the
methods built on it: NNGP.fisher_information, fit(stderr=True) and fit(method="fisher").

Row tolerance 1e-9 (1 + |ref|): the kernel family's (test_gpu_grad.py); test_fisher_host.py shows the fp64
restatement itself within 1e-11 (1 + |ref|) of extended precision on the same field for every m and kind.
"""
import numpy as np
import pytest
import torch

import fisher_ref as R
from pynngp_amd import _lib

pytestmark = pytest.mark.gpu

M_ALL = tuple(range(1, 33))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sweep(coords, nbr, kind, theta, y, i0=0, order=None, rows=True):
    out = _lib.bf_fisher(dev(coords), nbr if torch.is_tensor(nbr) else dev(nbr), i0, kind, *theta,
                         None if y is None else dev(y), want_rows=rows, order=order)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]  # partials, grad, info, I_rows, G


def close_rows(got, ref, what):
    err = float(np.max(np.abs(got - ref) / (1 + np.abs(ref))))
    print(f"max |d{what}| / (1 + |{what}|) = {err:.3e}")
    return err <= 1e-9


@pytest.fixture(scope="module")
def f96():
    coords, y = R.field(96, seed=1)
    return coords, y, {}


def nbr_of(cache, coords, m):
    if m not in cache:
        cache[m] = R.knn_prior(coords, m)
    return cache[m]


# ---------------------------------------------------------------- rows against the restatement
@pytest.mark.parametrize("m", M_ALL)
@pytest.mark.parametrize("kind", R.KINDS)
def test_rows_match_restatement(f96, kind, m):
    coords, y, cache = f96
    nbr = nbr_of(cache, coords, m)
    th = R.theta_of(kind)
    ref = R.rows_bf(coords, nbr, kind, th, y)
    p, g, info, I, G = sweep(coords, nbr, kind, th, y)
    assert p[2] == -1 and p[3] == -1
    assert close_rows(I, ref["I"], "I")
    assert close_rows(G, ref["G"], "G")
    assert np.all(np.abs(info - ref["I"].sum(0)) <= 1e-9 * (1 + np.abs(ref["I"])).sum(0))
    assert np.all(np.abs(g - ref["G"].sum(0)) <= 1e-9 * (1 + np.abs(ref["G"])).sum(0))
    assert abs(p[0] - ref["logF"].sum()) <= 1e-11 * np.abs(ref["logF"]).sum()
    assert abs(p[1] - ref["q"].sum()) <= 1e-11 * np.abs(ref["q"]).sum()


# ---------------------------------------------------------------- agreement with the siblings
@pytest.mark.parametrize("m", (1, 8, 10, 15, 17, 24, 31, 32))
def test_siblings_and_null_values(f96, m):
    coords, y, cache = f96
    nbr = nbr_of(cache, coords, m)
    for kind in ("exponential", "matern52", "spherical"):
        th = R.theta_of(kind)
        p, g, info, I, G = sweep(coords, nbr, kind, th, y)
        pg, gg, Gg = _lib.bf_grad(dev(coords), dev(nbr), 0, kind, *th, dev(y), want_rows=True)
        pg, gg, Gg = pg.cpu().numpy(), gg.cpu().numpy(), Gg.cpu().numpy()
        assert close_rows(G, Gg, "G")
        assert np.all(np.abs(g - gg) <= 1e-9 * (1 + np.abs(Gg)).sum(0))
        assert abs(p[0] - pg[0]) <= 1e-11 * abs(pg[0]) and abs(p[1] - pg[1]) <= 1e-11 * abs(pg[1])
        p0, g0, info0, I0, G0 = sweep(coords, nbr, kind, th, None)
        assert np.array_equal(info0, info) and np.array_equal(I0, I)  # bit for bit: the information reads no data
        assert np.array_equal(g0, np.zeros(3)) and np.array_equal(G0, np.zeros((96, 3))) and p0[1] == 0.0
        assert p0[0] == p[0] and p0[2] == -1 and p0[3] == -1


# ---------------------------------------------------------------- dimensions
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_dimensions(dim):
    coords, y = R.field(96, dim=dim, seed=2)
    for m in (10, 17, 24, 32):
        nbr = R.knn_prior(coords, m)
        for kind in ("exponential", "matern52"):
            ref = R.rows_bf(coords, nbr, kind, R.THETA, y)
            _, _, _, I, G = sweep(coords, nbr, kind, R.THETA, y)
            assert close_rows(I, ref["I"], "I") and close_rows(G, ref["G"], "G"), (dim, m, kind)


# ---------------------------------------------------------------- known answer
@pytest.mark.parametrize("kind", R.KINDS)
def test_dense_known_answer(kind):
    """m = n - 1 with every earlier point a neighbour: the row sum is the dense GP's information.  The sweep serves
    m <= 32, so the largest such field has n = 33 (the host test does n = 40 on the restatement)."""
    n = 33
    coords, _ = R.field(n, seed=1)
    th = R.theta_of(kind)
    dense = R.dense_info(coords, kind, th)
    _, _, info, I, _ = sweep(coords, R.full_sets(n), kind, th, None)
    print(kind, "rel err", np.abs(info - dense) / np.abs(dense))
    assert np.allclose(info, dense, rtol=1e-9, atol=0)
    assert np.allclose(I.sum(0), dense, rtol=1e-9, atol=0)


# ---------------------------------------------------------------- fold
@pytest.fixture(scope="module")
def f3000():
    coords, y = R.field(3000, seed=5)
    nbr = R.knn_prior(coords, 10)
    th = (1.0, 12.0, 0.1)
    return coords, y, nbr, th, sweep(coords, nbr, "exponential", th, y)


def test_fold_and_reproducibility(f3000):
    coords, y, nbr, th, (p, g, info, I, G) = f3000
    p2, g2, info2, I2, G2 = sweep(coords, nbr, "exponential", th, y)
    for a, b in ((p, p2), (g, g2), (info, info2), (I, I2), (G, G2)):
        assert np.array_equal(a, b)
    print("info err / sum|rows| =", np.abs(info - I.sum(0)) / np.abs(I).sum(0))
    assert np.all(np.abs(info - I.sum(0)) <= 1e-12 * np.abs(I).sum(0))
    assert np.all(np.abs(g - G.sum(0)) <= 1e-12 * np.abs(G).sum(0))
    ref = R.rows_bf(coords, nbr, "exponential", th, y)
    assert close_rows(I, ref["I"], "I") and close_rows(G, ref["G"], "G")


def test_subranges_sum_to_the_whole(f3000):
    coords, y, nbr, th, (p, g, info, I, G) = f3000
    cut = 1237
    a = sweep(coords, np.ascontiguousarray(nbr[:cut]), "exponential", th, y, i0=0)
    b = sweep(coords, np.ascontiguousarray(nbr[cut:]), "exponential", th, y, i0=cut)
    assert np.array_equal(np.concatenate([a[3], b[3]]), I) and np.array_equal(np.concatenate([a[4], b[4]]), G)
    assert np.all(np.abs(a[2] + b[2] - info) <= 1e-12 * np.abs(I).sum(0))
    assert np.all(np.abs(a[1] + b[1] - g) <= 1e-12 * np.abs(G).sum(0))
    assert abs(a[0][0] + b[0][0] - p[0]) <= 1e-11 * abs(p[0])


def test_visiting_order(f3000):
    coords, y, nbr, th, (p, g, info, I, G) = f3000
    order, nbr_sorted = _lib.row_order(dev(coords), 0, len(nbr), dev(nbr))
    po, go, infoo, Io, Go = sweep(coords, nbr_sorted, "exponential", th, y, order=order)
    assert np.array_equal(Io, I) and np.array_equal(Go, G)  # the same rows at their locations, bit for bit
    assert np.all(np.abs(infoo - I.sum(0)) <= 1e-12 * np.abs(I).sum(0))
    assert po[2] == -1 and po[3] == -1


# ---------------------------------------------------------------- flags and masking
def test_bad_index_is_flagged_and_masked(f96):
    coords, y, cache = f96
    ok = nbr_of(cache, coords, 10)
    nbr = ok.copy()
    nbr[60, 3] = 96  # one past the end
    p, g, info, I, G = sweep(coords, nbr, "exponential", R.THETA, y)
    assert p[3] == 60 and p[2] == -1
    assert np.all(np.isfinite(I)) and np.all(np.isfinite(G))
    p1, g1, info1, I1, G1 = sweep(coords, ok, "exponential", R.THETA, y)
    keep = np.arange(96) != 60
    assert np.array_equal(I[keep], I1[keep]) and np.array_equal(G[keep], G1[keep])
    masked = ok.copy()
    masked[60, 3] = -1  # the slot adds exactly 0: the row is that of the set without it
    ref = R.rows_bf(coords, masked, "exponential", R.THETA, y)
    assert close_rows(I[60], ref["I"][60], "I") and close_rows(G[60], ref["G"][60], "G")
    pm, _, _, Im, Gm = sweep(coords, masked, "exponential", R.THETA, y)
    assert pm[3] == -1 and np.array_equal(Im[60], I[60]) and np.array_equal(Gm[60], G[60])


def test_bad_pivot_is_flagged_with_nan_rows():
    coords, y = R.field(96, seed=1)
    coords[50] = coords[49]  # duplicate points, no nugget: C_N singular wherever both are neighbours
    nbr = R.knn_prior(coords, 5)
    p, g, info, I, G = sweep(coords, nbr, "exponential", (1.0, 6.0, 0.0), y)
    assert p[2] >= 0
    assert np.all(np.isnan(I[int(p[2])])) and np.all(np.isnan(G[int(p[2])]))


def test_flags_raise_through_the_methods():
    from pynngp_amd import nngp as N

    coords, y = R.field(96, seed=1)
    coords[50] = coords[49]
    model = N.NNGP(coords, y, None, "S=T", 5, N.Covariance("exponential", 1.0, 6.0, 0.0))
    with pytest.raises(N.NNGPNumericalError):
        model.fisher_information(values=y)
    with pytest.raises(N.NNGPNumericalError):
        model.fisher_information()


# ---------------------------------------------------------------- refusals
def test_refusals(f96):
    from pynngp_amd import nngp as N, ops

    coords, y, cache = f96
    c, v = dev(coords), dev(y)
    with pytest.raises(NotImplementedError):
        _lib.bf_fisher(c, dev(np.zeros((96, 33), np.int32)), 0, "exponential", 1.0, 1.0, 0.1, v)
    with pytest.raises(NotImplementedError):
        _lib.bf_fisher(c, dev(nbr_of(cache, coords, 5)), 0, "matern", 1.0, 1.0, 0.1, v)
    with pytest.raises(ValueError):
        _lib.bf_fisher(c, dev(nbr_of(cache, coords, 5)), 0, "exponential", 1.0, 1.0, 0.1, v[:50])
    with pytest.raises(ValueError):
        _lib.bf_fisher(c, dev(nbr_of(cache, coords, 5))[0], 0, "exponential", 1.0, 1.0, 0.1, v)
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.bf_fisher(c, dev(nbr_of(cache, coords, 5)), 0, "exponential", 1.0, 1.0, 0.1, v.cpu())
    ops.load()
    nb = dev(nbr_of(cache, coords, 5))
    with pytest.raises((RuntimeError, NotImplementedError)):  # no CPU kernel is registered
        torch.ops.nngp.bf_fisher(c.cpu(), nb.cpu(), None, 0, 0, 1.0, 1.0, 0.1, v.cpu(), False)
    with pytest.raises(RuntimeError):
        torch.ops.nngp.bf_fisher(c, nb, None, 0, 5, 1.0, 1.0, 0.1, v, False)  # the matern kind
    with pytest.raises(RuntimeError):
        torch.ops.nngp.bf_fisher(c, nb, None, 0, 0, 1.0, 1.0, 0.1, v[:50], False)
    # the operator agrees with the ctypes path bit for bit
    th = R.theta_of("matern32")
    a = ops.bf_fisher(c, nb, None, 0, "matern32", th, v, want_rows=True)
    b = _lib.bf_fisher(c, nb, 0, "matern32", *th, v, want_rows=True)
    for x, z in zip(a, b):
        assert torch.equal(x, z)
    a0 = ops.bf_fisher(c, nb, None, 0, "matern32", th)
    assert torch.equal(a0[2], a[2]) and a0[3].shape == (0, 6) and torch.equal(a0[1], torch.zeros_like(a0[1]))

    model = N.NNGP(coords, y, None, "S=T", 5, N.Covariance("exponential", 1.0, 8.0, 0.1))
    for kw in (dict(method="fisher"), dict(stderr=True)):
        with pytest.raises(NotImplementedError):
            model.fit(kind="matern", nu=0.7, **kw)
    with pytest.raises(NotImplementedError):
        model.fit(method="fisher", reml=True)
    with pytest.raises(NotImplementedError):
        model.fisher_information(cov=N.Covariance("matern", 1.0, 8.0, 0.1, nu=0.7))
    with pytest.raises(NotImplementedError):
        N.NNGP(coords, y, None, "S=T", 33, N.Covariance("exponential", 1.0, 8.0, 0.1)).fit(method="fisher")
    with pytest.raises(TypeError):
        N.NNGP(coords, y, None, "S=T", 5, lambda a, b: np.exp(-np.abs(a[:, None, 0] - b[None, :, 0]))).fit(
            method="fisher")
    with pytest.raises(ValueError):
        model.fisher_information(mean="constant")  # a mean needs values


# ---------------------------------------------------------------- NNGP.fisher_information
@pytest.fixture(scope="module")
def model400():
    from pynngp_amd import nngp as N

    coords, y = R.field(400, seed=9)
    rng = np.random.default_rng(3)
    X = np.column_stack([np.ones(400), rng.standard_normal((400, 2))])
    y = y + X @ np.array([0.7, -0.4, 0.25])
    cov = N.Covariance("matern32", 1.1, 7.0, 0.2)
    return N.NNGP(coords, y, None, "S=T", 10, cov), coords, y, X


def test_fisher_information_method(model400):
    model, coords, y, X = model400
    th = np.array([1.1, 7.0, 0.2])
    nbr = model.nbr.cpu().numpy()
    ref = R.rows_bf(coords, nbr, "matern32", tuple(th), y)
    out = model.fisher_information(values=y, rows=True)
    assert set(out) == {"info", "grad", "loglik", "I_rows", "G"}
    assert np.array_equal(out["info"], out["info"].T) and out["info"].shape == (3, 3)
    assert np.all(np.abs(out["info"] - R.info3(ref["I"].sum(0))) <= 1e-9 * R.info3((1 + np.abs(ref["I"])).sum(0)))
    assert np.all(np.abs(out["grad"] - ref["G"].sum(0)) <= 1e-9 * (1 + np.abs(ref["G"])).sum(0))
    assert close_rows(out["I_rows"], ref["I"], "I") and close_rows(out["G"], ref["G"], "G")
    assert abs(out["loglik"] - model.loglik(y)) <= 1e-11 * abs(out["loglik"])
    assert np.all(np.linalg.eigvalsh(out["info"]) > 0)
    # log-parameter forms
    lg = model.fisher_information(values=y, log=True, rows=True)
    assert np.allclose(lg["info"], np.diag(th) @ out["info"] @ np.diag(th), rtol=1e-15, atol=0)
    assert np.allclose(lg["grad"], th * out["grad"], rtol=1e-15, atol=0)
    assert np.allclose(lg["G"], out["G"] * th, rtol=1e-15, atol=0)
    assert np.allclose(lg["I_rows"][:, 1], out["I_rows"][:, 1] * th[0] * th[1], rtol=1e-15, atol=0)
    # design stage: the information alone, the bits of the call with values
    d = model.fisher_information()
    assert np.array_equal(d["info"], out["info"]) and np.array_equal(d["grad"], np.zeros(3)) and d["loglik"] is None
    # profiled means: the call on the residual
    c = model.fisher_information(values=y, mean="constant")
    ll, mu, g = model.profile_loglik_grad(model.cov, y)
    r = model.fisher_information(values=y - mu)
    assert c["mu"] == mu and np.array_equal(c["grad"], r["grad"]) and np.array_equal(c["info"], out["info"])
    assert abs(c["loglik"] - ll) <= 1e-11 * abs(ll) and np.all(np.abs(c["grad"] - g) <= 1e-9 * (1 + np.abs(g)))
    lin = model.fisher_information(values=y, mean="linear", X=X)
    ll, beta, g = model.profile_loglik_grad(model.cov, y, mean="linear", X=X)
    r = model.fisher_information(values=y - X @ beta)
    assert np.array_equal(lin["beta"], beta) and np.allclose(lin["grad"], r["grad"], rtol=1e-10, atol=1e-10)
    assert abs(lin["loglik"] - ll) <= 1e-11 * abs(ll) and np.all(np.abs(lin["grad"] - g) <= 1e-9 * (1 + np.abs(g)))


def test_fit_stderr(model400):
    from pynngp_amd import nngp as N

    _, coords, y, _ = model400
    start = N.Covariance("exponential", 0.8, 6.0, 0.3)
    plain = N.NNGP(coords, y, None, "S=T", 10, start).fit(gradient=True, maxiter=40)
    assert set(plain) == {"theta", "mu", "loglik", "n_evals", "n_grad_evals", "converged"}
    nm = N.NNGP(coords, y, None, "S=T", 10, start).fit(maxiter=5)
    assert set(nm) == {"theta", "mu", "loglik", "n_evals", "converged"}
    model = N.NNGP(coords, y, None, "S=T", 10, start)
    res = model.fit(gradient=True, maxiter=40, stderr=True)
    assert set(res) == set(plain) | {"info", "cov_theta", "se"}
    assert res["theta"] == plain["theta"] and res["loglik"] == plain["loglik"]
    rows = R.rows_bf(coords, model.nbr.cpu().numpy(), "exponential", res["theta"])["I"]
    ref = R.info3(rows.sum(0))
    se = np.sqrt(np.diag(np.linalg.inv(ref)))
    # the sums' tolerance 1e-9 sum(1 + |rows|), relative to the sums, through an inverse whose relative error is at
    # most the condition number of the unit-diagonal form times that
    s = 1.0 / np.sqrt(np.diag(ref))
    rtol = 1e-9 * np.linalg.cond(ref * np.outer(s, s)) * float(np.max((1 + np.abs(rows)).sum(0) / np.abs(rows.sum(0))))
    print("se", res["se"], "restatement", se, "rtol", rtol)
    assert rtol < 1e-4 and np.allclose(res["se"], se, rtol=rtol, atol=0)
    assert np.allclose(res["cov_theta"], np.linalg.inv(res["info"]), rtol=1e-9, atol=0)
    fx = N.NNGP(coords, y, None, "S=T", 10, start).fit(gradient=True, maxiter=40, stderr=True, fix_tau2=0.25)
    assert fx["info"].shape == (2, 2) and fx["se"].shape == (2,)


# ---------------------------------------------------------------- Fisher scoring
@pytest.fixture(scope="module")
def sim2000():
    from pynngp_amd import nngp as N

    n = 2000
    coords, _ = R.field(n, seed=11)
    rng = np.random.default_rng(12)
    X = np.column_stack([np.ones(n), rng.standard_normal((n, 2))])
    gen = N.NNGP(coords, np.zeros(n), None, "S=T", 10, N.Covariance("exponential", 1.0, 12.0, 0.1))
    y = gen.simulate(1, seed=7, beta=0.5)[0]
    y_lin = gen.simulate(1, seed=7)[0] + X @ np.array([0.5, -0.3, 0.2])
    y_clean = gen.simulate(1, seed=7, noise=False, beta=0.5)[0]
    return coords, X, y, y_lin, y_clean


def check_scoring(make, th_index, label, **kw):
    from pynngp_amd import nngp as N

    start = N.Covariance("exponential", 0.5, 5.0, 0.3)
    lb = make(start).fit(gradient=True, **kw)
    model = make(start)
    fs = model.fit(method="fisher", **kw)
    print(f"{label}: fisher n_iter={fs['n_iter']} n_evals={fs['n_evals']} loglik={fs['loglik']:.9f} | L-BFGS-B "
          f"n_evals={lb['n_evals']} loglik={lb['loglik']:.9f} | theta={fs['theta']} se={fs['se']}")
    assert fs["converged"]
    assert fs["loglik"] >= lb["loglik"] - 1e-5 * (1 + abs(lb["loglik"]))
    _, _, g = model.profile_loglik_grad(model.cov, mean=kw.get("mean", "constant"), X=kw.get("X"))
    score = np.abs(np.array(fs["theta"]) * g)[th_index]
    print(f"{label}: max |theta_k dl/dtheta_k| = {score.max():.3e}")
    assert score.max() <= 1e-3
    assert set(fs) >= {"theta", "mu", "loglik", "n_evals", "converged", "n_iter", "info", "cov_theta", "se"}
    assert fs["info"].shape == (len(th_index),) * 2 and np.all(fs["se"] > 0)
    return fs, lb


def test_fisher_scoring_constant_mean(sim2000):
    from pynngp_amd import nngp as N

    coords, X, y, _, _ = sim2000
    fs, _ = check_scoring(lambda c: N.NNGP(coords, y, None, "S=T", 10, c), [0, 1, 2], "constant")
    assert abs(fs["mu"] - 0.5) < 0.5 and "n_grad_evals" not in fs


def test_fisher_scoring_fixed_zero_nugget(sim2000):
    from pynngp_amd import nngp as N

    coords, X, _, _, y_clean = sim2000
    fs, _ = check_scoring(lambda c: N.NNGP(coords, y_clean, None, "S=T", 10, c), [0, 1], "fix_tau2=0", fix_tau2=0.0)
    assert fs["theta"][2] == 0.0


def test_fisher_scoring_linear_mean(sim2000):
    from pynngp_amd import nngp as N

    coords, X, _, y_lin, _ = sim2000
    fs, lb = check_scoring(lambda c: N.NNGP(coords, y_lin, None, "S=T", 10, c), [0, 1, 2], "linear", mean="linear",
                           X=X)
    assert fs["mu"] is None and fs["beta"].shape == (3,) and fs["cov_beta"].shape == (3, 3)
    model = N.NNGP(coords, y_lin, None, "S=T", 10, N.Covariance("exponential", *fs["theta"]))
    g = model.gls(model.cov, X)
    assert np.array_equal(fs["beta"], g.beta) and np.array_equal(fs["cov_beta"], g.cov_beta)
