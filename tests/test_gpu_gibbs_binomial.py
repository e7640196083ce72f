"""GPU: the binomial / logistic NNGP sampler (pynngp_amd.BinomialSeqNNGP) and its statistics kernel.

The stationary-law test compares the GPU chain with a dense numpy restatement of the same Gibbs sampler kept
in this file; its Polya-Gamma draws come from an independent construction (the sum-of-gammas series of Polson,
Scott and Windle truncated at 200 terms plus the mean of the dropped tail) -- nothing of polya_gamma.h is shared.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------- statistics kernel
def test_pg_stats_against_numpy(dev):
    from pynngp_amd import _lib

    rng = np.random.default_rng(0)
    n, p = 1000, 3
    r, w = rng.normal(size=n), rng.normal(size=n)
    Ft = rng.uniform(0.2, 1.0, n)
    om = rng.uniform(0.0, 2.0, n)
    om[::7] = 0.0
    kap = rng.integers(-3, 4, n) * 0.5
    X = rng.normal(size=(n, p))
    t = lambda a: torch.as_tensor(a).to(dev)  # noqa: E731
    args = (t(r), t(Ft), t(om), t(kap), t(X), t(w))
    got = _lib.gibbs_pg_stats(*args).cpu().numpy()
    again = _lib.gibbs_pg_stats(*args).cpu().numpy()
    assert got.shape == (1 + 6 + 3,) and np.array_equal(got, again)  # bit-identical across calls
    iu = np.triu_indices(p)
    terms = [r * r / Ft] + [X[:, a] * om * X[:, b] for a, b in zip(*iu)] + [X[:, c] * (kap - om * w) for c in range(p)]
    for v, term in enumerate(terms):
        assert abs(got[v] - term.sum()) <= 1e-12 * np.abs(term).sum(), v


# ---------------------------------------------------------------------------- stationary law
def _nngp_factors(coords, m, phi):
    """Dense restatement: B (n, n) strictly lower triangular over the m nearest earlier points, F (n,) of the
    unit-variance exponential field."""
    n = coords.shape[0]
    D = np.linalg.norm(coords[:, None] - coords[None], axis=2)
    C = np.exp(-phi * D)
    B, F = np.zeros((n, n)), np.ones(n)
    for i in range(1, n):
        nb = np.argsort(D[i, :i], kind="stable")[:m]
        b = np.linalg.solve(C[np.ix_(nb, nb)], C[nb, i])
        B[i, nb] = b
        F[i] = 1.0 - b @ C[nb, i]
    return B, F


def _pg_series(rng, b, c, terms=200):
    """PG(b, c) = (1 / 2 pi^2) sum_k g_k / ((k - 1/2)^2 + c^2 / 4 pi^2), g_k ~ Gamma(b, 1): the first `terms`
    terms drawn, the rest replaced by its mean.  (b, c) arrays; b = 0 gives 0."""
    k = np.arange(1, terms + 1)[None, :]
    d = (k - 0.5) ** 2 + (c[:, None] / (2 * math.pi)) ** 2
    g = rng.gamma(np.maximum(b, 1)[:, None], 1.0, size=d.shape)
    # tail mean: b sum_{k > terms} 1 / d_k ~ b integral, midpoint rule from terms + 1/2 (error ~ 1e-8)
    a = np.abs(c) / (2 * math.pi)
    x0 = float(terms)
    with np.errstate(divide="ignore", invalid="ignore"):
        tail = np.where(a > 1e-12, (math.pi / 2 - np.arctan(x0 / np.maximum(a, 1e-300))) / np.maximum(a, 1e-300), 1.0 / x0)
    out = ((g / d).sum(axis=1) + b * tail) / (2 * math.pi ** 2)
    return np.where(b > 0, out, 0.0)


def _numpy_chain(coords, s, b, m, phi, sigma2, n_iter, seed):
    """The same Gibbs sampler, dense: omega | eta; w_i | rest site by site from the dense NNGP precision;
    beta | omega, w (p = 1, intercept).  Returns the draws of logistic(eta) (n_iter, n) and beta (n_iter,)."""
    rng = np.random.default_rng(seed)
    n = coords.shape[0]
    B, F = _nngp_factors(coords, m, phi)
    IB = np.eye(n) - B
    Q = IB.T @ (IB / F[:, None]) / sigma2
    kap = np.where(b > 0, s - 0.5 * b, 0.0)
    w, beta = np.zeros(n), 0.0
    P, Bt = np.empty((n_iter, n)), np.empty(n_iter)
    for it in range(n_iter):
        om = _pg_series(rng, b, beta + w)
        z = rng.standard_normal(n)
        for i in range(n):
            prec = Q[i, i] + om[i]
            lin = (kap[i] - om[i] * beta) - (Q[i] @ w - Q[i, i] * w[i])
            w[i] = lin / prec + z[i] / math.sqrt(prec)
        v = 1.0 / om.sum()
        beta = v * (kap - om * w).sum() + math.sqrt(v) * rng.standard_normal()
        P[it] = 1.0 / (1.0 + np.exp(-(beta + w)))
        Bt[it] = beta
    return P, Bt


def _batch_means(x, n_batches=40):
    """(mean, Monte-Carlo standard error) per column by batch means"""
    x = x.reshape(x.shape[0], -1)
    bm = x.reshape(n_batches, x.shape[0] // n_batches, -1).mean(axis=1)
    return bm.mean(axis=0), bm.std(axis=0, ddof=1) / math.sqrt(n_batches)


STAT = dict(n=40, m=5, phi=6.0, sigma2=1.0, burn=500, keep=4000)


def _stationary_data():
    rng = np.random.default_rng(12)
    n = STAT["n"]
    coords = rng.uniform(0, 1, (n, 2))
    b = np.array([0, 1, 5])[np.arange(n) % 3]
    pr = 1.0 / (1.0 + np.exp(-(0.3 + rng.normal(0, 1, n))))
    s = rng.binomial(b, pr).astype(np.float64)
    return coords, s, b


def test_stationary_law_against_dense_numpy(dev):
    from pynngp_amd import BinomialSeqNNGP

    coords, s, b = _stationary_data()
    n_iter = STAT["burn"] + STAT["keep"]
    g = BinomialSeqNNGP(coords, s, b, m=STAT["m"], kind="exponential", phi=STAT["phi"], sigma2=STAT["sigma2"],
                        fix_phi=True, fix_sigma2=True, seed=5, device=dev)
    Pg, Bg = np.empty((n_iter, STAT["n"])), np.empty(n_iter)
    for it in range(n_iter):
        g.step()
        Pg[it] = g.probability("data").cpu().numpy()
        Bg[it] = g.beta[0]
    Pn, Bn = _numpy_chain(coords, s, b, STAT["m"], STAT["phi"], STAT["sigma2"], n_iter, seed=77)
    k = STAT["burn"]
    for name, a, c in (("prob", Pg[k:], Pn[k:]), ("beta", Bg[k:], Bn[k:])):
        m1, e1 = _batch_means(a)
        m2, e2 = _batch_means(c)
        z = np.abs(m1 - m2) / np.sqrt(e1 ** 2 + e2 ** 2)
        print(name, "largest |difference| in combined MC standard errors:", float(z.max()))
        assert np.all(z <= 5.0), (name, z)


# ---------------------------------------------------------------------------- usefulness
def _logistic_field(n, seed, trials):
    rng = np.random.default_rng(seed)
    coords = rng.uniform(0, 1, (n, 2))
    # a smooth field: a few random cosine waves, sd ~ 1.2
    eta = -0.4 + sum(0.8 * np.cos(coords @ rng.normal(0, 4.0, 2) + rng.uniform(0, 6.28)) for _ in range(5))
    pr = 1.0 / (1.0 + np.exp(-eta))
    return coords, pr, rng.binomial(trials, pr).astype(np.float64), rng


def test_held_out_brier_beats_pooled_rate(dev):
    from pynngp_amd import BinomialSeqNNGP

    n = 1500
    coords, pr, s, rng = _logistic_field(n, 4, 10)
    b = np.full(n, 10)
    held = rng.permutation(n)[: n // 5]
    b[held] = 0
    g = BinomialSeqNNGP(coords, s, b, m=10, seed=1, device=dev)
    res = g.run(500, burn=200)
    assert np.array_equal(np.sort(g.unobserved_t), np.sort(held))
    phat = res["prob_unobserved_mean"][: held.size]
    truth = pr[g.unobserved_t]
    obs = b > 0
    pooled = s[obs].sum() / b[obs].sum()
    brier, brier0 = np.mean((phat - truth) ** 2), np.mean((pooled - truth) ** 2)
    print("held-out Brier", brier, "pooled rate", brier0)
    assert brier < brier0
    assert res["beta"].shape == (300, 1) and set(res["summary"]["phi"]) == {"mean", "q025", "q50", "q975"}
    assert res["prob_mean"].shape == (n,) and np.all((res["prob_mean"] > 0) & (res["prob_mean"] < 1))


# ---------------------------------------------------------------------------- checkpoint, S != T, refusals
def _small(dev, seed=3, **kw):
    from pynngp_amd import BinomialSeqNNGP

    coords, _, s, rng = _logistic_field(600, 9, 3)
    b = np.full(600, 3)
    b[::6] = 0
    s[5] = np.nan
    X = np.column_stack([np.ones(600), coords[:, 0]])
    return BinomialSeqNNGP(coords, s, b, X=X, m=8, seed=seed, device=dev, trials_unobserved=3, **kw), coords


def test_checkpoint_resumes_bit_for_bit(dev, tmp_path):
    a, _ = _small(dev)
    for _ in range(5):
        a.step()
    path = str(tmp_path / "ck.npz")
    a.save(path)
    for _ in range(5):
        a.step()
    c, _ = _small(dev)
    c.load(path)
    assert torch.equal(c.prob_unobserved, _small_prob_at_save(a, path, dev))
    for _ in range(5):
        c.step()
    assert torch.equal(a.w, c.w) and np.array_equal(a.beta, c.beta)
    assert a.sigma2 == c.sigma2 and a.phi == c.phi and a.iteration == c.iteration == 10
    assert torch.equal(a.prob_unobserved, c.prob_unobserved) and torch.equal(a.y_unobserved, c.y_unobserved)


def _small_prob_at_save(a, path, dev):
    """logistic(x beta + w) at the unobserved nodes from the checkpoint's own (w, beta)"""
    with np.load(path, allow_pickle=False) as z:
        w = torch.as_tensor(z["w"]).to(dev)[a.perm]
        beta = torch.as_tensor(z["beta"]).to(dev)
    return torch.sigmoid(a._un_X @ beta + w[a._un_nodes])


def test_reference_set(dev):
    from pynngp_amd import BinomialSeqNNGP

    coords, _, s, rng = _logistic_field(600, 10, 4)
    ref = rng.uniform(0, 1, (200, 2))
    g = BinomialSeqNNGP(coords, s, np.full(600, 4), m=6, ref=ref, seed=2, device=dev)
    assert g.n == 800 and g.n_s == 200
    w0 = g.w_t.clone()
    for _ in range(20):
        g.step()
    assert bool(torch.isfinite(g.w).all()) and np.all(np.isfinite(g.beta)) and math.isfinite(g.sigma2)
    assert math.isfinite(g.phi)
    assert bool((g.w_t != w0).all())  # the leaves are updated
    for where in ("data", "nodes", "unobserved"):
        pr = g.probability(where)
        assert bool(((pr > 0) & (pr < 1)).all()), where
    assert g.prob_unobserved.numel() == 200  # the reference points carry no data


def test_refusals(dev):
    from pynngp_amd import BinomialSeqNNGP, SeqNNGPChains, ShardedSeqNNGP

    rng = np.random.default_rng(0)
    coords = rng.uniform(0, 1, (50, 2))
    s, b = np.ones(50), np.ones(50, dtype=np.int64)
    for cls in (SeqNNGPChains, ShardedSeqNNGP):
        with pytest.raises(NotImplementedError, match="binomial"):
            cls(coords, s, trials=b)
        with pytest.raises(NotImplementedError, match="binomial"):
            cls(coords, s, family="binomial")
    bad = s.copy()
    bad[3] = 2.0
    with pytest.raises(ValueError, match="successes"):
        BinomialSeqNNGP(coords, bad, b, device=dev)
    with pytest.raises(ValueError, match="integers"):
        BinomialSeqNNGP(coords, s * 0.5, b, device=dev)
    with pytest.raises(ValueError, match="trials"):
        BinomialSeqNNGP(coords, s, b * 2000, device=dev)
    with pytest.raises(ValueError, match="eps"):
        BinomialSeqNNGP(coords, s, b, eps=np.ones(50), device=dev)
    with pytest.raises(NotImplementedError):
        BinomialSeqNNGP(coords, s, b, sweep="tiled", device=dev)
    with pytest.raises(NotImplementedError):
        BinomialSeqNNGP(coords, s, b, cov=lambda a, c: 1.0, device=dev)
    g = BinomialSeqNNGP(coords, s, b, device=dev)
    with pytest.raises(NotImplementedError, match="binomial"):
        SeqNNGPChains(g, None)
