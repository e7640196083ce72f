"""GPU: the binomial latent posterior by Laplace approximation -- nngp_binomial_newton_step and nngp_logistic_normal
against extended-precision restatements, and BinomialLatentPosterior (mode, Laplace evidence, predictions, fit, draws)
against dense numpy algebra built from the class's own B, F and nbr (storage order throughout).

Tolerances.  Link kernel: the fp64 numpy restatement of the header's formulas against its np.longdouble twin on the
test's input, measured in the test and printed (9.4e-14: eta = offset + w is rounded once in fp64, which exp
magnifies at |eta| ~ 745; the kernel itself is 2.3e-14 from the twin), times 8 -- the test_gpu_grad.py convention.  Relative errors are taken against max(|exact|, max_trials * 2^-1022): e = exp(-|eta|) is subnormal beyond
|eta| = 708.4 and then carries an absolute error of one unit of 2^-1074, which b e / (1 + e)^2 scales by at most
max_trials -- below that floor fp64 holds no relative precision.  logistic_normal: 1e-8 absolute against mpmath.quad
(the issue's bound).  Mode: the strong-concavity bound |x - x*|_2 <= |grad|_2 / lambda_min with |grad|_2 <= sqrt(N)
|grad|_inf and the factor 2 of the dense gradient check."""
import functools
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIGMA2, PHI = 1.5, 6.0
TINY = 2.0 ** -1022


def _dt(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)


# ---------------------------------------------------------------- 1. the link kernel
def link_restatement(trials, succ, offset, w, ft):
    """include/nngp.h's formulas in the float type ``ft`` (np.float64: the kernel's operations; np.longdouble: the
    reference): (d, rhs, g, l)."""
    b, s, wv = trials.astype(ft), succ.astype(ft), w.astype(ft)
    eta = offset.astype(ft) + wv
    a = np.abs(eta)
    e = np.exp(-a)
    den = 1 + e
    big, small = 1 / den, e / den
    pos = eta >= 0
    p, q = np.where(pos, big, small), np.where(pos, small, big)
    d = b * (e / (den * den))
    g = s * q - (b - s) * p
    rhs = d * wv + g
    ll = -(np.where(pos, b - s, s) * a) - b * np.log1p(e)
    z = trials == 0
    return tuple(np.where(z, ft(0), v) for v in (d, rhs, g, ll))


@functools.lru_cache(maxsize=None)
def link_input(n=1000):
    rng = np.random.default_rng(42)
    special = np.array([0.0, 1e-300, -1e-300, 36, -36, 709, -709, 745, -745, 800, -800, 1e6, -1e6])
    eta = rng.normal(0.0, 3.0, n)
    trials = rng.choice([0, 1, 7, 10 ** 6], n).astype(np.int32)
    k = 0
    for b in (1, 7, 10 ** 6, 0):  # every special eta with every trials value
        for e in special:
            eta[k], trials[k] = e, b
            k += 1
    kind = rng.integers(0, 3, n)  # successes: 0, b, mid
    succ = np.where(kind == 0, 0, np.where(kind == 1, trials, trials // 2)).astype(np.float64)
    w = rng.normal(0.0, 1.0, n)
    w[:k] = np.where(np.abs(eta[:k]) < 1e-200, eta[:k], w[:k])  # eta = +-1e-300 needs offset = 0
    offset = eta - w
    offset[:k] = np.where(np.abs(eta[:k]) < 1e-200, 0.0, offset[:k])
    out = (trials, succ, offset, w)
    for a in out:
        a.setflags(write=False)
    return out


def _rel(x, exact, floor):
    return float(np.max(np.abs(x.astype(np.longdouble) - exact) / np.maximum(np.abs(exact), floor)))


def test_link_kernel_matches_longdouble_restatement(dev):
    from pynngp_amd import _lib

    trials, succ, offset, w = link_input()
    n = trials.size
    floor = np.longdouble(10 ** 6) * np.longdouble(TINY)
    ex = link_restatement(trials, succ, offset, w, np.longdouble)
    f64 = link_restatement(trials, succ, offset, w, np.float64)
    measured = max(_rel(a, b, floor) for a, b in zip(f64[:3], ex[:3]))
    tol = 8.0 * measured
    args = [_dt(a, dev) for a in (trials, succ, offset, w)]
    d, rhs, g, part = _lib.binomial_newton_step(*args)
    got = [t.cpu().numpy() for t in (d, rhs, g)]
    errs = [_rel(a, b, floor) for a, b in zip(got, ex[:3])]
    print(f"fp64 restatement vs longdouble {measured:.3g}; kernel d/rhs/g {errs}; asserted {tol:.3g}")
    assert measured > 0
    assert max(errs) <= tol
    z = trials == 0
    for a in got:
        assert np.all(a[z] == 0.0) and np.all(np.isfinite(a))
    p0 = part.cpu().numpy()
    p1 = _lib.binomial_newton_step(*args)[3].cpu().numpy()
    assert p0.tobytes() == p1.tobytes()  # the fold is fixed-order
    sum_ex = ex[3].sum()
    print(f"sum l: kernel {p0[0]!r} exact {float(sum_ex)!r}")
    assert abs(np.longdouble(p0[0]) - sum_ex) <= tol * n * abs(sum_ex)
    assert p0[1] == np.abs(got[2]).max() and p0[2] == 0.0 and p0[3] == 0.0
    # the ops path gives the same bits
    from pynngp_amd import load_ops

    load_ops()
    o = torch.ops.nngp.binomial_newton_step(*args)
    assert all(torch.equal(a, b) for a, b in zip(o, (d, rhs, g, part)))


def test_link_kernel_reports_a_nan_eta_as_data(dev):
    from pynngp_amd import _lib

    trials, succ, offset, w = (a.copy() for a in link_input())
    k = 613
    trials[k], w[k] = 7, np.nan
    d, rhs, g, part = _lib.binomial_newton_step(*[_dt(a, dev) for a in (trials, succ, offset, w)])
    p = part.cpu().numpy()
    assert p[2] == k + 1 and p[3] == 0.0 and np.isfinite(p[0]) and np.isfinite(p[1])
    assert np.isnan(d[k].item()) and np.isnan(rhs[k].item()) and np.isnan(g[k].item())
    assert _lib.binomial_check_partials(p) == (k, -1)
    trials[5] = -3
    p = _lib.binomial_newton_step(*[_dt(a, dev) for a in (trials, succ, offset, w)])[3].cpu().numpy()
    assert p[2] == k + 1 and p[3] == 6.0


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_link_kernel_block_record_edges(dev, n):
    from pynngp_amd import _lib

    rng = np.random.default_rng(n)
    trials = rng.choice([0, 1, 7], n).astype(np.int32)
    succ = np.floor(rng.uniform(size=n) * (trials + 1)).astype(np.float64)
    offset, w = rng.normal(0, 2, n), rng.normal(0, 1, n)
    ex = link_restatement(trials, succ, offset, w, np.longdouble)
    f64 = link_restatement(trials, succ, offset, w, np.float64)
    d, rhs, g, part = _lib.binomial_newton_step(*[_dt(a, dev) for a in (trials, succ, offset, w)])
    p = part.cpu().numpy()
    # fp64 terms summed in another order: n roundings of the partial sums (<= sum |l|), plus the terms' own error
    bound = (n + 8) * 2.0 ** -52 * float(np.abs(ex[3]).sum()) + 1e-300
    assert abs(np.longdouble(p[0]) - ex[3].sum()) <= bound
    assert p[1] == np.abs(g.cpu().numpy()).max() and p[2] == 0 and p[3] == 0
    assert np.allclose(g.cpu().numpy(), f64[2], rtol=1e-14, atol=1e-14)
    assert np.allclose(d.cpu().numpy(), f64[0], rtol=1e-14, atol=0)


# ---------------------------------------------------------------- 2. logistic_normal
MUS, SDS = [-30.0, -5.0, -0.3, 0.0, 2.0, 30.0], [0.0, 1e-8, 0.5, 2.0, 5.0, 10.0]


@functools.lru_cache(maxsize=None)
def logistic_normal_exact(mu, s):
    import mpmath as mp

    mp.mp.dps = 30
    if s == 0:
        return float(1 / (1 + mp.e ** (-mp.mpf(mu))))
    f = lambda x: mp.npdf(x) / (1 + mp.e ** (-(mu + s * x)))  # noqa: E731
    pts = sorted({-40.0, -10.0, -3.0, 0.0, 3.0, 10.0, 40.0, min(max(-mu / s, -40.0), 40.0)})
    return float(mp.quad(f, pts))


def test_logistic_normal_matches_mpmath(dev):
    from pynngp_amd import _lib

    grid = [(m, s) for m in MUS for s in SDS]
    mu, sd = np.array([g[0] for g in grid]), np.array([g[1] for g in grid])
    got = _lib.logistic_normal(_dt(mu, dev), _dt(sd, dev)).cpu().numpy()
    exact = np.array([logistic_normal_exact(m, s) for m, s in grid])
    err = np.abs(got - exact)
    print(f"logistic_normal max abs err {err.max():.3g} at {grid[int(err.argmax())]}")
    assert err.max() <= 1e-8
    # s = 0: the link kernel's p, to the last bit (g = s - b p with s = 0, b = 1 is -p)
    z = sd == 0
    m0 = np.ascontiguousarray(mu[z])
    one = torch.ones(m0.size, dtype=torch.int32, device=dev)
    zero = torch.zeros(m0.size, dtype=torch.float64, device=dev)
    g = _lib.binomial_newton_step(one, zero, _dt(m0, dev), zero)[2].cpu().numpy()
    assert np.array_equal(got[z], -g)
    from pynngp_amd import load_ops

    load_ops()
    assert torch.equal(torch.ops.nngp.logistic_normal(_dt(mu, dev), _dt(sd, dev)), _dt(got, dev))


# ---------------------------------------------------------------- dense algebra on the class's own factors
def dense_Q(nbr, B, F, sigma2):
    n = F.size
    L = np.eye(n)
    for i in range(n):
        for k in range(nbr.shape[1]):
            if nbr[i, k] >= 0:
                L[i, nbr[i, k]] -= B[i, k]
    return L.T @ (L / (sigma2 * F)[:, None])


def dense_parts(x, Q, X, trials, succ):
    p = X.shape[1]
    beta, w = x[:p], x[p:]
    d, _, g, ll = link_restatement(trials, succ, X @ beta, w, np.float64)
    grad = np.concatenate([X.T @ g, g - Q @ w])
    H = np.block([[X.T @ (d[:, None] * X), X.T * d], [d[:, None] * X, Q + np.diag(d)]])
    return grad, H, ll.sum() - 0.5 * w @ Q @ w, d


def dense_mode(Q, X, trials, succ, tol=1e-13):
    x = np.zeros(X.shape[1] + Q.shape[0])
    best = (np.inf, x)
    for _ in range(60):
        grad, H, lp, _ = dense_parts(x, Q, X, trials, succ)
        gn = np.abs(grad).max()
        if gn < best[0]:
            best = (gn, x.copy())
        if gn <= tol:
            break
        step, t = np.linalg.solve(H, grad), 1.0
        while t > 1e-6 and dense_parts(x + t * step, Q, X, trials, succ)[2] < lp - 1e-12 * abs(lp):
            t *= 0.5
        x = x + t * step
    return best[1], best[0]


@functools.lru_cache(maxsize=None)
def setup_data(kind, n=300):
    """(coords, X, succ, trials, ref, held-out points and their X) of set-up 3: kind in bern / tri5 / sat, each with
    and without a reference set."""
    rng = np.random.default_rng(7)
    coords = rng.uniform(size=(n + 40, 2))
    X = np.column_stack([np.ones(n + 40), coords[:, 0]])
    field = np.sin(5 * coords[:, 0]) * np.cos(4 * coords[:, 1]) * 1.3
    pr = 1 / (1 + np.exp(-(0.3 - 0.8 * coords[:, 0] + field)))
    b = 5 if kind == "tri5" else 1
    trials = np.full(n + 40, b)
    succ = rng.binomial(b, pr).astype(np.float64)
    trials[rng.choice(n, 20, replace=False)] = 0  # 20 rows unobserved
    if kind == "sat":  # the 10 points nearest the centre: all successes
        near = np.argsort(((coords[:n] - 0.5) ** 2).sum(axis=1))[:10]
        trials[near], succ[near] = 5, 5.0
    ref = np.concatenate([coords[:30], rng.uniform(size=(90, 2))])  # 120 points, 30 of them data locations
    out = dict(coords=coords[:n], X=X[:n], succ=succ[:n], trials=trials[:n], ref=ref, q=coords[n:], Xq=X[n:])
    for a in out.values():
        a.setflags(write=False)
    return out


_POSTS = {}


def get_post(dev, kind, with_ref):
    """The class on a set-up with its mode computed at gtol 1e-8, and the dense system (shared, read-only)."""
    from pynngp_amd import BinomialLatentPosterior, Covariance

    key = (kind, with_ref)
    if key not in _POSTS:
        c = setup_data(kind)
        post = BinomialLatentPosterior(c["coords"], c["succ"], c["trials"], Covariance("exponential", SIGMA2, PHI), m=10,
                                       X=c["X"], device=dev, ref=c["ref"] if with_ref else None)
        beta, _, info = post.mode(gtol=1e-8)
        Q = dense_Q(post.nbr.cpu().numpy(), post.B.cpu().numpy(), post.F.cpu().numpy(), SIGMA2)
        dense = dict(Q=Q, X=post.X.cpu().numpy(), trials=post.trials.cpu().numpy(), succ=post.successes.cpu().numpy())
        xs, gs = dense_mode(Q, dense["X"], dense["trials"], dense["succ"])
        dense.update(xs=xs, gs=gs)
        _POSTS[key] = (post, beta, info, dense)
    return _POSTS[key]


CASES = [("bern", False), ("tri5", False), ("bern", True), ("tri5", True), ("sat", False), ("sat", True)]


# ---------------------------------------------------------------- 3. the mode is the mode
@pytest.mark.parametrize("kind,with_ref", CASES)
def test_mode_is_the_mode(dev, kind, with_ref):
    post, _, _, dn = get_post(dev, kind, with_ref)
    beta, info = post._beta, post._mode["info"]
    gtol, bmax = 1e-8, max(1, int(dn["trials"].max()))
    assert post.n_nodes == (390 if with_ref else 300) and post.max_trials == bmax
    x = np.concatenate([beta, post._w.cpu().numpy()])
    grad, _, _, _ = dense_parts(x, dn["Q"], dn["X"], dn["trials"], dn["succ"])
    print(f"{kind} ref={with_ref}: steps {info.newton_steps} cg {info.cg_iterations} reported |grad| "
          f"{info.grad_norm:.3g} dense |grad| {np.abs(grad).max():.3g}; dense Newton reached {dn['gs']:.3g}")
    assert info.converged and info.grad_norm <= gtol * bmax
    assert np.abs(grad).max() <= 2 * gtol * bmax
    assert dn["gs"] <= 1e-13
    _, H, _, _ = dense_parts(dn["xs"], dn["Q"], dn["X"], dn["trials"], dn["succ"])
    lam = np.linalg.eigvalsh(H)[0]
    bound = 2 * np.sqrt(x.size) * gtol * bmax / lam
    dist = np.linalg.norm(x - dn["xs"])
    print(f"  |x - x*| {dist:.3g} bound {bound:.3g} lambda_min {lam:.3g}")
    assert lam > 0 and dist <= bound
    assert np.array_equal(post.w_hat_nodes[post.perm.cpu().numpy()], post._w.cpu().numpy())


def test_mode_raises_on_a_nonfinite_start_and_warns_without_steps(dev):
    from pynngp_amd import NNGPNumericalError

    post, _, _, _ = get_post(dev, "bern", False)
    w0 = np.zeros(post.n_nodes)
    node = int(post.perm[int(torch.nonzero(post.trials > 0)[0])])
    w0[node] = np.inf
    with pytest.raises(NNGPNumericalError, match=f"node {node}"):
        post.mode(w0=w0)
    with pytest.warns(RuntimeWarning, match="stopped after 0 steps"):
        _, _, info = post.mode(max_newton=0, beta0=np.zeros(2), w0=np.zeros(post.n_nodes))
    assert not info.converged
    post.mode(gtol=1e-8)  # leave the shared object at its mode


# ---------------------------------------------------------------- 4. the Laplace evidence
def dense_evidence(dn):
    """The Laplace evidence by dense algebra: its own Newton solve, numpy slogdet."""
    Q = dn["Q"]
    xs, _ = dense_mode(Q, dn["X"], dn["trials"], dn["succ"])
    _, _, lp, d = dense_parts(xs, Q, dn["X"], dn["trials"], dn["succ"])
    return lp + 0.5 * np.linalg.slogdet(Q)[1] - 0.5 * np.linalg.slogdet(Q + np.diag(d))[1]


@pytest.mark.parametrize("kind,with_ref", CASES[:4])
def test_laplace_evidence_against_slogdet(dev, kind, with_ref):
    from pynngp_amd import Covariance

    post, _, _, dn = get_post(dev, kind, with_ref)
    val, se = post.log_marginal(n_probes=64)
    exact = dense_evidence(dn)
    print(f"{kind} ref={with_ref}: evidence {val:.6f} +- {se:.3g}, dense {exact:.6f}")
    assert abs(val - exact) <= 4 * se
    # theta' = (32 sigma2, 8 phi): the dense values must differ by >= 10 se, and the GPU values order the same way.
    # (sigma2, 8 phi) was computed first, on the CPU: the Bernoulli set-ups' dense evidence moves by 9.3 there and no
    # further as phi grows (-185.1 -> -194.4 at 8 phi, 32 phi and 64 phi), under 10 of their standard errors of 1.8;
    # with sigma2 moved too the dense gaps are 33 (Bernoulli) and 294 (trials 5).
    try:
        post.update(Covariance("exponential", 32 * SIGMA2, 8 * PHI))
        val2, se2 = post.log_marginal(n_probes=64)
        Q2 = dense_Q(post.nbr.cpu().numpy(), post.B.cpu().numpy(), post.F.cpu().numpy(), 32 * SIGMA2)
        exact2 = dense_evidence(dict(dn, Q=Q2))
    finally:
        post.update(Covariance("exponential", SIGMA2, PHI))
        post.mode(gtol=1e-8)
    print(f"  theta': evidence {val2:.6f} +- {se2:.3g}, dense {exact2:.6f}")
    assert abs(exact - exact2) >= 10 * max(se, se2)
    assert abs(val2 - exact2) <= 4 * se2
    assert (val > val2) == (exact > exact2)


# ---------------------------------------------------------------- 5. predictions
@pytest.mark.parametrize("with_ref", [False, True])
def test_predict_against_dense_and_mpmath(dev, with_ref):
    from pynngp_amd import _lib

    post, beta, _, dn = get_post(dev, "bern", with_ref)
    c = setup_data("bern")
    rtol = 1e-11
    prob, draws = post.predict(c["q"], X_query=c["Xq"], rtol=rtol)
    assert prob.shape == (40,) and draws.shape == (0, 40)
    # the dense Gaussian approximation at the dense mode, the query points conditioned as unobserved leaves
    n_s, p = post.n_s, 2
    xs = dn["xs"]
    _, H, _, d = dense_parts(xs, dn["Q"], dn["X"], dn["trials"], dn["succ"])
    cov_w = np.linalg.inv(dn["Q"] + np.diag(d))
    q = _dt(c["q"], dev)
    s_coords = post.coords[:n_s].contiguous()
    nbr_q = _lib.knn_query(s_coords, q, min(post.m, n_s))
    B_q, F_q, _ = _lib.bf_cross(s_coords, q, nbr_q, "exponential", 1.0, PHI, 0.0)
    nbr_q, B_q, F_q = nbr_q.cpu().numpy(), B_q.cpu().numpy(), F_q.cpu().numpy()
    Bm = np.zeros((40, post.n_nodes))
    for i in range(40):
        Bm[i, nbr_q[i]] = B_q[i]
    mu = c["Xq"] @ xs[:p] + Bm @ xs[p:]
    var = SIGMA2 * F_q + np.einsum("ij,jk,ik->i", Bm, cov_w, Bm)
    exact = np.array([logistic_normal_exact(float(m), float(np.sqrt(v))) for m, v in zip(mu, var)])
    # |d prob / d mu| <= 1/4 and |d prob / d s| <= E|Z| / 4 < 0.2.  mu moves by at most |(x_q, B_q)|_2 times test 3's
    # bound b3 on |x - x*|_2, plus the re-solve of w_hat to rtol (|B_q|_2 rtol |rhs|_2 / lambda_min(A)).  The variance
    # B_q A^-1 B_q^T moves with W_hat -- |dW / d eta| <= b / (6 sqrt 3) < 0.1 b, eta_i by at most |(x_i, e_i)|_2 b3 --
    # by |A^-1 B_q^T|_2^2 max |dW|, and with the solves' rtol by rtol |B_q|_2^2 / lambda_min(A).
    lam = np.linalg.eigvalsh(H)[0]
    lam_a = np.linalg.eigvalsh(dn["Q"] + np.diag(d))[0]
    b3 = 2 * np.sqrt(xs.size) * 1e-8 / lam
    rhs_norm = np.linalg.norm(link_restatement(dn["trials"], dn["succ"], dn["X"] @ xs[:p], xs[p:], np.float64)[1])
    bq = np.sqrt((Bm ** 2).sum(axis=1))
    row = np.sqrt((c["Xq"] ** 2).sum(axis=1) + bq ** 2)
    dmu = row * b3 + bq * rtol * rhs_norm / lam_a
    dw = 0.1 * np.sqrt((dn["X"] ** 2).sum(axis=1) + 1).max() * b3
    dvar = ((Bm @ cov_w) ** 2).sum(axis=1) * dw + rtol * bq ** 2 / lam_a
    tol = 1e-8 + 0.25 * dmu + 0.2 * dvar / (2 * np.sqrt(var))
    err = np.abs(prob - exact)
    print(f"ref={with_ref}: predict max err {err.max():.3g}, tolerance {tol.min():.3g} .. {tol.max():.3g}")
    assert np.all(err <= tol)
    pd = post.probability(where="data")
    assert pd.shape == (300,) and np.all((pd > 0) & (pd < 1))
    prob2, draws2 = post.predict(c["q"][:5], n_draws=3, X_query=c["Xq"][:5], var_draws=8)
    assert prob2.shape == (5,) and draws2.shape == (3, 5) and np.all((draws2 > 0) & (draws2 < 1))


# ---------------------------------------------------------------- 6. fit
def test_fit_improves_the_evidence_and_repeats(dev):
    from pynngp_amd import BinomialLatentPosterior, Covariance

    rng = np.random.default_rng(3)
    n = 500
    coords = rng.uniform(size=(n, 2))
    field = 1.2 * np.sin(6 * coords[:, 0]) * np.cos(5 * coords[:, 1])
    succ = rng.binomial(5, 1 / (1 + np.exp(-field))).astype(np.float64)
    start = (0.5 * SIGMA2, 3 * PHI)
    out = []
    for _ in range(2):
        post = BinomialLatentPosterior(coords, succ, np.full(n, 5), Covariance("exponential", *start), m=10, device=dev)
        ll0, se0 = post.log_marginal(n_probes=32, seed=5)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            cov, res = post.fit(start, n_probes=32, seed=5, maxfev=25)
        out.append((cov.sigma2, cov.phi, -res.fun, res.se, ll0, se0))
    s2, phi, ll, se, ll0, se0 = out[0]
    print(f"fit: start {start} ll {ll0:.4f} +- {se0:.3g} -> ({s2:.4f}, {phi:.4f}) ll {ll:.4f} +- {se:.3g}")
    assert ll - ll0 > 4 * max(se, se0)
    assert out[0][:3] == out[1][:3]  # the same seed: the same theta and value, bit for bit


# ---------------------------------------------------------------- 7. draws
def test_draws_repeat_and_an_isolated_node_keeps_its_prior_variance(dev):
    from pynngp_amd import BinomialLatentPosterior, Covariance

    rng = np.random.default_rng(11)
    n = 300
    coords = rng.uniform(size=(n, 2))
    succ = rng.binomial(1, 0.5, n).astype(np.float64)
    trials = np.ones(n, dtype=np.int64)
    trials[coords[:, 0] > 0.45] = 0  # masked: the right-hand part of the square carries no observation
    post = BinomialLatentPosterior(coords, succ, trials, Covariance("exponential", SIGMA2, 3 * PHI), m=10, device=dev)
    a, b, one = post.sample(2, seed=9), post.sample(2, seed=9), post.sample(1, seed=9)
    assert a.tobytes() == b.tobytes() and np.array_equal(a[0], one[0])
    # a node with trials 0 whose parents and children are all unobserved, the farthest such from the data
    nbr = post.nbr.cpu().numpy()
    tr = post.trials.cpu().numpy()
    ok = tr == 0
    for i in range(n):
        js = nbr[i][nbr[i] >= 0]
        if tr[i] > 0 or np.any(tr[js] > 0):
            ok[i] = False
            ok[js] = ok[js] & (tr[i] == 0)
    xs = post.coords.cpu().numpy()[:, 0]
    slot = int(np.argmax(np.where(ok, xs, -1.0)))
    assert ok[slot] and xs[slot] > 0.9
    row = int(np.nonzero(post.slot_of_t.cpu().numpy() == slot)[0][0])
    draws = post.sample(4096, seed=1)[:, row]
    prior = np.linalg.inv(dense_Q(nbr, post.B.cpu().numpy(), post.F.cpu().numpy(), SIGMA2))[slot, slot]
    v = draws.var(ddof=1)
    print(f"isolated node: variance of 4096 draws {v:.4f}, prior {prior:.4f}")
    assert abs(v - prior) <= 5 * np.sqrt(2.0 / 4095) * prior
