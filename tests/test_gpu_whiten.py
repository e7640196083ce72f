"""GPU: the whitened Gram sweep (nngp_whiten_gram) and the response-model regression built on it (NNGP.gls, the
linear mean of profile_loglik / profile_loglik_grad / fit, universal kriging, the conjugate NNGP).

B, F and nbr are always the GPU sweep's own on uniform random 2-D points.  References are in numpy long double.

Bounds (eps = 2^-52):
* U: per column, |gpu - ld| / max|U| <= 4 max(|fp64 numpy - ld| / max|U|, eps) -- the K = 4 rule of DESIGN 4.7.
* G: |G_gpu - G_ld| <= gamma_n sum_t |u_a u_b| + (e_b sum|u_a| + e_a sum|u_b| + n e_a e_b), gamma_n = n eps / (1 - n eps)
  the dot-product bound for any summation order and e_c the absolute U bound of column c (the propagated term).
* GLS: beta relative to max|beta| inside 8 cond(X'QX) eps; loglik / reml inside the Gram bound carried through the
  quadratic form (c = (1, -beta): sum |c_a| |c_b| E_G[a, b]) plus gamma_n sum |log F| for the sweep's own fold, and for
  reml p cond(X'QX) times the largest relative Gram bound for log det X'QX.
* dense known answer (n = 33, m = 32): 8 cond eps.  For beta, cov_beta, the likelihoods and the conjugate posterior
  cond = cond(X'QX), the GLS section's reading; for the kriging mean and variance, which also solve with each query's
  neighbour block of C, cond = max(cond(C), cond(X'QX)).  (The product of the two, the first-order worst case of a
  perturbed factor fed to the GLS solve, would be 20 times wider here; it is printed, not asserted.)

The measured gaps are printed by each test (pytest -s) and recorded in DESIGN.md 4.8.
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LD = np.longdouble
THETA = (1.3, 6.0, 0.25)
KIND = "exponential"


def _dt(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _case(n, m, seed=0):
    """Points, the GPU's neighbour sets (natural and Z-ordered) and the GPU sweep's B and F, device and host."""
    from pynngp_amd import _lib

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1000 * seed + 7 * n + m)
    coords = rng.uniform(size=(n, 2))
    c = _dt(coords, dev)
    nbr = _lib.knn_prior(c, m)
    order, nbr_sorted = _lib.row_order(c, nbr=nbr)
    B, F, p = _lib.bf_sweep(c, nbr, 0, KIND, *THETA)
    assert p[2].item() == -1 and p[3].item() == -1
    return dict(n=n, m=m, coords=coords, c=c, nbr=nbr, order=order, nbr_sorted=nbr_sorted, B=B, F=F,
                nbr_h=nbr.cpu().numpy(), B_h=B.cpu().numpy(), F_h=F.cpu().numpy(), sum_log_f=p[0].item())


def _whiten_ref(nbr, B, F, V, self_vals, ft):
    """(self - sum_s B[t,s] V[nbr[t,s]]) / sqrt(F) in the float type ft; slots < 0 or >= len(V) add nothing."""
    ok = (nbr >= 0) & (nbr < V.shape[0])
    idx = np.where(ok, nbr, 0)
    Bm = np.where(ok, B, 0.0).astype(ft)
    acc = (Bm[:, :, None] * V.astype(ft)[idx]).sum(axis=1)
    return (self_vals.astype(ft) - acc) / np.sqrt(F.astype(ft))[:, None]


def _u_bound(U_ld, U_np):
    """Per column: the absolute bound on |gpu - ld| (K = 4 rule)."""
    scale = np.abs(U_ld).max(axis=0).astype(np.float64)
    err_np = np.abs(U_np.astype(LD) - U_ld).max(axis=0).astype(np.float64)
    return 4.0 * np.maximum(err_np, EPS * scale), scale


def _check_u(U_gpu, U_ld, U_np, what):
    bound, scale = _u_bound(U_ld, U_np)
    err = np.abs(U_gpu.astype(LD) - U_ld).max(axis=0).astype(np.float64)
    ratio = float((err / bound).max())
    print(f"  {what}: max |gpu - ld| / bound = {ratio:.3g} (|gpu - ld| / max|U| <= {float((err / scale).max()):.3g})")
    assert np.all(err <= bound), (what, err / bound)
    return bound


def _gram_bound(U_ld, e):
    n = U_ld.shape[0]
    gam = n * EPS / (1.0 - n * EPS)
    A = np.abs(U_ld).astype(np.float64)
    s1 = A.sum(axis=0)
    return gam * (A.T @ A) + np.outer(s1, e) + np.outer(e, s1) + n * np.outer(e, e)


def _check_g(G_gpu, U_ld, e, what):
    G_ld = U_ld.T @ U_ld
    bound = _gram_bound(U_ld, e)
    err = np.abs(G_gpu.astype(LD) - G_ld).astype(np.float64)
    print(f"  {what}: max |G - G_ld| / bound = {float((err / bound).max()):.3g}")
    assert np.all(err <= bound), (what, (err / bound).max())
    return bound


def _columns(n, k, seed):
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((n, k))
    V[:, 0] += 3.0
    if k > 1:
        V[:, 1] = 1.0  # an intercept column
    return V


# ---------------------------------------------------------------- whitening and Gram accuracy
@pytest.mark.parametrize("m", [1, 5, 15, 32])
def test_whiten_and_gram_accuracy(dev, m):
    from pynngp_amd import _lib

    cs = _case(700, m)
    for k in (1, 3, 16):
        V = _columns(700, k, 11 * m + k)
        U_ld = _whiten_ref(cs["nbr_h"], cs["B_h"], cs["F_h"], V, V, LD)
        U_np = _whiten_ref(cs["nbr_h"], cs["B_h"], cs["F_h"], V, V, np.float64)
        V_d = _dt(V, dev)
        U, G = _lib.whiten_gram(cs["nbr"], cs["B"], cs["F"], V_d)
        e = _check_u(U.cpu().numpy(), U_ld, U_np, f"m={m} ncol={k}")
        _check_g(G.cpu().numpy(), U_ld, e, f"m={m} ncol={k}")
        Uo, Go = _lib.whiten_gram(cs["nbr_sorted"], cs["B"], cs["F"], V_d, order=cs["order"])
        assert torch.equal(U, Uo) and torch.equal(G, Go)  # the visiting order changes nothing: natural rows, same fold
        assert torch.equal(G, G.t())


# ---------------------------------------------------------------- bit identity
@pytest.mark.parametrize("k", [3, 8, 16])
def test_bit_identity_of_columns_and_pairs(dev, k):
    from pynngp_amd import _lib

    cs = _case(2500, 7)
    V = _columns(2500, k, k)
    V_d = _dt(V, dev)
    args = (cs["nbr_sorted"], cs["B"], cs["F"])
    U, G = _lib.whiten_gram(*args, V_d, order=cs["order"])
    U2, G2 = _lib.whiten_gram(*args, V_d, order=cs["order"])
    assert torch.equal(U, U2) and torch.equal(G, G2)  # run to run
    U3, none = _lib.whiten_gram(*args, V_d, order=cs["order"], want_gram=False)
    assert none is None and torch.equal(U, U3)  # with or without gram
    for c in range(k):
        u1, g1 = _lib.whiten_gram(*args, V_d[:, c:c + 1].contiguous(), order=cs["order"])
        assert torch.equal(u1[:, 0], U[:, c]) and g1[0, 0].item() == G[c, c].item()
    pairs = [(a, b) for a in range(k) for b in range(a + 1, k)]
    for a, b in pairs:
        _, g2 = _lib.whiten_gram(*args, V_d[:, [a, b]].contiguous(), order=cs["order"])
        assert torch.equal(g2, G[[a, b]][:, [a, b]]), (a, b)
    # a NaN planted in one column stays in that column of U and in its row and column of G
    c = k // 2
    Vn = V.copy()
    Vn[1234, c] = np.nan
    Un, Gn = _lib.whiten_gram(*args, _dt(Vn, dev), order=cs["order"])
    keep = [j for j in range(k) if j != c]
    assert torch.equal(Un[:, keep], U[:, keep]) and torch.isnan(Un[:, c]).any()
    assert torch.isnan(Gn[c]).all() and torch.isnan(Gn[:, c]).all()
    assert torch.equal(Gn[keep][:, keep], G[keep][:, keep])


def test_torch_op_agrees(dev):
    from pynngp_amd import _lib, load_ops

    load_ops()
    cs = _case(700, 5)
    V_d = _dt(_columns(700, 4, 1), dev)
    U, G = _lib.whiten_gram(cs["nbr_sorted"], cs["B"], cs["F"], V_d, order=cs["order"])
    Uo, Go = torch.ops.nngp.whiten_gram(cs["nbr_sorted"], cs["order"], cs["B"], cs["F"], 0, V_d, None, True)
    assert torch.equal(U, Uo) and torch.equal(G, Go)
    Uo, Go = torch.ops.nngp.whiten_gram(cs["nbr"], None, cs["B"], cs["F"], 0, V_d, None, False)
    assert torch.equal(U, Uo) and Go.numel() == 0


# ---------------------------------------------------------------- shapes
# whitening tiles hold 256 / KP rows (16 .. 256), the Gram stages 256 rows at a time and records 1,024 per tile
@pytest.mark.parametrize("n,m", [(1, 1), (2, 1), (6, 5), (16, 3), (17, 3), (255, 4), (256, 4), (257, 4), (1023, 6),
                                 (1024, 6), (1025, 6), (4097, 3)])
def test_shapes_across_tile_boundaries(dev, n, m):
    from pynngp_amd import _lib

    cs = _case(n, m, seed=1)
    assert np.all(cs["nbr_h"][: min(n, m)][np.triu_indices(min(n, m), 0, m)] == -1)  # the first rows are -1 padded
    for k in (1, 2, 5, 16):
        V = _columns(n, k, n + k)
        U_ld = _whiten_ref(cs["nbr_h"], cs["B_h"], cs["F_h"], V, V, LD)
        U_np = _whiten_ref(cs["nbr_h"], cs["B_h"], cs["F_h"], V, V, np.float64)
        U, G = _lib.whiten_gram(cs["nbr_sorted"], cs["B"], cs["F"], _dt(V, dev), order=cs["order"])
        e = _check_u(U.cpu().numpy(), U_ld, U_np, f"n={n} ncol={k}")
        _check_g(G.cpu().numpy(), U_ld, e, f"n={n} ncol={k}")


def test_zero_rows_zeroes_gram_and_bad_rows_give_nan(dev):
    from pynngp_amd import _lib

    cs = _case(300, 4)
    V_d = _dt(_columns(300, 3, 5), dev)
    empty_i = torch.empty((0, 4), dtype=torch.int32, device=dev)
    empty_f = torch.empty((0, 4), dtype=torch.float64, device=dev)
    U, G = _lib.whiten_gram(empty_i, empty_f, empty_f[:, 0].contiguous(), V_d,
                            Vq=torch.empty((0, 3), dtype=torch.float64, device=dev))
    assert U.shape == (0, 3) and torch.equal(G, torch.zeros_like(G))
    # F that is 0, negative or NaN gives NaN rows; a slot out of range adds exactly 0 even under a NaN coefficient
    F = cs["F"].clone()
    F[10], F[20], F[30] = 0.0, -1.0, float("nan")
    nbr, B = cs["nbr"].clone(), cs["B"].clone()
    nbr[100, 1], B[100, 1] = 300, float("nan")
    nbr[101, 0], B[101, 0] = -7, float("inf")
    U, G = _lib.whiten_gram(nbr, B, F, V_d)
    U0, _ = _lib.whiten_gram(cs["nbr"], cs["B"], cs["F"], V_d)
    bad = torch.isnan(U).all(dim=1).nonzero().flatten().tolist()
    assert bad == [10, 20, 30] and torch.isnan(G).all()
    B0 = cs["B"].clone()
    B0[100, 1] = B0[101, 0] = 0.0  # the reference: those two slots dropped
    nb0 = cs["nbr"].clone()
    nb0[100, 1] = nb0[101, 0] = -1
    U1, _ = _lib.whiten_gram(nb0, B0, cs["F"], V_d)
    assert torch.equal(U[100:102], U1[100:102]) and torch.isfinite(U[100:102]).all()
    rest = [i for i in range(300) if i not in (10, 20, 30, 100, 101)]
    assert torch.equal(U[rest], U0[rest])


@pytest.mark.parametrize("n_q", [5, 300])
def test_cross_mode(dev, n_q):
    from pynngp_amd import _lib

    cs = _case(500, 6)
    rng = np.random.default_rng(n_q)
    q = rng.uniform(size=(n_q, 2))
    q_d = _dt(q, dev)
    nbr = _lib.knn_query(cs["c"], q_d, 6)
    Bq, Fq, _ = _lib.bf_cross(cs["c"], q_d, nbr, KIND, *THETA)
    V, Vq = _columns(500, 4, 3), _columns(n_q, 4, 4)
    U, G = _lib.whiten_gram(nbr, Bq, Fq, _dt(V, dev), Vq=_dt(Vq, dev))
    ref = [_whiten_ref(nbr.cpu().numpy(), Bq.cpu().numpy(), Fq.cpu().numpy(), V, Vq, ft) for ft in (LD, np.float64)]
    e = _check_u(U.cpu().numpy(), ref[0], ref[1], f"cross n_q={n_q}")
    _check_g(G.cpu().numpy(), ref[0], e, f"cross n_q={n_q}")
    order = _dt(rng.permutation(n_q).astype(np.int32), dev)
    Uo, Go = _lib.whiten_gram(nbr[order.long()].contiguous(), Bq, Fq, _dt(V, dev), Vq=_dt(Vq, dev), order=order)
    assert torch.equal(U, Uo) and torch.equal(G, Go)


# ---------------------------------------------------------------- long double linear algebra (numpy's is fp64 only)
def _ld_chol(A):
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _ld_lower_solve(L, b):
    b = np.array(b, dtype=LD)
    x = np.zeros_like(b)
    for i in range(L.shape[0]):
        x[i] = (b[i] - L[i, :i] @ x[:i]) / L[i, i]
    return x


def _ld_spd_solve(A, b):
    L = _ld_chol(A)
    return _ld_lower_solve(L.T[::-1, ::-1], _ld_lower_solve(L, b)[::-1])[::-1]


def _ld_gls(G, sum_log_f, n):
    """beta, cov_beta, loglik, reml from a long double Gram matrix of [y, X]."""
    p = G.shape[0] - 1
    XX, Xy = G[1:, 1:], G[1:, 0]
    beta = _ld_spd_solve(XX, Xy)
    quad = G[0, 0] - beta @ Xy
    logdet = 2 * np.sum(np.log(np.diag(_ld_chol(XX))))
    l2pi = np.log(LD(2) * np.arctan(LD(1)) * 4)
    ll = -(n * l2pi + sum_log_f + quad) / 2
    reml = -((n - p) * l2pi + sum_log_f + quad + logdet) / 2
    return beta, _ld_spd_solve(XX, np.eye(p, dtype=LD)), ll, reml, quad, logdet


def _nngp_precision_ld(nbr, B, F):
    n = nbr.shape[0]
    ImB = np.eye(n, dtype=LD)
    for i in range(n):
        for s in range(nbr.shape[1]):
            if nbr[i, s] >= 0:
                ImB[i, nbr[i, s]] -= LD(B[i, s])
    return ImB.T @ (ImB / F.astype(LD)[:, None])


def _model(n, m, seed, p, beta=(2.0, -1.0, 0.5, 0.25)):
    """An NNGP instance on uniform points with y = X beta + a smooth field + noise; X = [1, x, y, xy][:p]."""
    from pynngp_amd import NNGP, Covariance

    rng = np.random.default_rng(seed)
    coords = rng.uniform(size=(n, 2))
    X = np.column_stack([np.ones(n), coords[:, 0], coords[:, 1], coords[:, 0] * coords[:, 1]])[:, :p]
    w = np.sin(5 * coords[:, 0]) * np.cos(4 * coords[:, 1])
    y = X @ np.array(beta[:p]) + w + 0.3 * rng.standard_normal(n)
    return NNGP(coords, y, None, "S=T", m, Covariance(KIND, *THETA)), coords, X, y


# ---------------------------------------------------------------- GLS against the dense GLS
@pytest.mark.parametrize("p", [1, 4])
def test_gls_against_dense_longdouble(dev, p):
    from pynngp_amd import Covariance

    n, m = 400, 10
    model, coords, X, y = _model(n, m, 5, p)
    cov = Covariance(KIND, *THETA)
    res = model.gls(cov, X)
    B, F = (t.cpu().numpy() for t in model.compute_BF())
    nbr = model.nbr.cpu().numpy()
    Q = _nngp_precision_ld(nbr, B, F)
    V = np.column_stack([y, X]).astype(LD)
    G_ld = V.T @ Q @ V
    slf_ld = np.sum(np.log(F.astype(LD)))
    beta, covb, ll, reml, quad, logdet = _ld_gls(G_ld, slf_ld, n)
    cond = float(np.linalg.cond(G_ld[1:, 1:].astype(np.float64)))
    # the Gram bound from the long double whitened columns
    Vf = np.column_stack([y, X])
    U_ld = _whiten_ref(nbr, B, F, Vf, Vf, LD)
    e, _ = _u_bound(U_ld, _whiten_ref(nbr, B, F, Vf, Vf, np.float64))
    EG = _gram_bound(U_ld, e)
    g_gap = np.abs(res.gram.astype(LD) - G_ld).astype(np.float64)
    assert np.all(g_gap <= EG), (g_gap / EG).max()
    rel_beta = float(np.max(np.abs(res.beta.astype(LD) - beta)) / np.max(np.abs(beta)))
    cvec = np.abs(np.concatenate([[1.0], -beta.astype(np.float64)]))
    gam = n * EPS / (1 - n * EPS)
    tol_ll = 0.5 * (cvec @ EG @ cvec + gam * float(np.sum(np.abs(np.log(F))))) + 4 * EPS * abs(float(ll))
    relG = float((EG[1:, 1:] / np.abs(G_ld[1:, 1:]).astype(np.float64)).max())
    tol_reml = tol_ll + 0.5 * p * cond * relG + 4 * EPS * abs(float(reml))
    print(f"  p={p}: cond(X'QX) = {cond:.3g}; |beta - ld| / max|beta| = {rel_beta:.3g} = "
          f"{rel_beta / (cond * EPS):.3g} cond eps; |loglik - ld| = {abs(float(res.loglik - ll)):.3g} (bound "
          f"{tol_ll:.3g}); |reml - ld| = {abs(float(res.reml - reml)):.3g} (bound {tol_reml:.3g}); max Gram gap / "
          f"bound {(g_gap / EG).max():.3g}")
    assert rel_beta <= 8 * cond * EPS
    assert abs(float(res.loglik - ll)) <= tol_ll and abs(float(res.reml - reml)) <= tol_reml
    assert float(np.max(np.abs(res.cov_beta.astype(LD) - covb)) / np.max(np.abs(covb))) <= 8 * cond * max(EPS, relG)
    if p == 1:  # X = 1 is the constant mean: the two-sweep path's mu and ll, in another fold order
        ll_c, mu_c = model.profile_loglik(cov, mean="constant")
        ll_l, beta_l = model.profile_loglik(cov, mean="linear", X=X)
        assert ll_l == res.loglik and beta_l[0] == res.beta[0]
        relXy = float(EG[0, 1] / abs(float(G_ld[0, 1])))
        print(f"  constant mean: |mu - beta| / |mu| = {abs(mu_c - res.beta[0]) / abs(mu_c):.3g}, |ll - ll| = "
              f"{abs(ll_c - res.loglik):.3g}")
        assert abs(mu_c - res.beta[0]) <= 2 * (relXy + relG) * abs(mu_c)
        assert abs(ll_c - res.loglik) <= 2 * tol_ll


# ---------------------------------------------------------------- known answer: n = 33, m = 32 is the dense GP
def _dense_cov_ld(a, b, theta, nugget):
    d = np.sqrt(((a.astype(LD)[:, None, :] - b.astype(LD)[None, :, :]) ** 2).sum(-1))
    C = LD(theta[0]) * np.exp(-LD(theta[1]) * d)
    return C + LD(theta[2]) * np.eye(len(a), dtype=LD) if nugget else C


def test_known_answer_dense_gp(dev):
    from pynngp_amd import Covariance
    from pynngp_amd import regression as R

    n, m, p = 33, 32, 3
    model, coords, X, y = _model(n, m, 8, p)
    phi, alpha = 6.0, 0.2
    th = (1.0, phi, alpha)
    C = _dense_cov_ld(coords, coords, th, True)
    L = _ld_chol(C)
    W = np.column_stack([_ld_lower_solve(L, col) for col in np.column_stack([y, X]).T])
    G_ld = W.T @ W
    slf = 2 * np.sum(np.log(np.diag(L)))
    beta, covb, ll, reml, quad, logdet = _ld_gls(G_ld, slf, n)
    cond_c, cond = float(np.linalg.cond(C.astype(np.float64))), float(np.linalg.cond(G_ld[1:, 1:].astype(np.float64)))
    tol = 8 * cond * EPS
    res = model.gls(Covariance(KIND, *th), X)
    prior = dict(a=2.5, b=1.5)
    cj = model.conjugate(KIND, phi, alpha, X, prior=prior)
    a1 = LD(prior["a"]) + LD(n - p) / 2
    b1 = LD(prior["b"]) + quad / 2
    l2pi = np.log(LD(8) * np.arctan(LD(1)))
    ev = (-(n - p) * l2pi / 2 - slf / 2 - logdet / 2 + prior["a"] * np.log(LD(prior["b"])) - a1 * np.log(b1)
          + LD(math.lgamma(float(a1))) - LD(math.lgamma(prior["a"])))
    rel = lambda got, want: float(np.max(np.abs(np.asarray(got).astype(LD) - want)) / np.max(np.abs(want)))  # noqa: E731
    gaps = {"beta": rel(res.beta, beta), "cov_beta": rel(res.cov_beta, covb), "loglik": rel(res.loglik, ll),
            "reml": rel(res.reml, reml), "mu*": rel(cj.mu, beta), "V*": rel(cj.V, covb), "a*": rel(cj.a, a1),
            "b*": rel(cj.b, b1), "evidence": rel(cj.log_evidence, ev)}
    print(f"  cond(X'QX) = {cond:.3g}, cond(C) = {cond_c:.3g}, bound 8 cond(X'QX) eps = {tol:.3g} (with the product: "
          f"{tol * cond_c:.3g}); gaps: " + ", ".join(f"{k} {v:.3g}" for k, v in gaps.items()))
    for k, v in gaps.items():
        assert v <= tol, (k, v, tol)
    # a proper prior: the host algebra on this Gram matrix equals the dense multivariate-t evidence
    m0, V0 = np.array([1.0, 0.0, 0.5]), np.diag([9.0, 4.0, 4.0])
    cp = R.nig_from_gram(cj.gram, slf.astype(np.float64), n, dict(mu=m0, V=V0, **prior))
    S = C + X.astype(LD) @ V0.astype(LD) @ X.astype(LD).T
    Ls = _ld_chol(S)
    z = _ld_lower_solve(Ls, (y - X @ m0).astype(LD))
    maha = z @ z
    ev_p = (LD(math.lgamma(prior["a"] + n / 2)) - LD(math.lgamma(prior["a"])) - n * (l2pi + np.log(LD(prior["b"]))) / 2
            - np.sum(np.log(np.diag(Ls))) - (prior["a"] + LD(n) / 2) * np.log1p(maha / (2 * prior["b"])))
    print(f"  proper prior: evidence gap {rel(cp.log_evidence, ev_p):.3g}, b* gap {rel(cp.b, prior['b'] + maha / 2):.3g}")
    assert rel(cp.log_evidence, ev_p) <= tol and rel(cp.b, prior["b"] + maha / 2) <= tol

    # universal kriging and the conjugate predictive at 5 points: each query conditions on its 32 nearest points
    rng = np.random.default_rng(3)
    q = rng.uniform(size=(5, 2))
    Xq = np.column_stack([np.ones(5), q[:, 0], q[:, 1]])
    from pynngp_amd import _lib

    nbr = _lib.knn_query(model._s_dev, _dt(q, dev), m).cpu().numpy()
    mean, var = model.predict(cov=Covariance(KIND, *th), query=q, X=X, X_query=Xq)
    loc, scale, df = cj.predict(q, Xq)
    want_mean, want_var = np.zeros(5, dtype=LD), np.zeros(5, dtype=LD)
    for i in range(5):
        N = nbr[i]
        cN = _dense_cov_ld(coords[N], coords[N], th, True)
        cq = _dense_cov_ld(q[i:i + 1], coords[N], th, False)[0]
        b = _ld_spd_solve(cN, cq)
        h = Xq[i].astype(LD) - b @ X[N].astype(LD)
        want_mean[i] = Xq[i].astype(LD) @ beta + b @ (y[N].astype(LD) - X[N].astype(LD) @ beta)
        want_var[i] = (LD(th[0]) + LD(th[2]) - b @ cq) + h @ covb @ h
    want_scale = np.sqrt(b1 / a1 * want_var)
    kg = {"mean": rel(mean, want_mean), "var": rel(var, want_var), "t location": rel(loc, want_mean),
          "t scale": rel(scale, want_scale)}
    tol_k = 8 * max(cond, cond_c) * EPS
    print(f"  kriging gaps (bound {tol_k:.3g}): " + ", ".join(f"{k} {v:.3g}" for k, v in kg.items()))
    for k, v in kg.items():
        assert v <= tol_k, (k, v, tol_k)
    assert df == 2 * float(a1)


# ---------------------------------------------------------------- gradient and fit
def test_linear_mean_gradient_against_central_differences(dev):
    """Step and tolerance of tests/test_gpu_grad.py::test_loglik_grad_methods (the constant mean): h = 1e-6 theta,
    |fd - g| <= 1e-5 max(1, |g|)."""
    from pynngp_amd import Covariance

    model, coords, X, y = _model(300, 10, 9, 3)
    th = (1.0, 8.0, 0.1)
    ll, beta, g = model.profile_loglik_grad(Covariance(KIND, *th), mean="linear", X=X)
    ll0, beta0 = model.profile_loglik(Covariance(KIND, *th), mean="linear", X=X)
    assert ll == ll0 and np.array_equal(beta, beta0)
    for mean in ("constant", "zero"):  # X belongs to the linear mean alone
        with pytest.raises(ValueError):
            model.profile_loglik_grad(Covariance(KIND, *th), mean=mean, X=X)
        with pytest.raises(ValueError):
            model.profile_loglik(Covariance(KIND, *th), mean=mean, X=X)
    for k in range(3):
        h = 1e-6 * th[k]
        tp, tm = list(th), list(th)
        tp[k] += h
        tm[k] -= h
        fd = (model.profile_loglik(Covariance(KIND, *tp), mean="linear", X=X)[0]
              - model.profile_loglik(Covariance(KIND, *tm), mean="linear", X=X)[0]) / (2 * h)
        print(f"  d/dtheta[{k}]: analytic {g[k]:.9g}, central difference {fd:.9g}")
        assert abs(fd - g[k]) <= 1e-5 * max(1.0, abs(g[k])), (k, fd, g[k])


def test_fit_linear_recovers_planted_beta(dev):
    from pynngp_amd import NNGP, Covariance

    n, m = 2000, 10
    rng = np.random.default_rng(21)
    coords = rng.uniform(size=(n, 2))
    d = np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(-1))
    w = np.linalg.cholesky(1.0 * np.exp(-8.0 * d) + 1e-10 * np.eye(n)) @ rng.standard_normal(n)
    X = np.column_stack([np.ones(n), coords[:, 0]])
    beta = np.array([1.5, -2.0])
    y = X @ beta + w + math.sqrt(0.1) * rng.standard_normal(n)
    model = NNGP(coords, y, None, "S=T", m, Covariance(KIND, 0.5, 4.0, 0.2))
    fit = model.fit(mean="linear", X=X, gradient=True)
    se = np.sqrt(np.diag(fit["cov_beta"]))
    print(f"  theta {fit['theta']}, beta {fit['beta']}, se {se}, (beta - planted) / se {(fit['beta'] - beta) / se}, "
          f"{fit['n_evals']} evaluations")
    assert fit["converged"] and fit["mu"] is None
    assert np.all(np.abs(fit["beta"] - beta) <= 4 * se)
    g = model.gls(model.cov, X)
    assert np.array_equal(g.beta, fit["beta"]) and abs(g.loglik - fit["loglik"]) <= 1e-9 * abs(g.loglik)
    # the restricted likelihood, derivative-free, from the estimate: no lower than where it started
    from pynngp_amd import regression

    r0 = regression.gls(model, model.cov, X)
    assert r0.objective == r0.loglik == g.objective and regression.gls(model, model.cov, X, reml=True).objective == r0.reml
    start = model.gls(model.cov, X, reml=True).objective
    rf = model.fit(mean="linear", X=X, reml=True, maxiter=60)
    assert rf["loglik"] >= start and rf["beta"].shape == (2,)
    with pytest.raises(NotImplementedError):
        model.fit(mean="linear", X=X, reml=True, gradient=True)
    with pytest.raises(ValueError):
        model.fit(mean="linear")


# ---------------------------------------------------------------- kriging from the downloaded factors, the grid
def test_universal_kriging_and_conjugate_from_downloaded_factors(dev):
    from pynngp_amd import Covariance, NNGPNumericalError, _lib

    n, m, p = 500, 10, 3
    model, coords, X, y = _model(n, m, 12, p)
    cov = Covariance(KIND, *THETA)
    rng = np.random.default_rng(4)
    q = rng.uniform(size=(40, 2))
    Xq = np.column_stack([np.ones(40), q[:, 0], q[:, 1]])
    res = model.gls(cov, X)
    mean, var = model.predict(cov=cov, query=q, X=X, X_query=Xq)
    q_d = _dt(q, dev)
    nbr = _lib.knn_query(model._s_dev, q_d, m)
    Bq, Fq, _ = _lib.bf_cross(model._s_dev, q_d, nbr, KIND, *THETA)
    nbr, Bq, Fq = nbr.cpu().numpy(), Bq.cpu().numpy(), Fq.cpu().numpy()

    def formulas(ft, mu, Vb, scale2):
        mu, Vb = mu.astype(ft), Vb.astype(ft)
        r = y.astype(ft) - X.astype(ft) @ mu
        kr = (Bq.astype(ft) * r[nbr]).sum(axis=1)
        h = Xq.astype(ft) - (Bq.astype(ft)[:, :, None] * X.astype(ft)[nbr]).sum(axis=1)
        return Xq.astype(ft) @ mu + kr, ft(scale2) * (Fq.astype(ft) + ((h @ Vb) * h).sum(axis=1))

    def check(got, ld, f64, what):
        scale = float(np.abs(ld).max())
        bound = 4 * max(float(np.abs(f64.astype(LD) - ld).max()), EPS * scale)
        err = float(np.abs(got.astype(LD) - ld).max())
        print(f"  {what}: |gpu - ld| / bound = {err / bound:.3g}")
        assert err <= bound, (what, err, bound)

    (m_ld, v_ld), (m_np, v_np) = (formulas(ft, res.beta, res.cov_beta, 1.0) for ft in (LD, np.float64))
    check(mean, m_ld, m_np, "kriging mean")
    check(var, v_ld, v_np, "kriging variance")
    assert np.all(var >= Fq)  # the beta term only adds
    # the conjugate predictive at (phi, alpha): the same assembly with (mu*, V*) and the scale b* / a*
    cj = model.conjugate(KIND, 6.0, 0.2, X)
    Bq, Fq, _ = (t.cpu().numpy() for t in _lib.bf_cross(model._s_dev, q_d, _dt(nbr, dev), KIND, 1.0, 6.0, 0.2))
    loc, scale, df = cj.predict(q, Xq)
    (m_ld, v_ld), (m_np, v_np) = (formulas(ft, cj.mu, cj.V, cj.b / cj.a) for ft in (LD, np.float64))
    check(loc, m_ld, m_np, "t location")
    check(scale ** 2, v_ld, v_np, "t scale^2")
    assert df == 2 * cj.a and cj.a == 2.0 + (n - p) / 2
    # the grid returns the argmax of its own surface
    phis, alphas = [3.0, 6.0, 12.0], [0.05, 0.2, 0.8]
    grid = model.conjugate_grid(phis, alphas, KIND, X)
    surf = grid["log_evidence"]
    i, j = np.unravel_index(np.argmax(surf), surf.shape)
    assert surf.shape == (3, 3) and np.all(np.isfinite(surf))
    assert (grid["phi"], grid["alpha"]) == (phis[i], alphas[j]) and grid["best"].log_evidence == surf[i, j]
    assert surf[1, 1] == cj.log_evidence
    # refusals of the Python layer
    with pytest.raises(NNGPNumericalError):
        model.gls(cov, np.column_stack([X, X[:, 1] + X[:, 2]]))
    with pytest.raises(ValueError):
        model.gls(cov, np.ones((n, 16)))
    with pytest.raises(ValueError):
        model.predict(cov=cov, query=q, X=X)
