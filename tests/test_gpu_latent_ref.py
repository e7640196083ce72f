"""GPU: the latent posterior on a reference set (S != T) with the leaves integrated out -- the nngp_precision_ref_*
operator family, nngp_latent_ref_cg_batch, nngp_latent_ref_leaves_batch, LatentPosterior(ref=...), its predict and
NNGP.latent_posterior -- against dense algebra on the oracle's node DAG (oracle/nngp_gibbs_oracle.py::reference_dag,
dag_posterior; the formulas restated in tests/test_latent_ref_host.py::dense_ref_system).

Rounding bounds.  With L = [(I - B_S); -B_L] and s the row scale, (A_S x)_i = sum_r L_ri s_r (L_r. x) + d_i x_i.  The
inner dot has at most m + 1 terms, the outer one deg_i + 1, s_r carries two more roundings on a leaf row (g = f d /
(f + d)) and sigma2 one: |err|_i <= 4 (m + deg_i + 6) u (sum_r |L_ri| s_r |L_r.| |x|)_i + 4 u d_i |x_i|, u = 2^-52
(the factor 4 covers the (1 + u)^k - 1 <= 1.01 k u expansion and the products' own roundings, as in
tests/test_gpu_latent.py)."""
import functools
import warnings

import numpy as np
import pytest
import torch

from oracle import nngp_gibbs_oracle as G
from oracle import nngp_oracle as O
from test_latent_ref_host import dense_ref_system

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
SIGMA2, PHI, TAU2 = 1.3, 6.0, 0.25
# (n_s, n_out, m, dim): the three lane groups and a ragged last tile; (6, 700, 5): every reverse list above 512
# entries (the whole-block path, several long lists in one tile); n_s < m (-1 padded leaf rows); one node; no leaves
SHAPES = [(60, 200, 3, 2), (60, 200, 7, 2), (120, 300, 15, 2), (40, 90, 32, 2), (6, 700, 5, 2), (3, 50, 5, 2),
          (1, 20, 1, 2), (50, 0, 7, 2), (60, 200, 7, 1), (60, 200, 7, 3)]
IDS = ["-".join(map(str, s)) for s in SHAPES]


def _dt(a, dev):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)


@functools.lru_cache(maxsize=None)
def _case(n_s, n_out, m, dim):
    """Node DAG, oracle B / F, d with ~30 % zeros on reference nodes and on leaves, and the dense system
    (shared, read-only)."""
    rng = np.random.default_rng(1000 * n_s + 10 * n_out + m + dim)
    s, t_out = rng.uniform(size=(n_s, dim)), rng.uniform(size=(n_out, dim))
    if (n_s, m) == (6, 5):
        # a regular hexagon about the centre: a leaf leaves out only its farthest reference point, about a sixth of
        # the leaves each, so every reference node keeps a reverse list above 512 entries
        ang = 2.0 * np.pi * (np.arange(6) + 0.25) / 6.0
        s = 0.5 + 0.3 * np.column_stack([np.cos(ang), np.sin(ang)])
    coords, nbr = G.reference_dag(s, t_out, m)
    n = n_s + n_out
    B, F, _ = O.bf_sweep(coords, nbr, "exponential", (1.0, PHI, 0.0))
    eps = rng.uniform(0.5, 2.0, n)
    h = np.where(rng.uniform(size=n) < 0.3, 0.0, 1.0 / eps ** 2)
    h[0] = 1.0 / eps[0] ** 2
    d = h / TAU2
    v = rng.standard_normal(n)
    A, b, diag, L, sc = dense_ref_system(nbr, B, F, n_s, SIGMA2, d, v)
    deg = np.bincount(nbr[nbr >= 0], minlength=n)[:n_s]
    out = dict(n_s=n_s, n=n, m=m, coords=coords, s=s, t_out=t_out, nbr=nbr, B=B, F=F, h=h, eps=eps, d=d, v=v, A=A,
               b=b, diag=diag, L=L, sc=sc, deg=deg)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _geom(dev, c):
    from pynngp_amd import _lib

    nbr_d, B_d, F_d = _dt(c["nbr"].astype(np.int32), dev), _dt(c["B"], dev), _dt(c["F"], dev)
    off, rev_j, rev_k = _lib.reverse_neighbors(nbr_d)
    prep = _lib.gibbs_prepare(B_d, F_d, off, rev_j, rev_k)
    return nbr_d, B_d, off, rev_j, rev_k, prep, c["n_s"]


def _op_bound(c, X, with_d=True):
    """The docstring's bound for L^T diag(s) L X (+ d X)."""
    aL = np.abs(c["L"])
    bound = 4.0 * (c["m"] + c["deg"] + 6)[:, None] * U * (aL.T @ (c["sc"][:, None] * (aL @ np.abs(X))))
    if with_d:
        bound = bound + 4.0 * U * c["d"][:c["n_s"], None] * np.abs(X)
    return bound


# ---------------------------------------------------------------- operator, fold, diag, sqrt^T against dense
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_operator_fold_diag_sqrt_match_dense(dev, shape):
    from pynngp_amd import _lib

    c = _case(*shape)
    n, n_s, m = c["n"], c["n_s"], c["m"]
    geom = _geom(dev, c)
    d_d = _dt(c["d"], dev)
    rng = np.random.default_rng(7)
    X = rng.standard_normal((n_s, 3))
    out = _lib.precision_ref_apply_batch(*geom, SIGMA2, _dt(X, dev), d=d_d).cpu().numpy()
    err, bound = np.abs(out - c["A"] @ X), _op_bound(c, X)
    print(f"apply max err/bound {(err / np.maximum(bound, 1e-300)).max():.3g}")
    assert np.all(err <= bound)
    # d NULL: the prior precision of S alone (every g is 0)
    out0 = _lib.precision_ref_apply_batch(*geom, SIGMA2, _dt(X, dev)).cpu().numpy()
    LS = c["L"][:n_s]
    fS = 1.0 / (SIGMA2 * c["F"][:n_s])
    exact0 = LS.T @ (fS[:, None] * (LS @ X))
    c0 = dict(c, L=np.concatenate([LS, np.zeros((n - n_s, n_s))]), sc=np.concatenate([fS, np.zeros(n - n_s)]))
    assert np.all(np.abs(out0 - exact0) <= _op_bound(c0, X, with_d=False))

    # fold: d_S v_S + B_L^T (g v_L); the column c["v"] gives b_S
    V = np.concatenate([c["v"][:, None], rng.standard_normal((n, 2))], axis=1)
    got = _lib.precision_ref_fold_batch(*geom, SIGMA2, _dt(V, dev), d=d_d).cpu().numpy()
    LL = c["L"].copy()
    LL[:n_s] = 0.0
    exact = -LL.T @ (c["sc"][:, None] * V) + c["d"][:n_s, None] * V[:n_s]
    bound = 4.0 * (c["deg"] + 6)[:, None] * U * (np.abs(LL).T @ (c["sc"][:, None] * np.abs(V))) \
        + 4.0 * U * c["d"][:n_s, None] * np.abs(V[:n_s])
    assert np.all(np.abs(got - exact) <= bound)
    assert np.all(np.abs(got[:, 0] - c["b"]) <= bound[:, 0] + 4 * U * np.abs(c["b"]))

    # diag
    got = _lib.precision_ref_diag(*geom, SIGMA2, d=d_d).cpu().numpy()
    assert np.all(np.abs(got - c["diag"]) <= 4.0 * (c["deg"] + 6) * U * c["diag"])

    # sqrt^T on given normals: (I - B_S)^T f_S^1/2 z1_S + B_L^T g^1/2 z1_L + d_S^1/2 z2
    Z1, Z2 = rng.standard_normal((n, 3)), rng.standard_normal((n_s, 3))
    got = _lib.precision_ref_sqrt_t_apply_batch(*geom, SIGMA2, _dt(Z1, dev), _dt(Z2, dev), d=d_d).cpu().numpy()
    sign = np.concatenate([np.ones(n_s), -np.ones(n - n_s)])  # L's leaf rows are -B_L
    rs = np.sqrt(c["sc"])
    exact = c["L"].T @ ((sign * rs)[:, None] * Z1) + np.sqrt(c["d"][:n_s])[:, None] * Z2
    bound = 4.0 * (c["deg"] + 8)[:, None] * U * (np.abs(c["L"]).T @ (rs[:, None] * np.abs(Z1))) \
        + 4.0 * U * np.sqrt(c["d"][:n_s])[:, None] * np.abs(Z2)
    assert np.all(np.abs(got - exact) <= bound)


def test_long_reverse_lists_are_exercised():
    c = _case(6, 700, 5, 2)
    assert np.all(c["deg"] > 512)


# ---------------------------------------------------------------- n_s = n: the existing calls, bit for bit
@pytest.mark.parametrize("n,m", [(300, 7), (257, 15)])
def test_ns_equal_n_is_the_batch_call_bit_for_bit(dev, n, m):
    from pynngp_amd import _lib

    c = _case(n, 0, m, 2)
    geom = _geom(dev, c)
    old = geom[:6]
    d_d = _dt(c["d"], dev)
    rng = np.random.default_rng(3)
    for nrhs in (1, 3, 8):
        X, Z2 = _dt(rng.standard_normal((n, nrhs)), dev), _dt(rng.standard_normal((n, nrhs)), dev)
        for d in (None, d_d):
            np.testing.assert_array_equal(_lib.precision_ref_apply_batch(*geom, SIGMA2, X, d=d).cpu().numpy(),
                                          _lib.precision_apply_batch(*old, SIGMA2, X, d=d).cpu().numpy())
            z2 = None if d is None else Z2
            np.testing.assert_array_equal(
                _lib.precision_ref_sqrt_t_apply_batch(*geom, SIGMA2, X, z2, d=d).cpu().numpy(),
                _lib.precision_sqrt_t_apply_batch(*old, SIGMA2, X, z2, d=d).cpu().numpy())
        Bm = _dt(rng.standard_normal((n, nrhs)), dev)
        x_new, info_new = _lib.latent_ref_cg_batch(*geom, SIGMA2, Bm, torch.zeros_like(Bm), d=d_d, rtol=1e-9)
        x_old, info_old = _lib.latent_cg_batch(*old, SIGMA2, Bm, torch.zeros_like(Bm), d=d_d, rtol=1e-9)
        np.testing.assert_array_equal(x_new.cpu().numpy(), x_old.cpu().numpy())
        np.testing.assert_array_equal(info_new, info_old)
    for d in (None, d_d):
        np.testing.assert_array_equal(_lib.precision_ref_diag(*geom, SIGMA2, d=d).cpu().numpy(),
                                      _lib.precision_diag(old[5], n, m, SIGMA2, d=d).cpu().numpy())


# ---------------------------------------------------------------- column independence, repeatability
@pytest.mark.parametrize("shape", [(60, 200, 3, 2), (120, 300, 15, 2), (6, 700, 5, 2), (3, 50, 5, 2)],
                         ids=["60-200-3", "120-300-15", "6-700-5", "3-50-5"])
def test_columns_equal_one_column_calls(dev, shape):
    from pynngp_amd import _lib

    c = _case(*shape)
    n, n_s = c["n"], c["n_s"]
    geom = _geom(dev, c)
    d_d = _dt(c["d"], dev)
    rng = np.random.default_rng(11)
    for K in (2, 3, 8):
        scale = 10.0 ** rng.integers(-6, 7, K)
        X = _dt(rng.standard_normal((n_s, K)) * scale, dev)
        V = _dt(rng.standard_normal((n - n_s, K)), dev)
        Z = _dt(rng.standard_normal((n - n_s, K)), dev)
        Bm = _dt(rng.standard_normal((n_s, K)) * scale, dev)
        out = _lib.precision_ref_apply_batch(*geom, SIGMA2, X, d=d_d)
        np.testing.assert_array_equal(out.cpu().numpy(),
                                      _lib.precision_ref_apply_batch(*geom, SIGMA2, X, d=d_d).cpu().numpy())
        lv = _lib.latent_ref_leaves_batch(*geom, SIGMA2, X, v=V, z=Z, d=d_d)
        np.testing.assert_array_equal(lv.cpu().numpy(),
                                      _lib.latent_ref_leaves_batch(*geom, SIGMA2, X, v=V, z=Z, d=d_d).cpu().numpy())
        sol, info = _lib.latent_ref_cg_batch(*geom, SIGMA2, Bm, torch.zeros_like(Bm), d=d_d, rtol=1e-9)
        sol2, info2 = _lib.latent_ref_cg_batch(*geom, SIGMA2, Bm, torch.zeros_like(Bm), d=d_d, rtol=1e-9)
        np.testing.assert_array_equal(sol.cpu().numpy(), sol2.cpu().numpy())
        np.testing.assert_array_equal(info, info2)
        for k in range(K):
            col = lambda T: T[:, k:k + 1].contiguous()  # noqa: E731
            np.testing.assert_array_equal(
                out[:, k].cpu().numpy(), _lib.precision_ref_apply_batch(*geom, SIGMA2, col(X), d=d_d)[:, 0].cpu().numpy())
            np.testing.assert_array_equal(
                lv[:, k].cpu().numpy(),
                _lib.latent_ref_leaves_batch(*geom, SIGMA2, col(X), v=col(V), z=col(Z), d=d_d)[:, 0].cpu().numpy())
            b1 = col(Bm)
            s1, i1 = _lib.latent_ref_cg_batch(*geom, SIGMA2, b1, torch.zeros_like(b1), d=d_d, rtol=1e-9)
            np.testing.assert_array_equal(sol[:, k].cpu().numpy(), s1[:, 0].cpu().numpy())
            np.testing.assert_array_equal(info[k], i1[0])


# ---------------------------------------------------------------- solves
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("check_every", [1, 8])
def test_solves_match_dense(dev, shape, check_every):
    from pynngp_amd import _lib

    c = _case(*shape)
    n_s = c["n_s"]
    geom = _geom(dev, c)
    d_d = _dt(c["d"], dev)
    rng = np.random.default_rng(13)
    rtol = 1e-10
    Bm = np.concatenate([c["b"][:, None], rng.standard_normal((n_s, 2))], axis=1)
    exact = np.linalg.solve(c["A"], Bm)
    cond = np.linalg.cond(c["A"])
    X0 = np.zeros_like(Bm)
    X0[:, 2] = rng.standard_normal(n_s)  # a non-zero start in one column
    x, info = _lib.latent_ref_cg_batch(*geom, SIGMA2, _dt(Bm, dev), _dt(X0, dev), d=d_d, rtol=rtol,
                                       max_iter=20 * n_s + 100, check_every=check_every)
    x = x.cpu().numpy()
    assert np.all(info[:, 1] == 1), info
    for k in range(3):
        err = np.linalg.norm(x[:, k] - exact[:, k])
        assert err <= 2 * cond * rtol * np.linalg.norm(exact[:, k]), (k, err, cond)


def test_max_iter_cut_off_and_breakdown_stay_in_their_column(dev):
    from pynngp_amd import _lib

    c = _case(120, 300, 15, 2)
    n_s = c["n_s"]
    geom = _geom(dev, c)
    d_d = _dt(c["d"], dev)
    rng = np.random.default_rng(17)
    Bm = _dt(rng.standard_normal((n_s, 3)), dev)
    x, info = _lib.latent_ref_cg_batch(*geom, SIGMA2, Bm, torch.zeros_like(Bm), d=d_d, rtol=1e-14, max_iter=3)
    assert np.all(info[:, 0] == 3) and np.all(info[:, 1] == 0)
    good, ginfo = _lib.latent_ref_cg_batch(*geom, SIGMA2, Bm, torch.zeros_like(Bm), d=d_d, rtol=1e-10)
    # a NaN in one right-hand side breaks that column down and no other
    Bn = Bm.clone()
    Bn[5, 1] = float("nan")
    x, info = _lib.latent_ref_cg_batch(*geom, SIGMA2, Bn, torch.zeros_like(Bn), d=d_d, rtol=1e-10)
    assert info[1, 1] == -1 and info[0, 1] == 1 and info[2, 1] == 1
    for k in (0, 2):
        np.testing.assert_array_equal(x[:, k].cpu().numpy(), good[:, k].cpu().numpy())
        np.testing.assert_array_equal(info[k], ginfo[k])


# ---------------------------------------------------------------- the leaves kernel
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] > 0], ids=[i for s, i in zip(SHAPES, IDS) if s[1] > 0])
def test_leaves_match_closed_form(dev, shape):
    from pynngp_amd import _lib

    c = _case(*shape)
    n, n_s, m = c["n"], c["n_s"], c["m"]
    geom = _geom(dev, c)
    d_d = _dt(c["d"], dev)
    rng = np.random.default_rng(19)
    X = rng.standard_normal((n_s, 3))
    V, Z = rng.standard_normal((n - n_s, 3)), rng.standard_normal((n - n_s, 3))
    BL = -c["L"][n_s:]
    f, d = 1.0 / (SIGMA2 * c["F"][n_s:]), c["d"][n_s:]
    a, abs_a = BL @ X, np.abs(BL) @ np.abs(X)
    # the row-phase bound on the dot (m terms), and a few roundings for the closed form around it
    for v, z in ((V, Z), (V, None), (None, Z), (None, None)):
        got = _lib.latent_ref_leaves_batch(*geom, SIGMA2, _dt(X, dev), v=_dt(v, dev), z=_dt(z, dev), d=d_d).cpu().numpy()
        vv = np.zeros_like(V) if v is None else v
        exact = (f[:, None] * a + d[:, None] * vv) / (f + d)[:, None]
        mag = (f[:, None] * abs_a + d[:, None] * np.abs(vv)) / (f + d)[:, None]
        if z is not None:
            exact = exact + z / np.sqrt(f + d)[:, None]
            mag = mag + np.abs(z) / np.sqrt(f + d)[:, None]
        assert np.all(np.abs(got - exact) <= 4.0 * (m + 8) * U * mag)
    # d NULL: kriging of the columns, NNGP.predict's mean
    got = _lib.latent_ref_leaves_batch(*geom, SIGMA2, _dt(X, dev)).cpu().numpy()
    assert np.all(np.abs(got - a) <= 4.0 * (m + 2) * U * abs_a)
    gz = _lib.latent_ref_leaves_batch(*geom, SIGMA2, _dt(X, dev), z=_dt(Z, dev)).cpu().numpy()
    sd = np.sqrt(SIGMA2 * c["F"][n_s:])[:, None]
    assert np.all(np.abs(gz - (a + Z * sd)) <= 4.0 * (m + 8) * U * (abs_a + np.abs(Z) * sd))


def test_leaves_without_data_equal_nngp_predict(dev):
    """d NULL is kriging: the leaf rows' B / F come from the device's own knn_query + bf_cross (unit variance, no
    nugget), the very coefficients NNGP.predict factorises, so the two means differ by their two dot products of at
    most m terms alone -- the row-phase bound, nothing added."""
    from pynngp_amd import NNGP, Covariance, _lib

    c = _case(60, 200, 7, 2)
    n_s, m = c["n_s"], c["m"]
    rng = np.random.default_rng(23)
    w = rng.standard_normal(n_s)
    s_d, q_d = _dt(c["s"], dev), _dt(c["t_out"], dev)
    nbr_q = _lib.knn_query(s_d, q_d, m)
    B_q, F_q, _ = _lib.bf_cross(s_d, q_d, nbr_q, "exponential", 1.0, PHI, 0.0)
    nbr_a = torch.cat([_dt(c["nbr"][:n_s].astype(np.int32), dev), nbr_q]).contiguous()
    B_a = torch.cat([_dt(c["B"][:n_s], dev), B_q]).contiguous()
    F_a = torch.cat([_dt(c["F"][:n_s], dev), F_q]).contiguous()
    off, rev_j, rev_k = _lib.reverse_neighbors(nbr_a)
    prep = _lib.gibbs_prepare(B_a, F_a, off, rev_j, rev_k)
    got = _lib.latent_ref_leaves_batch(nbr_a, B_a, off, rev_j, rev_k, prep, n_s, 1.0,
                                       _dt(w[:, None], dev))[:, 0].cpu().numpy()
    model = NNGP(np.array(c["s"]), np.zeros(n_s), None, "S=T", m, Covariance("exponential", 1.0, PHI, 0.0), device=dev)
    mean, _ = model.predict(values=w, query=np.array(c["t_out"]))
    abs_a = (np.abs(B_q.cpu().numpy()) * np.abs(w[nbr_q.cpu().numpy()])).sum(axis=1)
    err = np.abs(got - mean)
    print(f"leaves vs predict: max err/bound {(err / (4.0 * (m + 2) * U * abs_a)).max():.3g}")
    assert np.all(err <= 4.0 * (m + 2) * U * abs_a)


# ---------------------------------------------------------------- LatentPosterior(ref=...)
def _device_dag(lp):
    """The node DAG and its unit-variance factors as the device built them, in MODEL node order (storage slot s
    holds node perm[s]).  The dense comparisons below use these coefficients, so that what they bound is the solve
    and the kernels' sums, not the difference between two evaluations of B."""
    perm = lp.perm.cpu().numpy()
    nbs = lp.nbr.cpu().numpy()
    n, m = nbs.shape
    nbr, B, F = np.full((n, m), -1, dtype=np.int32), np.zeros((n, m)), np.zeros(n)
    nbr[perm] = np.where(nbs >= 0, perm[np.maximum(nbs, 0)], -1)
    B[perm] = lp.B.cpu().numpy()
    F[perm] = lp.F.cpu().numpy()
    return nbr, B, F


@functools.lru_cache(maxsize=None)
def _posterior(dev, n_s, n_out, m, dim, with_X=True, on_ref=5):
    """A LatentPosterior on a reference set, ``on_ref`` data locations coinciding with reference points, ~30 %
    unobserved, random eps; and the dense posterior over its nodes in MODEL node order."""
    from pynngp_amd import Covariance, LatentPosterior

    c = _case(n_s, n_out, m, dim)
    rng = np.random.default_rng(29 + n_s)
    on_ref = min(on_ref, n_s)
    hit = rng.choice(n_s, size=on_ref, replace=False)
    t = np.concatenate([c["s"][hit], c["t_out"]])
    shuffle = rng.permutation(len(t))
    t = t[shuffle]
    N = len(t)
    X = np.column_stack([np.ones(N), rng.standard_normal(N)]) if with_X else None
    eps = rng.uniform(0.5, 2.0, N)
    y = rng.standard_normal(N) + (X @ np.array([0.7, -0.4]) if with_X else 0.0)
    y[rng.uniform(size=N) < 0.3] = np.nan
    y[0] = 0.3
    cov = Covariance("exponential", SIGMA2, PHI, TAU2)
    lp = LatentPosterior(t, y, cov, m=m, X=X, eps=eps, device=dev, ref=c["s"])
    node = lp.node_of_t
    n = lp.n_nodes
    assert n == n_s + n_out and lp.n_s == n_s
    coords_n = np.zeros((n, dim))
    coords_n[:n_s] = c["s"]
    coords_n[node] = t
    # the construction against the oracle's: the same DAG and, to the two sweeps' accuracy, the same factors
    _, nbr_o = G.reference_dag(coords_n[:n_s], coords_n[n_s:], m)
    B_o, F_o, _ = O.bf_sweep(coords_n, nbr_o, "exponential", (1.0, PHI, 0.0))
    nbr, B, F = _device_dag(lp)
    assert np.abs(G.dense_B(nbr, B) - G.dense_B(nbr_o, B_o)).max() <= 1e-9 and np.allclose(F, F_o, rtol=1e-9, atol=0)
    h, yn = np.zeros(n), np.zeros(n)
    obs = np.isfinite(y)
    h[node[obs]] = 1.0 / eps[obs] ** 2
    yn[node[obs]] = y[obs]
    Xn = np.zeros((n, 2 if with_X else 0))
    if with_X:
        Xn[node] = X
    return dict(lp=lp, t=t, y=y, X=X, eps=eps, node=node, nbr=nbr, B=B, F=F, h=h, yn=yn, Xn=Xn, n=n, n_s=n_s, m=m,
                coords_n=coords_n)


def _dense_gls(p):
    """Dense GLS beta under V = C~ + tau2 H^-1 over the observed nodes (C~ from the node DAG's precision)."""
    Q = G.precision(p["nbr"], p["B"], p["F"] * SIGMA2)
    C = np.linalg.inv(Q)
    o = p["h"] > 0
    V = C[np.ix_(o, o)] + np.diag(TAU2 / p["h"][o])
    Vi = np.linalg.inv(V)
    Xo, yo = p["Xn"][o], p["yn"][o]
    return np.linalg.solve(Xo.T @ Vi @ Xo, Xo.T @ Vi @ yo)


@pytest.mark.parametrize("shape", [(60, 200, 7, 2), (3, 50, 5, 2), (40, 90, 32, 2), (60, 200, 7, 3)],
                         ids=["60-200-7", "3-50-5", "40-90-32", "60-200-7-d3"])
def test_posterior_mean_and_gls_match_dense(dev, shape):
    p = _posterior(dev, *shape)
    lp, n_s = p["lp"], p["n_s"]
    rtol = 1e-11
    beta_exact = _dense_gls(p)
    w_data, beta = lp.mean(rtol=rtol)
    # p + 1 solves to rtol 1e-11 enter X^T V^-1 X and X^T V^-1 y through d (X - A^-1 d X): cond rtol ~ 1e-8 of unit-
    # scale sums, and the 2 x 2 normal equations are well conditioned
    assert np.allclose(beta, beta_exact, rtol=1e-7, atol=1e-9), (beta, beta_exact)
    yres = p["yn"] - p["Xn"] @ beta
    P, _, mu, _ = G.dag_posterior(p["nbr"], p["B"], p["F"], SIGMA2, TAU2, p["h"], yres)
    tol = 2 * np.linalg.cond(P) * rtol * np.linalg.norm(mu)
    assert np.abs(w_data - mu[p["node"]]).max() <= tol
    w_ref, _ = lp.mean(beta=beta, rtol=rtol, where="ref")
    assert w_ref.shape == (n_s,) and np.abs(w_ref - mu[:n_s]).max() <= tol
    # the operator and the solver take vectors on S in the order of ref
    A, b, _, _, _ = dense_ref_system(p["nbr"], p["B"], p["F"], n_s, SIGMA2, p["h"] / TAU2, yres)
    x = np.random.default_rng(1).standard_normal(n_s)
    assert np.allclose(lp.matvec(x), A @ x, rtol=0, atol=1e-10 * np.abs(A).sum(axis=1).max())
    sol, info = lp.solve(b, rtol=rtol)
    assert info.converged and np.abs(sol - mu[:n_s]).max() <= tol
    many, infos = lp.solve_many(np.stack([b, 2.0 * b]), rtol=rtol)
    assert np.abs(many[1] - 2.0 * mu[:n_s]).max() <= 2 * tol and all(i.converged for i in infos)


def test_draws_with_given_normals_match_dense_perturbation(dev):
    p = _posterior(dev, 60, 200, 7, 2)
    lp, n, n_s = p["lp"], p["n"], p["n_s"]
    rtol = 1e-11
    rng = np.random.default_rng(31)
    K = 5
    z1, z2, z3 = rng.standard_normal((K, n)), rng.standard_normal((K, n_s)), rng.standard_normal((K, n - n_s))
    beta = np.array([0.6, -0.3])
    yres = p["yn"] - p["Xn"] @ beta
    d = p["h"] / TAU2
    A, b, _, L, sc = dense_ref_system(p["nbr"], p["B"], p["F"], n_s, SIGMA2, d, yres)
    sign = np.concatenate([np.ones(n_s), -np.ones(n - n_s)])
    eta = (L.T @ ((sign * np.sqrt(sc))[:, None] * z1.T) + np.sqrt(d[:n_s])[:, None] * z2.T)
    WS = np.linalg.solve(A, b[:, None] + eta)  # (n_s, K)
    BL = -L[n_s:]
    f, dl = 1.0 / (SIGMA2 * p["F"][n_s:]), d[n_s:]
    WL = (f[:, None] * (BL @ WS) + (dl * yres[n_s:])[:, None]) / (f + dl)[:, None] + z3.T / np.sqrt(f + dl)[:, None]
    W = np.concatenate([WS, WL])
    tol = 2 * np.linalg.cond(A) * rtol * np.linalg.norm(W, axis=0).max()
    got = lp.sample(K, z=(z1, z2, z3), beta=beta, rtol=rtol, batch=3)
    assert got.shape == (K, len(p["t"])) and np.abs(got - W[p["node"]].T).max() <= tol
    got_ref = lp.sample(K, z=(z1, z2, z3), beta=beta, rtol=rtol, where="ref")
    assert np.abs(got_ref - WS.T).max() <= tol
    # Philox draws repeat bit for bit and do not depend on the chunking
    a = lp.sample(4, seed=9, beta=beta, batch=8)
    np.testing.assert_array_equal(a, lp.sample(4, seed=9, beta=beta, batch=3))
    assert np.abs(a - lp.sample(4, seed=10, beta=beta)).max() > 1e-3
    # without beta the draws use the GLS estimate
    d0 = lp.sample(2, seed=9)
    np.testing.assert_array_equal(d0, lp.sample(2, seed=9, beta=lp._beta_hat))
    assert np.allclose(lp._beta_hat, _dense_gls(p), rtol=1e-5, atol=1e-7)

    # marginal variance: the same estimator evaluated densely on the same normals (deterministic)
    diag = np.diag(A)
    C = WS - (A @ WS - b[:, None]) / diag[:, None]
    CL = (f[:, None] * (BL @ WS) + (dl * yres[n_s:])[:, None]) / (f + dl)[:, None]
    v_exact = np.concatenate([1.0 / diag + C.var(axis=1, ddof=1), 1.0 / (f + dl) + CL.var(axis=1, ddof=1)])
    v = lp.marginal_variance(K, z=(z1, z2), beta=beta, rtol=rtol, batch=2)
    # C carries the solve error amplified by A_ii^-1 |A| <= cond; the variance of K values of size |C| to that error
    scale = np.abs(np.concatenate([C, CL])).max()
    vtol = 8 * np.linalg.cond(A) * rtol * scale * scale + 1e-12 * v_exact.max()
    assert np.abs(v - v_exact[p["node"]]).max() <= vtol
    v_ref = lp.marginal_variance(K, z=(z1, z2), beta=beta, rtol=rtol, where="ref")
    assert np.abs(v_ref - v_exact[:n_s]).max() <= vtol


def test_predict_matches_dense(dev):
    for ref_case in (True, False):
        if ref_case:
            p = _posterior(dev, 60, 200, 7, 2)
            lp, n, n_s = p["lp"], p["n"], p["n_s"]
            s_pts = p["coords_n"][:n_s]
        else:
            from pynngp_amd import Covariance, LatentPosterior

            rng0 = np.random.default_rng(41)
            s_pts = rng0.uniform(size=(150, 2))
            y0 = rng0.standard_normal(150)
            lp = LatentPosterior(s_pts, y0, Covariance("exponential", SIGMA2, PHI, TAU2), m=7, X=np.ones((150, 1)),
                                 device=dev)
            n = n_s = 150
        m = lp.m
        rng = np.random.default_rng(37)
        Qn = 33
        q = rng.uniform(size=(Qn, 2))
        K = 6
        rtol = 1e-11
        if ref_case:
            z = (rng.standard_normal((K, n)), rng.standard_normal((K, n_s)), rng.standard_normal((K, n - n_s)))
        else:
            z = (rng.standard_normal((K, n)), rng.standard_normal((K, n)))
        zq = rng.standard_normal((K, Qn))
        beta = np.array([0.6, -0.3]) if ref_case else np.array([0.1])
        mean, var, draws = lp.predict(q, n_draws=K, z=z, zq=zq, beta=beta, rtol=rtol, batch=4)
        # dense: the query points as leaves of the reference points (model order)
        cq, nq = G.reference_dag(s_pts, q, m)
        Bq_rows, Fq, _ = O.bf_sweep(cq, nq, "exponential", (1.0, PHI, 0.0))
        Bq, Fq = G.dense_B(nq, Bq_rows)[n_s:, :n_s], Fq[n_s:]
        w_hat, _ = lp.mean(beta=beta, rtol=rtol, where="ref")
        WS = lp.sample(K, z=z, beta=beta, rtol=rtol, where="ref").T  # checked against dense above
        scale = np.abs(Bq) @ np.abs(WS).max(axis=1)
        # predict keeps its B_q / F_q to itself, so the dense side has the oracle's: no solve lies between, only the
        # two evaluations of the coefficients, which agree to 1e-9 absolute (the bound smoke() and
        # tests/test_gpu_bf.py hold the device sweep to against this oracle)
        tol = 1e-9 * scale.max()
        assert np.abs(mean - Bq @ w_hat).max() <= tol
        M = Bq @ WS
        assert np.abs(draws.T - (M + np.sqrt(SIGMA2 * Fq)[:, None] * zq.T)).max() <= tol
        assert np.abs(var - (SIGMA2 * Fq + M.var(axis=1, ddof=1))).max() <= 1e-9 * (SIGMA2 + scale.max() ** 2)
        m0, v0, d0 = lp.predict(q, beta=beta, rtol=rtol)
        assert v0 is None and d0.shape == (0, Qn) and np.abs(m0 - mean).max() <= tol
        # Philox draws: draw k does not depend on how many draws are asked for, with the response noise too
        _, _, da = lp.predict(q, n_draws=2, seed=3, beta=beta, response=True)
        _, _, db = lp.predict(q, n_draws=5, seed=3, beta=beta, response=True, batch=3)
        np.testing.assert_array_equal(da, db[:2])
        # response draws add noise of variance tau2 from their own stream; the latent part is unchanged
        _, _, dr = lp.predict(q, n_draws=K, z=z, zq=zq, beta=beta, rtol=rtol, response=True)
        extra = dr - draws
        assert 0.2 * TAU2 < extra.var() < 3.0 * TAU2


def test_ref_none_is_the_existing_path_bit_for_bit(dev):
    """LatentPosterior without ref: the mean, a draw and marginal_variance equal the S = T calls issued by hand in the
    order the class issued them before it knew of reference sets."""
    from pynngp_amd import Covariance, LatentPosterior, _lib

    rng = np.random.default_rng(43)
    n, m = 300, 7
    t, y = rng.uniform(size=(n, 2)), rng.standard_normal(n)
    lp = LatentPosterior(t, y, Covariance("exponential", SIGMA2, PHI, TAU2), m=m, device=dev)
    assert not lp._ref and lp.n_s == lp.n_nodes == n
    w, _ = lp.mean()
    b = (lp.d * lp.y).contiguous()
    x = torch.zeros_like(b)
    _lib.latent_cg(*lp._geom(), b, x, d=lp.d, rtol=1e-8, max_iter=1000, check_every=8)
    np.testing.assert_array_equal(w, x[lp.pos].cpu().numpy())
    np.testing.assert_array_equal(lp.mean(where="ref")[0], w)
    # draw 0 is A^-1 (b + eta) with eta from the Philox streams 0 and 1
    zz = torch.empty(n, dtype=torch.float64, device=dev)
    Z1 = _lib.gibbs_normals(zz, 5, 0).clone()[:, None].contiguous()
    Z2 = _lib.gibbs_normals(zz, 5, 1).clone()[:, None].contiguous()
    eta = _lib.precision_sqrt_t_apply_batch(*lp._geom(), Z1, Z2, d=lp.d)
    rhs = (b[:, None] + eta).contiguous()
    X, _ = _lib.latent_cg_batch(*lp._geom(), rhs, torch.zeros_like(rhs), d=lp.d, rtol=1e-8, max_iter=1000)
    np.testing.assert_array_equal(lp.sample(1, seed=5)[0], X[:, 0][lp.pos].cpu().numpy())
    # marginal_variance(3): one chunk of three draws, A W, the conditional means and their running sums
    K = 3
    Z1, Z2 = (torch.empty((n, K), dtype=torch.float64, device=dev) for _ in range(2))
    for k in range(K):
        Z1[:, k] = _lib.gibbs_normals(zz, 5, 2 * k)
        Z2[:, k] = _lib.gibbs_normals(zz, 5, 2 * k + 1)
    eta = _lib.precision_sqrt_t_apply_batch(*lp._geom(), Z1, Z2, d=lp.d)
    rhs = (b[:, None] + eta).t().t().contiguous()
    W, _ = _lib.latent_cg_batch(*lp._geom(), rhs, torch.zeros_like(rhs), d=lp.d, rtol=1e-8, max_iter=1000)
    aii = _lib.precision_diag(lp._prep, n, m, SIGMA2, d=lp.d)
    C = W - (_lib.precision_apply_batch(*lp._geom(), W, d=lp.d) - b[:, None]) / aii[:, None]
    shift = C[:, 0].clone()
    s1, s2 = torch.zeros_like(shift), torch.zeros_like(shift)
    for k in range(K):
        dev_k = C[:, k] - shift
        s1 += dev_k
        s2 += dev_k * dev_k
    v = 1.0 / aii + (s2 - s1 * s1 / K) / (K - 1)
    np.testing.assert_array_equal(lp.marginal_variance(K, seed=5), v[lp.pos].cpu().numpy())
    np.testing.assert_array_equal(lp.marginal_variance(K, seed=5, where="ref"), v[lp.pos].cpu().numpy())


def test_reference_set_without_leaves(dev):
    """Every data location coincides with a reference point (('subset', N) without repeats): no leaf, n_s = n, the
    S = T launches serve the calls; mean, draws and variances run and agree with the dense posterior."""
    from pynngp_amd import Covariance, LatentPosterior

    rng = np.random.default_rng(53)
    n, m = 50, 7
    s = rng.uniform(size=(n, 2))
    order = rng.permutation(n)
    t, y = s[order], rng.standard_normal(n)
    y[3] = np.nan
    lp = LatentPosterior(t, y, Covariance("exponential", SIGMA2, PHI, TAU2), m=m, device=dev, ref=s)
    assert lp._ref and lp.n_nodes == lp.n_s == n and np.array_equal(lp.node_of_t, order)
    rtol = 1e-11
    nbr, B, F = _device_dag(lp)
    h, yn = np.zeros(n), np.zeros(n)
    obs = np.isfinite(y)
    h[order[obs]], yn[order[obs]] = 1.0, y[obs]
    P, _, mu, cov = G.dag_posterior(nbr, B, F, SIGMA2, TAU2, h, yn)
    tol = 2 * np.linalg.cond(P) * rtol * np.linalg.norm(mu)
    w, _ = lp.mean(rtol=rtol)
    assert np.abs(w - mu[order]).max() <= tol
    assert np.abs(lp.mean(rtol=rtol, where="ref")[0] - mu).max() <= tol
    d_data, d_ref = lp.sample(3, seed=2), lp.sample(3, seed=2, where="ref")
    np.testing.assert_array_equal(d_data, d_ref[:, order])
    K = 4
    z = (rng.standard_normal((K, n)), rng.standard_normal((K, n)), np.zeros((K, 0)))
    np.testing.assert_array_equal(lp.sample(K, z=z, where="ref")[:, order], lp.sample(K, z=z))
    v = lp.marginal_variance(K, z=z[:2], rtol=rtol, where="ref")
    assert v.shape == (n,) and np.all(v >= 1.0 / np.diag(P))  # 1 / A_ii plus a sample variance
    mean, var, draws = lp.predict(rng.uniform(size=(5, 2)), n_draws=3)
    assert mean.shape == (5,) and draws.shape == (3, 5) and np.all(var > 0)


@pytest.mark.parametrize("n,m,dim", [(300, 7, 2), (40, 3, 1)], ids=["300-7-2d", "line-40-3"])
def test_leafless_reference_set_is_s_equals_t_bit_for_bit(dev, n, m, dim):
    """ref = the data locations themselves: the same nodes, neighbour sets and storage as without ref, so every
    result of the class is the S = T one, bit for bit (the line: rows with -1 slots)."""
    from pynngp_amd import Covariance, LatentPosterior

    rng = np.random.default_rng(61)
    t = rng.uniform(size=(n, dim)) if dim > 1 else np.linspace(0.0, 1.0, n)[:, None]
    y = rng.standard_normal(n)
    y[[2, n // 3, n - 5]] = np.nan
    X = np.column_stack([np.ones(n), rng.standard_normal(n)])
    eps = rng.uniform(0.5, 2.0, n)
    q = rng.uniform(size=(5, dim))
    cov = Covariance("exponential", SIGMA2, PHI, TAU2)
    a = LatentPosterior(t, y, cov, m=m, X=X, eps=eps, device=dev)
    b = LatentPosterior(t, y, cov, m=m, X=X, eps=eps, device=dev, ref=t)
    assert not a._ref and b._ref
    for lp in (a, b):
        assert lp.n_s == lp.n_nodes == n
    for ra, rb in zip(a.mean(), b.mean()):
        np.testing.assert_array_equal(ra, rb)
    np.testing.assert_array_equal(a.gls_beta(), b.gls_beta())
    np.testing.assert_array_equal(a.sample(3, seed=5), b.sample(3, seed=5))
    np.testing.assert_array_equal(a.sample(9, seed=5, batch=4)[:3], b.sample(9, seed=5, batch=4)[:3])
    np.testing.assert_array_equal(a.marginal_variance(4, seed=5), b.marginal_variance(4, seed=5))
    for ra, rb in zip(a.predict(q, n_draws=3, seed=5), b.predict(q, n_draws=3, seed=5)):
        np.testing.assert_array_equal(ra, rb)


def test_nngp_latent_posterior_on_a_random_reference_set(dev):
    from pynngp_amd import NNGP, Covariance

    rng = np.random.default_rng(47)
    N, m = 250, 7
    t, y = rng.uniform(size=(N, 2)), rng.standard_normal(N)
    y[::9] = np.nan
    bounds = [(0.0, 1.0), (0.0, 1.0)]
    model = NNGP(t, y, None, ("random", 80, bounds), m, Covariance("exponential", SIGMA2, PHI, TAU2), device=dev)
    with pytest.raises(NotImplementedError):
        model.latent_mean()
    lp = model.latent_posterior(mean="zero")
    assert lp is model.latent_posterior(mean="zero") and lp.n_s == 80 and lp.n_nodes == 80 + N
    rtol = 1e-11
    w, beta = lp.mean(rtol=rtol)
    assert beta.shape == (0,)
    s = np.asarray(model.s, dtype=np.float64)
    coords_n, nbr_o = G.reference_dag(s, t, m)
    B_o, F_o, _ = O.bf_sweep(coords_n, nbr_o, "exponential", (1.0, PHI, 0.0))
    nbr, B, F = _device_dag(lp)  # nodes: s, then t in its order
    assert np.abs(G.dense_B(nbr, B) - G.dense_B(nbr_o, B_o)).max() <= 1e-9 and np.allclose(F, F_o, rtol=1e-9, atol=0)
    obs = np.isfinite(y)
    h = np.concatenate([np.zeros(80), obs.astype(float)])
    yn = np.concatenate([np.zeros(80), np.where(obs, y, 0.0)])
    P, _, mu, _ = G.dag_posterior(nbr, B, F, SIGMA2, TAU2, h, yn)
    tol = 2 * np.linalg.cond(P) * rtol * np.linalg.norm(mu)
    assert np.abs(w - mu[80:]).max() <= tol
    assert np.abs(lp.mean(rtol=rtol, where="ref")[0] - mu[:80]).max() <= tol
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        mean, var, draws = lp.predict(rng.uniform(size=(10, 2)), n_draws=4)
    assert mean.shape == (10,) and draws.shape == (4, 10) and np.all(var > 0)
