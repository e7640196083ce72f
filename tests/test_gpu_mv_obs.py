"""The packed-row multivariate sweep (outcomes missing at some sites) against a dense fp64 reference: per location the
joint covariance over the *observed* rows from LMCCovariance.__call__, np.linalg.cholesky and solves, scattered to the
slot-major shapes.  Bounds (tests/test_gpu_mv.py's): |dB| <= 1e-9 (1 + |B|), |dF| <= 1e-10 min diag F,
|dE| <= 1e-9 (1 + |E|), partials within 1e-11 sum |terms|.

The neighbour sets are the m nearest prior sites, cut to the longest prefix of slots with at most 64 observed rows (-1
beyond): at (3, 45, sparse) the first 45 sites alone carry 45 + 2 * 12 = 69 rows, whatever the seed."""
import numpy as np
import pytest
import torch

import pynngp_amd as A
from pynngp_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
AFULL = np.array([[1.0, 0, 0, 0], [0.5, 0.9, 0, 0], [0.3, 0.6, 0.8, 0], [0.7, 0.4, 0.35, 0.95]])
N = 160


def model(q, kind="exponential"):
    k = np.arange(q)
    return A.LMCCovariance(kind, AFULL[:q, :q], 3.0 + 2.5 * k, 0.05 * (1 + k))


def inputs(q, dim=2, c=1, seed=0, n=N):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (n, dim)), rng.standard_normal((n, q, c))


def masks(pattern, q, n=N):
    i = np.arange(n)
    if pattern == "full":
        return np.full(n, 2 ** q - 1, dtype=np.uint8)
    if pattern == "sparse":
        return (1 + (2 ** q - 2) * (i % 4 == 0)).astype(np.uint8)
    obs = (1 + (5 * i + 3) % (2 ** q - 1)).astype(np.uint8)
    if pattern == "cyc0":
        obs[[7, 30, 31, 90]] = 0  # sites with nothing observed
    return obs


def bits(obs, q):
    return (obs[:, None] >> np.arange(q)) & 1 != 0


def rows_of(nbr, obs, q):
    ok = (nbr >= 0) & (nbr < len(obs))
    return (bits(obs, q).sum(1)[np.clip(nbr, 0, len(obs) - 1)] * ok).sum(1)


def cut(nbr, obs, q):
    """Each row's longest prefix of slots with at most 64 observed rows; asserts the bound on the CPU."""
    ok = (nbr >= 0) & (nbr < len(obs))
    run = np.cumsum(bits(obs, q).sum(1)[np.clip(nbr, 0, len(obs) - 1)] * ok, axis=1)
    nbr = np.where(run <= 64, nbr, -1).astype(np.int32)
    rows_max = int(rows_of(nbr, obs, q).max())
    assert 1 <= rows_max <= 64
    return nbr, rows_max


def reference(cov, coords, nbr, vals, obs, query=None, noise=True):
    """B, F, E (or the conditional mean for query points) in the slot-major shapes, zeros where a row is not observed,
    and the per-row terms of the two partials."""
    q, (rows, m), c, ob = cov.q, nbr.shape, vals.shape[2], bits(obs, cov.q)
    B, F, E = np.zeros((rows, q, m * q)), np.zeros((rows, q, q)), np.zeros((rows, q, c))
    ld, qd = np.zeros(rows), np.zeros(rows)
    T = np.diag(cov.tau2)
    for i in range(rows):
        slots = np.nonzero((nbr[i] >= 0) & (nbr[i] < len(coords)))[0]
        js = nbr[i, slots]
        sel = ob[js].ravel()
        tm = np.nonzero(ob[i] if query is None else np.ones(q, bool))[0]
        if not len(tm):
            continue
        tgt = (coords if query is None else query)[i:i + 1]
        Fi, mu = (cov(tgt, tgt) + (T if noise else 0.0))[np.ix_(tm, tm)], np.zeros((len(tm), c))
        if sel.any():
            L = np.linalg.cholesky((cov(coords[js], coords[js]) + np.kron(np.eye(len(js)), T))[np.ix_(sel, sel)])
            W = np.linalg.solve(L, cov(coords[js], tgt)[np.ix_(sel, tm)]).T
            Bi = np.linalg.solve(L.T, W.T).T
            B[i][np.ix_(tm, (slots[:, None] * q + np.arange(q)).ravel()[sel])] = Bi
            Fi, mu = Fi - W @ W.T, Bi @ vals[js].reshape(len(js) * q, c)[sel]
        F[i][np.ix_(tm, tm)] = Fi
        LF = np.linalg.cholesky(Fi)
        E[i][tm] = mu if query is not None else np.linalg.solve(LF, vals[i][tm] - mu)
        ld[i], qd[i] = 2.0 * np.log(np.diag(LF)).sum(), (E[i][:, 0] ** 2).sum()
    return B, F, E, ld, qd


def dev(*xs):
    return [torch.as_tensor(np.ascontiguousarray(x)).to(DEV) for x in xs]


def check(got, ref, cross=False):
    B, LF, E, p = [x.cpu().numpy() for x in got]
    Br, Fr, Er, ld, qd = ref
    assert all(np.isfinite(x).all() for x in (B, LF, E, p))
    F = LF @ LF.transpose(0, 2, 1)
    d = np.diagonal(Fr, axis1=1, axis2=2)
    fmin = np.where(d > 0, d, np.inf).min(axis=1)[:, None, None]  # inf: nothing observed, F must be exactly 0
    eb, ef, ee = np.abs(B - Br) / (1 + np.abs(Br)), np.abs(F - Fr) / fmin, np.abs(E - Er) / (1 + np.abs(Er))
    print(f"max dB {eb.max():.2e} dF {ef.max():.2e} dE {ee.max():.2e}")
    assert np.all(np.triu(LF, 1) == 0) and p[2] == -1 and p[3] == -1
    assert np.all(B[Br == 0] == 0) and np.all(F[Fr == 0] == 0)
    assert eb.max() <= 1e-9 and ef.max() <= 1e-10 and ee.max() <= 1e-9
    assert abs(p[0] - ld.sum()) <= 1e-11 * np.abs(ld).sum()
    assert abs(p[1] - (0.0 if cross else qd.sum())) <= 1e-11 * qd.sum()


def setup(q, m, pattern, dim=2, c=None, n=N):
    """coords, values with NaN under every clear bit, masks and the cut sets, on the host and on the GPU."""
    coords, vals = inputs(q, dim, 1 + q if c is None else c, n=n)
    obs = masks(pattern, q, n)
    vals[~bits(obs, q)] = np.nan
    nbr, rows_max = cut(_lib.knn_prior(dev(coords)[0], m).cpu().numpy(), obs, q)
    return coords, vals, obs, nbr, rows_max, dev(coords, vals, obs, nbr)


SHAPES = [(2, 1, "cyc"), (2, 8, "full"), (3, 11, "full"), (4, 7, "cyc"), (3, 10, "cyc0"), (3, 20, "cyc"),
          (4, 15, "cyc"), (2, 31, "cyc"), (2, 40, "sparse"), (3, 45, "sparse")]
CASES = [(q, m, pat, kind, 2) for q, m, pat in SHAPES for kind in ("exponential", "matern32")] + \
        [(3, 10, "cyc0", "matern52", 2), (3, 10, "cyc0", "gaussian", 2), (3, 10, "cyc0", "matern32", 1),
         (3, 10, "cyc0", "matern32", 3)]


@pytest.mark.parametrize("q,m,pattern,kind,dim", CASES)
def test_sweep_parity(q, m, pattern, kind, dim):
    cov = model(q, kind)
    coords, vals, obs, nbr, rows_max, (cd, vd, od, nd) = setup(q, m, pattern, dim)
    args = (cd, nd, 0, kind, cov.A, cov.phi, cov.tau2, od, rows_max, vd)
    got = _lib.bf_sweep_mv_obs(*args)
    check(got, reference(cov, coords, nbr, vals, obs))
    lik = _lib.bf_sweep_mv_obs(*args, want_b=False, want_lf=False)
    assert lik[0] is None and torch.equal(lik[3], got[3])
    if pattern == "full":
        old = _lib.bf_sweep_mv(cd, nd, 0, kind, cov.A, cov.phi, cov.tau2, vd)
        for x, y in zip(got, old):
            assert float((x - y).abs().max()) <= 1e-12 * float(y.abs().max())


@pytest.mark.parametrize("kind", ["exponential", "matern32"])
def test_known_answer(kind):
    """28 sites, every location conditioning on all earlier ones: the dense normal log-density of the 48 observed
    entries."""
    q, n, cov = 3, 28, model(3, kind)
    coords, vals = inputs(q, 2, 1, seed=1, n=n)
    obs = (np.arange(n) % 7 + 1).astype(np.uint8)
    ob = bits(obs, q)
    vals[~ob] = np.nan
    cd, vd, od = dev(coords, vals, obs)
    nbr = _lib.knn_prior(cd, n - 1)
    rows_max = int(rows_of(nbr.cpu().numpy(), obs, q).max())
    assert ob.sum() == 48 and rows_max <= 64
    p = _lib.bf_sweep_mv_obs(cd, nbr, 0, kind, cov.A, cov.phi, cov.tau2, od, rows_max, vd, want_b=False)[3].cpu().numpy()
    ll = -0.5 * (48 * np.log(2 * np.pi) + p[0] + p[1])
    sel = ob.ravel()
    K = (cov(coords, coords) + np.kron(np.eye(n), np.diag(cov.tau2)))[np.ix_(sel, sel)]
    y = vals[:, :, 0].ravel()[sel]
    llr = -0.5 * (48 * np.log(2 * np.pi) + np.linalg.slogdet(K)[1] + y @ np.linalg.solve(K, y))
    assert p[2] == -1 and p[3] == -1 and abs(ll - llr) <= 1e-10 * abs(llr)


@pytest.mark.parametrize("q,m", [(2, 8), (4, 15)])
@pytest.mark.parametrize("noise", [True, False])
def test_cross_parity(q, m, noise):
    cov = model(q, "matern32")
    coords, vals, obs, _, _, (cd, vd, od, _) = setup(q, m, "cyc", c=2)
    query = np.random.default_rng(1).uniform(0.0, 1.0, (37, 2))
    query[5] = coords[11]  # a query on a data site that lacks outcome 0
    assert not bits(obs, q)[11, 0]
    qd = dev(query)[0]
    nbr = _lib.knn_query(cd, qd, m)
    rows_max = int(rows_of(nbr.cpu().numpy(), obs, q).max())
    assert rows_max <= 64
    ref = reference(cov, coords, nbr.cpu().numpy(), vals, obs, query, noise)
    check(_lib.bf_cross_mv_obs(cd, qd, nbr, cov.kind, cov.A, cov.phi, cov.tau2, od, rows_max, vd, target_noise=noise),
          ref, cross=True)


def test_bit_identity_order_and_ops():
    q, m, cov = 3, 10, model(3)
    _, _, obs, _, rows_max, (cd, vd, od, nd) = setup(q, m, "cyc", c=2)
    args = (cov.kind, cov.A, cov.phi, cov.tau2, od, rows_max, vd)
    a = _lib.bf_sweep_mv_obs(cd, nd, 0, *args)
    assert all(torch.equal(x, y) for x, y in zip(a, _lib.bf_sweep_mv_obs(cd, nd, 0, *args)))
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(3)).to(DEV)
    o = _lib.bf_sweep_mv_obs(cd, nd[perm].contiguous(), 0, *args, order=perm.int())
    assert all(torch.equal(x, y) for x, y in zip(a, o))
    ops = A.load_ops()
    flat, code = [x for row in cov.A for x in row], ops.kind_code(cov.kind)
    t = torch.ops.nngp.bf_sweep_mv_obs(cd, nd, None, 0, code, flat, cov.phi, cov.tau2, vd, od, rows_max, True)
    assert all(torch.equal(x, y) for x, y in zip(a, t))
    qd = dev(cd[:9].cpu().numpy() + 0.01)[0]
    nq = _lib.knn_query(cd, qd, m)
    rq = int(rows_of(nq.cpu().numpy(), obs, q).max())
    assert rq <= 64
    c1 = _lib.bf_cross_mv_obs(cd, qd, nq, cov.kind, cov.A, cov.phi, cov.tau2, od, rq, vd, target_noise=False)
    c2 = torch.ops.nngp.bf_cross_mv_obs(cd, qd, nq, code, flat, cov.phi, cov.tau2, False, vd, od, rq)
    assert all(torch.equal(x, y) for x, y in zip(c1[:3], c2))


def test_end_to_end():
    q, m = 3, 10
    cov = model(q, "matern32")
    coords, vals = inputs(q, 2, 1)
    obs = masks("cyc", q)
    ob = bits(obs, q)
    Y = np.where(ob, vals[:, :, 0] + np.array([1.0, -2.0, 0.5]), np.nan)
    g = A.MultivariateNNGP(coords, Y, m, cov)
    nbr = g._nbr.cpu().numpy()
    assert np.array_equal(g.obs, obs) and rows_of(nbr, obs, q).max() <= 64
    ll, mu = g.loglik(mean="constant")
    X = np.zeros((N, q, q))
    X[:, np.arange(q), np.arange(q)] = ob
    _, _, Er, ld, _ = reference(cov, coords, nbr, np.concatenate([Y[:, :, None], X], axis=2), obs)
    Er = Er.reshape(N * q, 1 + q)
    mur = np.linalg.lstsq(Er[:, 1:], Er[:, 0], rcond=None)[0]
    llr = -0.5 * (ob.sum() * np.log(2 * np.pi) + ld.sum() + ((Er[:, 0] - Er[:, 1:] @ mur) ** 2).sum())
    assert np.allclose(mu, mur, rtol=1e-9, atol=1e-9) and abs(ll - llr) <= 1e-10 * abs(llr)
    assert g.B.shape == (N, q, m * q) and g.LF.shape == (N, q, q)
    im, sd = g.impute()
    rows = np.nonzero(~ob.all(1))[0]
    qn = _lib.knn_query(*dev(coords, coords[rows]), m).cpu().numpy()
    _, Fr, mr, _, _ = reference(cov, coords, qn, Y[:, :, None], obs, coords[rows])
    assert np.array_equal(im[ob], Y[ob]) and np.all(sd[ob] == 0)
    miss = ~ob[rows]
    assert np.allclose(im[rows][miss], mr[:, :, 0][miss], rtol=1e-9, atol=1e-9)
    assert np.allclose(sd[rows][miss], np.sqrt(np.diagonal(Fr, axis1=1, axis2=2))[miss], rtol=1e-9, atol=1e-12)
    pm, pc = g.predict(np.random.default_rng(2).uniform(0.0, 1.0, (20, 2)), noise=False)
    assert np.isfinite(pm).all() and np.isfinite(pc).all()
    with pytest.raises(NotImplementedError):
        g.loglik_grad()


def test_refusals():
    cov = model(2)
    coords, vals = inputs(2)
    Y = vals[:, :, 0].copy()
    with pytest.raises(NotImplementedError):  # a full Y: bf_mv's limit, as before
        A.MultivariateNNGP(coords, Y, 32, cov)
    Y[0, 1] = np.nan
    nbr = np.where(np.arange(33) < np.arange(N)[:, None], np.arange(33), -1).astype(np.int32)
    with pytest.raises(ValueError, match="65 observed"):  # sites 0..32: 66 rows less the missing one
        A.MultivariateNNGP(coords, Y, 33, cov, nbr=nbr)
    g = A.MultivariateNNGP(coords, Y, 33, cov, nbr=np.where(nbr == 1, -1, nbr))
    assert g._rows_max == 63 and np.isfinite(g.loglik())
