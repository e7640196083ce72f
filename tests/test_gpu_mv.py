"""The multivariate (coregionalised) sweep on the GPU against a dense fp64 reference: per row the joint block from
LMCCovariance.__call__, np.linalg.cholesky and solves.  Bounds: |dB| <= 1e-9 (1 + |B|), |dF| / F <= 1e-10 relative to
the smallest diagonal of F, |d partial| <= 1e-11 sum |terms| (the project's forward bounds; the inputs below keep the
joint blocks' condition numbers below 1e3)."""
import numpy as np
import pytest
import torch

import pynngp_amd as A
from pynngp_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KINDS = ("exponential", "matern32", "matern52", "gaussian")
AFULL = np.array([[1.0, 0, 0, 0], [0.5, 0.9, 0, 0], [0.3, 0.6, 0.8, 0], [0.7, 0.4, 0.35, 0.95]])
N = 160


def model(q, kind="exponential", tau2=None):
    k = np.arange(q)
    return A.LMCCovariance(kind, AFULL[:q, :q], 3.0 + 2.5 * k, 0.05 * (1 + k) if tau2 is None else tau2)


def inputs(q, dim=2, c=1, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (N, dim)), rng.standard_normal((N, q, c))


def reference(cov, coords, nbr, vals, query=None, noise=True):
    """B, F, E (or the conditional mean for query points), and the per-row terms of the two partials."""
    q, (rows, m), c = cov.q, nbr.shape, vals.shape[2]
    B, F, E = np.zeros((rows, q, m * q)), np.zeros((rows, q, q)), np.zeros((rows, q, c))
    ld, qd = np.zeros(rows), np.zeros(rows)
    T = np.diag(cov.tau2)
    for i in range(rows):
        slots = np.nonzero((nbr[i] >= 0) & (nbr[i] < len(coords)))[0]
        js = nbr[i, slots]
        tgt = (coords if query is None else query)[i:i + 1]
        Fi, mu = cov(tgt, tgt) + (T if noise else 0.0), np.zeros((q, c))
        if len(js):
            L = np.linalg.cholesky(cov(coords[js], coords[js]) + np.kron(np.eye(len(js)), T))
            W = np.linalg.solve(L, cov(coords[js], tgt)).T
            Bi = np.linalg.solve(L.T, W.T).T
            B[i][:, (slots[:, None] * q + np.arange(q)).ravel()] = Bi
            Fi, mu = Fi - W @ W.T, Bi @ vals[js].reshape(len(js) * q, c)
        F[i] = Fi
        LF = np.linalg.cholesky(Fi)
        E[i] = mu if query is not None else np.linalg.solve(LF, vals[i] - mu)
        ld[i], qd[i] = 2.0 * np.log(np.diag(LF)).sum(), (E[i][:, 0] ** 2).sum()
    return B, F, E, ld, qd


def dev(*xs):
    return [torch.as_tensor(np.ascontiguousarray(x)).to(DEV) for x in xs]


def check(got, ref, cross=False):
    B, LF, E, p = [x.cpu().numpy() for x in got]
    Br, Fr, Er, ld, qd = ref
    F = LF @ LF.transpose(0, 2, 1)
    fmin = np.diagonal(Fr, axis1=1, axis2=2).min(axis=1)[:, None, None]
    eb, ef, ee = np.abs(B - Br) / (1 + np.abs(Br)), np.abs(F - Fr) / fmin, np.abs(E - Er) / (1 + np.abs(Er))
    print(f"max dB {eb.max():.2e} dF {ef.max():.2e} dE {ee.max():.2e}")
    assert np.all(np.triu(LF, 1) == 0) and p[2] == -1 and p[3] == -1
    assert eb.max() <= 1e-9 and ef.max() <= 1e-10 and ee.max() <= 1e-9
    assert abs(p[0] - ld.sum()) <= 1e-11 * np.abs(ld).sum()
    assert abs(p[1] - (0.0 if cross else qd.sum())) <= 1e-11 * qd.sum()


def run_parity(q, m, kind, dim=2):
    cov = model(q, kind)
    coords, vals = inputs(q, dim, 1 + q)
    cd, vd = dev(coords, vals)
    nbr = _lib.knn_prior(cd, m)
    ref = reference(cov, coords, nbr.cpu().numpy(), vals)
    check(_lib.bf_sweep_mv(cd, nbr, 0, kind, cov.A, cov.phi, cov.tau2, vd), ref)
    one = _lib.bf_sweep_mv(cd, nbr, 0, kind, cov.A, cov.phi, cov.tau2, vd[:, :, :1].contiguous())
    check(one, ref[:2] + (ref[2][:, :, :1],) + ref[3:])
    lik = _lib.bf_sweep_mv(cd, nbr, 0, kind, cov.A, cov.phi, cov.tau2, vd, want_b=False, want_lf=False)
    assert lik[0] is None and torch.equal(lik[3], _lib.bf_sweep_mv(cd, nbr, 0, kind, cov.A, cov.phi, cov.tau2, vd)[3])


def test_mfma_lane_map():
    """One tile (n = 16) with distinct columns of A and scattered points: a transposed or permuted operand or
    accumulator map (A[i][k] in lane i + 16 k, B[k][j] in lane j + 16 k, D[4 r + l / 16][l % 16]) cannot pass."""
    run_parity(4, 3, "exponential")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("q,m", [(2, 7), (2, 8), (4, 7), (3, 10), (3, 15), (2, 24), (3, 20), (4, 15), (2, 31), (2, 1)])
def test_sweep_parity(q, m, kind):
    run_parity(q, m, kind)


@pytest.mark.parametrize("dim", [1, 3])
def test_sweep_parity_dims(dim):
    run_parity(3, 10, "matern32", dim)


@pytest.mark.parametrize("q,m", [(2, 8), (4, 15)])
@pytest.mark.parametrize("noise", [True, False])
def test_cross_parity(q, m, noise):
    cov = model(q, "matern32")
    coords, vals = inputs(q, 2, 2)
    query = np.random.default_rng(1).uniform(0.0, 1.0, (37, 2))
    query[5] = coords[11]  # a query on a data point
    cd, vd, qd = dev(coords, vals, query)
    nbr = _lib.knn_query(cd, qd, m)
    ref = reference(cov, coords, nbr.cpu().numpy(), vals, query, noise)
    check(_lib.bf_cross_mv(cd, qd, nbr, cov.kind, cov.A, cov.phi, cov.tau2, vd, target_noise=noise), ref, cross=True)


def test_bit_identity_order_and_ops():
    q, m, cov = 3, 10, model(3)
    coords, vals = inputs(q, 2, 2)
    cd, vd = dev(coords, vals)
    nbr = _lib.knn_prior(cd, m)
    a = _lib.bf_sweep_mv(cd, nbr, 0, cov.kind, cov.A, cov.phi, cov.tau2, vd)
    b = _lib.bf_sweep_mv(cd, nbr, 0, cov.kind, cov.A, cov.phi, cov.tau2, vd)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(3)).to(DEV)
    o = _lib.bf_sweep_mv(cd, nbr[perm].contiguous(), 0, cov.kind, cov.A, cov.phi, cov.tau2, vd, order=perm.int())
    assert all(torch.equal(x, y) for x, y in zip(a, o))
    ops = A.load_ops()
    flat = [x for row in cov.A for x in row]
    t = torch.ops.nngp.bf_sweep_mv(cd, nbr, None, 0, ops.kind_code(cov.kind), flat, cov.phi, cov.tau2, vd, True)
    assert all(torch.equal(x, y) for x, y in zip(a, t))
    qd = dev(coords[:9] + 0.01)[0]
    nq = _lib.knn_query(cd, qd, m)
    c1 = _lib.bf_cross_mv(cd, qd, nq, cov.kind, cov.A, cov.phi, cov.tau2, vd, target_noise=False)
    c2 = torch.ops.nngp.bf_cross_mv(cd, qd, nq, ops.kind_code(cov.kind), flat, cov.phi, cov.tau2, False, vd)
    assert all(torch.equal(x, y) for x, y in zip(c1[:3], c2))


def test_flags():
    q, m = 2, 8
    coords, vals = inputs(q)
    cd, vd = dev(coords, vals)
    nbr = _lib.knn_prior(cd, m)
    nbr[40, 3] = N + 7  # out of range: flagged, masked like -1
    cov = model(q)
    B, LF, E, p = _lib.bf_sweep_mv(cd, nbr, 0, cov.kind, cov.A, cov.phi, cov.tau2, vd)
    assert p[3] == 40 and p[2] == -1 and all(bool(torch.isfinite(x).all()) for x in (B, LF, E, p))
    assert torch.all(B[40][:, 3 * q:4 * q] == 0)
    check((B, LF, E, torch.tensor(p.tolist()[:2] + [-1.0, -1.0], dtype=torch.float64)), reference(cov, coords, nbr.cpu().numpy(), vals))
    coords[50] = coords[51]  # two coincident neighbours without a nugget: a zero pivot at the rows that hold both
    cd = dev(coords)[0]
    nbr = _lib.knn_prior(cd, m)
    cov = model(q, tau2=[0.0, 0.0])
    B, LF, E, p = _lib.bf_sweep_mv(cd, nbr, 0, cov.kind, cov.A, cov.phi, cov.tau2, vd)
    both = ((nbr == 50).any(1) & (nbr == 51).any(1)).cpu().numpy()
    both[51] = True  # row 51 has point 50 among its neighbours
    assert both.sum() > 1 and p[2] == np.nonzero(both)[0][0] and p[3] == -1
    for x in (B, LF, E):
        bad = torch.isnan(x).reshape(N, -1)
        assert bool(bad[both].all()) and not bool(bad[~both].any())


def test_end_to_end():
    q, m = 3, 10
    cov = model(q, "matern32")
    coords, vals = inputs(q, 2, 1)
    Y = vals[:, :, 0] + np.array([1.0, -2.0, 0.5])
    g = A.MultivariateNNGP(coords, Y, m, cov)
    nbr = g._nbr.cpu().numpy()
    ll, mu = g.loglik(mean="constant")
    X = np.zeros((N, q, q))
    X[:, np.arange(q), np.arange(q)] = 1.0
    _, _, Er, ld, _ = reference(cov, coords, nbr, np.concatenate([Y[:, :, None], X], axis=2))
    Er = Er.reshape(N * q, 1 + q)
    mur = np.linalg.lstsq(Er[:, 1:], Er[:, 0], rcond=None)[0]
    llr = -0.5 * (N * q * np.log(2 * np.pi) + ld.sum() + ((Er[:, 0] - Er[:, 1:] @ mur) ** 2).sum())
    assert np.allclose(mu, mur, rtol=1e-9, atol=1e-9) and abs(ll - llr) <= 1e-10 * abs(llr)
    assert g.B.shape == (N, q, m * q) and g.LF.shape == (N, q, q)
    query = np.random.default_rng(2).uniform(0.0, 1.0, (20, 2))
    pm, pc = g.predict(query, noise=False)
    qn = _lib.knn_query(*dev(coords, query), m).cpu().numpy()
    _, Fr, mr, _, _ = reference(cov, coords, qn, Y[:, :, None], query, noise=False)
    assert np.allclose(pm, mr[:, :, 0], rtol=1e-9, atol=1e-9) and np.allclose(pc, Fr, rtol=1e-9, atol=1e-12)


def test_fit_recovers_the_likelihood():
    rng = np.random.default_rng(4)
    coords = rng.uniform(0.0, 1.0, (1500, 2))
    truth = A.LMCCovariance("exponential", AFULL[:2, :2], [6.0, 12.0], [0.1, 0.2])
    g = A.MultivariateNNGP(coords, np.zeros((1500, 2)), 8, truth)
    g.Y = g.simulate(seed=5)
    start = truth.replace(A=[[0.7, 0.0], [0.2, 1.2]], phi=[9.0, 8.0], tau2=[0.2, 0.1])
    fitted = g.fit(start=start, maxiter=60)
    assert g.loglik(fitted) >= g.loglik(truth) > g.loglik(start)
