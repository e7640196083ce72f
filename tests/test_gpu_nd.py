"""Points in 4 .. 16 dimensions on the GPU: nngp_bf_sweep_nd / nngp_bf_cross_nd / nngp_bf_grad_nd against the
long-double forward reference (bf_precision_ref on the scaled coordinates) and grad_aniso_ref.ref_rows_aniso, the torch
ops, and an NNGP over five columns end to end.  tests/test_nd_host.py conditions the tolerances on the same inputs.

Bounds (the family's).  Forward and cross sweeps: bf_precision_ref.check_sweep (BF_K U scale per row on the resolved
rows).  Gradient: every row of G within 1e-9 (1 + |G|) of the restatement, each of the dim + 2 sums within
1e-12 sum |row terms|, partials[0:2] within 1e-11 of sum |terms|."""
import numpy as np
import pytest
import torch

import nd_ref as R
from bf_precision_ref import RESOLVED_SHARE, check_sweep
from oracle import nngp_oracle as O
from pynngp_amd import _lib

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared inputs are read-only


def host(*ts):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def forward(c, nbr, kind, th, y, order=None):
    return host(*_lib.bf_sweep_nd(dev(c), nbr if torch.is_tensor(nbr) else dev(nbr), 0, kind, th[0], th[1:-1], th[-1],
                                  values=dev(y), order=order, want_r=True))


def grad(c, nbr, kind, th, y, order=None):
    return host(*_lib.bf_grad_nd(dev(c), nbr if torch.is_tensor(nbr) else dev(nbr), 0, kind, th[0], th[1:-1], th[-1],
                                 dev(y), want_rows=True, order=order))


def check_grad(ref, p, g, G, where):
    Gr, lf, q = ref[:, 2:], ref[:, 0], ref[:, 1]
    Sm = np.abs(Gr).sum(0)
    err = np.abs(g - Gr.sum(0))
    print(f"{where}: grad err / sum|G| {(err / Sm).max():.3g}, worst row / (1 + |G|) "
          f"{(np.abs(G - Gr) / (1 + np.abs(Gr))).max():.3g}")
    assert p[2] == -1 and p[3] == -1, (where, p)
    assert G.shape == Gr.shape and g.shape == (Gr.shape[1],)
    assert np.all(np.abs(G - Gr) <= 1e-9 * (1 + np.abs(Gr))), (where, "rows")
    assert np.all(err <= 1e-12 * Sm), (where, "sums", err, Sm)
    assert abs(p[0] - lf.sum()) <= 1e-11 * np.abs(lf).sum(), (where, p[0], lf.sum())
    assert abs(p[1] - q.sum()) <= 1e-11 * q.sum(), (where, p[1], q.sum())


@pytest.mark.parametrize("m", R.MS)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("dim", R.DIMS)
def test_sweeps_against_references(dim, kind, m):
    c, y, q, yq = R.field(dim)
    th = R.theta(dim, kind)
    nbr = R.neighbours(dim, kind, m)
    where = f"d{dim} {kind} m{m}"
    ref = R.prior_reference(dim, kind, m)
    assert ref.resolved.mean() >= RESOLVED_SHARE, (where, ref.resolved.mean())
    B, F, Rr, p = forward(c, nbr, kind, th, y)
    print("sweep", where, check_sweep(ref, B, F, Rr, p, "sweep " + where))
    cref = R.cross_reference(dim, kind, m)
    assert cref.resolved.mean() >= RESOLVED_SHARE, (where, cref.resolved.mean())
    got = host(*_lib.bf_cross_nd(dev(c), dev(q), dev(R.cross_neighbours(dim, kind, m)), kind, th[0], th[1:-1], th[-1],
                                 ref_values=dev(y), query_values=dev(yq), want_r=True))
    print("cross", where, check_sweep(cref, *got, "cross " + where))
    check_grad(R.grad_all(dim, kind, m), *grad(c, nbr, kind, th, y), "grad " + where)


@pytest.mark.parametrize("dim,m", [(4, 15), (8, 7), (16, 32), (5, 24)])
def test_bit_identity(dim, m):
    kind = "matern32"
    c = np.random.default_rng(dim).uniform(size=(R.N, dim)) if dim == 5 else R.field(dim)[0]
    y = R.field(4)[1]
    ph = R.phis(8, kind)[:dim] if dim == 5 else R.phis(dim, kind)
    th = (R.SIGMA2, *ph, R.TAU2)
    nbr = O.knn_prior(c * np.array(ph), m).astype(np.int32)
    a, b = forward(c, nbr, kind, th, y), forward(c, nbr, kind, th, y)
    ga, gb = grad(c, nbr, kind, th, y), grad(c, nbr, kind, th, y)
    for u, v in zip(a + ga, b + gb):
        assert np.array_equal(u, v, equal_nan=True)
    # a visiting order: nbr row t is location order[t]; the rows are bit-identical
    perm = np.random.default_rng(1).permutation(R.N).astype(np.int32)
    o = forward(c, nbr[perm], kind, th, y, order=dev(perm))
    go = grad(c, nbr[perm], kind, th, y, order=dev(perm))
    for k in range(3):
        assert np.array_equal(o[k], a[k])
    assert np.array_equal(go[2], ga[2])
    assert abs(o[3][0] - a[3][0]) <= 1e-12 * np.abs(np.log(a[1])).sum()


def test_isotropic_covariance_is_all_equal_decays():
    """All-equal phi on dim 4 and Covariance's isotropic path through NNGP run the same kernel: the same bits."""
    import pynngp_amd as A

    c, y = R.field(4)[:2]
    iso = A.Covariance("matern52", 1.3, 2.2, 0.05)
    ard = A.ARDCovariance("matern52", 1.3, (2.2,) * 4, 0.05)
    a, b = A.NNGP(c, y, None, "S=T", 10, iso), A.NNGP(c, y, None, "S=T", 10, ard)
    assert isinstance(a, A.NNGPnd) and torch.equal(a.nbr, b.nbr)
    assert a.loglik() == b.loglik()
    assert torch.equal(a.B, b.B) and torch.equal(a.F, b.F)
    (la, ga), (lb, gb) = a.loglik_grad(), b.loglik_grad()
    assert la == lb and ga.shape == (3,) and gb.shape == (6,)
    assert ga[0] == gb[0] and ga[2] == gb[5] and ga[1] == gb[1:5].sum()


def test_flags():
    c, y = R.field(8)[:2]
    kind, m = "exponential", 9
    th = R.theta(8, kind)
    nbr = np.array(R.neighbours(8, kind, m))
    nbr[100, 3] = R.N + 5  # out of range: flagged, masked, every row finite
    B, F, Rr, p = forward(c, nbr, kind, th, y)
    assert p[3] == 100 and p[2] == -1 and np.all(np.isfinite(B)) and np.all(np.isfinite(F)) and B[100, 3] == 0.0
    pg, g, G = grad(c, nbr, kind, th, y)
    assert pg[3] == 100 and np.all(np.isfinite(G))
    # coincident neighbours without a nugget: the pivot is flagged, that row is NaN, the others are not
    c2 = np.array(c)
    nb = np.array(R.neighbours(8, kind, m))
    c2[nb[200, 1]] = c2[nb[200, 0]]
    th0 = (*th[:-1], 0.0)
    B, F, Rr, p = forward(c2, nb, kind, th0, y)
    # no row before the later of the two points can hold both (that point's own row can: itself and its neighbour)
    first = int(max(nb[200, 0], nb[200, 1]))
    assert p[2] >= first and np.isnan(F[int(p[2])]) and np.isnan(F[200]) and np.isfinite(F[:first]).all()
    pg, g, G = grad(c2, nb, kind, th0, y)
    assert pg[2] >= 0 and np.isnan(G[200]).all()


def test_ops_and_autograd():
    from pynngp_amd import load_ops, loglik_ard

    load_ops()
    dim, kind, m = 8, "gaussian", 15
    c, y, q, _ = R.field(dim)
    th = R.theta(dim, kind)
    nbr = dev(R.neighbours(dim, kind, m))
    code = _lib.KIND_CODES[kind]
    B, F, Rr, p = forward(c, nbr, kind, th, y)
    oB, oF, oR, op = host(*torch.ops.nngp.bf_sweep_nd(dev(c), nbr, None, 0, code, th[0], list(th[1:-1]), th[-1], dev(y),
                                                     True))
    assert np.array_equal(oB, B) and np.array_equal(oF, F) and np.array_equal(oR, Rr) and np.array_equal(op, p)
    pg, g, G = grad(c, nbr, kind, th, y)
    o = host(*torch.ops.nngp.bf_grad_nd(dev(c), nbr, None, 0, code, th[0], list(th[1:-1]), th[-1], dev(y), True))
    assert np.array_equal(o[0], pg) and np.array_equal(o[1], g) and np.array_equal(o[2], G)
    cn = dev(R.cross_neighbours(dim, kind, m))
    cB, cF, cR, _ = host(*_lib.bf_cross_nd(dev(c), dev(q), cn, kind, th[0], th[1:-1], th[-1], ref_values=dev(y),
                                           want_r=True))
    oB, oF, mean = host(*torch.ops.nngp.bf_cross_nd(dev(c), dev(q), cn, code, th[0], list(th[1:-1]), th[-1], dev(y)))
    assert np.array_equal(oB, cB) and np.array_equal(oF, cF) and np.array_equal(mean, -cR)
    theta = torch.tensor(th, dtype=torch.float64, requires_grad=True)
    ll = loglik_ard(dev(c), nbr, kind, theta, dev(y))
    ll.backward()
    assert float(ll) == -0.5 * (R.N * np.log(2 * np.pi) + pg[0] + pg[1])
    assert np.array_equal(theta.grad.numpy(), g)


@pytest.fixture(scope="module")
def model():
    import pynngp_amd as A

    rng = np.random.default_rng(77)
    n, dim, m = 1500, 5, 10
    t = rng.uniform(size=(n, dim))
    true = A.ARDCovariance("exponential", 1.0, (3.0, 0.4, 1.2, 0.8, 2.0), 0.1)
    # a draw from the model's own NNGP (sequential, from the oracle's factors)
    nbr = O.knn_prior(t * np.array(true.phi), m).astype(np.int32)
    B, F, _ = O.bf_sweep(t * np.array(true.phi), nbr, "exponential", (1.0, 1.0, 0.1))
    z = rng.standard_normal(n)
    y = np.zeros(n)
    for i in range(n):
        k = min(i, m)
        y[i] = B[i, :k] @ y[nbr[i, :k]] + np.sqrt(F[i]) * z[i]
    return A, t, y + 0.7, true, nbr, m


def test_nngp_end_to_end(model):
    A, t, y, true, nbr, m = model
    phi = np.array(true.phi)
    mod = A.NNGP(t, y, None, "S=T", m, true)
    assert isinstance(mod, A.NNGPnd)
    assert np.array_equal(mod.nbr.cpu().numpy(), nbr)
    assert np.allclose(mod.ws, O.ws_init(t, y, t), rtol=1e-13, atol=0)
    want = O.nngp_loglik(t * phi, nbr, "exponential", (1.0, 1.0, 0.1), y)
    got = mod.loglik()
    assert abs(got - want) <= 1e-11 * abs(want), (got, want)
    B, F, _ = O.bf_sweep(t * phi, nbr, "exponential", (1.0, 1.0, 0.1))
    assert np.allclose(mod.B.cpu().numpy(), B, rtol=0, atol=1e-11) and np.allclose(mod.F.cpu().numpy(), F, rtol=1e-11)
    # predict(query=): dense kriging from the same neighbour sets
    q = np.random.default_rng(5).uniform(size=(40, 5))
    mean, var = mod.predict(values=y, query=q)
    qn = O.knn_all(q * phi, t * phi, m)
    for i in range(40):
        X = t[qn[i]]
        CN = true(X, X) + 0.1 * np.eye(m)
        cv = true(q[i:i + 1], X)[0]
        b = np.linalg.solve(CN, cv)
        assert abs(mean[i] - b @ y[qn[i]]) <= 1e-10 * (1 + abs(mean[i]))
        assert abs(var[i] - (1.1 - cv @ b)) <= 1e-10
    # profile likelihood and its gradient against central differences
    ll, mu, g = mod.profile_loglik_grad(true)
    # the GLS mean under the NNGP precision, from the oracle's factors
    ok = nbr >= 0
    res = lambda v: v - np.einsum("ij,ij->i", B, np.where(ok, v[np.where(ok, nbr, 0)], 0.0))  # noqa: E731
    ry, r1 = res(y), res(np.ones_like(y))
    mu_ref = (r1 * ry / F).sum() / (r1 * r1 / F).sum()
    assert g.shape == (7,) and abs(mu - mu_ref) <= 1e-9 * (1 + abs(mu_ref)), (mu, mu_ref)
    for k in (0, 2, 6):
        th = np.array(true.theta)
        h = 1e-5 * th[k]
        lp = mod.profile_loglik(A.ARDCovariance("exponential", *_split(th, k, +h)))[0]
        lm = mod.profile_loglik(A.ARDCovariance("exponential", *_split(th, k, -h)))[0]
        assert abs((lp - lm) / (2 * h) - g[k]) <= 1e-5 * (1 + abs(g[k])), (k, (lp - lm) / (2 * h), g[k])
    # random ordering and an explicit permutation
    r = A.NNGP(t, y, None, "S=T", m, true, ordering="random")
    perm = r.perm.cpu().numpy()
    assert sorted(perm) == list(range(len(y))) and np.array_equal(r.t, t[perm])
    assert np.array_equal(r.nbr.cpu().numpy(), O.knn_prior(t[perm] * phi, m))
    e = A.NNGP(t, y, None, "S=T", m, true, ordering=perm)
    assert e.loglik() == r.loglik()
    with pytest.raises(NotImplementedError, match="maxmin"):
        A.NNGP(t, y, None, "S=T", m, true, ordering="maxmin")


def _split(th, k, h):
    th = np.array(th)
    th[k] += h
    return th[0], tuple(th[1:-1]), th[-1]


def test_fit_beats_derivative_free(model):
    A, t, y, true, nbr, m = model
    start = A.ARDCovariance("exponential", 0.6, (1.5, 0.8, 0.8, 1.5, 1.0), 0.2)
    tol = 1e-3
    a = A.NNGP(t, y, None, "S=T", m, start)
    ra = a.fit(tol=tol, maxiter=300)
    b = A.NNGP(t, y, None, "S=T", m, start)
    rb = b.fit(gradient=False, maxiter=400)
    print(f"analytic gradient: {ra['n_evals']} evaluations, loglik {ra['loglik']:.6f}; derivative-free: "
          f"{rb['n_evals']} evaluations, loglik {rb['loglik']:.6f}; |grad|_inf {np.abs(ra['grad']).max():.3g}")
    assert ra["converged"], ra["message"]
    assert ra["loglik"] >= rb["loglik"] and ra["n_evals"] < rb["n_evals"]
    assert np.abs(ra["grad"]).max() < tol
    assert isinstance(a.cov, A.ARDCovariance) and a.cov.theta == ra["theta"]
    # reneighbor: the sets follow the estimate's metric
    c = A.NNGP(t, y, None, "S=T", m, start)
    rc = c.fit(tol=tol, maxiter=300, reneighbor=1)
    assert rc["rounds"] == 2
    assert np.array_equal(c.nbr.cpu().numpy(), O.knn_prior(t * np.array(c.cov.phi), m))
