"""The packed-row multivariate gradient sweep (nngp_bf_grad_mv_obs) on the GPU against the dense fp64
reference of tests/mv_obs_grad_ref.py, on the inputs, masks and cut neighbour sets of tests/test_gpu_mv_obs.py (N = 160).
Bounds (tests/test_gpu_mv_grad.py's): every entry of G within 1e-9 (1 + |G_ref|), each of the P sums within
1e-11 sum_rows |row term|, partials[0:2] within 1e-11 sum |terms|."""
import numpy as np
import pytest
import torch

import mv_obs_grad_ref
import pynngp_amd as A
from pynngp_amd import _lib
from test_gpu_mv_obs import AFULL, DEV, N, bits, dev, inputs, masks, model, rows_of, setup

pytestmark = pytest.mark.gpu


def check(got, ref):
    (p, grad, G), (ld, qd, Gr) = [x.cpu().numpy() for x in got], ref
    tot = np.abs(Gr).sum(0)
    eg = np.abs(G - Gr) / (1 + np.abs(Gr))
    ds, dp = np.abs(grad - Gr.sum(0)), np.array([abs(p[0] - ld.sum()), abs(p[1] - qd.sum())])
    tp = np.array([np.abs(ld).sum(), qd.sum()])
    print(f"max dG {eg.max():.2e} dsum {(ds / np.where(tot > 0, tot, 1)).max():.2e} dpartials {(dp / tp).max():.2e}")
    assert eg.max() <= 1e-9 and np.all(ds <= 1e-11 * tot) and np.all(dp <= 1e-11 * tp)


def rare_setup(q, m):
    """Outcome 0 at every eighth site and nothing elsewhere: one tile of packed rows under up to 496 point pairs."""
    coords, vals = inputs(q, 2, 1)
    obs = (np.arange(N) % 8 == 0).astype(np.uint8)
    vals[~bits(obs, q)] = np.nan
    nbr = _lib.knn_prior(dev(coords)[0], m).cpu().numpy()
    rows_max = int(rows_of(nbr, obs, q).max())
    assert 1 <= rows_max <= 16
    return coords, vals, obs, nbr, rows_max, dev(coords, vals, obs, nbr)


SHAPES = [(2, 1, "cyc"), (4, 7, "cyc"), (3, 10, "cyc0"), (3, 20, "cyc"), (2, 40, "sparse"), (4, 15, "full"),
          (4, 30, "rare")]
CASES = [(q, m, pat, "exponential", 2) for q, m, pat in SHAPES] + \
        [(3, 10, "cyc0", kind, 2) for kind in ("matern32", "matern52", "gaussian")] + \
        [(3, 10, "cyc", "exponential", 1), (3, 10, "cyc", "exponential", 3)]


@pytest.mark.parametrize("q,m,pattern,kind,dim", CASES)
def test_grad_parity(q, m, pattern, kind, dim):
    cov = model(q, kind)
    coords, vals, obs, nbr, rows_max, (cd, vd, od, nd) = \
        rare_setup(q, m) if pattern == "rare" else setup(q, m, pattern, dim, c=1)
    got = _lib.bf_grad_mv_obs(cd, nd, 0, kind, cov.A, cov.phi, cov.tau2, od, rows_max, vd, want_rows=True)
    assert got[0][2] == -1 and got[0][3] == -1
    check(got, mv_obs_grad_ref.reference(cov, coords, nbr, vals[:, :, 0], bits(obs, q)))


def test_determinism_and_flags():
    q, m, cov = 3, 10, model(3)
    coords, vals, obs, nbr, rows_max, (cd, vd, od, nd) = setup(q, m, "cyc", c=1)
    args = (cov.kind, cov.A, cov.phi, cov.tau2, od, rows_max, vd)
    a = _lib.bf_grad_mv_obs(cd, nd, 0, *args, want_rows=True)
    assert all(torch.equal(x, y) for x, y in zip(a, _lib.bf_grad_mv_obs(cd, nd, 0, *args, want_rows=True)))
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(3)).to(DEV)
    o = _lib.bf_grad_mv_obs(cd, nd[perm].contiguous(), 0, *args, want_rows=True, order=perm.int())
    assert all(torch.equal(x, y) for x, y in zip(a, o))
    ops = A.load_ops()
    flat, code = [x for row in cov.A for x in row], ops.kind_code(cov.kind)
    t = torch.ops.nngp.bf_grad_mv_obs(cd, nd, None, 0, code, flat, cov.phi, cov.tau2, vd, od, rows_max, True)
    assert all(torch.equal(x, y) for x, y in zip(a, t))
    # a bound of 16 rows (one tile) where locations carry more: flagged, and equal to the reference on the kept prefix
    ob = bits(obs, q)
    run = np.cumsum(ob.sum(1)[np.clip(nbr, 0, N - 1)] * (nbr >= 0), axis=1)
    over = np.nonzero(run[:, -1] > 16)[0]
    assert rows_max > 16 and len(over) > 1
    got = _lib.bf_grad_mv_obs(cd, nd, 0, *args[:4], od, 16, vd, want_rows=True)
    assert got[0][3] == over[0] and got[0][2] == -1
    check(got, mv_obs_grad_ref.reference(cov, coords, np.where(run <= 16, nbr, -1), vals[:, :, 0], ob))
    # a coincident pair that shares outcome 1, without a nugget: flagged, exactly those rows NaN
    assert ob[50, 1] and ob[51, 1]
    coords[50] = coords[51]
    cd = dev(coords)[0]
    nb = _lib.knn_prior(cd, m)
    rows_max = int(_lib.mv_obs_rows(nb, od).max())
    assert rows_max <= 64
    p, grad, G = _lib.bf_grad_mv_obs(cd, nb, 0, cov.kind, cov.A, cov.phi, [0.0] * q, od, rows_max, vd, want_rows=True)
    both = ((nb == 50).any(1) & (nb == 51).any(1)).cpu().numpy()
    both[51] = True  # row 51 has point 50 among its neighbours
    nan = torch.isnan(G).cpu().numpy()
    assert both.sum() > 1 and p[2] == np.nonzero(both)[0][0] and p[3] == -1
    assert nan[both].all() and not nan[~both].any()


def test_python_layer():
    q, m, cov = 3, 10, model(3, "matern32")
    coords, vals = inputs(q, 2, 1)
    ob = bits(masks("cyc", q), q)
    g = A.MultivariateNNGP(coords, np.where(ob, vals[:, :, 0] + np.array([1.0, -2.0, 0.5]), np.nan), m, cov)
    theta, low = np.array(cov.theta), np.tril_indices(q)

    def at(th):
        Am = np.zeros((q, q))
        Am[low] = th[:len(low[0])]
        return A.LMCCovariance(cov.kind, Am, th[-2 * q:-q], th[-q:])

    for mean in (None, "constant"):
        value = (lambda c: g.loglik(c)) if mean is None else (lambda c: g.loglik(c, mean)[0])  # noqa: E731
        out = g.loglik_grad(mean=mean, missing="packed")
        assert abs(out[0] - value(cov)) <= 1e-11 * abs(out[0])
        for k in range(len(theta)):
            e = np.zeros_like(theta)
            e[k] = 1e-5 * theta[k]
            fd = (value(at(theta + e)) - value(at(theta - e))) / (2 * e[k])
            assert abs(out[-1][k] - fd) <= 1e-5 * (1 + abs(out[-1][k])), (mean, k, out[-1][k], fd)
    ll, grad = g.loglik_grad(missing="packed")
    At, ph, t2 = [torch.tensor(x, dtype=torch.float64, device=DEV, requires_grad=True) for x in (cov.A, cov.phi, cov.tau2)]
    lt = A.loglik_lmc(g._t_dev, g._nbr, cov.kind, At, ph, t2, torch.as_tensor(g.Y).to(DEV))
    lt.backward()
    auto = torch.cat([At.grad[low[0], low[1]], ph.grad, t2.grad]).cpu().numpy()
    assert abs(lt.item() - ll) <= 1e-13 * abs(ll) and np.array_equal(auto, grad) and bool((At.grad.triu(1) == 0).all())


def test_fit_with_the_gradient():
    rng = np.random.default_rng(4)
    coords = rng.uniform(0.0, 1.0, (1500, 2))
    truth = A.LMCCovariance("exponential", AFULL[:2, :2], [6.0, 12.0], [0.1, 0.2])
    Y = A.MultivariateNNGP(coords, np.zeros((1500, 2)), 8, truth).simulate(seed=5)
    Y[np.arange(1500) % 3 != 0, 1] = np.nan  # the second outcome at every third site only
    g = A.MultivariateNNGP(coords, Y, 8, truth)
    start = truth.replace(A=[[0.7, 0.0], [0.2, 1.2]], phi=[9.0, 8.0], tau2=[0.2, 0.1])
    fitted = g.fit(start=start, maxiter=60, gradient=True)
    sweeps = g.fit_sweeps
    assert g.loglik(fitted) >= g.loglik(truth)
    g.fit(start=start, maxiter=60)
    assert sweeps < g.fit_sweeps
