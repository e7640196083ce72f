"""The multivariate gradient sweep (nngp_bf_grad_mv) on the GPU against the dense fp64 reference of
tests/mv_grad_ref.py, on the inputs of tests/test_gpu_mv.py (N = 160, prior sets with -1 padding, cond <= 1e3).
Bounds: every entry of G within 1e-9 (1 + |G_ref|), each of the P sums within 1e-11 sum_rows |row term| (the
project's gradient bounds, tests/test_gpu_nd.py), partials[0:2] within 1e-11 sum |terms| (the sweep's own)."""
import numpy as np
import pytest
import torch

import mv_grad_ref
import pynngp_amd as A
from pynngp_amd import _lib
from test_gpu_mv import AFULL, DEV, KINDS, N, dev, inputs, model

pytestmark = pytest.mark.gpu


def check(got, ref):
    (p, grad, G), (ld, qd, Gr) = [x.cpu().numpy() for x in got], ref
    eg = np.abs(G - Gr) / (1 + np.abs(Gr))
    es = np.abs(grad - Gr.sum(0)) / np.abs(Gr).sum(0)
    ep = max(abs(p[0] - ld.sum()) / np.abs(ld).sum(), abs(p[1] - qd.sum()) / qd.sum())
    print(f"max dG {eg.max():.2e} dsum {es.max():.2e} dpartials {ep:.2e}")
    assert eg.max() <= 1e-9 and es.max() <= 1e-11 and ep <= 1e-11


def run_parity(q, m, kind, dim=2):
    cov = model(q, kind)
    coords, vals = inputs(q, dim)
    cd, vd = dev(coords, vals)
    nbr = _lib.knn_prior(cd, m)
    got = _lib.bf_grad_mv(cd, nbr, 0, kind, cov.A, cov.phi, cov.tau2, vd, want_rows=True)
    assert got[0][2] == -1 and got[0][3] == -1
    check(got, mv_grad_ref.reference(cov, coords, nbr.cpu().numpy(), vals[:, :, 0]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("q,m", [(2, 1), (4, 3), (2, 7), (3, 10), (2, 24), (4, 15), (2, 31)])
def test_grad_parity(q, m, kind):
    run_parity(q, m, kind)


@pytest.mark.parametrize("dim", [1, 3])
def test_grad_parity_dims(dim):
    run_parity(3, 10, "matern32", dim)


def test_determinism_and_flags():
    q, m, cov = 3, 10, model(3)
    coords, vals = inputs(q)
    cd, vd = dev(coords, vals)
    nbr = _lib.knn_prior(cd, m)
    args = (0, cov.kind, cov.A, cov.phi, cov.tau2, vd)
    a = _lib.bf_grad_mv(cd, nbr, *args, want_rows=True)
    assert all(torch.equal(x, y) for x, y in zip(a, _lib.bf_grad_mv(cd, nbr, *args, want_rows=True)))
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(3)).to(DEV)
    o = _lib.bf_grad_mv(cd, nbr[perm].contiguous(), *args, want_rows=True, order=perm.int())
    assert all(torch.equal(x, y) for x, y in zip(a, o))
    ops = A.load_ops()
    flat = [x for row in cov.A for x in row]
    t = torch.ops.nngp.bf_grad_mv(cd, nbr, None, 0, ops.kind_code(cov.kind), flat, cov.phi, cov.tau2, vd, True)
    assert all(torch.equal(x, y) for x, y in zip(a, t))
    # an out-of-range index: flagged, and that row equals the reference with the slot masked
    bad = nbr.clone()
    bad[40, 3] = N + 7
    got = _lib.bf_grad_mv(cd, bad, *args, want_rows=True)
    assert got[0][3] == 40 and got[0][2] == -1
    check(got, mv_grad_ref.reference(cov, coords, bad.cpu().numpy(), vals[:, :, 0]))
    # a coincident pair without a nugget: flagged, exactly those rows NaN
    coords[50] = coords[51]
    cd = dev(coords)[0]
    nbr = _lib.knn_prior(cd, m)
    p, grad, G = _lib.bf_grad_mv(cd, nbr, 0, cov.kind, cov.A, cov.phi, [0.0] * q, vd, want_rows=True)
    both = ((nbr == 50).any(1) & (nbr == 51).any(1)).cpu().numpy()
    both[51] = True  # row 51 has point 50 among its neighbours
    nan = torch.isnan(G).cpu().numpy()
    assert both.sum() > 1 and p[2] == np.nonzero(both)[0][0] and p[3] == -1
    assert nan[both].all() and not nan[~both].any()


def test_python_layer():
    q, m, cov = 3, 10, model(3, "matern32")
    coords, vals = inputs(q)
    g = A.MultivariateNNGP(coords, vals[:, :, 0] + np.array([1.0, -2.0, 0.5]), m, cov)
    theta, low = np.array(cov.theta), np.tril_indices(q)

    def at(th):
        Am = np.zeros((q, q))
        Am[low] = th[:len(low[0])]
        return A.LMCCovariance(cov.kind, Am, th[-2 * q:-q], th[-q:])

    for mean in (None, "constant"):
        value = (lambda c: g.loglik(c)) if mean is None else (lambda c: g.loglik(c, mean)[0])  # noqa: E731
        out = g.loglik_grad(mean=mean)
        assert abs(out[0] - value(cov)) <= 1e-11 * abs(out[0])
        for k in range(len(theta)):
            e = np.zeros_like(theta)
            e[k] = 1e-5 * theta[k]
            fd = (value(at(theta + e)) - value(at(theta - e))) / (2 * e[k])
            assert abs(out[-1][k] - fd) <= 1e-5 * (1 + abs(out[-1][k])), (mean, k, out[-1][k], fd)
    ll, grad = g.loglik_grad()
    At, ph, t2 = [torch.tensor(x, dtype=torch.float64, device=DEV, requires_grad=True) for x in (cov.A, cov.phi, cov.tau2)]
    lt = A.loglik_lmc(g._t_dev, g._nbr, cov.kind, At, ph, t2, torch.as_tensor(g.Y).to(DEV))
    lt.backward()
    auto = torch.cat([At.grad[low[0], low[1]], ph.grad, t2.grad]).cpu().numpy()
    assert abs(lt.item() - ll) <= 1e-13 * abs(ll) and np.array_equal(auto, grad) and bool((At.grad.triu(1) == 0).all())


def test_fit_with_the_gradient():
    rng = np.random.default_rng(4)
    coords = rng.uniform(0.0, 1.0, (1500, 2))
    truth = A.LMCCovariance("exponential", AFULL[:2, :2], [6.0, 12.0], [0.1, 0.2])
    g = A.MultivariateNNGP(coords, np.zeros((1500, 2)), 8, truth)
    g.Y = g.simulate(seed=5)
    start = truth.replace(A=[[0.7, 0.0], [0.2, 1.2]], phi=[9.0, 8.0], tau2=[0.2, 0.1])
    fitted = g.fit(start=start, maxiter=60, gradient=True)
    sweeps = g.fit_sweeps
    assert g.loglik(fitted) >= g.loglik(truth)
    g.fit(start=start, maxiter=60)
    assert sweeps < g.fit_sweeps
