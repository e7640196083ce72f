"""Per-axis gradient sweep (nngp_bf_grad_aniso) on the GPU against the numpy restatement of grad_aniso_ref.py (pinned on
the host by test_grad_aniso_host.py, which also conditions the 1e-9 (1 + |G|) parity tolerance on these inputs), the
isotropic kernel, and the layers above it up to NNGP.fit(anisotropic=True)."""
import numpy as np
import pytest
import torch

from grad_aniso_ref import PARITY_SEED, field, parity_theta, ref_rows_aniso
from oracle import nngp_oracle as O
from pynngp_amd import _lib
from pynngp_amd import nngp as N

pytestmark = pytest.mark.gpu

M_LIST = list(range(1, 33))  # every instantiation of bf_grad_aniso<M, P>
M_SOME = (10, 17, 24, 32)    # every lane-group width from 4 up


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sweep(coords, nbr, kind, theta, y, i0=0, order=None, rows=True):
    p, g, G = _lib.bf_grad_aniso(dev(coords), dev(nbr), i0, kind, theta[0], theta[1:-1], theta[-1], dev(y),
                                 order=order, want_rows=rows)
    torch.cuda.synchronize()
    return p.cpu().numpy(), g.cpu().numpy(), None if G is None else G.cpu().numpy()


def check_rows(coords, nbr, kind, th, y, tag):
    ref = ref_rows_aniso(coords, nbr, kind, th, y)
    p, g, G = sweep(coords, nbr, kind, th, y)
    assert p[2] == -1 and p[3] == -1, tag
    assert G.shape == ref[:, 2:].shape
    err = np.abs(G - ref[:, 2:]) / (1 + np.abs(ref[:, 2:]))
    print(tag, "max |dG| / (1 + |G|) =", err.max())
    assert err.max() <= 1e-9, tag
    assert abs(p[0] - ref[:, 0].sum()) <= 1e-11 * np.abs(ref[:, 0]).sum(), tag
    assert abs(p[1] - ref[:, 1].sum()) <= 1e-11 * np.abs(ref[:, 1]).sum(), tag
    return ref, p, g, G


@pytest.fixture(scope="module")
def f96():
    cache = {}

    def get(dim, th, m):
        key = (dim, tuple(th[1:-1]), m)
        if key not in cache:
            coords, y = field(96, dim=dim, seed=PARITY_SEED)
            cache[key] = (coords, y, O.c_knn_prior(coords * np.array(th[1:-1]), m))
        return cache[key]

    return get


# ---------------------------------------------------------------- per-row parity
@pytest.mark.parametrize("m", M_LIST)
@pytest.mark.parametrize("kind", ["exponential", "matern52"])
def test_rows_every_m(f96, kind, m):
    th = parity_theta(kind)
    coords, y, nbr = f96(2, th, m)
    check_rows(coords, nbr, kind, th, y, (kind, m))


@pytest.mark.parametrize("kind", ["exponential", "matern32", "matern52", "gaussian", "spherical"])
def test_rows_every_kind(f96, kind):
    th = parity_theta(kind)
    for m in M_SOME:
        coords, y, nbr = f96(2, th, m)
        check_rows(coords, nbr, kind, th, y, (kind, m))


def test_rows_spherical_beyond_range(f96):
    th = (1.3, 3.0, 9.0, 0.05)  # ranges 1/3 and 1/9 on the unit square
    for m in M_SOME:
        coords, y, nbr = f96(2, th, m)
        X = coords * np.array(th[1:-1])
        far = 0
        for i in range(1, 96):
            idx = [j for j in nbr[i] if j >= 0] + [i]
            u = np.sqrt(((X[idx][:, None, :] - X[idx][None, :, :]) ** 2).sum(-1))
            far += int((u > 1).sum())
        assert far > 0  # some pairs of the joint blocks lie beyond u = 1
        check_rows(coords, nbr, "spherical", th, y, ("spherical-far", m))


@pytest.mark.parametrize("dim,th", [(1, (1.3, 5.0, 0.05)), (3, (1.3, 3.0, 9.0, 0.7, 0.05))])
def test_rows_dimensions(f96, dim, th):
    for m in M_SOME:
        coords, y, nbr = f96(dim, th, m)
        for kind in ("exponential", "matern52"):
            check_rows(coords, nbr, kind, th, y, (dim, kind, m))


# ---------------------------------------------------------------- the isotropic kernel
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_equal_phi_agrees_with_bf_grad(dim):
    coords, y = field(96, dim=dim, seed=2)
    phi = 6.0
    for m in M_SOME:
        nbr = O.c_knn_prior(coords, m)
        for kind in ("exponential", "matern32", "gaussian"):
            th = (1.3,) + (phi,) * dim + (0.05,)
            p, g, G = sweep(coords, nbr, kind, th, y)
            pi, gi, Gi = _lib.bf_grad(dev(coords), dev(nbr), 0, kind, 1.3, phi, 0.05, dev(y), want_rows=True)
            pi, gi, Gi = pi.cpu().numpy(), gi.cpu().numpy(), Gi.cpu().numpy()
            S = np.abs(Gi).sum(0)
            euler = float(np.dot(th[1:-1], g[1:-1]))
            assert abs(euler - phi * gi[1]) <= 1e-12 * phi * S[1], (dim, m, kind)
            assert abs(g[0] - gi[0]) <= 1e-12 * S[0] and abs(g[-1] - gi[2]) <= 1e-12 * S[2], (dim, m, kind)
            assert p[2] == -1 and p[3] == -1
            assert abs(p[0] - pi[0]) <= 1e-12 * max(1.0, abs(pi[0])) and abs(p[1] - pi[1]) <= 1e-12 * abs(pi[1])


# ---------------------------------------------------------------- masks
def test_padded_rows_and_duplicate_location():
    coords, y = field(96, seed=1)
    coords[50] = coords[49]  # x == 0 between them; the nugget keeps the block positive definite
    th = (1.3, 3.0, 9.0, 0.05)
    for m in (5, 10, 17):
        nbr = O.c_knn_prior(coords * np.array(th[1:-1]), m)
        assert (nbr[:m] == -1).any() and 49 in nbr[50]
        ref, p, g, G = check_rows(coords, nbr, "exponential", th, y, ("pad-dup", m))
        assert np.all(np.isfinite(G))


def test_bad_index_flag(f96):
    th = parity_theta("exponential")
    coords, y, ok = f96(2, th, 10)
    nbr = ok.copy()
    nbr[60, 3] = 96  # one past the end
    p, g, G = sweep(coords, nbr, "exponential", th, y)
    assert p[3] == 60 and p[2] == -1
    assert np.all(np.isfinite(G))
    ref = ref_rows_aniso(coords, ok, "exponential", th, y)
    keep = np.arange(96) != 60
    assert np.max(np.abs(G[keep] - ref[keep, 2:]) / (1 + np.abs(ref[keep, 2:]))) <= 1e-9
    # the slot adds exactly 0: row 60 is the row of the set without that neighbour
    drop = ok.copy()
    drop[60, 3] = -1
    _, _, Gd = sweep(coords, drop, "exponential", th, y)
    assert np.array_equal(G[60], Gd[60])


def test_not_pd_rows_are_nan():
    coords, y = field(96, seed=1)
    # no nugget and 17 coincident locations: every joint block that holds several of them is singular to rounding.
    # One duplicate alone may pass (a pivot of 2^-52 instead of 0); with this many, in the sets of every later
    # location too, some elimination step rounds to a pivot that is not above 0
    coords[40:57] = coords[40]
    th = (1.0, 3.0, 9.0, 0.0)
    nbr = O.c_knn_prior(coords * np.array(th[1:-1]), 16)
    assert sorted(nbr[56]) == list(range(40, 56))
    p, g, G = sweep(coords, nbr, "exponential", th, y)
    assert p[2] >= 41 and p[3] == -1  # some row with coincident neighbours; none before them
    assert np.all(np.isnan(G[int(p[2])]))
    assert np.all(np.isfinite(G[:41]))


# ---------------------------------------------------------------- sub-range and visiting order
def test_row_subrange_and_order(f96):
    th = parity_theta("matern32")
    coords, y, nbr = f96(2, th, 10)
    i0, rows = 37, 41
    ref = ref_rows_aniso(coords, nbr, "matern32", th, y, rows=range(i0, i0 + rows))
    sub = np.ascontiguousarray(nbr[i0:i0 + rows])
    p, g, G = sweep(coords, sub, "matern32", th, y, i0=i0)
    assert np.max(np.abs(G - ref[:, 2:]) / (1 + np.abs(ref[:, 2:]))) <= 1e-9
    order, nbr_sorted = _lib.row_order(dev(coords), i0, rows, dev(sub))
    p2, g2, G2 = _lib.bf_grad_aniso(dev(coords), nbr_sorted, i0, "matern32", th[0], th[1:-1], th[-1], dev(y),
                                    order=order, want_rows=True)
    assert np.array_equal(G2.cpu().numpy(), G)  # bit for bit: only the visiting order changes
    for pp, gg in ((p, g), (p2.cpu().numpy(), g2.cpu().numpy())):
        assert pp[2] == -1 and pp[3] == -1
        assert abs(pp[0] - ref[:, 0].sum()) <= 1e-11 * np.abs(ref[:, 0]).sum()
        assert np.all(np.abs(gg - ref[:, 2:].sum(0)) <= 1e-12 * np.abs(ref[:, 2:]).sum(0))


# ---------------------------------------------------------------- reproducibility and the summed gradient
@pytest.fixture(scope="module")
def f2000():
    coords, y = field(2000, seed=5)
    th = (1.0, 8.0, 20.0, 0.1)
    nbr = O.c_knn_prior(coords * np.array(th[1:-1]), 15)
    return coords, y, th, nbr, ref_rows_aniso(coords, nbr, "exponential", th, y)


def test_summed_gradient_and_reproducibility(f2000):
    coords, y, th, nbr, ref = f2000
    p, g, G = sweep(coords, nbr, "exponential", th, y)
    p2, g2, G2 = sweep(coords, nbr, "exponential", th, y)
    assert np.array_equal(g, g2) and np.array_equal(p, p2) and np.array_equal(G, G2)
    tol = 1e-12 * np.abs(ref[:, 2:]).sum(0)
    print("grad err / sum|G| =", np.abs(g - ref[:, 2:].sum(0)) / np.abs(ref[:, 2:]).sum(0))
    assert np.all(np.abs(g - ref[:, 2:].sum(0)) <= tol)


# ---------------------------------------------------------------- forward paths, neighbours, ops
def test_forward_consistency_and_neighbours(f2000):
    coords, y, th, nbr, ref = f2000
    cov = N.AnisotropicCovariance("exponential", th[0], th[1:-1], th[-1])
    model = N.NNGP(coords, y, None, "S=T", 15, cov)
    assert np.array_equal(model.nbr.cpu().numpy(), nbr)  # the existing search on the scaled coordinates
    ll = model.loglik()
    want = O.nngp_loglik(coords * np.array(th[1:-1]), nbr, "exponential", (th[0], 1.0, th[-1]), y)
    assert abs(ll - want) <= 1e-11 * abs(want)
    llg, g = model.loglik_grad()
    assert abs(llg - ll) <= 1e-11 * abs(ll)
    assert g.shape == (4,) and np.all(np.abs(g - ref[:, 2:].sum(0)) <= 1e-12 * np.abs(ref[:, 2:]).sum(0))
    # B, F, a profiled constant mean and a regression mean agree with the same calls on scaled coordinates
    iso = N.NNGP(coords * np.array(th[1:-1]), y, None, "S=T", 15, N.Covariance("exponential", th[0], 1.0, th[-1]))
    # (the two visit the rows in different orders, so sums agree to rounding; smoke()'s tolerances for B and F)
    assert np.allclose(model.B.cpu().numpy(), iso.B.cpu().numpy(), rtol=0, atol=1e-9)
    assert np.allclose(model.F.cpu().numpy(), iso.F.cpu().numpy(), rtol=1e-10, atol=0)
    (la, mua), (li, mui) = model.profile_loglik(cov), iso.profile_loglik(iso.cov)
    assert abs(la - li) <= 1e-11 * abs(li) and abs(mua - mui) <= 1e-9 * (1 + abs(mui))
    X = np.stack([np.ones(2000), coords[:, 0]], 1)
    ga, gi = model.gls(cov, X), iso.gls(iso.cov, X)
    assert abs(ga.loglik - gi.loglik) <= 1e-11 * abs(gi.loglik) and np.allclose(ga.beta, gi.beta, rtol=1e-9, atol=1e-9)
    q = np.random.default_rng(3).uniform(0, 1, (50, 2))
    ma, va = model.predict(values=y, query=q)
    mi, vi = iso.predict(values=y, query=q * np.array(th[1:-1]))
    assert np.allclose(ma, mi, rtol=0, atol=1e-9) and np.allclose(va, vi, rtol=1e-10, atol=0)
    pl, mu, pg = model.profile_loglik_grad(cov)
    for k in range(4):  # the profiled gradient against central differences of the profiled likelihood
        h = 1e-6 * th[k]
        tp, tm = list(th), list(th)
        tp[k] += h
        tm[k] -= h
        fd = (model.profile_loglik(N.AnisotropicCovariance("exponential", tp[0], tp[1:-1], tp[-1]))[0]
              - model.profile_loglik(N.AnisotropicCovariance("exponential", tm[0], tm[1:-1], tm[-1]))[0]) / (2 * h)
        assert abs(fd - pg[k]) <= 1e-5 * max(1.0, abs(pg[k])), (k, fd, pg[k])
    # another metric: the sets follow it and the kept factors are dropped
    other = cov.replace(phi=(20.0, 8.0))
    model.rebuild_neighbors(other)
    assert np.array_equal(model.nbr.cpu().numpy(), O.c_knn_prior(coords * np.array(other.phi), 15))
    assert model._B is None
    model.rebuild_neighbors(N.Covariance("exponential", 1.0, 8.0, 0.1))
    assert np.array_equal(model.nbr.cpu().numpy(), O.c_knn_prior(coords, 15))


def test_ops_and_autograd():
    import pynngp_amd

    ops = pynngp_amd.load_ops()
    coords, y = field(300, seed=9)
    th = (1.0, 5.0, 12.0, 0.1)
    nbr = O.c_knn_prior(coords * np.array(th[1:-1]), 10)
    p, g, G = sweep(coords, nbr, "matern32", th, y)
    po, go, Go = torch.ops.nngp.bf_grad_aniso(dev(coords), dev(nbr), None, 0, ops.kind_code("matern32"), th[0],
                                              list(th[1:-1]), th[-1], dev(y), True)
    assert np.array_equal(po.cpu().numpy(), p) and np.array_equal(go.cpu().numpy(), g)
    assert np.array_equal(Go.cpu().numpy(), G)
    with pytest.raises((NotImplementedError, RuntimeError)):  # CPU tensors are refused like the other ops'
        torch.ops.nngp.bf_grad_aniso(torch.from_numpy(coords), torch.from_numpy(nbr), None, 0, 0, th[0],
                                     list(th[1:-1]), th[-1], torch.from_numpy(y), False)
    theta = torch.tensor(th, dtype=torch.float64, requires_grad=True)
    v = dev(y).requires_grad_(True)
    ll = pynngp_amd.loglik(dev(coords), dev(nbr), theta, v, "matern32")
    gt, gv = torch.autograd.grad(2.0 * ll, (theta, v))
    assert np.array_equal(gt.numpy(), 2.0 * g)
    ref = ref_rows_aniso(coords, nbr, "matern32", th, y)
    want = -0.5 * (300 * np.log(2 * np.pi) + ref[:, 0].sum() + ref[:, 1].sum())
    assert abs(ll.item() - want) <= 1e-11 * abs(want)
    # d l / d y from one ordinary sweep on the scaled coordinates: the isotropic path's values there (its scatter
    # adds in no fixed order, so to rounding; test_gpu_grad.py's bound for this gradient)
    vi = dev(y).requires_grad_(True)
    ti = torch.tensor((th[0], 1.0, th[-1]), dtype=torch.float64)
    pynngp_amd.loglik(dev(coords * np.array(th[1:-1])), dev(nbr), ti, vi, "matern32").backward()
    err = (gv - 2.0 * vi.grad).abs() / (1 + (2.0 * vi.grad).abs())
    assert err.max().item() <= 1e-9


# ---------------------------------------------------------------- fit
def test_fit_anisotropic():
    """N = 1500, exponential, phi = (4, 16), sigma2 = 1, tau2 = 0.1, simulated by a dense Cholesky.  The isotropic
    model is nested in the per-axis one (equal phi_k) and the true parameters are one point of it, so on the same
    sets the fit's profiled likelihood is at least either's (measured: -1274.00 against -1356.67 and -1276.39).
    The reported gradient is held to the optimiser's own rule: the fit runs with ``tol=1e-3``, L-BFGS-B's ``gtol``,
    must stop on that rule (measured: "NORM OF PROJECTED GRADIENT <= PGTOL" at max |g| = 5.3e-4), and then no free
    log-parameter's derivative exceeds 1e-3.  With scipy's default gtol = 1e-5 the run ended at the same iterate,
    which that rule cannot have stopped: the relative-decrease rule (ftol = 2.22e-9) ends this problem first, so
    1e-5 is not a tolerance the reported gradient could be held to."""
    rng = np.random.default_rng(21)
    n, m = 1500, 10
    coords = rng.uniform(0.0, 1.0, (n, 2))
    true = N.AnisotropicCovariance("exponential", 1.0, (4.0, 16.0), 0.1)
    K = true(coords, coords) + 0.1 * np.eye(n)
    y = np.linalg.cholesky(K) @ rng.standard_normal(n) + 0.5
    start = N.Covariance("exponential", 0.5, 8.0, 0.3)
    model = N.NNGP(coords, y, None, "S=T", m, start)
    sets = model.nbr.cpu().numpy().copy()
    iso = model.fit(gradient=True)
    ll_iso = model.profile_loglik(N.AnisotropicCovariance("exponential", iso["theta"][0], (iso["theta"][1],) * 2,
                                                          iso["theta"][2]))[0]
    assert abs(ll_iso - iso["loglik"]) <= 1e-11 * abs(ll_iso)  # the nested point is the isotropic optimum itself
    ll_true = model.profile_loglik(true)[0]
    model.cov = start
    res = model.fit(anisotropic=True, tol=1e-3)
    print(res["message"])
    print("iso", iso["theta"], ll_iso, "aniso", res["theta"], res["loglik"], "true", ll_true, "grad", res["grad"])
    assert np.array_equal(model.nbr.cpu().numpy(), sets)  # fixed sets
    assert isinstance(res["phi"], tuple) and len(res["phi"]) == 2 and isinstance(model.cov, N.AnisotropicCovariance)
    assert res["theta"] == (res["sigma2"], *res["phi"], res["tau2"])
    assert res["loglik"] >= ll_iso
    assert res["loglik"] >= ll_true
    assert res["n_grad_evals"] >= 1
    assert res["converged"] and "PROJECTED" in res["message"].upper() and "GRADIENT" in res["message"].upper()
    assert res["grad"].shape == (4,) and np.max(np.abs(res["grad"])) <= 1e-3
    assert res["phi"][1] > res["phi"][0]  # the data's anisotropy is found
    # x0 with one phi per axis and a fixed nugget
    model.cov = start
    fixed = model.fit(anisotropic=True, x0=(0.5, (8.0, 8.0), 0.3), fix_tau2=0.1, maxiter=30)
    assert fixed["tau2"] == 0.1 and len(fixed["grad"]) == 3
    # one further round on the sets of the estimate's own metric
    model.cov = start
    ren = model.fit(anisotropic=True, reneighbor=1)
    assert ren["rounds"] == 2
    assert np.array_equal(model.nbr.cpu().numpy(), O.c_knn_prior(coords * np.array(ren["phi"]), m))
    assert abs(ren["loglik"] - model.profile_loglik(model.cov)[0]) <= 1e-11 * abs(ren["loglik"])
