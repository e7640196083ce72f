"""GPU: the general-nu Matern gradient sweep (nngp_bf_grad_matern), its derivative tables (nngp_matern_eval_d) and
everything above them, against tests/grad_matern_ref.py and mpmath.

Per-row tolerance: 1e-9 (1 + |G|) in all four components, the tolerance test_gpu_grad.py applies to bf_grad
against its restatement.  There the restatement's fp64-versus-longdouble disagreement is bounded by 1e-11 (1 + |G|);
test_grad_matern_host.py::test_restatement_against_longdouble_twin bounds this file's reference the same way for
the nu component (measured below 2e-12 on these inputs), so it gets the same multiple, 100.
"""
import mpmath as mp
import numpy as np
import pytest
import torch

import grad_matern_ref as R
from pynngp_amd import _lib

pytestmark = pytest.mark.gpu

# four times the host table fit's measured worst errors (test_grad_matern_host.py): the GPU evaluates the same
# functions with its own libm, so the bound is that of the host table, not a tighter one
BOUND_H, BOUND_N = 4 * 6.4e-15, 4 * 1.4e-14


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sweep(coords, nbr, theta, y, i0=0, order=None, rows=True, workspace=None):
    p, g, G = _lib.bf_grad_matern(dev(coords), dev(nbr), i0, *theta, dev(y), want_rows=rows, order=order,
                                  workspace=workspace)
    torch.cuda.synchronize()
    return p.cpu().numpy(), g.cpu().numpy(), None if G is None else G.cpu().numpy()


def lib_nbr(coords, m):
    from pynngp_amd import load_ops

    load_ops()
    return torch.ops.nngp.knn_prior(dev(coords), m, 0, coords.shape[0]).cpu().numpy()


def close_rows(G, ref):
    err = np.abs(G - ref) / (1 + np.abs(ref))
    print("max |dG| / (1 + |G|) per component =", err.max(0))
    return err.max() <= 1e-9


# ---------------------------------------------------------------- 6. the derivative tables
@pytest.mark.parametrize("nu", [0.3, 0.5, 1.0, 1.3, 2.5, 7.3, 50.0])
def test_matern_eval_d_vs_mpmath(nu):
    u = np.concatenate([[0.0], np.exp(np.random.default_rng(6).uniform(np.log(1e-12), np.log(60.0), 2000))])
    h, n = _lib.matern_eval_d(dev(u), nu)
    h, n = h.cpu().numpy(), n.cpu().numpy()
    assert h[0] == 0.0 and n[0] == 0.0
    mp.mp.dps = 30
    wh = wn = 0.0
    for k in range(1, len(u)):
        wh = max(wh, abs(h[k] - float(R.h_mp(nu, float(u[k])))))
        wn = max(wn, abs(n[k] - R.dnu_mp(nu, float(u[k]))))
    print(nu, "worst |dh|, |dn|:", wh, wn)
    assert wh <= BOUND_H and wn <= BOUND_N, (wh, wn)


# ---------------------------------------------------------------- 7. rows against the host reference
_FIELDS = {}


def parity_case(dim, nu):
    """coords, y, theta and the reference's pair tables, computed once per (dim, nu) and never changed."""
    key = (dim, nu)
    if key not in _FIELDS:
        coords, y = R.field(R.PARITY_N, dim=dim, seed=R.PARITY_SEED)
        th = R.parity_theta(nu, dim)
        _FIELDS[key] = (coords, y, th, R.pair_tables(coords, th), {})
    return _FIELDS[key]


@pytest.mark.parametrize("nu", R.PARITY_NUS)
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_rows_match_reference(dim, nu):
    coords, y, th, T, nbrs = parity_case(dim, nu)
    for m in R.PARITY_MS:
        if m not in nbrs:
            nbrs[m] = lib_nbr(coords, m)
        nbr = nbrs[m]
        ref = R.ref_rows_matern(coords, nbr, th, y, tables=T)
        p, g, G = sweep(coords, nbr, th, y)
        assert p[2] == -1 and p[3] == -1, (m, p)
        assert G.shape == (R.PARITY_N, 4) and close_rows(G, ref[:, 2:]), m
        assert abs(p[0] - ref[:, 0].sum()) <= 1e-11 * np.abs(ref[:, 0]).sum(), m
        assert abs(p[1] - ref[:, 1].sum()) <= 1e-11 * np.abs(ref[:, 1]).sum(), m
        assert np.all(np.abs(g - ref[:, 2:].sum(0)) <= 1e-9 * (1 + np.abs(ref[:, 2:])).sum(0)), m


# ---------------------------------------------------------------- 8. every instantiation
@pytest.fixture(scope="module")
def f64case():
    coords, y = R.field(64, seed=2)
    th = R.parity_theta(1.3)
    return coords, y, th, R.pair_tables(coords, th)


@pytest.mark.parametrize("m", range(1, 33))
def test_every_instantiation(f64case, m):
    coords, y, th, T = f64case
    nbr = lib_nbr(coords, m)
    ref = R.ref_rows_matern(coords, nbr, th, y, tables=T)
    p, g, _ = sweep(coords, nbr, th, y, rows=False)
    assert p[2] == -1 and p[3] == -1
    assert abs(p[0] - ref[:, 0].sum()) <= 1e-11 * np.abs(ref[:, 0]).sum()
    assert abs(p[1] - ref[:, 1].sum()) <= 1e-11 * np.abs(ref[:, 1]).sum()
    assert np.all(np.abs(g - ref[:, 2:].sum(0)) <= 1e-9 * (1 + np.abs(ref[:, 2:])).sum(0))


# ---------------------------------------------------------------- 9. agreement with the fixed kinds
@pytest.mark.parametrize("nu,kind", [(0.5, "exponential"), (1.5, "matern32"), (2.5, "matern52")])
@pytest.mark.parametrize("m", [7, 15, 20])
def test_half_integer_nu_equals_fixed_kinds(nu, kind, m):
    coords, y = R.field(R.PARITY_N, seed=R.PARITY_SEED)
    nbr = lib_nbr(coords, m)
    th = R.parity_theta(nu)
    p, g, G = sweep(coords, nbr, th, y)
    p2, g2, G2 = _lib.bf_grad(dev(coords), dev(nbr), 0, kind, *th[:3], dev(y), want_rows=True)
    p2, g2, G2 = p2.cpu().numpy(), g2.cpu().numpy(), G2.cpu().numpy()
    assert close_rows(G[:, :3], G2)
    assert np.all(np.abs(g[:3] - g2) <= 1e-9 * (1 + np.abs(G2)).sum(0))
    assert abs(p[0] - p2[0]) <= 1e-11 * abs(p2[0]) and abs(p[1] - p2[1]) <= 1e-11 * abs(p2[1])
    assert p[2] == p2[2] == -1 and p[3] == p2[3] == -1


# ---------------------------------------------------------------- 10. masks
def test_masks_padding_and_bad_index():
    coords, y = R.field(96, seed=4)
    th = R.parity_theta(1.3)
    nbr = lib_nbr(coords, 10)  # rows i < m are -1 padded by themselves
    nbr[40, 3:] = -1
    nbr[41, :] = -1
    nbr[42, ::2] = -1
    ref = R.ref_rows_matern(coords, nbr, th, y)
    p, g, G = sweep(coords, nbr, th, y)
    assert p[2] == -1 and p[3] == -1 and close_rows(G, ref[:, 2:])
    bad = nbr.copy()
    bad[50, 2] = 96  # out of range: flagged, and the slot adds exactly 0
    nbr50 = nbr.copy()
    nbr50[50, 2] = -1
    pb, gb, Gb = sweep(coords, bad, th, y)
    pg, gg, Gg = sweep(coords, nbr50, th, y)
    assert pb[3] == 50 and pg[3] == -1
    assert np.array_equal(Gb, Gg) and np.array_equal(gb, gg)


@pytest.mark.parametrize("nu", [0.3, 1.3])
def test_masks_coincident_points(nu):
    coords, y = R.field(96, seed=4)
    coords[31] = coords[30]
    nbr = lib_nbr(coords, 10)
    assert 30 in nbr[31]
    th = (1.3, 6.0, 0.05, nu)
    ref = R.ref_rows_matern(coords, nbr, th, y)  # h = n = 0 at u = 0 in the reference: D exactly 0
    p, g, G = sweep(coords, nbr, th, y)
    assert p[2] == -1 and np.all(np.isfinite(G)) and close_rows(G, ref[:, 2:])
    p0, g0, G0 = sweep(coords, nbr, (1.3, 6.0, 0.0, nu), y)  # tau2 = 0: the joint block is singular
    assert p0[2] >= 0 and np.all(np.isnan(G0[int(p0[2])]))
    assert np.all(np.isnan(G0[31])) or np.all(np.isnan(G0[[r for r in range(96) if 30 in nbr[r] and 31 in nbr[r]][0]]))


def test_row_order():
    coords, y = R.field(R.PARITY_N, seed=R.PARITY_SEED)
    th = R.parity_theta(1.3)
    nbr = lib_nbr(coords, 15)
    order, nbr_sorted = _lib.row_order(dev(coords), 0, R.PARITY_N, dev(nbr))
    p, g, G = sweep(coords, nbr, th, y)
    p2, g2, G2 = _lib.bf_grad_matern(dev(coords), nbr_sorted, 0, *th, dev(y), want_rows=True, order=order)
    G2 = G2.cpu().numpy()
    assert np.all(np.abs(G - G2) <= 1e-12 * (1 + np.abs(G)))
    assert np.all(np.abs(g - g2.cpu().numpy()) <= 1e-12 * np.abs(G).sum(0))


# ---------------------------------------------------------------- 11. reproducibility
def test_reproducible_and_workspace_reuse():
    coords, y = R.field(R.PARITY_N, seed=R.PARITY_SEED)
    nbr = lib_nbr(coords, 15)
    th = R.parity_theta(1.3)
    a, b = sweep(coords, nbr, th, y), sweep(coords, nbr, th, y)
    for x, z in zip(a, b):
        assert np.array_equal(x, z)
    p, g, G = a
    assert np.all(np.abs(G.sum(0) - g) <= 1e-12 * np.abs(G).sum(0))
    need = _lib.load().nngp_bf_grad_matern_workspace_bytes(R.PARITY_N, 15)
    ws = _lib._workspace(need, torch.device("cuda", torch.cuda.current_device()))
    for nu in (0.7, 2.2, 0.7, 2.2):  # one workspace across alternating nu: no stale table
        t = (1.3, 6.0, 0.05, nu)
        fresh, reused = sweep(coords, nbr, t, y), sweep(coords, nbr, t, y, workspace=ws)
        for x, z in zip(fresh, reused):
            assert np.array_equal(x, z), nu


# ---------------------------------------------------------------- 12, 13. forward bits, autograd, methods
@pytest.fixture(scope="module")
def model():
    from pynngp_amd import Covariance, MaternCovariance, NNGP

    coords, y = R.field(600, seed=8)
    mdl = NNGP(coords, y, None, "S=T", 10, Covariance("matern", 1.0, 8.0, 0.1, nu=1.3), device="cuda")
    return mdl, coords, y, Covariance, MaternCovariance


def test_forward_bits_unchanged(model):
    mdl, coords, y, Covariance, MaternCovariance = model
    a = mdl.loglik(cov=MaternCovariance(1.0, 8.0, 0.1, 1.3))
    b = mdl.loglik(cov=Covariance("matern", 1.0, 8.0, 0.1, nu=1.3))
    assert a == b


def test_autograd_and_methods(model):
    import pynngp_amd

    mdl, coords, y, Covariance, MaternCovariance = model
    th = (1.0, 8.0, 0.1, 1.3)
    cv = MaternCovariance(*th)
    ll, g = mdl.loglik_grad(cov=cv)
    assert g.shape == (4,) and abs(ll - mdl.loglik(cov=cv)) <= 1e-11 * abs(ll)
    with pytest.raises(NotImplementedError):
        mdl.loglik_grad(cov=Covariance("matern", 1.0, 8.0, 0.1, nu=1.3))
    nbr = lib_nbr(coords, 10)
    p, gop, _ = sweep(coords, nbr, th, y, rows=False)
    t = torch.tensor(th, dtype=torch.float64, requires_grad=True)
    l2 = pynngp_amd.loglik_matern(dev(coords), dev(nbr), t, dev(y))
    l2.backward()
    assert np.array_equal(t.grad.numpy(), gop)
    for mean, X in (("zero", None), ("constant", None), ("linear", np.stack([np.ones(600), coords[:, 0]], 1))):
        pl, _, pg = mdl.profile_loglik_grad(cv, mean=mean, X=X)
        assert pg.shape == (4,)
        for k in range(4):
            h = 1e-6 * th[k]
            tp, tm = list(th), list(th)
            tp[k] += h
            tm[k] -= h
            fp = mdl.profile_loglik(MaternCovariance(*tp), mean=mean, X=X)[0]
            fm = mdl.profile_loglik(MaternCovariance(*tm), mean=mean, X=X)[0]
            fd = (fp - fm) / (2 * h)
            assert abs(fd - pg[k]) <= 1e-5 * max(1.0, abs(pg[k])), (mean, k, fd, pg[k])


# ---------------------------------------------------------------- 14. fit
def test_fit_estimate_nu():
    """N = 2,000, m = 10, y simulated at (1, 12, 0.05, nu = 1.5).  Sweeps are counted from the objective
    evaluations (n_evals, as test_gpu_fisher.py reports them): two forward sweeps each for the profiled mean, plus
    one gradient sweep where there is a gradient.
    nu-hat itself is not asserted: the data at this size do not pin it tighter than the likelihood comparisons."""
    from pynngp_amd import Covariance, NNGP

    coords = np.random.default_rng(21).uniform(0, 1, (2000, 2))
    mdl = NNGP(coords, np.zeros(2000), None, "S=T", 10, Covariance("matern", 1.0, 12.0, 0.05, nu=1.5), device="cuda")
    y = np.asarray(mdl.simulate(1, seed=3)[0], dtype=np.float64)
    x0 = (0.8, 8.0, 0.1)

    def fresh():
        return NNGP(coords, y, None, "S=T", 10, Covariance("matern", *x0, nu=1.5), device="cuda")

    nm = {nu: fresh().fit(kind="matern", nu=nu, x0=x0) for nu in (0.5, 1.5, 2.5)}
    est = fresh().fit(kind="matern", nu=0.8, x0=x0, estimate_nu=True, tol=1e-3)
    print("estimate_nu:", est["theta"], est["loglik"], est["n_evals"], est["message"], est["grad"])
    # the gradient rule as test_gpu_grad_aniso.py::test_fit_anisotropic holds it: tol = L-BFGS-B's gtol = 1e-3
    assert est["converged"] and "PROJECTED GRADIENT" in est["message"] and np.max(np.abs(est["grad"])) <= 1e-3
    assert 0.05 <= est["nu"] <= 50.0 and len(est["theta"]) == 4 and est["grad"].shape == (4,)
    for nu, r in nm.items():
        assert est["loglik"] >= r["loglik"] - 1e-6 * abs(r["loglik"]), (nu, est["loglik"], r["loglik"])
    # 3 sweeps per gradient evaluation against 2 per derivative-free evaluation
    assert 3 * est["n_evals"] < 2 * nm[1.5]["n_evals"], (est["n_evals"], nm[1.5]["n_evals"])
    fix = fresh().fit(kind="matern", nu=1.5, x0=x0, estimate_nu=False)
    assert fix["nu"] == 1.5 and fix["grad"].shape == (3,)
    assert abs(fix["loglik"] - nm[1.5]["loglik"]) <= 1e-6 * abs(nm[1.5]["loglik"])
