"""GPU: the phi-derivative sweep (nngp_bf_dphi), the two-weight row gather (nngp_latent_rows_dot2_batch), the gradient
of the latent marginal likelihood (LatentPosterior.log_marginal_grad) and the gradient fit, against the numpy closed
forms of tests/test_latent_grad_host.py (``host_dphi``, ``dense_grad``), which that file pins against central
differences of the oracle."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch

from oracle import nngp_gibbs_oracle as G
from oracle import nngp_oracle as O
from test_latent_grad_host import DPHI_K, KINDS, dense_grad, host_dphi, resolved

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
SIGMA2, PHI, TAU2 = 1.3, 6.0, 0.25


def _dt(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)


# ---------------------------------------------------------------- 1. dB, dF against host_dphi
@functools.lru_cache(maxsize=None)
def _points(dim):
    rng = np.random.default_rng(300 + dim)
    coords = rng.uniform(size=(300, dim))
    coords.setflags(write=False)
    return coords, rng.permutation(300).astype(np.int32)


DPHI_M = [1, 2, 8, 9, 15, 16, 23, 24, 31, 32]  # both ends of every lane-group width (the inputs DPHI_K was measured on)
# d = 2: every instantiation of bf_dphi, m = 1 .. 32
DPHI_CASES = [(dim, m) for dim in (1, 2, 3) for m in (range(1, 33) if dim == 2 else DPHI_M)]


@pytest.mark.parametrize("dim,m", DPHI_CASES)
def test_dphi_sweep_against_the_closed_form(dev, dim, m):
    """n = 300 uniform points, phi = 6, the five kinds, (sigma2, tau2) = (1, 0) and (1.7, 0.3); the first rows are -1
    padded, row 200 names a point that does not exist, and the rows are visited through an ``order`` permutation.
    Per row |dB - host| <= K U cond(C_N) |C_N^-1| (|D_c| + |D_N| |b|) and |dF - host| <= K U cond(C_N) |D| |u|^2 with K
    = DPHI_K = 224 (tests/test_latent_grad_host.py: 8 x the largest ratio by which the fp64 closed form differs from the
    same formula in np.longdouble on these inputs; measured over DPHI_M, and the other m of d = 2 give no larger ratio:
``dphi_precision_ratios`` there returns at most 23.1 (dB) and 1.41 (dF) for them, against 27.6 and 3.45 at m = 1)."""
    from pynngp_amd import _lib

    coords, perm = _points(dim)
    n = len(coords)
    nbr = O.c_knn_prior(coords, m).astype(np.int32)
    nbr[200, 0] = n + 5
    c_d, order_d = _dt(coords, dev), _dt(perm, dev)
    nbr_d, nbr_sorted_d = _dt(nbr, dev), _dt(nbr[perm], dev)
    worst, vs_sweep, n_ok = [0.0, 0.0], [0.0, 0.0], 0
    for kind in KINDS:
        for sigma2, tau2 in ((1.0, 0.0), (1.7, 0.3)):
            B, F, dB, dF, p = (t.cpu().numpy() for t in
                               _lib.bf_dphi(c_d, nbr_sorted_d, 0, kind, sigma2, PHI, tau2, order=order_d))
            again = _lib.bf_dphi(c_d, nbr_sorted_d, 0, kind, sigma2, PHI, tau2, order=order_d)
            for a, b in zip((B, F, dB, dF, p), again):
                np.testing.assert_array_equal(a, b.cpu().numpy())
            with np.errstate(all="ignore"):
                Bh, Fh, dBh, dFh, sB, sF, cond = host_dphi(coords, nbr, kind, sigma2, PHI, tau2, want_scale=True)
            # Rows whose neighbour block is singular to fp64 (host file: DPHI_K U cond >= 1; the Gaussian kind on many
            # close neighbours without a nugget) have no value to compare: there a row is either flagged and NaN, or
            # finite.  Everywhere else nothing is flagged and the bounds hold.
            ok = resolved(cond)
            assert p[3] == 200
            nan_rows = np.isnan(dF)
            assert not nan_rows[ok].any() and (p[2] == -1) == (not nan_rows.any())
            if p[2] >= 0:
                assert nan_rows[int(p[2])] and np.all(np.isnan(dB[nan_rows])) and np.all(np.isnan(F[nan_rows]))
            assert np.all(dB[ok][nbr[ok] < 0] == 0) and np.all(dB[0] == 0)
            assert nan_rows[200] or (dB[200, 0] == 0 and B[200, 0] == 0)  # the slot with the index out of range
            assert dF[0] == 0  # no neighbour: F is the variance itself
            eB, eF = np.abs(dB - dBh).max(axis=1)[ok], np.abs(dF - dFh)[ok]
            sBo, sFo = sB[ok], sF[ok]
            worst = [max(worst[0], (eB[sBo > 0] / (U * sBo[sBo > 0])).max()),
                     max(worst[1], (eF[sFo > 0] / (U * sFo[sFo > 0])).max())]
            assert np.all(eB <= DPHI_K * U * sBo), (kind, sigma2, tau2, (eB / np.maximum(U * sBo, 1e-300)).max())
            assert np.all(eF <= DPHI_K * U * sFo), (kind, sigma2, tau2, (eF / np.maximum(U * sFo, 1e-300)).max())
            if not nan_rows.any():
                # the folds are sums of the rows' own log F and dF / F (checked above row by row): a sum of n terms in
                # another order than numpy's, each term within a few u of numpy's
                for got, terms in ((p[0], np.log(F)), (p[1], dF / F)):
                    assert abs(got - terms.sum()) <= 4 * n * U * np.abs(terms).sum()
            # B and F are the forward sweep's, to that sweep's tolerance
            Bs, Fs, ps = _lib.bf_sweep(c_d, nbr_d, 0, kind, sigma2, PHI, tau2)
            # (1e-9 (1 + |B|) and 1e-10 relative, the project's.  F is the difference (sigma2 + tau2) - c^T b, so no fp64
            # sweep holds it better than a few u of the terms it subtracts: at tau2 = 0 in d = 1 two neighbours 1e-6
            # apart leave F = 5e-11, where u (sigma2 + tau2) alone is 4e-6 of F -- measured: the two sweeps differ by
            # 1e-6 F there, 5e-17 in absolute terms.  Hence the floor 4 u (sigma2 + tau2) (1 + |b|_1) next to 1e-10 |F|;
            # it is below 1e-10 |F| wherever F >= 1e-5 (sigma2 + tau2) (1 + |b|_1).)
            Bs, Fs = Bs.cpu().numpy(), Fs.cpu().numpy()
            both = ~np.isnan(F) & ~np.isnan(Fs)
            # Two backward-stable eliminations of one block agree to about u cond(C_N) and no better, so on the rows
            # where K u cond(C_N) exceeds the project's figures (smooth kernels without a nugget on many neighbours)
            # that product stands in for them; everywhere else the project's figures hold as they are.
            floor = 4 * U * (sigma2 + tau2) * (1.0 + np.abs(Bs).sum(axis=1))
            kc = np.where(np.isfinite(cond), DPHI_K * U * cond, np.inf)
            both &= ok
            rB = (np.abs(B - Bs) / (np.maximum(1e-9, kc)[:, None] * (1.0 + np.abs(Bs))))[both].max()
            rF = (np.abs(F - Fs) / (np.maximum(1e-10, kc) * np.abs(Fs) + floor))[both].max()
            vs_sweep = [max(vs_sweep[0], rB), max(vs_sweep[1], rF)]
            print(f"  {kind} ({sigma2}, {tau2}): B, F against bf_sweep / tolerance {rB:.3g} {rF:.3g}; "
                  f"{int(ok.sum())} rows resolved, min F {np.nanmin(F):.3g}")
            assert rB <= 1.0 and rF <= 1.0
            n_ok += int(ok.sum())
    print(f"d={dim} m={m}: largest error / (U scale): dB {worst[0]:.3g} dF {worst[1]:.3g} (K = {DPHI_K}); "
          f"{n_ok} of {10 * n} rows resolved")
    assert n_ok >= 7 * n  # the singular blocks are the exception (gaussian, tau2 = 0, many neighbours)


def test_dphi_flags_a_bad_pivot_and_the_torch_op_agrees(dev):
    from pynngp_amd import _lib, load_ops

    coords, _ = _points(2)
    coords = coords.copy()
    coords[11] = coords[10]  # a repeated point: C_N is singular at tau2 = 0 for every row that holds both
    nbr = O.c_knn_prior(coords, 5).astype(np.int32)
    c_d, nbr_d = _dt(coords, dev), _dt(nbr, dev)
    B, F, dB, dF, p = (t.cpu().numpy() for t in _lib.bf_dphi(c_d, nbr_d, 0, "exponential", 1.0, PHI, 0.0))
    bad = int(p[2])
    assert bad >= 0 and p[3] == -1
    assert np.all(np.isnan(dB[bad])) and np.isnan(dF[bad]) and np.all(np.isnan(B[bad])) and np.isnan(F[bad])
    pg = _lib.bf_grad(c_d, nbr_d, 0, "exponential", 1.0, PHI, 0.0,
                      torch.zeros(len(coords), dtype=torch.float64, device=dev))[0].cpu().numpy()
    assert pg[2] == p[2]  # flagged as the gradient sweep flags it
    ops = load_ops()
    coords2, _ = _points(3)
    nbr2 = _dt(O.c_knn_prior(coords2, 9).astype(np.int32), dev)
    got = torch.ops.nngp.bf_dphi(_dt(coords2, dev), nbr2, None, 0, ops.kind_code("matern52"), 1.7, PHI, 0.3)
    ref = _lib.bf_dphi(_dt(coords2, dev), nbr2, 0, "matern52", 1.7, PHI, 0.3)
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())


# ---------------------------------------------------------------- 2. the gather
def test_rows_dot2_against_numpy_and_column_independence(dev):
    """n_s = 40 reference nodes, 120 leaves, m = 6; a slot naming a leaf and the -1 padding count 0.  Each output is a
    sum of at most m products accumulated by fma and a butterfly: within 4 m U sum|terms| of numpy's."""
    from pynngp_amd import _lib

    rng = np.random.default_rng(40)
    n_s, m = 40, 6
    _, nbr = G.reference_dag(rng.uniform(size=(n_s, 2)), rng.uniform(size=(120, 2)), m)
    nbr = nbr.astype(np.int32)
    nbr[70, 3] = 55  # a leaf where a reference node belongs
    n = nbr.shape[0]
    assert (nbr < 0).any()
    B, dB = rng.standard_normal((n, m)), rng.standard_normal((n, m)) * 10.0
    ok = (nbr >= 0) & (nbr < n_s)
    j = np.where(ok, nbr, 0)
    nbr_d, B_d, dB_d = _dt(nbr, dev), _dt(B, dev), _dt(dB, dev)
    for K in (1, 3, 8):
        X = rng.standard_normal((n_s, K)) * 10.0 ** rng.integers(-3, 4, K)
        Pd, Qd = _lib.latent_rows_dot2_batch(nbr_d, B_d, dB_d, n_s, _dt(X, dev))
        Pd, Qd = Pd.cpu().numpy(), Qd.cpu().numpy()
        assert Pd.shape == Qd.shape == (n, K)
        for W, got in ((B, Pd), (dB, Qd)):
            terms = np.where(ok[:, :, None], W[:, :, None] * X[j], 0.0)
            assert np.all(np.abs(got - terms.sum(axis=1)) <= 4 * m * U * np.abs(terms).sum(axis=1))
        assert np.all(Pd[0] == 0) and np.all(Qd[0] == 0)  # the first reference node has no parent
        for c in range(K):
            p1, q1 = _lib.latent_rows_dot2_batch(nbr_d, B_d, dB_d, n_s, _dt(X[:, c:c + 1], dev))
            np.testing.assert_array_equal(Pd[:, c], p1.cpu().numpy()[:, 0])
            np.testing.assert_array_equal(Qd[:, c], q1.cpu().numpy()[:, 0])


# ---------------------------------------------------------------- 3. the exact gradient
def _device_system(lp):
    """The node DAG, its coordinates, unit-variance factors and d = h / tau2 as the device holds them, in MODEL node
    order (tests/test_gpu_latent_logdet.py::_device_system, with the coordinates)."""
    perm = lp.perm.cpu().numpy()
    nbs = lp.nbr.cpu().numpy()
    n, m = nbs.shape
    nbr, B, F, d = np.full((n, m), -1, dtype=np.int32), np.zeros((n, m)), np.zeros(n), np.zeros(n)
    coords = np.zeros((n, lp.coords.shape[1]))
    nbr[perm] = np.where(nbs >= 0, perm[np.maximum(nbs, 0)], -1)
    B[perm] = lp.B.cpu().numpy()
    F[perm] = lp.F.cpu().numpy()
    d[perm] = lp.d.cpu().numpy()
    coords[perm] = lp.coords.cpu().numpy()
    return coords, nbr, B, F, d


def _node_data(lp, y, X=None):
    n = lp.n_nodes
    obs = np.isfinite(y)
    yn = np.zeros(n)
    yn[lp.node_of_t[obs]] = y[obs]
    Xn = None
    if X is not None:
        Xn = np.zeros((n, X.shape[1]))
        Xn[lp.node_of_t] = X
    return yn, Xn


def _dense_side(lp, y, X, beta):
    coords, nbr, B, F, d = _device_system(lp)
    cov = lp.cov
    yn, Xn = _node_data(lp, y, X)
    v = yn if X is None else yn - Xn @ beta
    _, _, dB, dF = host_dphi(coords, nbr, cov.kind, 1.0, cov.phi, 0.0)
    return dense_grad(nbr, B, F, dB, dF, lp.n_s, cov.sigma2, cov.tau2, d, v)


def _check_exact_gradient(lp, y, X, beta=None, rtol=1e-10):
    """Basis probes: the trace is exact, so grad is the dense closed form up to (cond(A_S) rtol + n u) of the sum of
    the magnitudes of its terms on the device side -- the solves to rtol, sums of n terms -- plus the dense side's own
    100 u cond(A_S) of the same sum (test_gpu_latent_logdet.py::_check_logdet_and_marginal's construction)."""
    n_s, n = lp.n_s, lp.n_nodes
    Z = math.sqrt(n_s) * np.eye(n_s)
    kw = dict(z=Z, rtol=rtol, logdet_rtol=rtol)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        value, se, grad, grad_se = lp.log_marginal_grad(beta=beta, **kw)
        assert (value, se) == lp.log_marginal(beta=beta, **kw)
    exact, mag, cond = _dense_side(lp, y, X, beta if beta is not None else np.zeros(0))
    tol = (2 * cond * rtol + 4 * n * U + 100 * U * cond) * mag
    print(f"n_s={n_s} n={n}: grad {grad} dense {exact} err/tol {np.abs(grad - exact) / tol} grad_se {grad_se}")
    assert grad.shape == (3,) and grad_se.shape == (3,)
    assert np.all(np.abs(grad - exact) <= tol)
    assert np.all(np.isfinite(grad_se))
    return grad


@pytest.mark.parametrize("n,m", [(48, 5), (64, 8)])
def test_exact_gradient_s_equals_t(dev, n, m):
    from pynngp_amd import Covariance, LatentPosterior

    rng = np.random.default_rng(n)
    t, y = rng.uniform(size=(n, 2)), rng.standard_normal(n)
    y[rng.uniform(size=n) < 0.25] = np.nan
    y[0] = 0.4
    eps = rng.uniform(0.5, 2.0, n)
    lp = LatentPosterior(t, y, Covariance("exponential", SIGMA2, PHI, TAU2), m=m, eps=eps, device=dev)
    assert lp.n_s == lp.n_nodes == n
    _check_exact_gradient(lp, y, None)


@pytest.mark.parametrize("case", ["A-40-120", "A-with-X", "B-8-700"])
def test_exact_gradient_reference_set(dev, case):
    from pynngp_amd import Covariance, LatentPosterior

    rng = np.random.default_rng(5)
    X = None
    if case.startswith("A"):  # 40 reference points, 120 data locations of which 10 coincide with reference points
        s = rng.uniform(size=(40, 2))
        t = np.concatenate([s[rng.choice(40, size=10, replace=False)], rng.uniform(size=(110, 2))])
        t = t[rng.permutation(120)]
        m = 6
        if case == "A-with-X":
            X = np.column_stack([np.ones(120), rng.standard_normal(120)])
    else:  # 8 knots, 700 leaves, m = 4: reverse lists above 512 entries
        s = np.array([[0.42, 0.45], [0.58, 0.44], [0.45, 0.57], [0.57, 0.58], [0.02, 0.03], [0.97, 0.02],
                      [0.03, 0.98], [0.98, 0.97]])
        t = rng.uniform(size=(700, 2))
        m = 4
    N = len(t)
    y = rng.standard_normal(N) + (X @ np.array([0.7, -0.4]) if X is not None else 0.0)
    y[rng.uniform(size=N) < 0.25] = np.nan
    y[0] = 0.3
    eps = rng.uniform(0.5, 2.0, N)
    lp = LatentPosterior(t, y, Covariance("exponential", SIGMA2, PHI, TAU2), m=m, X=X, eps=eps, device=dev, ref=s)
    assert lp.n_s == len(s)
    beta = None
    if X is not None:
        beta = lp.gls_beta(rtol=1e-10)
    grad = _check_exact_gradient(lp, y, X, beta=beta)
    if X is not None:  # beta_hat is what beta=None plugs in: the same call, bit for bit
        Z = math.sqrt(lp.n_s) * np.eye(lp.n_s)
        lp._beta_hat = None
        other = lp.log_marginal_grad(z=Z, rtol=1e-10, logdet_rtol=1e-10)
        np.testing.assert_array_equal(other[2], grad)


@pytest.mark.parametrize("kind", ["matern32", "matern52", "gaussian", "spherical"])
def test_exact_gradient_other_kinds(dev, kind):
    from pynngp_amd import Covariance, LatentPosterior

    rng = np.random.default_rng(77)
    s, t = rng.uniform(size=(30, 2)), rng.uniform(size=(50, 2))
    y = rng.standard_normal(50)
    y[::5] = np.nan
    phi = 2.5 if kind == "spherical" else PHI
    lp = LatentPosterior(t, y, Covariance(kind, SIGMA2, phi, TAU2), m=5, device=dev, ref=s)
    _check_exact_gradient(lp, y, None)


# ---------------------------------------------------------------- 4. the stochastic gradient
def test_rademacher_gradient_and_batch_independence(dev):
    """n = 600, m = 10, theta = (1, 12, 0.1), 32 Rademacher probes: |grad - exact| <= 4 grad_se per component.  (The
    numpy restatement ``hutchinson_ratios`` of the trace estimate on this very system with numpy's own signs gave
    |estimate - exact| / se = (0.76, 0.76, 0.76), (0.27, 0.24, 0.27), (1.39, 1.38, 1.39) and (0.15, 0.20, 0.15) for
    (sigma2, phi, tau2) over the seeds 0 .. 3 -- with S = T and one noise level the sigma2 and tau2 traces are the same
    estimate up to scale; the device's probes are Philox signs, which numpy cannot restate, so the seed is the default
    one, at which the device gave 0.67, 0.64 and 0.67.)"""
    from pynngp_amd import Covariance, LatentPosterior

    rng = np.random.default_rng(12)
    n, m = 600, 10
    t, y = rng.uniform(size=(n, 2)), rng.standard_normal(n)
    lp = LatentPosterior(t, y, Covariance("exponential", 1.0, 12.0, 0.1), m=m, device=dev)
    exact, _, _ = _dense_side(lp, y, None, np.zeros(0))
    value, se, grad, grad_se = lp.log_marginal_grad(n_probes=32, seed=0)
    print(f"grad {grad} +- {grad_se}, exact {exact}: error / se {np.abs(grad - exact) / grad_se}")
    assert (value, se) == lp.log_marginal(n_probes=32, seed=0)
    assert np.all(grad_se > 0) and np.all(np.abs(grad - exact) <= 4 * grad_se)
    for batch in (1, 3, 8):
        other = lp.log_marginal_grad(n_probes=32, seed=0, batch=batch)
        assert other[0] == value and other[1] == se
        np.testing.assert_array_equal(other[2], grad)
        np.testing.assert_array_equal(other[3], grad_se)


# ---------------------------------------------------------------- 5. fit
def test_gradient_fit_reaches_the_truth_in_fewer_evaluations(dev):
    from pynngp_amd import Covariance, LatentPosterior

    rng = np.random.default_rng(2000)
    n, m = 2000, 10
    truth = Covariance("exponential", 1.5, 8.0, 0.2)
    t = rng.uniform(size=(n, 2))
    nbr = O.c_knn_prior(t, m)
    Bt, Ft, _ = O.c_bf_sweep(t, nbr, "exponential", (1.0, truth.phi, 0.0))
    w = O.c_nngp_simulate(nbr, Bt, Ft * truth.sigma2, rng.standard_normal(n))
    y = w + math.sqrt(truth.tau2) * rng.standard_normal(n)
    start = Covariance("exponential", truth.sigma2 * 3.0, truth.phi / 3.0, truth.tau2 * 3.0)
    lp = LatentPosterior(t, y, start, m=m, device=dev)
    kw = dict(n_probes=16, seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ll_truth, _ = lp.update(truth).log_marginal(**kw)
        lp.update(start)
        cov_nm, res_nm = lp.fit(maxiter=40, **kw)
        ll_nm, se_nm = lp.log_marginal(**kw)
        lp.update(start)
        cov, res = lp.fit(gradient=True, maxiter=15, **kw)
        ll_fit, se = lp.log_marginal(**kw)
    print(f"truth {ll_truth:.3f}; Nelder-Mead {ll_nm:.3f} at {cov_nm.theta} after {res_nm.nfev} evaluations; "
          f"L-BFGS-B {ll_fit:.3f} +- {se:.3f} at {cov.theta} after {res.nfev} evaluations")
    assert lp.cov == cov and ll_fit == -res.fun
    assert ll_fit >= ll_truth
    assert ll_fit >= ll_nm - 2 * se
    assert res.nfev < res_nm.nfev


def test_gradient_fit_thin_callers_and_general_nu(dev):
    from pynngp_amd import NNGP, Covariance, LatentPosterior

    rng = np.random.default_rng(31)
    t, y = rng.uniform(size=(300, 2)), rng.standard_normal(300)
    start = Covariance("exponential", 1.0, 6.0, 0.3)
    model = NNGP(t, y, None, ("random", 60, [(0.0, 1.0), (0.0, 1.0)]), 6, start, device=dev)
    val, se, grad, grad_se = model.latent_loglik_grad(mean="zero", n_probes=8)
    assert (val, se) == model.latent_loglik(mean="zero", n_probes=8)
    assert grad.shape == (3,) and np.all(np.isfinite(grad)) and np.all(grad_se > 0)
    cov2, res2 = model.latent_fit(mean="zero", n_probes=8, maxiter=3, gradient=True)
    assert model.cov == cov2 and -res2.fun >= val
    lp = LatentPosterior(t[:50], y[:50], Covariance("matern", 1.0, 6.0, 0.3, nu=1.2), m=5, device=dev)
    with pytest.raises(ValueError, match="matern"):
        lp.fit(gradient=True)
    with pytest.raises(ValueError, match="matern"):
        lp.log_marginal_grad()
