"""Spatially varying coefficients on the GPU: nngp_bf_sweep_svc / nngp_bf_cross_svc / nngp_bf_grad_svc against the
long-double restatement tests/svc_ref.py (pinned on the CPU by tests/test_svc_host.py), the torch ops, and SVCNNGP
(loglik, coef, predict, fit).

Bounds (the family's, from test_gpu_sep.py).  Forward and cross sweeps: bf_precision_ref.check_sweep (BF_K U scale per
row on the resolved rows, the scale's sigma2 + tau2 the joint block's largest diagonal entry).  Gradient: every row of G
within 1e-9 (1 + |G|) of the restatement, each of the 2 r + 1 sums within 1e-12 sum |row terms|.
"""
import numpy as np
import pytest
import torch

import svc_ref as S
from bf_precision_ref import BF_K, RESOLVED_SHARE, U, check_sweep
from pynngp_amd import SVCCovariance, SVCNNGP, _lib

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared inputs are read-only


def host(*ts):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def forward(coords, Z, nbr, kind, th, y, order=None):
    return host(*_lib.bf_sweep_svc(dev(coords), dev(Z), dev(nbr), 0, kind, *th, values=dev(y), order=order, want_r=True))


def grad(coords, Z, nbr, kind, th, y, order=None):
    return host(*_lib.bf_grad_svc(dev(coords), dev(Z), dev(nbr), 0, kind, *th, dev(y), want_rows=True, order=order))


def cross(coords, Z, q, zq, nbr, kind, th, y, yq=None, noise=True):
    return host(*_lib.bf_cross_svc(dev(coords), dev(Z), dev(q), dev(zq), dev(nbr), kind, *th, ref_values=dev(y),
                                   query_values=None if yq is None else dev(yq), target_noise=noise, want_r=True))


def check_grad(ref, p, g, G, where):
    Gr = ref.G.astype(np.float64)
    Sm = np.abs(Gr).sum(0)
    err = np.abs(g - Gr.sum(0))
    print(f"{where}: grad err {err}, sum|G| {Sm}, worst row / (1 + |G|) "
          f"{(np.abs(G - Gr) / (1 + np.abs(Gr))).max():.3g}")
    assert p[2] == -1 and p[3] == -1, (where, p)
    assert G.shape == Gr.shape and g.shape == (Gr.shape[1],)
    assert np.all(err <= 1e-12 * Sm), (where, "sums", err, Sm)
    assert np.all(np.abs(G - Gr) <= 1e-9 * (1 + np.abs(Gr))), (where, "rows")


def one_case(dim, kind, r, m):
    coords, Z, y = S.field(dim, r)
    th = S.theta_of(kind, r)
    nbr = S.neighbours(dim, m)
    ref = S.prior_reference(dim, m, kind, r)
    where = f"d{dim} {kind} r{r} m{m}"
    assert ref.resolved.mean() >= RESOLVED_SHARE, (where, ref.resolved.mean())
    check_sweep(ref, *forward(coords, Z, nbr, kind, th, y), "sweep " + where)
    check_grad(ref, *grad(coords, Z, nbr, kind, th, y), "grad " + where)
    q, zq, yq = S.query(dim, r)
    cref = S.cross_reference(dim, m, kind, r)
    assert cref.resolved.mean() >= RESOLVED_SHARE, (where, cref.resolved.mean())
    check_sweep(cref, *cross(coords, Z, q, zq, S.query_neighbours(dim, m), kind, th, y, yq), "cross " + where)


# ---------------------------------------------------------------- every instantiation against the restatement
@pytest.mark.parametrize("m", S.M_ALL)
def test_every_m(m):
    """Forward, gradient and cross sweeps of two exponential components at every m; the first m rows carry -1."""
    one_case(2, "exponential", 2, m)


@pytest.mark.parametrize("m", S.M_EDGES)
@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("r", [1, 3, 4])
@pytest.mark.parametrize("kind", S.KINDS)
def test_every_kind_count_and_dimension(kind, r, dim, m):
    one_case(dim, kind, r, m)


@pytest.mark.parametrize("m", [8, 15, 23, 31, 32])
def test_bits_are_reproducible_and_independent_of_order(m):
    """Two runs give equal bits, without and with an ``order`` permutation; every per-row result (B, F, R, G) has the
    same bits under the permutation.  The sums are folded block by block in launch order, as the family's are
    (bf_finalize's fold): under another order they move within check_grad's bound, not bit for bit."""
    coords, Z, y = S.field(2, 3)
    th, nbr = S.theta_of("matern32", 3), S.neighbours(2, m)
    perm = np.random.default_rng(m).permutation(S.N).astype(np.int32)
    runs = [grad(coords, Z, nbr, "matern32", th, y) + forward(coords, Z, nbr, "matern32", th, y) for _ in range(2)]
    moved = [grad(coords, Z, nbr[perm], "matern32", th, y, order=dev(perm))
             + forward(coords, Z, nbr[perm], "matern32", th, y, order=dev(perm)) for _ in range(2)]
    for pair in (runs, moved):
        assert all(np.array_equal(a, b) for a, b in zip(*pair))
    pg, g, G, B, F, R, p = moved[0]
    for a, b in zip((G, B, F, R), (runs[0][2], *runs[0][3:6])):
        assert np.array_equal(a, b)
    check_grad(S.prior_reference(2, m, "matern32", 3), pg, g, G, f"ordered m{m}")
    check_sweep(S.prior_reference(2, m, "matern32", 3), B, F, R, p, f"ordered m{m}")


# ---------------------------------------------------------------- known answers
def model(coords, y, Z, m, kind, th, **kw):
    return SVCNNGP(coords, y, Z, m, SVCCovariance(kind, *th), **kw)


@pytest.mark.parametrize("kind", ["exponential", "gaussian", "spherical"])
@pytest.mark.parametrize("m", [9, 32])
def test_one_constant_covariate_is_the_isotropic_model(kind, m):
    """r = 1, Z = 1: SVCNNGP.loglik equals NNGP.loglik at the matching Covariance within the sum of both sweeps' bounds
    on sum log F and sum r^2 / F (check_sweep's slacks, from the restatement's scales)."""
    import pynngp_amd

    coords, _, y = S.field(2, 1)
    th = S.theta_of(kind, 1)
    ref = S.prior_reference(2, m, kind, 1)
    n, F, r = S.N, ref.F.astype(np.float64), np.abs(ref.r.astype(np.float64))
    eF, eR = BF_K * U * ref.sF, BF_K * U * ref.sR
    slack = (4 * n * U * np.abs(np.log(F)).sum() + (eF / F).sum() + 4 * n * U * (r * r / F).sum()
             + ((r + eR) ** 2 / (F - eF) - r * r / F).sum())
    got = model(coords, y, np.ones((n, 1)), m, kind, th).loglik()
    iso = pynngp_amd.NNGP(coords, y, None, "S=T", m, pynngp_amd.Covariance(kind, th[0][0], th[1][0], th[2])).loglik()
    print(f"{kind} m{m}: svc {got!r} iso {iso!r} slack {slack:.3g}")
    assert abs(got - iso) <= 2 * 0.5 * slack


def test_full_sets_give_the_dense_density():
    """n = 33, m = 32, r = 3: loglik is the dense Gaussian log density of the SVC covariance in long double, to the
    forward bound on the two sums."""
    coords, Z, y = (a[:33] for a in S.field(2, 3))
    th = S.theta_of("matern32", 3)
    md = model(coords, y, Z, 32, "matern32", th)
    ref = S.rows(coords, Z, coords, Z, md.nbr.cpu().numpy(), "matern32", th, y, y)
    want = S.dense_loglik(coords, Z, "matern32", th, y)
    assert abs(float(ref.ll.sum()) - want) <= 1e-13 * abs(want)
    F, r = ref.F.astype(np.float64), np.abs(ref.r.astype(np.float64))
    eF, eR = BF_K * U * ref.sF, BF_K * U * ref.sR
    slack = 0.5 * (4 * 33 * U * (np.abs(np.log(F)) + r * r / F).sum() + (eF / F).sum()
                   + ((r + eR) ** 2 / (F - eF) - r * r / F).sum())
    got = md.loglik()
    print(f"dense {want!r} nngp {got!r} slack {slack:.3g}")
    assert abs(got - want) <= slack + 1e-13 * abs(want)


def test_rescaling_a_covariate_against_its_variance():
    """Z[:, k] * c with sigma2_k / c^2 is the same model: the log-likelihood moves by rounding only."""
    coords, Z, y = S.field(2, 3)
    s2, ph, t2 = S.theta_of("exponential", 3)
    base = model(coords, y, Z, 15, "exponential", (s2, ph, t2)).loglik()
    for k, c in ((1, 4.0), (2, 0.3)):
        Zs, s2s = Z.copy(), list(s2)
        Zs[:, k] *= c
        s2s[k] /= c * c
        got = model(coords, y, Zs, 15, "exponential", (s2s, ph, t2)).loglik()
        assert abs(got - base) <= 1e-12 * abs(base), (k, c, got, base)


# ---------------------------------------------------------------- masks
@pytest.mark.parametrize("m", [9, 16, 32])
def test_masked_slots_flags_and_coincident_points(m):
    coords, Z, y = S.field(2, 2)
    coords, Z = coords.copy(), Z.copy()
    coords[70] = coords[3]  # two coincident points with different z rows
    th = S.theta_of("matern52", 2)
    nbr = S.neighbours(2, m).copy()
    nbr[60:, m // 2] = -1
    nbr[80:, 0] = 3  # rows past 70 hold both coincident points where 70 is a neighbour already, or gain point 3
    ref = S.rows(coords, Z, coords, Z, nbr, "matern52", th, y, y)
    B, F, R, p = forward(coords, Z, nbr, "matern52", th, y)
    check_sweep(ref, B, F, R, p, f"masked m{m}")
    assert np.all(B[60:, m // 2] == 0.0)
    check_grad(ref, *grad(coords, Z, nbr, "matern52", th, y), f"masked grad m{m}")
    if m > 1:  # a -1 slot is otherwise the shorter set
        short = np.delete(nbr, m // 2, axis=1)
        Bs, Fs, Rs, _ = forward(coords, Z, short, "matern52", th, y)
        ok = ref.resolved[60:]
        assert np.all(np.abs(np.delete(B, m // 2, axis=1) - Bs)[60:][ok] <= 2 * BF_K * U * ref.sB[60:][ok, None])
        assert np.all(np.abs(F - Fs)[60:][ok] <= 2 * BF_K * U * ref.sF[60:][ok])
    nbr[90, 1] = S.N + 5  # out of range: flagged, and masked like -1
    _, _, _, p = forward(coords, Z, nbr, "matern52", th, y)
    pg, _, _ = grad(coords, Z, nbr, "matern52", th, y)
    assert p[3] == 90 and pg[3] == 90 and p[2] == -1


# ---------------------------------------------------------------- coef and predict
def test_coef_and_predict_are_the_dense_conditionals():
    """n = 96, m = 10, r = 2: coef(query) is the conditional of w_k(s0) on the query's m nearest data points, and
    predict(noise=True) that of y0, both dense in long double.  Bounds: BF_K U sB |y_N| for the means (check_sweep's sR
    without the residual), BF_K U sF for the variances, from a restatement with the same z_query."""
    coords, Z, y = S.field(2, 2)
    q, zq, _ = S.query(2, 2)
    th = S.theta_of("exponential", 2)
    md = model(coords, y, Z, 10, "exponential", th)
    nbr = _lib.knn_query(dev(coords), dev(q), 10).cpu().numpy()
    cm, cv = md.coef(q)
    pm, pv = md.predict(q, zq)
    assert cm.shape == cv.shape == (S.N_QUERY, 2)
    for k in range(3):  # the two coefficients, then y itself
        z0 = zq if k == 2 else np.tile(np.eye(2)[k], (S.N_QUERY, 1))
        ref = S.rows(coords, Z, q, z0, nbr, "exponential", th, y, None, target_noise=k == 2)
        want = np.array([S.conditional(coords, Z, y, nbr[i], q[i:i + 1], z0[i:i + 1], "exponential", th, k == 2)
                         for i in range(S.N_QUERY)])
        assert np.allclose(-ref.r.astype(np.float64), want[:, 0], rtol=1e-12, atol=1e-13)
        got_m, got_v = (pm, pv) if k == 2 else (cm[:, k], cv[:, k])
        assert np.all(np.abs(got_m - want[:, 0]) <= BF_K * U * ref.sR + 1e-13 * np.abs(want[:, 0]))
        assert np.all(np.abs(got_v - want[:, 1]) <= BF_K * U * ref.sF + 1e-13 * np.abs(want[:, 1]))


# ---------------------------------------------------------------- fit
def test_fit_with_and_without_the_gradient():
    """n = 600, m = 10, r = 2, exponential, drawn by a dense Cholesky at a known theta plus X beta."""
    rng = np.random.default_rng(77)
    n = 600
    coords = rng.uniform(0.0, 1.0, (n, 2))
    Z = np.stack([np.ones(n), rng.standard_normal(n)], axis=1)
    X = np.stack([np.ones(n), Z[:, 1], rng.standard_normal(n)], axis=1)
    true = ((1.0, 0.6), (5.0, 9.0), 0.1)
    K = S.dense_cov(coords, Z, coords, Z, "exponential", true, np.float64) + true[2] * np.eye(n)
    y = X @ np.array([1.0, -0.5, 2.0]) + np.linalg.cholesky(K) @ rng.standard_normal(n)
    start = ((0.5, 0.5), (3.0, 3.0), 0.3)
    md = model(coords, y, Z, 10, "exponential", start, X=X)
    at_true = md.profile_loglik(SVCCovariance("exponential", *true))[0]
    with_g = md.fit(gradient=True)
    md.cov = SVCCovariance("exponential", *start)
    without = md.fit(gradient=False)
    print(f"fit: true {at_true:.6f}; gradient {with_g['loglik']:.6f} in {with_g['n_evals']} evaluations, theta "
          f"{with_g['theta']}; Nelder-Mead {without['loglik']:.6f} in {without['n_evals']} evaluations")
    assert with_g["loglik"] >= at_true
    assert abs(with_g["loglik"] - without["loglik"]) <= 1e-3


# ---------------------------------------------------------------- torch operators
@pytest.mark.parametrize("m", [15, 24])
def test_torch_ops_and_autograd(m):
    import pynngp_amd

    pynngp_amd.load_ops()
    coords, Z, y = S.field(3, 3)
    s2, ph, t2 = S.theta_of("matern52", 3)
    c, z, nb, v = dev(coords), dev(Z), dev(S.neighbours(3, m)), dev(y)
    B, F, R, p = torch.ops.nngp.bf_sweep_svc(c, z, nb, None, 0, 2, s2, ph, t2, v, True)
    B2, F2, R2, p2 = _lib.bf_sweep_svc(c, z, nb, 0, "matern52", s2, ph, t2, values=v, want_r=True)
    pg, g, G = torch.ops.nngp.bf_grad_svc(c, z, nb, None, 0, 2, s2, ph, t2, v, True)
    pg2, g2, G2 = _lib.bf_grad_svc(c, z, nb, 0, "matern52", s2, ph, t2, v, want_rows=True)
    q, zq, _ = S.query(3, 3)
    qn = dev(S.query_neighbours(3, m))
    Bc, Fc, mean = torch.ops.nngp.bf_cross_svc(c, z, dev(q), dev(zq), qn, 2, s2, ph, t2, False, v)
    Bc2, Fc2, Rc2, _ = _lib.bf_cross_svc(c, z, dev(q), dev(zq), qn, "matern52", s2, ph, t2, ref_values=v,
                                         target_noise=False, want_r=True)
    for a, b in ((B, B2), (F, F2), (R, R2), (p, p2), (pg, pg2), (g, g2), (G, G2), (Bc, Bc2), (Fc, Fc2), (mean, -Rc2)):
        assert torch.equal(a, b)
    th = torch.tensor([*s2, *ph, t2], dtype=torch.float64, requires_grad=True)
    ll = pynngp_amd.loglik_svc(c, z, nb, "matern52", th, v)
    ll.backward()
    assert torch.equal(th.grad, g.cpu())
    assert abs(ll.item() - (-0.5 * (S.N * np.log(2.0 * np.pi) + pg[0] + pg[1])).item()) <= 1e-13 * abs(ll.item())
