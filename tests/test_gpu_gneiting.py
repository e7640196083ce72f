"""The Gneiting space-time sweeps, torch ops and model paths on the GPU against tests/gneiting_ref.py, at
tests/test_gpu_sep.py's bounds: check_sweep for the rows, 1e-9 (1 + |G|) per gradient row, 1e-12 sum |row terms|."""
import numpy as np
import pytest
import torch

import gneiting_ref as Gn
from bf_precision_ref import BF_K, RESOLVED_SHARE, U, check_sweep
from oracle import nngp_oracle as O
from pynngp_amd import _lib
from gneiting_ref import N, scaled

pytestmark = pytest.mark.gpu
EXP = "exponential"


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared inputs are read-only


def host(*ts):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def forward(coords, nbr, kind, th, y, i0=0, order=None):
    return host(*_lib.bf_sweep_gneiting(dev(coords), nbr if torch.is_tensor(nbr) else dev(nbr), i0, kind, *th,
                                        values=dev(y), order=order, want_r=True))


def grad(coords, nbr, kind, th, y, i0=0, order=None):
    return host(*_lib.bf_grad_gneiting(dev(coords), nbr if torch.is_tensor(nbr) else dev(nbr), i0, kind, *th, dev(y),
                                       want_rows=True, order=order))


def check_grad(ref, p, g, G, where):
    Gr = ref.G.astype(np.float64)
    Sm = np.abs(Gr).sum(0)
    err = np.abs(g - Gr.sum(0))
    print(f"{where}: grad err {err}, sum|G| {Sm}, worst row / (1 + |G|) "
          f"{(np.abs(G - Gr) / (1 + np.abs(Gr))).max():.3g}")
    assert p[2] == -1 and p[3] == -1, (where, p)
    assert G.shape == Gr.shape and g.shape == (5,)
    assert np.all(err <= 1e-12 * Sm), (where, "sums", err, Sm)
    assert np.all(np.abs(G - Gr) <= 1e-9 * (1 + np.abs(Gr))), (where, "rows")


def one_case(dim, kind, beta, m):
    coords, y = Gn.field(dim)
    th = Gn.theta_of(beta)
    nbr = Gn.neighbours(dim, m)
    ref = Gn.prior_reference(dim, m, kind, beta)
    where = f"d{dim} {kind} beta{beta} m{m}"
    assert ref.resolved.mean() >= RESOLVED_SHARE, (where, ref.resolved.mean())
    check_sweep(ref, *forward(coords, nbr, kind, th, y), "sweep " + where)
    check_grad(ref, *grad(coords, nbr, kind, th, y), "grad " + where)
    q, yq = Gn.query(dim)
    cref = Gn.cross_reference(dim, m, kind, beta)
    assert cref.resolved.mean() >= RESOLVED_SHARE, (where, cref.resolved.mean())
    check_sweep(cref, *host(*_lib.bf_cross_gneiting(dev(coords), dev(q), dev(Gn.query_neighbours(dim, m)), kind, *th,
                                                    ref_values=dev(y), query_values=dev(yq), want_r=True)),
                "cross " + where)


@pytest.mark.parametrize("dim,kind,beta,m", Gn.CASES)
def test_rows_and_gradient(dim, kind, beta, m):
    """Forward, gradient and cross sweeps; the first m rows carry -1 padding."""
    one_case(dim, kind, beta, m)


@pytest.mark.parametrize("m", [8, 15, 23, 32])
def test_constant_time_against_the_noise_sweeps(m):
    """All times equal (psi = 1): nngp_bf_sweep_noise / nngp_bf_grad_noise at v = 1 on the spatial columns; the a and
    beta components are exactly 0."""
    coords, y = (a.copy() for a in Gn.field(3))
    coords[:, 2] = 0.37
    th = Gn.theta_of(0.5)
    nbr = Gn.neighbours(3, m)
    ref = Gn.rows(coords, coords, nbr, "matern52", th, y, y)
    ok = ref.resolved
    assert ok.mean() >= RESOLVED_SHARE
    B, F, R, p = forward(coords, nbr, "matern52", th, y)
    check_sweep(ref, B, F, R, p, f"constant time m{m}")
    one, sp = dev(np.ones(N)), dev(coords[:, :2])
    Bn, Fn, Rn, _ = host(*_lib.bf_sweep_noise(sp, dev(nbr), 0, "matern52", th[0], th[1], th[4], one, values=dev(y),
                                              want_r=True))
    assert np.all(np.abs(B - Bn).max(1)[ok] <= BF_K * U * ref.sB[ok])
    assert np.all(np.abs(F - Fn)[ok] <= BF_K * U * ref.sF[ok])
    assert np.all(np.abs(R - Rn)[ok] <= BF_K * U * ref.sR[ok])
    pg, g, G = grad(coords, nbr, "matern52", th, y)
    check_grad(ref, pg, g, G, f"constant time grad m{m}")
    assert np.all(G[:, 2:4] == 0.0) and np.all(g[2:4] == 0.0)
    pn, gn, Gn_ = host(*_lib.bf_grad_noise(sp, dev(nbr), 0, "matern52", th[0], th[1], th[4], dev(y), one,
                                           want_rows=True))
    assert np.all(np.abs(G[:, [0, 1, 4]] - Gn_) <= 1e-9 * (1 + np.abs(Gn_)))
    assert np.all(np.abs(g[[0, 1, 4]] - gn) <= 1e-12 * np.abs(ref.G.astype(np.float64)).sum(0)[[0, 1, 4]])


@pytest.mark.parametrize("one_site", [False, True])
def test_coincident_sites_and_times(one_site):
    """Pairs at one site and twenty points at one time; or every point at one site (h = 0, so dv = 0): there the c and
    with it the beta column are exactly 0 and the a column is not.  (Every point at one time: the constant-time test.)"""
    coords, y = (a.copy() for a in Gn.field(3))
    coords[1::2, :2] = coords[0::2, :2]
    coords[40:60, 2] = coords[40, 2]
    if one_site:
        coords[:, :2] = (0.3, 0.6)
    th = Gn.theta_of(0.5)
    nbr = O.c_knn_prior(coords, 9)
    ref = Gn.rows(coords, coords, nbr, EXP, th, y, y)
    assert ref.resolved.mean() >= RESOLVED_SHARE
    check_sweep(ref, *forward(coords, nbr, EXP, th, y), "coincident")
    p, g, G = grad(coords, nbr, EXP, th, y)
    check_grad(ref, p, g, G, "coincident grad")
    if one_site:
        assert np.all(G[:, [1, 3]] == 0.0) and g[1] == 0.0 and g[3] == 0.0 and np.any(G[:, 2] != 0.0)


def test_dense_known_answer():
    """n = 33, m = 32: every row conditions on all earlier points, so the log-likelihood is the dense density."""
    coords, y = Gn.field(3, 33)
    th = Gn.theta_of(0.5)
    nbr = Gn.neighbours(3, 32, 33)
    p = forward(coords, nbr, EXP, th, y)[3]
    ll = -0.5 * (33 * Gn.LOG_2PI + p[0] + p[1])
    want = Gn.dense_loglik(coords, EXP, th, y)
    assert abs(ll - want) <= 1e-10 * abs(want), (ll, want)


@pytest.mark.parametrize("m", [9, 31])
def test_equal_bits_subranges_order_and_torch_ops(m):
    import pynngp_amd

    pynngp_amd.load_ops()
    coords, y = Gn.field(3)
    th = Gn.theta_of(0.5)
    nbr = Gn.neighbours(3, m)
    a, b = forward(coords, nbr, EXP, th, y), forward(coords, nbr, EXP, th, y)
    ga, gb = grad(coords, nbr, EXP, th, y), grad(coords, nbr, EXP, th, y)
    for u, v in zip(a + ga, b + gb):
        assert np.array_equal(u, v)
    lo, hi = forward(coords, nbr[:50], EXP, th, y), forward(coords, nbr[50:], EXP, th, y, i0=50)
    for k in range(3):
        assert np.array_equal(np.concatenate([lo[k], hi[k]]), a[k])
    glo, ghi = grad(coords, nbr[:50], EXP, th, y), grad(coords, nbr[50:], EXP, th, y, i0=50)
    assert np.array_equal(np.concatenate([glo[2], ghi[2]]), ga[2])
    perm = np.random.default_rng(3).permutation(N).astype(np.int32)
    po = forward(coords, nbr[perm], EXP, th, y, order=dev(perm))
    for k in range(3):
        assert np.array_equal(po[k], a[k])
    assert np.array_equal(grad(coords, nbr[perm], EXP, th, y, order=dev(perm))[2], ga[2])
    k = _lib.KIND_CODES[EXP]
    t = host(*torch.ops.nngp.bf_sweep_gneiting(dev(coords), dev(nbr), None, 0, k, *th, dev(y), True))
    for u, v in zip(t, a):
        assert np.array_equal(u, v)
    tg = host(*torch.ops.nngp.bf_grad_gneiting(dev(coords), dev(nbr), None, 0, k, *th, dev(y), True))
    for u, v in zip(tg, ga):
        assert np.array_equal(u, v)
    q, _ = Gn.query(3)
    qd, qn = dev(q), dev(Gn.query_neighbours(3, m))
    tc = host(*torch.ops.nngp.bf_cross_gneiting(dev(coords), qd, qn, k, *th, dev(y)))
    cc = host(*_lib.bf_cross_gneiting(dev(coords), qd, qn, EXP, *th, ref_values=dev(y), want_r=True))
    assert np.array_equal(tc[0], cc[0]) and np.array_equal(tc[1], cc[1]) and np.array_equal(tc[2], -cc[2])
    cpu = [torch.from_numpy(np.array(a)) for a in (coords, nbr, y, q, Gn.query_neighbours(3, m))]
    with pytest.raises(RuntimeError):
        torch.ops.nngp.bf_sweep_gneiting(cpu[0], cpu[1], None, 0, k, *th, cpu[2], True)
    with pytest.raises(RuntimeError):
        torch.ops.nngp.bf_grad_gneiting(cpu[0], cpu[1], None, 0, k, *th, cpu[2], True)
    with pytest.raises(RuntimeError):
        torch.ops.nngp.bf_cross_gneiting(cpu[0], cpu[3], cpu[4], k, *th, cpu[2])


def test_empty_slots_and_flags():
    coords, y = Gn.field(3)
    th = Gn.theta_of(0.5)
    nbr = np.array(Gn.neighbours(3, 9))
    base = forward(coords, nbr, EXP, th, y)
    gbase = grad(coords, nbr, EXP, th, y)
    wide = np.concatenate([nbr, np.full((N, 3), -1, np.int32)], axis=1)  # three empty slots more: m = 12
    w = forward(coords, wide, EXP, th, y)
    assert np.all(w[0][:, 9:] == 0.0)
    assert np.all(np.abs(w[1] - base[1]) <= BF_K * U * np.abs(base[1])) and w[3][2] == -1 and w[3][3] == -1
    gw = grad(coords, wide, EXP, th, y)
    assert np.all(np.abs(gw[2] - gbase[2]) <= 1e-9 * (1 + np.abs(gbase[2])))
    bad = nbr.copy()
    bad[20, 0] = N + 5
    assert forward(coords, bad, EXP, th, y)[3][3] == 20 and grad(coords, bad, EXP, th, y)[0][3] == 20
    from pynngp_amd import nngp as NN

    model = NN.NNGP(np.array(coords), np.array(y), None, "S=T", 9, NN.GneitingCovariance(EXP, *th))
    model.set_neighbor_sets(dev(bad))
    for call in (model.loglik, model.loglik_grad, model.compute_BF, lambda: model.profile_loglik(model.cov),
                 lambda: model.gls(model.cov, np.ones((N, 1))), model.fit):
        with pytest.raises(NN.NNGPIndexError, match="index"):
            call()
    dup = np.array(coords)
    dup[31] = dup[30]
    pd = forward(dup, O.c_knn_prior(dup, 9), EXP, (1.3, 6.0, 3.0, 0.5, 0.0), y)[3]
    assert pd[2] >= 0


def test_model_paths():
    """An NNGP with a GneitingCovariance against the restatement, as tests/test_gpu_sep.py holds the separable model."""
    import pynngp_amd
    from pynngp_amd import nngp as NN

    with pytest.raises(ValueError):
        pynngp_amd.GneitingCovariance("spherical", *Gn.theta_of(0.5))
    kind, n = "matern32", 400
    rng = np.random.default_rng(21)
    t, y = rng.uniform(0.0, 1.0, (n, 3)), rng.standard_normal(n) + 0.3
    cov = pynngp_amd.GneitingCovariance(kind, *Gn.theta_of(0.5))
    th = cov.theta
    model = NN.NNGP(t, y, None, "S=T", 10, cov)
    assert np.array_equal(model.nbr.cpu().numpy(), O.c_knn_prior(scaled(t, th), 10))  # the (c, c, a) metric
    nbr = model.nbr.cpu().numpy()
    ref = Gn.rows(t, t, nbr, kind, th, y, y)
    assert ref.resolved.all()
    ll = model.loglik()
    assert abs(ll - float(ref.ll.sum())) <= 1e-11 * abs(ll)
    B, F = (a.cpu().numpy() for a in model.compute_BF())
    assert np.all(np.abs(B - ref.b).max(1) <= BF_K * U * ref.sB) and np.all(np.abs(F - ref.F) <= BF_K * U * ref.sF)
    lg, g = model.loglik_grad()
    Gs = ref.G.astype(np.float64)
    assert abs(lg - ll) <= 1e-11 * abs(ll) and np.all(np.abs(g - Gs.sum(0)) <= 1e-12 * np.abs(Gs).sum(0))
    th5 = torch.tensor(th, dtype=torch.float64, requires_grad=True)
    la = pynngp_amd.loglik_gneiting(dev(t), model._nbr_sorted, kind, th5, dev(y), order=model._order)
    la.backward()
    assert float(la.detach()) == lg and np.array_equal(th5.grad.numpy(), g)
    tq = np.random.default_rng(3).uniform(0, 1, (50, 3))
    mean, var = model.predict(values=y, query=tq)
    qn = O.knn_all(scaled(tq, th), scaled(t, th), 10).astype(np.int32)
    cref = Gn.rows(t, tq, qn, kind, th, y, None)
    assert cref.resolved.all()
    assert np.all(np.abs(mean + cref.r.astype(np.float64)) <= BF_K * U * cref.sR)
    assert np.all(np.abs(var - cref.F.astype(np.float64)) <= BF_K * U * cref.sF)
    llp, mu, gp = model.profile_loglik_grad(cov)
    assert model.profile_loglik(cov)[0] == llp
    r1 = Gn.rows(t, t, nbr, kind, th, np.ones(n), np.ones(n))
    mu_ref = float((r1.r * ref.r / ref.F).sum() / (r1.r * r1.r / ref.F).sum())
    assert abs(mu - mu_ref) <= 1e-10 * (1 + abs(mu_ref))
    rm = Gn.rows(t, t, nbr, kind, th, y - mu, y - mu)
    Gm = rm.G.astype(np.float64)
    assert abs(llp - float(rm.ll.sum())) <= 1e-11 * abs(llp)
    assert np.all(np.abs(gp - Gm.sum(0)) <= 1e-10 * np.abs(Gm).sum(0))
    # the linear mean: GLS through the whitened Gram on this sweep's B and F; the restatement at the residual
    X = np.stack([np.ones(n), t[:, 0], t[:, 2]], 1)
    res = model.gls(cov, X)
    sF = np.sqrt(ref.F.astype(np.float64))
    W = np.stack([Gn.rows(t, t, nbr, kind, th, X[:, k], X[:, k]).r.astype(np.float64) for k in range(3)], 1) / sF[:, None]
    beta = np.linalg.lstsq(W, ref.r.astype(np.float64) / sF, rcond=None)[0]
    assert np.allclose(res.beta, beta, rtol=1e-9, atol=1e-9), (res.beta, beta)
    rl = Gn.rows(t, t, nbr, kind, th, y - X @ res.beta, y - X @ res.beta)
    assert abs(res.loglik - float(rl.ll.sum())) <= 1e-11 * abs(res.loglik)
    lll, bl, gl = model.profile_loglik_grad(cov, mean="linear", X=X)
    assert lll == model.profile_loglik(cov, mean="linear", X=X)[0] and abs(lll - res.loglik) <= 1e-12 * abs(lll)
    Gl = rl.G.astype(np.float64)
    assert np.all(np.abs(gl - Gl.sum(0)) <= 1e-10 * np.abs(Gl).sum(0))
    # a linear-mean fit with beta held: the interaction keeps its own key beside the regression's beta
    out = model.fit(mean="linear", X=X, fix_beta=0.5, tol=1e-2, reneighbor=1)
    assert out["beta_st"] == 0.5 and out["theta"][3] == 0.5 and out["grad"].shape == (4,) and out["rounds"] == 2
    assert np.asarray(out["beta"]).shape == (3,) and out["loglik"] >= lll
    assert np.array_equal(model.nbr.cpu().numpy(), O.c_knn_prior(scaled(t, out["theta"]), 10))
    other = cov.replace(a=12.0)
    model.rebuild_neighbors(other)
    assert np.array_equal(model.nbr.cpu().numpy(), O.c_knn_prior(scaled(t, other.theta), 10))
    for call in (lambda: model.fit(stderr=True), lambda: model.fit(reml=True), lambda: model.fit(anisotropic=True),
                 lambda: model.fit(method="fisher"), lambda: model.fit(estimate_nu=True),
                 lambda: model.fisher_information(), lambda: model.loglik(noise=np.ones(n)),
                 lambda: model.predict(values=y, X=X, X_query=X),
                 lambda: NN.NNGP(t, y, None, ("subset", 40), 5, cov)):
        with pytest.raises(TypeError, match="GneitingCovariance"):
            call()


def test_fit():
    """The issue's simulated fit: not below the true theta's likelihood, and the gradient-free fit agrees."""
    import pynngp_amd
    from pynngp_amd import nngp as NN

    rng = np.random.default_rng(77)
    n, true = 1500, (1.0, 6.0, 3.0, 0.5, 0.1)
    s = rng.uniform(0.0, 1.0, (n, 3))
    K = Gn.cov_matrix(s, s, EXP, true) + true[4] * np.eye(n)
    y = np.linalg.cholesky(K) @ rng.standard_normal(n) + 0.7
    mod = NN.NNGP(s, y, None, "S=T", 10, pynngp_amd.GneitingCovariance(EXP, *true))
    ll_true = mod.profile_loglik(mod.cov)[0]
    out = mod.fit(x0=(0.5, 3.0, 6.0, 0.2, 0.3), tol=1e-3)
    print("fit", out["theta"], out["loglik"], ll_true, out["n_evals"], out["n_grad_evals"])
    assert out["loglik"] >= ll_true and 0.0 <= out["beta_st"] <= 1.0 and out["beta_st"] == out["theta"][3]
    mod2 = NN.NNGP(s, y, None, "S=T", 10, pynngp_amd.GneitingCovariance(EXP, *true))
    out2 = mod2.fit(x0=(0.5, 3.0, 6.0, 0.2, 0.3), gradient=False)
    print("fit nm", out2["theta"], out2["loglik"], out2["n_evals"])
    assert abs(out["loglik"] - out2["loglik"]) <= 1e-6 * abs(out2["loglik"])
