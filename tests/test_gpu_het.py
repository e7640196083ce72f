"""Per-point noise in the response model on the GPU: nngp_bf_sweep_noise / nngp_bf_cross_noise / nngp_bf_grad_noise
against the long-double restatement tests/het_ref.py (pinned on the CPU by tests/test_het_host.py), the torch ops, and
the ``noise=`` keyword of NNGP.loglik / loglik_grad / profile_loglik / fit / predict.

Bounds.  Forward and cross sweeps: bf_precision_ref.check_sweep (BF_K U scale per row on the resolved rows, the
scales with the row's largest diagonal entry; at least RESOLVED_SHARE of the rows resolved).  Gradient: each of the
three sums within 1e-12 sum |row terms| of the restatement (test_gpu_grad.py's bound); every row of G within that same
scale, and within test_gpu_grad.py's per-row rule 1e-9 (1 + |G|).
"""
import numpy as np
import pytest
import torch

import het_ref as H
from bf_precision_ref import BF_K, RESOLVED_SHARE, U, check_sweep
from oracle import nngp_oracle as O
from pynngp_amd import _lib

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared inputs are read-only


def host(*ts):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def forward(coords, nbr, kind, th, y, v, i0=0, order=None):
    return host(*_lib.bf_sweep_noise(dev(coords), nbr if torch.is_tensor(nbr) else dev(nbr), i0, kind, *th, dev(v),
                                     values=dev(y), order=order, want_r=True))


def grad(coords, nbr, kind, th, y, v, i0=0, order=None):
    return host(*_lib.bf_grad_noise(dev(coords), nbr if torch.is_tensor(nbr) else dev(nbr), i0, kind, *th, dev(y), dev(v),
                                    want_rows=True, order=order))


def check_grad(ref, p, g, G, where, rows=slice(None)):
    Gr = ref.G.astype(np.float64)[rows]
    S = np.abs(Gr).sum(0)
    err, rerr = np.abs(g - Gr.sum(0)) / S, np.abs(G - Gr).max(0) / S
    print(f"{where}: grad err / sum|G| {err}, worst row / sum|G| {rerr}, "
          f"worst row / (1 + |G|) {(np.abs(G - Gr) / (1 + np.abs(Gr))).max():.3g}")
    assert p[2] == -1 and p[3] == -1, (where, p)
    assert np.all(err <= 1e-12), (where, "sums", err)
    assert np.all(rerr <= 1e-12), (where, "rows", rerr)
    assert np.all(np.abs(G - Gr) <= 1e-9 * (1 + np.abs(Gr))), (where, "rows, relative")
    lf, q = ref.logF.astype(np.float64)[rows], ref.q.astype(np.float64)[rows]
    assert abs(p[0] - lf.sum()) <= 1e-11 * np.abs(lf).sum(), (where, p[0], lf.sum())
    assert abs(p[1] - q.sum()) <= 1e-11 * q.sum(), (where, p[1], q.sum())


# ---------------------------------------------------------------- every instantiation against the restatement
@pytest.mark.parametrize("m", H.M_LIST)
@pytest.mark.parametrize("kind", H.KINDS)
@pytest.mark.parametrize("dim", H.DIMS)
def test_sweeps_match_restatement(dim, kind, m):
    """Forward, gradient and cross sweeps of one (dim, kind, m); the first m rows carry -1 padding."""
    coords, y, _, v = H.field(dim)
    th = H.theta_of(kind)
    nbr = H.neighbours(dim, m)
    ref = H.prior_reference(dim, m, kind)
    where = f"d{dim} {kind} m{m}"
    assert ref.resolved.mean() >= RESOLVED_SHARE, (where, ref.resolved.mean())
    B, F, R, p = forward(coords, nbr, kind, th, y, v)
    check_sweep(ref, B, F, R, p, "sweep " + where)
    check_grad(ref, *grad(coords, nbr, kind, th, y, v), "grad " + where)
    q, yq, vq = H.query(dim)
    cref = H.cross_reference(dim, m, kind)
    assert cref.resolved.mean() >= RESOLVED_SHARE, (where, cref.resolved.mean())
    Bc, Fc, Rc, pc = host(*_lib.bf_cross_noise(dev(coords), dev(q), dev(H.query_neighbours(dim, m)), kind, *th, dev(v),
                                               noise_query=dev(vq), ref_values=dev(y), query_values=dev(yq),
                                               want_r=True))
    check_sweep(cref, Bc, Fc, Rc, pc, "cross " + where)


@pytest.mark.parametrize("m", [3, 15, 18, 32])
def test_zero_weights(m):
    """Every 7th point is known exactly (v = 0) while tau2 > 0 elsewhere."""
    coords, y, _, v = H.field(2, zeros=True)
    th = H.theta_of("exponential")
    ref = H.prior_reference(2, m, "exponential", True)
    assert ref.resolved.mean() >= RESOLVED_SHARE
    nbr = H.neighbours(2, m)
    check_sweep(ref, *forward(coords, nbr, "exponential", th, y, v), f"zeros m{m}")
    check_grad(ref, *grad(coords, nbr, "exponential", th, y, v), f"zeros grad m{m}")


def test_cross_default_query_weight():
    """noise_query = NULL is the weight 1 on the query point's own diagonal entry; no values: R is not written."""
    coords, y, _, v = H.field(2)
    q, _, _ = H.query(2)
    th = H.theta_of("matern32")
    nbr = H.query_neighbours(2, 15)
    ref = H.rows(coords, q, nbr, "matern32", th, y, None, v, None)
    B, F, R, p = host(*_lib.bf_cross_noise(dev(coords), dev(q), dev(nbr), "matern32", *th, dev(v), ref_values=dev(y),
                                           want_r=True))
    check_sweep(ref, B, F, R, p, "cross, default weight")


# ---------------------------------------------------------------- layouts, sub-ranges, flags
def test_row_order_layout_and_subrange():
    coords, y, _, v = H.field(2)
    th = H.theta_of("matern52")
    i0, n = 137, 301
    sub = np.ascontiguousarray(H.neighbours(2, 17)[i0:i0 + n])
    ref = H.rows(coords, coords[i0:i0 + n], sub, "matern52", th, y, y[i0:], v, v[i0:])
    B, F, R, p = forward(coords, sub, "matern52", th, y, v, i0=i0)
    check_sweep(ref, B, F, R, p, "sub-range", i0=i0)
    pg, g, G = grad(coords, sub, "matern52", th, y, v, i0=i0)
    check_grad(ref, pg, g, G, "sub-range grad")
    order, nbr_sorted = _lib.row_order(dev(coords), i0, n, dev(sub))
    B2, F2, R2, p2 = forward(coords, nbr_sorted, "matern52", th, y, v, i0=i0, order=order)
    # only the visiting order changes: the rows bit for bit, the fold to the sweep's bound
    assert np.array_equal(B2, B) and np.array_equal(F2, F) and np.array_equal(R2, R)
    check_sweep(ref, B2, F2, R2, p2, "row_order layout", i0=i0)
    pg2, g2, G2 = grad(coords, nbr_sorted, "matern52", th, y, v, i0=i0, order=order)
    assert np.array_equal(G2, G)
    check_grad(ref, pg2, g2, G2, "row_order grad")


def test_bad_index_flag():
    coords, y, _, v = H.field(2)
    th = H.theta_of("exponential")
    nbr = H.neighbours(2, 8).copy()
    nbr[321, 3] = H.N  # one past the end
    B, F, R, p = forward(coords, nbr, "exponential", th, y, v)
    assert p[3] == 321 and p[2] == -1
    assert np.all(np.isfinite(B)) and np.all(np.isfinite(F))
    pg, g, G = grad(coords, nbr, "exponential", th, y, v)
    assert pg[3] == 321 and pg[2] == -1 and np.all(np.isfinite(G))
    keep = np.arange(H.N) != 321
    ref = H.prior_reference(2, 8, "exponential")
    assert np.all(np.abs(B - ref.b)[keep].max(1) <= BF_K * U * ref.sB[keep])


def test_not_pd_flag():
    """Two coincident points known exactly (v = 0): every block that holds both is singular."""
    coords, y, _, v = (a.copy() for a in H.field(2))
    coords[50] = coords[49]
    v[49] = v[50] = 0.0
    nbr = O.c_knn_prior(coords, 5)
    th = H.theta_of("exponential")
    B, F, R, p = forward(coords, nbr, "exponential", th, y, v)
    bad = int(p[2])
    assert bad >= 50 and p[3] == -1
    assert np.isnan(F[bad]) and np.all(np.isnan(B[bad])) and np.isnan(R[bad])
    assert np.all(np.isfinite(F[:50]))
    pg, g, G = grad(coords, nbr, "exponential", th, y, v)
    assert pg[2] == bad and np.all(np.isnan(G[bad]))


# ---------------------------------------------------------------- v = 1 against the homoscedastic twins
@pytest.mark.parametrize("m", [7, 15, 18, 31])
def test_unit_weights_against_twins(m):
    coords, y, _, _ = H.field(2)
    one = np.ones(H.N)
    kind, th = "matern32", H.theta_of("matern32")
    nbr = H.neighbours(2, m)
    ref = H.rows(coords, coords, nbr, kind, th, y, y, one, one)
    B, F, R, p = forward(coords, nbr, kind, th, y, one)
    Rt = torch.empty(H.N, dtype=torch.float64, device="cuda")
    Bt, Ft, pt = _lib.bf_sweep(dev(coords), dev(nbr), 0, kind, *th, values=dev(y), R=Rt)
    Bt, Ft, Rt, pt = host(Bt, Ft, Rt, pt)
    print(f"m{m}: sweep bit-identical to nngp_bf_sweep: {np.array_equal(B, Bt) and np.array_equal(F, Ft)}")
    ok = ref.resolved
    assert np.all(np.abs(B - Bt).max(1)[ok] <= BF_K * U * ref.sB[ok])
    assert np.all(np.abs(F - Ft)[ok] <= BF_K * U * ref.sF[ok])
    assert np.all(np.abs(R - Rt)[ok] <= BF_K * U * ref.sR[ok])
    q, yq, _ = H.query(2)
    qn = H.query_neighbours(2, m)
    cref = H.rows(coords, q, qn, kind, th, y, yq, one, None)
    Bc, Fc, Rc, _ = host(*_lib.bf_cross_noise(dev(coords), dev(q), dev(qn), kind, *th, dev(one), ref_values=dev(y),
                                              query_values=dev(yq), want_r=True))
    Rx = torch.empty(len(q), dtype=torch.float64, device="cuda")
    Bx, Fx, _ = _lib.bf_cross(dev(coords), dev(q), dev(qn), kind, *th, ref_values=dev(y), query_values=dev(yq), R=Rx)
    Bx, Fx, Rx = host(Bx, Fx, Rx)
    ok = cref.resolved
    assert np.all(np.abs(Bc - Bx).max(1)[ok] <= BF_K * U * cref.sB[ok])
    assert np.all(np.abs(Fc - Fx)[ok] <= BF_K * U * cref.sF[ok])
    assert np.all(np.abs(Rc - Rx)[ok] <= BF_K * U * cref.sR[ok])
    pg, g, G = grad(coords, nbr, kind, th, y, one)
    p0, g0, G0 = host(*_lib.bf_grad(dev(coords), dev(nbr), 0, kind, *th, dev(y), want_rows=True))
    print(f"m{m}: gradient bit-identical to nngp_bf_grad: {np.array_equal(G, G0) and np.array_equal(g, g0)}")
    assert np.all(np.abs(g - g0) <= 1e-12 * np.abs(ref.G.astype(np.float64)).sum(0))


# ---------------------------------------------------------------- known answers, reproducibility
def make_model(n, m, kind="exponential", seed=21, dim=2, eps="array", **kw):
    from pynngp_amd import nngp as N

    rng = np.random.default_rng(seed)
    t = rng.uniform(0.0, 1.0, (n, dim))
    y = rng.standard_normal(n) + 0.3
    e = np.exp(rng.uniform(np.log(0.2), np.log(5.0), n))
    th = H.theta_of(kind)
    return N.NNGP(t, y, e if eps == "array" else eps, kw.pop("refType", "S=T"), m, N.Covariance(kind, *th), **kw), t, y, e


@pytest.mark.parametrize("n", [33, 20])
def test_dense_known_answer(n):
    """m = n - 1: NNGP.loglik(noise=e) is the dense N(0, sigma2 R + tau2 diag(e^2)) density."""
    for kind in ("exponential", "gaussian"):
        model, t, y, e = make_model(n, n - 1, kind)
        ll, g = H.dense_loglik_grad(t, kind, H.theta_of(kind), y, e * e)
        got = model.loglik(noise=e)
        assert abs(got - ll) <= 1e-10 * abs(ll), (kind, got, ll)
        ll2, g2 = model.loglik_grad(noise=e)
        assert abs(ll2 - ll) <= 1e-10 * abs(ll)
        assert np.allclose(g2, g, rtol=1e-8, atol=1e-8), (kind, g2, g)


def test_reproducible_bits():
    coords, y, _, v = H.field(3)
    th = H.theta_of("gaussian")
    nbr = H.neighbours(3, 24)
    a, b = forward(coords, nbr, "gaussian", th, y, v), forward(coords, nbr, "gaussian", th, y, v)
    assert all(np.array_equal(x, z, equal_nan=True) for x, z in zip(a, b))
    a, b = grad(coords, nbr, "gaussian", th, y, v), grad(coords, nbr, "gaussian", th, y, v)
    assert all(np.array_equal(x, z, equal_nan=True) for x, z in zip(a, b))


# ---------------------------------------------------------------- the keyword and the torch ops
def test_keyword_none_eps_array_and_ordering():
    from pynngp_amd import nngp as N

    model, t, y, e = make_model(400, 10)
    assert model.loglik(noise=None) == model.loglik()
    assert np.array_equal(model.loglik_grad(noise=None)[1], model.loglik_grad()[1])
    assert model.profile_loglik(model.cov, noise=None) == model.profile_loglik(model.cov)
    ll = model.loglik(noise="eps")
    assert ll == model.loglik(noise=e) and ll != model.loglik()
    assert model.profile_loglik(model.cov, noise="eps") == model.profile_loglik(model.cov, noise=e)
    lg, gg = model.loglik_grad(noise="eps")
    assert lg == model.loglik_grad(noise=e)[0] and abs(lg - ll) <= 1e-11 * abs(ll)
    # the profiled mean and the envelope gradient against the restatement's log-likelihood at y - mu
    llp, mu, gp = model.profile_loglik_grad(model.cov, noise=e)
    nbr = model.nbr.cpu().numpy()
    ref = H.rows(t, t, nbr, "exponential", model.cov.theta[:3], y - mu, y - mu, e * e, e * e)
    assert abs(llp - float(ref.ll.sum())) <= 1e-11 * abs(llp)
    assert np.all(np.abs(gp - ref.G.astype(np.float64).sum(0)) <= 1e-10 * np.abs(ref.G.astype(np.float64)).sum(0))
    # a scalar or missing eps
    for bad in (None, 0.3):
        with pytest.raises(ValueError):
            make_model(50, 5, eps=bad)[0].loglik(noise="eps")
    # ordering= permutes eps with t and y: the instance built from the permuted inputs is the same model
    a = N.NNGP(t, y, e, "S=T", 10, model.cov, ordering="maxmin")
    perm = a.perm.cpu().numpy()
    b = N.NNGP(t[perm], y[perm], e[perm], "S=T", 10, model.cov)
    la, lb = a.loglik(noise="eps"), b.loglik(noise="eps")
    assert abs(la - lb) <= 1e-12 * abs(lb), (la, lb)
    assert la == a.loglik(noise=e[perm])


def test_refusals():
    from pynngp_amd import nngp as N

    model, t, y, e = make_model(120, 6)
    cov = model.cov
    calls = [
        lambda: model.fisher_information(noise=e),
        lambda: model.fit(noise=e, stderr=True),
        lambda: model.fit(noise=e, method="fisher"),
        lambda: model.fit(noise=e, anisotropic=True),
        lambda: model.fit(noise=e, kind="matern", nu=1.3),
        lambda: model.loglik(noise=e, cov=N.Covariance("matern", 1.0, 6.0, 0.05, nu=1.3)),
        lambda: model.loglik_grad(noise=e, cov=N.MaternCovariance(1.0, 6.0, 0.05, nu=1.3)),
        lambda: model.loglik(noise=e, cov=N.AnisotropicCovariance("exponential", 1.0, (5.0, 7.0), 0.05)),
        lambda: model.profile_loglik(cov, mean="linear", X=np.ones((120, 1)), noise=e),
        lambda: model.profile_loglik_grad(cov, mean="linear", X=np.ones((120, 1)), noise=e),
        lambda: model.fit(noise=e, mean="linear", X=np.ones((120, 1))),
        lambda: model.gls(cov, np.ones((120, 1)), noise=e),
        lambda: model.conjugate("exponential", 6.0, 0.1, np.ones((120, 1)), noise=e),
        lambda: model.predict(values=y, X=np.ones((120, 1)), X_query=np.ones((120, 1)), noise=e),
        lambda: model.loglik(noise=e, cov=lambda a, b: np.exp(-np.linalg.norm(a - b))),
        lambda: make_model(120, 6, refType=("subset", 40))[0].loglik(noise=e),
    ]
    for k, call in enumerate(calls):
        with pytest.raises(NotImplementedError, match="noise="):
            call()
            pytest.fail(f"call {k} was not refused")
    for bad in (np.ones(119), -np.ones(120), np.full(120, np.nan), "sigma"):
        with pytest.raises(ValueError):
            model.loglik(noise=bad)


def test_torch_ops_match_ctypes():
    from pynngp_amd import load_ops

    ops = load_ops()
    coords, y, _, v = H.field(2)
    th = H.theta_of("spherical")
    k = ops.kind_code("spherical")
    c, nb, yy, vv = dev(coords), dev(H.neighbours(2, 16)), dev(y), dev(v)
    B, F, R, p = torch.ops.nngp.bf_sweep_noise(c, nb, None, 0, k, *th, yy, vv, True)
    B2, F2, R2, p2 = _lib.bf_sweep_noise(c, nb, 0, "spherical", *th, vv, values=yy, want_r=True)
    assert all(torch.equal(a, b) for a, b in ((B, B2), (F, F2), (R, R2), (p, p2)))
    pg, g, G = torch.ops.nngp.bf_grad_noise(c, nb, None, 0, k, *th, yy, vv, True)
    pg2, g2, G2 = _lib.bf_grad_noise(c, nb, 0, "spherical", *th, yy, vv, want_rows=True)
    assert torch.equal(pg, pg2) and torch.equal(g, g2) and torch.equal(G, G2)
    q, _, vq = H.query(2)
    qd, qn, vqd = dev(q), dev(H.query_neighbours(2, 16)), dev(vq)
    Bc, Fc, mean = torch.ops.nngp.bf_cross_noise(c, qd, qn, k, *th, yy, vv, vqd)
    Bc2, Fc2, Rc2, _ = _lib.bf_cross_noise(c, qd, qn, "spherical", *th, vv, noise_query=vqd, ref_values=yy, want_r=True)
    assert torch.equal(Bc, Bc2) and torch.equal(Fc, Fc2) and torch.equal(mean, -Rc2)
    with pytest.raises(RuntimeError):
        torch.ops.nngp.bf_sweep_noise(c.cpu(), nb.cpu(), None, 0, k, *th, yy.cpu(), vv.cpu(), True)
    # autograd: the gradient in theta is the sweep's, none flows to the noise
    import pynngp_amd

    theta = torch.tensor(th, dtype=torch.float64, requires_grad=True)
    e = dev(np.sqrt(v))
    ll = pynngp_amd.loglik(c, nb, theta, yy, "spherical", noise=e)
    ll.backward()
    pn, gn, _ = _lib.bf_grad_noise(c, nb, 0, "spherical", *th, yy, e * e)
    assert torch.equal(theta.grad, gn.cpu())


# ---------------------------------------------------------------- fit and predict
@pytest.fixture(scope="module")
def simulated():
    """n = 1500 + 50 held-out points in 2-D, exponential, sigmas in {0.2, 2.0}, simulated at tau2 = 1."""
    rng = np.random.default_rng(2024)
    n, hold = 1500, 50
    t = rng.uniform(0.0, 1.0, (n + hold, 2))
    e = np.where(rng.uniform(size=n + hold) < 0.5, 0.2, 2.0)
    theta = (1.0, 6.0, 1.0)
    d = np.sqrt(((t[:, None, :] - t[None, :, :]) ** 2).sum(-1))
    K = theta[0] * np.exp(-theta[1] * d) + theta[2] * np.diag(e * e)
    y = 0.5 + np.linalg.cholesky(K) @ rng.standard_normal(n + hold)
    return t[:n], y[:n], e[:n], t[n:], theta


def test_fit_and_predict(simulated):
    from pynngp_amd import nngp as N

    t, y, e, tq, theta = simulated
    tol = 1e-6
    model = N.NNGP(t, y, e, "S=T", 10, N.Covariance("exponential", 0.5, 3.0, 1.0))
    ll_true = model.profile_loglik(N.Covariance("exponential", *theta), noise="eps")[0]
    res = model.fit(noise="eps", fix_tau2=1.0, gradient=True, tol=tol)
    rel = float(np.abs(res["grad"]).max() / max(1.0, abs(res["loglik"])))
    print("gradient fit:", res["theta"], res["loglik"], "grad", res["grad"], "relative", rel, "evals", res["n_evals"])
    assert res["converged"] and res["theta"][2] == 1.0
    assert rel < tol, (res["grad"], rel)
    assert res["loglik"] >= ll_true, (res["loglik"], ll_true)
    model2 = N.NNGP(t, y, e, "S=T", 10, N.Covariance("exponential", 0.5, 3.0, 1.0))
    free = model2.fit(noise="eps", fix_tau2=1.0)
    print("derivative-free fit:", free["theta"], free["loglik"], "evals", free["n_evals"])
    for k in (0, 1):
        assert abs(free["theta"][k] - res["theta"][k]) <= 1e-3 * res["theta"][k], (k, free["theta"], res["theta"])
    # the free-tau2 fit rescales the error bars: it runs and does no worse
    both = model2.fit(noise="eps", gradient=True, tol=tol)
    print("free tau2:", both["theta"], both["loglik"])
    assert both["loglik"] >= res["loglik"] - 1e-9 * abs(res["loglik"])
    # kriging at the held-out points against the restatement (the predicted point's own weight 1)
    th, mu = res["theta"], res["mu"]
    mean, var = model.predict(values=y - mu, cov=N.Covariance("exponential", *th), query=tq, noise="eps")
    nbr = O.knn_all(tq, t, 10).astype(np.int32)
    ref = H.rows(t, tq, nbr, "exponential", th, y - mu, None, e * e, None)
    assert ref.resolved.all()
    assert np.all(np.abs(mean + ref.r.astype(np.float64)) <= BF_K * U * ref.sR)
    assert np.all(np.abs(var - ref.F.astype(np.float64)) <= BF_K * U * ref.sF)
    # noise_query sets the predicted point's own weight: var moves by tau2 (v_q - 1) exactly in the model
    _, var0 = model.predict(values=y - mu, cov=N.Covariance("exponential", *th), query=tq, noise="eps",
                            noise_query=np.zeros(len(tq)))
    assert np.allclose(var - var0, th[2], rtol=0, atol=1e-12 * (th[0] + th[2]) * 100)
