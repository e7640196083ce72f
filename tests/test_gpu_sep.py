"""The separable space-time covariance on the GPU: nngp_bf_sweep_sep / nngp_bf_cross_sep / nngp_bf_grad_sep against the
long-double restatement tests/sep_ref.py (pinned on the CPU by tests/test_sep_host.py), the torch ops, and an NNGP built
with a SeparableCovariance (loglik, compute_BF, predict, profile_loglik, gls, loglik_grad, fit).

Bounds (the family's, from test_gpu_het.py).  Forward and cross sweeps: bf_precision_ref.check_sweep (BF_K U scale per
row on the resolved rows).  Gradient: every row of G within 1e-9 (1 + |G|) of the restatement, each of the four sums
within 1e-12 sum |row terms|, partials[0:2] within 1e-11 of sum |terms|.
"""
import numpy as np
import pytest
import torch

import sep_ref as S
from bf_precision_ref import BF_K, RESOLVED_SHARE, U, check_sweep
from oracle import nngp_oracle as O
from pynngp_amd import _lib

pytestmark = pytest.mark.gpu
PAIRS = [(a, b) for a in S.KINDS for b in S.KINDS]
EE = ("exponential", "exponential")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared inputs are read-only


def host(*ts):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def forward(coords, nbr, ks, kt, th, y, i0=0, order=None):
    return host(*_lib.bf_sweep_sep(dev(coords), nbr if torch.is_tensor(nbr) else dev(nbr), i0, ks, kt, *th,
                                   values=dev(y), order=order, want_r=True))


def grad(coords, nbr, ks, kt, th, y, i0=0, order=None):
    return host(*_lib.bf_grad_sep(dev(coords), nbr if torch.is_tensor(nbr) else dev(nbr), i0, ks, kt, *th, dev(y),
                                  want_rows=True, order=order))


def cross(coords, q, nbr, ks, kt, th, y, yq):
    return host(*_lib.bf_cross_sep(dev(coords), dev(q), dev(nbr), ks, kt, *th, ref_values=dev(y),
                                   query_values=None if yq is None else dev(yq), want_r=True))


def check_grad(ref, p, g, G, where, rows=slice(None)):
    Gr = ref.G.astype(np.float64)[rows]
    Sm = np.abs(Gr).sum(0)
    err = np.abs(g - Gr.sum(0))
    print(f"{where}: grad err {err}, sum|G| {Sm}, worst row / (1 + |G|) "
          f"{(np.abs(G - Gr) / (1 + np.abs(Gr))).max():.3g}")
    assert p[2] == -1 and p[3] == -1, (where, p)
    assert G.shape == Gr.shape and g.shape == (4,)
    assert np.all(err <= 1e-12 * Sm), (where, "sums", err, Sm)
    assert np.all(np.abs(G - Gr) <= 1e-9 * (1 + np.abs(Gr))), (where, "rows")
    lf, q = ref.logF.astype(np.float64)[rows], ref.q.astype(np.float64)[rows]
    assert abs(p[0] - lf.sum()) <= 1e-11 * np.abs(lf).sum(), (where, p[0], lf.sum())
    assert abs(p[1] - q.sum()) <= 1e-11 * q.sum(), (where, p[1], q.sum())


def one_case(dim, ks, kt, m):
    coords, y = S.field(dim)
    th = S.theta_of(ks, kt)
    nbr = S.neighbours(dim, m)
    ref = S.prior_reference(dim, m, ks, kt)
    where = f"d{dim} {ks} x {kt} m{m}"
    assert ref.resolved.mean() >= RESOLVED_SHARE, (where, ref.resolved.mean())
    check_sweep(ref, *forward(coords, nbr, ks, kt, th, y), "sweep " + where)
    check_grad(ref, *grad(coords, nbr, ks, kt, th, y), "grad " + where)
    q, yq = S.query(dim)
    cref = S.cross_reference(dim, m, ks, kt)
    assert cref.resolved.mean() >= RESOLVED_SHARE, (where, cref.resolved.mean())
    check_sweep(cref, *cross(coords, q, S.query_neighbours(dim, m), ks, kt, th, y, yq), "cross " + where)


# ---------------------------------------------------------------- every instantiation against the restatement
@pytest.mark.parametrize("m", S.M_ALL)
def test_every_m(m):
    """Forward, gradient and cross sweeps of exponential x exponential at every m; the first m rows carry -1 padding."""
    one_case(3, *EE, m)


@pytest.mark.parametrize("m", S.M_EDGES)
@pytest.mark.parametrize("ks,kt", PAIRS)
def test_every_kind_pair(ks, kt, m):
    one_case(3, ks, kt, m)


@pytest.mark.parametrize("m", [7, 15, 20, 32])
@pytest.mark.parametrize("ks,kt", [EE, ("matern52", "spherical"), ("gaussian", "matern32")])
def test_two_columns(ks, kt, m):
    """dim 2: one spatial column, then time."""
    one_case(2, ks, kt, m)


# ---------------------------------------------------------------- identities against the sibling sweeps
@pytest.mark.parametrize("m", [8, 15, 23, 32])
def test_gaussian_product_against_the_metric_sweeps(m):
    """gaussian x gaussian is the per-axis model: nngp_bf_grad_aniso at phi = (phi_s, phi_s, phi_t) (the phi_s entry the
    sum of the spatial axes') and the phi = 1 sweep on the scaled coordinates.  To the bounds, not bit for bit."""
    coords, y = S.field(3)
    th = (1.3, 2.5, 1.1, 0.05)
    nbr = S.neighbours(3, m)
    ref = S.rows(coords, coords, nbr, "gaussian", "gaussian", th, y, y)
    ok = ref.resolved
    assert ok.mean() >= RESOLVED_SHARE
    B, F, R, p = forward(coords, nbr, "gaussian", "gaussian", th, y)
    check_sweep(ref, B, F, R, p, f"gaussian m{m}")
    Rt = torch.empty(S.N, dtype=torch.float64, device="cuda")
    Bt, Ft, _ = _lib.bf_sweep(dev(S.scaled(coords, th)), dev(nbr), 0, "gaussian", th[0], 1.0, th[3], values=dev(y), R=Rt)
    Bt, Ft, Rt = host(Bt, Ft, Rt)
    # the sibling sweeps against each other at the family's own bounds, as test_gpu_het.py compares its twins
    assert np.all(np.abs(B - Bt).max(1)[ok] <= BF_K * U * ref.sB[ok])
    assert np.all(np.abs(F - Ft)[ok] <= BF_K * U * ref.sF[ok])
    assert np.all(np.abs(R - Rt)[ok] <= BF_K * U * ref.sR[ok])
    pg, g, G = grad(coords, nbr, "gaussian", "gaussian", th, y)
    check_grad(ref, pg, g, G, f"gaussian grad m{m}")
    pa, ga, Ga = host(*_lib.bf_grad_aniso(dev(coords), dev(nbr), 0, "gaussian", th[0], (th[1], th[1], th[2]), th[3],
                                          dev(y), want_rows=True))
    Gm = np.stack([Ga[:, 0], Ga[:, 1] + Ga[:, 2], Ga[:, 3], Ga[:, 4]], axis=1)
    assert np.all(np.abs(G - Gm) <= 1e-9 * (1 + np.abs(Gm)))
    gm = np.array([ga[0], ga[1] + ga[2], ga[3], ga[4]])
    assert np.all(np.abs(g - gm) <= 1e-12 * np.abs(ref.G.astype(np.float64)).sum(0))


@pytest.mark.parametrize("m", [8, 15, 23, 32])
@pytest.mark.parametrize("ks", ["exponential", "matern52", "spherical"])
def test_constant_time_against_the_noise_sweeps(ks, m):
    """All times equal: the spatial model, i.e. nngp_bf_sweep_noise / nngp_bf_grad_noise at v = 1 on the spatial
    columns, and the phi_t column exactly 0.  To the bounds, not bit for bit."""
    coords, y = (a.copy() for a in S.field(3))
    coords[:, 2] = 0.37
    th = S.theta_of(ks, "matern32")
    nbr = S.neighbours(3, m)
    ref = S.rows(coords, coords, nbr, ks, "matern32", th, y, y)
    ok = ref.resolved
    assert ok.mean() >= RESOLVED_SHARE
    B, F, R, p = forward(coords, nbr, ks, "matern32", th, y)
    check_sweep(ref, B, F, R, p, f"constant time {ks} m{m}")
    one = dev(np.ones(S.N))
    sp = dev(coords[:, :2])
    Bn, Fn, Rn, _ = host(*_lib.bf_sweep_noise(sp, dev(nbr), 0, ks, th[0], th[1], th[3], one, values=dev(y), want_r=True))
    assert np.all(np.abs(B - Bn).max(1)[ok] <= BF_K * U * ref.sB[ok])
    assert np.all(np.abs(F - Fn)[ok] <= BF_K * U * ref.sF[ok])
    assert np.all(np.abs(R - Rn)[ok] <= BF_K * U * ref.sR[ok])
    pg, g, G = grad(coords, nbr, ks, "matern32", th, y)
    check_grad(ref, pg, g, G, f"constant time grad {ks} m{m}")
    assert np.all(G[:, 2] == 0.0) and g[2] == 0.0
    pn, gn, Gn = host(*_lib.bf_grad_noise(sp, dev(nbr), 0, ks, th[0], th[1], th[3], dev(y), one, want_rows=True))
    assert np.all(np.abs(G[:, [0, 1, 3]] - Gn) <= 1e-9 * (1 + np.abs(Gn)))
    assert np.all(np.abs(g[[0, 1, 3]] - gn) <= 1e-12 * np.abs(ref.G.astype(np.float64)).sum(0)[[0, 1, 3]])


def test_coincident_in_one_factor():
    """Pairs that coincide in space only (or in time only): that factor's derivative is exactly 0 for the pair, and the
    rows still match the restatement."""
    coords, y = (a.copy() for a in S.field(3))
    coords[1::2, :2] = coords[0::2, :2]  # pairs at one site, different times
    coords[40:60, 2] = coords[40, 2]     # twenty points at one time
    th = S.theta_of(*EE)
    nbr = O.c_knn_prior(coords, 9)
    ref = S.rows(coords, coords, nbr, *EE, th, y, y)
    assert ref.resolved.mean() >= RESOLVED_SHARE
    check_sweep(ref, *forward(coords, nbr, *EE, th, y), "coincident")
    check_grad(ref, *grad(coords, nbr, *EE, th, y), "coincident grad")


# ---------------------------------------------------------------- known answers, folds, layouts
def make_model(n, m, ks="exponential", kt="exponential", seed=21, dim=3, theta=None, **kw):
    from pynngp_amd import nngp as N

    rng = np.random.default_rng(seed)
    t = rng.uniform(0.0, 1.0, (n, dim))
    y = rng.standard_normal(n) + 0.3
    th = S.theta_of(ks, kt) if theta is None else theta
    return N.NNGP(t, y, None, kw.pop("refType", "S=T"), m, N.SeparableCovariance(ks, kt, *th), **kw), t, y


@pytest.mark.parametrize("ks,kt", [EE, ("gaussian", "matern32"), ("spherical", "matern52")])
def test_dense_known_answer(ks, kt):
    """n = 33, m = 32: NNGP.loglik is the dense Gaussian log density under the product covariance."""
    model, t, y = make_model(33, 32, ks, kt)
    ll = S.dense_loglik(t, ks, kt, S.theta_of(ks, kt), y)
    got = model.loglik()
    assert abs(got - ll) <= 1e-10 * abs(ll), (got, ll)
    ll2, g2 = model.loglik_grad()
    assert abs(ll2 - ll) <= 1e-10 * abs(ll) and g2.shape == (4,)
    # the gradient against central differences of the dense density (h = 1e-6 theta: truncation ~1e-11 relative)
    th = S.theta_of(ks, kt)
    for k in range(4):
        tp, tm = list(th), list(th)
        tp[k], tm[k] = th[k] * (1 + 1e-6), th[k] * (1 - 1e-6)
        fd = (S.dense_loglik(t, ks, kt, tp, y) - S.dense_loglik(t, ks, kt, tm, y)) / (2e-6 * th[k])
        assert abs(fd - g2[k]) <= 1e-6 * max(1.0, abs(g2[k])), (k, fd, g2[k])


@pytest.fixture(scope="module")
def big():
    """n = 3000, m = 10 (more than one block of every lane-group width in use), with its restatement."""
    coords, y = S.field(3, 3000)
    nbr = S.neighbours(3, 10, 3000)
    th = S.theta_of(*EE)
    return coords, y, nbr, th, S.rows(coords, coords, nbr, *EE, th, y, y)


def test_two_calls_give_equal_bits(big):
    coords, y, nbr, th, ref = big
    a, b = forward(coords, nbr, *EE, th, y), forward(coords, nbr, *EE, th, y)
    assert all(np.array_equal(x, z, equal_nan=True) for x, z in zip(a, b))
    check_sweep(ref, *a, "n = 3000")
    a, b = grad(coords, nbr, *EE, th, y), grad(coords, nbr, *EE, th, y)
    assert all(np.array_equal(x, z, equal_nan=True) for x, z in zip(a, b))
    check_grad(ref, *a, "n = 3000 grad")


def test_subranges_concatenate(big):
    coords, y, nbr, th, ref = big
    B, F, R, _ = forward(coords, nbr, *EE, th, y)
    _, _, G = grad(coords, nbr, *EE, th, y)
    cuts = (0, 137, 1501, 3000)
    parts = [forward(coords, np.ascontiguousarray(nbr[a:b]), *EE, th, y, i0=a) for a, b in zip(cuts, cuts[1:])]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), B)
    assert np.array_equal(np.concatenate([p[1] for p in parts]), F)
    assert np.array_equal(np.concatenate([p[2] for p in parts]), R)
    gparts = [grad(coords, np.ascontiguousarray(nbr[a:b]), *EE, th, y, i0=a) for a, b in zip(cuts, cuts[1:])]
    assert np.array_equal(np.concatenate([p[2] for p in gparts]), G)
    a, b = cuts[1], cuts[2]
    check_grad(ref, *gparts[1], "sub-range grad", rows=slice(a, b))


def test_row_order_layout(big):
    coords, y, nbr, th, ref = big
    B, F, R, _ = forward(coords, nbr, *EE, th, y)
    _, _, G = grad(coords, nbr, *EE, th, y)
    order, nbr_sorted = _lib.row_order(dev(coords), 0, len(coords), dev(nbr))
    B2, F2, R2, p2 = forward(coords, nbr_sorted, *EE, th, y, order=order)
    assert np.array_equal(B2, B) and np.array_equal(F2, F) and np.array_equal(R2, R)
    check_sweep(ref, B2, F2, R2, p2, "row_order layout")
    pg2, g2, G2 = grad(coords, nbr_sorted, *EE, th, y, order=order)
    assert np.array_equal(G2, G)
    check_grad(ref, pg2, g2, G2, "row_order grad")


# ---------------------------------------------------------------- masks and flags
def test_empty_slot_contributes_nothing():
    """A -1 slot in the middle of a row: the row is the one with that neighbour removed, B there exactly 0."""
    coords, y = S.field(3)
    th = S.theta_of("matern32", "gaussian")
    nbr = S.neighbours(3, 9).copy()
    nbr[20:, 4] = -1
    ref = S.rows(coords, coords, nbr, "matern32", "gaussian", th, y, y)
    B, F, R, p = forward(coords, nbr, "matern32", "gaussian", th, y)
    check_sweep(ref, B, F, R, p, "-1 slot")
    assert np.all(B[20:, 4] == 0.0)
    check_grad(ref, *grad(coords, nbr, "matern32", "gaussian", th, y), "-1 slot grad")


def test_bad_index_flag():
    from pynngp_amd import nngp as N

    coords, y = S.field(3)
    th = S.theta_of(*EE)
    nbr = S.neighbours(3, 8).copy()
    nbr[61, 3] = S.N  # one past the end
    B, F, R, p = forward(coords, nbr, *EE, th, y)
    assert p[3] == 61 and p[2] == -1
    assert np.all(np.isfinite(B)) and np.all(np.isfinite(F)) and B[61, 3] == 0.0
    pg, g, G = grad(coords, nbr, *EE, th, y)
    assert pg[3] == 61 and pg[2] == -1 and np.all(np.isfinite(G))
    ref = S.rows(coords, coords, nbr, *EE, th, y, y)  # the restatement masks the slot the same way
    assert np.all(np.abs(B - ref.b).max(1) <= BF_K * U * ref.sB)
    assert np.all(np.abs(G - ref.G.astype(np.float64)) <= 1e-9 * (1 + np.abs(ref.G.astype(np.float64))))
    model = N.NNGP(coords.copy(), y.copy(), None, "S=T", 8, N.SeparableCovariance(*EE, *th))
    model.set_neighbor_sets(dev(nbr))
    for call in (model.loglik, model.loglik_grad, model.compute_BF, lambda: model.profile_loglik(model.cov),
                 lambda: model.gls(model.cov, np.ones((S.N, 1))), model.fit):
        with pytest.raises(N.NNGPNumericalError, match="index"):
            call()


def test_not_pd_flag():
    """Two coincident points (in space and time) with tau2 = 0: every block that holds both is singular."""
    from pynngp_amd import nngp as N

    coords, y = (a.copy() for a in S.field(3))
    coords[50] = coords[49]
    th = (1.3, 6.0, 3.0, 0.0)
    nbr = O.c_knn_prior(coords, 5)
    B, F, R, p = forward(coords, nbr, *EE, th, y)
    bad = int(p[2])
    assert bad >= 50 and p[3] == -1
    assert np.isnan(F[bad]) and np.all(np.isnan(B[bad])) and np.isnan(R[bad])
    assert np.all(np.isfinite(F[:50]))
    pg, g, G = grad(coords, nbr, *EE, th, y)
    assert pg[2] == bad and np.all(np.isnan(G[bad]))
    model = N.NNGP(coords, y, None, "S=T", 5, N.SeparableCovariance(*EE, *th))
    for call in (model.loglik, model.loglik_grad):
        with pytest.raises(N.NNGPNumericalError):
            call()


# ---------------------------------------------------------------- the torch ops and autograd
def test_torch_ops_match_ctypes():
    import pynngp_amd
    from pynngp_amd import load_ops

    ops = load_ops()
    coords, y = S.field(3)
    ks, kt = "spherical", "matern32"
    th = S.theta_of(ks, kt)
    k1, k2 = ops.kind_code(ks), ops.kind_code(kt)
    c, nb, yy = dev(coords), dev(S.neighbours(3, 16)), dev(y)
    B, F, R, p = torch.ops.nngp.bf_sweep_sep(c, nb, None, 0, k1, k2, *th, yy, True)
    B2, F2, R2, p2 = _lib.bf_sweep_sep(c, nb, 0, ks, kt, *th, values=yy, want_r=True)
    assert all(torch.equal(a, b) for a, b in ((B, B2), (F, F2), (R, R2), (p, p2)))
    pg, g, G = torch.ops.nngp.bf_grad_sep(c, nb, None, 0, k1, k2, *th, yy, True)
    pg2, g2, G2 = _lib.bf_grad_sep(c, nb, 0, ks, kt, *th, yy, want_rows=True)
    assert torch.equal(pg, pg2) and torch.equal(g, g2) and torch.equal(G, G2)
    q, _ = S.query(3)
    qd, qn = dev(q), dev(S.query_neighbours(3, 16))
    Bc, Fc, mean = torch.ops.nngp.bf_cross_sep(c, qd, qn, k1, k2, *th, yy)
    Bc2, Fc2, Rc2, _ = _lib.bf_cross_sep(c, qd, qn, ks, kt, *th, ref_values=yy, want_r=True)
    assert torch.equal(Bc, Bc2) and torch.equal(Fc, Fc2) and torch.equal(mean, -Rc2)
    with pytest.raises(RuntimeError):
        torch.ops.nngp.bf_sweep_sep(c.cpu(), nb.cpu(), None, 0, k1, k2, *th, yy.cpu(), True)
    with pytest.raises(RuntimeError):
        torch.ops.nngp.bf_grad_sep(c.cpu(), nb.cpu(), None, 0, k1, k2, *th, yy.cpu(), True)
    with pytest.raises(RuntimeError):
        torch.ops.nngp.bf_cross_sep(c.cpu(), qd.cpu(), qn.cpu(), k1, k2, *th, yy.cpu())
    # autograd: the gradient in theta is the sweep's; the gradient in the values against the restatement's
    theta = torch.tensor(th, dtype=torch.float64, requires_grad=True)
    yv = yy.clone().requires_grad_(True)
    ll = pynngp_amd.loglik_sep(c, nb, ks, kt, theta, yv)
    ll.backward()
    assert torch.equal(theta.grad, g2.cpu())
    ref = S.prior_reference(3, 16, ks, kt)
    assert abs(float(ll.detach()) - float(ref.ll.sum())) <= 1e-11 * abs(float(ll.detach()))
    w = (ref.r / ref.F).astype(np.float64)
    want = -w.copy()
    nbr = S.neighbours(3, 16)
    for i in range(S.N):
        for a, j in enumerate(nbr[i]):
            if j >= 0:
                want[j] += float(ref.b[i, a]) * w[i]
    assert np.allclose(yv.grad.cpu().numpy(), want, rtol=1e-9, atol=1e-9)


# ---------------------------------------------------------------- the model: predict, gls, profile, fit
def test_model_sweeps_predict_gls_profile():
    from pynngp_amd import nngp as N

    ks, kt = "matern32", "exponential"
    model, t, y = make_model(400, 10, ks, kt)
    cov, th = model.cov, model.cov.theta
    # the sets come from the search in the (phi_s, phi_s, phi_t) metric
    assert np.array_equal(model.nbr.cpu().numpy(), O.c_knn_prior(S.scaled(t, th), 10))
    nbr = model.nbr.cpu().numpy()
    ref = S.rows(t, t, nbr, ks, kt, th, y, y)
    assert ref.resolved.all()
    ll = model.loglik()
    assert abs(ll - float(ref.ll.sum())) <= 1e-11 * abs(ll)
    B, F = (a.cpu().numpy() for a in model.compute_BF())
    assert np.all(np.abs(B - ref.b).max(1) <= BF_K * U * ref.sB) and np.all(np.abs(F - ref.F) <= BF_K * U * ref.sF)
    lg, g = model.loglik_grad()
    assert abs(lg - ll) <= 1e-11 * abs(ll)
    Gs = ref.G.astype(np.float64)
    assert np.all(np.abs(g - Gs.sum(0)) <= 1e-12 * np.abs(Gs).sum(0))
    # kriging at new points: the cross restatement on the sets of the same metric
    tq = np.random.default_rng(3).uniform(0, 1, (50, 3))
    mean, var = model.predict(values=y, query=tq)
    qn = O.knn_all(S.scaled(tq, th), S.scaled(t, th), 10).astype(np.int32)
    cref = S.rows(t, tq, qn, ks, kt, th, y, None)
    assert cref.resolved.all()
    assert np.all(np.abs(mean + cref.r.astype(np.float64)) <= BF_K * U * cref.sR)
    assert np.all(np.abs(var - cref.F.astype(np.float64)) <= BF_K * U * cref.sF)
    # the constant mean and the envelope gradient: the restatement at y - mu
    llp, mu, gp = model.profile_loglik_grad(cov)
    assert model.profile_loglik(cov)[0] == llp
    r1 = S.rows(t, t, nbr, ks, kt, th, np.ones(400), np.ones(400))
    mu_ref = float((r1.r * ref.r / ref.F).sum() / (r1.r * r1.r / ref.F).sum())
    assert abs(mu - mu_ref) <= 1e-10 * (1 + abs(mu_ref))
    rm = S.rows(t, t, nbr, ks, kt, th, y - mu, y - mu)
    assert abs(llp - float(rm.ll.sum())) <= 1e-11 * abs(llp)
    Gm = rm.G.astype(np.float64)
    assert np.all(np.abs(gp - Gm.sum(0)) <= 1e-10 * np.abs(Gm).sum(0))
    # the linear mean: GLS through the whitened Gram on this sweep's B and F; the restatement at the residual
    X = np.stack([np.ones(400), t[:, 0], t[:, 2]], 1)
    res = model.gls(cov, X)
    ones = np.ones(400)
    W = [S.rows(t, t, nbr, ks, kt, th, X[:, k], X[:, k]).r.astype(np.float64) for k in range(3)]
    W = np.stack(W, 1) / np.sqrt(ref.F.astype(np.float64))[:, None]
    wy = ref.r.astype(np.float64) / np.sqrt(ref.F.astype(np.float64))
    beta = np.linalg.lstsq(W, wy, rcond=None)[0]
    assert np.allclose(res.beta, beta, rtol=1e-9, atol=1e-9), (res.beta, beta)
    rl = S.rows(t, t, nbr, ks, kt, th, y - X @ res.beta, y - X @ res.beta)
    assert abs(res.loglik - float(rl.ll.sum())) <= 1e-11 * abs(res.loglik)
    lll, bl, gl = model.profile_loglik_grad(cov, mean="linear", X=X)
    assert lll == model.profile_loglik(cov, mean="linear", X=X)[0] and abs(lll - res.loglik) <= 1e-12 * abs(lll)
    Gl = rl.G.astype(np.float64)
    assert np.all(np.abs(gl - Gl.sum(0)) <= 1e-10 * np.abs(Gl).sum(0))
    del ones
    # rebuild_neighbors moves the sets to another metric
    other = cov.replace(phi_t=12.0)
    model.rebuild_neighbors(other)
    assert np.array_equal(model.nbr.cpu().numpy(), O.c_knn_prior(S.scaled(t, other.theta), 10))
    with pytest.raises(TypeError, match="SeparableCovariance"):
        model.predict(values=y, X=X, X_query=X)
    with pytest.raises(TypeError, match="SeparableCovariance"):
        make_model(100, 5, refType=("subset", 40))


@pytest.fixture(scope="module")
def simulated():
    """n = 1500 in 2-D space + time, exponential x exponential, drawn on the host by a dense Cholesky at
    (1, 6, 3, 0.1) plus a constant."""
    rng = np.random.default_rng(2025)
    n = 1500
    t = rng.uniform(0.0, 1.0, (n, 3))
    theta = (1.0, 6.0, 3.0, 0.1)
    K = S.cov_matrix(t, t, *EE, theta) + theta[3] * np.eye(n)
    y = 0.5 + np.linalg.cholesky(K) @ rng.standard_normal(n)
    return t, y, theta


def test_fit(simulated):
    from pynngp_amd import nngp as N

    t, y, theta = simulated
    start = N.SeparableCovariance(*EE, 0.5, 3.0, 6.0, 0.3)
    model = N.NNGP(t, y, None, "S=T", 10, start)
    sets = model.nbr.cpu().numpy().copy()
    ll_true = model.profile_loglik(N.SeparableCovariance(*EE, *theta))[0]
    res = model.fit(tol=1e-3)
    print("fit:", res["theta"], "loglik", res["loglik"], "true", ll_true, "grad", res["grad"], "evals", res["n_evals"],
          "grad evals", res["n_grad_evals"], res["message"])
    assert np.array_equal(model.nbr.cpu().numpy(), sets)  # fixed sets
    assert isinstance(model.cov, N.SeparableCovariance) and model.cov.theta == res["theta"]
    assert (model.cov.kind_s, model.cov.kind_t) == EE
    assert res["converged"] and res["n_grad_evals"] >= 1 and res["n_evals"] >= 1
    assert res["grad"].shape == (4,) and np.max(np.abs(res["grad"])) <= 1e-3
    assert res["loglik"] >= ll_true
    # a fixed nugget drops its log-parameter; reneighbor runs further rounds on the estimate's own metric
    model.cov = start
    fixed = model.fit(tol=1e-3, fix_tau2=0.1, reneighbor=1)
    print("fix_tau2, reneighbor=1:", fixed["theta"], fixed["loglik"], fixed["grad"])
    assert fixed["theta"][3] == 0.1 and fixed["grad"].shape == (3,) and fixed["rounds"] == 2
    assert np.array_equal(model.nbr.cpu().numpy(), O.c_knn_prior(S.scaled(t, fixed["theta"]), 10))
    # the derivative-free fit on the forward sweep agrees
    model2 = N.NNGP(t, y, None, "S=T", 10, start)
    free = model2.fit(gradient=False)
    print("derivative-free:", free["theta"], free["loglik"], "evals", free["n_evals"])
    assert "grad" not in free and free["n_grad_evals"] == 0
    assert abs(free["loglik"] - res["loglik"]) <= 1e-6 * abs(res["loglik"])
    for k in range(4):
        assert abs(free["theta"][k] - res["theta"][k]) <= 2e-2 * res["theta"][k], (k, free["theta"], res["theta"])
