"""GPU: the level-scheduled solves with the NNGP factor (nngp_factor_solve_batch), the covariance product and
prior draws composed from them, and their Python / torch layers (pynngp_amd.NNGPFactor).

The oracle is the sequential recurrence in index order, written here in numpy: forward x_i = b_i + sum_k B[i,k]
x[nbr[i,k]] over the row's slots in slot order, transposed x_j = b_j + sum_e B[rev_j[e], rev_k[e]] x[rev_j[e]] over
j's reverse list in list order, each product rounded and then added (the GPU fuses the two: that, and nothing
else, is what the accuracy margin K absorbs -- the order of every sum is the oracle's own).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
# Accuracy margin of test_solve_accuracy / test_deep_chain: |gpu - long double| <= K max(|fp64 - long double|, eps)
# relative to max|x|.  A fused multiply-add drops one of the two roundings of a rounded product and sum, so the
# GPU's error is of the fp64 oracle's size, not a multiple of it; K = 4 leaves room for the two to differ in sign.
K_FMA = 4.0
PHI = 3.0  # range 1/3 of the unit square: strong correlation, B rows with large entries of both signs


def oracle(nbr, B, b, dtype, rev=None):
    """The recurrence in ``dtype``; ``rev`` = (off, rev_j, rev_k) selects the transposed solve.  b (n, c)."""
    n, m = nbr.shape
    x = np.array(b, dtype=dtype)
    Bd = B.astype(dtype)
    if rev is None:
        for i in range(n):
            acc = x[i].copy()
            for k in range(m):
                j = nbr[i, k]
                if 0 <= j < i:
                    acc = acc + Bd[i, k] * x[j]
            x[i] = acc
    else:
        off, rev_j, rev_k = rev
        for j in range(n - 1, -1, -1):
            acc = x[j].copy()
            for e in range(off[j], off[j + 1]):
                i = rev_j[e]
                if j < i < n:
                    acc = acc + Bd[i, rev_k[e]] * x[i]
            x[j] = acc
    return x


def host(f):
    """(nbr, B, F, (off, rev_j, rev_k)) of a factor as numpy arrays."""
    return (f.nbr.cpu().numpy(), f.B.cpu().numpy(), f.F.cpu().numpy(),
            (f.off.cpu().numpy(), f.rev_j.cpu().numpy(), f.rev_k.cpu().numpy()))


def make(dev, n, m, seed=0, coords=None, **kw):
    from pynngp_amd import Covariance, NNGPFactor

    if coords is None:
        coords = np.random.default_rng(seed).uniform(size=(n, 2))
    return NNGPFactor(coords, Covariance("exponential", 1.3, PHI), m=m, device=dev, **kw)


def check_against_oracle(f, b, trans, label):
    nbr, B, _, rev = host(f)
    x = f.solve(b, trans=trans)
    x64 = oracle(nbr, B, b, np.float64, rev if trans else None)
    xld = oracle(nbr, B, b, np.longdouble, rev if trans else None)
    scale = float(np.max(np.abs(xld)))
    gap = float(np.max(np.abs(x64 - xld))) / scale
    err = np.abs(x - xld).astype(np.float64) / scale
    print(f"{label}: max|gpu - ld| / max|x| = {err.max():.3e}, fp64 oracle gap = {gap:.3e}, "
          f"ratio = {err.max() / max(gap, EPS):.3f}")
    assert np.all(err <= K_FMA * max(gap, EPS)), (label, err.max(), gap)
    return x


def residual_ok(f, b, x, trans):
    """(I - B) x - b (or its transpose) row by row in long double from the GPU's x: at the rounding level of one
    row sum, <= (m + 2) ulp of sum |B x| + |b_i|."""
    nbr, B, _, (off, rev_j, rev_k) = host(f)
    n, m = nbr.shape
    xl, bl, Bl = x.astype(np.longdouble), b.astype(np.longdouble), B.astype(np.longdouble)
    worst = 0.0
    for i in range(n):
        if trans:
            es = [e for e in range(off[i], off[i + 1]) if i < rev_j[e] < n]
            terms = np.array([Bl[rev_j[e], rev_k[e]] * xl[rev_j[e]] for e in es], dtype=np.longdouble)
        else:
            ks = [k for k in range(m) if 0 <= nbr[i, k] < i]
            terms = np.array([Bl[i, k] * xl[nbr[i, k]] for k in ks], dtype=np.longdouble)
        terms = terms.reshape(-1, x.shape[1])
        r = np.abs(xl[i] - terms.sum(axis=0) - bl[i])
        bound = (m + 2) * EPS * (np.abs(terms).sum(axis=0) + np.abs(bl[i]))
        worst = max(worst, float(np.max(r / np.maximum(bound, np.finfo(np.float64).tiny))))
    return worst


@pytest.fixture(scope="module")
def f700(dev):
    return {m: make(dev, 700, m, seed=11) for m in (1, 5, 15, 32)}


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("m", [1, 5, 15, 32])
def test_solve_accuracy(f700, m, trans):
    """K = K_FMA = 4, fixed before the first GPU run.  Measured on MI355X: the fp64 oracle's gap to long double is
    2.4e-16 .. 8.3e-16 of max|x| over m = 1, 5, 15, 32 in both directions, the GPU's 1.4e-16 .. 8.3e-16, i.e. 0.50 ..
    1.02 of the oracle's own gap; the worst row residual is 0.23 of the (m + 2)-ulp bound."""
    f = f700[m]
    b = np.random.default_rng(3).standard_normal((700, 2))
    x = check_against_oracle(f, b, trans, f"m={m} trans={trans}")
    worst = residual_ok(f, b, x, trans)
    print(f"m={m} trans={trans}: worst residual / bound = {worst:.3f}")
    assert worst <= 1.0


def test_schedule_independence(dev):
    from pynngp_amd import _lib
    from pynngp_amd.factor import DEFAULT_FUSE_WIDTH

    f = make(dev, 3000, 5, seed=5)
    assert f.fuse_width == DEFAULT_FUSE_WIDTH
    counts = f.n_launches
    assert counts["wide"] > 0 and counts["runs"] > 0, counts  # both kernels run at the default
    assert counts["wide_t"] > 0 and counts["runs_t"] > 0, counts
    assert counts["forward"] < f.depth and counts["transposed"] < f.depth_t
    b = torch.from_numpy(np.random.default_rng(1).standard_normal((3000, 3))).to(dev)
    got = {}
    for w in (0, 1, 8, DEFAULT_FUSE_WIDTH, _lib.FACTOR_MAX_FUSE_WIDTH):
        f.fuse_width = w
        got[w] = (f.solve(b), f.solve(b, trans=True), f.cov_apply(b))
    f.fuse_width = 0
    assert f.n_launches["runs"] == 0 and f.n_launches["wide"] == f.depth
    for w, xs in got.items():
        for a, ref in zip(xs, got[0]):
            assert torch.equal(a, ref), f"fuse_width={w} changed the bits"
    with pytest.raises(ValueError):
        f.fuse_width = _lib.FACTOR_MAX_FUSE_WIDTH + 1


@pytest.mark.parametrize("trans", [False, True])
def test_batch_contract(f700, dev, trans):
    f = f700[15]
    rng = np.random.default_rng(8)
    col = torch.from_numpy(rng.standard_normal(700)).to(dev)
    single = f.solve(col, trans=trans)
    for nrhs in range(1, 9):
        for c in {0, nrhs // 2, nrhs - 1}:
            Bm = torch.from_numpy(rng.standard_normal((700, nrhs))).to(dev)
            if nrhs > 1:
                Bm[:, (c + 1) % nrhs] = float("nan")  # another column's NaN must not leak
            Bm[:, c] = col
            X = f.solve(Bm, trans=trans)
            assert torch.equal(X[:, c], single), (nrhs, c)
    inplace = col.clone()[:, None].contiguous()
    _lib_solve_inplace(f, inplace, trans)
    assert torch.equal(inplace[:, 0], single), "b and x may be one buffer"


def _lib_solve_inplace(f, v, trans):
    from pynngp_amd import _lib

    _lib.factor_solve_batch(*f._geom(), f.sched_t if trans else f.sched, v, trans=trans, fuse_width=f.fuse_width, out=v)


def test_deep_chain(dev):
    n = 2000
    f = make(dev, n, 3, coords=np.sort(np.random.default_rng(2).uniform(size=n))[:, None])
    assert f.depth == n and f.depth_t == n
    assert f.n_launches["forward"] <= 4 and f.n_launches["transposed"] <= 4, f.n_launches
    b = np.random.default_rng(4).standard_normal((n, 1))
    for trans in (False, True):
        x = check_against_oracle(f, b, trans, f"chain trans={trans}")
        assert residual_ok(f, b, x, trans) <= 1.0


def test_degenerate_shapes(dev):
    rng = np.random.default_rng(21)
    for n, m in ((1, 4), (6, 5), (257, 7)):  # n = 1; n = m + 1: every row padded with -1; no tile's multiple
        f = make(dev, n, m, seed=n)
        b = rng.standard_normal((n, 3))
        for trans in (False, True):
            x = check_against_oracle(f, b, trans, f"n={n} m={m} trans={trans}")
            assert residual_ok(f, b, x, trans) <= 1.0
    # scattered -1 slots: a third of the slots of a built neighbour array removed
    from pynngp_amd import _lib

    coords = rng.uniform(size=(300, 2))
    nbr = _lib.knn_prior(torch.from_numpy(coords).to(dev), 6).cpu().numpy()
    nbr[rng.uniform(size=nbr.shape) < 1 / 3] = -1
    f = make(dev, 300, 6, coords=coords, nbr=torch.from_numpy(nbr).to(dev))
    b = rng.standard_normal((300, 2))
    for trans in (False, True):
        x = check_against_oracle(f, b, trans, f"scattered trans={trans}")
        assert residual_ok(f, b, x, trans) <= 1.0


def dense_cov(coords, sigma2):
    d = np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(axis=2))
    return sigma2 * np.exp(-PHI * d)


@pytest.fixture(scope="module")
def f33(dev):
    coords = np.random.default_rng(33).uniform(size=(33, 2))
    return make(dev, 33, 32, coords=coords), dense_cov(coords, 1.3)


def test_exactness_anchor(f33):
    """n = 33, m = 32: every row conditions on all earlier ones, so the NNGP is the full GP and cov_apply on the
    identity is the dense covariance.  Tolerance: 8 cond(C) eps max|C| -- the factors come from solves with
    blocks of C, whose relative error is cond x eps; 8 covers the few such steps a column passes through."""
    f, C = f33
    cond = np.linalg.cond(C)
    assert cond <= 1e6, cond
    got = f.cov_apply(np.eye(33))  # 33 columns: batches of 8, 8, 8, 8, 1
    err = np.max(np.abs(got - C))
    print(f"anchor: cond(C) = {cond:.3e}, max|C~ - C| = {err:.3e}, bound = {8 * cond * EPS * C.max():.3e}")
    assert err <= 8 * cond * EPS * np.max(np.abs(C))


def dense_precision(f):
    nbr, B, F, _ = host(f)
    n, m = nbr.shape
    L = np.eye(n)
    for i in range(n):
        for k in range(m):
            if 0 <= nbr[i, k] < i:
                L[i, nbr[i, k]] -= B[i, k]
    return L.T @ np.diag(1.0 / (f.cov.sigma2 * F)) @ L


@pytest.mark.parametrize("layout", ["S=T", "ref"])
def test_round_trip(dev, f700, layout):
    """Q (C~ v) = v within 8 cond(Q) eps max|v|, cond(Q) computed densely on the CPU (the same kind of bound as the
    anchor's: two triangular solves and one operator application, each backward stable)."""
    if layout == "S=T":
        f = f700[15]
    else:
        rng = np.random.default_rng(17)
        f = make(dev, 500, 15, coords=rng.uniform(size=(500, 2)), ref=rng.uniform(size=(200, 2)))
        assert f.n_nodes == 700 and f.n_s == 200
    cond = np.linalg.cond(dense_precision(f))
    v = np.random.default_rng(6).standard_normal((f.n_nodes, 4))
    back = f.precision_apply(f.cov_apply(v))
    err = np.max(np.abs(back - v))
    print(f"round trip {layout}: cond(Q) = {cond:.3e}, max|Q C~ v - v| = {err:.3e}")
    assert err <= 8 * cond * EPS * np.max(np.abs(v))


def test_prior_draws_given_z_and_seeds(f700, dev):
    from pynngp_amd import _lib

    f = f700[15]
    z = torch.from_numpy(np.random.default_rng(9).standard_normal((11, 700))).to(dev)
    w = f.sample_prior(11, z=z)
    scaled = (torch.sqrt(f.cov.sigma2 * f.F)[:, None] * z.t()).contiguous()
    assert torch.equal(w, f.solve(scaled).t().contiguous())
    a, b, c = f.sample_prior(10, seed=4), f.sample_prior(10, seed=4), f.sample_prior(10, seed=5)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(f.sample_prior(3, seed=4), a[:3]), "draw k does not depend on how many are drawn"
    zk = _lib.gibbs_normals(torch.empty(700, dtype=torch.float64, device=dev), 4, 9)  # draw 9's normals
    assert np.array_equal(f.sample_prior(1, z=zk[None, :].contiguous()).cpu().numpy()[0], a[9])


def zscores(W, C):
    """Entrywise z-scores of the zero-mean sample covariance of the rows of W against C: for N Gaussian draws
    N S ~ Wishart(C, N), so Var(S_ij) = (C_ii C_jj + C_ij^2) / N."""
    N = W.shape[0]
    S = W.T @ W / N
    return np.abs(S - C) / np.sqrt((np.outer(np.diag(C), np.diag(C)) + C ** 2) / N)


def test_prior_draws_covariance(f33):
    f, C = f33
    N = 4096
    ref = np.random.default_rng(1).standard_normal((N, 33)) @ np.linalg.cholesky(C).T
    assert zscores(ref, C).max() <= 5.0, "the bound must hold for dense-Cholesky draws too"
    z = zscores(f.sample_prior(N, seed=2), C)
    print(f"prior draws: max z-score = {z.max():.3f}")
    assert z.max() <= 5.0


def test_wrappers(dev):
    from pynngp_amd import NNGP, Covariance, LatentPosterior

    rng = np.random.default_rng(12)
    t = rng.uniform(size=(400, 2))
    cov = Covariance("exponential", 1.5, 6.0, 0.2)
    g = NNGP(t, np.zeros(400), None, "S=T", 10, cov, device=dev)
    y0 = g.simulate(5, seed=3, noise=False)
    assert y0.shape == (5, 400)
    assert np.array_equal(y0, g.prior_factor().sample_prior(5, seed=3))
    y1 = g.simulate(5, seed=3)
    resid = y1 - y0
    assert np.array_equal(g.simulate(5, seed=3), y1) and abs(resid.std() / np.sqrt(0.2) - 1.0) < 0.1
    assert np.allclose(g.simulate(2, seed=3, noise=False, beta=2.5), y0[:2] + 2.5, rtol=0, atol=1e-14)
    with pytest.raises(NotImplementedError):
        NNGP(t, np.zeros(400), None, "S=T", 10, lambda a, b: np.exp(-np.abs(a - b).sum()), device=dev).simulate()

    y = y1[0]
    lp = LatentPosterior(t, y, cov, m=10, device=dev)
    w = lp.sample_prior(6, seed=1)
    assert w.shape == (6, 400) and np.all(np.isfinite(w)) and np.array_equal(w, lp.sample_prior(6, seed=1))
    assert np.array_equal(w, g.prior_factor().sample_prior(6, seed=1)), "the same DAG, the same draws"
    s = rng.uniform(size=(120, 2))
    lr = LatentPosterior(t, y, cov, m=10, device=dev, ref=s)
    wd, ws = lr.sample_prior(6, seed=1), lr.sample_prior(6, seed=1, where="ref")
    assert wd.shape == (6, 400) and ws.shape == (6, 120) and np.all(np.isfinite(wd)) and np.all(np.isfinite(ws))
    # the marginal variance of every node of the prior is close to sigma2 (exactly so on the first reference point)
    assert abs(lr.sample_prior(512, seed=2).var() / 1.5 - 1.0) < 0.2
    with pytest.raises(ValueError):
        lr.sample_prior(1, where="leaves")


def test_torch_ops(f700, dev):
    from pynngp_amd import load_ops

    load_ops()
    f = f700[5]
    b = torch.from_numpy(np.random.default_rng(14).standard_normal((700, 5))).to(dev)
    geom = (f.nbr, f.B, f.off, f.rev_j, f.rev_k, f._prep)

    def sched(s):
        return (s.rows_dev, s.level_off_dev, torch.from_numpy(s.level_off))

    for trans, s in ((False, f.sched), (True, f.sched_t)):
        x = torch.ops.nngp.factor_solve(*geom, *sched(s), trans, f.fuse_width, b)
        assert torch.equal(x, f.solve(b, trans=trans))
    c = torch.ops.nngp.factor_cov_apply(f.nbr, f.B, f.F, *geom[2:], *sched(f.sched), *sched(f.sched_t), f.cov.sigma2,
                                        f.fuse_width, b)
    assert torch.equal(c, f.cov_apply(b))

    def meta(t):
        return torch.empty(t.shape, dtype=t.dtype, device="meta")

    mg = tuple(meta(t) for t in geom)
    ms = tuple(meta(t) for t in sched(f.sched))
    out = torch.ops.nngp.factor_solve(*mg, *ms, False, 8, meta(b))
    assert out.device.type == "meta" and out.shape == b.shape and out.dtype == torch.float64
    out = torch.ops.nngp.factor_cov_apply(mg[0], mg[1], meta(f.F), *mg[2:], *ms, *ms, 1.0, 8, meta(b))
    assert out.device.type == "meta" and out.shape == b.shape

    cpu = tuple(t.cpu() for t in geom)
    cs = tuple(t.cpu() for t in sched(f.sched))
    with pytest.raises(NotImplementedError):
        torch.ops.nngp.factor_solve(*cpu, *cs, False, 8, b.cpu())
    with pytest.raises(NotImplementedError):
        torch.ops.nngp.factor_cov_apply(cpu[0], cpu[1], f.F.cpu(), *cpu[2:], *cs, *cs, 1.0, 8, b.cpu())


def test_refusals(f700, dev):
    from pynngp_amd import Covariance, NNGPFactor, _lib

    f = f700[5]
    with pytest.raises(NotImplementedError):
        NNGPFactor(np.zeros((4, 2)), lambda a, b: 1.0, device=dev)
    with pytest.raises(ValueError):
        f.solve(np.zeros(699))
    b = torch.zeros((700, 9), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        _lib.factor_solve_batch(*f._geom(), f.sched, b)
    with pytest.raises(_lib.NNGPExtensionError, match="fuse_width"):
        _lib.factor_solve_batch(*f._geom(), f.sched, b[:, :2].contiguous(), fuse_width=_lib.FACTOR_MAX_FUSE_WIDTH + 1)
    assert f.update(Covariance("matern", 1.0, 4.0, nu=1.2)).depth == f700[5].depth  # general-nu Matern; schedules stay
    x = f.solve(np.ones(700))
    assert np.all(np.isfinite(x))
    f.update(Covariance("exponential", 1.3, PHI))
