"""GPU: nngp_order_maxmin against the numpy restatement of tests/order_ref.py, index for index; its defining
properties and run-to-run bit identity at a size that spans many blocks and table sizes; streams, the torch
operator, NNGP(ordering=), the ("maxmin", nRef) reference set, and the reason for the feature: a smaller KL
divergence from the exact process than the as-drawn and the coordinate-sorted orders."""
import numpy as np
import pytest
import torch

import order_ref as R

pytestmark = pytest.mark.gpu


def gpu_order(dev, x, seed=0):
    from pynngp_amd import order_maxmin

    perm, level = order_maxmin(torch.as_tensor(np.ascontiguousarray(x)).to(dev), seed, return_level=True)
    assert perm.dtype == torch.int64 and level.dtype == torch.int32 and perm.device == level.device
    return perm.cpu().numpy(), level.cpu().numpy()


def assert_same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:5]}: {got[bad[:5]]} vs {want[bad[:5]]}"


@pytest.mark.parametrize("name", ["uniform1d", "uniform2d", "uniform3d", "lattice32", "duplicates", "one", "two",
                                  "coincident"])
def test_equals_restatement_on_the_host_inputs(dev, name):
    perm, level = gpu_order(dev, R.case(name))
    want_perm, want_level = R.reference(name)
    assert_same(level, want_level, f"{name} level")
    assert_same(perm, want_perm, f"{name} perm")


def test_equals_restatement_with_another_seed(dev):
    perm, level = gpu_order(dev, R.case("uniform2d"), seed=7)
    want_perm, want_level = R.reference("uniform2d", seed=7)
    assert_same(level, want_level, "level")
    assert_same(perm, want_perm, "perm")
    big_seed = 0xFFFFFFFF  # seed * 0x9e3779b9 wraps mod 2^32
    perm, level = gpu_order(dev, R.case("duplicates"), seed=big_seed)
    want_perm, want_level = R.order_maxmin(R.case("duplicates"), big_seed)
    assert_same(level, want_level, "level")
    assert_same(perm, want_perm, "perm")


def clustered(n=20000):
    """Three Gaussian clusters of very different widths: deep levels, unevenly filled cells."""
    rng = np.random.default_rng(11)
    centres = np.array([[0.2, 0.3], [0.7, 0.8], [0.75, 0.2]])
    widths = np.array([0.1, 0.01, 0.001])
    which = rng.integers(0, 3, size=n)
    return centres[which] + rng.standard_normal((n, 2)) * widths[which][:, None]


@pytest.mark.parametrize("name", ["clustered2d", "uniform3d"])
def test_equals_restatement_at_20000(dev, name):
    x = clustered() if name == "clustered2d" else np.random.default_rng(12).uniform(size=(20000, 3))
    stats = {}
    want_perm, want_level = R.order_maxmin(x, 0, stats)
    perm, level = gpu_order(dev, x)
    print(f"{name}: levels used {int(want_level.max())}, rounds per level {stats['rounds']}")
    assert_same(level, want_level, "level")
    assert_same(perm, want_perm, "perm")


def test_properties_and_bit_identity_at_70000(dev):
    from pynngp_amd import _lib

    x = np.random.default_rng(13).uniform(size=(70000, 2))
    x[:35000] = 0.5 + (x[:35000] - 0.5) * 0.05  # half of the points in a dense patch: several table sizes
    c = torch.as_tensor(x).to(dev)
    ws_bytes = _lib.load().nngp_order_maxmin_workspace_bytes
    assert ws_bytes(10 ** 6, 2) > ws_bytes(70000, 2) > 7 * 4 * 70000 and ws_bytes(70000, 2) % 256 == 0
    perm, level, stats = _lib.order_maxmin(c, 0, want_stats=True)
    perm2, level2 = _lib.order_maxmin(c, 0)
    assert torch.equal(perm, perm2) and torch.equal(level, level2)
    perm, level = perm.cpu().numpy(), level.cpu().numpy()
    R.check_properties(x, perm, level)
    key = R.keys(len(x))
    for l in np.unique(level):
        k = key[perm[level == l]]
        assert np.all(k[1:] > k[:-1]), f"level {l} is not in key order"
    assert sum(stats["selected"]) + stats["n_tail"] == len(x)
    assert np.array_equal(np.bincount(level, minlength=21)[:20], stats["selected"])
    assert stats["launches"] > 0 and stats["host_reads"] <= 2 + sum(stats["rounds"]) + sum(stats["accept_iterations"]) \
        + stats["levels"]


def test_streams_and_torch_op(dev):
    from pynngp_amd import _lib, load_ops

    load_ops()
    x = R.case("uniform2d")
    c = torch.as_tensor(x).to(dev)
    want_perm, want_level = R.reference("uniform2d")
    results = []
    for _ in range(2):
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            results.append(_lib.order_maxmin(c, 0))
        torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize(dev)
    for perm, level in results:
        assert_same(perm.cpu().numpy(), want_perm, "perm on a side stream")
        assert_same(level.cpu().numpy(), want_level, "level on a side stream")
    perm_op, level_op = torch.ops.nngp.order_maxmin(c, 0)
    assert torch.equal(perm_op, results[0][0]) and torch.equal(level_op, results[0][1])
    with pytest.raises(RuntimeError, match="uint32"):
        torch.ops.nngp.order_maxmin(c, -1)


def test_refusals_on_the_device(dev):
    from pynngp_amd import _lib

    x = R.case("uniform2d").copy()
    x[17, 1] = np.nan
    with pytest.raises(_lib.NNGPExtensionError, match="finite"):  # the C ABI's own check (the wrapper above it has one too)
        _lib.order_maxmin(torch.as_tensor(x).to(dev))
    x[17, 1] = 1e200  # finite, but its squared distances are not
    with pytest.raises(_lib.NNGPExtensionError, match="finite"):
        _lib.order_maxmin(torch.as_tensor(x).to(dev))


def test_other_orders(dev):
    import pynngp_amd

    assert_same(pynngp_amd.order_random(5000, 3, dev).cpu().numpy(), R.order_random(5000, 3), "order_random")
    x = np.round(R.case("uniform3d"), 2)  # many equal coordinates: the sorts must be stable
    c = torch.as_tensor(x).to(dev)
    assert_same(pynngp_amd.order_coordinate(c, 1).cpu().numpy(), np.argsort(x[:, 1], kind="stable"), "coordinate")
    mid = pynngp_amd.order_middleout(c).cpu().numpy()
    d2 = ((c - c.mean(dim=0, keepdim=True)) ** 2).sum(dim=1).cpu().numpy()
    assert np.array_equal(np.sort(mid), np.arange(len(x))) and np.all(np.diff(d2[mid]) >= 0)
    sub = pynngp_amd.maxmin_subset(c, 40).cpu().numpy()
    assert_same(sub, gpu_order(dev, x)[0][:40], "maxmin_subset")


def test_nngp_ordering_maxmin(dev):
    from pynngp_amd import NNGP, Covariance, order_maxmin

    rng = np.random.default_rng(21)
    coords = rng.uniform(size=(1200, 2))
    y = rng.standard_normal(1200)
    eps = rng.uniform(0.1, 0.2, size=1200)
    cov = Covariance("exponential", 1.0, 6.0, 0.05)
    model = NNGP(coords, y, eps, "S=T", 10, cov, ordering="maxmin")
    perm = order_maxmin(torch.as_tensor(coords).to(dev))
    assert torch.equal(model.perm, perm)
    p = perm.cpu().numpy()
    assert np.array_equal(model.t, coords[p]) and np.array_equal(model.y, y[p]) and np.array_equal(model.eps, eps[p])
    assert model.s is model.t
    by_hand = NNGP(coords[p], y[p], eps[p], "S=T", 10, cov)
    assert by_hand.perm is None
    assert torch.equal(model.nbr, by_hand.nbr)
    assert model.loglik() == by_hand.loglik()  # bit for bit
    assert torch.equal(model.F, by_hand.F) and torch.equal(model.B, by_hand.B)
    a = rng.standard_normal((1200, 2))
    assert np.array_equal(model.to_model_order(a), a[p])
    assert np.array_equal(model.to_input_order(model.to_model_order(a)), a)
    ta = torch.as_tensor(a).to(dev)
    assert torch.equal(model.to_input_order(model.to_model_order(ta)), ta)
    # values= are in model order: the input-order y converted gives the same number
    assert model.loglik(values=model.to_model_order(y)) == model.loglik()

    plain = NNGP(coords, y, eps, "S=T", 10, cov)  # ordering=None: the caller's order, as before
    assert plain.perm is None and plain.t is coords and plain.y is y
    assert plain.to_model_order(a) is a

    explicit = NNGP(coords, y, eps, "S=T", 10, cov, ordering=p)
    assert explicit.loglik() == model.loglik()
    rnd = NNGP(coords, y, None, "S=T", 10, cov, ordering="random")
    assert np.array_equal(rnd.perm.cpu().numpy(), R.order_random(1200, 0))
    with pytest.raises(ValueError, match="length 1200"):
        NNGP(coords, y, None, "S=T", 10, cov, ordering=np.arange(1199))
    with pytest.raises(ValueError, match="unknown ordering"):
        NNGP(coords, y, None, "S=T", 10, cov, ordering="hilbert")


def test_reference_set_maxmin_and_ordered_reference_set(dev):
    from pynngp_amd import NNGP, Covariance, order_maxmin

    rng = np.random.default_rng(22)
    t = rng.uniform(size=(1500, 2))
    y = rng.standard_normal(1500)
    cov = Covariance("exponential", 1.0, 6.0, 0.05)
    model = NNGP(t, y, None, ("maxmin", 200), 8, cov)
    perm = order_maxmin(torch.as_tensor(t).to(dev)).cpu().numpy()
    assert model.s.shape == (200, 2) and np.array_equal(model.s, t[perm[:200]])
    assert len({tuple(p) for p in model.s}) == 200
    assert model.t is t and model.perm is None and model.nbr.shape == (200, 8)
    assert np.isfinite(model.loglik(values=np.zeros(200)))

    np.random.seed(5)
    ordered = NNGP(t, y, None, ("random", 300, ((0, 1), (0, 1))), 8, cov, ordering="maxmin")
    np.random.seed(5)
    drawn = NNGP(t, y, None, ("random", 300, ((0, 1), (0, 1))), 8, cov)
    sp = order_maxmin(torch.as_tensor(drawn.s).to(dev)).cpu().numpy()
    assert np.array_equal(ordered.s, drawn.s[sp]) and np.array_equal(ordered.perm.cpu().numpy(), sp)
    assert ordered.t is t and ordered.y is y  # only S is ordered


def kl_exact_to_nngp(coords, nbr, B, F, sigma2, phi, tau2):
    """KL(exact GP || NNGP) = 1/2 [tr(Q Sigma) - n - log det(Q Sigma)] with Q = (I - B)^T F^-1 (I - B)."""
    n, m = nbr.shape
    d = np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(-1))
    Sigma = sigma2 * np.exp(-phi * d) + tau2 * np.eye(n)
    L = np.eye(n)
    for k in range(m):
        ok = nbr[:, k] >= 0
        L[np.flatnonzero(ok), nbr[ok, k]] -= B[ok, k]
    Q = L.T @ (L / F[:, None])
    logdet = np.linalg.slogdet(Sigma)[1] - np.log(F).sum()  # det(I - B) = 1
    return 0.5 * (np.trace(Q @ Sigma) - n - logdet)


def test_maxmin_is_closer_to_the_exact_process(dev):
    """n = 900 uniform 2-D points, exponential (1, 6, 0.05), m = 10: KL(exact || NNGP) under max-min order is below
    that of the rows as drawn and of the rows sorted by x (a numpy run of the same set-up gave 1.10 / 2.65 / 3.16)."""
    from pynngp_amd import NNGP, Covariance

    rng = np.random.default_rng(31)
    coords = rng.uniform(size=(900, 2))
    y = np.zeros(900)
    theta = (1.0, 6.0, 0.05)
    cov = Covariance("exponential", *theta)
    kl = {}
    for name, pts, ordering in (("sorted", coords[np.argsort(coords[:, 0], kind="stable")], None),
                                ("as_drawn", coords, None), ("maxmin", coords, "maxmin")):
        model = NNGP(pts, y, None, "S=T", 10, cov, ordering=ordering)
        kl[name] = kl_exact_to_nngp(np.asarray(model.t), model.nbr.cpu().numpy(), model.B.cpu().numpy(),
                                    model.F.cpu().numpy(), *theta)
    print(f"KL(exact || NNGP): maxmin {kl['maxmin']:.3f}, as drawn {kl['as_drawn']:.3f}, sorted {kl['sorted']:.3f}")
    assert all(np.isfinite(v) and v > 0 for v in kl.values())
    assert kl["maxmin"] < kl["as_drawn"]
    assert kl["maxmin"] < kl["sorted"]
