"""A sweep with a neighbour-set certificate (include/nngp.h nngp_nbr_cert_build / nngp_bf_sweep_cert) returns the
bits of the uncertified sweep: the trusted tiles leave out only index checks, far-point / zero-value selects and
distance clamps that are the identity on them.

n = 300 throughout: three tiles of 100 rows, tile 0 holds the padded rows (checked), tiles 1-2 are trusted.
No test sweeps with a certificate built for other contents (that would be an unchecked out-of-range read).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 300
THETA = (1.3, 9.0, 0.2)
KINDS = ("exponential", "matern32", "matern52", "gaussian", "spherical")


@pytest.fixture(scope="module")
def ops():
    from pynngp_amd import load_ops

    return load_ops()


def _field(dim, seed=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (N, dim)), rng.standard_normal(N)


def _sweep(ops, c, nbr, kind, theta, v, cert):
    """One sweep into fresh NaN-filled buffers: (B, F, R, partials)."""
    from pynngp_amd import _lib

    dev = c.device
    m = nbr.shape[1]
    B = torch.full((N, m), np.nan, dtype=torch.float64, device=dev)
    F = torch.full((N,), np.nan, dtype=torch.float64, device=dev)
    R = torch.full((N,), np.nan, dtype=torch.float64, device=dev)
    p = torch.full((4,), np.nan, dtype=torch.float64, device=dev)
    ws = _lib.bf_workspace(N, m, "auto", dev, kind=kind, dim=c.shape[1])
    cb, ci = cert if cert is not None else (None, None)
    torch.ops.nngp.bf_sweep_out(c, nbr, None, 0, ops.kind_code(kind), *theta, v, B, F, R, p, ws,
                                ops.algo_code("auto"), -1.0, None, None, cb, ci)
    return B, F, R, p


def _same(a, b):
    # (NaN-aware: a bad-index row's bits are compared too)
    return all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a, b))


def _ab(ops, dev, m, dim, kind, theta=THETA, trusted=2):
    from pynngp_amd import _lib

    coords, y = _field(dim)
    c, v = torch.from_numpy(coords).to(dev), torch.from_numpy(y).to(dev)
    nbr = _lib.knn_prior(c, m)
    cert = ops.nbr_cert(c, nbr, None, 0)
    info = cert[1].tolist()
    assert info[9] == 3 and info[10] == 1  # three tiles, the padded rows' tile checked
    assert ops.nbr_cert_trusted_tiles(cert[1], kind, theta) == trusted
    plain = _sweep(ops, c, nbr, kind, theta, v, None)
    certified = _sweep(ops, c, nbr, kind, theta, v, cert)
    torch.cuda.synchronize()
    assert plain[3][2].item() == -1 and plain[3][3].item() == -1
    assert _same(plain, certified)


@pytest.mark.parametrize("m", [2, 13, 15, 16, 18, 20, 23])
def test_certified_sweep_bit_identical_every_m(ops, dev, m):
    """Three, two and one wave per SIMD, odd and even last pair, right- and left-looking kernels."""
    _ab(ops, dev, m, 2, "exponential")


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_certified_sweep_bit_identical_every_dim(ops, dev, dim):
    _ab(ops, dev, 15, dim, "exponential")


@pytest.mark.parametrize("kind", KINDS)
def test_certified_sweep_bit_identical_every_kind(ops, dev, kind):
    _ab(ops, dev, 15, 2, kind)


def test_clamp_may_bind_runs_checked(ops, dev):
    """phi = 1000 on the unit square: phi diag log2(e) ~ 2040 > 1023, no tile is trusted; same bits."""
    _ab(ops, dev, 15, 2, "exponential", theta=(1.3, 1000.0, 0.2), trusted=0)


def test_bad_index_before_certifying_is_checked(ops, dev):
    from pynngp_amd import _lib

    coords, y = _field(2)
    c, v = torch.from_numpy(coords).to(dev), torch.from_numpy(y).to(dev)
    nbr = _lib.knn_prior(c, 15)
    nbr[150, 3] = N  # out of range, in tile 1, BEFORE certifying
    cert = ops.nbr_cert(c, nbr, None, 0)
    info = cert[1].tolist()
    assert info[9] == 3 and info[10] == 2
    assert ops.nbr_cert_trusted_tiles(cert[1], "exponential", THETA) == 1
    plain = _sweep(ops, c, nbr, "exponential", THETA, v, None)
    certified = _sweep(ops, c, nbr, "exponential", THETA, v, cert)
    torch.cuda.synchronize()
    assert plain[3][3].item() == 150 and certified[3][3].item() == 150
    assert _same(plain, certified)


def test_non_finite_coordinate_refused(ops, dev):
    from pynngp_amd import _lib

    coords, _ = _field(2)
    c = torch.from_numpy(coords).to(dev)
    nbr = _lib.knn_prior(c, 15)
    c2 = c.clone()
    c2[17, 1] = float("inf")
    with pytest.raises(RuntimeError, match="finite"):
        ops.nbr_cert(c2, nbr, None, 0)


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
@pytest.mark.parametrize("api", ["ops", "ctypes"])
def test_storage_layout(ops, dev, api, rank, world, monkeypatch):
    """ShardedLogLik(layout="storage"): the padded rows (input index < m) are scattered over the tiles; rank 1 of
    world 2 sweeps rows i0 > 0.  The checked tiles are exactly those holding a padded row."""
    from pynngp_amd.sweep import Covariance, ShardedLogLik

    coords, y = _field(2)
    c, v = torch.from_numpy(coords).to(dev), torch.from_numpy(y).to(dev)
    cov = Covariance("matern32", *THETA)
    res = {}
    for on in ("0", "1"):
        monkeypatch.setenv("NNGP_NBR_CERT", on)
        sw = ShardedLogLik(c, 15, rank, world, layout="storage", api=api, collective=False)
        if on == "1":
            info = sw._cert[1].tolist()
            rows = sw.hi - sw.lo
            tiles = -(-rows // 128)
            q, rem = divmod(rows, tiles)
            padded = (sw._nbr_sweep < 0).any(dim=1).cpu().numpy()
            starts = [t * q + min(t, rem) for t in range(tiles + 1)]
            want = sum(bool(padded[starts[t]:starts[t + 1]].any()) for t in range(tiles))
            assert (rank == 0 or sw.lo > 0) and info[8] == sw.lo and info[9] == tiles and info[10] == want
            assert ops.nbr_cert_trusted_tiles(sw._cert[1], cov.kind, THETA) == tiles - want
        else:
            assert sw._cert is None
        p = sw.local_partials(cov, v, True).clone()
        res[on] = (sw.B.clone(), sw.F.clone(), p)
    torch.cuda.synchronize()
    assert res["0"][2][3].item() == -1
    assert _same(res["0"], res["1"])


def test_certified_graph_replay_bit_identical(ops, dev):
    """A certified sweep captured in a HIP graph replays with the direct call's bits."""
    from pynngp_amd.sweep import Covariance, ShardedLogLik

    coords, y = _field(2)
    c, v = torch.from_numpy(coords).to(dev), torch.from_numpy(y).to(dev)
    sweep = ShardedLogLik(c, 15, 0, 1, layout="storage")
    assert sweep._cert is not None
    cov = Covariance("exponential", *THETA)
    direct = sweep.local_partials(cov, v, True).clone()
    B0, F0 = sweep.B.clone(), sweep.F.clone()
    vs = sweep.to_storage(v).clone()
    out = torch.empty(4, dtype=torch.float64, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sweep.local_partials(cov, vs, True, "storage", out=out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sweep.local_partials(cov, vs, True, "storage", out=out)
    sweep.B.fill_(np.nan)
    sweep.F.fill_(np.nan)
    out.fill_(np.nan)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, direct) and torch.equal(sweep.B, B0) and torch.equal(sweep.F, F0)
