"""GPU: the Polya-Gamma kernels (pynngp_amd.polya_gamma, gibbs_pg_update) -- moments against the closed forms of
PG(b, c) at 5 sigma (the bounds of tests/test_pg_host.py, tests/pg_moments.py), draws that depend on the
location's own (seed, sweep, i, b, c) alone, the fused update against the plain call, faults as data, refusals."""
import numpy as np
import pytest
import torch

import pg_moments as M

pytestmark = pytest.mark.gpu
N = 2 ** M.LOG2_N


def _pg(dev, trials, c, **kw):
    import pynngp_amd

    t = torch.as_tensor(np.asarray(trials, dtype=np.int32)).to(dev)
    return pynngp_amd.polya_gamma(t, torch.as_tensor(np.asarray(c, dtype=np.float64)).to(dev), **kw)


@pytest.mark.parametrize("b", M.BS)
@pytest.mark.parametrize("c", M.CS)
def test_moments(dev, b, c):
    om = _pg(dev, np.full(N, b), np.full(N, c), seed=20240611, sweep=3 + b)
    assert bool(torch.isfinite(om).all()) and float(om.min()) > 0.0
    mean = float(om.mean())
    d = om - mean
    var = float((d * d).sum() / (N - 1))
    m4 = float((d ** 4).mean())
    M.check_cell(b, c, N, mean, var, m4, float(torch.exp(-om).mean()))


def test_position_only(dev):
    rng = np.random.default_rng(1)
    n = 257
    c = rng.normal(0.0, 3.0, n)
    b = rng.integers(0, 9, n)
    full = _pg(dev, b, c, seed=7, sweep=11)
    assert torch.equal(full, _pg(dev, b, c, seed=7, sweep=11))  # two identical calls: identical bits
    for k in (1, 63, 64, 65):
        assert torch.equal(full[:k], _pg(dev, b[:k], c[:k], seed=7, sweep=11)), k
    live = torch.as_tensor(b > 0).to(dev)
    assert bool((full[~live] == 0).all())
    for kw in ({"seed": 8, "sweep": 11}, {"seed": 7, "sweep": 12}):
        other = _pg(dev, b, c, **kw)
        assert bool((other[live] != full[live]).all()), kw


def test_mixed_waves(dev):
    """trials cycling (0, 1, 7, 64) along i: divergent trip counts share waves, the last block is ragged; every
    omega_i is the uniform-trials call's at the same i and c"""
    n = 300
    c = np.linspace(-6.0, 6.0, n)
    b = np.array([0, 1, 7, 64])[np.arange(n) % 4]
    mixed = _pg(dev, b, c, seed=3, sweep=5)
    for bb in (0, 1, 7, 64):
        uni = _pg(dev, np.full(n, bb), c, seed=3, sweep=5)
        sel = torch.as_tensor(b == bb).to(dev)
        assert torch.equal(mixed[sel], uni[sel]), bb
    assert bool((mixed[torch.as_tensor(b == 0).to(dev)] == 0).all())


def test_fused_against_plain(dev):
    from pynngp_amd import _lib

    rng = np.random.default_rng(2)
    n = 1000
    b = torch.as_tensor(rng.integers(0, 12, n).astype(np.int32)).to(dev)
    s = torch.floor(torch.rand(n, dtype=torch.float64, device=dev) * (b + 1))
    kappa = s - 0.5 * b
    xb = torch.as_tensor(rng.normal(0.0, 1.0, n)).to(dev)
    w = torch.as_tensor(rng.normal(0.0, 2.0, n)).to(dev)
    omega, yres, status = _lib.gibbs_pg_update(b, kappa, xb, w, seed=5, sweep=9)
    assert int(status.item()) == 0
    plain, _ = _lib.polya_gamma(b, xb + w, seed=5, sweep=9)
    assert torch.equal(omega, plain)
    live = b > 0
    assert torch.equal(yres[live], kappa[live] / omega[live] - xb[live])
    assert bool((yres[~live] == 0).all()) and bool((omega[~live] == 0).all())


def test_faults_as_data(dev):
    import pynngp_amd
    from pynngp_amd import NNGPNumericalError

    rng = np.random.default_rng(3)
    n = 1000
    c = rng.normal(0.0, 2.0, n)
    b = np.full(n, 2)
    clean = _pg(dev, b, c, seed=1, sweep=2)
    bad = c.copy()
    bad[700], bad[413] = np.nan, np.inf
    status = torch.full((1,), -5, dtype=torch.int32, device=dev)
    om = _pg(dev, b, bad, seed=1, sweep=2, status=status)  # returns: the fault is data
    assert int(status.item()) == 413 + 1
    nan = torch.isnan(om)
    assert int(nan.sum()) == 2 and bool(nan[413]) and bool(nan[700])
    assert torch.equal(om[~nan], clean[~nan])
    with pytest.raises(NNGPNumericalError, match="location 413"):
        _pg(dev, b, bad, seed=1, sweep=2)


def test_refusals(dev):
    for t in (1025, -1):
        with pytest.raises(ValueError, match="trials"):
            _pg(dev, [1, t, 1], [0.0, 0.0, 0.0])
    import pynngp_amd

    with pytest.raises(NotImplementedError):
        pynngp_amd.polya_gamma(torch.ones(3, dtype=torch.int32), torch.zeros(3, dtype=torch.float64))


def test_torch_op(dev):
    import pynngp_amd

    pynngp_amd.load_ops()
    b = torch.full((500,), 3, dtype=torch.int32, device=dev)
    c = torch.linspace(-4.0, 4.0, 500, dtype=torch.float64, device=dev)
    om, st = torch.ops.nngp.polya_gamma(b, c, 4, 6)
    assert int(st.item()) == 0 and torch.equal(om, pynngp_amd.polya_gamma(b, c, seed=4, sweep=6))
