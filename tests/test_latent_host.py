"""CPU: the latent-field entry points (nngp_precision_apply, nngp_precision_sqrt_t_apply, nngp_latent_cg) are
exported and bound, reject bad arguments before any GPU call, size their workspaces sanely, and the Python layer
(LatentPosterior, NNGP.latent_mean / latent_sample, torch.ops.nngp.*) refuses what it does not serve."""
import ctypes
import os

import numpy as np
import pytest
import torch

NEW = ("nngp_precision_workspace_bytes", "nngp_precision_apply", "nngp_precision_sqrt_t_apply",
       "nngp_latent_cg_workspace_bytes", "nngp_latent_cg")


@pytest.fixture(scope="module")
def lib():
    from pynngp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build()")
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    from pynngp_amd import _lib

    for s in NEW:
        assert s in _lib.SYMBOLS, s
        fn = getattr(lib, s)
        assert fn.argtypes is not None, s


P = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731

# fake non-null, 256-byte aligned "device" addresses: every case below must fail before any launch
GEOM = dict(nbr=256, B=256, off=256, rev_j=256, rev_k=256, prep=256, n=10, m=4, sigma2=1.0, d=None, workspace=256,
            workspace_bytes=1 << 20)


def _apply(lib, **kw):
    a = dict(GEOM, x=256, out=512)
    a.update(kw)
    return lib.nngp_precision_apply(P(a["nbr"]), P(a["B"]), P(a["off"]), P(a["rev_j"]), P(a["rev_k"]), P(a["prep"]),
                                    a["n"], a["m"], a["sigma2"], P(a["d"]), P(a["x"]), P(a["out"]), P(a["workspace"]),
                                    a["workspace_bytes"], None)


def _sqrt(lib, **kw):
    a = dict(GEOM, z1=256, z2=256, out=512)
    a.update(kw)
    return lib.nngp_precision_sqrt_t_apply(P(a["nbr"]), P(a["B"]), P(a["off"]), P(a["rev_j"]), P(a["rev_k"]),
                                           P(a["prep"]), a["n"], a["m"], a["sigma2"], P(a["d"]), P(a["z1"]),
                                           P(a["z2"]), P(a["out"]), P(a["workspace"]), a["workspace_bytes"], None)


def _cg(lib, **kw):
    a = dict(GEOM, b=256, x=512, rtol=1e-8, max_iter=10, check_every=8)
    a.update(kw)
    info = (ctypes.c_double * 4)() if a.get("info", True) else None
    return lib.nngp_latent_cg(P(a["nbr"]), P(a["B"]), P(a["off"]), P(a["rev_j"]), P(a["rev_k"]), P(a["prep"]), a["n"],
                              a["m"], a["sigma2"], P(a["d"]), P(a["b"]), P(a["x"]), a["rtol"], a["max_iter"],
                              a["check_every"], info, P(a["workspace"]), a["workspace_bytes"], None)


COMMON_BAD = [
    (dict(nbr=None), "non-null"),
    (dict(B=None), "non-null"),
    (dict(off=None), "non-null"),
    (dict(rev_j=None), "non-null"),
    (dict(prep=None), "non-null"),
    (dict(workspace=None), "non-null"),
    (dict(n=-1), "bad n"),
    (dict(m=0), "m=0"),
    (dict(m=64), "m=64"),
    (dict(sigma2=0.0), "sigma2"),
    (dict(sigma2=-1.0), "sigma2"),
    (dict(sigma2=float("nan")), "sigma2"),
    (dict(workspace_bytes=16), "workspace too small"),
    (dict(workspace=264), "aligned"),
]


@pytest.mark.parametrize("call", [_apply, _sqrt, _cg])
@pytest.mark.parametrize("kw,msg", COMMON_BAD)
def test_bad_arguments_are_einval(lib, call, kw, msg):
    assert call(lib, **kw) == -1, (call.__name__, kw)
    assert msg in lib.nngp_last_error().decode()


@pytest.mark.parametrize("call,kw,msg", [
    (_apply, dict(x=None), "non-null"),
    (_apply, dict(out=None), "non-null"),
    (_apply, dict(out=256), "alias"),
    (_sqrt, dict(z1=None), "non-null"),
    (_sqrt, dict(out=None), "non-null"),
    (_sqrt, dict(d=256, z2=None), "z2"),
    (_cg, dict(b=None), "non-null"),
    (_cg, dict(x=None), "non-null"),
    (_cg, dict(info=False), "non-null"),
    (_cg, dict(rtol=0.0), "rtol"),
    (_cg, dict(rtol=1.0), "rtol"),
    (_cg, dict(rtol=-1e-3), "rtol"),
    (_cg, dict(rtol=float("nan")), "rtol"),
    (_cg, dict(max_iter=-1), "max_iter"),
    (_cg, dict(check_every=0), "check_every"),
])
def test_call_specific_bad_arguments(lib, call, kw, msg):
    assert call(lib, **kw) == -1, (call.__name__, kw)
    assert msg in lib.nngp_last_error().decode()


def test_workspace_sizes(lib):
    for fn in (lib.nngp_latent_cg_workspace_bytes, lib.nngp_precision_workspace_bytes):
        assert fn(-1) == 0 and fn(-10 ** 12) == 0
        sizes = [fn(n) for n in (0, 1, 31, 32, 33, 1000, 1001, 10 ** 6, 10 ** 6 + 1, 10 ** 8)]
        assert all(s % 256 == 0 for s in sizes), sizes
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[-1] > sizes[0]
    # the solver keeps six vectors; one application one
    assert lib.nngp_latent_cg_workspace_bytes(10 ** 6) >= 6 * 8 * 10 ** 6
    assert lib.nngp_precision_workspace_bytes(10 ** 6) >= 8 * 10 ** 6


# ---------------------------------------------------------------- Python refusals (no GPU needed)
def _cpu_geometry(n=6, m=2):
    nbr = torch.full((n, m), -1, dtype=torch.int32)
    B = torch.zeros((n, m), dtype=torch.float64)
    off = torch.zeros(n + 1, dtype=torch.int32)
    rev = torch.zeros(n * m, dtype=torch.int32)
    prep = torch.zeros(1 << 16, dtype=torch.uint8)
    return nbr, B, off, rev, rev.clone(), prep


def test_lib_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from pynngp_amd import _lib

    nbr, B, off, rj, rk, prep = _cpu_geometry()
    x = torch.zeros(6, dtype=torch.float64)
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.precision_apply(nbr, B, off, rj, rk, prep, 1.0, x)
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.precision_sqrt_t_apply(nbr, B, off, rj, rk, prep, 1.0, x)
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.latent_cg(nbr, B, off, rj, rk, prep, 1.0, x, x.clone())
    # a short or mistyped array never reaches the library
    for bad in (dict(x=torch.zeros(5, dtype=torch.float64)), dict(x=torch.zeros(6, dtype=torch.float32)),
                dict(B=torch.zeros((6, 3), dtype=torch.float64)), dict(off=torch.zeros(6, dtype=torch.int32)),
                dict(rj=torch.zeros(11, dtype=torch.int32)), dict(nbr=nbr.long())):
        a = dict(nbr=nbr, B=B, off=off, rj=rj, rk=rk, x=x)
        a.update(bad)
        with pytest.raises(ValueError):
            _lib.precision_apply(a["nbr"], a["B"], a["off"], a["rj"], a["rk"], prep, 1.0, a["x"])
    with pytest.raises(ValueError):
        _lib.precision_apply(nbr, B, off, rj, rk, prep, 1.0, x, d=torch.zeros(7, dtype=torch.float64))


def test_torch_ops_refuse_cpu_tensors():
    from pynngp_amd import load_ops

    load_ops()
    assert hasattr(torch.ops.nngp, "precision_apply") and hasattr(torch.ops.nngp, "latent_cg")
    nbr, B, off, rj, rk, prep = _cpu_geometry()
    x = torch.zeros(6, dtype=torch.float64)
    with pytest.raises(NotImplementedError):
        torch.ops.nngp.precision_apply(nbr, B, off, rj, rk, prep, 1.0, None, x)
    with pytest.raises(NotImplementedError):
        torch.ops.nngp.latent_cg(nbr, B, off, rj, rk, prep, 1.0, None, x)
    schema = str(torch.ops.nngp.latent_cg.default._schema)
    assert "check_every=8" in schema and "-> (Tensor, Tensor)" in schema


def test_latent_posterior_refusals():
    from pynngp_amd import Covariance, LatentPosterior

    rng = np.random.default_rng(0)
    c, y = rng.uniform(size=(20, 2)), rng.standard_normal(20)
    cov = Covariance("exponential", 1.0, 6.0, 0.1)
    with pytest.raises(ValueError, match="tau2 = 0"):
        LatentPosterior(c, y, cov.replace(tau2=0.0), m=4)
    with pytest.raises(NotImplementedError, match="callable"):
        LatentPosterior(c, y, lambda a, b: np.exp(-np.abs(a - b).sum(-1)), m=4)
    with pytest.raises(TypeError):
        LatentPosterior(c, y, None, m=4)
    with pytest.raises(ValueError, match="one response per location"):
        LatentPosterior(c, y[:-1], cov, m=4)
    with pytest.raises(ValueError, match="X must be"):
        LatentPosterior(c, y, cov, m=4, X=np.ones((19, 1)))
    with pytest.raises(ValueError, match="eps"):
        LatentPosterior(c, y, cov, m=4, eps=np.ones(19))
    with pytest.raises(ValueError, match="outside"):
        LatentPosterior(c, y, cov, m=0)
    with pytest.raises(ValueError, match="all NaN"):
        LatentPosterior(c, np.full(20, np.nan), cov, m=4)


@pytest.mark.gpu
def test_s_equals_t_object_has_the_reference_set_maps(dev):
    """S = T is the reference set without leaves: the object carries the reference-set maps like any other, and they
    are perm / pos and the identity."""
    from pynngp_amd import Covariance, LatentPosterior

    rng = np.random.default_rng(3)
    n = 37
    lp = LatentPosterior(rng.uniform(size=(n, 2)), rng.standard_normal(n), Covariance("exponential", 1.0, 6.0, 0.1),
                         m=4, device=dev)
    assert not lp._ref and lp.n_s == lp.n_nodes == lp.n == n
    ar = torch.arange(n, device=dev)
    assert np.array_equal(lp.node_of_t, np.arange(n))
    assert torch.equal(lp.pos[lp.perm], ar) and torch.equal(lp.perm.sort().values, ar)
    assert torch.equal(lp.perm_s, lp.perm) and torch.equal(lp.slot_of_ref, lp.pos) and torch.equal(lp.slot_of_t, lp.pos)


def test_nngp_latent_needs_s_equals_t():
    """The wrappers serve the field on the data locations only; the check comes before any device work."""
    from pynngp_amd import NNGP, Covariance

    obj = NNGP.__new__(NNGP)  # no GPU here: the constructor would refuse; the wrappers' own check is under test
    obj.refType = ("subset", 5)
    obj.cov = Covariance("exponential", 1.0, 6.0, 0.1)
    with pytest.raises(NotImplementedError, match="S=T"):
        obj.latent_mean()
    with pytest.raises(NotImplementedError, match="S=T"):
        obj.latent_sample(2)
