"""CPU: the batched latent-field entry points (nngp_precision_apply_batch, nngp_precision_sqrt_t_apply_batch,
nngp_latent_cg_batch, nngp_precision_diag) are exported and bound, reject bad arguments before any GPU call,
size their workspaces sanely, and the Python layer (the _lib wrappers, torch.ops.nngp.*_batch,
LatentPosterior.solve_many / marginal_variance, NNGP.latent_sd) refuses what it does not serve."""
import ctypes
import os

import numpy as np
import pytest
import torch

NEW = ("nngp_precision_batch_workspace_bytes", "nngp_precision_apply_batch", "nngp_precision_sqrt_t_apply_batch",
       "nngp_latent_cg_batch_workspace_bytes", "nngp_latent_cg_batch", "nngp_precision_diag")


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
    assert _lib.LATENT_MAX_RHS == 8
    assert lib.nngp_abi_version() == 4  # pure additions


P = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731

# fake non-null, 256-byte aligned "device" addresses: every case below must fail before any launch
GEOM = dict(nbr=256, B=256, off=256, rev_j=256, rev_k=256, prep=256, n=10, m=4, sigma2=1.0, d=None, nrhs=3,
            workspace=256, workspace_bytes=1 << 20)


def _apply(lib, **kw):
    a = dict(GEOM, x=256, out=512)
    a.update(kw)
    return lib.nngp_precision_apply_batch(P(a["nbr"]), P(a["B"]), P(a["off"]), P(a["rev_j"]), P(a["rev_k"]),
                                          P(a["prep"]), a["n"], a["m"], a["sigma2"], P(a["d"]), a["nrhs"], P(a["x"]),
                                          P(a["out"]), P(a["workspace"]), a["workspace_bytes"], None)


def _sqrt(lib, **kw):
    a = dict(GEOM, z1=256, z2=256, out=512)
    a.update(kw)
    return lib.nngp_precision_sqrt_t_apply_batch(P(a["nbr"]), P(a["B"]), P(a["off"]), P(a["rev_j"]), P(a["rev_k"]),
                                                 P(a["prep"]), a["n"], a["m"], a["sigma2"], P(a["d"]), a["nrhs"],
                                                 P(a["z1"]), P(a["z2"]), P(a["out"]), P(a["workspace"]),
                                                 a["workspace_bytes"], None)


def _cg(lib, **kw):
    a = dict(GEOM, b=256, x=512, rtol=1e-8, max_iter=10, check_every=8)
    a.update(kw)
    info = (ctypes.c_double * 32)() if a.get("info", True) else None
    return lib.nngp_latent_cg_batch(P(a["nbr"]), P(a["B"]), P(a["off"]), P(a["rev_j"]), P(a["rev_k"]), P(a["prep"]),
                                    a["n"], a["m"], a["sigma2"], P(a["d"]), a["nrhs"], P(a["b"]), P(a["x"]),
                                    a["rtol"], a["max_iter"], a["check_every"], info, P(a["workspace"]),
                                    a["workspace_bytes"], None)


# the single calls' table (tests/test_latent_host.py), plus nrhs
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
    (dict(nrhs=0), "nrhs"),
    (dict(nrhs=9), "nrhs"),
    (dict(nrhs=-1), "nrhs"),
]


@pytest.mark.parametrize("call", [_apply, _sqrt, _cg])
@pytest.mark.parametrize("kw,msg", COMMON_BAD)
def test_bad_arguments_are_einval(lib, call, kw, msg):
    assert call(lib, **kw) == -1, (call.__name__, kw)
    assert msg in lib.nngp_last_error().decode()


def _diag(lib, **kw):
    a = dict(prep=256, n=10, m=4, sigma2=1.0, d=None, out=512)
    a.update(kw)
    return lib.nngp_precision_diag(P(a["prep"]), a["n"], a["m"], a["sigma2"], P(a["d"]), P(a["out"]), None)


@pytest.mark.parametrize("call,kw,msg", [
    (_apply, dict(x=None), "non-null"),
    (_apply, dict(out=None), "non-null"),
    (_apply, dict(out=256), "alias"),
    (_sqrt, dict(z1=None), "non-null"),
    (_sqrt, dict(out=None), "non-null"),
    (_sqrt, dict(out=256), "alias"),
    (_sqrt, dict(d=256, z2=None), "z2"),
    (_cg, dict(b=None), "non-null"),
    (_cg, dict(x=None), "non-null"),
    (_cg, dict(x=256), "alias"),
    (_cg, dict(info=False), "non-null"),
    (_cg, dict(rtol=0.0), "rtol"),
    (_cg, dict(rtol=1.0), "rtol"),
    (_cg, dict(rtol=float("nan")), "rtol"),
    (_cg, dict(max_iter=-1), "max_iter"),
    (_cg, dict(check_every=0), "check_every"),
    (_diag, dict(prep=None), "non-null"),
    (_diag, dict(out=None), "non-null"),
    (_diag, dict(n=-1), "bad n"),
    (_diag, dict(m=0), "m=0"),
    (_diag, dict(sigma2=0.0), "sigma2"),
    (_diag, dict(prep=264), "aligned"),
])
def test_call_specific_bad_arguments(lib, call, kw, msg):
    assert call(lib, **kw) == -1, (call.__name__, kw)
    assert msg in lib.nngp_last_error().decode()


def test_workspace_sizes(lib):
    ns = (0, 1, 31, 32, 33, 1000, 1001, 10 ** 6, 10 ** 6 + 1, 10 ** 8)
    for fn in (lib.nngp_latent_cg_batch_workspace_bytes, lib.nngp_precision_batch_workspace_bytes):
        for bad in (0, 9, -1):
            assert fn(1000, bad) == 0
        table = np.array([[fn(n, k) for k in range(1, 9)] for n in ns], dtype=np.int64)
        assert np.all(table % 256 == 0) and np.all(table > 0)
        assert np.all(np.diff(table, axis=0) >= 0) and np.all(np.diff(table, axis=1) >= 0)  # monotone in n and nrhs
        assert table[-1, 0] > table[0, 0] and table[-1, -1] > table[-1, 0]
        for k in range(1, 9):
            assert fn(-1, k) == 0 and fn(-10 ** 12, k) == 0
    for k in range(1, 9):
        assert lib.nngp_latent_cg_batch_workspace_bytes(10 ** 6, k) >= 6 * 8 * 10 ** 6 * k
        assert lib.nngp_precision_batch_workspace_bytes(10 ** 6, k) >= 8 * 10 ** 6 * k


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
    x = torch.zeros((6, 3), dtype=torch.float64)
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.precision_apply_batch(nbr, B, off, rj, rk, prep, 1.0, x)
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.precision_sqrt_t_apply_batch(nbr, B, off, rj, rk, prep, 1.0, x)
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.latent_cg_batch(nbr, B, off, rj, rk, prep, 1.0, x, x.clone())
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.precision_diag(prep, 6, 2, 1.0)
    # a short, mistyped or too wide array never reaches the library
    for bad in (torch.zeros((5, 3), dtype=torch.float64), torch.zeros((6, 3), dtype=torch.float32),
                torch.zeros(6, dtype=torch.float64), torch.zeros((6, 9), dtype=torch.float64),
                torch.zeros((6, 0), dtype=torch.float64), torch.zeros((3, 6), dtype=torch.float64).t()):
        with pytest.raises(ValueError):
            _lib.precision_apply_batch(nbr, B, off, rj, rk, prep, 1.0, bad)
        with pytest.raises(ValueError):
            _lib.latent_cg_batch(nbr, B, off, rj, rk, prep, 1.0, bad, torch.zeros_like(bad).contiguous())
    with pytest.raises(ValueError):
        _lib.precision_apply_batch(nbr, B, off, rj, rk, prep, 1.0, x, d=torch.zeros(7, dtype=torch.float64))
    with pytest.raises(ValueError):
        _lib.precision_apply_batch(nbr, B, off, rj, rk, prep, 1.0, x, out=torch.zeros((6, 2), dtype=torch.float64))
    with pytest.raises(ValueError):
        _lib.precision_sqrt_t_apply_batch(nbr, B, off, rj, rk, prep, 1.0, x, z2=torch.zeros((6, 2), dtype=torch.float64))
    with pytest.raises(ValueError):
        _lib.latent_cg_batch(nbr, B, off, rj, rk, prep, 1.0, x, torch.zeros((6, 2), dtype=torch.float64))
    with pytest.raises(ValueError):
        _lib.precision_diag(prep, 6, 2, 1.0, d=torch.zeros(5, dtype=torch.float64))
    with pytest.raises(ValueError):
        _lib.precision_diag(prep, 6, 0, 1.0)


def test_torch_ops_refuse_cpu_tensors():
    from pynngp_amd import load_ops

    load_ops()
    assert hasattr(torch.ops.nngp, "precision_apply_batch") and hasattr(torch.ops.nngp, "latent_cg_batch")
    nbr, B, off, rj, rk, prep = _cpu_geometry()
    x = torch.zeros((6, 3), dtype=torch.float64)
    with pytest.raises(NotImplementedError):
        torch.ops.nngp.precision_apply_batch(nbr, B, off, rj, rk, prep, 1.0, None, x)
    with pytest.raises(NotImplementedError):
        torch.ops.nngp.latent_cg_batch(nbr, B, off, rj, rk, prep, 1.0, None, x)
    schema = str(torch.ops.nngp.latent_cg_batch.default._schema)
    assert "check_every=8" in schema and "max_iter=1000" in schema and "-> (Tensor, Tensor)" in schema
    assert str(torch.ops.nngp.precision_apply_batch.default._schema).endswith("-> Tensor")


def _hollow_posterior(n=5):
    """A LatentPosterior without a device: the argument checks under test come before any device work."""
    from pynngp_amd import LatentPosterior

    lp = LatentPosterior.__new__(LatentPosterior)
    lp.n, lp.p, lp.m = n, 0, 2
    lp.n_nodes = lp.n_s = n  # S = T: every node is a reference node
    lp.device = torch.device("cpu")
    lp.perm = lp.pos = lp.perm_s = lp.slot_of_ref = torch.arange(n)
    return lp


def test_solve_many_and_marginal_variance_argument_errors():
    lp = _hollow_posterior()
    for bad in (0, 9, -1):
        with pytest.raises(ValueError, match="batch"):
            lp.solve_many(np.zeros((2, 5)), batch=bad)
        with pytest.raises(ValueError, match="batch"):
            lp.marginal_variance(4, batch=bad)
        with pytest.raises(ValueError, match="batch"):
            lp.sample(2, batch=bad)
    with pytest.raises(ValueError, match="rhs must be"):
        lp.solve_many(np.zeros(5))
    with pytest.raises(ValueError, match="rhs must be"):
        lp.solve_many(np.zeros((2, 4)))
    with pytest.raises(ValueError, match="rhs must be"):
        lp.solve_many(torch.zeros((2, 5), dtype=torch.float32))
    with pytest.raises(ValueError, match="x0"):
        lp.solve_many(np.zeros((2, 5)), x0=np.zeros((3, 5)))
    with pytest.raises(ValueError, match="rtol"):
        lp.solve_many(np.zeros((2, 5)), rtol=0.0)
    for bad in (1, 0, -3):
        with pytest.raises(ValueError, match="n_draws"):
            lp.marginal_variance(bad)


def test_nngp_latent_sd_needs_s_equals_t():
    from pynngp_amd import NNGP, Covariance

    obj = NNGP.__new__(NNGP)  # no GPU here: the wrapper's own check is under test
    obj.refType = ("subset", 5)
    obj.cov = Covariance("exponential", 1.0, 6.0, 0.1)
    with pytest.raises(NotImplementedError, match="S=T"):
        obj.latent_sd()
