"""Gradient sweep C entry points (nngp_bf_grad*): argument refusals before any HIP call (no GPU needed)."""
import ctypes

import pytest

from pynngp_amd import _lib

@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _codes():
    # the header's error codes, read from include/nngp.h so the test does not pin their values itself
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nngp.h")).read()
    out = {}
    for name in ("NNGP_OK", "NNGP_EINVAL", "NNGP_EUNSUP"):
        m = re.search(r"#define\s+" + name + r"\s+\(?(-?\d+)", hdr)
        assert m, name
        out[name] = int(m.group(1))
    return out


def _call(lib, *, coords=256, n_points=100, dim=2, nbr=512, order=None, n_rows=100, m=10, i0=0, kind=0,
          theta=(1.0, 6.0, 0.1), values=768, G=None, partials=1024, grad=1280, workspace=4096, ws_bytes=None):
    # fake (never dereferenced) device addresses: every refusal below happens before any HIP call
    if ws_bytes is None:
        ws_bytes = lib.nngp_bf_grad_workspace_bytes(n_rows, m) or 4096
    return lib.nngp_bf_grad(coords, n_points, dim, nbr, order, n_rows, m, i0, kind, *theta, values, G, partials, grad,
                            workspace, ws_bytes, None)


def test_workspace_bytes_monotone_and_refusals(lib):
    prev = 0
    for n in (0, 1, 63, 64, 65, 1000, 10**6, 10**7):
        for m in (1, 8, 9, 32):
            assert lib.nngp_bf_grad_workspace_bytes(n, m) % 256 == 0
        b = lib.nngp_bf_grad_workspace_bytes(n, 15)
        assert b >= prev and b > 0
        prev = b
    assert lib.nngp_bf_grad_workspace_bytes(100, 0) == 0
    assert lib.nngp_bf_grad_workspace_bytes(100, 33) == 0
    assert lib.nngp_bf_grad_workspace_bytes(-1, 10) == 0


def test_unsupported(lib):
    c = _codes()
    assert _call(lib, kind=5) == c["NNGP_EUNSUP"]
    assert b"matern" in lib.nngp_last_error()
    assert _call(lib, m=0, ws_bytes=4096) == c["NNGP_EUNSUP"]
    assert _call(lib, m=33, ws_bytes=4096) == c["NNGP_EUNSUP"]
    assert _call(lib, dim=4) == c["NNGP_EUNSUP"]


@pytest.mark.parametrize("kw", [
    dict(values=None), dict(partials=None), dict(grad=None), dict(coords=None), dict(workspace=None), dict(nbr=None),
    dict(ws_bytes=255), dict(workspace=4097), dict(kind=-1), dict(kind=6), dict(n_rows=-1, ws_bytes=4096),
    dict(i0=-1), dict(i0=1), dict(n_points=0), dict(theta=(0.0, 6.0, 0.1)), dict(theta=(1.0, -1.0, 0.1)),
    dict(theta=(1.0, 6.0, -0.1)), dict(theta=(float("nan"), 6.0, 0.1)), dict(theta=(1.0, float("inf"), 0.1)),
])
def test_invalid(lib, kw):
    assert _call(lib, **kw) == _codes()["NNGP_EINVAL"], lib.nngp_last_error()


def test_python_refusals():
    import torch

    c = torch.zeros((4, 2), dtype=torch.float64)
    nbr = torch.zeros((4, 2), dtype=torch.int32)
    with pytest.raises(ValueError):
        _lib.bf_grad(c, nbr, 0, "exponential", 1.0, 1.0, 0.1, None)
