"""The multivariate (coregionalised) path without a GPU: LMCCovariance, the refusals of the Python wrapper and of the C
entry points, the workspace sizes, and mv_host.h under AddressSanitizer + UBSan in a stand-alone program
(tests/host/mv_check.cpp; never loaded into Python)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL, EUNSUP = -1, -4


@pytest.fixture(scope="module")
def lib():
    from pynngp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build()")
    return _lib.load()


def test_lmc_covariance():
    from pynngp_amd import LMCCovariance

    A = [[1.0, 0.0], [0.5, 0.8]]
    c = LMCCovariance("exponential", A, [2.0, 3.0], [0.1, 0.2])
    assert c.q == 2 and c.theta == (1.0, 0.5, 0.8, 2.0, 3.0, 0.1, 0.2)
    assert c.replace(phi=(4.0, 5.0)).phi == (4.0, 5.0)
    # two points at distance 0.5, by hand: K(d) = sum_k a_k a_k^T exp(-phi_k d)
    a0, a1 = np.array([1.0, 0.5]), np.array([0.0, 0.8])
    K = lambda d: np.outer(a0, a0) * np.exp(-2.0 * d) + np.outer(a1, a1) * np.exp(-3.0 * d)
    want = np.block([[K(0.0), K(0.5)], [K(0.5), K(0.0)]])
    np.testing.assert_allclose(c(np.array([[0.0, 0.0], [0.3, 0.4]]), np.array([[0.0, 0.0], [0.3, 0.4]])), want, rtol=1e-15)
    for bad in (dict(A=[[1.0, 0.1], [0.5, 0.8]]), dict(A=[[1.0, 0.0], [0.5, 0.0]]), dict(phi=[2.0, 0.0]),
                dict(phi=[2.0, float("nan")]), dict(tau2=[0.1, -0.2]), dict(tau2=[0.1])):
        with pytest.raises(ValueError):
            c.replace(**bad)
    for kind in ("spherical", "matern"):
        with pytest.raises(NotImplementedError):
            c.replace(kind=kind)
    with pytest.raises(NotImplementedError):
        LMCCovariance("exponential", np.eye(5), [1.0] * 5, [0.0] * 5)


def test_wrapper_refuses_before_any_gpu_work():
    import torch

    from pynngp_amd import _lib

    co = torch.zeros((4, 2), dtype=torch.float64)
    A2, A5 = np.eye(2), np.eye(5)

    def call(m=3, kind="exponential", A=A2, phi=(1.0, 1.0), tau2=(0.0, 0.0)):
        return _lib.bf_sweep_mv(co, torch.zeros((4, m), dtype=torch.int32), 0, kind, A, phi, tau2)

    for kw in (dict(A=A5, phi=[1.0] * 5, tau2=[0.0] * 5), dict(m=32), dict(m=0), dict(kind="spherical"), dict(kind="matern")):
        with pytest.raises(NotImplementedError):
            call(**kw)
    for kw in (dict(A=[[1.0, 0.2], [0.0, 1.0]]), dict(A=[[1.0, 0.0], [0.0, -1.0]]), dict(phi=(1.0, -1.0)),
               dict(tau2=(0.0, -1.0)), dict(phi=(1.0,)), dict(kind="cubic")):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(_lib.NNGPExtensionError):  # a valid model on CPU tensors: there is no CPU fallback
        call()


def _call(lib, which, m=3, q=2, kind=0, A=None, phi=None, tau2=None, c=1):
    """One call that must stop at the argument checks (host pointers: nothing may be launched)."""
    raw = ctypes.create_string_buffer(4096 + 256)
    w = ctypes.c_void_p((ctypes.addressof(raw) + 255) & ~255)
    co = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)
    nb = ctypes.cast((ctypes.c_int32 * 64)(*([-1] * 64)), ctypes.c_void_p)
    p = ctypes.cast((ctypes.c_double * 4)(), ctypes.c_void_p)
    Aa = (ctypes.c_double * 25)(*(np.eye(max(q, 1)).ravel() if A is None else A))
    ph = (ctypes.c_double * 5)(*([1.0] * 5 if phi is None else phi))
    t2 = (ctypes.c_double * 5)(*([0.0] * 5 if tau2 is None else tau2))
    if which == "sweep":
        return lib.nngp_bf_sweep_mv(co, 2, 2, nb, None, 1, 0, m, q, kind, Aa, ph, t2, None, c, None, None, None, p, w,
                                    4096, None)
    return lib.nngp_bf_cross_mv(co, 2, 2, co, 2, nb, None, 1, 0, m, q, kind, Aa, ph, t2, 1, None, c, None, None, None, p,
                                w, 4096, None)


@pytest.mark.parametrize("which", ["sweep", "cross"])
def test_entry_points_refuse(lib, which):
    for kw in (dict(q=5), dict(q=1), dict(q=2, m=32), dict(q=3, m=21), dict(q=4, m=16), dict(m=0), dict(kind=4),
               dict(kind=5)):
        assert _call(lib, which, **kw) == EUNSUP, kw
    assert b"kinds" in lib.nngp_last_error()
    for kw in (dict(A=[1.0, 0.3, 0.0, 1.0]), dict(A=[1.0, 0.0, 0.5, 0.0]), dict(A=[1.0, 0.0, float("nan"), 1.0]),
               dict(phi=[1.0, 0.0]), dict(phi=[float("inf"), 1.0]), dict(tau2=[0.0, -0.1]), dict(c=0), dict(c=9),
               dict(kind=8)):
        assert _call(lib, which, **kw) == EINVAL, kw
    assert lib.nngp_abi_version() == 4


def test_workspace_sizes(lib):
    for m, q in ((31, 2), (20, 3), (15, 4), (1, 2)):
        assert lib.nngp_bf_sweep_mv_workspace_bytes(0, m, q) == 256
        assert lib.nngp_bf_sweep_mv_workspace_bytes(1000, m, q) == 250 * 32 + 192
    for m, q in ((32, 2), (21, 3), (16, 4), (3, 5), (3, 1), (0, 2)):
        assert lib.nngp_bf_sweep_mv_workspace_bytes(1000, m, q) == 0


def test_host_checks_under_sanitizers(tmp_path, lib):
    """mv_host.h (workspace size and argument checks) in a stand-alone program built with
    -fsanitize=address,undefined; the size it prints is the library's."""
    exe = tmp_path / "mv_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "pynngp_amd", "csrc"), os.path.join(HERE, "host", "mv_check.cpp"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out[0] == "ok" and int(out[1]) == lib.nngp_bf_sweep_mv_workspace_bytes(1001, 15, 4)
