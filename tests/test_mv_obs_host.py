"""The packed-row multivariate path without a GPU: the refusals of the C entry points, the workspace sizes, and
mv_obs_host.h under AddressSanitizer + UBSan in a stand-alone program (tests/host/mv_obs_check.cpp; never loaded into
Python)."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT
from test_mv_host import lib  # noqa: F401  (the fixture: the built library, loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL, EUNSUP = -1, -4


def _call(lib, which, m=3, q=2, kind=0, rows_max=6, obs=True, tau2=0.0):
    """One call that must stop at the argument checks (host pointers: nothing may be launched)."""
    raw = ctypes.create_string_buffer(4096 + 256)
    w = ctypes.c_void_p((ctypes.addressof(raw) + 255) & ~255)
    co = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)
    nb = ctypes.cast((ctypes.c_int32 * 64)(*([-1] * 64)), ctypes.c_void_p)
    p = ctypes.cast((ctypes.c_double * 4)(), ctypes.c_void_p)
    ob = ctypes.cast((ctypes.c_uint8 * 8)(), ctypes.c_void_p) if obs else None
    Aa = (ctypes.c_double * 25)(*[float(i // max(q, 1) == i % max(q, 1)) for i in range(25)])
    ph, t2 = (ctypes.c_double * 5)(*([1.0] * 5)), (ctypes.c_double * 5)(*([tau2] * 5))
    if which == "sweep":
        return lib.nngp_bf_sweep_mv_obs(co, 2, 2, nb, None, 1, 0, m, q, kind, Aa, ph, t2, None, 1, ob, rows_max, None,
                                        None, None, p, w, 4096, None)
    return lib.nngp_bf_cross_mv_obs(co, 2, 2, co, 2, nb, None, 1, 0, m, q, kind, Aa, ph, t2, 1, None, 1, ob, rows_max,
                                    None, None, None, p, w, 4096, None)


@pytest.mark.parametrize("which", ["sweep", "cross"])
def test_entry_points_refuse(lib, which):
    for kw in (dict(q=5), dict(q=1), dict(m=64), dict(m=0), dict(rows_max=0), dict(rows_max=65), dict(kind=4),
               dict(kind=5)):
        assert _call(lib, which, **kw) == EUNSUP, kw
    for kw in (dict(obs=False), dict(tau2=-0.1), dict(kind=8)):
        assert _call(lib, which, **kw) == EINVAL, kw
    assert lib.nngp_bf_sweep_mv_obs_workspace_bytes(1000, 63, 2) == 32000  # a record per location
    assert lib.nngp_bf_sweep_mv_obs_workspace_bytes(1000, 64, 2) == 0


def test_host_checks_under_sanitizers(tmp_path, lib):
    exe = tmp_path / "mv_obs_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "pynngp_amd", "csrc"), os.path.join(HERE, "host", "mv_obs_check.cpp"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out[0] == "ok" and int(out[1]) == lib.nngp_bf_sweep_mv_obs_workspace_bytes(1001, 50, 2)
