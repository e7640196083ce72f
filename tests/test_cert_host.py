"""CPU: the neighbour-set certificate's C ABI (include/nngp.h nngp_nbr_cert_*, nngp_bf_sweep_cert).

Argument checks come before any device call, so they run without a GPU (fake, never dereferenced
pointers); the theta-dependent decision nngp_nbr_cert_trusted_tiles is a pure host function; the
bitmask / span / decision logic (pynngp_amd/csrc/nbr_cert.h) also runs as a stand-alone program under
AddressSanitizer and UBSan (tests/host/nbr_cert_check.cpp).
"""
import ctypes
import os
import struct
import subprocess

import pytest

from pynngp_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL = -1
MAGIC = 0x4E42524345525431  # nbr_cert.h kCertMagic
PTR = 1 << 20  # a non-null, 256-B aligned address that is never dereferenced


def _info(coords=PTR, nbr=2 * PTR, order=0, n_points=300, dim=2, n_rows=300, m=15, i0=0, tiles=3, checked=1,
          span=2.0, magic=MAGIC):
    span_bits = struct.unpack("<q", struct.pack("<d", span))[0]
    words = [magic, coords, nbr, order, n_points, dim, n_rows, m, i0, tiles, checked, span_bits, 0, 0, 0, 0]
    assert len(words) == _lib.CERT_INFO_LEN
    return (ctypes.c_int64 * _lib.CERT_INFO_LEN)(*words)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_info_len_matches_header():
    import re

    src = open(os.path.join(HERE, "..", "include", "nngp.h")).read()
    assert int(re.search(r"#define\s+NNGP_CERT_INFO_LEN\s+(\d+)", src).group(1)) == _lib.CERT_INFO_LEN


def test_cert_bytes(lib):
    assert lib.nngp_nbr_cert_bytes(-1) == 0
    b = lib.nngp_nbr_cert_bytes(300)
    assert b > 256 and b % 256 == 0
    big = lib.nngp_nbr_cert_bytes(10 ** 6)  # 7,813 tiles: one bit each after the 256-B header
    assert big > b and big % 256 == 0 and big >= 256 + 4 * -(-7813 // 32)


def test_cert_build_rejects_bad_arguments(lib):
    info = (ctypes.c_int64 * _lib.CERT_INFO_LEN)()
    nb = lib.nngp_nbr_cert_bytes(300)

    def build(coords=PTR, n_points=300, dim=2, nbr=2 * PTR, n_rows=300, m=15, i0=0, cert=3 * PTR, cert_bytes=nb,
              info=info):
        return lib.nngp_nbr_cert_build(coords, n_points, dim, nbr, None, n_rows, m, i0, cert, cert_bytes, info, None)

    assert build(coords=None) == EINVAL
    assert build(nbr=None) == EINVAL
    assert build(cert=None) == EINVAL
    assert build(info=None) == EINVAL
    assert build(cert_bytes=nb - 1) == EINVAL and b"too small" in lib.nngp_last_error()
    assert build(cert=3 * PTR + 8) == EINVAL
    assert build(n_rows=301) == EINVAL  # rows past the points
    assert build(i0=1) == EINVAL
    assert build(dim=4) != 0 and build(m=0) != 0 and build(m=64) != 0


def test_sweep_cert_rejects_null_and_mismatched_info(lib):
    nb = lib.nngp_nbr_cert_bytes(300)

    def sweep(info, coords=PTR, n_points=300, dim=2, nbr=2 * PTR, order=None, n_rows=300, m=15, i0=0, cert=3 * PTR,
              cert_bytes=nb):
        return lib.nngp_bf_sweep_cert(coords, n_points, dim, nbr, order, n_rows, m, i0, 0, 1.0, 30.0, 0.0, -1.0, None,
                                      None, None, None, 4 * PTR, 5 * PTR, 1 << 20, 0, cert, cert_bytes, info, None)

    good = _info()
    assert sweep(None) == EINVAL
    assert sweep(good, cert=None) == EINVAL
    assert sweep(_info(magic=MAGIC + 1)) == EINVAL
    assert sweep(good, coords=PTR + 256) == EINVAL and b"other coords" in lib.nngp_last_error()
    assert sweep(good, nbr=2 * PTR + 256) == EINVAL
    assert sweep(good, order=6 * PTR) == EINVAL
    assert sweep(good, n_points=301) == EINVAL
    assert sweep(good, dim=3) == EINVAL
    assert sweep(_info(n_rows=200), n_rows=300) == EINVAL
    assert sweep(good, m=14) == EINVAL
    assert sweep(_info(i0=0, n_rows=200), n_rows=200, i0=100) == EINVAL
    assert sweep(good, cert_bytes=nb - 1) == EINVAL and b"too small" in lib.nngp_last_error()
    assert sweep(_info(tiles=4)) == EINVAL


def test_trusted_tiles_decision(lib):
    tt = lib.nngp_nbr_cert_trusted_tiles
    unit = _info(span=2.0)  # the unit square: three tiles, one of them checked
    assert tt(unit, 0, 1.0, 30.0, 0.0) == 2
    assert tt(unit, 0, 1.0, 1000.0, 0.0) == 0  # phi diag log2(e) ~ 2040 > 1023: the clamp may bind
    for kind in (1, 2):
        assert tt(unit, kind, 1.0, 30.0, 0.0) == 2 and tt(unit, kind, 1.0, 1000.0, 0.0) == 0
    assert tt(unit, 3, 1.0, 10.0, 0.0) == 2 and tt(unit, 3, 1.0, 30.0, 0.0) == 0  # gaussian clamps d2 itself
    assert tt(unit, 4, 1.0, 1000.0, 0.0) == 2  # spherical: no clamp
    for kind in (-1, 5, 6, 99):
        assert tt(unit, kind, 1.0, 30.0, 0.0) == 0
    assert tt(None, 0, 1.0, 30.0, 0.0) == 0
    assert tt(_info(magic=0), 0, 1.0, 30.0, 0.0) == 0
    assert tt(_info(checked=3), 0, 1.0, 30.0, 0.0) == 0
    assert tt(_info(m=25), 0, 1.0, 30.0, 0.0) == 0
    assert tt(_info(span=float("nan")), 0, 1.0, 30.0, 0.0) == 0
    assert tt(unit, 0, 0.0, 30.0, 0.0) == 0 and tt(unit, 0, 1.0, 0.0, 0.0) == 0 and tt(unit, 0, 1.0, 30.0, -1.0) == 0


def test_host_logic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "nbr_cert_check")
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "host", "nbr_cert_check.cpp"), "-o", exe, "-lm"],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
