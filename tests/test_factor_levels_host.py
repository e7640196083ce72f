"""CPU: the level schedule of the NNGP factor's triangular solves (nngp_factor_levels) -- its defining
properties on random 2-D sets, a sorted 1-D series and a reference-set layout, the edge cases, the argument
refusals, and the level builder under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program
(tests/host/factor_levels_check.cpp; host code only, never loaded into Python)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))


def knn_prior_host(coords, m):
    """Prior neighbour sets by brute force: row i holds its min(i, m) nearest among coords[:i], -1 padded."""
    n = coords.shape[0]
    nbr = np.full((n, m), -1, dtype=np.int32)
    for i in range(1, n):
        d = ((coords[:i] - coords[i]) ** 2).sum(axis=1)
        k = min(i, m)
        nbr[i, :k] = np.argsort(d, kind="stable")[:k]
    return nbr


def ref_layout(rng, n_s, n_leaves, m):
    """Nodes 0 .. n_s - 1: prior sets among themselves; leaves n_s ..: their m nearest reference points."""
    s, t = rng.uniform(size=(n_s, 2)), rng.uniform(size=(n_leaves, 2))
    nbr_s = knn_prior_host(s, m)
    d = ((t[:, None, :] - s[None, :, :]) ** 2).sum(axis=2)
    nbr_t = np.argsort(d, axis=1, kind="stable")[:, :m].astype(np.int32)
    return np.concatenate([nbr_s, nbr_t])


def _cases():
    rng = np.random.default_rng(7)
    pts = rng.uniform(size=(500, 2))
    out = {f"random2d_m{m}": knn_prior_host(pts, m) for m in (1, 5, 32)}
    out["sorted1d"] = knn_prior_host(np.sort(rng.uniform(size=300))[:, None], 3)
    out["ref"] = ref_layout(rng, 100, 200, 5)
    return out


CASES = _cases()


def levels(nbr, trans):
    from pynngp_amd import _lib

    return _lib.factor_levels(nbr, trans)


def valid(nbr):
    """The valid slots: 0 <= nbr[i, k] < i."""
    return (nbr >= 0) & (nbr < np.arange(nbr.shape[0])[:, None])


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_schedule(name):
    nbr = CASES[name]
    n = nbr.shape[0]
    level, rows, off = levels(nbr, False)
    ok = valid(nbr)
    nl = np.where(ok, level[np.where(ok, nbr, 0)], -1)  # neighbours' levels, -1 where absent
    assert np.all(nl < level[:, None]), "a valid neighbour must have a strictly smaller level"
    assert np.array_equal(level, nl.max(axis=1) + 1), "tight: some neighbour sits exactly one level below (or 0)"
    _check_rows(level, rows, off, n)


@pytest.mark.parametrize("name", sorted(CASES))
def test_transposed_schedule(name):
    nbr = CASES[name]
    n = nbr.shape[0]
    level, rows, off = levels(nbr, True)
    ok = valid(nbr)
    i_idx, k_idx = np.nonzero(ok)
    j_idx = nbr[i_idx, k_idx]
    assert np.all(level[i_idx] < level[j_idx]), "every row listing j must have a strictly smaller level than j"
    want = np.zeros(n, dtype=np.int64)
    np.maximum.at(want, j_idx, level[i_idx] + 1)
    assert np.array_equal(level, want), "tight: some listing row sits exactly one level below (or no row lists j)"
    _check_rows(level, rows, off, n)


def _check_rows(level, rows, off, n):
    depth = off.shape[0] - 1
    assert off[0] == 0 and off[-1] == n and np.all(np.diff(off) > 0)
    assert np.array_equal(np.sort(rows), np.arange(n)), "rows is a permutation"
    assert depth == level.max() + 1
    key = level[rows].astype(np.int64) * n + rows
    assert np.all(np.diff(key) > 0), "rows sorted by (level, index)"
    assert np.array_equal(np.repeat(np.arange(depth), np.diff(off)), level[rows])


def test_series_is_a_chain():
    nbr = CASES["sorted1d"]
    n = nbr.shape[0]
    for trans in (False, True):
        level, rows, off = levels(nbr, trans)
        assert off.shape[0] - 1 == n, "a sorted 1-D series has depth n"
        assert np.array_equal(rows, np.arange(n)[::-1] if trans else np.arange(n))


def test_leaves_follow_their_parents():
    nbr, n_s = CASES["ref"], 100
    level, _, _ = levels(nbr, False)
    parents = level[nbr[n_s:]]  # every leaf slot is valid (m <= n_s)
    assert np.array_equal(level[n_s:], parents.max(axis=1) + 1)
    level_t, _, _ = levels(nbr, True)
    assert np.all(level_t[n_s:] == 0), "nothing lists a leaf: the transposed solve starts with all of them"


def test_edge_cases():
    level, rows, off = levels(np.empty((0, 4), dtype=np.int32), False)
    assert level.shape == (0,) and rows.shape == (0,) and off.tolist() == [0]
    for trans in (False, True):
        level, rows, off = levels(np.array([[-1, -1]], dtype=np.int32), trans)
        assert level.tolist() == [0] and rows.tolist() == [0] and off.tolist() == [0, 1]
        level, rows, off = levels(np.full((6, 3), -1, dtype=np.int32), trans)
        assert level.tolist() == [0] * 6 and rows.tolist() == list(range(6)) and off.tolist() == [0, 6]
    # slots >= the row index count as absent: row 1 names itself and a later row, row 2 names row 1 and row 3
    nbr = np.array([[-1, -1], [1, 3], [1, 3], [2, -7]], dtype=np.int32)
    level, rows, off = levels(nbr, False)
    assert level.tolist() == [0, 0, 1, 2] and rows.tolist() == [0, 1, 2, 3] and off.tolist() == [0, 2, 3, 4]
    level, rows, off = levels(nbr, True)
    assert level.tolist() == [0, 2, 1, 0] and rows.tolist() == [0, 3, 2, 1] and off.tolist() == [0, 2, 3, 4]


def test_refusals():
    from pynngp_amd import _lib

    lib = _lib.load()
    nbr = np.zeros((4, 2), dtype=np.int32)
    level, rows, off = (np.zeros(8, dtype=np.int32) for _ in range(3))
    depth = ctypes.c_int64(-5)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for n, m, trans, word in ((4, 2, 2, "trans"), (4, 2, -1, "trans"), (4, 0, 0, "m="), (4, _lib.MAX_M + 1, 0, "m="),
                              (-1, 2, 0, "n=")):
        rc = lib.nngp_factor_levels(p(nbr), n, m, trans, p(level), p(rows), p(off), ctypes.byref(depth))
        assert rc == -1, (n, m, trans, rc)  # NNGP_EINVAL
        assert word in lib.nngp_last_error().decode(), lib.nngp_last_error()
    assert depth.value == -5, "a refused call writes nothing"


def test_launch_counts():
    from pynngp_amd import _lib

    sched_off = np.array([0, 1, 2, 3, 103, 104, 204, 205], dtype=np.int32)  # widths 1 1 1 100 1 100 1
    wide, runs = ctypes.c_int64(), ctypes.c_int64()
    lib = _lib.load()
    for fuse, want in ((0, (7, 0)), (1, (2, 3)), (99, (2, 3)), (100, (0, 1))):
        assert lib.nngp_factor_launch_counts(sched_off.ctypes.data_as(ctypes.c_void_p), 7, fuse, ctypes.byref(wide),
                                             ctypes.byref(runs)) == 0
        assert (wide.value, runs.value) == want, fuse
    assert lib.nngp_factor_launch_counts(sched_off.ctypes.data_as(ctypes.c_void_p), 7,
                                         _lib.FACTOR_MAX_FUSE_WIDTH + 1, ctypes.byref(wide), ctypes.byref(runs)) == -1


def test_level_builder_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "factor_levels_check")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-g", "-O1", os.path.join(HERE, "host", "factor_levels_check.cpp"),
                    "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    assert os.path.exists(os.path.join(ROOT, "pynngp_amd", "csrc", "factor_levels.h"))
